// Training-mode pieces of the path: one convolution layer of the encoder /
// Postnet stacks as the reference runs it in .train() mode - conv1d + BatchNorm1d with BATCH statistics + activation +
// dropout (models/tts/tacotron2.py:149-199, :207-220, :234-235) - forward and backward, and the backward of the criterion
// (Tacotron2Loss, :598-615).  Weights come in the reference's own parameter layout (training updates them in place: there
// is no packed blob on this side); activations cross the C ABI in the reference's [B, C, T] layout.
//
// Every contraction runs on the exact-fp32 MFMA GEMM of the forward path (gemm_f32.hip):
//   forward  z[(b,t)][co]  = sum_{j,ci} xcl[b][t + j][ci] * Wk[co][j][ci] + bias        implicit GEMM on the halo-padded input
//   dgrad    dx[(b,t)][ci] = sum_{j,co} dzh[b][t + j][co] * W2[ci][j][co],  W2[ci][j][co] = W[co][ci][k-1-j]   the same, flipped taps
//   wgrad    dW[co][(j,ci)] = sum_r dz^T[co][r] * X^T[(j,ci)][r]                        both operands transposed to row-contiguous
// BatchNorm statistics and the reductions of its backward are column sums in double precision; everything else is
// elementwise.
#include "train_internal.h"

namespace gvx {
namespace {

constexpr float BN_EPS_F = 1e-5f;
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// [Cout][Cin][k] -> Wk[Cout][k][Cin] (forward)  and  W2[Cin][k][Cout] with flipped taps (dgrad)
__global__ void repack_conv_kernel(const float* w, float* wk, float* w2, int Cout, int Cin, int k) {
    const long n = (long)Cout * Cin * k;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % k), ci = (int)((i / k) % Cin), co = (int)(i / ((long)k * Cin));
        const float v = w[i];
        if (wk) wk[((long)co * k + j) * Cin + ci] = v;
        if (w2) w2[((long)ci * k + (k - 1 - j)) * Cout + co] = v;
    }
}

// biased batch variance in double from the centred values (two passes keep it exact enough for invstd); also the running
// statistics update of torch.nn.BatchNorm1d (momentum 0.1, unbiased variance).  Same 32 x 32 walk as col_reduce_kernel.
__global__ __launch_bounds__(1024) void bn_stats_kernel(const float* Z, long rows, int C, float* mean, float* invstd, float* running_mean,
                                                        float* running_var, float momentum) {
    __shared__ double s1[CR_LANES][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (c < C) {
        long r = rl;
        for (; r + 3 * CR_LANES < rows; r += 4 * CR_LANES) {
            a0 += (double)Z[r * C + c]; a1 += (double)Z[(r + CR_LANES) * C + c];
            a2 += (double)Z[(r + 2 * CR_LANES) * C + c]; a3 += (double)Z[(r + 3 * CR_LANES) * C + c];
        }
        for (; r < rows; r += CR_LANES) a0 += (double)Z[r * C + c];
    }
    s1[rl][cl] = (a0 + a1) + (a2 + a3);
    __syncthreads();
    double m = 0.0;
    for (int i = 0; i < CR_LANES; ++i) m += s1[i][cl];
    m /= (double)rows;
    __syncthreads();
    double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
    if (c < C) {
        long r = rl;
        for (; r + 3 * CR_LANES < rows; r += 4 * CR_LANES) {
            const double d0 = (double)Z[r * C + c] - m, d1 = (double)Z[(r + CR_LANES) * C + c] - m;
            const double d2 = (double)Z[(r + 2 * CR_LANES) * C + c] - m, d3 = (double)Z[(r + 3 * CR_LANES) * C + c] - m;
            v0 += d0 * d0; v1 += d1 * d1; v2 += d2 * d2; v3 += d3 * d3;
        }
        for (; r < rows; r += CR_LANES) { const double d = (double)Z[r * C + c] - m; v0 += d * d; }
    }
    s1[rl][cl] = (v0 + v1) + (v2 + v3);
    __syncthreads();
    if (rl == 0 && c < C) {
        double var = 0.0;
        for (int i = 0; i < CR_LANES; ++i) var += s1[i][cl];
        var /= (double)rows;
        mean[c] = (float)m;
        invstd[c] = (float)(1.0 / sqrt(var + (double)BN_EPS_F));
        if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)m;
        if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)(var * (double)rows / (double)(rows > 1 ? rows - 1 : 1));
    }
}

__device__ __forceinline__ float act_fwd(float u, int act) { return act == ACT_TANH ? tanhf(u) : (act == ACT_RELU ? fmaxf(u, 0.f) : u); }

// z [(b,t)][c] -> xhat, a (channels-last, saved) and y[b][c][t] = a * keep / (1 - p)
__global__ void bn_act_drop_fwd_kernel(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta,
                                       const uint8_t* keep, float scale, int act, int B, int C, int T, float* xhat, float* a, float* y) {
    const long n = (long)B * T * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long bt = i / C;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const float xh = (z[i] - mean[c]) * invstd[c];
        const float av = act_fwd(xh * gamma[c] + beta[c], act);
        xhat[i] = xh; a[i] = av;
        const long o = ((long)b * C + c) * T + t;
        y[o] = keep ? (keep[o] ? av * scale : 0.f) : av;
    }
}

// du[(b,t)][c] = dy[b][c][t] * keep / (1 - p) * act'(a)
__global__ void act_drop_bwd_kernel(const float* dy, const uint8_t* keep, float scale, int act, const float* a, int B, int C, int T, float* du) {
    const long n = (long)B * T * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long bt = i / C;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const long o = ((long)b * C + c) * T + t;
        float g = dy[o];
        if (keep) g = keep[o] ? g * scale : 0.f;
        const float av = a[i];
        if (act == ACT_TANH) g *= 1.f - av * av;
        else if (act == ACT_RELU) g = av > 0.f ? g : 0.f;
        du[i] = g;
    }
}

// dz = gamma * invstd * (du - dbeta / n - xhat * dgamma / n), written compact [(b,t)][c] and halo-padded [b][t + pad][c]
__global__ void bn_bwd_kernel(const float* du, const float* xhat, const float* gamma, const float* invstd, const float* dbeta,
                              const float* dgamma, int B, int C, int T, int pad, float* dz, float* dzh) {
    const long n = (long)B * T * C;
    const float inv_n = 1.f / (float)((long)B * T);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long bt = i / C;
        const int t = (int)(bt % T), b = (int)(bt / T);
        const float v = gamma[c] * invstd[c] * (du[i] - dbeta[c] * inv_n - xhat[i] * dgamma[c] * inv_n);
        dz[i] = v;
        dzh[((long)b * (T + 2 * pad) + pad + t) * C + c] = v;
    }
}

// dwk [Cout][k][Cin] -> dw [Cout][Cin][k]
__global__ void unpack_dw_kernel(const float* dwk, float* dw, int Cout, int Cin, int k) {
    const long n = (long)Cout * Cin * k;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int j = (int)(i % k), ci = (int)((i / k) % Cin), co = (int)(i / ((long)k * Cin));
        dw[i] = dwk[((long)co * k + j) * Cin + ci];
    }
}
// x [(b,t)][c] -> y [b][c][t]
__global__ void to_channels_first_kernel(const float* x, float* y, int B, int C, int T) {
    const long n = (long)B * T * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long bt = i / C;
        const int t = (int)(bt % T), b = (int)(bt / T);
        y[((long)b * C + c) * T + t] = x[i];
    }
}

__global__ void loss_backward_kernel(const float* mel, const float* post, const float* gate, const float* mel_t, const float* gate_t,
                                     long n_mel, long n_gate, float* dmel, float* dpost, float* dgate) {
    const float cm = 2.f / (float)n_mel, cg = 1.f / (float)n_gate;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_mel; i += (long)gridDim.x * blockDim.x) {
        dmel[i] = cm * (mel[i] - mel_t[i]);
        dpost[i] = cm * (post[i] - mel_t[i]);
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_gate; i += (long)gridDim.x * blockDim.x)
        dgate[i] = cg * (1.f / (1.f + expf(-gate[i])) - gate_t[i]);
}


// layout of the saved-for-backward buffer and of the scratch of one layer (byte offsets)
struct ConvTrainPlan {
    size_t xcl, xhat, a, mean, invstd, saved_total;                       // saved
    size_t wk, w2, z, du, dz, dzh, dwk, dxcl, xcl2, dwk_part, ws_total;   // workspace
};
ConvTrainPlan conv_train_plan(int B, int Cin, int Cout, int T, int k) {
    const int pad = (k - 1) / 2;
    const long rows = (long)B * T;
    ConvTrainPlan p{};
    size_t o = 0;
    auto take = [&](size_t floats) { size_t r = o; o = up256(o + floats * sizeof(float)); return r; };
    p.xcl = take((size_t)B * (T + 2 * pad) * Cin);
    p.xhat = take((size_t)rows * Cout);
    p.a = take((size_t)rows * Cout);
    p.mean = take(Cout);
    p.invstd = take(Cout);
    p.saved_total = o;
    o = 0;
    p.wk = take((size_t)Cout * k * Cin);
    p.w2 = take((size_t)Cin * k * Cout);
    p.z = take((size_t)rows * Cout);
    p.du = take((size_t)rows * Cout);
    p.dz = take((size_t)rows * Cout);
    p.dzh = take((size_t)B * (T + 2 * pad) * Cout);
    p.dwk = take((size_t)Cout * k * Cin);
    p.dxcl = take((size_t)rows * Cin);
    p.xcl2 = take((size_t)B * (T + 2 * pad) * Cin);
    p.dwk_part = take((size_t)8 * Cout * k * Cin);   // split-K partial tiles of the weight gradient (at most 8 splits)
    p.ws_total = o;
    return p;
}

template <typename T>
T* at(void* base, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + off); }
template <typename T>
const T* at(const void* base, size_t off) { return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + off); }

// The three products of one layer as launch_gemm / launch_gemm_splitk get them, buffers left open: the two entry points fill in the
// pointers and launch exactly these, and gvx_debug_conv_train_plan reports what plan_gemm / choose_splitk / set_splitk make of them
// (tests/test_host_cpu.py pins which layer shape takes which tile and how its weight gradient is cut).
// forward: z[(b, t)][co] = sum_{j, ci} xcl[b][t + j][ci] * wk[co][j][ci] + bias - implicit GEMM on the halo-padded input
GemmParams conv_forward_gemm(int B, int Cin, int Cout, int T, int k) {
    const int pad = (k - 1) / 2;
    const long rows = (long)B * T;
    GemmParams g{};
    g.amap = RowMap{T, (long)(T + 2 * pad) * Cin, (long)Cin};
    g.ldw = (long)k * Cin;
    g.cmap = RowMap{(int)rows, 0, (long)Cout};
    g.M = (int)rows; g.N = Cout; g.K = k * Cin; g.act = ACT_NONE;
    return g;
}
// weight gradient: dwk[co][(j, ci)] = sum over the rows r = (b, t) of dz[r][co] * xcl[b][t + j][ci]: both operands K-major as they
// lie in memory (the im2col row of r is the k * Cin contiguous floats at padded row t) - no transposed copies
GemmParams conv_wgrad_gemm(int B, int Cin, int Cout, int T, int k) {
    const int pad = (k - 1) / 2;
    const long rows = (long)B * T;
    GemmParams g{};
    g.kmajor = true;
    g.amap = RowMap{(int)rows, 0, (long)Cout};
    g.wmap = RowMap{T, (long)(T + 2 * pad) * Cin, (long)Cin};
    g.cmap = RowMap{Cout, 0, (long)k * Cin};
    g.M = Cout; g.N = k * Cin; g.K = (int)rows; g.act = ACT_NONE;
    return g;
}
// few output tiles, thousands of rows to sum over: K split over enough workgroups to fill the chip (the Postnet's 512 x 2560
// gradients are 160 tiles, its first layer's 32: 290 / 330 us each as one round)
int conv_wgrad_splitk(int B, int Cin, int Cout, int T, int k) {
    const long tiles = (long)((Cout + 63) / 64) * ((k * Cin + 127) / 128);
    return choose_splitk(tiles, (int)((long)B * T));
}
// data gradient: flipped-tap implicit GEMM on the halo-padded dz
GemmParams conv_dgrad_gemm(int B, int Cin, int Cout, int T, int k) {
    const int pad = (k - 1) / 2;
    const long rows = (long)B * T;
    GemmParams g{};
    g.amap = RowMap{T, (long)(T + 2 * pad) * Cout, (long)Cout};
    g.ldw = (long)k * Cout;
    g.cmap = RowMap{(int)rows, 0, (long)Cin};
    g.M = (int)rows; g.N = Cin; g.K = k * Cout; g.act = ACT_NONE;
    return g;
}

int check_conv_args(int B, int Cin, int Cout, int T, int k) {
    if (B < 1 || T < 1 || Cin < 8 || Cout < 8 || (Cin % 8) || (Cout % 8) || k < 1 || !(k & 1))
        return tfail(GVX_ERR_UNSUPPORTED, "conv training op: channels must be positive multiples of 8, kernel size odd");
    if ((long)B * T > (1L << 30)) return tfail(GVX_ERR_UNSUPPORTED, "conv training op: B * T exceeds the GEMM row index range");
    return GVX_OK;
}

}  // namespace
}  // namespace gvx

using namespace gvx;

extern "C" {

// Host-only query for the tests (not part of the public header; touches no device): how one gvx_conv_bn_act_train_forward /
// _backward pair runs its three products, from the functions the two entry points launch through.  out[0 .. 7] = forward tile,
// forward rows_big, data-gradient tile, data-gradient rows_big, weight-gradient tile (K-major), weight-gradient rows_big, the K
// pieces of the weight gradient (1 = no split-K) and the length of a piece (0 without a split).  Tiles and rows_big as GemmPlan.
int gvx_debug_conv_train_plan(int B, int Cin, int Cout, int T, int k, int* out) {
    if (!out) return GVX_ERR_INVALID_ARG;
    const int rc = check_conv_args(B, Cin, Cout, T, k);
    if (rc != GVX_OK) return rc;
    GemmParams w = conv_wgrad_gemm(B, Cin, Cout, T, k);
    const int splitk = conv_wgrad_splitk(B, Cin, Cout, T, k);
    if (splitk > 1) set_splitk(w, splitk);   // (what launch_gemm_splitk does before it plans)
    const GemmPlan pf = plan_gemm(conv_forward_gemm(B, Cin, Cout, T, k)), pd = plan_gemm(conv_dgrad_gemm(B, Cin, Cout, T, k)), pw = plan_gemm(w);
    if (pf.err != hipSuccess || pd.err != hipSuccess || pw.err != hipSuccess) return GVX_ERR_INVALID_ARG;
    out[0] = pf.tile; out[1] = pf.rows_big; out[2] = pd.tile; out[3] = pd.rows_big;
    out[4] = pw.tile; out[5] = pw.rows_big; out[6] = w.splitk; out[7] = w.splitk > 1 ? w.kchunk : 0;
    return GVX_OK;
}

size_t gvx_conv_train_saved_bytes(int B, int Cin, int Cout, int T, int k) {
    if (check_conv_args(B, Cin, Cout, T, k) != GVX_OK) return 0;
    return conv_train_plan(B, Cin, Cout, T, k).saved_total;
}
size_t gvx_conv_train_workspace_bytes(int B, int Cin, int Cout, int T, int k) {
    if (check_conv_args(B, Cin, Cout, T, k) != GVX_OK) return 0;
    return conv_train_plan(B, Cin, Cout, T, k).ws_total;
}

int gvx_conv_bn_act_train_forward(const float* x, const float* w, const float* bias, const float* gamma, const float* beta,
                                  float* running_mean, float* running_var, int B, int Cin, int Cout, int T, int k, int act,
                                  const uint8_t* keep, float p_drop, float* y, void* saved, size_t saved_bytes, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    int rc = check_conv_args(B, Cin, Cout, T, k);
    if (rc != GVX_OK) return rc;
    if (!x || !w || !bias || !gamma || !beta || !y || !saved || !workspace) return tfail(GVX_ERR_INVALID_ARG, "null argument");
    if (act != ACT_NONE && act != ACT_RELU && act != ACT_TANH) return tfail(GVX_ERR_INVALID_ARG, "activation must be 0 (none), 1 (relu) or 2 (tanh)");
    if (keep && !(p_drop >= 0.f && p_drop < 1.f)) return tfail(GVX_ERR_INVALID_ARG, "dropout probability must be in [0, 1)");
    const ConvTrainPlan pl = conv_train_plan(B, Cin, Cout, T, k);
    if (saved_bytes < pl.saved_total || workspace_bytes < pl.ws_total) return tfail(GVX_ERR_WORKSPACE, "saved / workspace buffer too small");
    if ((reinterpret_cast<uintptr_t>(saved) | reinterpret_cast<uintptr_t>(workspace)) & 255) return tfail(GVX_ERR_WORKSPACE, "buffers must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int pad = (k - 1) / 2;
    const long rows = (long)B * T;
    float* xcl = at<float>(saved, pl.xcl);
    TR_TRY(launch_to_channels_last(x, xcl, B, Cin, T, pad, nullptr, s));
    float* wk = at<float>(workspace, pl.wk);
    hipLaunchKernelGGL(repack_conv_kernel, dim3(blocks_for((long)Cout * Cin * k)), dim3(256), 0, s, w, wk, (float*)nullptr, Cout, Cin, k);
    float* z = at<float>(workspace, pl.z);
    GemmParams g = conv_forward_gemm(B, Cin, Cout, T, k);
    g.A = xcl; g.W = wk; g.C = z; g.bias = bias;
    TR_TRY(launch_gemm(g, s));
    float* mean = at<float>(saved, pl.mean);
    float* invstd = at<float>(saved, pl.invstd);
    hipLaunchKernelGGL(bn_stats_kernel, dim3((Cout + 31) / 32), dim3(1024), 0, s, z, rows, Cout, mean, invstd, running_mean, running_var, 0.1f);
    hipLaunchKernelGGL(bn_act_drop_fwd_kernel, dim3(blocks_for(rows * Cout)), dim3(256), 0, s, z, mean, invstd, gamma, beta, keep,
                       keep ? 1.f / (1.f - p_drop) : 1.f, act, B, Cout, T, at<float>(saved, pl.xhat), at<float>(saved, pl.a), y);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}

int gvx_conv_bn_act_train_backward(const float* dy, const void* saved, size_t saved_bytes, const float* w, const float* gamma,
                                   const float* x_wgrad, int B, int Cin, int Cout, int T, int k, int act, const uint8_t* keep,
                                   float p_drop, float* dx, float* dw, float* dbias, float* dgamma, float* dbeta, void* workspace,
                                   size_t workspace_bytes, void* stream) {
    int rc = check_conv_args(B, Cin, Cout, T, k);
    if (rc != GVX_OK) return rc;
    if (!dy || !saved || !w || !gamma || !dw || !dbias || !dgamma || !dbeta || !workspace) return tfail(GVX_ERR_INVALID_ARG, "null argument");
    if (act != ACT_NONE && act != ACT_RELU && act != ACT_TANH) return tfail(GVX_ERR_INVALID_ARG, "activation must be 0 (none), 1 (relu) or 2 (tanh)");
    if (keep && !(p_drop >= 0.f && p_drop < 1.f)) return tfail(GVX_ERR_INVALID_ARG, "dropout probability must be in [0, 1)");
    const ConvTrainPlan pl = conv_train_plan(B, Cin, Cout, T, k);
    if (saved_bytes < pl.saved_total || workspace_bytes < pl.ws_total) return tfail(GVX_ERR_WORKSPACE, "saved / workspace buffer too small");
    if ((reinterpret_cast<uintptr_t>(saved) | reinterpret_cast<uintptr_t>(workspace)) & 255) return tfail(GVX_ERR_WORKSPACE, "buffers must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int pad = (k - 1) / 2;
    const long rows = (long)B * T;
    const float* xhat = at<float>(saved, pl.xhat);
    const float* a = at<float>(saved, pl.a);
    const float* invstd = at<float>(saved, pl.invstd);
    float* du = at<float>(workspace, pl.du);
    hipLaunchKernelGGL(act_drop_bwd_kernel, dim3(blocks_for(rows * Cout)), dim3(256), 0, s, dy, keep, keep ? 1.f / (1.f - p_drop) : 1.f, act, a,
                       B, Cout, T, du);
    // dbeta = sum du, dgamma = sum du * xhat
    launch_col_reduce(du, xhat, rows, Cout, dbeta, dgamma, s);
    float* dz = at<float>(workspace, pl.dz);
    float* dzh = at<float>(workspace, pl.dzh);
    TR_TRY(hipMemsetAsync(dzh, 0, (size_t)B * (T + 2 * pad) * Cout * sizeof(float), s));
    hipLaunchKernelGGL(bn_bwd_kernel, dim3(blocks_for(rows * Cout)), dim3(256), 0, s, du, xhat, gamma, invstd, dbeta, dgamma, B, Cout, T, pad, dz, dzh);
    launch_col_reduce(dz, nullptr, rows, Cout, dbias, nullptr, s);
    const float* xcl = at<float>(saved, pl.xcl);
    const float* xcl_w = xcl;
    if (x_wgrad) {   // (the reference masks the Postnet's input in place after its forward - outside autograd, so the first
                     // layer's weight gradient sees the MASKED input: models/tts/tacotron2.py:463, :466-473)
        float* x2 = at<float>(workspace, pl.xcl2);
        TR_TRY(launch_to_channels_last(x_wgrad, x2, B, Cin, T, pad, nullptr, s));
        xcl_w = x2;
    }
    float* dwk = at<float>(workspace, pl.dwk);
    {
        GemmParams g = conv_wgrad_gemm(B, Cin, Cout, T, k);
        g.A = dz; g.W = xcl_w; g.C = dwk;
        TR_TRY(launch_gemm_splitk(g, conv_wgrad_splitk(B, Cin, Cout, T, k), at<float>(workspace, pl.dwk_part), s));
    }
    hipLaunchKernelGGL(unpack_dw_kernel, dim3(blocks_for((long)Cout * Cin * k)), dim3(256), 0, s, dwk, dw, Cout, Cin, k);
    if (dx) {   // data gradient: flipped-tap implicit GEMM on the halo-padded dz
        float* w2 = at<float>(workspace, pl.w2);
        hipLaunchKernelGGL(repack_conv_kernel, dim3(blocks_for((long)Cout * Cin * k)), dim3(256), 0, s, w, (float*)nullptr, w2, Cout, Cin, k);
        float* dxcl = at<float>(workspace, pl.dxcl);
        GemmParams g = conv_dgrad_gemm(B, Cin, Cout, T, k);
        g.A = dzh; g.W = w2; g.C = dxcl;
        TR_TRY(launch_gemm(g, s));
        hipLaunchKernelGGL(to_channels_first_kernel, dim3(blocks_for(rows * Cin)), dim3(256), 0, s, dxcl, dx, B, Cin, T);
    }
    TR_TRY(hipGetLastError());
    return GVX_OK;
}

int gvx_tacotron2_loss_backward(const float* mel_out, const float* mel_post_out, const float* gate_out, const float* mel_target,
                                const float* gate_target, int B, int n_mels, int T, float* dmel_out, float* dmel_post_out,
                                float* dgate_out, void* stream) {
    if (!mel_out || !mel_post_out || !gate_out || !mel_target || !gate_target || !dmel_out || !dmel_post_out || !dgate_out)
        return tfail(GVX_ERR_INVALID_ARG, "null argument");
    if (B < 1 || n_mels < 1 || T < 1) return tfail(GVX_ERR_INVALID_ARG, "B, n_mels and T must be >= 1");
    const long n_mel = (long)B * n_mels * T, n_gate = (long)B * T;
    hipLaunchKernelGGL(loss_backward_kernel, dim3(blocks_for(n_mel)), dim3(256), 0, (hipStream_t)stream, mel_out, mel_post_out, gate_out,
                       mel_target, gate_target, n_mel, n_gate, dmel_out, dmel_post_out, dgate_out);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}

}  // extern "C"
