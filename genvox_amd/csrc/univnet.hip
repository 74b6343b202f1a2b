// UnivNet generator inference: mel [B][n_mels][T], noise [B][noise_dim][T] -> waveform [B][T * hop].  The model is defined in
// include/genvox_amd.h ("UnivNet generator"); the float64 restatement the tests hold this file to is tests/univnet_ref64.py.
//
// Noise upsampled through blocks whose convolutions carry weights of their own for every mel frame (location-variable convolution).
// What runs on kernels that existed: conv_pre and kernel_conv + bias_conv as implicit GEMMs over haloed rows (launch_gemm, EPI_BIAS and
// row_len), the transposed convolution (two-tap phase split), the dilated convolution and the predictor's small convolutions (hg_launch,
// hifigan.hip).  What is new here:
//
//   un_lvc_kernel<MFMA>   the LVC layer: o = bias_t + W_t y over a frame's positions, then x += sigmoid(o[:C]) * tanh(o[C:]).  A workgroup
//                         owns up to 128 positions of ONE frame (a tile never crosses a frame boundary of its weights): the frame's
//                         [2C][3C] weights (24 KB at C = 32) and the window of y - one position either side, LeakyReLU applied, zeros
//                         outside the row - go into LDS once.  MFMA (C = 32, cum a multiple of 32): a wave per 32 positions on
//                         v_mfma_f32_32x32x2_f32, positions on M, the 64 output channels as two 32-wide N tiles, 3C = 96 on K: lane r
//                         holds o[r] and o[r + 32] of its 16 positions, so bias, gate and residual add are its own epilogue.  Otherwise
//                         (C = 16, or the first block's 8 positions per frame, a quarter of a 32-row tile: that launch is bound by
//                         fetching 24 KB of weights per 98 kFLOP either way): fmaf code, a thread per (position, gate pair).
//   un_noise_reflect_kernel   noise [B][nd][T] -> channels-last [B][T + 6][Np] reflected by 3 at the row's own ends
//   un_pair_kernel        the predictor's "c + lrelu(u)" between two hg_launch convolutions; its last call writes the zero-haloed
//                         [B][T + 2][H] operand of kernel_conv
//   un_post_kernel        lrelu, the 7-tap C -> 1 convolution reflected at the row's own ends, tanh; zeros behind the row
// No atomics anywhere.  Order of this file: kernels, dims / blob / workspace layouts, the C ABI.
#include "hifigan_internal.h"

#include <algorithm>

using namespace gvx_gen;
using gvx::GemmParams;
using gvx::RowMap;
using gvx_hg::HgLayer;

namespace gvx { hipError_t gemm_init(); }

struct gvx_univnet : GenHandle {
    gvx_univnet_dims d;
    bool lds_ready = false;   // hg_prepare
};

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int UN_LDA = 36;    // floats per LDS row of the MFMA window: 32 channels, K-contiguous (HG_LD's reasoning)
constexpr int UN_LDW = 100;   // floats per LDS row of the MFMA weights: 96 k, the same residue modulo 32 banks as UN_LDA
constexpr int UN_PW_MFMA = 128, UN_PW_VALU = 64;   // most positions per workgroup

// gen_frames' `least` is GVX_UNIVNET_MIN_FRAMES where a reflection by 3 needs them, 1 for the LVC layer on its own

__device__ __forceinline__ float un_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }
__device__ __forceinline__ float4 un_lrelu4(float4 v, float s) { return make_float4(un_lrelu(v.x, s), un_lrelu(v.y, s), un_lrelu(v.z, s), un_lrelu(v.w, s)); }
__device__ __forceinline__ float un_gate(float a, float b) { return (1.f / (1.f + expf(-a))) * tanhf(b); }

struct UnLvc {
    const float* x; float* out;   // [B][T * cum][C]; out may be x: an element is read and written by one lane
    const float* y;               // [B][T * cum][C], the dilated convolution's output BEFORE its LeakyReLU
    const float* kern;            // [B][T][ld], the device order
    const int32_t* lens;
    int T, cum, C, ld, w_off, b_off;   // the layer's weights and bias inside a frame's ld floats
    int pw, tiles;                // positions per workgroup, workgroups per frame
    float slope;
};

template <bool MFMA>
__global__ void __launch_bounds__(256) un_lvc_kernel(const UnLvc p) {
    extern __shared__ __attribute__((aligned(16))) float un_smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int b = blockIdx.y, t = (int)blockIdx.x / p.tiles, st = (int)blockIdx.x - t * p.tiles;
    const int len = gen_frames(p.lens, b, p.T, 1);
    if (t >= len) return;   // (uniform over the workgroup) nothing of this row here: x stays as the transposed convolution left it
    const int C = p.C, K = 3 * C;
    const int ldw = MFMA ? UN_LDW : K + 1, lda = MFMA ? UN_LDA : C + 1;
    const int p0 = st * p.pw, np = min(p.pw, p.cum - p0);
    const long L = (long)len * p.cum, q0 = (long)t * p.cum + p0;   // the row's positions; this tile's first
    float* Ws = un_smem;                  // [2C][ldw]
    float* As = un_smem + 2 * C * ldw;    // [np + 2][lda]: y[q0 - 1 .. q0 + np]
    const float* frame = p.kern + ((size_t)b * p.T + t) * p.ld;
    const float* w = frame + p.w_off;
    const int k4 = K / 4, c4n = C / 4;
    for (int i = tid; i < 2 * C * k4; i += nthr) {
        const int n = i / k4, c4 = i - n * k4;
        const float4 v = *reinterpret_cast<const float4*>(w + (size_t)n * K + 4 * c4);
        float* d = Ws + n * ldw + 4 * c4;
        if constexpr (MFMA) { *reinterpret_cast<float4*>(d) = v; }
        else { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
    }
    const size_t row0 = (size_t)b * p.T * p.cum;
    for (int i = tid; i < (np + 2) * c4n; i += nthr) {
        const int r = i / c4n, c4 = i - r * c4n;
        const long q = q0 - 1 + r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q >= 0 && q < L) v = un_lrelu4(*reinterpret_cast<const float4*>(p.y + (row0 + (size_t)q) * C + 4 * c4), p.slope);
        float* d = As + r * lda + 4 * c4;
        if constexpr (MFMA) { *reinterpret_cast<float4*>(d) = v; }
        else { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
    }
    __syncthreads();
    const float* bias = frame + p.b_off;
    if constexpr (MFMA) {   // C = 32, np = pw = 32 * waves
        const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
        f32x16 acc0, acc1;
#pragma unroll
        for (int e = 0; e < 16; ++e) { acc0[e] = 0.f; acc1[e] = 0.f; }
#pragma unroll
        for (int tap = 0; tap < 3; ++tap)
#pragma unroll
            for (int kg = 0; kg < 4; ++kg) {
                const float4 a = *reinterpret_cast<const float4*>(&As[(wave * 32 + r + tap) * UN_LDA + 8 * kg + 4 * h]);
                const float4 w0 = *reinterpret_cast<const float4*>(&Ws[r * UN_LDW + tap * 32 + 8 * kg + 4 * h]);
                const float4 w1 = *reinterpret_cast<const float4*>(&Ws[(32 + r) * UN_LDW + tap * 32 + 8 * kg + 4 * h]);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w0.x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, w1.x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w0.y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, w1.y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w0.z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, w1.z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w0.w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, w1.w, acc1, 0, 0, 0);
            }
        // lane (r, h) holds column r of rows (e & 3) + 8 (e >> 2) + 4 h of both tiles: o[r] and o[r + 32] of 16 positions
        const float b0 = bias[r], b1 = bias[32 + r];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const long q = q0 + wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;   // inside the frame, and the frame inside the row
            const size_t at = (row0 + (size_t)q) * 32 + r;
            p.out[at] = p.x[at] + un_gate(acc0[e] + b0, acc1[e] + b1);
        }
    } else {
        for (int idx = tid; idx < np * C; idx += nthr) {
            const int pp = idx / C, j = idx - pp * C;
            const float* w0 = Ws + j * ldw;
            const float* w1 = Ws + (C + j) * ldw;
            float a0 = 0.f, a1 = 0.f;
            for (int k = 0; k < 3; ++k) {
                const float* yr = As + (pp + k) * lda;
                for (int i = 0; i < C; ++i) {
                    a0 = fmaf(yr[i], w0[k * C + i], a0);
                    a1 = fmaf(yr[i], w1[k * C + i], a1);
                }
            }
            const size_t at = (row0 + (size_t)(q0 + pp)) * C + j;
            p.out[at] = p.x[at] + un_gate(a0 + bias[j], a1 + bias[C + j]);
        }
    }
}

bool un_lvc_on_mfma(int C, int cum) { return C == 32 && cum % 32 == 0 && (cum <= UN_PW_MFMA || cum % UN_PW_MFMA == 0); }

int un_lvc(UnLvc p, int B, hipStream_t s) {
    if (un_lvc_on_mfma(p.C, p.cum)) {
        p.pw = std::min(p.cum, UN_PW_MFMA);
        p.tiles = p.cum / p.pw;
        const size_t lds = (size_t)(64 * UN_LDW + (p.pw + 2) * UN_LDA) * sizeof(float);
        un_lvc_kernel<true><<<dim3((unsigned)(p.T * p.tiles), (unsigned)B), p.pw * 2, lds, s>>>(p);
    } else {
        p.pw = std::min(p.cum, UN_PW_VALU);
        p.tiles = (p.cum + p.pw - 1) / p.pw;
        const size_t lds = (size_t)(2 * p.C * (3 * p.C + 1) + (p.pw + 2) * (p.C + 1)) * sizeof(float);
        un_lvc_kernel<false><<<dim3((unsigned)(p.T * p.tiles), (unsigned)B), 256, lds, s>>>(p);
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// noise [B][nd][T] -> out [B][T + 6][Np]: frame t at row t + 3, the row's own frames reflected by 3 at either end, zeros behind that and
// in the channel padding.  Nothing at or behind a row's length is read
__global__ void __launch_bounds__(256) un_noise_reflect_kernel(const float* __restrict__ z, const int32_t* __restrict__ lens, int nd, int T, int Np,
                                                               float* __restrict__ out) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)(T + 6) * Np) return;
    const int r = (int)(idx % (T + 6)), c = (int)(idx / (T + 6));   // consecutive threads along t, as z lies
    const int len = gen_frames(lens, b, T, GVX_UNIVNET_MIN_FRAMES);
    int t = r - 3;
    float v = 0.f;
    if (c < nd && t < len + 3 && len > 0) {
        t = t < 0 ? -t : (t >= len ? 2 * (len - 1) - t : t);
        v = z[((size_t)b * nd + c) * T + t];
    }
    out[((size_t)b * (T + 6) + r) * Np + c] = v;
}

// out = (act_a ? lrelu(a) : a) + lrelu(u) for a row's frames, [B][T][H].  halo = 1: out is [B][T + 2][H], frame t at row t + 1, and every
// other row of it - the halo and what lies behind the row's frames - is written as zeros
__global__ void __launch_bounds__(256) un_pair_kernel(const float* a, const float* __restrict__ u, const int32_t* __restrict__ lens, int T, int H,
                                                      int act_a, int halo, float slope, float* out) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int rows = T + 2 * halo;
    if (idx >= (long)rows * H) return;
    const int r = (int)(idx / H), c = (int)(idx - (long)r * H), t = r - halo;
    const int len = gen_frames(lens, b, T, 1);
    if (t >= 0 && t < len) {
        const size_t at = ((size_t)b * T + t) * H + c;
        const float av = a[at];
        out[((size_t)b * rows + r) * H + c] = (act_a ? un_lrelu(av, slope) : av) + un_lrelu(u[at], slope);
    } else if (halo) {
        out[((size_t)b * rows + r) * H + c] = 0.f;
    }
}

// wav[b][q] = tanh(bias + sum over taps, channels of w[tau][c] * lrelu(x[b][reflect(q + tau - 3)][c])) for q < T_b * hop, zeros behind;
// eight lanes per sample, each a float4 of channels at a time; pre (or nullptr) takes the value in front of the tanh
__global__ void __launch_bounds__(256) un_post_kernel(const float* __restrict__ x, const int32_t* __restrict__ lens, int T, int hop, int C,
                                                      const float* __restrict__ w, const float* __restrict__ bias, float slope, float* __restrict__ pre,
                                                      float* __restrict__ wav) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int g = (int)(idx & 7);
    const long q = idx >> 3, Lmax = (long)T * hop, L = (long)gen_frames(lens, b, T, GVX_UNIVNET_MIN_FRAMES) * hop;
    if (q >= Lmax) return;   // (the eight lanes of a sample leave together)
    float sum = 0.f;
    if (q < L) {
        for (int tau = 0; tau < 7; ++tau) {
            long pos = q + tau - 3;
            pos = pos < 0 ? -pos : (pos >= L ? 2 * (L - 1) - pos : pos);
            const float* row = x + ((size_t)b * Lmax + (size_t)pos) * C;
            for (int c = 4 * g; c < C; c += 32) {
                const float4 v = un_lrelu4(*reinterpret_cast<const float4*>(row + c), slope);
                const float4 k = *reinterpret_cast<const float4*>(w + tau * C + c);
                sum = fmaf(v.x, k.x, sum); sum = fmaf(v.y, k.y, sum); sum = fmaf(v.z, k.z, sum); sum = fmaf(v.w, k.w, sum);
            }
        }
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (g == 0) {
        const float v = q < L ? sum + bias[0] : 0.f;
        if (pre) pre[(size_t)b * Lmax + q] = v;
        wav[(size_t)b * Lmax + q] = q < L ? tanhf(v) : 0.f;
    }
}

// ---- dims, blob, workspace
inline int un_mp(const gvx_univnet_dims& d) { return (d.n_mels + 3) & ~3; }
inline int un_np(const gvx_univnet_dims& d) { return (d.noise_dim + 3) & ~3; }
inline size_t un_layer_floats(int C) { return (size_t)6 * C * C; }   // one layer's [2C][3C] weights
inline size_t un_ld(int C, int n_layers) { return (size_t)n_layers * (un_layer_floats(C) + 2 * C); }
inline int un_hop(const gvx_univnet_dims& d) {
    int hop = 1;
    for (int i = 0; i < d.n_blocks; ++i) hop *= d.strides[i];
    return hop;
}

const char* un_lvc_problem(int C, int cum, int dilation) {
    if (C < 4 || C > 32 || (C & 3)) return "channel_size must be a multiple of 4 in [4, 32]";
    if (cum < 1 || cum > 4096) return "the positions per frame must be in [1, 4096]";
    if (dilation < 1 || dilation > GVX_UNIVNET_MAX_DILATION) return "every dilation must be in [1, GVX_UNIVNET_MAX_DILATION]";
    return nullptr;
}

const char* un_dims_problem(const gvx_univnet_dims* d) {
    if (!d) return "null dims";
    if (d->n_mels < 1 || d->n_mels > 4096) return "n_mels must be in [1, 4096]";
    if (d->noise_dim < 1 || d->noise_dim > 1024) return "noise_dim must be in [1, 1024]";
    if (d->n_dilations < 1 || d->n_dilations > GVX_UNIVNET_MAX_DILATIONS) return "there must be 1 to GVX_UNIVNET_MAX_DILATIONS dilations";
    if (d->n_blocks < 1 || d->n_blocks > GVX_UNIVNET_MAX_BLOCKS) return "there must be 1 to GVX_UNIVNET_MAX_BLOCKS strides";
    long hop = 1;
    for (int i = 0; i < d->n_blocks; ++i) {
        const int s = d->strides[i];
        if (s < 2 || s > 64 || (s & 1)) return "every stride must be even and in [2, 64] (the two-tap phase split of the transposed convolution; an odd stride's output_padding form is not built)";
        hop *= s;
        if (hop > 4096) return "the strides multiply to more than 4096";
    }
    for (int m = 0; m < d->n_dilations; ++m)
        if (const char* why = un_lvc_problem(d->channel_size, 1, d->dilations[m])) return why;
    const int H = d->kpnet_hidden_channels;
    if (H < 32 || H > GVX_UNIVNET_MAX_HIDDEN || H % 32) return "kpnet_hidden_channels must be a multiple of 32 in [32, GVX_UNIVNET_MAX_HIDDEN]";
    if (d->kpnet_conv_size != 3) return "kpnet_conv_size must be 3";
    if (!(d->slope >= 0.f && d->slope <= 1.f)) return "lReLU_slope must be in [0, 1]";
    return nullptr;
}

struct UnBlock { size_t up_w, up_b, in_w, in_b, res_w[6], res_b[6], kb_w, kb_b, conv_w[GVX_UNIVNET_MAX_DILATIONS], conv_b[GVX_UNIVNET_MAX_DILATIONS]; };
struct UnBlob {
    size_t pre_w, pre_b;
    UnBlock block[GVX_UNIVNET_MAX_BLOCKS];
    size_t post_w, post_b, total;
};

UnBlob un_blob_layout(const gvx_univnet_dims& d) {
    UnBlob L{};
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t o = at; at += gvx::round64(floats); return o; };
    const size_t C = d.channel_size, H = d.kpnet_hidden_channels, ld = un_ld(d.channel_size, d.n_dilations);
    L.pre_w = take(C * 7 * un_np(d)); L.pre_b = take(C);
    for (int i = 0; i < d.n_blocks; ++i) {
        UnBlock& k = L.block[i];
        k.up_w = take((size_t)d.strides[i] * C * 2 * C); k.up_b = take(C);
        k.in_w = take(H * 5 * un_mp(d)); k.in_b = take(H);
        for (int j = 0; j < 6; ++j) { k.res_w[j] = take(H * 3 * H); k.res_b[j] = take(H); }
        k.kb_w = take(ld * 3 * H); k.kb_b = take(ld);
        for (int m = 0; m < d.n_dilations; ++m) { k.conv_w[m] = take(C * 3 * C); k.conv_b[m] = take(C); }
    }
    L.post_w = take(7 * C); L.post_b = take(1);
    L.total = at;
    return L;
}

struct UnWs { size_t mel_t, noise_t, pc, pt, pu, hal, kern, xa, xb, y, total; };

UnWs un_ws_plan(const gvx_univnet_dims& d, int B, int T) {
    UnWs w{};
    GenRows ws{B};
    const size_t H = d.kpnet_hidden_channels, wide = (size_t)T * un_hop(d) * d.channel_size;
    w.mel_t = ws.rows((size_t)T * un_mp(d));
    w.noise_t = ws.rows((size_t)(T + 6) * un_np(d));
    w.pc = ws.rows(T * H); w.pt = ws.rows(T * H); w.pu = ws.rows(T * H);
    w.hal = ws.rows((size_t)(T + 2) * H);
    w.kern = ws.rows((size_t)T * un_ld(d.channel_size, d.n_dilations));
    w.xa = ws.rows(wide); w.xb = ws.rows(wide); w.y = ws.rows(wide);
    w.total = ws.total;
    return w;
}

const char* un_shape_problem(int B, int T) {
    if (B < 1 || B > 65535) return "B must be in [1, 65535]";
    if (T < 1 || T > GVX_UNIVNET_MAX_FRAMES) return "T must be in [1, GVX_UNIVNET_MAX_FRAMES]";
    if ((long)B * T > (1L << 24)) return "B * T is beyond 2^24 frames";
    return nullptr;
}

// [B][T][N] = A W^T + bias over rows of K floats that start `a_stride` floats apart inside a row group of `a_rows` rows
int un_gemm(const float* A, int a_rows, int a_stride, int K, const float* W, const float* bias, float* out, int N, int B, int T, const int32_t* lens,
            hipStream_t s) {
    GemmParams g{};
    g.A = A; g.amap = RowMap{T, (long)a_rows * a_stride, (long)a_stride}; g.W = W; g.ldw = K;
    g.C = out; g.cmap = RowMap{T, (long)T * N, (long)N};
    g.bias = bias; g.keep = nullptr; g.keep_ld = 0;
    g.M = B * T; g.N = N; g.K = K;
    g.act = gvx::ACT_NONE; g.row_len = lens;
    HIP_TRY(gvx::launch_gemm(g, s));
    return GVX_OK;
}

HgLayer un_layer(const float* src, const float* w, const float* bias, float* out, const int32_t* lens, int T, int in_mul, int Cin, int Cout, int taps,
                 int dil, int phases, int act, float slope) {
    HgLayer p{};
    p.lens = lens; p.T = T; p.slope = slope;
    p.src = src; p.W = w; p.bias = bias; p.out = out;
    p.in_mul = in_mul; p.Cin = Cin; p.Cout = Cout; p.taps = taps; p.K = taps * Cin; p.dil = dil; p.phases = phases; p.act = act;
    return p;
}

// gvx_lvc_gated has no handle: the dynamic-LDS sizes of its hg_launch are set once per process (a static local: one thread runs it)
int un_lone_prepare() {
    static bool ready = false;
    static const int rc = gvx_hg::hg_prepare(&ready);
    return rc;
}

}  // namespace

extern "C" {

int gvx_lvc_gated(const float* x, const float* kern, int n_layers, int layer, const float* conv_w, const float* conv_b, int dilation,
                  const int32_t* lens, int B, int T, int cum, int C, float slope, float* scratch, float* out, void* stream) {
    if (!x || !kern || !out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if ((conv_w == nullptr) != (conv_b == nullptr)) return fail(GVX_ERR_INVALID_ARG, "the dilated convolution needs its weight and its bias, or neither");
    if (conv_w && (!scratch || scratch == x || scratch == out)) return fail(GVX_ERR_INVALID_ARG, "with a convolution, scratch must be a tensor of its own");
    // without a convolution y IS x: a workgroup reads one position either side of its own, which a neighbour would be writing in place
    if (!conv_w && out == x) return fail(GVX_ERR_INVALID_ARG, "without a convolution out must not be x: the layer reads its neighbours' positions of x");
    if (const char* why = un_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (const char* why = un_lvc_problem(C, cum, dilation)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if ((long)T * cum > (1L << 28)) return fail(GVX_ERR_INVALID_ARG, "T * cum is beyond 2^28 positions");
    if (n_layers < 1 || n_layers > GVX_UNIVNET_MAX_DILATIONS || layer < 0 || layer >= n_layers)
        return fail(GVX_ERR_INVALID_ARG, "layer %d of %d: there are 1 to %d layers", layer, n_layers, (int)GVX_UNIVNET_MAX_DILATIONS);
    if (!(slope >= 0.f && slope <= 1.f)) return fail(GVX_ERR_INVALID_ARG, "slope must be in [0, 1]");
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)kern | (uintptr_t)scratch | (uintptr_t)conv_w) & 15)
        return fail(GVX_ERR_INVALID_ARG, "x, out, kern, scratch and conv_w must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    const float* y = x;
    if (conv_w) {
        if ((rc = un_lone_prepare()) != GVX_OK) return rc;
        const HgLayer p = un_layer(x, conv_w, conv_b, scratch, lens, T, cum, C, C, 3, dilation, 1, 1, slope);
        if ((rc = gvx_hg::hg_launch(p, B, s)) != GVX_OK) return rc;
        y = scratch;
    }
    UnLvc a{};
    a.x = x; a.out = out; a.y = y; a.kern = kern; a.lens = lens; a.T = T; a.cum = cum; a.C = C; a.slope = slope;
    a.ld = (int)un_ld(C, n_layers);
    a.w_off = (int)(layer * un_layer_floats(C));
    a.b_off = (int)(n_layers * un_layer_floats(C)) + layer * 2 * C;
    if (out != x && lens) {   // what the LVC leaves alone: the positions behind a row's own.  Without lengths it writes every position
        HIP_TRY(hipMemcpyAsync(out, x, (size_t)B * T * cum * C * sizeof(float), hipMemcpyDeviceToDevice, s));
        a.x = out;
    }
    return un_lvc(a, B, s);
}

size_t gvx_univnet_blob_floats(const gvx_univnet_dims* dims) {
    if (un_dims_problem(dims)) return 0;
    return un_blob_layout(*dims).total;
}

size_t gvx_univnet_workspace_bytes(const gvx_univnet_dims* dims, int B, int T) {
    if (un_dims_problem(dims) || un_shape_problem(B, T)) return 0;
    return un_ws_plan(*dims, B, T).total;
}

int gvx_univnet_pack_weights_device(const gvx_univnet_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = un_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_univnet_dims& d = *dims;
    const UnBlob L = un_blob_layout(d);
    GenPacker P{{table, n}};
    auto pair = [&](const std::string& name, size_t dst_w, size_t numel_w, size_t dst_b, size_t numel_b) {
        P.take(name + ".weight", dst_w, numel_w);
        P.take(name + ".bias", dst_b, numel_b);
    };
    const size_t C = d.channel_size, H = d.kpnet_hidden_channels, ld = un_ld(d.channel_size, d.n_dilations);
    pair("conv_pre", L.pre_w, C * 7 * un_np(d), L.pre_b, C);
    for (int i = 0; i < d.n_blocks; ++i) {
        const std::string base = "res_stack." + std::to_string(i) + ".", kp = base + "kernel_predictor.";
        const UnBlock& k = L.block[i];
        pair(base + "convt_pre", k.up_w, (size_t)d.strides[i] * C * 2 * C, k.up_b, C);
        pair(kp + "input_conv", k.in_w, H * 5 * un_mp(d), k.in_b, H);
        for (int j = 0; j < 6; ++j) pair(kp + "residual_convs." + std::to_string(j / 2) + (j & 1 ? ".3" : ".1"), k.res_w[j], H * 3 * H, k.res_b[j], H);
        pair(kp + "kb", k.kb_w, ld * 3 * H, k.kb_b, ld);
        for (int m = 0; m < d.n_dilations; ++m) pair(base + "conv_blocks." + std::to_string(m), k.conv_w[m], C * 3 * C, k.conv_b[m], C);
    }
    pair("conv_post", L.post_w, 7 * C, L.post_b, 1);
    return P.run(device_blob, 0, L.total, (hipStream_t)stream);
}

int gvx_univnet_create(const gvx_univnet_dims* dims, gvx_univnet** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = un_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_univnet* h = new gvx_univnet();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_univnet_destroy(gvx_univnet* h) { delete h; }

int gvx_univnet_bind(gvx_univnet* h, const float* device_blob) {
    if (const int rc = gen_bind(h, device_blob)) return rc;
    HIP_TRY(gvx::gemm_init());   // the big tiles' dynamic LDS
    return gvx_hg::hg_prepare(&h->lds_ready);
}

int gvx_univnet_timing_enable(gvx_univnet* h, int enable) { return gen_timing_enable(h, enable, h ? 2 * h->d.n_blocks + 3 : 0); }

int gvx_univnet_stage_times_ms(gvx_univnet* h, float* ms_out, int* n_out) { return gen_stage_times_ms(h, h ? 2 * h->d.n_blocks + 2 : 0, ms_out, n_out); }

int gvx_univnet_forward(gvx_univnet* h, const float* mel, const float* noise, const int32_t* frame_lengths, int B, int T, float* wav_out,
                        float* const* stage_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !mel || !noise || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    const gvx_univnet_dims& d = h->d;
    if (const char* why = un_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (T < GVX_UNIVNET_MIN_FRAMES) return fail(GVX_ERR_INVALID_ARG, "T = %d: a row needs at least %d frames", T, (int)GVX_UNIVNET_MIN_FRAMES);
    const UnWs wp = un_ws_plan(d, B, T);
    const int n_stage = d.n_blocks + 2;
    int ev = 0, rc;
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    if ((rc = gen_check_stage_out(stage_out, n_stage)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const UnBlob L = un_blob_layout(d);
    const float* blob = h->blob;
    const int C = d.channel_size, H = d.kpnet_hidden_channels, Mp = un_mp(d), Np = un_np(d), D = d.n_dilations;
    const int ld = (int)un_ld(C, D);
    const float slope = d.slope;
    const int32_t* lens = frame_lengths;
    float* mel_t = gvx::ws_ptr<float>(workspace, wp.mel_t);
    float* noise_t = gvx::ws_ptr<float>(workspace, wp.noise_t);
    float* pc = gvx::ws_ptr<float>(workspace, wp.pc);
    float* pt = gvx::ws_ptr<float>(workspace, wp.pt);
    float* pu = gvx::ws_ptr<float>(workspace, wp.pu);
    float* hal = gvx::ws_ptr<float>(workspace, wp.hal);
    float* kern = gvx::ws_ptr<float>(workspace, wp.kern);
    float* xa = gvx::ws_ptr<float>(workspace, wp.xa);
    float* xb = gvx::ws_ptr<float>(workspace, wp.xb);
    float* y = gvx::ws_ptr<float>(workspace, wp.y);
    auto stamp = [&] { return gen_mark(h, ev++, s); };
    auto hg = [&](const float* src, size_t w, size_t bias, float* out, int in_mul, int Cin, int Cout, int taps, int dil, int phases, int act, int zero_tail) {
        HgLayer p = un_layer(src, blob + w, blob + bias, out, lens, T, in_mul, Cin, Cout, taps, dil, phases, act, slope);
        p.zero_tail = zero_tail;
        return gvx_hg::hg_launch(p, B, s);
    };
    auto pairs = [&](const float* a, const float* u, int act_a, int halo, float* out) -> int {
        const long count = (long)(T + 2 * halo) * H;
        un_pair_kernel<<<dim3((unsigned)((count + 255) / 256), (unsigned)B), 256, 0, s>>>(a, u, lens, T, H, act_a, halo, slope, out);
        HIP_TRY(hipGetLastError());
        return GVX_OK;
    };
    if ((rc = stamp()) != GVX_OK) return rc;

    // conv_pre: the im2col row of (b, t) is the 7 Np floats from row t of the reflected noise
    un_noise_reflect_kernel<<<dim3((unsigned)(((long)(T + 6) * Np + 255) / 256), (unsigned)B), 256, 0, s>>>(noise, lens, d.noise_dim, T, Np, noise_t);
    HIP_TRY(hipGetLastError());
    float* cur = stage_out ? stage_out[0] : xa;
    if ((rc = un_gemm(noise_t, T + 6, Np, 7 * Np, blob + L.pre_w, blob + L.pre_b, cur, C, B, T, lens, s)) != GVX_OK) return rc;
    if ((rc = gvx_hg::hg_mel_transpose(mel, lens, B, d.n_mels, T, Mp, mel_t, s)) != GVX_OK) return rc;
    if ((rc = stamp()) != GVX_OK) return rc;

    int cum = 1;
    for (int i = 0; i < d.n_blocks; ++i) {
        const UnBlock& k = L.block[i];
        // the kernel predictor, at the frame rate.  pc holds input_conv's output before its lrelu, then the running c
        if ((rc = hg(mel_t, k.in_w, k.in_b, pc, 1, Mp, H, 5, 1, 1, 0, 0)) != GVX_OK) return rc;
        for (int j = 0; j < 3; ++j) {
            if ((rc = hg(pc, k.res_w[2 * j], k.res_b[2 * j], pt, 1, H, H, 3, 1, 1, j == 0, 0)) != GVX_OK) return rc;
            if ((rc = hg(pt, k.res_w[2 * j + 1], k.res_b[2 * j + 1], pu, 1, H, H, 3, 1, 1, 1, 0)) != GVX_OK) return rc;
            if ((rc = pairs(pc, pu, j == 0, j == 2, j == 2 ? hal : pc)) != GVX_OK) return rc;
        }
        if ((rc = un_gemm(hal, T + 2, H, 3 * H, blob + k.kb_w, blob + k.kb_b, kern, ld, B, T, lens, s)) != GVX_OK) return rc;
        if ((rc = stamp()) != GVX_OK) return rc;

        const int st = d.strides[i];
        float* next = stage_out ? stage_out[i + 1] : (cur == xa ? xb : xa);
        if ((rc = hg(cur, k.up_w, k.up_b, next, cum, C, C, 2, 0, st, 1, 1)) != GVX_OK) return rc;
        cum *= st;
        for (int m = 0; m < D; ++m) {
            if ((rc = hg(next, k.conv_w[m], k.conv_b[m], y, cum, C, C, 3, d.dilations[m], 1, 1, 0)) != GVX_OK) return rc;
            UnLvc a{};
            a.x = next; a.out = next; a.y = y; a.kern = kern; a.lens = lens; a.T = T; a.cum = cum; a.C = C; a.slope = slope;
            a.ld = ld; a.w_off = (int)(m * un_layer_floats(C)); a.b_off = (int)(D * un_layer_floats(C)) + m * 2 * C;
            if ((rc = un_lvc(a, B, s)) != GVX_OK) return rc;
        }
        cur = next;
        if ((rc = stamp()) != GVX_OK) return rc;
    }
    const long samples = (long)T * cum;
    un_post_kernel<<<dim3((unsigned)((samples * 8 + 255) / 256), (unsigned)B), 256, 0, s>>>(cur, lens, T, cum, C, blob + L.post_w, blob + L.post_b, slope,
                                                                                             stage_out ? stage_out[n_stage - 1] : nullptr, wav_out);
    HIP_TRY(hipGetLastError());
    return stamp();
}

}  // C ABI
