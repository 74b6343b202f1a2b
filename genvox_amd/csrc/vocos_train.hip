// Vocos generator: the forward that keeps a tape, and the backward (include/genvox_amd.h, "Vocos generator: training").  The float64
// autograd the tests hold this file to is tests/vocos_grad_ref64.py.
//
// Every product is the dense fp32 GEMM (gemm_f32.hip): data gradients are launch_gemm with row_len on weights transposed from the bound
// blob at the start of the call, weight gradients its K-major form with split-K partials in the workspace, bias gradients
// launch_col_reduce.  What is new here:
//
//   vcb_ln_kernel<NC>     LayerNorm backward behind the recomputed 7-tap filter, the twin of vc_dwconv_ln_kernel: a workgroup of four waves
//                         per piece of GVX_VOCOS_GRAD_PIECE frames of one row - not per GVX_VOCOS_TILE frames as the forward, so that the
//                         piece's sums stay in registers - wave w taking frames w, w + 4, .. of the piece, lanes along the channels; the
//                         filter's seven inputs come straight from memory (no LDS tile: seven loads per element, neighbours' in L2);
//                         u = dwconv(x) + b and its statistics as the forward forms them (the mean, the mean of what is
//                         left, then the squared deviations, all over registers), du = rstd (dxh - mean(dxh) - xh mean(dxh xh)).  taps = 7
//                         writes du; taps = 0 writes dx = du + d_res.  The sums over frames of dy xh, dy and du stay in registers over the
//                         piece, the four waves are added in wave order through LDS, and the piece's partial goes to the workspace.
//   vcb_dw_kernel         the filter's adjoint, a wave per 64 channels of a piece (nothing crosses channels here): dx[t] = d_res[t] +
//                         sum_j w[j] du[t + 3 - j] and the piece's d w[j] = sum_t du[t] x[t + j - 3], frames in ascending order.
//   vcb_sum_kernel        adds the pieces' partials in piece order and writes the four parameter gradients, the filter's as [C][1][7].
//   vcb_gelu_kernel       h = gelu(p) and dp = dh (Phi(p) + p phi(p)), 16 bytes per lane, on gelu.h's one function.
//   vcb_env_kernel        d_wav / envelope inside a row's delivered samples, 0 behind them (the envelope summed as vc_ola_kernel sums it).
//   vcb_istft_kernel<H>   a frame per wave: the gather through the trim, the window and 1 / N, the forward real transform in LDS
//                         (fft_lds.h), and the chain rule through mag (cos p + i sin p) with the forward's own expf, clamp and sincosf.
//   vcb_unfold_kernel     gradients with respect to gamma (.) pwconv2 -> those of gamma, pwconv2.weight and pwconv2.bias.
// No atomics anywhere; every sum over frames is a sum of pieces in a fixed order.  Frames at and behind a row's length are written as
// zeros by every launch and read by none.
//
// Order of this file: kernels, layouts, the two kernels' own entry points, forward_train, backward.
#include "fft_lds.h"
#include "gelu.h"
#include "gen_backward.h"
#include "train_internal.h"
#include "vocos_internal.h"

#include <algorithm>

using namespace gvx_gen;
using namespace gvx_vc;
using gvx::GemmParams;
using gvx::RowMap;

namespace {

constexpr int VCB_PIECE = GVX_VOCOS_GRAD_PIECE;
constexpr int VCB_SUMS = 10;   // per piece and channel: d ln_w, d ln_b, d b, d w[0 .. 6]

struct VcbNorm {
    const float* x; const float* dy; const float* d_res;
    float* out; long out_bs;   // taps 7: du, taps 0: dx; row b at out + b * out_bs
    const int32_t* lens;
    int T, C, taps;
    const float* w; const float* b; const float* ln_w;
    float eps;
    float* part;               // [B * pieces per row][VCB_SUMS][C]
};

template <int NC>   // channels per lane: C <= 64 NC
__global__ void __launch_bounds__(VC_WAVES * 64) vcb_ln_kernel(const VcbNorm p) {
    extern __shared__ __attribute__((aligned(16))) float sums[];   // [VC_WAVES][3][C]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, piece = blockIdx.x, t0 = piece * VCB_PIECE, C = p.C;
    const int len = gen_frames(p.lens, b, p.T);
    const size_t row = (size_t)b * p.T;
    const int t_end = min(t0 + VCB_PIECE, p.T);
    const bool filter = p.taps != 0;
    float lw[NC], cb[NC], cw[7][NC], g_w[NC], g_b[NC], g_cb[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        const bool ok = c < C;
        lw[i] = ok ? p.ln_w[c] : 0.f;
        cb[i] = ok && filter ? p.b[c] : 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) cw[j][i] = ok && filter ? p.w[j * C + c] : 0.f;
        g_w[i] = g_b[i] = g_cb[i] = 0.f;
    }
    const float c_f = (float)C;
    for (int t = t0 + wave; t < t_end; t += VC_WAVES) {
        float* o = p.out + (size_t)b * p.out_bs + (size_t)t * C;
        if (t >= len) {
#pragma unroll
            for (int i = 0; i < NC; ++i)
                if (lane + 64 * i < C) o[lane + 64 * i] = 0.f;
            continue;
        }
        float v[NC], sum = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c = lane + 64 * i;
            float a = 0.f;
            if (c < C) {
                if (filter) {
                    a = cb[i];
#pragma unroll
                    for (int j = 0; j < 7; ++j) {   // the forward's order; zeros outside the row, which is never read there
                        const int tj = t + j - 3;
                        const float xv = tj >= 0 && tj < len ? p.x[(row + tj) * C + c] : 0.f;
                        a = fmaf(xv, cw[j][i], a);
                    }
                } else {
                    a = p.x[(row + t) * C + c];
                }
            }
            v[i] = a;
            sum += a;
        }
        // the forward's statistics, word for word: an offset of 1e3 must not cost the digits of xh
        const float mean = vc_wave_sum(sum) / c_f;
        float rest = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            v[i] = lane + 64 * i < C ? v[i] - mean : 0.f;
            rest += v[i];
        }
        const float mean2 = vc_wave_sum(rest) / c_f;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            v[i] = lane + 64 * i < C ? v[i] - mean2 : 0.f;
            sq = fmaf(v[i], v[i], sq);
        }
        const float rstd = 1.f / sqrtf(vc_wave_sum(sq) / c_f + p.eps);
        float dxh[NC], s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c = lane + 64 * i;
            v[i] *= rstd;   // xh
            const float g = c < C ? p.dy[(row + t) * C + c] : 0.f;
            dxh[i] = g * lw[i];
            s1 += dxh[i];
            s2 = fmaf(dxh[i], v[i], s2);
            g_w[i] = fmaf(g, v[i], g_w[i]);
            g_b[i] += g;
        }
        const float m1 = vc_wave_sum(s1) / c_f, m2 = vc_wave_sum(s2) / c_f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c = lane + 64 * i;
            if (c >= C) continue;
            const float du = rstd * ((dxh[i] - m1) - v[i] * m2);
            if (filter) {
                o[c] = du;
                g_cb[i] += du;
            } else {
                o[c] = p.d_res ? du + p.d_res[(row + t) * C + c] : du;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (c < C) {
            sums[(wave * 3 + 0) * C + c] = g_w[i];
            sums[(wave * 3 + 1) * C + c] = g_b[i];
            sums[(wave * 3 + 2) * C + c] = g_cb[i];
        }
    }
    __syncthreads();
    float* part = p.part + ((size_t)b * gridDim.x + piece) * VCB_SUMS * C;
    for (int idx = tid; idx < 3 * C; idx += VC_WAVES * 64) {
        const int k = idx / C, c = idx - k * C;
        float s = sums[k * C + c];
#pragma unroll
        for (int w = 1; w < VC_WAVES; ++w) s += sums[(w * 3 + k) * C + c];
        part[k * C + c] = s;
    }
}

struct VcbFilter {
    const float* x; const float* du; const float* d_res; float* dx;
    const int32_t* lens;
    int T, C;
    const float* w;
    float* part;
};

__global__ void __launch_bounds__(64) vcb_dw_kernel(const VcbFilter p) {
    const int c = (int)blockIdx.z * 64 + threadIdx.x, C = p.C;
    if (c >= C) return;
    const int b = blockIdx.y, piece = blockIdx.x, t0 = piece * VCB_PIECE;
    const int len = gen_frames(p.lens, b, p.T);
    const size_t row = (size_t)b * p.T;
    const int t_end = min(t0 + VCB_PIECE, p.T);
    float w[7], acc[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) { w[j] = p.w[j * C + c]; acc[j] = 0.f; }
    for (int t = t0; t < t_end; ++t) {
        const size_t at = (row + t) * C + c;
        if (t >= len) { p.dx[at] = 0.f; continue; }
        float r = p.d_res ? p.d_res[at] : 0.f;
        const float d0 = p.du[at];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int tq = t + 3 - j, tx = t + j - 3;
            if (tq >= 0 && tq < len) r = fmaf(w[j], p.du[(row + tq) * C + c], r);
            if (tx >= 0 && tx < len) acc[j] = fmaf(d0, p.x[(row + tx) * C + c], acc[j]);
        }
        p.dx[at] = r;
    }
    float* part = p.part + ((size_t)b * gridDim.x + piece) * VCB_SUMS * C;
#pragma unroll
    for (int j = 0; j < 7; ++j) part[(3 + j) * C + c] = acc[j];
}

// the pieces in index order; d_w in PyTorch's [C][1][7]
__global__ void __launch_bounds__(256) vcb_sum_kernel(const float* __restrict__ part, int pieces, int C, int taps, float* d_lnw, float* d_lnb, float* d_b,
                                                      float* d_w) {
    const int idx = (int)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (taps ? VCB_SUMS : 2) * C) return;
    const int k = idx / C, c = idx - k * C;
    double s = 0.0;
    for (int i = 0; i < pieces; ++i) s += (double)part[((size_t)i * VCB_SUMS + k) * C + c];
    const float v = (float)s;
    if (k == 0) d_lnw[c] = v;
    else if (k == 1) d_lnb[c] = v;
    else if (k == 2) d_b[c] = v;
    else d_w[c * 7 + (k - 3)] = v;
}

__global__ void __launch_bounds__(256) vcb_gelu_kernel(const float4* __restrict__ p, const float4* dh, float4* __restrict__ h, float4* dp, long n4) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const float4 v = p[i];
    h[i] = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
    if (dh) {
        const float4 g = dh[i];
        dp[i] = make_float4(g.x * gelu_erf_grad(v.x), g.y * gelu_erf_grad(v.y), g.z * gelu_erf_grad(v.z), g.w * gelu_erf_grad(v.w));
    }
}

// out[b][i] = d_wav[b][i] / envelope(i) inside the row's delivered samples, 0 behind them (d_wav is not read there)
__global__ void __launch_bounds__(256) vcb_env_kernel(const float* __restrict__ d_wav, const int32_t* __restrict__ lens, int T, const float* __restrict__ win,
                                                      int N, int hop, int center, float* __restrict__ out) {
    const long i_long = (long)blockIdx.x * 256 + threadIdx.x;
    const long n_max = (long)T * hop;
    const int b = blockIdx.y;
    if (i_long >= n_max) return;
    const int i = (int)i_long;
    const int len = gen_frames(lens, b, T);
    const int nb = center ? (len - 1) * hop : len * hop;
    float r = 0.f;
    if (i < nb) {
        const int p = i + (center ? N / 2 : (N - hop) / 2);
        const int t_lo = p >= N ? (p - N) / hop + 1 : 0;
        const int t_hi = min(len - 1, p / hop);
        float den = 0.f;
        for (int t = t_lo; t <= t_hi; ++t) {
            const float w = win[p - t * hop];
            den += w * w;
        }
        r = d_wav[(long)b * n_max + i] / den;
    }
    out[(long)b * n_max + i] = r;
}

struct VcbIstft {
    const float* coeffs;   // [B][T][N + 2]
    const float* dwe;      // [B][T * hop]: d_wav / envelope
    const int32_t* lens;
    int T, hop, center, ld;
    const float* win; const float2* tw; const float2* tw2;
    float* d_coeffs;       // [B][T][ld], ld >= N + 2: zeros in the columns from N + 2 on
};

template <int H>
__global__ void __launch_bounds__(VC_WAVES * 64) vcb_istft_kernel(const VcbIstft p) {
    constexpr int Q = H / 64, N = 2 * H;
    __shared__ __attribute__((aligned(16))) float2 fsm[VC_WAVES * fft_lds_words<H>()];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t = (int)blockIdx.x * VC_WAVES + wave;
    if (t >= p.T) return;
    const int len = gen_frames(p.lens, b, p.T);
    const long f = (long)b * p.T + t;
    float* dc = p.d_coeffs + f * p.ld;
    if (t >= len) {
        for (int k = j; k < p.ld; k += 64) dc[k] = 0.f;
        return;
    }
    const float* c = p.coeffs + f * (N + 2);
    float2* buf = fsm + wave * fft_lds_words<H>();
    const int nb = p.center ? (len - 1) * p.hop : len * p.hop;
    const int base = t * p.hop - (p.center ? N / 2 : (N - p.hop) / 2);
    const float* g = p.dwe + (long)b * p.T * p.hop;
    const float inv_n = 1.f / (float)N;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int m = j + 64 * q, i0 = base + 2 * m;
        const float g0 = i0 >= 0 && i0 < nb ? g[i0] : 0.f;
        const float g1 = i0 + 1 >= 0 && i0 + 1 < nb ? g[i0 + 1] : 0.f;
        const float2 w = *reinterpret_cast<const float2*>(p.win + 2 * m);
        buf[fpad(m)] = make_float2(w.x * (g0 * inv_n), w.y * (g1 * inv_n));
    }
    wave_lds_fence();
    fft_lds_wave<H, false>(buf, p.tw, j);
#pragma unroll
    for (int q = 0; q <= Q; ++q) {
        const int k = j + 64 * q;
        if (k <= H) {
            const bool edge = k == 0 || k == H;
            const float2 X = rfft_split(buf[fpad(k & (H - 1))], buf[fpad((H - k) & (H - 1))], p.tw2[k], edge);
            const float ck = edge ? 1.f : 2.f;
            const float d_re = ck * X.x, d_im = ck * X.y;   // (X.y is 0 at DC and Nyquist)
            const float e = expf(c[k]);
            const float mag = fminf(e, VC_MAG_MAX);
            float sn, cs;
            sincosf(c[H + 1 + k], &sn, &cs);
            dc[k] = e <= VC_MAG_MAX ? (d_re * cs + d_im * sn) * mag : 0.f;
            dc[H + 1 + k] = mag * (d_im * cs - d_re * sn);
        }
    }
    for (int k = N + 2 + j; k < p.ld; k += 64) dc[k] = 0.f;
}

// dst[c][r] = src[r][c] for r < rows, 0 for rows <= r < rows_p; dst rows are rows_p long
__global__ void __launch_bounds__(256) vcb_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int rows, int cols, int rows_p) {
    __shared__ float tile[32][33];
    const int r0 = (int)blockIdx.x * 32, c0 = (int)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = r < rows && c < cols ? src[(size_t)r * cols + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows_p) dst[(size_t)c * rows_p + r] = tile[tx][i];
    }
}

// the embedding's weight [C][7][Cp] -> [Cp][7][C] with the taps reversed: the operand of its data gradient
__global__ void __launch_bounds__(256) vcb_embed_t_kernel(const float* __restrict__ w, float* __restrict__ dst, int C, int Cp) {
    const int idx = (int)blockIdx.x * 256 + threadIdx.x;
    if (idx >= Cp * 7 * C) return;
    const int m = idx / (7 * C), rem = idx - m * 7 * C, j = rem / C, c = rem - j * C;
    dst[idx] = w[((size_t)c * 7 + (6 - j)) * Cp + m];
}

// the embedding's weight gradient [C][7][Cp] -> PyTorch's [C][n_mels][7]
__global__ void __launch_bounds__(256) vcb_embed_grad_kernel(const float* __restrict__ g, float* __restrict__ dst, int C, int M, int Cp) {
    const int idx = (int)blockIdx.x * 256 + threadIdx.x;
    if (idx >= C * M * 7) return;
    const int c = idx / (7 * M), rem = idx - c * 7 * M, m = rem / 7, j = rem - m * 7;
    dst[idx] = g[((size_t)c * 7 + j) * Cp + m];
}

// Gradients with respect to the folded W2' = gamma (.) W2 and b2' = gamma (.) b2 -> those of gamma, W2 and b2; a workgroup per output
// channel, the channel's sum as 256 strided sums and a tree.  No division by gamma
__global__ void __launch_bounds__(256) vcb_unfold_kernel(const float* __restrict__ dw2f, const float* __restrict__ db2f, const float* __restrict__ gamma,
                                                         const float* __restrict__ w2, const float* __restrict__ b2, int I, float* __restrict__ dw2,
                                                         float* __restrict__ db2, float* __restrict__ dgamma) {
    __shared__ double red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const float g = gamma[c];
    double s = 0.0;
    for (int i = tid; i < I; i += 256) {
        const float v = dw2f[(size_t)c * I + i];
        dw2[(size_t)c * I + i] = g * v;
        s += (double)v * (double)w2[(size_t)c * I + i];
    }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const float v = db2f[c];
        dgamma[c] = (float)(red[0] + (double)v * (double)b2[c]);
        db2[c] = g * v;
    }
}

// ---- launches
inline int vcb_pieces(int T) { return (T + VCB_PIECE - 1) / VCB_PIECE; }

int vcb_ln(const VcbNorm& p, int B, hipStream_t s) {
    const dim3 grid((unsigned)vcb_pieces(p.T), (unsigned)B);
    const size_t lds = (size_t)VC_WAVES * 3 * p.C * sizeof(float);
    const int nc = (p.C + 63) / 64;
    if (nc <= 1) vcb_ln_kernel<1><<<grid, VC_WAVES * 64, lds, s>>>(p);
    else if (nc <= 2) vcb_ln_kernel<2><<<grid, VC_WAVES * 64, lds, s>>>(p);
    else if (nc <= 4) vcb_ln_kernel<4><<<grid, VC_WAVES * 64, lds, s>>>(p);
    else vcb_ln_kernel<8><<<grid, VC_WAVES * 64, lds, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// the whole "filter + LayerNorm" backward up to its partials: dx [B][T][C] (row b at dx + b * dx_bs for taps 0), du: scratch [B][T][C]
int vcb_norm_backward(const float* x, const float* dy, const float* d_res, const int32_t* lens, int B, int T, int C, int taps, const float* w,
                      const float* b, const float* ln_w, float eps, float* du, float* dx, long dx_bs, float* part, hipStream_t s) {
    VcbNorm p{};
    p.x = x; p.dy = dy; p.d_res = taps ? nullptr : d_res; p.lens = lens; p.T = T; p.C = C; p.taps = taps;
    p.w = w; p.b = b; p.ln_w = ln_w; p.eps = eps; p.part = part;
    p.out = taps ? du : dx; p.out_bs = taps ? (long)T * C : dx_bs;
    if (const int rc = vcb_ln(p, B, s)) return rc;
    if (!taps) return GVX_OK;
    VcbFilter f{};
    f.x = x; f.du = du; f.d_res = d_res; f.dx = dx; f.lens = lens; f.T = T; f.C = C; f.w = w; f.part = part;
    vcb_dw_kernel<<<dim3((unsigned)vcb_pieces(T), (unsigned)B, (unsigned)((C + 63) / 64)), 64, 0, s>>>(f);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int vcb_sum(const float* part, int B, int T, int C, int taps, float* d_lnw, float* d_lnb, float* d_b, float* d_w, hipStream_t s) {
    const int n = (taps ? VCB_SUMS : 2) * C;
    vcb_sum_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(part, B * vcb_pieces(T), C, taps, d_lnw, d_lnb, d_b, d_w);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int vcb_gelu(const float* p, const float* dh, float* h, float* dp, long n, hipStream_t s) {
    const long n4 = n / 4;
    vcb_gelu_kernel<<<(unsigned)((n4 + 255) / 256), 256, 0, s>>>(reinterpret_cast<const float4*>(p), reinterpret_cast<const float4*>(dh),
                                                                 reinterpret_cast<float4*>(h), reinterpret_cast<float4*>(dp), n4);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int vcb_istft(const VcbIstft& a, const float* d_wav, float* dwe, int B, int N, hipStream_t s) {
    const long n_max = (long)a.T * a.hop;
    vcb_env_kernel<<<dim3((unsigned)((n_max + 255) / 256), (unsigned)B), 256, 0, s>>>(d_wav, a.lens, a.T, a.win, N, a.hop, a.center, dwe);
    HIP_TRY(hipGetLastError());
    const dim3 grid((unsigned)((a.T + VC_WAVES - 1) / VC_WAVES), (unsigned)B);
    switch (N) {
        case 512: vcb_istft_kernel<256><<<grid, VC_WAVES * 64, 0, s>>>(a); break;
        case 1024: vcb_istft_kernel<512><<<grid, VC_WAVES * 64, 0, s>>>(a); break;
        default: vcb_istft_kernel<1024><<<grid, VC_WAVES * 64, 0, s>>>(a); break;
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int vcb_transpose(const float* src, float* dst, int rows, int cols, int rows_p, hipStream_t s) {
    vcb_transpose_kernel<<<dim3((unsigned)((rows_p + 31) / 32), (unsigned)((cols + 31) / 32)), 256, 0, s>>>(src, dst, rows, cols, rows_p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// K pieces of a weight gradient [M][N] summed over K rows (train_internal.h's rule for the product's 64 x 128 tiles)
inline int vcb_split(int M, int N, long K) {
    return gvx::choose_splitk((long)((M + 63) / 64) * ((N + 127) / 128), (int)K);
}

// out [M][N] = sum_k A(k)[m] W(k)[n]: both operands as they lie in memory
int vcb_wgrad(const float* A, const RowMap& amap, int M, const float* W, const RowMap& wmap, int N, int K, float* out, float* scratch, hipStream_t s) {
    GemmParams g{};
    g.kmajor = true;
    g.A = A; g.amap = amap; g.W = W; g.wmap = wmap;
    g.C = out; g.cmap = RowMap{M, 0, (long)N};
    g.M = M; g.N = N; g.K = K; g.act = gvx::ACT_NONE;
    HIP_TRY(gvx::launch_gemm_splitk(g, vcb_split(M, N, K), scratch, s));
    return GVX_OK;
}

int vcb_colsum(const float* X, long rows, int C, float* out, hipStream_t s) {
    gvx::launch_col_reduce(X, nullptr, rows, C, out, nullptr, s);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// ---- the tape and the backward's workspace
inline int vcb_npad(const gvx_vocos_dims& d) { return (d.n_fft + 2 + 3) & ~3; }

// forward order: the haloed transposed mel, the embedding's output, x in front of the first block, per block its pre-GELU p and the x
// behind it, the head product.  A slot's rows are T, the first one's T + 6
struct VcbSlot { size_t off; int halo, C; };

std::vector<VcbSlot> vcb_tape_plan(const gvx_vocos_dims& d, int B, int T, size_t* total) {
    std::vector<VcbSlot> slots;
    size_t at = 0;
    auto take = [&](int halo, int C) {
        slots.push_back({at, halo, C});
        at += (size_t)B * (T + halo) * C;
    };
    take(6, vc_cpad(d));
    take(0, d.dim);
    take(0, d.dim);
    for (int i = 0; i < d.num_layers; ++i) { take(0, d.intermediate_dim); take(0, d.dim); }
    take(0, d.n_fft + 2);
    *total = at * sizeof(float);
    return slots;
}

struct VcbWs {
    size_t wht, w2t, w1t, wet, dwe, dco, a, h, dh, dx, da, du, deh, dmelt, parts, dw2f, db2f, tmp, tmpb, splitk, total;
    size_t part_floats;   // one LayerNorm's partials
};

VcbWs vcb_ws_plan(const gvx_vocos_dims& d, int B, int T) {
    VcbWs w{};
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t o = at; at += gvx::round256(floats * sizeof(float)); return o; };
    const size_t C = d.dim, I = d.intermediate_dim, L = d.num_layers, Np = vcb_npad(d), Cp = vc_cpad(d), rows = (size_t)B * T;
    w.wht = take(C * Np); w.w2t = take(L * I * C); w.w1t = take(L * C * I); w.wet = take(Cp * 7 * C);
    w.dwe = take(rows * d.hop_length); w.dco = take(rows * Np);
    w.a = take(rows * C); w.h = take(rows * I); w.dh = take(rows * I);
    w.dx = take(rows * C); w.da = take(rows * C); w.du = take(rows * C);
    w.deh = take((size_t)B * (T + 6) * C); w.dmelt = take(rows * Cp);
    w.part_floats = (size_t)B * vcb_pieces(T) * VCB_SUMS * C;
    w.parts = take((L + 2) * w.part_floats);
    w.dw2f = take(L * C * I); w.db2f = take(L * C);
    w.tmp = take(std::max(Np * C, C * 7 * Cp)); w.tmpb = take(Np);
    const long K = (long)rows;
    const size_t sk = std::max(std::max((size_t)vcb_split((int)Np, (int)C, K) * Np * C, (size_t)vcb_split((int)C, (int)I, K) * C * I),
                               std::max((size_t)vcb_split((int)I, (int)C, K) * I * C, (size_t)vcb_split((int)C, (int)(7 * Cp), K) * C * 7 * Cp));
    w.splitk = take(sk);
    w.total = at;
    return w;
}

inline const char* vcb_problem(const gvx_vocos_dims* d, int B, int T) {
    if (const char* why = vc_dims_problem(d)) return why;
    return vc_shape_problem(B, T);
}

}  // namespace

extern "C" {

// ---- the two kernels on their own
size_t gvx_dwconv_layernorm_backward_workspace_bytes(int B, int T, int C, int taps) {
    if (vc_shape_problem(B, T) || C < 4 || C > GVX_VOCOS_MAX_DIM || (C & 3) || (taps != 0 && taps != 7)) return 0;
    return gvx::round256((size_t)B * vcb_pieces(T) * VCB_SUMS * C * sizeof(float)) + (taps ? gvx::round256((size_t)B * T * C * sizeof(float)) : 0);
}

int gvx_dwconv_layernorm_backward(const float* x, const float* dy, const float* d_res, const int32_t* lens, int B, int T, int C, int taps,
                                  const float* w, const float* b, const float* ln_w, float eps, float* dx, float* d_w, float* d_b, float* d_ln_w,
                                  float* d_ln_b, void* workspace, size_t workspace_bytes, void* stream) {
    if (!x || !dy || !ln_w || !dx || !d_ln_w || !d_ln_b || dx == x || dx == dy) return fail(GVX_ERR_INVALID_ARG, "null argument, or dx is x or dy");
    if (taps != 0 && taps != 7) return fail(GVX_ERR_INVALID_ARG, "taps must be 7 or 0, not %d", taps);
    if (taps && (!w || !b || !d_w || !d_b)) return fail(GVX_ERR_INVALID_ARG, "taps = 7 needs the filter, its bias and their gradients' destinations");
    if (const char* why = vc_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (C < 4 || C > GVX_VOCOS_MAX_DIM || (C & 3)) return fail(GVX_ERR_INVALID_ARG, "C = %d must be a multiple of 4 in [4, %d]", C, (int)GVX_VOCOS_MAX_DIM);
    if (!(eps >= 0.f)) return fail(GVX_ERR_INVALID_ARG, "eps must be >= 0");
    if (const int rc = gen_check_workspace(workspace, workspace_bytes, gvx_dwconv_layernorm_backward_workspace_bytes(B, T, C, taps))) return rc;
    hipStream_t s = (hipStream_t)stream;
    float* part = static_cast<float*>(workspace);
    float* du = gvx::ws_ptr<float>(workspace, gvx::round256((size_t)B * vcb_pieces(T) * VCB_SUMS * C * sizeof(float)));
    if (const int rc = vcb_norm_backward(x, dy, d_res, lens, B, T, C, taps, w, b, ln_w, eps, du, dx, (long)T * C, part, s)) return rc;
    return vcb_sum(part, B, T, C, taps, d_ln_w, d_ln_b, d_b, d_w, s);
}

size_t gvx_istft_head_backward_workspace_bytes(int B, int T, int n_fft, int hop) {
    if (vc_shape_problem(B, T) || vc_fft_problem(n_fft, hop, 0)) return 0;
    return gvx::round256((size_t)B * T * hop * sizeof(float)) + gvx::round256((size_t)(n_fft + 1) * sizeof(float2));
}

int gvx_istft_head_backward(const float* coeffs, const float* d_wav, const int32_t* lens, int B, int T, int n_fft, int hop, int center,
                            const float* window, void* workspace, size_t workspace_bytes, float* d_coeffs, void* stream) {
    if (!coeffs || !d_wav || !window || !d_coeffs) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = vc_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (const char* why = vc_fft_problem(n_fft, hop, center)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if ((uintptr_t)window & 7) return fail(GVX_ERR_INVALID_ARG, "window must be 8-byte aligned");
    if (const int rc = gen_check_workspace(workspace, workspace_bytes, gvx_istft_head_backward_workspace_bytes(B, T, n_fft, hop))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int H = n_fft / 2;
    float* dwe = static_cast<float*>(workspace);
    float2* tw = gvx::ws_ptr<float2>(workspace, gvx::round256((size_t)B * T * hop * sizeof(float)));
    if (const int rc = vc_tables(nullptr, tw, tw + H, n_fft, s)) return rc;
    VcbIstft a{};
    a.coeffs = coeffs; a.dwe = dwe; a.lens = lens; a.T = T; a.hop = hop; a.center = center; a.ld = n_fft + 2;
    a.win = window; a.tw = tw; a.tw2 = tw + H; a.d_coeffs = d_coeffs;
    return vcb_istft(a, d_wav, dwe, B, n_fft, s);
}

// ---- the tape
size_t gvx_vocos_tape_bytes(const gvx_vocos_dims* dims, int B, int T) {
    if (vcb_problem(dims, B, T) || T < 1 + dims->center) return 0;
    size_t total;
    vcb_tape_plan(*dims, B, T, &total);
    return total;
}

int gvx_vocos_tape_layout(const gvx_vocos_dims* dims, int B, int T, gvx_vocos_tape_entry* entries, int max_entries) {
    if (vcb_problem(dims, B, T) || T < 1 + dims->center) return 0;
    size_t total;
    const std::vector<VcbSlot> slots = vcb_tape_plan(*dims, B, T, &total);
    const int n = (int)slots.size();
    for (int i = 0; entries && i < n && i < max_entries; ++i) {
        entries[i].byte_offset = slots[i].off * sizeof(float);
        entries[i].rows = T + slots[i].halo;
        entries[i].channels = slots[i].C;
    }
    return n;
}

size_t gvx_vocos_backward_workspace_bytes(const gvx_vocos_dims* dims, int B, int T) {
    if (vcb_problem(dims, B, T) || T < 1 + dims->center) return 0;
    return vcb_ws_plan(*dims, B, T).total;
}

int gvx_vocos_forward_train(gvx_vocos* h, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, void* tape, size_t tape_bytes,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !mel || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    const gvx_vocos_dims& d = h->d;
    if (const char* why = vc_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (T < 1 + d.center) return fail(GVX_ERR_INVALID_ARG, "T = %d: a row needs at least %d frames", T, 1 + d.center);
    size_t need;
    const std::vector<VcbSlot> slots = vcb_tape_plan(d, B, T, &need);
    const VcWs wp = vc_ws_plan(d, B, T);
    int rc;
    if ((rc = gen_check_tape(tape, tape_bytes, need)) != GVX_OK) return rc;
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const VcBlob L = vc_blob_layout(d);
    const float* blob = h->blob;
    const int C = d.dim, I = d.intermediate_dim, N = d.n_fft, Cp = vc_cpad(d), nl = d.num_layers;
    float* tp = static_cast<float*>(tape);
    float* a = gvx::ws_ptr<float>(workspace, wp.a);
    float* hid = gvx::ws_ptr<float>(workspace, wp.h);
    auto norm = [&](const float* src, float* dst, int taps, size_t w, size_t b, size_t ln_w, size_t ln_b) {
        VcNorm p{};
        p.x = src; p.out = dst; p.lens = frame_lengths; p.T = T; p.C = C; p.taps = taps;
        p.w = blob + w; p.b = blob + b; p.ln_w = blob + ln_w; p.ln_b = blob + ln_b; p.eps = VC_LN_EPS;
        return vc_norm(p, B, s);
    };
    const RowMap rows_c{T, (long)T * C, (long)C}, rows_i{T, (long)T * I, (long)I};

    float* mel_t = tp + slots[0].off;
    float* e = tp + slots[1].off;
    float* cur = tp + slots[2].off;
    if ((rc = vc_mel_transpose(mel, frame_lengths, B, d.n_mels, T, Cp, mel_t, s)) != GVX_OK) return rc;
    if ((rc = vc_gemm(mel_t, RowMap{T, (long)(T + 6) * Cp, (long)Cp}, 7 * Cp, blob + L.embed_w, blob + L.embed_b, e, C, B, T, frame_lengths,
                      gvx::ACT_NONE, nullptr, s)) != GVX_OK) return rc;
    if ((rc = norm(e, cur, 0, 0, 0, L.norm_w, L.norm_b)) != GVX_OK) return rc;
    for (int i = 0; i < nl; ++i) {
        const VcLayer& l = L.layer[i];
        float* p = tp + slots[3 + 2 * i].off;
        float* next = tp + slots[4 + 2 * i].off;
        if ((rc = norm(cur, a, 7, l.dw_w, l.dw_b, l.ln_w, l.ln_b)) != GVX_OK) return rc;
        // pwconv1 with its bias only into the tape, then gelu.h's function in a launch of its own: the bits of the fused epilogue
        if ((rc = vc_gemm(a, rows_c, C, blob + l.pw1_w, blob + l.pw1_b, p, I, B, T, frame_lengths, gvx::ACT_NONE, nullptr, s)) != GVX_OK) return rc;
        if ((rc = vcb_gelu(p, nullptr, hid, nullptr, (long)B * T * I, s)) != GVX_OK) return rc;
        if ((rc = vc_gemm(hid, rows_i, I, blob + l.pw2_w, blob + l.pw2_b, next, C, B, T, frame_lengths, gvx::ACT_NONE, cur, s)) != GVX_OK) return rc;
        cur = next;
    }
    float* coeffs = tp + slots[3 + 2 * nl].off;
    if ((rc = norm(cur, a, 0, 0, 0, L.fin_w, L.fin_b)) != GVX_OK) return rc;
    if ((rc = vc_gemm(a, rows_c, C, blob + L.head_w, blob + L.head_b, coeffs, N + 2, B, T, frame_lengths, gvx::ACT_NONE, nullptr, s)) != GVX_OK) return rc;
    VcIstft ia{};
    ia.coeffs = coeffs; ia.lens = frame_lengths; ia.T = T;
    ia.win = blob + L.window; ia.tw = reinterpret_cast<const float2*>(blob + L.tw); ia.tw2 = reinterpret_cast<const float2*>(blob + L.tw2);
    ia.frames = gvx::ws_ptr<float>(workspace, wp.frames);
    return vc_istft(ia, B, N, d.hop_length, d.center, wav_out, s);
}

int gvx_vocos_backward(gvx_vocos* h, const float* d_wav, const int32_t* frame_lengths, int B, int T, const void* tape, size_t tape_bytes,
                       const gvx_weight_desc* raw, int n_raw, const gvx_grad_desc* grads, int n_grads, float* d_mel_out, void* workspace,
                       size_t workspace_bytes, void* stream) {
    if (!h || !d_wav || !grads || n_grads < 1 || !raw || n_raw < 1) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    const gvx_vocos_dims& d = h->d;
    if (const char* why = vc_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (T < 1 + d.center) return fail(GVX_ERR_INVALID_ARG, "T = %d: a row needs at least %d frames", T, 1 + d.center);
    size_t need;
    const std::vector<VcbSlot> slots = vcb_tape_plan(d, B, T, &need);
    const VcbWs wp = vcb_ws_plan(d, B, T);
    int rc = GVX_OK;
    if ((rc = gen_check_tape(tape, tape_bytes, need)) != GVX_OK) return rc;
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    const int C = d.dim, I = d.intermediate_dim, N = d.n_fft, Cp = vc_cpad(d), Np = vcb_npad(d), nl = d.num_layers, M = d.n_mels;
    const long rows = (long)B * T;

    // every destination and every raw parameter, before anything is launched
    struct LayerGrads { float *dw_w, *dw_b, *ln_w, *ln_b, *pw1_w, *pw1_b, *pw2_w, *pw2_b, *gamma; const float *r_gamma, *r_w2, *r_b2; };
    std::vector<LayerGrads> lg(nl);
    auto grad = [&](const std::string& name, size_t numel) { return gen_grad(grads, n_grads, name, numel, rc); };
    float* g_embed_w = grad("backbone.embed.weight", (size_t)C * M * 7);
    float* g_embed_b = grad("backbone.embed.bias", C);
    float* g_norm_w = grad("backbone.norm.weight", C);
    float* g_norm_b = grad("backbone.norm.bias", C);
    GenLookup rawp{raw, n_raw};
    for (int i = 0; i < nl; ++i) {
        const std::string base = "backbone.convnext." + std::to_string(i) + ".";
        LayerGrads& g = lg[i];
        g.dw_w = grad(base + "dwconv.weight", (size_t)C * 7); g.dw_b = grad(base + "dwconv.bias", C);
        g.ln_w = grad(base + "norm.weight", C); g.ln_b = grad(base + "norm.bias", C);
        g.pw1_w = grad(base + "pwconv1.weight", (size_t)I * C); g.pw1_b = grad(base + "pwconv1.bias", I);
        g.pw2_w = grad(base + "pwconv2.weight", (size_t)C * I); g.pw2_b = grad(base + "pwconv2.bias", C);
        g.gamma = grad(base + "gamma", C);
        g.r_gamma = rawp.find(base + "gamma", C); g.r_w2 = rawp.find(base + "pwconv2.weight", (size_t)C * I); g.r_b2 = rawp.find(base + "pwconv2.bias", C);
    }
    float* g_fin_w = grad("backbone.final_layer_norm.weight", C);
    float* g_fin_b = grad("backbone.final_layer_norm.bias", C);
    float* g_head_w = grad("head.out.weight", (size_t)(N + 2) * C);
    float* g_head_b = grad("head.out.bias", N + 2);
    if (rc != GVX_OK) return rc;
    if (rawp.rc != GVX_OK) return rawp.rc;

    hipStream_t s = (hipStream_t)stream;
    const VcBlob L = vc_blob_layout(d);
    const float* blob = h->blob;
    const float* tp = static_cast<const float*>(tape);
    auto ws = [&](size_t off) { return gvx::ws_ptr<float>(workspace, off); };
    float *wht = ws(wp.wht), *w2t = ws(wp.w2t), *w1t = ws(wp.w1t), *wet = ws(wp.wet), *dwe = ws(wp.dwe), *dco = ws(wp.dco), *a = ws(wp.a), *hid = ws(wp.h),
          *dh = ws(wp.dh), *dx = ws(wp.dx), *da = ws(wp.da), *du = ws(wp.du), *deh = ws(wp.deh), *dmelt = ws(wp.dmelt), *parts = ws(wp.parts),
          *dw2f = ws(wp.dw2f), *db2f = ws(wp.db2f), *tmp = ws(wp.tmp), *tmpb = ws(wp.tmpb), *sk = ws(wp.splitk);
    int ev = 0;
    auto stamp = [&] { return gen_mark(h, ev++, s, &h->bwd_marks); };
    auto norm = [&](const float* src, float* dst, int taps, size_t w, size_t b, size_t ln_w, size_t ln_b) {
        VcNorm p{};
        p.x = src; p.out = dst; p.lens = frame_lengths; p.T = T; p.C = C; p.taps = taps;
        p.w = blob + w; p.b = blob + b; p.ln_w = blob + ln_w; p.ln_b = blob + ln_b; p.eps = VC_LN_EPS;
        return vc_norm(p, B, s);
    };
    const RowMap rows_c{T, (long)T * C, (long)C}, rows_i{T, (long)T * I, (long)I};
    const RowMap flat_c{(int)rows, 0, (long)C}, flat_i{(int)rows, 0, (long)I};
    const float* x_last = tp + slots[2 + 2 * nl].off;
    const float* coeffs = tp + slots[3 + 2 * nl].off;
    if ((rc = stamp()) != GVX_OK) return rc;

    // the transposed weights, from the blob that is bound now
    if ((rc = vcb_transpose(blob + L.head_w, wht, N + 2, C, Np, s)) != GVX_OK) return rc;
    for (int i = 0; i < nl; ++i) {
        if ((rc = vcb_transpose(blob + L.layer[i].pw2_w, w2t + (size_t)i * I * C, C, I, C, s)) != GVX_OK) return rc;
        if ((rc = vcb_transpose(blob + L.layer[i].pw1_w, w1t + (size_t)i * C * I, I, C, I, s)) != GVX_OK) return rc;
    }
    if (d_mel_out) {
        vcb_embed_t_kernel<<<(unsigned)((Cp * 7 * C + 255) / 256), 256, 0, s>>>(blob + L.embed_w, wet, C, Cp);
        HIP_TRY(hipGetLastError());
    }

    // ISTFT and head
    VcbIstft ia{};
    ia.coeffs = coeffs; ia.dwe = dwe; ia.lens = frame_lengths; ia.T = T; ia.hop = d.hop_length; ia.center = d.center; ia.ld = Np;
    ia.win = blob + L.window; ia.tw = reinterpret_cast<const float2*>(blob + L.tw); ia.tw2 = reinterpret_cast<const float2*>(blob + L.tw2);
    ia.d_coeffs = dco;
    if ((rc = vcb_istft(ia, d_wav, dwe, B, N, s)) != GVX_OK) return rc;
    if ((rc = norm(x_last, a, 0, 0, 0, L.fin_w, L.fin_b)) != GVX_OK) return rc;   // the head's input again, with the forward's bits
    if ((rc = vcb_wgrad(dco, RowMap{(int)rows, 0, (long)Np}, Np, a, flat_c, C, (int)rows, tmp, sk, s)) != GVX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(g_head_w, tmp, (size_t)(N + 2) * C * sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = vcb_colsum(dco, rows, Np, tmpb, s)) != GVX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(g_head_b, tmpb, (size_t)(N + 2) * sizeof(float), hipMemcpyDeviceToDevice, s));
    if ((rc = vc_gemm(dco, RowMap{T, (long)T * Np, (long)Np}, Np, wht, nullptr, da, C, B, T, frame_lengths, gvx::ACT_NONE, nullptr, s)) != GVX_OK) return rc;
    float* part = parts + (size_t)(nl + 1) * wp.part_floats;
    if ((rc = vcb_norm_backward(x_last, da, nullptr, frame_lengths, B, T, C, 0, nullptr, nullptr, blob + L.fin_w, VC_LN_EPS, du, dx, (long)T * C, part,
                                s)) != GVX_OK) return rc;
    if ((rc = stamp()) != GVX_OK) return rc;

    // the blocks, last to first: dx is the gradient at the block's output on entry and at its input on exit
    for (int i = nl - 1; i >= 0; --i) {
        const VcLayer& l = L.layer[i];
        const float* x_in = tp + slots[2 + 2 * i].off;
        const float* p = tp + slots[3 + 2 * i].off;
        if ((rc = vc_gemm(dx, rows_c, C, w2t + (size_t)i * I * C, nullptr, dh, I, B, T, frame_lengths, gvx::ACT_NONE, nullptr, s)) != GVX_OK) return rc;
        if ((rc = vcb_gelu(p, dh, hid, dh, rows * I, s)) != GVX_OK) return rc;   // h again and dp over dh
        if ((rc = vcb_wgrad(dx, flat_c, C, hid, flat_i, I, (int)rows, dw2f + (size_t)i * C * I, sk, s)) != GVX_OK) return rc;
        if ((rc = vcb_colsum(dx, rows, C, db2f + (size_t)i * C, s)) != GVX_OK) return rc;
        if ((rc = norm(x_in, a, 7, l.dw_w, l.dw_b, l.ln_w, l.ln_b)) != GVX_OK) return rc;   // pwconv1's input again
        if ((rc = vcb_wgrad(dh, flat_i, I, a, flat_c, C, (int)rows, lg[i].pw1_w, sk, s)) != GVX_OK) return rc;
        if ((rc = vcb_colsum(dh, rows, I, lg[i].pw1_b, s)) != GVX_OK) return rc;
        if ((rc = vc_gemm(dh, rows_i, I, w1t + (size_t)i * C * I, nullptr, da, C, B, T, frame_lengths, gvx::ACT_NONE, nullptr, s)) != GVX_OK) return rc;
        if ((rc = vcb_norm_backward(x_in, da, dx, frame_lengths, B, T, C, 7, blob + l.dw_w, blob + l.dw_b, blob + l.ln_w, VC_LN_EPS, du, dx, (long)T * C,
                                    parts + (size_t)(i + 1) * wp.part_floats, s)) != GVX_OK) return rc;
    }
    if ((rc = stamp()) != GVX_OK) return rc;

    // embed + norm: de into a buffer with a 3-frame zero halo, the A operand of the data gradient and of the weight gradient
    const float* e = tp + slots[1].off;
    const float* mel_t = tp + slots[0].off;
    HIP_TRY(hipMemsetAsync(deh, 0, (size_t)B * (T + 6) * C * sizeof(float), s));
    if ((rc = vcb_norm_backward(e, dx, nullptr, frame_lengths, B, T, C, 0, nullptr, nullptr, blob + L.norm_w, VC_LN_EPS, du, deh + 3 * C, (long)(T + 6) * C,
                                parts, s)) != GVX_OK) return rc;
    const RowMap halo_c{T, (long)(T + 6) * C, (long)C};
    if ((rc = vcb_wgrad(deh + 3 * C, halo_c, C, mel_t, RowMap{T, (long)(T + 6) * Cp, (long)Cp}, 7 * Cp, (int)rows, tmp, sk, s)) != GVX_OK) return rc;
    vcb_embed_grad_kernel<<<(unsigned)((C * M * 7 + 255) / 256), 256, 0, s>>>(tmp, g_embed_w, C, M, Cp);
    HIP_TRY(hipGetLastError());
    if ((rc = vcb_colsum(deh, (long)B * (T + 6), C, g_embed_b, s)) != GVX_OK) return rc;
    if (d_mel_out) {
        if ((rc = vc_gemm(deh, halo_c, 7 * C, wet, nullptr, dmelt, Cp, B, T, frame_lengths, gvx::ACT_NONE, nullptr, s)) != GVX_OK) return rc;
        gen_dmel_kernel<1><<<dim3((unsigned)(((long)M * T + 255) / 256), (unsigned)B), 256, 0, s>>>(dmelt, frame_lengths, M, T, Cp, d_mel_out);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = stamp()) != GVX_OK) return rc;

    // the pieces' sums and the unfold
    if ((rc = vcb_sum(parts, B, T, C, 0, g_norm_w, g_norm_b, nullptr, nullptr, s)) != GVX_OK) return rc;
    if ((rc = vcb_sum(parts + (size_t)(nl + 1) * wp.part_floats, B, T, C, 0, g_fin_w, g_fin_b, nullptr, nullptr, s)) != GVX_OK) return rc;
    for (int i = 0; i < nl; ++i) {
        const LayerGrads& g = lg[i];
        if ((rc = vcb_sum(parts + (size_t)(i + 1) * wp.part_floats, B, T, C, 7, g.ln_w, g.ln_b, g.dw_b, g.dw_w, s)) != GVX_OK) return rc;
        vcb_unfold_kernel<<<(unsigned)C, 256, 0, s>>>(dw2f + (size_t)i * C * I, db2f + (size_t)i * C, g.r_gamma, g.r_w2, g.r_b2, I, g.pw2_w, g.pw2_b, g.gamma);
        HIP_TRY(hipGetLastError());
    }
    return stamp();
}

int gvx_vocos_backward_stage_times_ms(gvx_vocos* h, float* ms_out, int* n_out) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    return gen_stage_times_ms(h, 4, ms_out, n_out, &h->bwd_marks);
}

}  // C ABI
