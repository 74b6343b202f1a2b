// Vocos generator inference: mel [B][n_mels][T] -> waveform [B][T * hop].  The model is defined in include/genvox_amd.h ("Vocos
// generator"); the float64 restatement the tests hold this file to is tests/vocos_ref64.py.
//
// A ConvNeXt backbone at the frame rate and an inverse STFT.  Every product - the embedding as an implicit k = 7 GEMM over a 3-frame
// zero halo, the two Linear layers of every block, the head - is launch_gemm (gemm_f32.hip): bias + GELU and bias + residual are its
// compile-time epilogue kinds EPI_GELU and EPI_RES, row_len writes the zeros behind a row.  What is new here:
//
//   vc_dwconv_ln_kernel<NC>  "k = 7 channel-wise filter, then LayerNorm" as ONE launch that writes the A operand of pwconv1.  A workgroup
//                            of four waves owns VC_P = 16 frames of one row; the tile's P + 6 input frames go into LDS once (zeros
//                            outside the row: the load tests the row's own length), then a wave owns one frame at a time, lanes along
//                            the channels (lane l: channels l, l + 64, ..: every global and LDS access of a wave is a run of consecutive
//                            floats), seven taps and the bias per channel in registers, and mean and variance as two passes over those
//                            registers - the mean (and the mean of what is left, an ulp of it), then the squared deviations - each a
//                            butterfly over the wave.  taps = 0 skips the filter and the LDS: the plain LayerNorm behind the embedding
//                            and in front of the head.
//   vc_istft_kernel<H>       a frame per wave: exp, the clamp, sincosf and the product in registers, irfft_pack into the H-point complex
//                            transform, the inverse transform in LDS (fft_lds.h), 1 / N and the window; the frame goes to the workspace.
//   vc_ola_kernel            the overlap-add as a gather: a thread per output sample sums the row's frames that cover it and the squared
//                            window under them in ascending frame order, divides, applies the trim of the padding mode and writes zeros
//                            behind the row's samples.
// No atomics anywhere.  Frames at and behind a row's length are written as zeros by every launch and never read by one.
//
// Order of this file: kernels and their launches, dims / blob / workspace layouts (what vocos_train.hip shares is declared in
// vocos_internal.h), the C ABI.
#include "fft_lds.h"
#include "vocos_internal.h"

#include <algorithm>

using namespace gvx_gen;
using namespace gvx_vc;
using gvx::GemmParams;
using gvx::RowMap;

namespace {

// mel [B][M][T] -> out [B][T + 6][Cp]: frame t at row t + 3, zeros in the halo rows, at and behind the row's length and in the
// channel padding.  32 x 32 tiles through LDS: reads run along t, writes along c
__global__ void __launch_bounds__(256) vc_mel_transpose_kernel(const float* __restrict__ mel, const int32_t* __restrict__ lens, int M, int T, int Cp,
                                                               float* __restrict__ out) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, r0 = (int)blockIdx.x * 32, c0 = (int)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int len = gen_frames(lens, b, T);
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, t = r0 + tx - 3;
        tile[i][tx] = (c < M && t >= 0 && t < len) ? mel[((size_t)b * M + c) * T + t] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        if (r < T + 6 && c < Cp) out[((size_t)b * (T + 6) + r) * Cp + c] = tile[tx][i];
    }
}

template <int NC>   // channels per lane: C <= 64 NC
__global__ void __launch_bounds__(VC_WAVES * 64) vc_dwconv_ln_kernel(const VcNorm p) {
    extern __shared__ __attribute__((aligned(16))) float xs[];   // taps: [VC_P + 6][C], x[t0 - 3 .. t0 + P + 2]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t0 = (int)blockIdx.x * VC_P, C = p.C;
    const int len = gen_frames(p.lens, b, p.T);
    const size_t row = (size_t)b * p.T;
    const int t_end = min(t0 + VC_P, p.T);
    const bool filter = p.taps != 0;
    if (filter && t0 < len) {   // (uniform over the workgroup)
        const int n4 = (VC_P + 6) * C / 4;
        for (int i = tid; i < n4; i += VC_WAVES * 64) {
            const int e = 4 * i, fr = e / C, c = e - fr * C, t = t0 - 3 + fr;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t >= 0 && t < len) v = *reinterpret_cast<const float4*>(p.x + (row + t) * C + c);
            *reinterpret_cast<float4*>(xs + e) = v;
        }
        __syncthreads();
    }
    float lw[NC], lb[NC], cb[NC], cw[7][NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        const bool ok = c < C;
        lw[i] = ok ? p.ln_w[c] : 0.f;
        lb[i] = ok ? p.ln_b[c] : 0.f;
        cb[i] = ok && filter ? p.b[c] : 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) cw[j][i] = ok && filter ? p.w[j * C + c] : 0.f;
    }
    const float c_f = (float)C;
    for (int tt = wave; t0 + tt < t_end; tt += VC_WAVES) {
        const int t = t0 + tt;
        float* o = p.out + (row + t) * C;
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
                    for (int j = 0; j < 7; ++j) a = fmaf(xs[(tt + j) * C + c], cw[j][i], a);
                } else {
                    a = p.x[(row + t) * C + c];
                }
            }
            v[i] = a;
            sum += a;
        }
        // two passes over the registers, the first one twice: the deviations from the rounded mean have a mean of their own - an ulp of
        // the mean, which under an offset of 1e3 is 1e-4 of a unit deviation - and it is taken off before the squares are summed
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
#pragma unroll
        for (int i = 0; i < NC; ++i)
            if (lane + 64 * i < C) o[lane + 64 * i] = fmaf(v[i] * rstd, lw[i], lb[i]);
    }
}

}  // namespace

int gvx_vc::vc_norm(const VcNorm& p, int B, hipStream_t s) {
    const dim3 grid((unsigned)((p.T + VC_P - 1) / VC_P), (unsigned)B);
    const size_t lds = p.taps ? (size_t)(VC_P + 6) * p.C * sizeof(float) : 0;
    const int nc = (p.C + 63) / 64;
    if (nc <= 1) vc_dwconv_ln_kernel<1><<<grid, VC_WAVES * 64, lds, s>>>(p);
    else if (nc <= 2) vc_dwconv_ln_kernel<2><<<grid, VC_WAVES * 64, lds, s>>>(p);
    else if (nc <= 4) vc_dwconv_ln_kernel<4><<<grid, VC_WAVES * 64, lds, s>>>(p);
    else vc_dwconv_ln_kernel<8><<<grid, VC_WAVES * 64, lds, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

namespace {

// window [N] (if asked for), w_H^m [H] and w_N^k [H + 1], in float64
__global__ void vc_tables_kernel(float* win, float2* tw, float2* tw2, int N) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x, H = N / 2;
    if (win && i < N) win[i] = (float)(0.5 - 0.5 * cospi(2.0 * (double)i / (double)N));
    double sn, cs;
    if (i < H) { sincospi(2.0 * (double)i / (double)H, &sn, &cs); tw[i] = make_float2((float)cs, (float)-sn); }
    if (i <= H) { sincospi(2.0 * (double)i / (double)N, &sn, &cs); tw2[i] = make_float2((float)cs, (float)-sn); }
}

template <int H>
__global__ void __launch_bounds__(VC_WAVES * 64) vc_istft_kernel(const VcIstft p) {
    constexpr int Q = H / 64, N = 2 * H;
    __shared__ __attribute__((aligned(16))) float2 fsm[VC_WAVES * fft_lds_words<H>()];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t = (int)blockIdx.x * VC_WAVES + wave;
    if (t >= gen_frames(p.lens, b, p.T)) return;   // behind the row's frames: the gather reads no such frame
    const long f = (long)b * p.T + t;
    const float* c = p.coeffs + f * (N + 2);
    float2* buf = fsm + wave * fft_lds_words<H>();
    float2 ys[Q + 1];
#pragma unroll
    for (int q = 0; q <= Q; ++q) {
        const int k = j + 64 * q;
        if (k <= H) {
            const float mag = fminf(expf(c[k]), VC_MAG_MAX);
            float sn, cs;
            sincosf(c[H + 1 + k], &sn, &cs);
            ys[q] = make_float2(mag * cs, mag * sn);
            buf[k] = ys[q];   // S_k and S_{H-k} meet through this wave's LDS row, unpadded at [k], k = 0 .. H
        }
    }
    wave_lds_fence();
    float2 z[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int k = j + 64 * q;
        z[q] = irfft_pack(ys[q], buf[H - k], p.tw2[k], k == 0);   // at k = 0 the partner is the Nyquist bin
    }
    wave_lds_fence();
#pragma unroll
    for (int q = 0; q < Q; ++q) buf[fpad(j + 64 * q)] = z[q];
    wave_lds_fence();
    fft_lds_wave<H, true>(buf, p.tw, j);
    float* g = p.frames + f * N;
    const float inv_n = 1.f / (float)N;   // a power of two: exact
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int m = j + 64 * q;
        const float2 v = buf[fpad(m)];
        const float2 w = *reinterpret_cast<const float2*>(p.win + 2 * m);
        *reinterpret_cast<float2*>(g + 2 * m) = make_float2(w.x * (v.x * inv_n), w.y * (v.y * inv_n));
    }
}

// out[b][i] for i < T * hop: sample i of a row lies at position p = i + pad of the untrimmed overlap-add
__global__ void __launch_bounds__(256) vc_ola_kernel(const int32_t* __restrict__ lens, int T, const float* __restrict__ frames,
                                                     const float* __restrict__ win, int N, int hop, int center, float* __restrict__ out) {
    const long i_long = (long)blockIdx.x * 256 + threadIdx.x;
    const long n_max = (long)T * hop;
    const int b = blockIdx.y;
    if (i_long >= n_max) return;
    const int i = (int)i_long;
    const int len = gen_frames(lens, b, T);
    const int nb = center ? (len - 1) * hop : len * hop;   // (len = 0 or 1 under "center": nothing)
    float r = 0.f;
    if (i < nb) {
        const float* g = frames + (long)b * T * N;
        const int p = i + (center ? N / 2 : (N - hop) / 2);
        const int t_lo = p >= N ? (p - N) / hop + 1 : 0;
        const int t_hi = min(len - 1, p / hop);
        float num = 0.f, den = 0.f;
        for (int t = t_lo; t <= t_hi; ++t) {
            const int o = p - t * hop;
            const float w = win[o];
            num += g[(long)t * N + o];
            den += w * w;
        }
        r = num / den;
    }
    out[(long)b * n_max + i] = r;
}

}  // namespace

namespace gvx_vc {

int vc_tables(float* win, float2* tw, float2* tw2, int N, hipStream_t s) {
    vc_tables_kernel<<<(unsigned)(N / 256 + 1), 256, 0, s>>>(win, tw, tw2, N);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int vc_mel_transpose(const float* mel, const int32_t* lens, int B, int M, int T, int Cp, float* out, hipStream_t s) {
    vc_mel_transpose_kernel<<<dim3((unsigned)((T + 6 + 31) / 32), (unsigned)((Cp + 31) / 32), (unsigned)B), 256, 0, s>>>(mel, lens, M, T, Cp, out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int vc_istft(const VcIstft& a, int B, int N, int hop, int center, float* wav, hipStream_t s) {
    const dim3 grid((unsigned)((a.T + VC_WAVES - 1) / VC_WAVES), (unsigned)B);
    switch (N) {
        case 512: vc_istft_kernel<256><<<grid, VC_WAVES * 64, 0, s>>>(a); break;
        case 1024: vc_istft_kernel<512><<<grid, VC_WAVES * 64, 0, s>>>(a); break;
        default: vc_istft_kernel<1024><<<grid, VC_WAVES * 64, 0, s>>>(a); break;
    }
    HIP_TRY(hipGetLastError());
    const long n_max = (long)a.T * hop;
    vc_ola_kernel<<<dim3((unsigned)((n_max + 255) / 256), (unsigned)B), 256, 0, s>>>(a.lens, a.T, a.frames, a.win, N, hop, center, wav);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// ---- dims, blob, workspace
const char* vc_fft_problem(int n_fft, int hop, int center) {
    if (n_fft != 512 && n_fft != 1024 && n_fft != 2048) return "n_fft must be 512, 1024 or 2048";
    if (hop < n_fft / 8 || hop > n_fft / 2) return "hop_length must be in [n_fft / 8, n_fft / 2]";
    if ((n_fft - hop) & 1) return "n_fft - hop_length must be even";
    if (center != 0 && center != 1) return "center must be 0 or 1";
    return nullptr;
}

const char* vc_dims_problem(const gvx_vocos_dims* d) {
    if (!d) return "null dims";
    if (d->n_mels < 1 || d->n_mels > 4096) return "n_mels must be in [1, 4096]";
    if (d->dim < 32 || d->dim > GVX_VOCOS_MAX_DIM || d->dim % 32) return "dim must be a multiple of 32 in [32, GVX_VOCOS_MAX_DIM]";
    if (d->intermediate_dim < 32 || d->intermediate_dim > GVX_VOCOS_MAX_INTERMEDIATE || d->intermediate_dim % 32)
        return "intermediate_dim must be a multiple of 32 in [32, GVX_VOCOS_MAX_INTERMEDIATE]";
    if (d->num_layers < 1 || d->num_layers > GVX_VOCOS_MAX_LAYERS) return "num_layers must be in [1, GVX_VOCOS_MAX_LAYERS]";
    return vc_fft_problem(d->n_fft, d->hop_length, d->center);
}

VcBlob vc_blob_layout(const gvx_vocos_dims& d) {
    VcBlob L{};
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t o = at; at += gvx::round64(floats); return o; };
    const size_t C = d.dim, I = d.intermediate_dim, N = d.n_fft;
    L.embed_w = take(C * 7 * vc_cpad(d)); L.embed_b = take(C); L.norm_w = take(C); L.norm_b = take(C);
    for (int i = 0; i < d.num_layers; ++i) {
        VcLayer& l = L.layer[i];
        l.dw_w = take(7 * C); l.dw_b = take(C); l.ln_w = take(C); l.ln_b = take(C);
        l.pw1_w = take(I * C); l.pw1_b = take(I); l.pw2_w = take(C * I); l.pw2_b = take(C);
    }
    L.fin_w = take(C); L.fin_b = take(C); L.head_w = take((N + 2) * C); L.head_b = take(N + 2);
    L.window = take(N); L.tw = take(N); L.tw2 = take(N + 2);
    L.total = at;
    return L;
}

VcWs vc_ws_plan(const gvx_vocos_dims& d, int B, int T) {
    VcWs w{};
    GenRows ws{B};
    w.mel_t = ws.rows((size_t)(T + 6) * vc_cpad(d));
    w.x = ws.rows((size_t)T * d.dim);
    w.a = ws.rows((size_t)T * d.dim);
    w.h = ws.rows((size_t)T * d.intermediate_dim);
    w.coeffs = ws.rows((size_t)T * (d.n_fft + 2));
    w.frames = ws.rows((size_t)T * d.n_fft);
    w.total = ws.total;
    return w;
}

const char* vc_shape_problem(int B, int T) {
    if (B < 1 || B > 65535) return "B must be in [1, 65535]";
    if (T < 1 || T > GVX_VOCOS_MAX_FRAMES) return "T must be in [1, GVX_VOCOS_MAX_FRAMES]";
    if ((long)B * T > (1L << 26)) return "B * T is beyond 2^26 frames";
    return nullptr;
}

// C [B][T][N] = epilogue(A W^T + bias): rows grouped by T for row_len
int vc_gemm(const float* A, const RowMap& amap, int K, const float* W, const float* bias, float* out, int N, int B, int T, const int32_t* lens,
            int act, const float* res, hipStream_t s) {
    GemmParams g{};
    g.A = A; g.amap = amap; g.W = W; g.ldw = K;
    g.C = out; g.cmap = RowMap{T, (long)T * N, (long)N};
    g.bias = bias; g.keep = nullptr; g.keep_ld = 0;
    g.M = B * T; g.N = N; g.K = K;
    g.act = act; g.row_len = lens; g.res = res;
    HIP_TRY(gvx::launch_gemm(g, s));
    return GVX_OK;
}

}  // namespace gvx_vc

extern "C" {

int gvx_dwconv_layernorm(const float* x, const int32_t* lens, int B, int T, int C, int taps, const float* w, const float* b, const float* ln_w,
                         const float* ln_b, float eps, float* out, void* stream) {
    if (!x || !ln_w || !ln_b || !out || x == out) return fail(GVX_ERR_INVALID_ARG, "null argument, or out is x");
    if (taps != 0 && taps != 7) return fail(GVX_ERR_INVALID_ARG, "taps must be 7 or 0, not %d", taps);
    if (taps && (!w || !b)) return fail(GVX_ERR_INVALID_ARG, "taps = 7 needs the filter and its bias");
    if (const char* why = vc_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (C < 4 || C > GVX_VOCOS_MAX_DIM || (C & 3)) return fail(GVX_ERR_INVALID_ARG, "C = %d must be a multiple of 4 in [4, %d]", C, (int)GVX_VOCOS_MAX_DIM);
    if (((uintptr_t)x | (uintptr_t)out) & 15) return fail(GVX_ERR_INVALID_ARG, "x and out must be 16-byte aligned");
    if (!(eps >= 0.f)) return fail(GVX_ERR_INVALID_ARG, "eps must be >= 0");
    VcNorm p{};
    p.x = x; p.out = out; p.lens = lens; p.T = T; p.C = C; p.taps = taps; p.w = w; p.b = b; p.ln_w = ln_w; p.ln_b = ln_b; p.eps = eps;
    return vc_norm(p, B, (hipStream_t)stream);
}

size_t gvx_istft_head_workspace_bytes(int B, int T, int n_fft) {
    if (vc_shape_problem(B, T) || vc_fft_problem(n_fft, n_fft / 2, 0)) return 0;
    return gvx::round256((size_t)B * T * n_fft * sizeof(float)) + gvx::round256((size_t)(n_fft + 1) * sizeof(float2));
}

int gvx_istft_head(const float* coeffs, const int32_t* lens, int B, int T, int n_fft, int hop, int center, const float* window, void* workspace,
                   float* wav_out, void* stream) {
    if (!coeffs || !window || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = vc_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (const char* why = vc_fft_problem(n_fft, hop, center)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!workspace || (uintptr_t)workspace % 256) return fail(GVX_ERR_WORKSPACE, "the workspace is missing or not 256-byte aligned");
    if ((uintptr_t)window & 7) return fail(GVX_ERR_INVALID_ARG, "window must be 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int H = n_fft / 2;
    VcIstft a{};
    a.coeffs = coeffs; a.lens = lens; a.T = T; a.win = window;
    a.frames = static_cast<float*>(workspace);
    float2* tw = gvx::ws_ptr<float2>(workspace, gvx::round256((size_t)B * T * n_fft * sizeof(float)));
    a.tw = tw; a.tw2 = tw + H;
    vc_tables_kernel<<<(unsigned)(n_fft / 256 + 1), 256, 0, s>>>(nullptr, tw, tw + H, n_fft);
    HIP_TRY(hipGetLastError());
    return vc_istft(a, B, n_fft, hop, center, wav_out, s);
}

size_t gvx_vocos_blob_floats(const gvx_vocos_dims* dims) {
    if (vc_dims_problem(dims)) return 0;
    return vc_blob_layout(*dims).total;
}

size_t gvx_vocos_workspace_bytes(const gvx_vocos_dims* dims, int B, int T) {
    if (vc_dims_problem(dims) || vc_shape_problem(B, T)) return 0;
    return vc_ws_plan(*dims, B, T).total;
}

int gvx_vocos_pack_weights_device(const gvx_vocos_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = vc_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_vocos_dims& d = *dims;
    const VcBlob L = vc_blob_layout(d);
    hipStream_t s = (hipStream_t)stream;
    GenPacker P{{table, n}};
    const size_t C = d.dim, I = d.intermediate_dim, N = d.n_fft;
    P.take("embed.weight", L.embed_w, C * 7 * vc_cpad(d));
    P.take("embed.bias", L.embed_b, C);
    P.take("norm.weight", L.norm_w, C);
    P.take("norm.bias", L.norm_b, C);
    for (int i = 0; i < d.num_layers; ++i) {
        const std::string base = "convnext." + std::to_string(i) + ".";
        const VcLayer& l = L.layer[i];
        const struct { const char* name; size_t dst, numel; } parts[] = {
            {"dwconv.weight", l.dw_w, 7 * C}, {"dwconv.bias", l.dw_b, C}, {"norm.weight", l.ln_w, C}, {"norm.bias", l.ln_b, C},
            {"pwconv1.weight", l.pw1_w, I * C}, {"pwconv1.bias", l.pw1_b, I}, {"pwconv2.weight", l.pw2_w, C * I}, {"pwconv2.bias", l.pw2_b, C}};
        for (const auto& part : parts) P.take(base + part.name, part.dst, part.numel);
    }
    P.take("final_layer_norm.weight", L.fin_w, C);
    P.take("final_layer_norm.bias", L.fin_b, C);
    P.take("head.weight", L.head_w, (N + 2) * C);
    P.take("head.bias", L.head_b, N + 2);
    if (const int rc = P.run(device_blob, 0, L.total, s)) return rc;
    vc_tables_kernel<<<(unsigned)(d.n_fft / 256 + 1), 256, 0, s>>>(device_blob + L.window, reinterpret_cast<float2*>(device_blob + L.tw),
                                                                   reinterpret_cast<float2*>(device_blob + L.tw2), d.n_fft);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int gvx_vocos_create(const gvx_vocos_dims* dims, gvx_vocos** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = vc_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_vocos* h = new gvx_vocos();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_vocos_destroy(gvx_vocos* h) { delete h; }

int gvx_vocos_bind(gvx_vocos* h, const float* device_blob) {
    if (const int rc = gen_bind(h, device_blob)) return rc;
    HIP_TRY(gvx::gemm_init());   // the big tiles' dynamic LDS
    return GVX_OK;
}

int gvx_vocos_timing_enable(gvx_vocos* h, int enable) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (enable)
        if (const int rc = gen_make_marks(h->bwd_marks, 5)) return rc;
    return gen_timing_enable(h, enable, 5);
}

int gvx_vocos_stage_times_ms(gvx_vocos* h, float* ms_out, int* n_out) { return gen_stage_times_ms(h, 4, ms_out, n_out); }

int gvx_vocos_forward(gvx_vocos* h, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, float* const* stage_out,
                      void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !mel || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    const gvx_vocos_dims& d = h->d;
    if (const char* why = vc_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (T < 1 + d.center) return fail(GVX_ERR_INVALID_ARG, "T = %d: a row needs at least %d frames", T, 1 + d.center);
    const VcWs wp = vc_ws_plan(d, B, T);
    const int n_stage = d.num_layers + 3;
    int ev = 0, rc;
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    if ((rc = gen_check_stage_out(stage_out, n_stage)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const VcBlob L = vc_blob_layout(d);
    const float* blob = h->blob;
    const int C = d.dim, I = d.intermediate_dim, N = d.n_fft, Cp = vc_cpad(d);
    float* mel_t = gvx::ws_ptr<float>(workspace, wp.mel_t);
    float* x = gvx::ws_ptr<float>(workspace, wp.x);
    float* a = gvx::ws_ptr<float>(workspace, wp.a);
    float* hid = gvx::ws_ptr<float>(workspace, wp.h);
    float* coeffs = stage_out ? stage_out[n_stage - 1] : gvx::ws_ptr<float>(workspace, wp.coeffs);
    auto stamp = [&] { return gen_mark(h, ev++, s); };
    auto norm = [&](const float* src, float* dst, int taps, size_t w, size_t b, size_t ln_w, size_t ln_b) {
        VcNorm p{};
        p.x = src; p.out = dst; p.lens = frame_lengths; p.T = T; p.C = C; p.taps = taps;
        p.w = blob + w; p.b = blob + b; p.ln_w = blob + ln_w; p.ln_b = blob + ln_b; p.eps = VC_LN_EPS;
        return vc_norm(p, B, s);
    };
    const RowMap rows_c{T, (long)T * C, (long)C}, rows_i{T, (long)T * I, (long)I};
    if ((rc = stamp()) != GVX_OK) return rc;

    // embed: the im2col row of (b, t) is the 7 Cp floats from row t of the halo-padded mel
    vc_mel_transpose_kernel<<<dim3((unsigned)((T + 6 + 31) / 32), (unsigned)((Cp + 31) / 32), (unsigned)B), 256, 0, s>>>(mel, frame_lengths, d.n_mels, T,
                                                                                                                          Cp, mel_t);
    HIP_TRY(hipGetLastError());
    if ((rc = vc_gemm(mel_t, RowMap{T, (long)(T + 6) * Cp, (long)Cp}, 7 * Cp, blob + L.embed_w, blob + L.embed_b, a, C, B, T, frame_lengths,
                      gvx::ACT_NONE, nullptr, s)) != GVX_OK) return rc;
    float* cur = stage_out ? stage_out[0] : x;
    if ((rc = norm(a, cur, 0, 0, 0, L.norm_w, L.norm_b)) != GVX_OK) return rc;
    if ((rc = stamp()) != GVX_OK) return rc;

    for (int i = 0; i < d.num_layers; ++i) {
        const VcLayer& l = L.layer[i];
        float* next = stage_out ? stage_out[i + 1] : cur;   // in place without stage outputs: an element is read and written by one lane
        if ((rc = norm(cur, a, 7, l.dw_w, l.dw_b, l.ln_w, l.ln_b)) != GVX_OK) return rc;
        if ((rc = vc_gemm(a, rows_c, C, blob + l.pw1_w, blob + l.pw1_b, hid, I, B, T, frame_lengths, gvx::ACT_GELU, nullptr, s)) != GVX_OK) return rc;
        if ((rc = vc_gemm(hid, rows_i, I, blob + l.pw2_w, blob + l.pw2_b, next, C, B, T, frame_lengths, gvx::ACT_NONE, cur, s)) != GVX_OK) return rc;
        cur = next;
    }
    if ((rc = stamp()) != GVX_OK) return rc;

    float* fin = stage_out ? stage_out[d.num_layers + 1] : a;
    if ((rc = norm(cur, fin, 0, 0, 0, L.fin_w, L.fin_b)) != GVX_OK) return rc;
    if ((rc = vc_gemm(fin, rows_c, C, blob + L.head_w, blob + L.head_b, coeffs, N + 2, B, T, frame_lengths, gvx::ACT_NONE, nullptr, s)) != GVX_OK) return rc;
    if ((rc = stamp()) != GVX_OK) return rc;

    VcIstft ia{};
    ia.coeffs = coeffs; ia.lens = frame_lengths; ia.T = T;
    ia.win = blob + L.window; ia.tw = reinterpret_cast<const float2*>(blob + L.tw); ia.tw2 = reinterpret_cast<const float2*>(blob + L.tw2);
    ia.frames = gvx::ws_ptr<float>(workspace, wp.frames);
    if ((rc = vc_istft(ia, B, N, d.hop_length, d.center, wav_out, s)) != GVX_OK) return rc;
    return stamp();
}

}  // C ABI
