// FastPitch inference: tokens [B][L] -> mel [B][n_mels][T].  The model is defined in include/genvox_amd.h ("FastPitch acoustic model");
// the float64 restatement the tests hold this file to is tests/fastpitch_ref64.py.
//
// Two FFT stacks (self-attention + a two-convolution feed-forward, post-LayerNorm), three small convolutional predictors and a length
// regulator between the stacks.  Every product - qkv, o_net, both convolutions of a layer as implicit GEMMs over haloed rows, the
// predictors' convolutions, fc, proj - is launch_gemm (gemm_f32.hip) with what it already has.  What is new here:
//
//   fp_attention_kernel<D>   masked multi-head self-attention on v_mfma_f32_32x32x2_f32.  A workgroup of four waves owns 128 queries of one
//                            (row, head), a wave 32 of them; key / value tiles of 64 positions go through LDS (zeros at and behind the
//                            row's length), the next tile's loads in flight while the current one is multiplied.  The wave forms the
//                            TRANSPOSED products S^T = K Q^T and O^T = V^T P^T: a query is then a lane's column in both accumulators, so the
//                            running maximum, the running sum and the rescale of the online softmax are the lane's own (one cross-lane
//                            move per tile joins the two half-waves), and P goes from the first product's accumulator into the second
//                            product's B operand without leaving its registers.
//   fp_add_ln_kernel<NC>     x (+ y), then LayerNorm, vc_dwconv_ln_kernel's body (vocos.hip) with a second input: a wave per position,
//                            lanes along the channels, the mean, the mean of what is left and the squared deviations as butterflies.  It
//                            writes the haloed layout [B][N + 2][C] the implicit GEMM reads, zero halo rows included.
//   fp_embed_kernel, fp_cond_add_kernel, fp_plan_kernel, fp_regulate_kernel, fp_to_channels_first_kernel: the gathers around them.
// No atomics anywhere.  Positions at and behind a row's length are written as zeros by every launch and never read by one.
//
// Order of this file: kernels, dims / blob / workspace layouts, the C ABI.
#include "gen_host.h"

#include <algorithm>

using namespace gvx_gen;
using gvx::GemmParams;
using gvx::RowMap;

namespace gvx { hipError_t gemm_init(); }

struct gvx_fastpitch : GenHandle {
    gvx_fastpitch_dims d;
    bool encoded = false, decoded = false;   // which marks have been recorded since timing was enabled
};

namespace {

typedef __attribute__((ext_vector_type(16))) float fp_f32x16;

constexpr int FP_WAVES = 4;
constexpr int FP_P = GVX_ADD_LN_POSITIONS;             // positions per workgroup of the LayerNorm kernel
constexpr float FP_LN_EPS = 1e-5f;
constexpr int FP_BQ = GVX_ATTN_Q_TILE, FP_BK = GVX_ATTN_K_TILE;

__device__ __forceinline__ int fp_len(const int32_t* lens, int b, int N) {
    int v = lens ? lens[b] : N;
    v = v > N ? N : v;
    return v < 0 ? 0 : v;
}

__device__ __forceinline__ float fp_wave_sum(float v) {   // a butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// ---- self-attention: qkv [B][T][3 H D] -> out [B][T][H D]
template <int D>
__global__ void __launch_bounds__(FP_WAVES * 64) fp_attention_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ lens, int T, int H,
                                                                      float scale, float* __restrict__ out) {
    constexpr int KG = D / 8, JD = D / 32, KLD = D + 4;     // k-groups of a score, 32-column blocks of the output, the K tile's row stride
    constexpr int NL = FP_BK * D / 4 / (FP_WAVES * 64);     // float4 per thread and tile of K (and of V)
    __shared__ __attribute__((aligned(16))) float Ks[FP_BK * KLD];
    __shared__ __attribute__((aligned(16))) float Vs[FP_BK * D];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.z, head = blockIdx.y, q0 = (int)blockIdx.x * FP_BQ;
    const int len = fp_len(lens, b, T);
    const int HD = H * D;
    const long W = 3L * HD;
    const float* base = qkv + (long)b * T * W + (long)head * D;
    const int query = q0 + wave * 32 + r;
    const bool q_ok = query < len;
    float* o_row = out + ((long)b * T + query) * HD + (long)head * D + 4 * h;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    fp_f32x16 acc_o[JD];
#pragma unroll
    for (int j = 0; j < JD; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc_o[j][q] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    if (q0 < len) {   // (uniform over the workgroup) otherwise: nothing of the row is read, zeros are written
        float4 qf[KG];   // Q[query][8 kg + 4 h ..]: the B operand of S^T, in the k order the K tile is read in
#pragma unroll
        for (int kg = 0; kg < KG; ++kg) qf[kg] = q_ok ? *reinterpret_cast<const float4*>(base + (long)query * W + 8 * kg + 4 * h) : zero4;
        const bool wave_live = q0 + wave * 32 < len;
        const int nkt = (len + FP_BK - 1) / FP_BK;   // tiles wholly behind the row's length are not visited
        float4 kr[NL], vr[NL];
#define FP_ATTN_LOAD(KT)                                                                                 \
        _Pragma("unroll") for (int j = 0; j < NL; ++j) {                                                 \
            const int e_ = tid + FP_WAVES * 64 * j, key_ = e_ / (D / 4), c4_ = e_ - key_ * (D / 4);     \
            const int gk_ = (KT) * FP_BK + key_;                                                         \
            const float* src_ = base + (long)gk_ * W + HD + 4 * c4_;                                     \
            kr[j] = gk_ < len ? *reinterpret_cast<const float4*>(src_) : zero4;                          \
            vr[j] = gk_ < len ? *reinterpret_cast<const float4*>(src_ + HD) : zero4;                     \
        }
        FP_ATTN_LOAD(0)
        for (int kt = 0; kt < nkt; ++kt) {
            __syncthreads();   // the previous tile has been multiplied
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int e = tid + FP_WAVES * 64 * j, key = e / (D / 4), c4 = e - key * (D / 4);
                *reinterpret_cast<float4*>(&Ks[key * KLD + 4 * c4]) = kr[j];
                *reinterpret_cast<float4*>(&Vs[key * D + 4 * c4]) = vr[j];
            }
            __syncthreads();
            if (kt + 1 < nkt) { FP_ATTN_LOAD(kt + 1) }
            if (!wave_live) continue;   // (uniform over the wave)
            // S^T = K Q^T: element q of block kb is key kb * 32 + (q & 3) + 8 (q >> 2) + 4 h of the tile, against this lane's query
            fp_f32x16 s[2];
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
                for (int q = 0; q < 16; ++q) s[kb][q] = 0.f;
#pragma unroll
                for (int kg = 0; kg < KG; ++kg) {
                    const float4 kf = *reinterpret_cast<const float4*>(&Ks[(kb * 32 + r) * KLD + 8 * kg + 4 * h]);
                    s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[kg].x, s[kb], 0, 0, 0);
                    s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[kg].y, s[kb], 0, 0, 0);
                    s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[kg].z, s[kb], 0, 0, 0);
                    s[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[kg].w, s[kb], 0, 0, 0);
                }
            }
            const int k0 = kt * FP_BK + 4 * h;
            float m_tile = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int key = k0 + kb * 32 + (q & 3) + 8 * (q >> 2);
                    const float v = key < len ? s[kb][q] * scale : -INFINITY;
                    s[kb][q] = v;
                    m_tile = fmaxf(m_tile, v);
                }
            m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 32));
            const float m_new = fmaxf(m_run, m_tile);   // finite: the tile's first key lies in front of the row's length
            const float alpha = expf(m_run - m_new);    // (0 at the first tile)
            float l_tile = 0.f;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float p = expf(s[kb][q] - m_new);   // exactly 0 for a key at or behind the length
                    s[kb][q] = p;
                    l_tile += p;
                }
            l_tile += __shfl_xor(l_tile, 32);
            l_run = l_run * alpha + l_tile;
            m_run = m_new;
#pragma unroll
            for (int j = 0; j < JD; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc_o[j][q] *= alpha;
            // O^T += V^T P^T: P's element q is this lane's B operand as it stands
#pragma unroll
            for (int kb = 0; kb < 2; ++kb)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const float* v_row = &Vs[(kb * 32 + (q & 3) + 8 * (q >> 2) + 4 * h) * D + r];
#pragma unroll
                    for (int j = 0; j < JD; ++j) acc_o[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(v_row[32 * j], s[kb][q], acc_o[j], 0, 0, 0);
                }
        }
#undef FP_ATTN_LOAD
    }
    if (query >= T) return;
    // element q of block j is column 32 j + (q & 3) + 8 (q >> 2) + 4 h of this lane's query
#pragma unroll
    for (int j = 0; j < JD; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float4 v = zero4;
            if (q_ok) v = make_float4(acc_o[j][4 * g] / l_run, acc_o[j][4 * g + 1] / l_run, acc_o[j][4 * g + 2] / l_run, acc_o[j][4 * g + 3] / l_run);
            *reinterpret_cast<float4*>(o_row + 32 * j + 8 * g) = v;
        }
}

int fp_attention(const float* qkv, const int32_t* lens, int B, int T, int H, int D, float* out, hipStream_t s) {
    const dim3 grid((unsigned)((T + FP_BQ - 1) / FP_BQ), (unsigned)H, (unsigned)B);
    const float scale = 1.f / sqrtf((float)D);
    if (D == 64) fp_attention_kernel<64><<<grid, FP_WAVES * 64, 0, s>>>(qkv, lens, T, H, scale, out);
    else fp_attention_kernel<32><<<grid, FP_WAVES * 64, 0, s>>>(qkv, lens, T, H, scale, out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// ---- (x + y), LayerNorm -> the haloed layout
struct FpNorm {
    const float* x; long x_bs;     // x[b][t][:] at x + b * x_bs + t * C
    const float* y;                // [B][N][C] or nullptr
    const int32_t* lens;
    int N, C;
    const float* ln_w; const float* ln_b;
    float* out;                    // [B][N + 2][C]: position t at row t + 1, zero halo rows
    float* out2;                   // [B][N][C] as well, or nullptr
};

template <int NC>   // channels per lane: C <= 64 NC
__global__ void __launch_bounds__(FP_WAVES * 64) fp_add_ln_kernel(const FpNorm p) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t0 = (int)blockIdx.x * FP_P, C = p.C, N = p.N;
    const int len = fp_len(p.lens, b, N);
    const int t_end = min(t0 + FP_P, N);
    float lw[NC], lb[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        lw[i] = c < C ? p.ln_w[c] : 0.f;
        lb[i] = c < C ? p.ln_b[c] : 0.f;
    }
    const float c_f = (float)C;
    float* out_b = p.out + (long)b * (N + 2) * C;
    for (int tt = wave; t0 + tt < t_end; tt += FP_WAVES) {
        const int t = t0 + tt;
        float* o = out_b + (long)(t + 1) * C;
        float* o2 = p.out2 ? p.out2 + ((long)b * N + t) * C : nullptr;
        if (t == 0 || t == N - 1) {   // the wave of an edge position writes that edge's halo row
#pragma unroll
            for (int i = 0; i < NC; ++i)
                if (lane + 64 * i < C) {
                    if (t == 0) out_b[lane + 64 * i] = 0.f;
                    if (t == N - 1) out_b[(long)(N + 1) * C + lane + 64 * i] = 0.f;
                }
        }
        if (t >= len) {
#pragma unroll
            for (int i = 0; i < NC; ++i)
                if (lane + 64 * i < C) {
                    o[lane + 64 * i] = 0.f;
                    if (o2) o2[lane + 64 * i] = 0.f;
                }
            continue;
        }
        const float* xr = p.x + (long)b * p.x_bs + (long)t * C;
        const float* yr = p.y ? p.y + ((long)b * N + t) * C : nullptr;
        float v[NC], sum = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c = lane + 64 * i;
            float a = 0.f;
            if (c < C) {
                a = xr[c];
                if (yr) a += yr[c];
            }
            v[i] = a;
            sum += a;
        }
        // the mean, the mean of what is left (an ulp of the mean) and then the squared deviations, as vc_dwconv_ln_kernel forms them
        const float mean = fp_wave_sum(sum) / c_f;
        float rest = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            v[i] = lane + 64 * i < C ? v[i] - mean : 0.f;
            rest += v[i];
        }
        const float mean2 = fp_wave_sum(rest) / c_f;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            v[i] = lane + 64 * i < C ? v[i] - mean2 : 0.f;
            sq = fmaf(v[i], v[i], sq);
        }
        const float rstd = 1.f / sqrtf(fp_wave_sum(sq) / c_f + FP_LN_EPS);
#pragma unroll
        for (int i = 0; i < NC; ++i)
            if (lane + 64 * i < C) {
                const float w = fmaf(v[i] * rstd, lw[i], lb[i]);
                o[lane + 64 * i] = w;
                if (o2) o2[lane + 64 * i] = w;
            }
    }
}

int fp_norm(const FpNorm& p, int B, hipStream_t s) {
    const dim3 grid((unsigned)((p.N + FP_P - 1) / FP_P), (unsigned)B);
    const int nc = (p.C + 63) / 64;
    if (nc <= 1) fp_add_ln_kernel<1><<<grid, FP_WAVES * 64, 0, s>>>(p);
    else if (nc <= 2) fp_add_ln_kernel<2><<<grid, FP_WAVES * 64, 0, s>>>(p);
    else if (nc <= 4) fp_add_ln_kernel<4><<<grid, FP_WAVES * 64, 0, s>>>(p);
    else fp_add_ln_kernel<8><<<grid, FP_WAVES * 64, 0, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// ---- pos[p] = cat(sin(p f), cos(p f)), f_i = 10000^(-2 i / C), in float64
__global__ void fp_pos_table_kernel(float* pos, int P, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)P * C) return;
    const int p = (int)(i / C), c = (int)(i - (long)p * C), half = C / 2;
    const int k = c < half ? c : c - half;
    const double f = pow(10000.0, -2.0 * (double)k / (double)C);
    pos[i] = (float)(c < half ? sin((double)p * f) : cos((double)p * f));
}

// ---- x[b][l + 1][:] = emb[tokens[b][l]] + pos[l] at the row's own positions, zeros behind them and in the halo rows; a wave per row of x
__global__ void __launch_bounds__(FP_WAVES * 64) fp_embed_kernel(const int32_t* __restrict__ tokens, const int32_t* __restrict__ lens, const float* __restrict__ emb,
                                                                  const float* __restrict__ pos, int n_tokens, int L, int C, float* __restrict__ x,
                                                                  float* __restrict__ x2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, row = (int)blockIdx.x * FP_WAVES + wave;   // row of the haloed layout
    if (row >= L + 2) return;
    const int l = row - 1, len = fp_len(lens, b, L);
    const bool live = l >= 0 && l < len;
    int tok = live ? tokens[(long)b * L + l] : 0;
    if (tok < 0 || tok >= n_tokens) tok = 0;
    float* o = x + ((long)b * (L + 2) + row) * C;
    float* o2 = x2 && l >= 0 && l < L ? x2 + ((long)b * L + l) * C : nullptr;
    for (int c = lane; c < C; c += 64) {
        const float v = live ? emb[(long)tok * C + c] + pos[(long)l * C + c] : 0.f;
        o[c] = v;
        if (o2) o2[c] = v;
    }
}

// ---- x[b][l + 1][c] += bias[c] + sum_j w[c][j] * p[b][l + j - 1] at the row's own positions (p is zero outside them): pitch_emb, energy_emb
__global__ void __launch_bounds__(256) fp_cond_add_kernel(float* __restrict__ x, const float* __restrict__ p, const int32_t* __restrict__ lens,
                                                          const float* __restrict__ w, const float* __restrict__ bias, int L, int C) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)L * C) return;
    const int l = (int)(i / C), c = (int)(i - (long)l * C), len = fp_len(lens, b, L);
    if (l >= len) return;   // zeros already
    const float* pr = p + (long)b * L;
    const float pm = l > 0 ? pr[l - 1] : 0.f, p0 = pr[l], pp = l + 1 < len ? pr[l + 1] : 0.f;
    float a = bias[c];
    a = fmaf(w[3 * c], pm, a);
    a = fmaf(w[3 * c + 1], p0, a);
    a = fmaf(w[3 * c + 2], pp, a);
    x[((long)b * (L + 2) + l + 1) * C + c] += a;
}

// ---- durations -> reps, starts, the row's frame count.  A workgroup per row; the scan is one thread's walk over LDS
__global__ void __launch_bounds__(256) fp_plan_kernel(const float* __restrict__ log_dur, const int32_t* __restrict__ dur_in, const int32_t* __restrict__ lens,
                                                      int L, float pace, float max_dur, int min_frames, int cap, int32_t* __restrict__ reps,
                                                      int32_t* __restrict__ starts, int32_t* __restrict__ counts) {
    __shared__ int r_s[GVX_FASTPITCH_MAX_TOKENS];
    const int b = blockIdx.x, tid = threadIdx.x, len = fp_len(lens, b, L);
    for (int l = tid; l < L; l += 256) {
        int r = 0;
        if (l < len) {
            const float d = dur_in ? (float)dur_in[(long)b * L + l] : fminf(fmaxf(expf(log_dur[(long)b * L + l]) - 1.f, 0.f), max_dur);
            const float f = floorf(d / pace + 0.5f);
            r = f >= (float)cap ? cap : f > 0.f ? (int)f : 0;   // (a NaN duration: 0)
            r = max(r, min_frames);
        }
        r_s[l] = r;
    }
    __syncthreads();
    if (tid == 0) {
        int cum = 0;
        for (int l = 0; l < L; ++l) {
            const int e = min(cum + r_s[l], cap);   // a row is cut at `cap` frames
            starts[(long)b * L + l] = cum;
            r_s[l] = e - cum;
            cum = e;
        }
        if (cum == 0 && len > 0) { r_s[len - 1] = 1; cum = 1; }   // an empty row gets one frame of its last token
        counts[b] = cum;
    }
    __syncthreads();
    for (int l = tid; l < L; l += 256) reps[(long)b * L + l] = r_s[l];
}

// ---- the regulator: y[b][t + 1][:] = enc[b][l + 1][:] + pos[t] for the token l with start_l <= t < start_l + reps_l, the alignment row
// and the gate.  A wave per row of the haloed output
__global__ void __launch_bounds__(FP_WAVES * 64) fp_regulate_kernel(const float* __restrict__ enc, const int32_t* __restrict__ reps, const int32_t* __restrict__ starts,
                                                                     const int32_t* __restrict__ counts, const int32_t* __restrict__ tok_lens,
                                                                     const float* __restrict__ pos, int L, int T, int C, float* __restrict__ y,
                                                                     float* __restrict__ y2, float* __restrict__ align, float* __restrict__ gate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, row = (int)blockIdx.x * FP_WAVES + wave;
    if (row >= T + 2) return;
    const int t = row - 1, n = fp_len(counts, b, T), len = fp_len(tok_lens, b, L);
    const bool live = t >= 0 && t < n;
    int tok = -1;
    if (live) {   // the first token whose end lies behind t (ends do not decrease)
        const int32_t* st = starts + (long)b * L;
        const int32_t* rp = reps + (long)b * L;
        int lo = 0, hi = len - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (st[mid] + rp[mid] > t) hi = mid; else lo = mid + 1;
        }
        tok = lo;
    }
    float* o = y + ((long)b * (T + 2) + row) * C;
    const bool inner = t >= 0 && t < T;
    float* o2 = y2 && inner ? y2 + ((long)b * T + t) * C : nullptr;
    const float* src = enc + ((long)b * (L + 2) + tok + 1) * C;
    for (int c = lane; c < C; c += 64) {
        const float v = live ? src[c] + pos[(long)t * C + c] : 0.f;
        o[c] = v;
        if (o2) o2[c] = v;
    }
    if (!inner) return;
    float* a = align + ((long)b * T + t) * L;
    for (int l = lane; l < L; l += 64) a[l] = l == tok ? 1.f : 0.f;
    if (lane == 0) gate[(long)b * T + t] = t < n - 1 ? -1e3f : 1e3f;
}

// ---- proj [B][T][M] -> mel [B][M][T], 32 x 32 tiles through LDS
__global__ void __launch_bounds__(256) fp_to_channels_first_kernel(const float* __restrict__ src, int T, int M, float* __restrict__ dst) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = (int)blockIdx.x * 32, c0 = (int)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int t = t0 + i, c = c0 + tx;
        tile[i][tx] = t < T && c < M ? src[((long)b * T + t) * M + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, t = t0 + tx;
        if (c < M && t < T) dst[((long)b * M + c) * T + t] = tile[tx][i];
    }
}

__global__ void fp_zero_kernel(float* p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.f;
}

// ---- dims, blob, workspace
const char* fp_stack_problem(const gvx_fft_stack_dims& s) {
    if (s.n_layers < 1 || s.n_layers > GVX_FASTPITCH_MAX_LAYERS) return "n_layers must be in [1, GVX_FASTPITCH_MAX_LAYERS]";
    if (s.n_head < 1 || s.n_head > GVX_FASTPITCH_MAX_HEADS) return "n_head must be in [1, GVX_FASTPITCH_MAX_HEADS]";
    if (s.d_head != 32 && s.d_head != 64) return "d_head must be 32 or 64";
    if (s.d_inner < 32 || s.d_inner > GVX_FASTPITCH_MAX_INNER || s.d_inner % 32) return "d_inner must be a multiple of 32 in [32, GVX_FASTPITCH_MAX_INNER]";
    if (s.kernel_size != 1 && s.kernel_size != 3) return "kernel_size must be 1 or 3";
    return nullptr;
}

const char* fp_dims_problem(const gvx_fastpitch_dims* d) {
    if (!d) return "null dims";
    if (d->n_tokens < 1 || d->n_tokens > (1 << 20)) return "n_tokens must be in [1, 2^20]";
    if (d->n_mels < 1 || d->n_mels > 4096) return "n_mels must be in [1, 4096]";
    if (d->d_model < 32 || d->d_model > GVX_FASTPITCH_MAX_DIM || d->d_model % 32) return "d_model must be a multiple of 32 in [32, GVX_FASTPITCH_MAX_DIM]";
    if (const char* why = fp_stack_problem(d->enc)) return why;
    if (const char* why = fp_stack_problem(d->dec)) return why;
    if (d->pred_filter < 32 || d->pred_filter > GVX_FASTPITCH_MAX_DIM || d->pred_filter % 32)
        return "pred_filter must be a multiple of 32 in [32, GVX_FASTPITCH_MAX_DIM]";
    if (d->pred_layers < 1 || d->pred_layers > 8) return "pred_layers must be in [1, 8]";
    if (d->energy != 0 && d->energy != 1) return "energy must be 0 or 1";
    if (d->max_tokens < 1 || d->max_tokens > GVX_FASTPITCH_MAX_TOKENS) return "max_tokens must be in [1, GVX_FASTPITCH_MAX_TOKENS]";
    if (d->max_decoder_steps < 1 || d->max_decoder_steps > GVX_FASTPITCH_MAX_POSITIONS) return "max_decoder_steps must be in [1, GVX_FASTPITCH_MAX_POSITIONS]";
    if (d->max_duration < 1 || d->max_duration > GVX_FASTPITCH_MAX_POSITIONS) return "max_duration must be in [1, GVX_FASTPITCH_MAX_POSITIONS]";
    if (d->min_token_frames < 0 || d->min_token_frames > d->max_duration) return "min_token_frames must be in [0, max_duration]";
    return nullptr;
}

struct FpLayer { size_t qkv_w, qkv_b, o_w, ln1_w, ln1_b, c1_w, c1_b, c2_w, c2_b, ln2_w, ln2_b; };
struct FpPredLayer { size_t w, b, ln_w, ln_b; };
struct FpPred { FpPredLayer layer[8]; size_t fc_w, fc_b; };
struct FpBlob {
    size_t emb;
    FpLayer enc[GVX_FASTPITCH_MAX_LAYERS], dec[GVX_FASTPITCH_MAX_LAYERS];
    FpPred pred[3];                // duration, pitch, energy
    size_t cond_w[2], cond_b[2];   // pitch_emb, energy_emb
    size_t proj_w, proj_b, pos, total;
};
const char* const FP_PRED_NAMES[3] = {"duration_predictor", "pitch_predictor", "energy_predictor"};
const char* const FP_COND_NAMES[2] = {"pitch_emb", "energy_emb"};

inline int fp_positions(const gvx_fastpitch_dims& d) { return std::max(d.max_tokens, d.max_decoder_steps); }

// `visit(name, offset, numel)` sees every packed tensor in blob order
template <typename F>
FpBlob fp_blob_layout(const gvx_fastpitch_dims& d, F&& visit) {
    FpBlob L{};
    size_t at = 0;
    auto take = [&](const std::string& name, size_t floats) { const size_t o = at; at += gvx::round64(floats); if (!name.empty()) visit(name, o, floats); return o; };
    const size_t C = d.d_model, F_ = d.pred_filter;
    L.emb = take("encoder.word_emb.weight", (size_t)d.n_tokens * C);
    for (int s = 0; s < 2; ++s) {
        const gvx_fft_stack_dims& sd = s ? d.dec : d.enc;
        const size_t HD = (size_t)sd.n_head * sd.d_head, I = sd.d_inner, k = sd.kernel_size;
        for (int i = 0; i < sd.n_layers; ++i) {
            FpLayer& l = (s ? L.dec : L.enc)[i];
            const std::string base = std::string(s ? "decoder" : "encoder") + ".layers." + std::to_string(i) + ".";
            l.qkv_w = take(base + "dec_attn.qkv_net.weight", 3 * HD * C); l.qkv_b = take(base + "dec_attn.qkv_net.bias", 3 * HD);
            l.o_w = take(base + "dec_attn.o_net.weight", C * HD);
            l.ln1_w = take(base + "dec_attn.layer_norm.weight", C); l.ln1_b = take(base + "dec_attn.layer_norm.bias", C);
            l.c1_w = take(base + "pos_ff.CoreNet.0.weight", I * k * C); l.c1_b = take(base + "pos_ff.CoreNet.0.bias", I);
            l.c2_w = take(base + "pos_ff.CoreNet.2.weight", C * k * I); l.c2_b = take(base + "pos_ff.CoreNet.2.bias", C);
            l.ln2_w = take(base + "pos_ff.layer_norm.weight", C); l.ln2_b = take(base + "pos_ff.layer_norm.bias", C);
        }
    }
    for (int p = 0; p < 2 + d.energy; ++p) {
        const std::string base = std::string(FP_PRED_NAMES[p]) + ".";
        for (int i = 0; i < d.pred_layers; ++i) {
            FpPredLayer& l = L.pred[p].layer[i];
            const std::string lb = base + "layers." + std::to_string(i) + ".";
            l.w = take(lb + "conv.weight", F_ * 3 * (i ? F_ : C)); l.b = take(lb + "conv.bias", F_);
            l.ln_w = take(lb + "norm.weight", F_); l.ln_b = take(lb + "norm.bias", F_);
        }
        L.pred[p].fc_w = take(base + "fc.weight", F_); L.pred[p].fc_b = take(base + "fc.bias", 1);
    }
    for (int p = 0; p < 1 + d.energy; ++p) {
        L.cond_w[p] = take(std::string(FP_COND_NAMES[p]) + ".weight", 3 * C); L.cond_b[p] = take(std::string(FP_COND_NAMES[p]) + ".bias", C);
    }
    L.proj_w = take("proj.weight", (size_t)d.n_mels * C); L.proj_b = take("proj.bias", d.n_mels);
    L.pos = take("", (size_t)fp_positions(d) * C);
    L.total = at;
    return L;
}
FpBlob fp_blob_layout(const gvx_fastpitch_dims& d) { return fp_blob_layout(d, [](const std::string&, size_t, size_t) {}); }

struct FpWs { size_t xa, xb, qkv, att, o, hid, pa, pb, pt, proj, total; };

// either phase at N positions: the stack's tensors at the larger of the two stacks' widths, the predictors' and the projection's
FpWs fp_ws_plan(const gvx_fastpitch_dims& d, int B, int N) {
    FpWs w{};
    GenRows ws{B};
    const size_t C = d.d_model, HD = std::max(d.enc.n_head * d.enc.d_head, d.dec.n_head * d.dec.d_head), I = std::max(d.enc.d_inner, d.dec.d_inner);
    const size_t F_ = d.pred_filter, n = N;
    w.xa = ws.rows((n + 2) * C); w.xb = ws.rows((n + 2) * C);
    w.qkv = ws.rows(n * 3 * HD); w.att = ws.rows(n * HD); w.o = ws.rows(n * C);
    w.hid = ws.rows((n + 2) * I);
    w.pa = ws.rows((n + 2) * F_); w.pb = ws.rows((n + 2) * F_); w.pt = ws.rows(n * F_);
    w.proj = ws.rows(n * d.n_mels);
    w.total = ws.total;
    return w;
}

const char* fp_shape_problem(int B, int N) {
    if (B < 1 || B > 65535) return "B must be in [1, 65535]";
    if (N < 1 || N > GVX_FASTPITCH_MAX_POSITIONS) return "the positions of a row must be in [1, GVX_FASTPITCH_MAX_POSITIONS]";
    if ((long)B * N > (1L << 24)) return "B times the positions of a row is beyond 2^24";
    return nullptr;
}

// C = epilogue(A W^T + bias), rows grouped by N positions per sequence
int fp_gemm(const float* A, const RowMap& amap, int K, const float* W, const float* bias, float* out, const RowMap& cmap, int n_out, int B, int N,
            const int32_t* lens, int act, int c_halo, hipStream_t s) {
    GemmParams g{};
    g.A = A; g.amap = amap; g.W = W; g.ldw = K;
    g.C = out; g.cmap = cmap;
    g.bias = bias; g.keep = nullptr; g.keep_ld = 0;
    g.M = B * N; g.N = n_out; g.K = K;
    g.act = act; g.row_len = lens; g.c_halo = c_halo;
    HIP_TRY(gvx::launch_gemm(g, s));
    return GVX_OK;
}

// one FFT stack on x (haloed, [B][N + 2][C]); `other` is the second haloed buffer.  Returns the buffer that holds the result in *result
int fp_stack(const gvx_fft_stack_dims& sd, const FpLayer* layers, const float* blob, int C, int B, int N, const int32_t* lens, float* x, float* other,
             void* workspace, const FpWs& wp, float* const* stage_out, float** result, hipStream_t s) {
    const int HD = sd.n_head * sd.d_head, I = sd.d_inner, k = sd.kernel_size, pad = k / 2;
    float* qkv = gvx::ws_ptr<float>(workspace, wp.qkv);
    float* att = gvx::ws_ptr<float>(workspace, wp.att);
    float* o = gvx::ws_ptr<float>(workspace, wp.o);
    float* hid = gvx::ws_ptr<float>(workspace, wp.hid);
    const long xs = (long)(N + 2) * C, hs = (long)(N + 2) * I;
    const RowMap x_rows{N, xs, (long)C};   // from the first interior row: the positions themselves; from a row's first tap: the k-tap rows
    int rc;
    for (int i = 0; i < sd.n_layers; ++i) {
        const FpLayer& l = layers[i];
        if ((rc = fp_gemm(x + C, x_rows, C, blob + l.qkv_w, blob + l.qkv_b, qkv, RowMap{N, (long)N * 3 * HD, 3L * HD}, 3 * HD, B, N, nullptr, gvx::ACT_NONE, 0,
                          s)) != GVX_OK) return rc;
        if ((rc = fp_attention(qkv, lens, B, N, sd.n_head, sd.d_head, att, s)) != GVX_OK) return rc;
        if ((rc = fp_gemm(att, RowMap{N, (long)N * HD, (long)HD}, HD, blob + l.o_w, nullptr, o, RowMap{N, (long)N * C, (long)C}, C, B, N, nullptr, gvx::ACT_NONE,
                          0, s)) != GVX_OK) return rc;
        FpNorm n1{};
        n1.x = x + C; n1.x_bs = xs; n1.y = o; n1.lens = lens; n1.N = N; n1.C = C; n1.ln_w = blob + l.ln1_w; n1.ln_b = blob + l.ln1_b; n1.out = other;
        if ((rc = fp_norm(n1, B, s)) != GVX_OK) return rc;
        // the feed-forward: row (b, t) of a k-tap product is the k C floats from haloed row t + 1 - pad
        if ((rc = fp_gemm(other + (1 - pad) * C, x_rows, k * C, blob + l.c1_w, blob + l.c1_b, hid + I, RowMap{N, hs, (long)I}, I, B, N, lens, gvx::ACT_RELU, 1,
                          s)) != GVX_OK) return rc;
        if ((rc = fp_gemm(hid + (1 - pad) * I, RowMap{N, hs, (long)I}, k * I, blob + l.c2_w, blob + l.c2_b, o, RowMap{N, (long)N * C, (long)C}, C, B, N, nullptr,
                          gvx::ACT_NONE, 0, s)) != GVX_OK) return rc;
        FpNorm n2{};
        n2.x = other + C; n2.x_bs = xs; n2.y = o; n2.lens = lens; n2.N = N; n2.C = C; n2.ln_w = blob + l.ln2_w; n2.ln_b = blob + l.ln2_b; n2.out = x;
        n2.out2 = stage_out ? stage_out[i] : nullptr;
        if ((rc = fp_norm(n2, B, s)) != GVX_OK) return rc;
    }
    *result = x;
    return GVX_OK;
}

// a predictor on x (haloed [B][L + 2][C]) -> out [B][L], zeros behind a row's length
int fp_predictor(const gvx_fastpitch_dims& d, const FpPred& P, const float* blob, const float* x, int B, int L, const int32_t* lens, void* workspace,
                 const FpWs& wp, float* out, hipStream_t s) {
    const int C = d.d_model, F_ = d.pred_filter;
    float* bufs[2] = {gvx::ws_ptr<float>(workspace, wp.pa), gvx::ws_ptr<float>(workspace, wp.pb)};
    float* pt = gvx::ws_ptr<float>(workspace, wp.pt);
    const float* in = x;
    int cin = C, rc;
    for (int i = 0; i < d.pred_layers; ++i) {
        const FpPredLayer& l = P.layer[i];
        if ((rc = fp_gemm(in, RowMap{L, (long)(L + 2) * cin, (long)cin}, 3 * cin, blob + l.w, blob + l.b, pt, RowMap{L, (long)L * F_, (long)F_}, F_, B, L, nullptr,
                          gvx::ACT_RELU, 0, s)) != GVX_OK) return rc;
        FpNorm n{};
        n.x = pt; n.x_bs = (long)L * F_; n.y = nullptr; n.lens = lens; n.N = L; n.C = F_; n.ln_w = blob + l.ln_w; n.ln_b = blob + l.ln_b; n.out = bufs[i & 1];
        if ((rc = fp_norm(n, B, s)) != GVX_OK) return rc;
        in = bufs[i & 1];
        cin = F_;
    }
    return fp_gemm(in + F_, RowMap{L, (long)(L + 2) * F_, (long)F_}, F_, blob + P.fc_w, blob + P.fc_b, out, RowMap{L, (long)L, 1L}, 1, B, L, lens, gvx::ACT_NONE, 0, s);
}

}  // namespace

extern "C" {

int gvx_self_attention(const float* qkv, const int32_t* lens, int B, int T, int n_head, int d_head, float* out, void* stream) {
    if (!qkv || !out || qkv == out) return fail(GVX_ERR_INVALID_ARG, "null argument, or out is qkv");
    if (const char* why = fp_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (d_head != 32 && d_head != 64) return fail(GVX_ERR_INVALID_ARG, "d_head = %d must be 32 or 64", d_head);
    if (n_head < 1 || n_head > GVX_FASTPITCH_MAX_HEADS) return fail(GVX_ERR_INVALID_ARG, "n_head = %d must be in [1, %d]", n_head, (int)GVX_FASTPITCH_MAX_HEADS);
    if (((uintptr_t)qkv | (uintptr_t)out) & 15) return fail(GVX_ERR_INVALID_ARG, "qkv and out must be 16-byte aligned");
    return fp_attention(qkv, lens, B, T, n_head, d_head, out, (hipStream_t)stream);
}

int gvx_add_layer_norm(const float* x, const float* y, const int32_t* lens, int B, int N, int C, const float* ln_w, const float* ln_b, float* out_haloed,
                       float* out_plain, void* stream) {
    if (!x || !ln_w || !ln_b || !out_haloed) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (C < 32 || C > GVX_FASTPITCH_MAX_DIM || C % 32) return fail(GVX_ERR_INVALID_ARG, "C = %d must be a multiple of 32 in [32, %d]", C, (int)GVX_FASTPITCH_MAX_DIM);
    if (const char* why = fp_shape_problem(B, N)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    const size_t plain = (size_t)B * N * C, haloed = (size_t)B * (N + 2) * C;
    auto overlap = [](const float* a, size_t na, const float* b, size_t nb) { return a && b && (uintptr_t)a < (uintptr_t)(b + nb) && (uintptr_t)b < (uintptr_t)(a + na); };
    const float* const outs[2] = {out_haloed, out_plain};
    const size_t out_n[2] = {haloed, plain};
    for (int i = 0; i < 2; ++i)
        if (overlap(outs[i], out_n[i], x, plain) || overlap(outs[i], out_n[i], y, plain) || overlap(outs[i], out_n[i], ln_w, (size_t)C) ||
            overlap(outs[i], out_n[i], ln_b, (size_t)C))
            return fail(GVX_ERR_INVALID_ARG, "an output overlaps an input");
    if (overlap(out_haloed, haloed, out_plain, plain)) return fail(GVX_ERR_INVALID_ARG, "out_haloed and out_plain overlap");
    FpNorm p{};
    p.x = x; p.x_bs = (long)N * C; p.y = y; p.lens = lens; p.N = N; p.C = C; p.ln_w = ln_w; p.ln_b = ln_b; p.out = out_haloed; p.out2 = out_plain;
    return fp_norm(p, B, (hipStream_t)stream);
}

size_t gvx_fastpitch_blob_floats(const gvx_fastpitch_dims* dims) {
    if (fp_dims_problem(dims)) return 0;
    return fp_blob_layout(*dims).total;
}

size_t gvx_fastpitch_workspace_bytes(const gvx_fastpitch_dims* dims, int B, int N) {
    if (fp_dims_problem(dims) || fp_shape_problem(B, N)) return 0;
    return fp_ws_plan(*dims, B, N).total;
}

int gvx_fastpitch_pack_weights_device(const gvx_fastpitch_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = fp_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_fastpitch_dims& d = *dims;
    hipStream_t s = (hipStream_t)stream;
    GenPacker P{{table, n}};
    const FpBlob L = fp_blob_layout(d, [&](const std::string& name, size_t dst, size_t numel) { P.take(name, dst, numel); });
    if (const int rc = P.run(device_blob, 0, L.total, s)) return rc;
    const long n_pos = (long)fp_positions(d) * d.d_model;
    fp_pos_table_kernel<<<(unsigned)((n_pos + 255) / 256), 256, 0, s>>>(device_blob + L.pos, fp_positions(d), d.d_model);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int gvx_fastpitch_create(const gvx_fastpitch_dims* dims, gvx_fastpitch** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = fp_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_fastpitch* h = new gvx_fastpitch();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_fastpitch_destroy(gvx_fastpitch* h) { delete h; }

int gvx_fastpitch_bind(gvx_fastpitch* h, const float* device_blob) {
    if (const int rc = gen_bind(h, device_blob)) return rc;
    HIP_TRY(gvx::gemm_init());   // the big tiles' dynamic LDS
    return GVX_OK;
}

int gvx_fastpitch_timing_enable(gvx_fastpitch* h, int enable) {
    if (const int rc = gen_timing_enable(h, enable, 7)) return rc;
    h->encoded = h->decoded = false;
    return GVX_OK;
}

// marks 0 .. 2: encode's start, behind the encoder, its end; marks 3 .. 6: decode's start, behind the regulator, the decoder, the projection
int gvx_fastpitch_stage_times_ms(gvx_fastpitch* h, float* ms_out, int* n_out) {
    if (!h || !ms_out || !n_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->timing) return fail(GVX_ERR_STATE, "timing is not enabled");
    if (!h->encoded || !h->decoded) return fail(GVX_ERR_STATE, "no encode and decode since timing was enabled");
    const std::vector<hipEvent_t>& ev = h->marks.ev;
    HIP_TRY(hipEventSynchronize(ev[6]));
    float reg = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms_out[0], ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms_out[1], ev[1], ev[2]));
    HIP_TRY(hipEventElapsedTime(&reg, ev[3], ev[4]));
    ms_out[1] += reg;
    HIP_TRY(hipEventElapsedTime(&ms_out[2], ev[4], ev[5]));
    HIP_TRY(hipEventElapsedTime(&ms_out[3], ev[5], ev[6]));
    *n_out = 4;
    return GVX_OK;
}

int gvx_fastpitch_encode(gvx_fastpitch* h, const int32_t* tokens, const int32_t* token_lengths, int B, int L, float pace, const int32_t* durations_in,
                         const float* pitch_in, float* enc_out, float* log_dur, float* pitch_pred, float* energy_pred, int32_t* reps, int32_t* starts,
                         int32_t* frame_counts, float* const* stage_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !tokens || !enc_out || !log_dur || !pitch_pred || !energy_pred || !reps || !starts || !frame_counts) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    const gvx_fastpitch_dims& d = h->d;
    if (const char* why = fp_shape_problem(B, L)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (L > d.max_tokens) return fail(GVX_ERR_INVALID_ARG, "L = %d is beyond max_tokens = %d", L, d.max_tokens);
    if (!(pace >= 0.125f && pace <= 8.f)) return fail(GVX_ERR_INVALID_ARG, "pace must be in [0.125, 8]");
    const FpWs wp = fp_ws_plan(d, B, L);
    int ev = 0, rc;
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    if ((uintptr_t)enc_out % 16) return fail(GVX_ERR_INVALID_ARG, "enc_out must be 16-byte aligned");
    if ((rc = gen_check_stage_out(stage_out, d.enc.n_layers + 1)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const FpBlob BL = fp_blob_layout(d);
    const float* blob = h->blob;
    const int C = d.d_model;
    auto stamp = [&] { return gen_mark(h, ev++, s); };
    if ((rc = stamp()) != GVX_OK) return rc;
    // the stack's last LayerNorm writes the buffer it started from: an even walk that ends in enc_out starts there
    float* xb = gvx::ws_ptr<float>(workspace, wp.xb);
    fp_embed_kernel<<<dim3((unsigned)((L + 2 + FP_WAVES - 1) / FP_WAVES), (unsigned)B), FP_WAVES * 64, 0, s>>>(tokens, token_lengths, blob + BL.emb, blob + BL.pos,
                                                                                                               d.n_tokens, L, C, enc_out, stage_out ? stage_out[0] : nullptr);
    HIP_TRY(hipGetLastError());
    float* x = nullptr;
    if ((rc = fp_stack(d.enc, BL.enc, blob, C, B, L, token_lengths, enc_out, xb, workspace, wp, stage_out ? stage_out + 1 : nullptr, &x, s)) != GVX_OK) return rc;
    if ((rc = stamp()) != GVX_OK) return rc;

    if ((rc = fp_predictor(d, BL.pred[0], blob, x, B, L, token_lengths, workspace, wp, log_dur, s)) != GVX_OK) return rc;
    if ((rc = fp_predictor(d, BL.pred[1], blob, x, B, L, token_lengths, workspace, wp, pitch_pred, s)) != GVX_OK) return rc;
    const dim3 cond_grid((unsigned)(((long)L * C + 255) / 256), (unsigned)B);
    fp_cond_add_kernel<<<cond_grid, 256, 0, s>>>(x, pitch_in ? pitch_in : pitch_pred, token_lengths, blob + BL.cond_w[0], blob + BL.cond_b[0], L, C);
    HIP_TRY(hipGetLastError());
    if (d.energy) {
        if ((rc = fp_predictor(d, BL.pred[2], blob, x, B, L, token_lengths, workspace, wp, energy_pred, s)) != GVX_OK) return rc;
        fp_cond_add_kernel<<<cond_grid, 256, 0, s>>>(x, energy_pred, token_lengths, blob + BL.cond_w[1], blob + BL.cond_b[1], L, C);
    } else {
        fp_zero_kernel<<<(unsigned)(((long)B * L + 255) / 256), 256, 0, s>>>(energy_pred, (long)B * L);
    }
    HIP_TRY(hipGetLastError());
    fp_plan_kernel<<<(unsigned)B, 256, 0, s>>>(log_dur, durations_in, token_lengths, L, pace, (float)d.max_duration, d.min_token_frames, d.max_decoder_steps, reps,
                                                starts, frame_counts);
    HIP_TRY(hipGetLastError());
    if ((rc = stamp()) != GVX_OK) return rc;
    h->encoded = h->timing;
    return GVX_OK;
}

int gvx_fastpitch_decode(gvx_fastpitch* h, const float* enc_out, const int32_t* reps, const int32_t* starts, const int32_t* frame_counts,
                         const int32_t* token_lengths, int B, int L, int T, float* mel_out, float* gate_out, float* align_out, float* const* stage_out,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !enc_out || !reps || !starts || !frame_counts || !mel_out || !gate_out || !align_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    const gvx_fastpitch_dims& d = h->d;
    if (const char* why = fp_shape_problem(B, L)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (const char* why = fp_shape_problem(B, T)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (T > d.max_decoder_steps) return fail(GVX_ERR_INVALID_ARG, "T = %d is beyond max_decoder_steps = %d", T, d.max_decoder_steps);
    const FpWs wp = fp_ws_plan(d, B, T);
    int ev = 3, rc;
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    if ((rc = gen_check_stage_out(stage_out, d.dec.n_layers + 1)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const FpBlob BL = fp_blob_layout(d);
    const float* blob = h->blob;
    const int C = d.d_model, M = d.n_mels;
    auto stamp = [&] { return gen_mark(h, ev++, s); };
    if ((rc = stamp()) != GVX_OK) return rc;
    float* xa = gvx::ws_ptr<float>(workspace, wp.xa);
    float* xb = gvx::ws_ptr<float>(workspace, wp.xb);
    fp_regulate_kernel<<<dim3((unsigned)((T + 2 + FP_WAVES - 1) / FP_WAVES), (unsigned)B), FP_WAVES * 64, 0, s>>>(
        enc_out, reps, starts, frame_counts, token_lengths, blob + BL.pos, L, T, C, xa, stage_out ? stage_out[0] : nullptr, align_out, gate_out);
    HIP_TRY(hipGetLastError());
    if ((rc = stamp()) != GVX_OK) return rc;
    float* x = nullptr;
    if ((rc = fp_stack(d.dec, BL.dec, blob, C, B, T, frame_counts, xa, xb, workspace, wp, stage_out ? stage_out + 1 : nullptr, &x, s)) != GVX_OK) return rc;
    if ((rc = stamp()) != GVX_OK) return rc;
    float* proj = gvx::ws_ptr<float>(workspace, wp.proj);
    if ((rc = fp_gemm(x + C, RowMap{T, (long)(T + 2) * C, (long)C}, C, blob + BL.proj_w, blob + BL.proj_b, proj, RowMap{T, (long)T * M, (long)M}, M, B, T,
                      frame_counts, gvx::ACT_NONE, 0, s)) != GVX_OK) return rc;
    fp_to_channels_first_kernel<<<dim3((unsigned)((T + 31) / 32), (unsigned)((M + 31) / 32), (unsigned)B), 256, 0, s>>>(proj, T, M, mel_out);
    HIP_TRY(hipGetLastError());
    if ((rc = stamp()) != GVX_OK) return rc;
    h->decoded = h->timing;
    return GVX_OK;
}

}  // C ABI
