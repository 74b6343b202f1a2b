// The HiFi-GAN generator's two layer kernels (HgLayer, hifigan_internal.h), shared by the inference path (hifigan.hip) and the training
// path (hifigan_train.hip).  BWD = false is the forward layer.  BWD = true is a data gradient: the same windowed product with dY as the
// operand and the transposed weights, no bias, and the epilogue of the backward - times lrelu'(tape value), plus the gradients that
// bypass the convolution, over the number of residual blocks.  Every translation unit instantiates what it launches.
#pragma once
#include "hifigan_internal.h"

namespace gvx_hg {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int HG_LD = 36;    // floats per LDS row of a 32-deep k-tile: the fragment reads of sixteen lanes fall on distinct 16-byte slots
constexpr int HG_BM = 128;   // positions per workgroup
constexpr int HG_A_PASS = (HG_BM + GVX_HIFIGAN_MAX_WINDOW + 31) / 32;   // 32 window rows per pass of the 256 threads
inline size_t hg_lds_bytes(int halo, int BN) { return (size_t)2 * (HG_BM + halo + BN) * HG_LD * sizeof(float); }

__device__ __forceinline__ float hg_finish(const HgLayer& p, float v, const float* res, float* o) {
    if (res) v += *res;
    if (p.accumulate) v = *o + v;
    if (p.divide > 0.f) v = v / p.divide;
    return v;
}

// a data gradient's element `at` of [B][len][Cout]: the product through lrelu'(tape value) - decided by `v > 0`, as hg_lrelu decides -
// plus what reaches the tensor past the convolution
__device__ __forceinline__ float hg_finish_bwd(const HgLayer& p, float v, size_t at) {
    if (p.mask) v = p.mask[at] > 0.f ? v : v * p.slope;
    if (p.res) v += p.res[at];
    if (p.add2) v += p.add2[at];
    if (p.divide > 0.f) v = v / p.divide;
    return v;
}

template <int WR, int WC, int TM, int TN, bool BWD = false>
__global__ void __launch_bounds__(256) hg_mfma_kernel(const HgLayer p) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32, B_V4 = BN / 32;
    static_assert(WR * WC == 4 && BM == HG_BM, "four waves, 128 positions");
    extern __shared__ __attribute__((aligned(16))) float hg_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / WC, wc = wave % WC, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z;
    const int n_tiles = (p.Cout + BN - 1) / BN;
    const int nt = (int)blockIdx.y % n_tiles, phase = (int)blockIdx.y / n_tiles;
    const int q0 = (int)blockIdx.x * BM, n0 = nt * BN;
    const int Lmax = p.T * p.in_mul;
    const int len = gen_frames(p.lens, b, p.T) * p.in_mul;
    float* out_b = p.out + (size_t)b * Lmax * p.phases * p.Cout;
    if (q0 >= len) {   // nothing of this row here
        if (p.zero_tail) {
            const int rows = min(BM, Lmax - q0), cols = min(BN, p.Cout - n0);
            for (int i = tid; i < rows * cols; i += 256) {
                const int q = q0 + i / cols, n = n0 + i % cols;
                out_b[((size_t)q * p.phases + phase) * p.Cout + n] = 0.f;
            }
        }
        return;
    }
    const HgTaps tp = hg_taps(p.taps, p.dil, p.phases, phase);
    const int win = BM + tp.halo;              // window rows: source positions q0 - left .. q0 - left + win - 1
    float* As = hg_smem;                       // [2][win][HG_LD]
    float* Bs = hg_smem + 2 * win * HG_LD;     // [2][BN][HG_LD]
    const float* src_b = p.src + (size_t)b * Lmax * p.Cin;

    const int ld_row = tid >> 3, ld_c4 = tid & 7;
    const float* w_row[B_V4];
#pragma unroll
    for (int i = 0; i < B_V4; ++i) {
        const int n = n0 + ld_row + 32 * i;
        w_row[i] = p.W + ((size_t)phase * p.Cout + (n < p.Cout ? n : 0)) * p.K;   // columns past Cout read row 0 and are never stored
    }
    float4 a_reg[HG_A_PASS], b_reg[B_V4];
    int a_keep = 0;               // bit i: a_reg[i] lies inside the row and inside the channels
    bool a_c_ok = false, b_c_ok = false;

    // global -> registers; what is zeroed is decided here and applied, with the activation, at the LDS stores, so that nothing waits
    // for the loads while the products of the current tile run
#define HG_LOAD_A(CB)                                                                                                \
    {                                                                                                                \
        const int c_ = 32 * (CB) + 4 * ld_c4;                                                                        \
        a_c_ok = c_ < p.Cin;                                                                                         \
        const float* s_ = src_b + (a_c_ok ? c_ : 0);                                                                 \
        a_keep = 0;                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < HG_A_PASS; ++i) {                                                      \
            const int w_ = ld_row + 32 * i;                                                                          \
            if (w_ < win) {                                                                                          \
                const int pos_ = q0 - tp.left + w_;                                                                  \
                const bool in_ = pos_ >= 0 && pos_ < len;                                                            \
                a_keep |= (int)(in_ && a_c_ok) << i;                                                                 \
                a_reg[i] = *reinterpret_cast<const float4*>(s_ + (size_t)(in_ ? pos_ : 0) * p.Cin);                  \
            }                                                                                                        \
        }                                                                                                            \
    }
#define HG_STORE_A(BUF)                                                                                              \
    {                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < HG_A_PASS; ++i) {                                                      \
            const int w_ = ld_row + 32 * i;                                                                          \
            if (w_ < win) {                                                                                          \
                const bool keep_ = (a_keep >> i) & 1;                                                                \
                float4 v_ = a_reg[i];                                                                                \
                if (p.act) v_ = make_float4(hg_lrelu(v_.x, p.slope), hg_lrelu(v_.y, p.slope), hg_lrelu(v_.z, p.slope), hg_lrelu(v_.w, p.slope)); \
                *reinterpret_cast<float4*>(&As[((BUF) * win + w_) * HG_LD + 4 * ld_c4]) =                            \
                    make_float4(keep_ ? v_.x : 0.f, keep_ ? v_.y : 0.f, keep_ ? v_.z : 0.f, keep_ ? v_.w : 0.f);     \
            }                                                                                                        \
        }                                                                                                            \
    }
#define HG_LOAD_B(TAU, CB)                                                                                           \
    {                                                                                                                \
        const int c_ = 32 * (CB) + 4 * ld_c4;                                                                        \
        b_c_ok = c_ < p.Cin;                                                                                         \
        const int k_ = b_c_ok ? (TAU) * p.Cin + c_ : 0;                                                              \
        _Pragma("unroll") for (int i = 0; i < B_V4; ++i) b_reg[i] = *reinterpret_cast<const float4*>(w_row[i] + k_); \
    }
#define HG_STORE_B(BUF)                                                                                              \
    {                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < B_V4; ++i)                                                             \
            *reinterpret_cast<float4*>(&Bs[((BUF) * BN + ld_row + 32 * i) * HG_LD + 4 * ld_c4]) =                    \
                make_float4(b_c_ok ? b_reg[i].x : 0.f, b_c_ok ? b_reg[i].y : 0.f, b_c_ok ? b_reg[i].z : 0.f, b_c_ok ? b_reg[i].w : 0.f); \
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int n_it = ((p.Cin + 31) / 32) * p.taps;   // (channel block, tap) pairs, the tap fastest
    HG_LOAD_A(0)
    HG_LOAD_B(0, 0)
    HG_STORE_A(0)
    HG_STORE_B(0)
    __syncthreads();
    int tau = 0, cb = 0;
    for (int it = 0; it < n_it; ++it) {
        int ntau = tau + 1, ncb = cb;
        if (ntau == p.taps) { ntau = 0; ++ncb; }
        const bool more = it + 1 < n_it, new_a = more && ntau == 0;
        if (more) HG_LOAD_B(ntau, ncb)
        if (new_a) HG_LOAD_A(ncb)
        const float* a_base = &As[((cb & 1) * win + tp.off0 + tau * tp.step + wr * TM * 32 + r) * HG_LD + 4 * h];
        const float* b_base = &Bs[((it & 1) * BN + wc * TN * 32 + r) * HG_LD + 4 * h];
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4*>(a_base + i * 32 * HG_LD + 8 * kg);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const float4*>(b_base + j * 32 * HG_LD + 8 * kg);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
                }
        }
        if (more) HG_STORE_B((it + 1) & 1)
        if (new_a) HG_STORE_A(ncb & 1)
        __syncthreads();
        tau = ntau;
        cb = ncb;
    }
#undef HG_LOAD_A
#undef HG_STORE_A
#undef HG_LOAD_B
#undef HG_STORE_B

    // epilogue: lane (r, h) holds column r of rows (e & 3) + 8 (e >> 2) + 4 h of every 32 x 32 tile
    const float* res_b = p.res ? p.res + (size_t)b * Lmax * p.Cout : nullptr;   // a residual comes with phases = 1 only
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + (wc * TN + j) * 32 + r;
        if (col >= p.Cout) continue;
        float bias = 0.f;
        if constexpr (!BWD) bias = p.bias[col];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int q = q0 + (wr * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                float* o = out_b + ((size_t)q * p.phases + phase) * p.Cout + col;
                if constexpr (BWD) {   // phases = 1
                    if (q < len) *o = hg_finish_bwd(p, acc[i][j][e], ((size_t)b * Lmax + q) * p.Cout + col);
                } else {
                    if (q < len) *o = hg_finish(p, acc[i][j][e] + bias, res_b ? res_b + (size_t)q * p.Cout + col : nullptr, o);
                    else if (p.zero_tail && q < Lmax) *o = 0.f;
                }
            }
    }
}

// G lanes per output element (position, channel), channel fastest; the G partial sums are added by shuffles.
template <int G, bool BWD = false>
__global__ void __launch_bounds__(256) hg_valu_kernel(const HgLayer p) {
    const int b = blockIdx.z, phase = blockIdx.y;
    const int Lmax = p.T * p.in_mul;
    const int len = gen_frames(p.lens, b, p.T) * p.in_mul;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int g = (int)(idx % G);
    const long e = idx / G;
    const int n = (int)(e % p.Cout);
    const long ql = e / p.Cout;
    const bool inside = ql < Lmax, live = ql < len;
    const int q = (int)ql;
    float sum = 0.f;
    if (live) {
        const HgTaps tp = hg_taps(p.taps, p.dil, p.phases, phase);
        const float* w = p.W + ((size_t)phase * p.Cout + n) * p.K;
        for (int tau = 0; tau < p.taps; ++tau) {
            const int pos = q - tp.left + tp.off0 + tau * tp.step;
            if (pos < 0 || pos >= len) continue;
            const float* x = p.src + ((size_t)b * Lmax + pos) * p.Cin;
            const float* wt = w + tau * p.Cin;
            for (int c = g; c < p.Cin; c += G) {
                float v = x[c];
                if (p.act) v = hg_lrelu(v, p.slope);
                sum = fmaf(v, wt[c], sum);
            }
        }
    }
#pragma unroll
    for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (g == 0 && inside) {
        float* o = p.out + (((size_t)b * Lmax + q) * p.phases + phase) * p.Cout + n;
        if constexpr (BWD) {
            if (live) *o = hg_finish_bwd(p, sum, ((size_t)b * Lmax + q) * p.Cout + n);
        } else if (live) {
            float v = hg_finish(p, sum + p.bias[n], p.res ? p.res + ((size_t)b * Lmax + q) * p.Cout + n : nullptr, o);
            if (p.tanh_out) v = tanhf(v);
            *o = v;
        } else if (p.zero_tail) {
            *o = 0.f;
        }
    }
}

}  // namespace gvx_hg
