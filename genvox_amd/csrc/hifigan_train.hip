// HiFi-GAN generator training: the forward that keeps a tape, and the backward (include/genvox_amd.h, "HiFi-GAN generator: training";
// the forward's definition and launches are in hifigan.hip, its kernels in hifigan_kernels.h).  gvx_hifigan_forward_train launches the
// forward's own kernels, every layer into its own tape slot, so the waveform has gvx_hifigan_forward's bits.  The backward walks the
// layers in reverse.  Every layer is, or is written as, a zero-padded convolution over channels-last rows
//
//     Y[q][n] = bias[n] + sum over taps tau, channels c of  act(src[q - left + tau d][c]) W[n][tau Cin + c]
//
// - a transposed convolution of stride r as the 3-tap convolution (left = 1, d = 1) from its input [len][Cin] to its output read as
// [len][r Cout]: output r q + phase is column phase Cout + n of row q, and a quarter of each outer tap's weights is structurally zero.
// With dY at hand a layer runs three things, all deterministic (no float atomics) and all confined to a row's own length:
//
//   data gradient    hg_mfma_kernel<.., BWD> (Cin >= 32) / hg_valu_kernel<1, BWD>: the forward's own windowed product with dY as the
//                    operand and Wt[c][tau' Cout + n] = W[n][(k - 1 - tau') Cin + c]; the epilogue multiplies by lrelu'(tape value) -
//                    `v > 0`, as hg_lrelu decides - adds the gradient that bypasses the convolution (the residual path, and the other
//                    blocks' share of d x at a block's first convolution) and divides by n_k where the tensor is a stage's average;
//   weight gradient  hgb_wgrad_mfma_kernel (Cout >= 32) / hgb_wgrad_valu_kernel: dW[n][tau Cin + c] = sum over positions of dY[q][n] *
//                    act(src[q - left + tau d][c]).  Every row is cut into pieces of HGB_PIECE positions; a workgroup owns one piece,
//                    32 TM output channels and 32 input channels, loads 64 positions of dY and the 64 + (k - 1) d rows of the
//                    activated source window into LDS at a time, and runs every tap off a row offset in that window, the taps dealt to
//                    its four waves; its partial product goes to the workspace;
//   bias gradient    column sums of dY over the same pieces: made by the matrix weight-gradient kernel from the dY tiles it holds in LDS
//                    anyway, by hgb_colsum_kernel for the dot-product layers and ups.<i>;
//   hgb_reduce_kernel adds the pieces in their order and writes PyTorch's layout (un-packing the 3-tap form of a transposed
//   convolution and the padded channels of conv_pre).
//
// The transposed weights come from the bound blob at the start of every backward call (hgb_transpose_kernel), so they are the weights
// the forward used.  Order of this file: descriptions, kernels, plans (tape, workspace), launches, the C ABI.
#include "gen_backward.h"
#include "hifigan_kernels.h"

using gvx::fail;
using namespace gvx_hg;

namespace {

constexpr int HGB_PIECE = 512;   // positions per partial product of a weight or bias gradient; a piece lies inside one row
constexpr int HGB_TP = 64;       // positions per LDS tile of the weight gradient
constexpr int HGB_WIN = HGB_TP + GVX_HIFIGAN_MAX_WINDOW;   // rows of its source window
constexpr int HGB_MAX_TAPS = 12; // four waves x three taps
constexpr long HGB_MAX_PIECES = GVX_HIFIGAN_MAX_TRAIN_PIECES;   // of one layer: a grid dimension

struct HgbW {   // one weight gradient
    const float* dy; int ldy;    // [B][T * mul][ldy], Cout columns used
    const float* src;            // [B][T * mul][Cin], raw
    float* part;                 // [pieces][Cout][taps * Cin]
    float* part_b;               // [pieces][Cout]: the piece's column sums of dy (the bias gradient's pieces), or nullptr; matrix kernel only
    const int32_t* lens;
    int T, mul, ppr;             // ppr pieces per row
    int Cin, Cout, taps, dil, left;
    int act; float slope;
};

// A workgroup: one piece, 32 TM columns of dY from n0, source channels c0 .. c0 + 31, every tap.  Wave w owns taps w, w + 4, w + 8.
template <int TM>
__global__ void __launch_bounds__(256, 2) hgb_wgrad_mfma_kernel(const HgbW p) {
    constexpr int BMN = 32 * TM, LDA = BMN == 32 ? 32 : BMN + 32, A_V4 = BMN / 4;   // row strides of 32 mod 64 floats: the two half-waves fall on different banks
    __shared__ __attribute__((aligned(16))) float Ad[HGB_TP * LDA];
    __shared__ __attribute__((aligned(16))) float Sw[HGB_WIN * 32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int piece = blockIdx.x, n0 = (int)blockIdx.y * BMN, c0 = (int)blockIdx.z * 32;
    const int b = piece / p.ppr, q_base = (piece - b * p.ppr) * HGB_PIECE;
    const int Lmax = p.T * p.mul;
    const int len = gen_frames(p.lens, b, p.T) * p.mul;
    const int K = p.taps * p.Cin;
    const int win = HGB_TP + (p.taps - 1) * p.dil;
    const float* src_b = p.src + (size_t)b * Lmax * p.Cin;
    const float* dy_b = p.dy + (size_t)b * Lmax * p.ldy;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);

    // global -> registers for the tile at QS; what is zeroed is decided here and applied, with the activation, at the LDS stores, so
    // that nothing waits for the loads while the products of the current tile run
    constexpr int SW_PASS = (HGB_WIN * 8 + 255) / 256, AD_PASS = HGB_TP * A_V4 / 256;
    float4 sw_reg[SW_PASS], ad_reg[AD_PASS];
    int sw_keep = 0, ad_keep = 0;
#define HGB_LOAD(QS)                                                                                                 \
    {                                                                                                                \
        sw_keep = 0;                                                                                                 \
        ad_keep = 0;                                                                                                 \
        _Pragma("unroll") for (int j_ = 0; j_ < SW_PASS; ++j_) {   /* source positions QS - left .. QS - left + win - 1 */ \
            const int i_ = tid + 256 * j_, w_ = i_ >> 3, c_ = c0 + 4 * (i_ & 7), pos_ = (QS) - p.left + w_;          \
            const bool ok_ = w_ < win && pos_ >= 0 && pos_ < len && c_ < p.Cin;                                      \
            sw_keep |= (int)ok_ << j_;                                                                               \
            sw_reg[j_] = *reinterpret_cast<const float4*>(src_b + (ok_ ? (size_t)pos_ * p.Cin + c_ : 0));            \
        }                                                                                                            \
        _Pragma("unroll") for (int j_ = 0; j_ < AD_PASS; ++j_) {                                                     \
            const int i_ = tid + 256 * j_, row_ = i_ / A_V4, n_ = n0 + 4 * (i_ - row_ * A_V4), q_ = (QS) + row_;     \
            const bool ok_ = q_ < len && n_ < p.Cout;                                                                \
            ad_keep |= (int)ok_ << j_;                                                                               \
            ad_reg[j_] = *reinterpret_cast<const float4*>(dy_b + (ok_ ? (size_t)q_ * p.ldy + n_ : 0));               \
        }                                                                                                            \
    }
#define HGB_STORE()                                                                                                  \
    {                                                                                                                \
        _Pragma("unroll") for (int j_ = 0; j_ < SW_PASS; ++j_) {                                                     \
            const int i_ = tid + 256 * j_, w_ = i_ >> 3;                                                             \
            if (w_ < win) {                                                                                          \
                float4 v_ = sw_reg[j_];                                                                              \
                if (p.act) v_ = make_float4(hg_lrelu(v_.x, p.slope), hg_lrelu(v_.y, p.slope), hg_lrelu(v_.z, p.slope), hg_lrelu(v_.w, p.slope)); \
                *reinterpret_cast<float4*>(&Sw[w_ * 32 + 4 * (i_ & 7)]) = ((sw_keep >> j_) & 1) ? v_ : zero4;        \
            }                                                                                                        \
        }                                                                                                            \
        _Pragma("unroll") for (int j_ = 0; j_ < AD_PASS; ++j_) {                                                     \
            const int i_ = tid + 256 * j_, row_ = i_ / A_V4;                                                         \
            *reinterpret_cast<float4*>(&Ad[row_ * LDA + 4 * (i_ - row_ * A_V4)]) = ((ad_keep >> j_) & 1) ? ad_reg[j_] : zero4; \
        }                                                                                                            \
    }

    f32x16 acc[3][TM];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][i][e] = 0.f;

    // the bias gradient's piece: the workgroups of the first channel block, on the wave with the fewest taps
    const bool do_bias = p.part_b && blockIdx.z == 0 && wave == 3 && lane < BMN;
    float b_sum = 0.f;

    // the piece's tiles that begin inside the row; the rest of the piece lies behind it
    const int n_st = min(HGB_PIECE / HGB_TP, (len - q_base + HGB_TP - 1) / HGB_TP);
    if (n_st > 0) HGB_LOAD(q_base)
    for (int st = 0; st < n_st; ++st) {
        __syncthreads();   // the previous tile has been read
        HGB_STORE()
        __syncthreads();
        if (st + 1 < n_st) HGB_LOAD(q_base + (st + 1) * HGB_TP)
        if (do_bias) {   // the tile's column sums, from the dY tile that is in LDS anyway
            float t_sum = 0.f;
#pragma unroll 8
            for (int row = 0; row < HGB_TP; ++row) t_sum += Ad[row * LDA + lane];
            b_sum += t_sum;
        }
#pragma unroll 4
        for (int ks = 0; ks < HGB_TP / 2; ++ks) {
            float a[TM];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = Ad[(2 * ks + h) * LDA + i * 32 + r];
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int tau = wave + 4 * t;
                if (tau < p.taps) {
                    const float bv = Sw[(2 * ks + h + tau * p.dil) * 32 + r];
#pragma unroll
                    for (int i = 0; i < TM; ++i) acc[t][i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], bv, acc[t][i], 0, 0, 0);
                }
            }
        }
    }
#undef HGB_LOAD
#undef HGB_STORE

    // lane (r, h) holds source channel c0 + r against dY columns (e & 3) + 8 (e >> 2) + 4 h of every 32 x 32 tile
    if (do_bias && n0 + lane < p.Cout) p.part_b[(size_t)piece * p.Cout + n0 + lane] = b_sum;
    const int c = c0 + r;
    if (c >= p.Cin) return;
    float* out = p.part + (size_t)piece * p.Cout * K;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int tau = wave + 4 * t;
        if (tau >= p.taps) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int n = n0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (n < p.Cout) out[(size_t)n * K + tau * p.Cin + c] = acc[t][i][e];
            }
    }
}

// one thread per element of a piece's partial product
__global__ void __launch_bounds__(256) hgb_wgrad_valu_kernel(const HgbW p) {
    const int piece = blockIdx.x;
    const int K = p.taps * p.Cin;
    const long idx = (long)blockIdx.y * 256 + threadIdx.x;
    const long per_piece = (long)p.Cout * K;
    if (idx >= per_piece) return;
    const int k = (int)(idx % K), n = (int)(idx / K);
    const int tau = k / p.Cin, c = k - tau * p.Cin;
    const int b = piece / p.ppr, q_base = (piece - b * p.ppr) * HGB_PIECE;
    const int Lmax = p.T * p.mul;
    const int len = gen_frames(p.lens, b, p.T) * p.mul;
    const int q_end = min(q_base + HGB_PIECE, len);
    const float* src_b = p.src + (size_t)b * Lmax * p.Cin + c;
    const float* dy_b = p.dy + (size_t)b * Lmax * p.ldy + n;
    float sum = 0.f;
    for (int q = q_base; q < q_end; ++q) {
        const int pos = q - p.left + tau * p.dil;
        if (pos < 0 || pos >= len) continue;
        float v = src_b[(size_t)pos * p.Cin];
        if (p.act) v = hg_lrelu(v, p.slope);
        sum = fmaf(dy_b[(size_t)q * p.ldy], v, sum);
    }
    p.part[(size_t)piece * per_piece + idx] = sum;
}

// part[piece][n] = sum over the piece's positions (inside the row) of dy[position][n]; G = 256 / N groups of positions are added in
// their order through LDS
__global__ void __launch_bounds__(256) hgb_colsum_kernel(const float* dy, int N, const int32_t* lens, int T, int mul, int ppr, float* part) {
    __shared__ float red[256];
    const int piece = blockIdx.x, tid = threadIdx.x;
    const int b = piece / ppr, q_base = (piece - b * ppr) * HGB_PIECE;
    const int Lmax = T * mul;
    const int len = gen_frames(lens, b, T) * mul;
    const int count = min(HGB_PIECE, len - q_base);   // <= 0: the piece lies behind the row
    const float* dy_p = dy + ((size_t)b * Lmax + q_base) * N;
    float* out = part + (size_t)piece * N;
    const int G = N >= 256 ? 1 : 256 / N;
    const int g = tid / N, n_first = tid - g * N;
    for (int n = n_first; n < N; n += 256) {   // more than one pass only where N > 256 (then G = 1)
        float sum = 0.f;
        if (g < G) {
#pragma unroll 8
            for (int i = g; i < count; i += G) sum += dy_p[(size_t)i * N + n];   // unrolled: the loads of eight steps are in flight together
        }
        if (G == 1) {
            if (g == 0) out[n] = sum;
        } else {
            red[tid] = sum;
            __syncthreads();
            if (g == 0) {
                for (int j = 1; j < G; ++j) sum += red[j * N + n];
                out[n] = sum;
            }
        }
    }
}

// dst (PyTorch layout) = the pieces added in a fixed order.  A workgroup owns 32 elements of a piece's partial product, in the partial
// product's own order so that the reads are contiguous; each of its 8 groups of threads adds every eighth piece in order, and the eight
// sums are added in theirs.  `count` elements are walked:
//   kind 0  Conv1d [Cout][Cin][k] from part[n][tau * Cp + c], count = Cout * k * Cin (a bias: Cin = Cp = k = 1)
//   kind 1  ConvTranspose1d [Cin][Cout][2 r] (k = 2 r) from the 3-tap form part[phase * Cout + n][tau * Cin + c], count = r * Cout * 3 * Cin:
//           kernel tap phase + r / 2 + r (1 - tau); the quarter of the taps outside [0, 2 r) belongs to no weight
__global__ void __launch_bounds__(256) hgb_reduce_kernel(const float* part, int pieces, size_t piece_stride, float* dst, long count, int kind, int Cout,
                                                          int Cin, int Cp, int k) {
    __shared__ float red[256];
    const int tid = threadIdx.x, e = tid & 31, g = tid >> 5;
    const long idx = (long)blockIdx.x * 32 + e;
    size_t src = 0;
    long to = -1;
    if (idx < count) {
        if (kind == 0) {
            const int c = (int)(idx % Cin), tau = (int)((idx / Cin) % k), n = (int)(idx / ((long)Cin * k));
            src = ((size_t)n * k + tau) * Cp + c;
            to = ((long)n * Cin + c) * k + tau;
        } else {
            const int r = k / 2;
            const int c = (int)(idx % Cin), tau = (int)((idx / Cin) % 3), n = (int)((idx / (3l * Cin)) % Cout), phase = (int)(idx / (3l * Cin * Cout));
            const int tap = phase + r / 2 + r * (1 - tau);
            src = (size_t)idx;
            if (tap >= 0 && tap < k) to = ((long)c * Cout + n) * k + tap;
        }
    }
    float sum = 0.f;
    if (to >= 0) {
#pragma unroll 8
        for (int i = g; i < pieces; i += 8) sum += part[(size_t)i * piece_stride + src];   // unrolled: eight loads in flight together
    }
    red[tid] = sum;
    __syncthreads();
    if (g == 0 && to >= 0) {
        for (int j = 1; j < 8; ++j) sum += red[j * 32 + e];
        dst[to] = sum;
    }
}

// The blob's K-contiguous weights, transposed (and the taps reversed) for the data gradients; one thread per element of dst.
//   kind 0  W[n][tau * Cin + c] -> Wt[c][(taps - 1 - tau) * Cout + n]
//   kind 1  the r two-tap phases Wp[phase][n][tau * Cin + c] -> the 3-tap form Wt[c][tau' * r Cout + phase * Cout + n] (taps = r): output
//           row s - 1 + tau' reaches input s through the phase's tap 0 (tau' = 1), through tap 1 of a phase < r / 2 (tau' = 2, its input
//           q - 1) or of a phase >= r / 2 (tau' = 0, its input q + 1); the other half of taps 0 and 2 is zero
__global__ void __launch_bounds__(256) hgb_transpose_kernel(float* dst, const float* src, int kind, int Cout, int Cin, int taps) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (kind == 0) {
        if (idx >= (long)Cin * taps * Cout) return;
        const int n = (int)(idx % Cout), tau = (int)((idx / Cout) % taps), c = (int)(idx / ((long)Cout * taps));
        dst[idx] = src[(size_t)n * taps * Cin + (size_t)(taps - 1 - tau) * Cin + c];
    } else {
        const int r = taps, half = r / 2;
        if (idx >= (long)Cin * 3 * r * Cout) return;
        const int n = (int)(idx % Cout), phase = (int)((idx / Cout) % r), tau3 = (int)((idx / ((long)Cout * r)) % 3), c = (int)(idx / (3l * Cout * r));
        int tau = -1;
        if (tau3 == 1) tau = 0;
        else if (tau3 == 2 ? phase < half : phase >= half) tau = 1;
        dst[idx] = tau < 0 ? 0.f : src[((size_t)phase * Cout + n) * 2 * Cin + (size_t)tau * Cin + c];
    }
}

// ---- plans
struct HgTape {
    std::vector<GenTapeSlot> slots;
    // indices into slots: mel 0, conv_pre 1, per stage ups' output, per (block, dilation) the inner tensor (resblock 1) and the running
    // value after the dilation (every dilation but the last), the stage's average
    int up[GVX_HIFIGAN_MAX_STAGES], avg[GVX_HIFIGAN_MAX_STAGES];
    int inner[GVX_HIFIGAN_MAX_STAGES][GVX_HIFIGAN_MAX_RESBLOCKS][GVX_HIFIGAN_MAX_DILATIONS];
    int run[GVX_HIFIGAN_MAX_STAGES][GVX_HIFIGAN_MAX_RESBLOCKS][GVX_HIFIGAN_MAX_DILATIONS];
    size_t floats;
};

HgTape hgb_tape_plan(const gvx_hifigan_dims& d, int B, int T) {
    HgTape t{};
    size_t at = 0;
    auto take = [&](int mul, int C) {
        t.slots.push_back({at, mul, C});
        at += (size_t)B * T * mul * C;
        return (int)t.slots.size() - 1;
    };
    int C = d.upsample_initial_channel, mul = 1;
    take(1, hg_cpad(d));
    take(1, C);
    for (int i = 0; i < d.n_stages; ++i) {
        mul *= d.upsample_rates[i];
        C /= 2;
        t.up[i] = take(mul, C);
        for (int j = 0; j < d.n_resblocks; ++j)
            for (int m = 0; m < d.n_dilations; ++m) {
                t.inner[i][j][m] = d.resblock == 1 ? take(mul, C) : -1;
                t.run[i][j][m] = m < d.n_dilations - 1 ? take(mul, C) : -1;
            }
        t.avg[i] = take(mul, C);
    }
    t.floats = at;
    return t;
}

bool hgb_shape_ok(const gvx_hifigan_dims* dims, int B, int T) {
    return !hg_dims_problem(dims) && B >= 1 && B <= 65535 && T >= 1 && T <= GVX_HIFIGAN_MAX_FRAMES;
}

inline int hgb_ppr(int T, int mul) { return (int)(((long)T * mul + HGB_PIECE - 1) / HGB_PIECE); }

// where each layer's transposed weights start: the blob's own plan with the 3-tap form of the transposed convolutions
HgBlob hgb_wt_layout(const gvx_hifigan_dims& d) {
    HgBlob L{};
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t o = at; at += gvx::round64(floats); return o; };
    size_t C = d.upsample_initial_channel;
    L.pre_w = take(C * 7 * hg_cpad(d));
    for (int i = 0; i < d.n_stages; ++i) {
        const size_t Cn = C / 2;
        L.up_w[i] = take(C * 3 * d.upsample_rates[i] * Cn);
        for (int j = 0; j < d.n_resblocks; ++j)
            for (int m = 0; m < d.n_dilations; ++m)
                for (int v = 0; v < hg_convs_per_dilation(d); ++v) L.conv_w[i][j][m][v] = take(Cn * d.resblock_kernel_sizes[j] * Cn);
        C = Cn;
    }
    L.post_w = take(7 * C);
    L.total = at;
    return L;
}

struct HgbWs {   // byte offsets, each a multiple of 256
    size_t wt, wav, dz, g[5], part, part_b, total;
    HgBlob wt_at;
};

HgbWs hgb_ws_plan(const gvx_hifigan_dims& d, int B, int T) {
    HgbWs w{};
    w.wt_at = hgb_wt_layout(d);
    size_t widest = std::max<size_t>(d.upsample_initial_channel, hg_cpad(d)), part = 0, part_b = 0, mul = 1, C = d.upsample_initial_channel;
    int k_max = 0;
    for (int j = 0; j < d.n_resblocks; ++j) k_max = std::max(k_max, (int)d.resblock_kernel_sizes[j]);
    auto need = [&](size_t m, size_t Cout, size_t K) {
        const size_t pieces = (size_t)B * hgb_ppr(T, (int)m);
        part = std::max(part, pieces * Cout * K);   // the pieces of hgb_colsum_kernel take less: K = 1
        part_b = std::max(part_b, pieces * Cout);
    };
    need(1, C, 7 * (size_t)hg_cpad(d));
    for (int i = 0; i < d.n_stages; ++i) {
        const size_t Cn = C / 2, r = d.upsample_rates[i];
        need(mul, r * Cn, 3 * C);
        mul *= r;
        need(mul, Cn, k_max * Cn);
        widest = std::max(widest, mul * Cn);
        C = Cn;
    }
    need(mul, 1, 7 * C);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += gvx::round256(bytes); return o; };
    w.wt = take(w.wt_at.total * sizeof(float));
    w.wav = take((size_t)B * T * mul * sizeof(float));
    w.dz = take((size_t)B * T * mul * sizeof(float));
    for (int i = 0; i < 5; ++i) w.g[i] = take((size_t)B * T * widest * sizeof(float));
    w.part = take(part * sizeof(float));
    w.part_b = take(part_b * sizeof(float));
    w.total = at;
    return w;
}

// ---- launches
template <int WR, int WC, int TM, int TN>
int hgb_launch_dgrad_mfma(const HgLayer& p, int B, hipStream_t s) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
    static bool ready = false;   // the dynamic LDS size of this instantiation, once per process
    if (!ready) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(hg_mfma_kernel<WR, WC, TM, TN, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)hg_lds_bytes(GVX_HIFIGAN_MAX_WINDOW, BN)));
        ready = true;
    }
    const dim3 grid((unsigned)((p.T * p.in_mul + BM - 1) / BM), (unsigned)((p.Cout + BN - 1) / BN), (unsigned)B);
    hg_mfma_kernel<WR, WC, TM, TN, true><<<grid, 256, hg_lds_bytes(hg_taps(p.taps, p.dil, 1, 0).halo, BN), s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// the data gradient of a layer stated as HgLayer: src = dY, W = the transposed weights, out = dX (phases = 1, no activation, no bias)
int hgb_dgrad(const HgLayer& p, int B, hipStream_t s) {
    if (p.Cout >= 32 && p.Cin % 4 == 0) {   // hg_launch's own split
        if (p.Cout >= 128) return hgb_launch_dgrad_mfma<2, 2, 2, 2>(p, B, s);
        if (p.Cout > 32) return hgb_launch_dgrad_mfma<4, 1, 1, 2>(p, B, s);
        return hgb_launch_dgrad_mfma<4, 1, 1, 1>(p, B, s);
    }
    const long threads = (long)p.T * p.in_mul * p.Cout;
    hg_valu_kernel<1, true><<<dim3((unsigned)((threads + 255) / 256), 1u, (unsigned)B), 256, 0, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// dY x act(src) into the pieces of p.part; `fused_bias`: p.part_b was asked for and holds the bias gradient's pieces
int hgb_wgrad(const HgbW& p, int B, hipStream_t s, bool& fused_bias) {
    const int pieces = B * p.ppr;
    fused_bias = false;
    if (p.Cout >= 32 && p.Cout % 4 == 0 && p.Cin % 4 == 0 && p.ldy % 4 == 0 && p.taps <= HGB_MAX_TAPS) {
        const unsigned cb = (unsigned)((p.Cin + 31) / 32);
        if (p.Cout > 32) hgb_wgrad_mfma_kernel<2><<<dim3((unsigned)pieces, (unsigned)((p.Cout + 63) / 64), cb), 256, 0, s>>>(p);
        else hgb_wgrad_mfma_kernel<1><<<dim3((unsigned)pieces, 1u, cb), 256, 0, s>>>(p);
        fused_bias = p.part_b != nullptr;
    } else {
        const long per_piece = (long)p.Cout * p.taps * p.Cin;
        hgb_wgrad_valu_kernel<<<dim3((unsigned)pieces, (unsigned)((per_piece + 255) / 256)), 256, 0, s>>>(p);
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int hgb_reduce(const float* part, int pieces, size_t piece_stride, float* dst, long count, int kind, int Cout, int Cin, int Cp, int k, hipStream_t s) {
    hgb_reduce_kernel<<<(unsigned)((count + 31) / 32), 256, 0, s>>>(part, pieces, piece_stride, dst, count, kind, Cout, Cin, Cp, k);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// the column sums of dy [B][T * mul][N] into a bias gradient
int hgb_bias(const float* dy, int N, const int32_t* lens, int B, int T, int mul, float* part, float* dst, hipStream_t s) {
    const int ppr = hgb_ppr(T, mul), pieces = B * ppr;
    hgb_colsum_kernel<<<(unsigned)pieces, 256, 0, s>>>(dy, N, lens, T, mul, ppr, part);
    HIP_TRY(hipGetLastError());
    return hgb_reduce(part, pieces, (size_t)N, dst, N, 0, N, 1, 1, 1, s);
}

int hgb_transpose(float* dst, const float* src, int kind, int Cout, int Cin, int taps, hipStream_t s) {
    const long count = kind == 0 ? (long)Cin * taps * Cout : (long)Cin * 3 * taps * Cout;
    hgb_transpose_kernel<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(dst, src, kind, Cout, Cin, taps);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

struct HgbGrads {
    float *pre_w, *pre_b, *post_w, *post_b;
    float *up_w[GVX_HIFIGAN_MAX_STAGES], *up_b[GVX_HIFIGAN_MAX_STAGES];
    float* conv_w[GVX_HIFIGAN_MAX_STAGES][GVX_HIFIGAN_MAX_RESBLOCKS][GVX_HIFIGAN_MAX_DILATIONS][2];
    float* conv_b[GVX_HIFIGAN_MAX_STAGES][GVX_HIFIGAN_MAX_RESBLOCKS][GVX_HIFIGAN_MAX_DILATIONS][2];
};

int hgb_check_call(const gvx_hifigan* h, int B, int T, const void* tape, size_t tape_bytes) {
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (T < 1) return fail(GVX_ERR_INVALID_ARG, "T = %d: a row needs at least 1 frame", T);
    if (T > GVX_HIFIGAN_MAX_FRAMES) return fail(GVX_ERR_UNSUPPORTED, "T = %d is beyond the limit of %d frames", T, GVX_HIFIGAN_MAX_FRAMES);
    return gen_check_tape(tape, tape_bytes, hgb_tape_plan(h->d, B, T).floats * sizeof(float));
}

HgLayer hgb_layer(const gvx_hifigan_dims& d, const int32_t* lens, int T, const float* src, const float* W, const float* bias, float* out, int in_mul,
                  int Cin, int Cout, int taps, int dil, int phases, int act) {
    HgLayer p{};
    p.lens = lens; p.T = T; p.slope = d.slope;
    p.src = src; p.W = W; p.bias = bias; p.out = out;
    p.in_mul = in_mul; p.Cin = Cin; p.Cout = Cout; p.taps = taps; p.K = taps * Cin; p.dil = dil; p.phases = phases; p.act = act;
    return p;
}

}  // namespace

extern "C" {

size_t gvx_hifigan_tape_bytes(const gvx_hifigan_dims* dims, int B, int T) {
    if (!hgb_shape_ok(dims, B, T)) return 0;
    return hgb_tape_plan(*dims, B, T).floats * sizeof(float);
}

int gvx_hifigan_tape_layout(const gvx_hifigan_dims* dims, int B, int T, gvx_hifigan_tape_entry* entries, int max_entries) {
    if (!hgb_shape_ok(dims, B, T)) return 0;
    return gen_tape_layout(hgb_tape_plan(*dims, B, T).slots, entries, max_entries);
}

size_t gvx_hifigan_backward_workspace_bytes(const gvx_hifigan_dims* dims, int B, int T) {
    if (!hgb_shape_ok(dims, B, T)) return 0;
    return hgb_ws_plan(*dims, B, T).total;
}

int gvx_hifigan_forward_train(gvx_hifigan* h, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, void* tape, size_t tape_bytes,
                              void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;   // every intermediate tensor is a tape slot: the call needs no scratch
    if (!h || !mel || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = hgb_check_call(h, B, T, tape, tape_bytes)) != GVX_OK) return rc;
    const gvx_hifigan_dims& d = h->d;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = hg_prepare(&h->lds_ready)) != GVX_OK) return rc;
    const HgTape tp = hgb_tape_plan(d, B, T);
    const HgBlob L = hg_blob_layout(d);
    const float* blob = h->blob;
    float* base = static_cast<float*>(tape);
    auto slot = [&](int i) { return base + tp.slots[i].off; };

    const int Cp = hg_cpad(d);
    if ((rc = hg_mel_transpose(mel, frame_lengths, B, d.n_mels, T, Cp, slot(0), s)) != GVX_OK) return rc;
    // from here on: the layers of gvx_hifigan_forward, argument for argument, but for where they write
    int C = d.upsample_initial_channel, mul = 1;
    const float* cur = slot(1);
    HgLayer p = hgb_layer(d, frame_lengths, T, slot(0), blob + L.pre_w, blob + L.pre_b, slot(1), 1, Cp, C, 7, 1, 1, 0);
    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
    for (int i = 0; i < d.n_stages; ++i) {
        const int Cn = C / 2, r = d.upsample_rates[i];
        float* sum = slot(tp.avg[i]);
        p = hgb_layer(d, frame_lengths, T, cur, blob + L.up_w[i], blob + L.up_b[i], slot(tp.up[i]), mul, C, Cn, 2, 0, r, 1);
        if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
        mul *= r;
        for (int j = 0; j < d.n_resblocks; ++j) {
            const int k = d.resblock_kernel_sizes[j];
            const float* in = slot(tp.up[i]);   // the block's running value
            for (int m = 0; m < d.n_dilations; ++m) {
                const bool last = m == d.n_dilations - 1;
                const int dil = d.resblock_dilation_sizes[j][m];
                const float* conv_in = in;
                int conv_dil = dil, v = 0;
                if (d.resblock == 1) {
                    float* t1 = slot(tp.inner[i][j][m]);
                    p = hgb_layer(d, frame_lengths, T, in, blob + L.conv_w[i][j][m][0], blob + L.conv_b[i][j][m][0], t1, mul, Cn, Cn, k, dil, 1, 1);
                    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
                    conv_in = t1; conv_dil = 1; v = 1;
                }
                float* next = last ? sum : slot(tp.run[i][j][m]);
                p = hgb_layer(d, frame_lengths, T, conv_in, blob + L.conv_w[i][j][m][v], blob + L.conv_b[i][j][m][v], next, mul, Cn, Cn, k, conv_dil, 1, 1);
                p.res = in;
                if (last) {   // y_j goes into the stage's sum, as in gvx_hifigan_forward
                    p.accumulate = j > 0;
                    p.divide = j == d.n_resblocks - 1 ? (float)d.n_resblocks : 0.f;
                }
                if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
                in = next;
            }
        }
        cur = sum;
        C = Cn;
    }
    p = hgb_layer(d, frame_lengths, T, cur, blob + L.post_w, blob + L.post_b, wav_out, mul, C, 1, 7, 1, 1, 1);
    p.slope = d.post_slope; p.tanh_out = 1; p.zero_tail = 1;
    return hg_launch(p, B, s);
}

int gvx_hifigan_backward(gvx_hifigan* h, const float* d_wav, const int32_t* frame_lengths, int B, int T, const void* tape, size_t tape_bytes,
                         const gvx_grad_desc* grads, int n_grads, float* d_mel_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !d_wav || !grads || n_grads < 1) return fail(GVX_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = hgb_check_call(h, B, T, tape, tape_bytes)) != GVX_OK) return rc;
    const gvx_hifigan_dims& d = h->d;
    const HgbWs wp = hgb_ws_plan(d, B, T);
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    const int S = d.n_stages, NK = d.n_resblocks, ND = d.n_dilations, NV = hg_convs_per_dilation(d), Cp = hg_cpad(d);
    int hop = 1, C_last = d.upsample_initial_channel;
    for (int i = 0; i < S; ++i) { hop *= d.upsample_rates[i]; C_last /= 2; }
    if ((long)B * hgb_ppr(T, hop) > HGB_MAX_PIECES)
        return fail(GVX_ERR_UNSUPPORTED, "B * ceil(T * hop / %d) = %ld pieces are beyond %ld", HGB_PIECE, (long)B * hgb_ppr(T, hop), HGB_MAX_PIECES);
    HgbGrads g{};
    {
        size_t C = d.upsample_initial_channel;
        g.pre_w = gen_grad(grads, n_grads, "conv_pre.weight", C * d.n_mels * 7, rc);
        g.pre_b = gen_grad(grads, n_grads, "conv_pre.bias", C, rc);
        for (int i = 0; i < S; ++i) {
            const size_t Cn = C / 2;
            const std::string up = "ups." + std::to_string(i);
            g.up_w[i] = gen_grad(grads, n_grads, up + ".weight", C * Cn * 2 * d.upsample_rates[i], rc);
            g.up_b[i] = gen_grad(grads, n_grads, up + ".bias", Cn, rc);
            for (int j = 0; j < NK; ++j)
                for (int m = 0; m < ND; ++m)
                    for (int v = 0; v < NV; ++v) {
                        const std::string name = hg_conv_name(d, i * NK + j, m, v);
                        g.conv_w[i][j][m][v] = gen_grad(grads, n_grads, name + ".weight", Cn * Cn * d.resblock_kernel_sizes[j], rc);
                        g.conv_b[i][j][m][v] = gen_grad(grads, n_grads, name + ".bias", Cn, rc);
                    }
            C = Cn;
        }
        g.post_w = gen_grad(grads, n_grads, "conv_post.weight", 7 * C, rc);
        g.post_b = gen_grad(grads, n_grads, "conv_post.bias", 1, rc);
        if (rc != GVX_OK) return rc;   // nothing was launched
    }
    hipStream_t s = (hipStream_t)stream;
    if ((rc = hg_prepare(&h->lds_ready)) != GVX_OK) return rc;
    const HgTape tp = hgb_tape_plan(d, B, T);
    const HgBlob L = hg_blob_layout(d);
    const HgBlob& WL = wp.wt_at;
    const float* blob = h->blob;
    const float* tbase = static_cast<const float*>(tape);
    auto slot = [&](int i) { return tbase + tp.slots[i].off; };
    float* wt = gvx::ws_ptr<float>(workspace, wp.wt);
    float* wav = gvx::ws_ptr<float>(workspace, wp.wav);
    float* dz = gvx::ws_ptr<float>(workspace, wp.dz);
    float* gs = gvx::ws_ptr<float>(workspace, wp.g[0]);   // the gradient every block of the stage starts from: d(average) / n_k
    float* dx = gvx::ws_ptr<float>(workspace, wp.g[1]);   // d(ups' output), summed over the blocks
    float* pa = gvx::ws_ptr<float>(workspace, wp.g[2]);   // a block's running gradient, in turns
    float* pb = gvx::ws_ptr<float>(workspace, wp.g[3]);
    float* dt = gvx::ws_ptr<float>(workspace, wp.g[4]);   // d(inner tensor)
    float* part = gvx::ws_ptr<float>(workspace, wp.part);
    float* part_b = gvx::ws_ptr<float>(workspace, wp.part_b);   // bias pieces that a weight-gradient launch makes on its way

    int ev = 0;
    // with gvx_hifigan_timing_enable: the transposes, conv_post, every stage from the last, conv_pre
    auto stamp = [&] { return gen_mark(h, ev++, s, &h->bwd_marks); };
    if ((rc = stamp()) != GVX_OK) return rc;

    // the transposed weights, from the blob the forward read
    {
        int C = d.upsample_initial_channel;
        if ((rc = hgb_transpose(wt + WL.pre_w, blob + L.pre_w, 0, C, Cp, 7, s)) != GVX_OK) return rc;
        for (int i = 0; i < S; ++i) {
            const int Cn = C / 2;
            if ((rc = hgb_transpose(wt + WL.up_w[i], blob + L.up_w[i], 1, Cn, C, d.upsample_rates[i], s)) != GVX_OK) return rc;
            for (int j = 0; j < NK; ++j)
                for (int m = 0; m < ND; ++m)
                    for (int v = 0; v < NV; ++v)
                        if ((rc = hgb_transpose(wt + WL.conv_w[i][j][m][v], blob + L.conv_w[i][j][m][v], 0, Cn, Cn, d.resblock_kernel_sizes[j], s)) != GVX_OK) return rc;
            C = Cn;
        }
        if ((rc = hgb_transpose(wt + WL.post_w, blob + L.post_w, 0, 1, C, 7, s)) != GVX_OK) return rc;
    }
    if ((rc = stamp()) != GVX_OK) return rc;

    // one convolution's weight and bias gradients (kind 0) from dy [B][T * mul][Cout] and its raw source
    auto conv_grads = [&](const float* dy, const float* src, int mul, int Cin, int Cin_true, int Cout, int k, int dil, int act, float slope, float* gw,
                          float* gb) -> int {
        HgbW w{};
        w.dy = dy; w.ldy = Cout; w.src = src; w.part = part; w.part_b = part_b; w.lens = frame_lengths; w.T = T; w.mul = mul; w.ppr = hgb_ppr(T, mul);
        w.Cin = Cin; w.Cout = Cout; w.taps = k; w.dil = dil; w.left = (k - 1) * dil / 2; w.act = act; w.slope = slope;
        int rc_;
        bool fused_bias;
        if ((rc_ = hgb_wgrad(w, B, s, fused_bias)) != GVX_OK) return rc_;
        if ((rc_ = hgb_reduce(part, B * w.ppr, (size_t)Cout * k * Cin, gw, (long)Cout * Cin_true * k, 0, Cout, Cin_true, Cin, k, s)) != GVX_OK) return rc_;
        if (fused_bias) return hgb_reduce(part_b, B * w.ppr, (size_t)Cout, gb, Cout, 0, Cout, 1, 1, 1, s);
        return hgb_bias(dy, Cout, frame_lengths, B, T, mul, part, gb, s);
    };
    auto dgrad = [&](const float* dy, const float* Wt, float* out, int mul, int Cy, int N, int k, int dil, const float* mask, float slope, const float* add,
                     const float* add2, float divide) -> int {
        HgLayer p = hgb_layer(d, frame_lengths, T, dy, Wt, nullptr, out, mul, Cy, N, k, dil, 1, 0);
        p.slope = slope; p.mask = mask; p.res = add; p.add2 = add2; p.divide = divide;
        return hgb_dgrad(p, B, s);
    };

    // conv_post: the waveform again (the forward's own launch), tanh', then the 7-tap convolution over lrelu(x, post_slope)
    {
        const float* x_last = slot(tp.avg[S - 1]);
        HgLayer p = hgb_layer(d, frame_lengths, T, x_last, blob + L.post_w, blob + L.post_b, wav, hop, C_last, 1, 7, 1, 1, 1);
        p.slope = d.post_slope; p.tanh_out = 1;
        if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
        gen_tanh_bwd_kernel<1><<<dim3((unsigned)(((long)T * hop + 255) / 256), (unsigned)B), 256, 0, s>>>(d_wav, wav, frame_lengths, T, hop, dz);
        HIP_TRY(hipGetLastError());
        if ((rc = conv_grads(dz, x_last, hop, C_last, C_last, 1, 7, 1, 1, d.post_slope, g.post_w, g.post_b)) != GVX_OK) return rc;
        if ((rc = dgrad(dz, wt + WL.post_w, gs, hop, 1, C_last, 7, 1, x_last, d.post_slope, nullptr, nullptr, (float)NK)) != GVX_OK) return rc;
    }
    if ((rc = stamp()) != GVX_OK) return rc;

    int C = C_last, mul = hop;   // gs holds d(stage average) / n_k, [B][T * mul][C]
    for (int i = S - 1; i >= 0; --i) {
        const int r = d.upsample_rates[i], Cin = 2 * C, in_mul = mul / r;
        const float* x = slot(tp.up[i]);
        for (int j = 0; j < NK; ++j) {
            const int k = d.resblock_kernel_sizes[j];
            const float* d_next = gs;   // d y_j = d(sum) / n_k whatever y_j's value
            for (int m = ND - 1; m >= 0; --m) {
                const int dil = d.resblock_dilation_sizes[j][m];
                const float* in = m == 0 ? x : slot(tp.run[i][j][m - 1]);
                const float* dy1 = d_next;
                if (d.resblock == 1) {   // next = in + convs2(lrelu(t)), t = convs1(lrelu(in))
                    const float* t = slot(tp.inner[i][j][m]);
                    if ((rc = conv_grads(d_next, t, mul, C, C, C, k, 1, 1, d.slope, g.conv_w[i][j][m][1], g.conv_b[i][j][m][1])) != GVX_OK) return rc;
                    if ((rc = dgrad(d_next, wt + WL.conv_w[i][j][m][1], dt, mul, C, C, k, 1, t, d.slope, nullptr, nullptr, 0.f)) != GVX_OK) return rc;
                    dy1 = dt;
                }
                if ((rc = conv_grads(dy1, in, mul, C, C, C, k, dil, 1, d.slope, g.conv_w[i][j][m][0], g.conv_b[i][j][m][0])) != GVX_OK) return rc;
                // d in = d next + lrelu'(in) * conv^T(dy1); at the block's first convolution `in` is x, which the earlier blocks reached too
                float* out = m == 0 ? dx : (d_next == pa ? pb : pa);
                if ((rc = dgrad(dy1, wt + WL.conv_w[i][j][m][0], out, mul, C, C, k, dil, in, d.slope, d_next, (m == 0 && j > 0) ? dx : nullptr, 0.f)) != GVX_OK)
                    return rc;
                d_next = out;
            }
        }
        // ups.<i> over lrelu(cur), as the 3-tap convolution cur [len][Cin] -> x [len][r C]
        const float* cur = i == 0 ? slot(1) : slot(tp.avg[i - 1]);
        {
            HgbW w{};
            w.dy = dx; w.ldy = r * C; w.src = cur; w.part = part; w.lens = frame_lengths; w.T = T; w.mul = in_mul; w.ppr = hgb_ppr(T, in_mul);
            w.Cin = Cin; w.Cout = r * C; w.taps = 3; w.dil = 1; w.left = 1; w.act = 1; w.slope = d.slope;
            bool unused;   // the bias of the 3-tap form would be per phase: ups' bias sums run on the plain view below
            if ((rc = hgb_wgrad(w, B, s, unused)) != GVX_OK) return rc;
            if ((rc = hgb_reduce(part, B * w.ppr, (size_t)r * C * 3 * Cin, g.up_w[i], (long)r * C * 3 * Cin, 1, C, Cin, Cin, 2 * r, s)) != GVX_OK) return rc;
            if ((rc = hgb_bias(dx, C, frame_lengths, B, T, mul, part, g.up_b[i], s)) != GVX_OK) return rc;
        }
        if ((rc = dgrad(dx, wt + WL.up_w[i], pa, in_mul, r * C, Cin, 3, 1, cur, d.slope, nullptr, nullptr, i > 0 ? (float)NK : 0.f)) != GVX_OK) return rc;
        std::swap(gs, pa);
        C = Cin;
        mul = in_mul;
        if ((rc = stamp()) != GVX_OK) return rc;
    }

    // conv_pre: no activation in front of it; gs holds d(its output)
    if ((rc = conv_grads(gs, slot(0), 1, Cp, d.n_mels, C, 7, 1, 0, d.slope, g.pre_w, g.pre_b)) != GVX_OK) return rc;
    if (d_mel_out) {
        if ((rc = dgrad(gs, wt + WL.pre_w, pb, 1, C, Cp, 7, 1, nullptr, d.slope, nullptr, nullptr, 0.f)) != GVX_OK) return rc;
        gen_dmel_kernel<1><<<dim3((unsigned)(((long)d.n_mels * T + 255) / 256), (unsigned)B), 256, 0, s>>>(pb, frame_lengths, d.n_mels, T, Cp, d_mel_out);
        HIP_TRY(hipGetLastError());
    }
    return stamp();
}

int gvx_hifigan_backward_stage_times_ms(gvx_hifigan* h, float* ms_out, int* n_out) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    return gen_stage_times_ms(h, h->d.n_stages + 3, ms_out, n_out, &h->bwd_marks);
}

// One layer on its own: the arguments fill an HgLayer, hg_launch (forward) or hgb_dgrad (data gradient) picks the kernel as the models'
// layers have it picked.  Everything the kernels take for granted is checked here, before a launch.
int gvx_hifigan_layer(const float* src, const float* W, const float* bias, const float* res, const float* mask, const float* add2, float* out,
                      const int32_t* lens, int B, int T, int in_mul, int Cin, int Cout, int taps, int dil, int phases, int act, int accumulate,
                      float divide, int zero_tail, int tanh_out, float slope, int gradient, void* stream) {
    if (!src || !W || !out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (((uintptr_t)src | (uintptr_t)W | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)mask | (uintptr_t)add2 | (uintptr_t)out) & 15)
        return fail(GVX_ERR_INVALID_ARG, "src, W, bias, res, mask, add2 and out must be 16-byte aligned");
    if ((uintptr_t)lens & 3) return fail(GVX_ERR_INVALID_ARG, "lens must be 4-byte aligned");
    if (out == src) return fail(GVX_ERR_INVALID_ARG, "out must not be src: a position's window reads its neighbours' positions of src");
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (T < 1 || in_mul < 1 || (long)T * in_mul > (1L << 24)) return fail(GVX_ERR_INVALID_ARG, "T and in_mul must be >= 1 and T * in_mul at most 2^24 positions");
    if (Cin < 1 || Cin > 4096 || Cout < 1 || Cout > 4096) return fail(GVX_ERR_INVALID_ARG, "Cin and Cout must be in [1, 4096]");
    if (phases < 1 || phases > 64) return fail(GVX_ERR_INVALID_ARG, "phases must be in [1, 64]");
    if ((long)T * in_mul * Cout > (1L << 28)) return fail(GVX_ERR_INVALID_ARG, "T * in_mul * Cout is beyond 2^28 elements per phase");
    if (phases > 1) {
        if (taps != 2) return fail(GVX_ERR_INVALID_ARG, "phases > 1 is the two-tap phase split: taps must be 2");
        if (phases & 1) return fail(GVX_ERR_INVALID_ARG, "phases > 1 must be even");
        if (res) return fail(GVX_ERR_INVALID_ARG, "a residual comes with phases = 1 only");
    } else {
        if (taps < 1 || !(taps & 1)) return fail(GVX_ERR_INVALID_ARG, "taps must be odd and >= 1 (the window is centred)");
        if (dil < 1) return fail(GVX_ERR_INVALID_ARG, "the dilation must be >= 1");
        if ((long)(taps - 1) * dil > GVX_HIFIGAN_MAX_WINDOW) return fail(GVX_ERR_INVALID_ARG, "(taps - 1) * dilation must not pass GVX_HIFIGAN_MAX_WINDOW (72)");
    }
    if (!(slope >= 0.f && slope <= 1.f)) return fail(GVX_ERR_INVALID_ARG, "slope must be in [0, 1]");
    if (!(divide >= 0.f) || !std::isfinite(divide)) return fail(GVX_ERR_INVALID_ARG, "divide must be finite and >= 0 (0: no division)");
    const bool matrix = Cout >= 32 && Cin % 4 == 0;   // hg_launch's and hgb_dgrad's split; every other layer runs on the dot-product kernel
    if (gradient) {
        if (phases != 1) return fail(GVX_ERR_INVALID_ARG, "a data gradient has phases = 1 (a transposed convolution's is its 3-tap form)");
        if (bias || act || accumulate || zero_tail || tanh_out)
            return fail(GVX_ERR_INVALID_ARG, "a data gradient takes no bias, act, accumulate, zero_tail or tanh_out");
    } else {
        if (!bias) return fail(GVX_ERR_INVALID_ARG, "the forward layer needs a bias");
        if (mask || add2) return fail(GVX_ERR_INVALID_ARG, "mask and add2 belong to the data gradient");
        if (tanh_out && matrix) return fail(GVX_ERR_INVALID_ARG, "tanh_out is the dot-product kernel's: Cout < 32 or Cin not a multiple of 4");
    }
    hipStream_t s = (hipStream_t)stream;
    int rc;
    // no handle: the dynamic-LDS sizes of hg_launch's kernels once per process (a static local: one thread runs it), on the device that is
    // current at the first call; a failure of that first preparation is what every later call returns (as un_lone_prepare, univnet.hip)
    static bool ready = false;
    static const int prepared = hg_prepare(&ready);
    if ((rc = prepared) != GVX_OK) return rc;
    HgLayer p{};
    p.src = src; p.W = W; p.bias = bias; p.res = res; p.out = out; p.lens = lens; p.T = T; p.in_mul = in_mul;
    p.Cin = Cin; p.Cout = Cout; p.K = taps * Cin; p.taps = taps; p.dil = phases > 1 ? 0 : dil; p.phases = phases;
    p.act = act != 0; p.accumulate = accumulate != 0; p.divide = divide; p.zero_tail = zero_tail != 0; p.tanh_out = tanh_out != 0; p.slope = slope;
    p.mask = mask; p.add2 = add2;
    return gradient ? hgb_dgrad(p, B, s) : hg_launch(p, B, s);
}

}  // C ABI
