// MelGAN generator training: the forward that keeps a tape, and the backward (include/genvox_amd.h, "Neural vocoder"; the forward's
// definition and kernels are in melgan.hip).  gvx_melgan_forward_train launches the forward's own kernels, every layer into its own
// tape slot, so the waveform has gvx_melgan_forward's bits.  The backward walks the layers in reverse; for a layer
//
//     Y[phases q + phase][n] = bias[n] + sum over taps tau, channels c of  act_tau(src_tau[row(q, tau, phase)][c]) W[phase][n][tau Cin + c]
//
// with dY [len_out][Cout] at hand it runs three things, all deterministic (no float atomics) and all confined to a row's own length:
//
//   data gradient    mgb_dgrad_mfma_kernel (N = Cin >= 32) / mgb_dgrad_valu_kernel: an implicit GEMM  dX[s][c] = sum_k A[s][k] Wt[c][k],
//                    K = taps * Cout, whose operand A is GATHERED from dY on its way into LDS:
//                      convolution      A[s][tau Cout + n] = dY[s - off_tau][n] + dY[-s - off_tau][n] + dY[2 (len - 1) - s - off_tau][n],
//                                       each term where its position lies in the row (and, for the two mirrored ones, its tap left the
//                                       row: s > 0, s < len - 1) - the transpose of the forward's reflection, as a gather
//                      transposed conv  A[s][k Cout + n] = dY[r s + k - r / 2][n] for the 2 r kernel taps k, zero outside the row
//                      residual tail    one tap: dY[s] against [W_s | W_m], N = 2 C
//                    the epilogue multiplies by lrelu'(tape value) - decided by `v > 0` as mg_lrelu decides it - and adds the shortcut's
//                    gradient (the first C columns of the tail's product) where the layer has one.
//   weight gradient  mgb_wgrad_mfma_kernel (Cout >= 32) / mgb_wgrad_valu_kernel:  dW[phase][n][tau Cin + c] = sum over rows and positions
//                    of dY[phases q + phase][n] * act(src[row(q, tau, phase)][c]): the forward's own operand gather (mg_src_row), the
//                    reduction over the positions of ALL rows laid end to end and cut into pieces of MGB_PIECE positions, one
//                    workgroup per (output tile, piece) writing its partial product to the workspace;
//   bias gradient    mgb_colsum_kernel: column sums of dY over the same pieces;
//   mgb_reduce_kernel adds the pieces in their order and writes the result in PyTorch's layout (un-packing the phases of a transposed
//   convolution and the padded channels of the first convolution).
//
// The transposed weights Wt come from the bound blob at the start of every backward call (mgb_transpose_kernel), so they are the
// weights the forward used.  Order of this file: descriptions, kernels, plans (tape, workspace), launches, the C ABI.
#include "gen_backward.h"
#include "melgan_internal.h"

using gvx::fail;
using namespace gvx_mg;

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int MGB_PIECE = 512;   // positions per partial product of a weight or bias gradient
constexpr int MGB_LD = 36;       // as MG_LD of melgan.hip

struct MgbD {   // one data gradient
    const float* dy; int ldy;      // [B][len_out][ldy], pointing at the first of the Cy columns used
    const float* Wt;               // [N][K], K = taps * Cy
    float* out; int ldo;           // [B][len][ldo]
    const float* mask; int ldm, mask_from;   // raw tape values [B][len][ldm]: columns c >= mask_from are scaled by lrelu'(mask[s][c - mask_from])
    const float* add; int lda;     // [B][len][lda] added after the scaling, or nullptr
    const int32_t* lens;
    int T, in_mul;                 // row b has T_b * in_mul positions of dX
    int N, Cy, K, taps, dil, r;    // r = 0: reflected convolution; r > 0: transposed convolution of stride r (taps = 2 r)
    float slope;
};

struct MgbW {   // one weight gradient: the forward's layer (sources, taps, activation) and its dY
    MgLayer L;
    const float* dy; int ldy;      // [B][len * phases][ldy]
    float* part;                   // [pieces][phases][Cout][K]
    int B;
};

// the up to three positions of dY that input position s receives tap tau from; returns the bits of the valid ones
__device__ __forceinline__ int mgb_rows(const MgbD& p, int s, int tau, int len, int rows[3]) {
    if (p.r > 0) {
        const int o = p.r * s + tau - (p.r >> 1);
        rows[0] = o; rows[1] = rows[2] = 0;
        return (o >= 0 && o < len * p.r) ? 1 : 0;
    }
    const int off = (tau - ((p.taps - 1) >> 1)) * p.dil;
    const int q1 = s - off, q2 = -s - off, q3 = 2 * (len - 1) - s - off;
    int v = (q1 >= 0 && q1 < len) ? 1 : 0;
    v |= (s > 0 && q2 >= 0 && q2 < len) ? 2 : 0;
    v |= (s < len - 1 && q3 >= 0 && q3 < len) ? 4 : 0;
    rows[0] = q1; rows[1] = q2; rows[2] = q3;
    return v;
}

__device__ __forceinline__ float mgb_epilogue(const MgbD& p, float v, size_t pos, int col) {
    if (p.mask && col >= p.mask_from) {
        const float m = p.mask[pos * p.ldm + col - p.mask_from];
        v = m > 0.f ? v : v * p.slope;
    }
    if (p.add) v += p.add[pos * p.lda + col];
    return v;
}

__device__ __forceinline__ float4 mgb_add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// The forward's tile (melgan.hip, mg_mfma_kernel) with the gathered dY as the position operand and Wt as the channel operand.
template <int WR, int WC, int TM, int TN>
__global__ void __launch_bounds__(256) mgb_dgrad_mfma_kernel(const MgbD p) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32, A_V4 = BM / 32, B_V4 = BN / 32;
    static_assert(WR * WC == 4, "four waves");
    extern __shared__ __attribute__((aligned(16))) float mgb_smem[];
    float* As = mgb_smem;                    // [2][BM][MGB_LD]
    float* Bs = mgb_smem + 2 * BM * MGB_LD;  // [2][BN][MGB_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / WC, wc = wave % WC, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z;
    const int s0 = (int)blockIdx.x * BM, n0 = (int)blockIdx.y * BN;
    const int Lmax = p.T * p.in_mul;
    const int len = mg_frames(p.lens, b, p.T) * p.in_mul;
    if (s0 >= len) return;
    const int out_mul = p.r > 0 ? p.r : 1;
    const float* dy_b = p.dy + (size_t)b * Lmax * out_mul * p.ldy;

    const int ld_row = tid >> 3, ld_c4 = tid & 7;
    const float* w_row[B_V4];
#pragma unroll
    for (int i = 0; i < B_V4; ++i) {
        const int n = n0 + ld_row + 32 * i;
        w_row[i] = p.Wt + (size_t)(n < p.N ? n : 0) * p.K;   // columns past N read row 0 and are never stored
    }
    float4 a_reg[3][A_V4], b_reg[B_V4];
    bool k_ok = false;

#define MGB_LOAD(K0)                                                                                                 \
    {                                                                                                                \
        const int k_ = (K0) + 4 * ld_c4;                                                                             \
        k_ok = k_ < p.K;                                                                                             \
        const int kk_ = k_ok ? k_ : 0;                                                                               \
        const int tau_ = kk_ / p.Cy, c_ = kk_ - tau_ * p.Cy;                                                         \
        _Pragma("unroll") for (int i = 0; i < A_V4; ++i) {                                                           \
            int rows_[3];                                                                                            \
            const int s_ = min(s0 + ld_row + 32 * i, len - 1);   /* positions past the row repeat its last one; never stored */ \
            const int v_ = k_ok ? mgb_rows(p, s_, tau_, len, rows_) : 0;                                             \
            _Pragma("unroll") for (int j = 0; j < 3; ++j)                                                            \
                a_reg[j][i] = ((v_ >> j) & 1) ? *reinterpret_cast<const float4*>(dy_b + (size_t)rows_[j] * p.ldy + c_) : make_float4(0.f, 0.f, 0.f, 0.f); \
        }                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < B_V4; ++i) b_reg[i] = *reinterpret_cast<const float4*>(w_row[i] + kk_); \
    }
#define MGB_STORE(BUF)                                                                                               \
    {                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < A_V4; ++i)                                                             \
            *reinterpret_cast<float4*>(&As[((BUF) * BM + ld_row + 32 * i) * MGB_LD + 4 * ld_c4]) =                   \
                mgb_add4(mgb_add4(a_reg[0][i], a_reg[1][i]), a_reg[2][i]);                                           \
        _Pragma("unroll") for (int i = 0; i < B_V4; ++i)                                                             \
            *reinterpret_cast<float4*>(&Bs[((BUF) * BN + ld_row + 32 * i) * MGB_LD + 4 * ld_c4]) =                   \
                make_float4(k_ok ? b_reg[i].x : 0.f, k_ok ? b_reg[i].y : 0.f, k_ok ? b_reg[i].z : 0.f, k_ok ? b_reg[i].w : 0.f); \
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int nk = (p.K + 31) / 32;
    MGB_LOAD(0)
    MGB_STORE(0)
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) MGB_LOAD((kt + 1) * 32)
        const float* a_base = &As[(buf * BM + wr * TM * 32 + r) * MGB_LD + 4 * h];
        const float* b_base = &Bs[(buf * BN + wc * TN * 32 + r) * MGB_LD + 4 * h];
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4*>(a_base + i * 32 * MGB_LD + 8 * kg);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const float4*>(b_base + j * 32 * MGB_LD + 8 * kg);
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
        if (kt + 1 < nk) MGB_STORE(buf ^ 1)
        __syncthreads();
    }
#undef MGB_LOAD
#undef MGB_STORE

    // lane (r, h) holds column r of rows (e & 3) + 8 (e >> 2) + 4 h of every 32 x 32 tile
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + (wc * TN + j) * 32 + r;
        if (col >= p.N) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int s = s0 + (wr * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (s >= len) continue;
                const size_t pos = (size_t)b * Lmax + s;
                p.out[pos * p.ldo + col] = mgb_epilogue(p, acc[i][j][e], pos, col);
            }
    }
}

// one thread per element of dX, channel fastest
__global__ void __launch_bounds__(256) mgb_dgrad_valu_kernel(const MgbD p) {
    const int b = blockIdx.y;
    const int Lmax = p.T * p.in_mul;
    const int len = mg_frames(p.lens, b, p.T) * p.in_mul;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int c = (int)(idx % p.N);
    const long sl = idx / p.N;
    if (sl >= len) return;
    const int s = (int)sl;
    const int out_mul = p.r > 0 ? p.r : 1;
    const float* dy_b = p.dy + (size_t)b * Lmax * out_mul * p.ldy;
    const float* w = p.Wt + (size_t)c * p.K;
    float sum = 0.f;
    for (int tau = 0; tau < p.taps; ++tau) {
        int rows[3];
        const int v = mgb_rows(p, s, tau, len, rows);
        if (!v) continue;
        const float* wt = w + tau * p.Cy;
        for (int n = 0; n < p.Cy; ++n) {
            float a = 0.f;
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if ((v >> j) & 1) a += dy_b[(size_t)rows[j] * p.ldy + n];
            sum = fmaf(a, wt[n], sum);
        }
    }
    const size_t pos = (size_t)b * Lmax + s;
    p.out[pos * p.ldo + c] = mgb_epilogue(p, sum, pos, c);
}

// Weight gradient on the matrix cores.  A workgroup owns 32 TM output channels x 128 columns of K and one piece of positions; k-tiles of
// 32 positions sit in LDS position-major, as they lie in memory, and every lane reads its two scalars of a k-step of two positions.
template <int TM>
__global__ void __launch_bounds__(256) mgb_wgrad_mfma_kernel(const MgbW p) {
    constexpr int BMN = 32 * TM, LDA = BMN == 32 ? 32 : BMN + 32, LDB = 160;   // row strides of 32 mod 64 floats: the two half-waves fall on different banks
    __shared__ __attribute__((aligned(16))) float Ad[32 * LDA];
    __shared__ __attribute__((aligned(16))) float Bs[32 * LDB];
    const MgLayer& L = p.L;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int n_tiles = (L.Cout + BMN - 1) / BMN;
    const int nt = (int)blockIdx.y % n_tiles, phase = (int)blockIdx.y / n_tiles;
    const int n0 = nt * BMN, k0 = (int)blockIdx.x * 128, piece = blockIdx.z;
    const int Lmax = L.T * L.in_mul;
    const long total = (long)p.B * Lmax;

    const int ld_pos = tid >> 3, ld_c = 4 * (tid & 7);
    // the columns of K this thread gathers do not change over the piece
    int col_tau[4], col_c[4];
    bool col_ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + ld_c + 32 * i;
        col_ok[i] = k < L.K;
        const int kk = col_ok[i] ? k : 0;
        col_tau[i] = kk / L.Cin;
        col_c[i] = kk - col_tau[i] * L.Cin;
    }

    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;

    for (int kt = 0; kt < MGB_PIECE / 32; ++kt) {
        const long g0 = (long)piece * MGB_PIECE + kt * 32;
        if (g0 >= total) break;
        const long g = g0 + ld_pos;
        const int b = (int)(g / Lmax), q = (int)(g - (long)b * Lmax);
        const int len = g < total ? mg_frames(L.lens, b, L.T) * L.in_mul : 0;
        const bool live = q < len;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 a4[TM], b4[4];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int n = n0 + ld_c + 32 * i;
            a4[i] = (live && n < L.Cout) ? *reinterpret_cast<const float4*>(p.dy + (((size_t)b * Lmax + q) * L.phases + phase) * p.ldy + n) : zero4;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            b4[i] = zero4;
            if (live && col_ok[i]) {
                bool z;
                const int row = mg_src_row(L, q, col_tau[i], phase, len, z);
                if (!z) {
                    const float* src = (L.two_src && col_tau[i]) ? L.src1 : L.src0;
                    float4 v = *reinterpret_cast<const float4*>(src + ((size_t)b * Lmax + row) * L.Cin + col_c[i]);
                    if ((L.act_mask >> col_tau[i]) & 1)
                        v = make_float4(mg_lrelu(v.x, L.slope), mg_lrelu(v.y, L.slope), mg_lrelu(v.z, L.slope), mg_lrelu(v.w, L.slope));
                    b4[i] = v;
                }
            }
        }
        __syncthreads();   // the previous k-tile has been read
#pragma unroll
        for (int i = 0; i < TM; ++i) *reinterpret_cast<float4*>(&Ad[ld_pos * LDA + ld_c + 32 * i]) = a4[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4*>(&Bs[ld_pos * LDB + ld_c + 32 * i]) = b4[i];
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) {
            const float bv = Bs[(2 * ks + h) * LDB + wave * 32 + r];
#pragma unroll
            for (int i = 0; i < TM; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ad[(2 * ks + h) * LDA + i * 32 + r], bv, acc[i], 0, 0, 0);
        }
    }

    // lane (r, h) holds K column r of channel rows (e & 3) + 8 (e >> 2) + 4 h
    const int col = k0 + wave * 32 + r;
    if (col >= L.K) return;
    float* out = p.part + ((size_t)piece * L.phases + phase) * L.Cout * L.K;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = n0 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (n < L.Cout) out[(size_t)n * L.K + col] = acc[i][e];
        }
}

// one thread per element of a piece's partial product
__global__ void __launch_bounds__(256) mgb_wgrad_valu_kernel(const MgbW p) {
    const MgLayer& L = p.L;
    const int piece = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long per_piece = (long)L.phases * L.Cout * L.K;
    if (idx >= per_piece) return;
    const int k = (int)(idx % L.K), n = (int)((idx / L.K) % L.Cout), phase = (int)(idx / ((long)L.K * L.Cout));
    const int tau = k / L.Cin, c = k - tau * L.Cin;
    const float* src = (L.two_src && tau) ? L.src1 : L.src0;
    const bool act = (L.act_mask >> tau) & 1;
    const int Lmax = L.T * L.in_mul;
    const long total = (long)p.B * Lmax;
    long g = (long)piece * MGB_PIECE;
    const long g_end = min(g + MGB_PIECE, total);
    float sum = 0.f;
    while (g < g_end) {
        const int b = (int)(g / Lmax);
        const int q_first = (int)(g - (long)b * Lmax);
        const int len = mg_frames(L.lens, b, L.T) * L.in_mul;
        const int q_end = (int)min((long)len, g_end - (long)b * Lmax);
        for (int q = q_first; q < q_end; ++q) {
            bool z;
            const int row = mg_src_row(L, q, tau, phase, len, z);
            if (z) continue;
            float v = src[((size_t)b * Lmax + row) * L.Cin + c];
            if (act) v = mg_lrelu(v, L.slope);
            sum = fmaf(p.dy[(((size_t)b * Lmax + q) * L.phases + phase) * p.ldy + n], v, sum);
        }
        g = (long)(b + 1) * Lmax;   // the next row
    }
    p.part[(size_t)piece * per_piece + idx] = sum;
}

// part[piece][n] = sum over the piece's positions (inside their rows) of dy[position][n]; G = 256 / N groups of positions are added in
// their order through LDS
__global__ void __launch_bounds__(256) mgb_colsum_kernel(const float* dy, int ldy, int N, const int32_t* lens, int B, int T, int mul, float* part) {
    __shared__ float red[256];
    const int piece = blockIdx.x, tid = threadIdx.x;
    const int Lmax = T * mul;
    const long total = (long)B * Lmax;
    const int G = N >= 256 ? 1 : 256 / N;
    const int g = tid / N, n_first = tid - g * N;
    for (int n = n_first; n < N; n += 256) {   // more than one pass only where N > 256 (then G = 1)
        float sum = 0.f;
        if (g < G)
            for (int i = g; i < MGB_PIECE; i += G) {
                const long pos = (long)piece * MGB_PIECE + i;
                if (pos >= total) break;
                const int b = (int)(pos / Lmax), q = (int)(pos - (long)b * Lmax);
                if (q < mg_frames(lens, b, T) * mul) sum += dy[(size_t)pos * ldy + n];
            }
        if (G == 1) {
            if (g == 0) part[(size_t)piece * N + n] = sum;
        } else {
            red[tid] = sum;
            __syncthreads();
            if (g == 0) {
                for (int j = 1; j < G; ++j) sum += red[j * N + n];
                part[(size_t)piece * N + n] = sum;
            }
        }
    }
}

// dst (PyTorch layout) = the pieces added in their order.
//   kind 0  Conv1d [Cout][Cin][k] from part[n][off + tau * Cp + c] with rows of K floats (a bias: Cin = Cp = k = K = 1)
//   kind 1  ConvTranspose1d [Cin][Cout][2 r] from part[phase][n][tau * Cin + c], the inverse of mg_pack_tconv_kernel's tap
__global__ void __launch_bounds__(256) mgb_reduce_kernel(const float* part, int pieces, size_t piece_stride, float* dst, long numel, int kind, int Cout,
                                                          int Cin, int Cp, int k, int K, int off) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= numel) return;
    size_t src;
    if (kind == 0) {
        const int tau = (int)(idx % k), c = (int)((idx / k) % Cin), n = (int)(idx / ((long)k * Cin));
        src = (size_t)n * K + off + tau * Cp + c;
    } else {
        const int r = k / 2, half = r / 2;
        const int tap = (int)(idx % k), n = (int)((idx / k) % Cout), c = (int)(idx / ((long)k * Cout));
        int tau, phase;
        if (tap >= half && tap < half + r) { tau = 0; phase = tap - half; }
        else if (tap >= half + r) { tau = 1; phase = tap - half - r; }
        else { tau = 1; phase = tap - half + r; }
        src = ((size_t)phase * Cout + n) * K + tau * Cin + c;
    }
    float sum = 0.f;
    for (int i = 0; i < pieces; ++i) sum += part[(size_t)i * piece_stride + src];
    dst[idx] = sum;
}

// The blob's K-contiguous weights, transposed for the data gradients.
//   kind 0  W[n][tau * Cin + c] -> Wt[c][tau * Cout + n]
//   kind 1  Wp[phase][n][tau * Cin + c] -> Wt[c][tap * Cout + n], tap the kernel tap of (phase, tau) as mg_pack_tconv_kernel has it (taps = r)
__global__ void __launch_bounds__(256) mgb_transpose_kernel(float* dst, const float* src, int kind, int Cout, int Cin, int taps) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (kind == 0) {
        if (idx >= (long)Cout * taps * Cin) return;
        const int c = (int)(idx % Cin), tau = (int)((idx / Cin) % taps), n = (int)(idx / ((long)Cin * taps));
        dst[(size_t)c * taps * Cout + tau * Cout + n] = src[idx];
    } else {
        const int r = taps, half = r / 2;
        if (idx >= (long)r * Cout * 2 * Cin) return;
        const int c = (int)(idx % Cin), tau = (int)((idx / Cin) % 2), n = (int)((idx / (2l * Cin)) % Cout), phase = (int)(idx / (2l * Cin * Cout));
        const int tap = tau == 0 ? phase + half : (phase < half ? phase + half + r : phase + half - r);
        dst[(size_t)c * 2 * r * Cout + tap * Cout + n] = src[idx];
    }
}

// ---- plans
struct MgTape {
    std::vector<GenTapeSlot> slots;   // the transposed mel, x after the first convolution, per stage: the transposed convolution's output, per layer h and x
    size_t floats;
};

MgTape mgb_tape_plan(const gvx_melgan_dims& d, int B, int T) {
    MgTape t;
    size_t at = 0;
    auto take = [&](int mul, int C) {
        t.slots.push_back({at, mul, C});
        at += (size_t)B * T * mul * C;
    };
    int C = d.base_channels, mul = 1;
    take(1, mg_cpad(d));
    take(1, C);
    for (int i = 0; i < d.n_stages; ++i) {
        mul *= d.ratios[i];
        C /= 2;
        take(mul, C);
        for (int j = 0; j < d.n_residual_layers; ++j) {
            take(mul, C);
            take(mul, C);
        }
    }
    t.floats = at;
    return t;
}

bool mgb_shape_ok(const gvx_melgan_dims* dims, int B, int T) {
    return !mg_dims_problem(dims) && B >= 1 && B <= 65535 && T >= GVX_MELGAN_MIN_FRAMES && T <= GVX_MELGAN_MAX_FRAMES;
}

inline long mgb_pieces(int B, int T, int mul) { return ((long)B * T * mul + MGB_PIECE - 1) / MGB_PIECE; }

struct MgbWs {   // byte offsets, each a multiple of 256
    size_t wt, wav, dz, g[2], dt, part, total;
    MgBlob wt_at;   // where each layer's transposed weights start inside wt: the blob's own offsets (a transposed tensor has its tensor's size)
};

MgbWs mgb_ws_plan(const gvx_melgan_dims& d, int B, int T) {
    MgbWs w{};
    w.wt_at = mg_blob_layout(d);
    size_t widest = d.base_channels, part = 0, mul = 1, C = d.base_channels, hop = 1;
    for (int i = 0; i < d.n_stages; ++i) hop *= d.ratios[i];
    auto need = [&](size_t m, size_t phases, size_t Cout, size_t K) { part = std::max(part, (size_t)mgb_pieces(B, T, (int)m) * phases * Cout * K); };
    need(1, 1, C, 7 * (size_t)mg_cpad(d));
    for (int i = 0; i < d.n_stages; ++i) {
        const size_t Cn = C / 2;
        need(mul, d.ratios[i], Cn, 2 * C);
        mul *= d.ratios[i];
        need(mul, 1, Cn, 3 * Cn);
        widest = std::max(widest, mul * Cn);
        C = Cn;
    }
    need(mul, 1, 1, 7 * C);
    widest = std::max(widest, (size_t)mg_cpad(d));
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += gvx::round256(bytes); return o; };
    w.wt = take(w.wt_at.total * sizeof(float));
    w.wav = take((size_t)B * T * hop * sizeof(float));
    w.dz = take((size_t)B * T * hop * sizeof(float));
    w.g[0] = take((size_t)B * T * widest * sizeof(float));
    w.g[1] = take((size_t)B * T * widest * sizeof(float));
    w.dt = take((size_t)B * T * 2 * widest * sizeof(float));
    w.part = take(part * sizeof(float));
    w.total = at;
    return w;
}

// ---- launches
bool mgb_wide(int n_out, int k_chan, int ld) { return n_out >= 32 && k_chan % 4 == 0 && ld % 4 == 0; }

template <int WR, int WC, int TM, int TN>
int mgb_launch_dgrad_mfma(const MgbD& p, int B, hipStream_t s) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
    constexpr size_t lds = (size_t)2 * (BM + BN) * MGB_LD * sizeof(float);
    static bool ready = false;   // the dynamic LDS size of this instantiation, once per process
    if (!ready) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mgb_dgrad_mfma_kernel<WR, WC, TM, TN>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        ready = true;
    }
    const dim3 grid((unsigned)((p.T * p.in_mul + BM - 1) / BM), (unsigned)((p.N + BN - 1) / BN), (unsigned)B);
    mgb_dgrad_mfma_kernel<WR, WC, TM, TN><<<grid, 256, lds, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int mgb_dgrad(const MgbD& p, int B, hipStream_t s) {
    if (mgb_wide(p.N, p.Cy, p.ldy)) {
        if (p.N >= 128) return mgb_launch_dgrad_mfma<2, 2, 2, 2>(p, B, s);
        if (p.N > 32) return mgb_launch_dgrad_mfma<4, 1, 1, 2>(p, B, s);
        return mgb_launch_dgrad_mfma<4, 1, 1, 1>(p, B, s);
    }
    const long threads = (long)p.T * p.in_mul * p.N;
    mgb_dgrad_valu_kernel<<<dim3((unsigned)((threads + 255) / 256), (unsigned)B), 256, 0, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// dY x act(src) into the pieces of p.part; returns the number of pieces through `pieces`
int mgb_wgrad(const MgbW& p, int& pieces, hipStream_t s) {
    const MgLayer& L = p.L;
    pieces = (int)mgb_pieces(p.B, L.T, L.in_mul);
    if (mgb_wide(L.Cout, L.Cin, p.ldy) && L.Cout % 4 == 0) {
        if (L.Cout > 32) {
            const dim3 grid((unsigned)((L.K + 127) / 128), (unsigned)(((L.Cout + 63) / 64) * L.phases), (unsigned)pieces);
            mgb_wgrad_mfma_kernel<2><<<grid, 256, 0, s>>>(p);
        } else {
            const dim3 grid((unsigned)((L.K + 127) / 128), (unsigned)L.phases, (unsigned)pieces);
            mgb_wgrad_mfma_kernel<1><<<grid, 256, 0, s>>>(p);
        }
    } else {
        const long per_piece = (long)L.phases * L.Cout * L.K;
        mgb_wgrad_valu_kernel<<<dim3((unsigned)((per_piece + 255) / 256), (unsigned)pieces), 256, 0, s>>>(p);
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int mgb_reduce(const float* part, int pieces, size_t piece_stride, float* dst, long numel, int kind, int Cout, int Cin, int Cp, int k, int K, int off,
               hipStream_t s) {
    mgb_reduce_kernel<<<(unsigned)((numel + 255) / 256), 256, 0, s>>>(part, pieces, piece_stride, dst, numel, kind, Cout, Cin, Cp, k, K, off);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// the column sums of dy [B][T * mul][ldy] (N columns) into one or two bias gradients
int mgb_bias(const float* dy, int ldy, int N, const int32_t* lens, int B, int T, int mul, float* part, float* dst0, float* dst1, hipStream_t s) {
    const int pieces = (int)mgb_pieces(B, T, mul);
    mgb_colsum_kernel<<<(unsigned)pieces, 256, 0, s>>>(dy, ldy, N, lens, B, T, mul, part);
    HIP_TRY(hipGetLastError());
    int rc = mgb_reduce(part, pieces, (size_t)N, dst0, N, 0, N, 1, 1, 1, 1, 0, s);
    if (rc == GVX_OK && dst1) rc = mgb_reduce(part, pieces, (size_t)N, dst1, N, 0, N, 1, 1, 1, 1, 0, s);
    return rc;
}

int mgb_transpose(float* dst, const float* src, int kind, int Cout, int Cin, int taps, hipStream_t s) {
    const long count = kind == 0 ? (long)Cout * taps * Cin : (long)taps * Cout * 2 * Cin;
    mgb_transpose_kernel<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(dst, src, kind, Cout, Cin, taps);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

struct MgbGrads {
    float *pre_w, *pre_b, *post_w, *post_b;
    float *up_w[GVX_MELGAN_MAX_STAGES], *up_b[GVX_MELGAN_MAX_STAGES];
    float *conv_w[GVX_MELGAN_MAX_STAGES][8], *conv_b[GVX_MELGAN_MAX_STAGES][8], *sc_w[GVX_MELGAN_MAX_STAGES][8], *sc_b[GVX_MELGAN_MAX_STAGES][8],
        *mix_w[GVX_MELGAN_MAX_STAGES][8], *mix_b[GVX_MELGAN_MAX_STAGES][8];
};

int mgb_check_call(const gvx_melgan* h, int B, int T, const void* tape, size_t tape_bytes) {
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (T < GVX_MELGAN_MIN_FRAMES) return fail(GVX_ERR_INVALID_ARG, "T = %d: the first convolution's reflection needs at least %d frames", T, GVX_MELGAN_MIN_FRAMES);
    if (T > GVX_MELGAN_MAX_FRAMES) return fail(GVX_ERR_UNSUPPORTED, "T = %d is beyond the limit of %d frames", T, GVX_MELGAN_MAX_FRAMES);
    return gen_check_tape(tape, tape_bytes, mgb_tape_plan(h->d, B, T).floats * sizeof(float));
}

}  // namespace

extern "C" {

size_t gvx_melgan_tape_bytes(const gvx_melgan_dims* dims, int B, int T) {
    if (!mgb_shape_ok(dims, B, T)) return 0;
    return mgb_tape_plan(*dims, B, T).floats * sizeof(float);
}

int gvx_melgan_tape_layout(const gvx_melgan_dims* dims, int B, int T, gvx_melgan_tape_entry* entries, int max_entries) {
    if (!mgb_shape_ok(dims, B, T)) return 0;
    return gen_tape_layout(mgb_tape_plan(*dims, B, T).slots, entries, max_entries);
}

size_t gvx_melgan_backward_workspace_bytes(const gvx_melgan_dims* dims, int B, int T) {
    if (!mgb_shape_ok(dims, B, T)) return 0;
    return mgb_ws_plan(*dims, B, T).total;
}

int gvx_melgan_forward_train(gvx_melgan* h, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, void* tape, size_t tape_bytes,
                             void* workspace, size_t workspace_bytes, void* stream) {
    (void)workspace; (void)workspace_bytes;   // every intermediate tensor is a tape slot: the call needs no scratch
    if (!h || !mel || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = mgb_check_call(h, B, T, tape, tape_bytes)) != GVX_OK) return rc;
    const gvx_melgan_dims& d = h->d;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = mg_prepare(h)) != GVX_OK) return rc;
    const MgTape tp = mgb_tape_plan(d, B, T);
    const MgBlob L = mg_blob_layout(d);
    const float* blob = h->blob;
    float* base = static_cast<float*>(tape);
    int slot = 0;
    auto next = [&]() { return base + tp.slots[slot++].off; };

    const int Cp = mg_cpad(d);
    float* mel_t = next();
    if ((rc = mg_mel_transpose(mel, frame_lengths, B, d.n_mels, T, Cp, mel_t, s)) != GVX_OK) return rc;
    // from here on: the layers of gvx_melgan_forward, argument for argument, but for where they write
    MgLayer p{};
    p.lens = frame_lengths; p.T = T; p.slope = d.slope;
    int C = d.base_channels, mul = 1;
    float* cur = next();
    p.src0 = mel_t; p.W = blob + L.pre_w; p.bias = blob + L.pre_b; p.out = cur;
    p.in_mul = 1; p.Cin = Cp; p.Cout = C; p.taps = 7; p.K = 7 * Cp; p.dil = 1; p.phases = 1; p.act_mask = 0;
    if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
    for (int i = 0; i < d.n_stages; ++i) {
        const int Cn = C / 2, r = d.ratios[i];
        float* x = next();
        p = MgLayer{};
        p.lens = frame_lengths; p.T = T; p.slope = d.slope;
        p.src0 = cur; p.W = blob + L.up_w[i]; p.bias = blob + L.up_b[i]; p.out = x;
        p.in_mul = mul; p.Cin = C; p.Cout = Cn; p.taps = 2; p.K = 2 * C; p.dil = 0; p.phases = r; p.act_mask = 3;
        if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
        mul *= r;
        int dil = 1;
        for (int j = 0; j < d.n_residual_layers; ++j, dil *= d.dilation_base) {
            float* hbuf = next();
            float* y = next();
            p = MgLayer{};
            p.lens = frame_lengths; p.T = T; p.slope = d.slope;
            p.src0 = x; p.W = blob + L.conv_w[i][j]; p.bias = blob + L.conv_b[i][j]; p.out = hbuf;
            p.in_mul = mul; p.Cin = Cn; p.Cout = Cn; p.taps = 3; p.K = 3 * Cn; p.dil = dil; p.phases = 1; p.act_mask = 7;
            if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
            p.src1 = hbuf; p.two_src = 1; p.W = blob + L.tail_w[i][j]; p.bias = blob + L.sc_b[i][j]; p.bias2 = blob + L.mix_b[i][j]; p.out = y;
            p.taps = 2; p.K = 2 * Cn; p.dil = 0; p.act_mask = 2;
            if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
            x = y;
        }
        cur = x;
        C = Cn;
    }
    p = MgLayer{};
    p.lens = frame_lengths; p.T = T; p.slope = d.slope;
    p.src0 = cur; p.W = blob + L.post_w; p.bias = blob + L.post_b; p.out = wav_out;
    p.in_mul = mul; p.Cin = C; p.Cout = 1; p.taps = 7; p.K = 7 * C; p.dil = 1; p.phases = 1; p.act_mask = 0x7f; p.tanh_out = 1; p.zero_tail = 1;
    return mg_launch(p, B, s);
}

int gvx_melgan_backward(gvx_melgan* h, const float* d_wav, const int32_t* frame_lengths, int B, int T, const void* tape, size_t tape_bytes,
                        const gvx_grad_desc* grads, int n_grads, float* d_mel_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !d_wav || !grads || n_grads < 1) return fail(GVX_ERR_INVALID_ARG, "null argument");
    int rc;
    if ((rc = mgb_check_call(h, B, T, tape, tape_bytes)) != GVX_OK) return rc;
    const gvx_melgan_dims& d = h->d;
    const MgbWs wp = mgb_ws_plan(d, B, T);
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    const int S = d.n_stages, R = d.n_residual_layers, Cp = mg_cpad(d);
    {
        int hop_ = 1;
        for (int i = 0; i < S; ++i) hop_ *= d.ratios[i];
        if (mgb_pieces(B, T, hop_) > 65535) return fail(GVX_ERR_UNSUPPORTED, "B * T * hop = %ld positions are beyond 65535 pieces of %d", (long)B * T * hop_, MGB_PIECE);
    }
    MgbGrads g{};
    {
        size_t C = d.base_channels;
        g.pre_w = gen_grad(grads, n_grads, "pre.weight", C * d.n_mels * 7, rc);
        g.pre_b = gen_grad(grads, n_grads, "pre.bias", C, rc);
        for (int i = 0; i < S; ++i) {
            const size_t Cn = C / 2;
            const std::string up = "ups." + std::to_string(i);
            g.up_w[i] = gen_grad(grads, n_grads, up + ".weight", C * Cn * 2 * d.ratios[i], rc);
            g.up_b[i] = gen_grad(grads, n_grads, up + ".bias", Cn, rc);
            for (int j = 0; j < R; ++j) {
                const std::string res = "res." + std::to_string(i) + "." + std::to_string(j);
                g.conv_w[i][j] = gen_grad(grads, n_grads, res + ".conv.weight", Cn * Cn * 3, rc);
                g.conv_b[i][j] = gen_grad(grads, n_grads, res + ".conv.bias", Cn, rc);
                g.sc_w[i][j] = gen_grad(grads, n_grads, res + ".shortcut.weight", Cn * Cn, rc);
                g.sc_b[i][j] = gen_grad(grads, n_grads, res + ".shortcut.bias", Cn, rc);
                g.mix_w[i][j] = gen_grad(grads, n_grads, res + ".mix.weight", Cn * Cn, rc);
                g.mix_b[i][j] = gen_grad(grads, n_grads, res + ".mix.bias", Cn, rc);
            }
            C = Cn;
        }
        g.post_w = gen_grad(grads, n_grads, "post.weight", 7 * C, rc);
        g.post_b = gen_grad(grads, n_grads, "post.bias", 1, rc);
        if (rc != GVX_OK) return rc;   // nothing was launched
    }
    hipStream_t s = (hipStream_t)stream;
    if ((rc = mg_prepare(h)) != GVX_OK) return rc;
    const MgTape tp = mgb_tape_plan(d, B, T);
    const MgBlob L = mg_blob_layout(d);
    const float* blob = h->blob;
    const float* tbase = static_cast<const float*>(tape);
    auto slot = [&](int i) { return tbase + tp.slots[i].off; };
    auto x_slot = [&](int i, int j) { return 2 + i * (1 + 2 * R) + 2 * j; };   // j = 0: the transposed convolution's output; j > 0: x after layer j - 1
    float* wt = gvx::ws_ptr<float>(workspace, wp.wt);
    float* wav = gvx::ws_ptr<float>(workspace, wp.wav);
    float* dz = gvx::ws_ptr<float>(workspace, wp.dz);
    float* G = gvx::ws_ptr<float>(workspace, wp.g[0]);
    float* G2 = gvx::ws_ptr<float>(workspace, wp.g[1]);
    float* dt = gvx::ws_ptr<float>(workspace, wp.dt);
    float* part = gvx::ws_ptr<float>(workspace, wp.part);

    // the transposed weights, from the blob the forward read
    {
        int C = d.base_channels;
        if ((rc = mgb_transpose(wt + L.pre_w, blob + L.pre_w, 0, C, Cp, 7, s)) != GVX_OK) return rc;
        for (int i = 0; i < S; ++i) {
            const int Cn = C / 2;
            if ((rc = mgb_transpose(wt + L.up_w[i], blob + L.up_w[i], 1, Cn, C, d.ratios[i], s)) != GVX_OK) return rc;
            for (int j = 0; j < R; ++j) {
                if ((rc = mgb_transpose(wt + L.conv_w[i][j], blob + L.conv_w[i][j], 0, Cn, Cn, 3, s)) != GVX_OK) return rc;
                if ((rc = mgb_transpose(wt + L.tail_w[i][j], blob + L.tail_w[i][j], 0, Cn, 2 * Cn, 1, s)) != GVX_OK) return rc;
            }
            C = Cn;
        }
        if ((rc = mgb_transpose(wt + L.post_w, blob + L.post_w, 0, 1, C, 7, s)) != GVX_OK) return rc;
    }

    int hop = 1, C_last = d.base_channels;
    for (int i = 0; i < S; ++i) { hop *= d.ratios[i]; C_last /= 2; }
    int pieces = 0;
    MgbW w{};
    MgbD dg{};
    auto layer = [&]() { MgLayer p{}; p.lens = frame_lengths; p.T = T; p.slope = d.slope; return p; };
    auto dgrad0 = [&]() { MgbD q{}; q.lens = frame_lengths; q.T = T; q.slope = d.slope; return q; };

    // the output layer: the waveform again (the forward's own launch), tanh', then the 7-tap convolution over lrelu(x)
    const float* x_last = slot(x_slot(S - 1, R));
    {
        MgLayer p = layer();
        p.src0 = x_last; p.W = blob + L.post_w; p.bias = blob + L.post_b; p.out = wav;
        p.in_mul = hop; p.Cin = C_last; p.Cout = 1; p.taps = 7; p.K = 7 * C_last; p.dil = 1; p.phases = 1; p.act_mask = 0x7f; p.tanh_out = 1;
        if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
        gen_tanh_bwd_kernel<GVX_MELGAN_MIN_FRAMES><<<dim3((unsigned)(((long)T * hop + 255) / 256), (unsigned)B), 256, 0, s>>>(d_wav, wav, frame_lengths, T, hop, dz);
        HIP_TRY(hipGetLastError());
        w = MgbW{p, dz, 1, part, B};
        if ((rc = mgb_wgrad(w, pieces, s)) != GVX_OK) return rc;
        if ((rc = mgb_reduce(part, pieces, (size_t)7 * C_last, g.post_w, 7l * C_last, 0, 1, C_last, C_last, 7, 7 * C_last, 0, s)) != GVX_OK) return rc;
        if ((rc = mgb_bias(dz, 1, 1, frame_lengths, B, T, hop, part, g.post_b, nullptr, s)) != GVX_OK) return rc;
        dg = dgrad0();
        dg.dy = dz; dg.ldy = 1; dg.Wt = wt + L.post_w; dg.out = G; dg.ldo = C_last; dg.mask = x_last; dg.ldm = C_last;
        dg.in_mul = hop; dg.N = C_last; dg.Cy = 1; dg.taps = 7; dg.K = 7; dg.dil = 1;
        if ((rc = mgb_dgrad(dg, B, s)) != GVX_OK) return rc;
    }

    int C = C_last, mul = hop;   // G holds d x [B][T * mul][C]
    for (int i = S - 1; i >= 0; --i) {
        const int r = d.ratios[i], Cin = 2 * C;
        int dil = 1;
        for (int j = 1; j < R; ++j) dil *= d.dilation_base;
        for (int j = R - 1; j >= 0; --j, dil /= d.dilation_base) {
            const float* x = slot(x_slot(i, j));
            const float* hbuf = slot(x_slot(i, j) + 1);
            // the tail: shortcut(x) + mix(lrelu(h))
            MgLayer p = layer();
            p.src0 = x; p.src1 = hbuf; p.two_src = 1; p.in_mul = mul; p.Cin = C; p.Cout = C; p.taps = 2; p.K = 2 * C; p.dil = 0; p.phases = 1; p.act_mask = 2;
            w = MgbW{p, G, C, part, B};
            if ((rc = mgb_wgrad(w, pieces, s)) != GVX_OK) return rc;
            if ((rc = mgb_reduce(part, pieces, (size_t)C * 2 * C, g.sc_w[i][j], (long)C * C, 0, C, C, C, 1, 2 * C, 0, s)) != GVX_OK) return rc;
            if ((rc = mgb_reduce(part, pieces, (size_t)C * 2 * C, g.mix_w[i][j], (long)C * C, 0, C, C, C, 1, 2 * C, C, s)) != GVX_OK) return rc;
            if ((rc = mgb_bias(G, C, C, frame_lengths, B, T, mul, part, g.sc_b[i][j], g.mix_b[i][j], s)) != GVX_OK) return rc;
            dg = dgrad0();   // dt = [d x through the shortcut | d h]
            dg.dy = G; dg.ldy = C; dg.Wt = wt + L.tail_w[i][j]; dg.out = dt; dg.ldo = 2 * C; dg.mask = hbuf; dg.ldm = C; dg.mask_from = C;
            dg.in_mul = mul; dg.N = 2 * C; dg.Cy = C; dg.taps = 1; dg.K = C; dg.dil = 0;
            if ((rc = mgb_dgrad(dg, B, s)) != GVX_OK) return rc;
            // the dilated convolution over lrelu(x)
            p = layer();
            p.src0 = x; p.in_mul = mul; p.Cin = C; p.Cout = C; p.taps = 3; p.K = 3 * C; p.dil = dil; p.phases = 1; p.act_mask = 7;
            w = MgbW{p, dt + C, 2 * C, part, B};
            if ((rc = mgb_wgrad(w, pieces, s)) != GVX_OK) return rc;
            if ((rc = mgb_reduce(part, pieces, (size_t)C * 3 * C, g.conv_w[i][j], 3l * C * C, 0, C, C, C, 3, 3 * C, 0, s)) != GVX_OK) return rc;
            if ((rc = mgb_bias(dt + C, 2 * C, C, frame_lengths, B, T, mul, part, g.conv_b[i][j], nullptr, s)) != GVX_OK) return rc;
            dg = dgrad0();   // d x = lrelu'(x) * conv^T(d h) + the shortcut's share; G is dead since the tail's product
            dg.dy = dt + C; dg.ldy = 2 * C; dg.Wt = wt + L.conv_w[i][j]; dg.out = G; dg.ldo = C; dg.mask = x; dg.ldm = C; dg.add = dt; dg.lda = 2 * C;
            dg.in_mul = mul; dg.N = C; dg.Cy = C; dg.taps = 3; dg.K = 3 * C; dg.dil = dil;
            if ((rc = mgb_dgrad(dg, B, s)) != GVX_OK) return rc;
        }
        // the transposed convolution over lrelu(cur)
        const int in_mul = mul / r;
        const float* cur = i == 0 ? slot(1) : slot(x_slot(i - 1, R));
        MgLayer p = layer();
        p.src0 = cur; p.in_mul = in_mul; p.Cin = Cin; p.Cout = C; p.taps = 2; p.K = 2 * Cin; p.dil = 0; p.phases = r; p.act_mask = 3;
        w = MgbW{p, G, C, part, B};
        if ((rc = mgb_wgrad(w, pieces, s)) != GVX_OK) return rc;
        if ((rc = mgb_reduce(part, pieces, (size_t)r * C * 2 * Cin, g.up_w[i], (long)Cin * C * 2 * r, 1, C, Cin, Cin, 2 * r, 2 * Cin, 0, s)) != GVX_OK) return rc;
        if ((rc = mgb_bias(G, C, C, frame_lengths, B, T, mul, part, g.up_b[i], nullptr, s)) != GVX_OK) return rc;
        dg = dgrad0();
        dg.dy = G; dg.ldy = C; dg.Wt = wt + L.up_w[i]; dg.out = G2; dg.ldo = Cin; dg.mask = cur; dg.ldm = Cin;
        dg.in_mul = in_mul; dg.N = Cin; dg.Cy = C; dg.taps = 2 * r; dg.K = 2 * r * C; dg.r = r;
        if ((rc = mgb_dgrad(dg, B, s)) != GVX_OK) return rc;
        std::swap(G, G2);
        C = Cin;
        mul = in_mul;
    }

    // the first convolution: no activation in front of it
    {
        MgLayer p = layer();
        p.src0 = slot(0); p.in_mul = 1; p.Cin = Cp; p.Cout = C; p.taps = 7; p.K = 7 * Cp; p.dil = 1; p.phases = 1; p.act_mask = 0;
        w = MgbW{p, G, C, part, B};
        if ((rc = mgb_wgrad(w, pieces, s)) != GVX_OK) return rc;
        if ((rc = mgb_reduce(part, pieces, (size_t)C * 7 * Cp, g.pre_w, (long)C * d.n_mels * 7, 0, C, d.n_mels, Cp, 7, 7 * Cp, 0, s)) != GVX_OK) return rc;
        if ((rc = mgb_bias(G, C, C, frame_lengths, B, T, 1, part, g.pre_b, nullptr, s)) != GVX_OK) return rc;
        if (d_mel_out) {
            dg = dgrad0();
            dg.dy = G; dg.ldy = C; dg.Wt = wt + L.pre_w; dg.out = G2; dg.ldo = Cp;
            dg.in_mul = 1; dg.N = Cp; dg.Cy = C; dg.taps = 7; dg.K = 7 * C; dg.dil = 1;
            if ((rc = mgb_dgrad(dg, B, s)) != GVX_OK) return rc;
            gen_dmel_kernel<GVX_MELGAN_MIN_FRAMES><<<dim3((unsigned)(((long)d.n_mels * T + 255) / 256), (unsigned)B), 256, 0, s>>>(G2, frame_lengths, d.n_mels, T, Cp, d_mel_out);
            HIP_TRY(hipGetLastError());
        }
    }
    return GVX_OK;
}

}  // C ABI
