// HiFi-GAN period discriminators (include/genvox_amd.h, "HiFi-GAN period discriminators"): forward, and the backward that reads the
// forward's own maps as its tape.  Maps are channels-last, [B][height][period][channels]: a grid cell's channels are contiguous, which
// is what an implicit GEMM with positions on M and channels on K wants.
//
// A workgroup owns PD_TILE positions (height, column) of one row.  Position m of a tile is (u, col) = (m / period, m % period); in a
// forward kernel u is the output height, in a data gradient the workgroup belongs to ONE stride phase ph and the input height is
// h = u * stride + ph, so that only the taps t = (ph + pad) mod stride, + stride, ... meet a dY height - the gather by stride phase.
//   pd_mfma_kernel     the wide layers, forward (BWD = false) and data gradient (BWD = true): 64 positions x 128 channels (64 where fewer
//                      than 128 are produced), four waves of two (one) 32 x 32 v_mfma_f32_32x32x2_f32 tiles each, k-steps of (one tap,
//                      32 channels) through LDS; the products of a channel block are summed apart and then added, so the 5 C_in terms
//                      never form one chain.
//   pd_valu_kernel     the same two products in fp32 VALU code, G lanes per output element: the first layer (which absorbs the
//                      reflection and the reshape: its operand is the waveform), the score (G = 64: the input channels dealt over a
//                      wave, added by a fixed butterfly) and narrow layers.
//   pd_wgrad_mfma_kernel / pd_wgrad_valu_kernel   one piece (rows, or a run of positions of one row) of a weight gradient, laid out
//                      [tap][c_out][c_in]; pd_reduce_kernel adds the pieces in their order into PyTorch's layout.
//   pd_db_kernel       bias gradients in float64 slices, added in their order.
//   pd_dwav_kernel     the adjoint of reshape + reflection as a gather, accumulated over the periods in their order.
// No atomics anywhere: two calls give the same bits.
#include "gvx_internal.h"
#include "hifigan_disc_internal.h"
#include "melgan_internal.h"

#include <string>
#include <vector>

using gvx::fail;
using namespace gvx_pd;

static_assert(PD_TILE == GVX_HIFIGAN_MPD_TILE && PD_TILE_N == GVX_HIFIGAN_MPD_TILE_N && PD_TILE_N_WIDE == GVX_HIFIGAN_MPD_TILE_N_WIDE &&
                  PD_MFMA_MULT == GVX_HIFIGAN_MPD_MFMA_MULT,
              "the public header states the tile constants");

struct gvx_hifigan_mpd {
    gvx_hifigan_mpd_dims d;
    const float* blob = nullptr;
    bool timing = false;                     // measurement only: events around every layer of the last forward / backward
    std::vector<hipEvent_t> fwd_ev, bwd_ev;  // per period n_maps + 1 marks
    bool fwd_timed = false, bwd_timed = false;
};

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int PD_LD = 36;    // floats per LDS row of a 32-deep k-tile: the fragment reads of sixteen lanes fall on distinct 16-byte slots
constexpr int PD_WLD = 96;   // floats per LDS row of the weight gradient's 64-wide operands: the two k rows of a step 32 banks apart

struct PdConv {
    const float* src;     // the operand: forward [B][Hs_max][period][KC] (layer 0: the waveform [B][n_max]); data gradient dY
    const float* W;       // [NC][taps][KC]
    const float* bias;    // forward
    float* out;           // [B][Ho_max][period][NC]
    const float* dfeat;   // data gradient: cotangent of the map that `out` is the gradient of (added before its mask)
    const float* mask;    // data gradient: that map itself, for its sign
    const float* dy;      // weight gradient: [B][Ho_max][period][NC] against src [B][Hs_max][period][KC]
    const int32_t* lens;
    int n_max, min_n, s;
    int period, KC, NC, k, stride, pad;
    int Hs_max, Ho_max, down_s, down_o;
    int act, wav_src;
    float slope;
};

__device__ __forceinline__ int pd_row_n(const PdConv& p, int b) {
    int n = p.lens ? p.lens[b] : p.n_max;
    n = n > p.n_max ? p.n_max : n;
    return n < p.min_n ? 0 : n;   // rows the caller should have refused are silent, never a bad address
}

// how the taps of one workgroup walk the operand's heights: tap j (weight tap t0 + j * tstep) of position u reads height
// u * mul + base + j * hstep
struct PdTaps { int n, t0, tstep, mul, base, hstep; };

template <bool BWD>
__device__ __forceinline__ PdTaps pd_taps(const PdConv& p, int ph) {
    if constexpr (!BWD) return PdTaps{p.k, 0, 1, p.stride, -p.pad, 1};
    const int t0 = (ph + p.pad) % p.stride;
    return PdTaps{t0 < p.k ? (p.k - 1 - t0) / p.stride + 1 : 0, t0, p.stride, 1, (ph + p.pad - t0) / p.stride, -1};
}

// a tile behind its row: exact zeros inside the buffer
template <bool BWD>
__device__ __forceinline__ void pd_zero_tile(const PdConv& p, int b, int m0, int ph, int n0, int cols) {
    for (int idx = threadIdx.x; idx < PD_TILE * cols; idx += blockDim.x) {
        const int m = m0 + idx / cols, u = m / p.period, col = m % p.period;
        const int h = BWD ? u * p.stride + ph : u;
        if (h < p.Ho_max) p.out[(((size_t)b * p.Ho_max + h) * p.period + col) * p.NC + n0 + idx % cols] = 0.f;
    }
}

template <bool BWD>
__device__ __forceinline__ void pd_finish(const PdConv& p, int b, int h, int col, int n, int Ho, float v) {
    if (h >= p.Ho_max) return;
    const size_t at = (((size_t)b * p.Ho_max + h) * p.period + col) * p.NC + n;
    if (h >= Ho) { p.out[at] = 0.f; return; }
    if constexpr (BWD) {
        if (p.dfeat) v += p.dfeat[at];
        v = p.mask[at] > 0.f ? v : v * p.slope;
    } else {
        v += p.bias[n];
        if (p.act) v = v > 0.f ? v : v * p.slope;
    }
    p.out[at] = v;
}

// TN = 1: 64 positions x 64 channels, a 32 x 32 tile per wave; TN = 2: 64 x 128, two tiles per wave off one A fragment
template <bool BWD, int TN>
__global__ void __launch_bounds__(256) pd_mfma_kernel(const PdConv p) {
    constexpr int BN = PD_TILE_N * TN;
    __shared__ __attribute__((aligned(16))) float As[PD_TILE * PD_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * PD_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1, r = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z;
    const int n_tiles = (p.NC + BN - 1) / BN;
    const int n0 = ((int)blockIdx.y % n_tiles) * BN, ph = (int)blockIdx.y / n_tiles;
    const int m0 = (int)blockIdx.x * PD_TILE;
    const int nb = pd_row_n(p, b);
    const int Hs = pd_height(nb, p.period, p.s, p.down_s), Ho = pd_height(nb, p.period, p.s, p.down_o);
    const int h_first = BWD ? (m0 / p.period) * p.stride + ph : m0 / p.period;
    if (h_first >= Ho) {
        pd_zero_tile<BWD>(p, b, m0, ph, n0, min(BN, p.NC - n0));
        return;
    }
    const PdTaps tp = pd_taps<BWD>(p, ph);
    const int ld_row = tid >> 3, ld_c4 = tid & 7;
    const int K = p.k * p.KC;
    const float* src_b = p.src + (size_t)b * p.Hs_max * p.period * p.KC;
    int a_u[2], a_col[2];
    bool a_live[2];
    const float* w_row[2 * TN];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + ld_row + 32 * i;
        a_u[i] = m / p.period;
        a_col[i] = m % p.period;
        a_live[i] = (BWD ? a_u[i] * p.stride + ph : a_u[i]) < Ho;
    }
#pragma unroll
    for (int i = 0; i < 2 * TN; ++i) {
        const int n = n0 + ld_row + 32 * i;
        w_row[i] = p.W + (size_t)(n < p.NC ? n : 0) * K;   // columns past NC read row 0 and are never stored
    }
    float4 a_reg[2], b_reg[2 * TN];
    bool a_keep[2] = {false, false};
    auto load = [&](int cb, int j) {
        const int c = 32 * cb + 4 * ld_c4;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int hs = a_u[i] * tp.mul + tp.base + j * tp.hstep;
            a_keep[i] = a_live[i] && hs >= 0 && hs < Hs;
            a_reg[i] = *reinterpret_cast<const float4*>(src_b + ((size_t)(a_keep[i] ? hs : 0) * p.period + a_col[i]) * p.KC + c);
        }
#pragma unroll
        for (int i = 0; i < 2 * TN; ++i) b_reg[i] = *reinterpret_cast<const float4*>(w_row[i] + (size_t)(tp.t0 + j * tp.tstep) * p.KC + c);
    };
    f32x16 acc[TN], part[TN];
#pragma unroll
    for (int t = 0; t < TN; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f, part[t][e] = 0.f;
    const int n_it = (p.KC / 32) * tp.n;   // (channel block, tap) pairs, the tap fastest
    int cb = 0, j = 0;
    if (n_it > 0) load(0, 0);
    for (int it = 0; it < n_it; ++it) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(&As[(ld_row + 32 * i) * PD_LD + 4 * ld_c4]) = a_keep[i] ? a_reg[i] : z;
#pragma unroll
        for (int i = 0; i < 2 * TN; ++i) *reinterpret_cast<float4*>(&Bs[(ld_row + 32 * i) * PD_LD + 4 * ld_c4]) = b_reg[i];
        __syncthreads();
        int nj = j + 1, ncb = cb;
        if (nj == tp.n) { nj = 0; ++ncb; }
        if (it + 1 < n_it) load(ncb, nj);
        const float* a_base = &As[(wr * 32 + r) * PD_LD + 4 * hh];
        const float* b_base = &Bs[(wc * 32 * TN + r) * PD_LD + 4 * hh];
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
            const float4 af = *reinterpret_cast<const float4*>(a_base + 8 * kg);
            float4 bf[TN];
#pragma unroll
            for (int t = 0; t < TN; ++t) bf[t] = *reinterpret_cast<const float4*>(b_base + t * 32 * PD_LD + 8 * kg);
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                part[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf[t].x, part[t], 0, 0, 0);
                part[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf[t].y, part[t], 0, 0, 0);
                part[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf[t].z, part[t], 0, 0, 0);
                part[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf[t].w, part[t], 0, 0, 0);
            }
        }
        if (nj == 0) {   // a channel block is done
#pragma unroll
            for (int t = 0; t < TN; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[t][e] += part[t][e], part[t][e] = 0.f;
        }
        __syncthreads();
        j = nj;
        cb = ncb;
    }
    // epilogue: lane (r, hh) holds column r of rows (e & 3) + 8 (e >> 2) + 4 hh of each of its 32 x 32 tiles
#pragma unroll
    for (int t = 0; t < TN; ++t) {
        const int n = n0 + (wc * TN + t) * 32 + r;
        if (n >= p.NC) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = m0 + wr * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh, u = m / p.period, col = m % p.period;
            pd_finish<BWD>(p, b, BWD ? u * p.stride + ph : u, col, n, Ho, acc[t][e]);
        }
    }
}

// G lanes per output element (position, channel), channel fastest; the G partial sums are added by a fixed butterfly
template <int G, bool BWD>
__global__ void __launch_bounds__(256) pd_valu_kernel(const PdConv p) {
    const int b = blockIdx.z;
    const int n_tiles = (p.NC + PD_TILE_N - 1) / PD_TILE_N;   // the output channels in slices of PD_TILE_N, as in the matrix kernel
    const int n0 = ((int)blockIdx.y % n_tiles) * PD_TILE_N, ph = (int)blockIdx.y / n_tiles;
    const int cols = min(PD_TILE_N, p.NC - n0);
    const int m0 = (int)blockIdx.x * PD_TILE;
    const int nb = pd_row_n(p, b);
    const int Hs = pd_height(nb, p.period, p.s, p.down_s), Ho = pd_height(nb, p.period, p.s, p.down_o);
    const int h_first = BWD ? (m0 / p.period) * p.stride + ph : m0 / p.period;
    if (h_first >= Ho) {
        pd_zero_tile<BWD>(p, b, m0, ph, n0, cols);
        return;
    }
    const PdTaps tp = pd_taps<BWD>(p, ph);
    const int K = p.k * p.KC;
    const float* src_b = p.wav_src ? p.src + (size_t)b * p.n_max : p.src + (size_t)b * p.Hs_max * p.period * p.KC;
    const int total = PD_TILE * cols * G;   // G = 64: a multiple of 256, so the lanes of a wave stay together for the butterfly
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int g = idx % G, el = idx / G, n = n0 + el % cols, m = m0 + el / cols;
        const int u = m / p.period, col = m % p.period, h = BWD ? u * p.stride + ph : u;
        float sum = 0.f;
        if (h < Ho) {
            const float* w = p.W + (size_t)n * K;
            for (int j = 0; j < tp.n; ++j) {
                const int hs = u * tp.mul + tp.base + j * tp.hstep;
                if (hs < 0 || hs >= Hs) continue;
                const float* wt = w + (size_t)(tp.t0 + j * tp.tstep) * p.KC;
                float run = 0.f;
                if (p.wav_src) {   // the reshape and the reflection: cell (hs, col) is sample hs * period + col, mirrored behind the row
                    int i = hs * p.period + col;
                    i = i >= nb ? 2 * (nb - 1) - i : i;
                    if (g == 0 && i >= 0) run = src_b[i] * wt[0];
                } else {
                    const float* x = src_b + ((size_t)hs * p.period + col) * p.KC;
                    if constexpr (G > 1) {   // KC is a multiple of 4 here (pd_launch_conv): a lane takes whole float4s
                        for (int c = 4 * g; c < p.KC; c += 4 * G) {
                            const float4 xv = *reinterpret_cast<const float4*>(x + c), wv = *reinterpret_cast<const float4*>(wt + c);
                            run = fmaf(xv.w, wv.w, fmaf(xv.z, wv.z, fmaf(xv.y, wv.y, fmaf(xv.x, wv.x, run))));
                        }
                    } else {
                        for (int c = 0; c < p.KC; ++c) run = fmaf(x[c], wt[c], run);
                    }
                }
                sum += run;
            }
        }
#pragma unroll
        for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (g == 0) pd_finish<BWD>(p, b, h, col, n, Ho, sum);
    }
}

// the positions [la, lb) of row b that a weight-gradient piece sums: rows dealt to pieces, or a row cut into runs
struct PdSpan { int b0, b1, chunk; };
__device__ __forceinline__ PdSpan pd_span(int piece, int B, int chunks, int rows_per_piece) {
    if (chunks > 1) return PdSpan{piece / chunks, piece / chunks + 1, piece % chunks};
    const int b0 = piece * rows_per_piece;
    return PdSpan{b0, b0 + rows_per_piece < B ? b0 + rows_per_piece : B, 0};
}

// one piece of dW[t][n][c] = sum over positions of dY[pos][n] X[source height of (pos, t)][c]: 64 n x 64 c of one tap, positions on k
__global__ void __launch_bounds__(256) pd_wgrad_mfma_kernel(const PdConv p, float* parts, int B, int chunks, int rows_per_piece, int run) {
    __shared__ __attribute__((aligned(16))) float As[PD_WG_CHUNK * PD_WLD];
    __shared__ __attribute__((aligned(16))) float Bs[PD_WG_CHUNK * PD_WLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1, r = lane & 31, hh = lane >> 5;
    const int n0 = (int)blockIdx.x * 64, c0 = (int)blockIdx.y * 64;
    const int piece = (int)blockIdx.z / p.k, t = (int)blockIdx.z % p.k;
    const PdSpan sp = pd_span(piece, B, chunks, rows_per_piece);
    const int ld_row = tid >> 4, ld_c4 = tid & 15;
    const bool n_ok = n0 + 4 * ld_c4 < p.NC, c_ok = c0 + 4 * ld_c4 < p.KC;   // both counts are multiples of 32: a float4 is whole
    f32x16 acc, part;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f, part[e] = 0.f;
    int since = 0;
    for (int b = sp.b0; b < sp.b1; ++b) {
        const int nb = pd_row_n(p, b);
        const int Hs = pd_height(nb, p.period, p.s, p.down_s), Ho = pd_height(nb, p.period, p.s, p.down_o);
        const int la = sp.chunk * run, lb = min(la + run, Ho * p.period);
        const float* dy_b = p.dy + (size_t)b * p.Ho_max * p.period * p.NC;
        const float* x_b = p.src + (size_t)b * p.Hs_max * p.period * p.KC;
        for (int l0 = la; l0 < lb; l0 += PD_WG_CHUNK) {
            float4 a_reg[2], b_reg[2];
            bool a_keep[2], b_keep[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = l0 + ld_row + 16 * i, u = m / p.period, col = m % p.period, hs = u * p.stride + t - p.pad;
                a_keep[i] = m < lb && n_ok;
                b_keep[i] = m < lb && c_ok && hs >= 0 && hs < Hs;
                a_reg[i] = *reinterpret_cast<const float4*>(dy_b + (size_t)(a_keep[i] ? m : 0) * p.NC + (n_ok ? n0 + 4 * ld_c4 : 0));
                b_reg[i] = *reinterpret_cast<const float4*>(x_b + ((size_t)(b_keep[i] ? hs : 0) * p.period + col) * p.KC + (c_ok ? c0 + 4 * ld_c4 : 0));
            }
            __syncthreads();   // the products of the chunk before are done with the LDS
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(&As[(ld_row + 16 * i) * PD_WLD + 4 * ld_c4]) = a_keep[i] ? a_reg[i] : z;
                *reinterpret_cast<float4*>(&Bs[(ld_row + 16 * i) * PD_WLD + 4 * ld_c4]) = b_keep[i] ? b_reg[i] : z;
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < PD_WG_CHUNK / 2; ++ks)
                part = __builtin_amdgcn_mfma_f32_32x32x2f32(As[(2 * ks + hh) * PD_WLD + wr * 32 + r], Bs[(2 * ks + hh) * PD_WLD + wc * 32 + r], part, 0, 0, 0);
            if (++since == 4) {   // 128 positions are summed apart, then added
                since = 0;
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] += part[e], part[e] = 0.f;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] += part[e];
    const int c = c0 + wc * 32 + r;
    if (c >= p.KC) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int n = n0 + wr * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        if (n < p.NC) parts[(((size_t)piece * p.k + t) * p.NC + n) * p.KC + c] = acc[e];
    }
}

// the same piece in VALU code: a thread per (tap, output channel, input channel), the input channel fastest
__global__ void __launch_bounds__(256) pd_wgrad_valu_kernel(const PdConv p, float* parts, int B, int chunks, int rows_per_piece, int run) {
    const size_t numel = (size_t)p.k * p.NC * p.KC;
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= numel) return;
    const int c = (int)(o % p.KC), n = (int)((o / p.KC) % p.NC), t = (int)(o / ((size_t)p.KC * p.NC));
    const int piece = blockIdx.y;
    const PdSpan sp = pd_span(piece, B, chunks, rows_per_piece);
    float acc = 0.f;
    for (int b = sp.b0; b < sp.b1; ++b) {
        const int nb = pd_row_n(p, b);
        const int Hs = pd_height(nb, p.period, p.s, p.down_s), Ho = pd_height(nb, p.period, p.s, p.down_o);
        const int la = sp.chunk * run, lb = min(la + run, Ho * p.period);
        const float* dy_b = p.dy + (size_t)b * p.Ho_max * p.period * p.NC;
        const float* x_b = p.wav_src ? p.src + (size_t)b * p.n_max : p.src + (size_t)b * p.Hs_max * p.period * p.KC;
        float part = 0.f;
        for (int m = la; m < lb; ++m) {
            const int u = m / p.period, col = m % p.period, hs = u * p.stride + t - p.pad;
            if (hs < 0 || hs >= Hs) continue;
            float xv;
            if (p.wav_src) {
                int i = hs * p.period + col;
                i = i >= nb ? 2 * (nb - 1) - i : i;
                xv = i >= 0 ? x_b[i] : 0.f;
            } else {
                xv = x_b[((size_t)hs * p.period + col) * p.KC + c];
            }
            part = fmaf(dy_b[(size_t)m * p.NC + n], xv, part);
        }
        acc += part;
    }
    parts[(size_t)piece * numel + o] = acc;
}

// parts [pieces][tap][n][c] -> out [n][c][tap] (PyTorch's layout): eight lanes per output take every eighth piece in order, and the eight
// sums are added by a fixed butterfly - the same order in every call
__global__ void __launch_bounds__(256) pd_reduce_kernel(const float* parts, float* out, int NC, int KC, int k, int pieces) {
    const size_t numel = (size_t)NC * KC * k;
    const size_t o = ((size_t)blockIdx.x * 256 + threadIdx.x) / 8;
    const int ln = threadIdx.x & 7;
    float v = 0.f;
    if (o < numel) {
        const int t = (int)(o % k), c = (int)((o / k) % KC), n = (int)(o / ((size_t)k * KC));
        const size_t at = ((size_t)t * NC + n) * KC + c;
        for (int i = ln; i < pieces; i += 8) v += parts[(size_t)i * numel + at];
    }
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    if (ln == 0 && o < numel) out[o] = v;
}

// db[n] = sum over rows and positions of dy, in float64 (a bias gradient is a plain sum of cotangents that may cancel): a workgroup
// takes 32 channels and one slice of the flat positions [B][Ho_max][period]; eight lanes per channel stride the slice
__global__ void __launch_bounds__(256) pd_db_kernel(const PdConv p, double* db_parts, int B) {
    __shared__ double red[8][32];
    const int ch = threadIdx.x & 31, ln = threadIdx.x >> 5;
    const int n = (int)blockIdx.x * 32 + ch, slice = blockIdx.y;
    const long per_row = (long)p.Ho_max * p.period, total = per_row * B;
    const long per = (total + PD_DB_SLICES - 1) / PD_DB_SLICES, lo = slice * per, hi = lo + per < total ? lo + per : total;
    double v = 0.0;
    int b_cur = -1, Ho = 0;
    for (long m = lo + ln; m < hi; m += 8) {
        const int b = (int)(m / per_row);
        if (b != b_cur) { b_cur = b; Ho = pd_height(pd_row_n(p, b), p.period, p.s, p.down_o); }
        const long rem = m % per_row;
        if (rem / p.period < Ho && n < p.NC) v += (double)p.dy[(size_t)m * p.NC + n];
    }
    red[ln][ch] = v;
    __syncthreads();
    if (ln == 0 && n < p.NC) {
        double sum = red[0][ch];
        for (int i = 1; i < 8; ++i) sum += red[i][ch];
        db_parts[(size_t)slice * p.NC + n] = sum;
    }
}

__global__ void __launch_bounds__(256) pd_db_reduce_kernel(const double* db_parts, float* out, int NC) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= NC) return;
    double v = 0.0;
    for (int i = 0; i < PD_DB_SLICES; ++i) v += db_parts[(size_t)i * NC + n];
    out[n] = (float)v;
}

// gradient of the waveform through one period: sample i collects its own cell and the cell behind the row that mirrors it; a cell's
// gradient is the first layer's data gradient, gathered by stride phase.  p.dy: gradient of the first layer's pre-activation
// [B][Ho_max][period][NC]; p.W its weights [NC][k].  accumulate: the periods before this one are already in d_wav.
__global__ void __launch_bounds__(256) pd_dwav_kernel(const PdConv p, float* d_wav, int accumulate) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n_max) return;
    const int nb = pd_row_n(p, b);
    float v = 0.f;
    if (i < nb) {
        const int H0 = pd_height(nb, p.period, p.s, 0), Ho = pd_height(nb, p.period, p.s, p.down_o);
        const int mirror = 2 * (nb - 1) - i;
        const int cell[2] = {i, (mirror >= nb && mirror < H0 * p.period) ? mirror : -1};
        const float* dy_b = p.dy + (size_t)b * p.Ho_max * p.period * p.NC;
        for (int q = 0; q < 2; ++q) {
            if (cell[q] < 0) continue;
            const int h = cell[q] / p.period, col = cell[q] % p.period;
            for (int t = 0; t < p.k; ++t) {
                const int num = h + p.pad - t;
                if (num < 0 || num % p.stride || num / p.stride >= Ho) continue;
                const float* d = dy_b + ((size_t)(num / p.stride) * p.period + col) * p.NC;
                float part = 0.f;
                for (int n = 0; n < p.NC; ++n) part = fmaf(d[n], p.W[n * p.k + t], part);
                v += part;
            }
        }
    }
    float* o = d_wav + (size_t)b * p.n_max + i;
    *o = accumulate ? (i < nb ? *o + v : 0.f) : v;
}

// W [n][c][t] (PyTorch) -> wf [n][t][c] and wb [c][t][n]
__global__ void __launch_bounds__(256) pd_pack_kernel(const float* W, float* wf, float* wb, int NC, int KC, int k) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= (size_t)NC * KC * k) return;
    const int t = (int)(o % k), c = (int)((o / k) % KC), n = (int)(o / ((size_t)k * KC));
    wf[((size_t)n * k + t) * KC + c] = W[o];
    wb[((size_t)c * k + t) * NC + n] = W[o];
}

__global__ void __launch_bounds__(256) pd_copy_kernel(float* dst, const float* src, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

PdConv pd_conv(const gvx_hifigan_mpd_dims& d, const PdLayer& l, const PdFeat& F, int j, int i, const int32_t* lens, int n_max) {
    PdConv p{};
    p.lens = lens; p.n_max = n_max; p.min_n = pd_min_samples(d); p.s = d.stride;
    p.period = d.periods[j]; p.KC = l.cin; p.NC = l.cout; p.k = l.k; p.stride = l.stride; p.pad = l.pad;
    p.Hs_max = i == 0 ? pd_height(n_max, p.period, d.stride, 0) : F.height[j][i - 1];
    p.Ho_max = F.height[j][i];
    p.down_s = l.down_in; p.down_o = l.down_out;
    p.act = l.act; p.wav_src = i == 0; p.slope = d.slope;
    return p;
}

// forward of layer (j, i), or with BWD its data gradient: there `p` already has the two sides exchanged
template <bool BWD>
int pd_launch_conv(const PdConv& p, bool mfma, int B, hipStream_t s) {
    const int phases = BWD ? p.stride : 1;
    const int heights = BWD ? (p.Ho_max + p.stride - 1) / p.stride : p.Ho_max;
    const unsigned tiles = (unsigned)(((size_t)heights * p.period + PD_TILE - 1) / PD_TILE);
    if (mfma && p.NC >= PD_TILE_N_WIDE) {   // the wide N tile wherever a whole one fits
        const int n_tiles = (p.NC + PD_TILE_N_WIDE - 1) / PD_TILE_N_WIDE;
        pd_mfma_kernel<BWD, 2><<<dim3(tiles, (unsigned)(n_tiles * phases), (unsigned)B), 256, 0, s>>>(p);
    } else if (mfma) {
        const int n_tiles = (p.NC + PD_TILE_N - 1) / PD_TILE_N;
        pd_mfma_kernel<BWD, 1><<<dim3(tiles, (unsigned)(n_tiles * phases), (unsigned)B), 256, 0, s>>>(p);
    } else {
        const int n_tiles = (p.NC + PD_TILE_N - 1) / PD_TILE_N;
        const dim3 grid(tiles, (unsigned)(n_tiles * phases), (unsigned)B);
        if (p.KC >= 64 && p.KC % 4 == 0 && !p.wav_src) pd_valu_kernel<64, BWD><<<grid, 256, 0, s>>>(p);   // a wave per output element
        else pd_valu_kernel<1, BWD><<<grid, 256, 0, s>>>(p);
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

bool pd_bad_shape(const gvx_hifigan_mpd_dims* dims, int B, int n_max) {
    return pd_dims_problem(dims) || B < 1 || B > 65535 || n_max < pd_min_samples(*dims) || n_max > GVX_HIFIGAN_MPD_MAX_SAMPLES;
}

int pd_check_call(const gvx_hifigan_mpd* h, const float* wav, const void* features, int B, int n_max) {
    if (!h || !wav || !features) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (n_max < pd_min_samples(h->d))
        return fail(GVX_ERR_INVALID_ARG, "n_max = %d: the largest period's reflection needs at least %d samples", n_max, pd_min_samples(h->d));
    if (n_max > GVX_HIFIGAN_MPD_MAX_SAMPLES) return fail(GVX_ERR_UNSUPPORTED, "n_max = %d is beyond the limit of %d samples", n_max, GVX_HIFIGAN_MPD_MAX_SAMPLES);
    return GVX_OK;
}

// the next of a call's marks on the stream: (n_maps + 1) per period, made on first use
int pd_mark(std::vector<hipEvent_t>& ev, size_t at, hipStream_t s) {
    while (ev.size() <= at) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
    }
    HIP_TRY(hipEventRecord(ev[at], s));
    return GVX_OK;
}

std::string pd_name(int j, int i, int nl) {
    return "discriminators." + std::to_string(j) + (i == nl - 1 ? std::string(".conv_post") : ".convs." + std::to_string(i));
}

}  // namespace

extern "C" {

size_t gvx_hifigan_mpd_blob_floats(const gvx_hifigan_mpd_dims* dims) {
    if (pd_dims_problem(dims)) return 0;
    PdLayer L[PD_MAX_MAPS];
    size_t per_period = 0;
    pd_layers(*dims, L, &per_period);
    return per_period * dims->n_periods;
}

int gvx_hifigan_mpd_layout(const gvx_hifigan_mpd_dims* dims, int B, int n_max, gvx_hifigan_mpd_entry* entries, int max_entries) {
    if (pd_bad_shape(dims, B, n_max)) return 0;
    const PdFeat F = pd_feat_layout(*dims, B, n_max);
    int n = 0;
    for (int j = 0; j < dims->n_periods; ++j)
        for (int i = 0; i < F.n_maps; ++i, ++n)
            if (entries && n < max_entries) {
                const int64_t C = F.channels[i], P = dims->periods[j], H = F.height[j][i];
                entries[n] = gvx_hifigan_mpd_entry{(uint64_t)F.off[j][i], (int32_t)C, (int32_t)H, (int32_t)P, 0, H * P * C, 1, P * C, C};
            }
    return n;
}

size_t gvx_hifigan_mpd_features_bytes(const gvx_hifigan_mpd_dims* dims, int B, int n_max) {
    if (pd_bad_shape(dims, B, n_max)) return 0;
    return pd_feat_layout(*dims, B, n_max).total;
}

size_t gvx_hifigan_mpd_workspace_bytes(const gvx_hifigan_mpd_dims* dims, int B, int n_max, int backward) {
    if (pd_bad_shape(dims, B, n_max)) return 0;
    return pd_ws_plan(*dims, B, n_max, backward != 0).total;
}

int gvx_hifigan_mpd_pack_weights_device(const gvx_hifigan_mpd_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = pd_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    PdLayer L[PD_MAX_MAPS];
    size_t per_period = 0;
    const int nl = pd_layers(*dims, L, &per_period);
    struct Job { int j, i; const float* w; const float* b; };
    std::vector<Job> jobs;
    int rc = GVX_OK;
    for (int j = 0; j < dims->n_periods; ++j)
        for (int i = 0; i < nl; ++i) {
            const std::string name = pd_name(j, i, nl);
            const gvx_weight_desc* w = gvx_mg::mg_find(table, n, name + ".weight", (size_t)L[i].cout * L[i].cin * L[i].k, rc);
            if (!w) return rc;
            const gvx_weight_desc* bs = gvx_mg::mg_find(table, n, name + ".bias", (size_t)L[i].cout, rc);
            if (!bs) return rc;   // nothing was launched
            jobs.push_back({j, i, w->data, bs->data});
        }
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(device_blob, 0, per_period * dims->n_periods * sizeof(float), s));   // the padding between the tensors
    for (const Job& jb : jobs) {
        const PdLayer& l = L[jb.i];
        float* base = device_blob + jb.j * per_period;
        const size_t wn = (size_t)l.cout * l.cin * l.k;
        pd_pack_kernel<<<(unsigned)((wn + 255) / 256), 256, 0, s>>>(jb.w, base + l.wf_off, base + l.wb_off, l.cout, l.cin, l.k);
        HIP_TRY(hipGetLastError());
        pd_copy_kernel<<<(unsigned)((l.cout + 255) / 256), 256, 0, s>>>(base + l.b_off, jb.b, (size_t)l.cout);
        HIP_TRY(hipGetLastError());
    }
    return GVX_OK;
}

int gvx_hifigan_mpd_create(const gvx_hifigan_mpd_dims* dims, gvx_hifigan_mpd** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = pd_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_hifigan_mpd* h = new gvx_hifigan_mpd();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_hifigan_mpd_destroy(gvx_hifigan_mpd* h) {
    if (!h) return;
    for (hipEvent_t e : h->fwd_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->bwd_ev) (void)hipEventDestroy(e);
    delete h;
}

int gvx_hifigan_mpd_timing_enable(gvx_hifigan_mpd* h, int enable) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    h->timing = enable != 0;
    h->fwd_timed = h->bwd_timed = false;
    return GVX_OK;
}

int gvx_hifigan_mpd_layer_times_ms(gvx_hifigan_mpd* h, float* forward_ms, float* backward_ms, int* n_layers_out) {
    if (!h || !forward_ms || !backward_ms || !n_layers_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    PdLayer L[PD_MAX_MAPS];
    const int nl = pd_layers(h->d, L);
    *n_layers_out = nl;
    for (int i = 0; i < nl; ++i) forward_ms[i] = backward_ms[i] = 0.f;
    for (int j = 0; j < h->d.n_periods; ++j)
        for (int i = 0; i < nl; ++i) {
            const size_t at = (size_t)j * (nl + 1) + i;
            float ms = 0.f;
            if (h->fwd_timed) {
                HIP_TRY(hipEventSynchronize(h->fwd_ev[at + 1]));
                HIP_TRY(hipEventElapsedTime(&ms, h->fwd_ev[at], h->fwd_ev[at + 1]));
                forward_ms[i] += ms;
            }
            if (h->bwd_timed) {   // the backward walks down: mark i + 1 comes before mark i
                HIP_TRY(hipEventSynchronize(h->bwd_ev[at]));
                HIP_TRY(hipEventElapsedTime(&ms, h->bwd_ev[at + 1], h->bwd_ev[at]));
                backward_ms[i] += ms;
            }
        }
    return GVX_OK;
}

int gvx_hifigan_mpd_bind(gvx_hifigan_mpd* h, const float* device_blob) {
    if (!h || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if ((uintptr_t)device_blob % 256) return fail(GVX_ERR_INVALID_ARG, "the blob must be 256-byte aligned");
    h->blob = device_blob;
    return GVX_OK;
}

int gvx_hifigan_mpd_forward(gvx_hifigan_mpd* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features,
                            size_t features_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = pd_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    const gvx_hifigan_mpd_dims& d = h->d;
    const PdFeat F = pd_feat_layout(d, B, n_max);
    if ((uintptr_t)features % 256 || features_bytes < F.total)
        return fail(GVX_ERR_WORKSPACE, "the features buffer is misaligned or smaller than %zu bytes", F.total);
    const PdWs wp = pd_ws_plan(d, B, n_max, false);
    if (!workspace || (uintptr_t)workspace % 256 || workspace_bytes < wp.total)
        return fail(GVX_ERR_WORKSPACE, "the workspace is missing, misaligned or smaller than %zu bytes", wp.total);
    hipStream_t s = (hipStream_t)stream;
    PdLayer L[PD_MAX_MAPS];
    size_t per_period = 0;
    const int nl = pd_layers(d, L, &per_period);
    for (int j = 0; j < d.n_periods; ++j) {
        const float* in = wav;
        if (h->timing && (rc = pd_mark(h->fwd_ev, (size_t)j * (nl + 1), s)) != GVX_OK) return rc;
        for (int i = 0; i < nl; ++i) {
            PdConv p = pd_conv(d, L[i], F, j, i, sample_lengths, n_max);
            p.src = in; p.W = h->blob + j * per_period + L[i].wf_off; p.bias = h->blob + j * per_period + L[i].b_off;
            p.out = gvx::ws_ptr<float>(features, F.off[j][i]);
            if ((rc = pd_launch_conv<false>(p, L[i].mfma != 0, B, s)) != GVX_OK) return rc;
            in = p.out;
            if (h->timing && (rc = pd_mark(h->fwd_ev, (size_t)j * (nl + 1) + i + 1, s)) != GVX_OK) return rc;
        }
    }
    h->fwd_timed = h->timing;
    return GVX_OK;
}

int gvx_hifigan_mpd_backward(gvx_hifigan_mpd* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, const void* features,
                             const void* d_features, const gvx_grad_desc* grads, int n_grads, float* d_wav,
                             void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = pd_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    if (!d_features) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_grads < 0 || (n_grads > 0 && !grads)) return fail(GVX_ERR_INVALID_ARG, "n_grads = %d without a table", n_grads);
    if (n_grads == 0 && !d_wav) return fail(GVX_ERR_INVALID_ARG, "neither parameter gradients nor d_wav are asked for");
    const gvx_hifigan_mpd_dims& d = h->d;
    const PdFeat F = pd_feat_layout(d, B, n_max);
    if ((uintptr_t)features % 256 || (uintptr_t)d_features % 256) return fail(GVX_ERR_WORKSPACE, "features or d_features is not 256-byte aligned");
    const PdWs wp = pd_ws_plan(d, B, n_max, true);
    if (!workspace || (uintptr_t)workspace % 256 || workspace_bytes < wp.total)
        return fail(GVX_ERR_WORKSPACE, "the workspace is missing, misaligned or smaller than %zu bytes", wp.total);
    PdLayer L[PD_MAX_MAPS];
    size_t per_period = 0;
    const int nl = pd_layers(d, L, &per_period);
    float* gw[GVX_HIFIGAN_MPD_MAX_PERIODS][PD_MAX_MAPS] = {};
    float* gb[GVX_HIFIGAN_MPD_MAX_PERIODS][PD_MAX_MAPS] = {};
    if (n_grads > 0) {
        const gvx_weight_desc* table = reinterpret_cast<const gvx_weight_desc*>(grads);   // same fields, the data pointer writable
        static_assert(sizeof(gvx_weight_desc) == sizeof(gvx_grad_desc), "the two tables share a layout");
        for (int j = 0; j < d.n_periods; ++j)
            for (int i = 0; i < nl; ++i) {
                const std::string name = pd_name(j, i, nl);
                rc = GVX_OK;
                const gvx_weight_desc* w = gvx_mg::mg_find(table, n_grads, name + ".weight", (size_t)L[i].cout * L[i].cin * L[i].k, rc);
                if (!w) return rc;
                gw[j][i] = const_cast<float*>(w->data);
                w = gvx_mg::mg_find(table, n_grads, name + ".bias", (size_t)L[i].cout, rc);
                if (!w) return rc;
                gb[j][i] = const_cast<float*>(w->data);
            }
    }
    hipStream_t s = (hipStream_t)stream;
    float* gbuf[2] = {gvx::ws_ptr<float>(workspace, wp.grad[0]), gvx::ws_ptr<float>(workspace, wp.grad[1])};
    float* parts = gvx::ws_ptr<float>(workspace, wp.parts);
    double* db_parts = gvx::ws_ptr<double>(workspace, wp.db_parts);
    auto feat = [&](const void* base, int j, int i) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + F.off[j][i]); };
    for (int j = 0; j < d.n_periods; ++j) {
        const float* blob = h->blob + j * per_period;
        const float* dcur = feat(d_features, j, nl - 1);   // the score has no activation: its cotangent is its pre-activation's
        if (h->timing && (rc = pd_mark(h->bwd_ev, (size_t)j * (nl + 1) + nl, s)) != GVX_OK) return rc;
        for (int i = nl - 1; i >= 0; --i) {
            PdConv p = pd_conv(d, L[i], F, j, i, sample_lengths, n_max);
            if (n_grads > 0) {
                p.src = i == 0 ? wav : feat(features, j, i - 1);
                p.dy = dcur;
                const PdPieces P = pd_pieces(L[i], B, p.Ho_max * p.period);
                if (L[i].mfma)
                    pd_wgrad_mfma_kernel<<<dim3((unsigned)((p.NC + 63) / 64), (unsigned)((p.KC + 63) / 64), (unsigned)(P.n * p.k)), 256, 0, s>>>(
                        p, parts, B, P.chunks, P.rows_per_piece, P.run);
                else
                    pd_wgrad_valu_kernel<<<dim3((unsigned)((P.numel + 255) / 256), (unsigned)P.n), 256, 0, s>>>(p, parts, B, P.chunks, P.rows_per_piece, P.run);
                HIP_TRY(hipGetLastError());
                pd_reduce_kernel<<<(unsigned)((P.numel + 31) / 32), 256, 0, s>>>(parts, gw[j][i], p.NC, p.KC, p.k, P.n);
                HIP_TRY(hipGetLastError());
                pd_db_kernel<<<dim3((unsigned)((p.NC + 31) / 32), PD_DB_SLICES), 256, 0, s>>>(p, db_parts, B);
                HIP_TRY(hipGetLastError());
                pd_db_reduce_kernel<<<(unsigned)((p.NC + 255) / 256), 256, 0, s>>>(db_parts, gb[j][i], p.NC);
                HIP_TRY(hipGetLastError());
            }
            if (i > 0) {
                // the data gradient is a convolution with the sides exchanged: dY is the operand, the layer's input map the output
                PdConv q = p;
                q.src = dcur; q.W = blob + L[i].wb_off; q.bias = nullptr; q.dy = nullptr;
                q.KC = L[i].cout; q.NC = L[i].cin;
                q.Hs_max = p.Ho_max; q.Ho_max = p.Hs_max; q.down_s = L[i].down_out; q.down_o = L[i].down_in;
                q.wav_src = 0;
                q.mask = feat(features, j, i - 1);
                q.dfeat = feat(d_features, j, i - 1);
                q.out = gbuf[i & 1];
                if ((rc = pd_launch_conv<true>(q, L[i].mfma != 0, B, s)) != GVX_OK) return rc;
                dcur = q.out;
            } else if (d_wav) {
                p.dy = dcur; p.W = blob + L[0].wf_off;
                pd_dwav_kernel<<<dim3((unsigned)((n_max + 255) / 256), (unsigned)B), 256, 0, s>>>(p, d_wav, j > 0);
                HIP_TRY(hipGetLastError());
            }
            if (h->timing && (rc = pd_mark(h->bwd_ev, (size_t)j * (nl + 1) + i, s)) != GVX_OK) return rc;   // mark i: layer i is done
        }
    }
    h->bwd_timed = h->timing;
    return GVX_OK;
}

}  // C ABI
