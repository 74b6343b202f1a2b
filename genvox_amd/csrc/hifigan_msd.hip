// HiFi-GAN scale discriminators (include/genvox_amd.h, "HiFi-GAN scale discriminators"): forward, and the backward that reads the
// forward's own maps as its tape.  Maps are channels-last, [B][length][channels]: a group's channels are contiguous at a position, which
// is what an implicit GEMM with positions on M and taps x group channels on K wants.  The waveform of a scale is such a map of 1 channel.
//
// A workgroup owns SD_TILE positions of one row.  In a forward kernel position m is the output position; in a data gradient the
// workgroup belongs to ONE stride phase ph and the input position is l = m * stride + ph, so that only the taps
// t = (ph + pad) mod stride, + stride, ... meet a dY position - the gather by stride phase.
//   sd_mfma_kernel     the grouped and the dense layers, forward (BWD = false) and data gradient (BWD = true): 64 positions x 16, 32 or 64
//                      channels of one group.  The window of the operand that the tile's taps touch - (SD_TILE - 1) * stride + k rows
//                      of a block of the group's channels, zeros outside the row - is staged into LDS once per channel block, and every
//                      tap runs off a row offset in it; the weights come as [group][tap][k channel][n channel], a coalesced read per
//                      fragment.  MF = 32: v_mfma_f32_32x32x2_f32, two waves on M; MF = 16: v_mfma_f32_16x16x4_f32, four waves on M.
//                      Eight taps are summed apart and then added, so the products never form one chain.
//   sd_valu_kernel     the same two products in fp32 VALU code, G lanes per output element: the first layer, the score (G = 64: the
//                      input channels dealt over a wave, added by a fixed butterfly) and narrow layers.
//   sd_wgrad_mfma_kernel / sd_wgrad_valu_kernel   one piece (rows, or a run of positions of one row) of a weight gradient in PyTorch's
//                      layout; the matrix form is a per-group GEMM with positions on K, a wave per tap; sd_reduce_kernel adds the pieces
//                      in their order.
//   sd_db_kernel       bias gradients in float64 slices, added in their order.
//   sd_pool_kernel     AvgPool1d(4, 2, 2) of a row at its own length; sd_dwav_kernel the first layer's data gradient plus the pooling's
//                      adjoint of the next scale's waveform gradient, both as gathers, the channels in the lanes of a wave.
// No atomics anywhere: two calls give the same bits.
#include "gvx_internal.h"
#include "hifigan_msd_internal.h"
#include "melgan_internal.h"

#include <string>
#include <vector>

using gvx::fail;
using namespace gvx_sd;

static_assert(SD_TILE == GVX_HIFIGAN_MSD_TILE && SD_MFMA_IN == GVX_HIFIGAN_MSD_MFMA_IN_MULT && SD_MFMA_OUT == GVX_HIFIGAN_MSD_MFMA_OUT_MULT &&
                  SD_WG_RUN == GVX_HIFIGAN_MSD_WG_RUN,
              "the public header states the tile constants");

struct gvx_hifigan_msd {
    gvx_hifigan_msd_dims d;
    const float* blob = nullptr;
    bool timing = false;                     // measurement only: events around every layer of the last forward / backward
    std::vector<hipEvent_t> fwd_ev, bwd_ev;  // per scale n_maps + 1 marks
    bool fwd_timed = false, bwd_timed = false;
};

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

struct SdConv {
    const float* src;     // the operand: forward [B][Ls_max][KC] (layer 0: the scale's waveform, KC = 1); data gradient dY
    const float* W;       // VALU: [NC][taps][KG]; matrix: [groups][taps][KG][NG]
    const float* bias;    // forward
    float* out;           // [B][Lo_max][NC]
    const float* dfeat;   // data gradient: cotangent of the map that `out` is the gradient of (added before its mask)
    const float* mask;    // data gradient: that map itself, for its sign
    const float* dy;      // weight gradient: [B][Lo_max][NC] against src [B][Ls_max][KC]
    const int32_t* lens;
    int n_max, scale;
    int KC, NC, KG, NG;   // channels of the operand and of the output, in all and per group
    int k, stride, pad;
    int Ls_max, Lo_max;
    int n_src, n_out;     // how many of str[] lie in front of the operand's / the output's length
    int str[SD_MAX_MAPS];
    int act, cb;          // cb: the matrix kernels' channel block
    float slope;
};

__device__ __forceinline__ int sd_row_n(const SdConv& p, int b) {
    int n = p.lens ? p.lens[b] : p.n_max;
    n = n > p.n_max ? p.n_max : n;
    return sd_scale_n(n, p.scale);   // rows the caller should have refused are silent, never a bad address
}

// how the taps of one workgroup walk the operand's positions: tap j (weight tap t0 + j * tstep) of position m reads position
// m * mul + base + j * hstep
struct SdTaps { int n, t0, tstep, mul, base, hstep; };

template <bool BWD>
__device__ __forceinline__ SdTaps sd_taps(const SdConv& p, int ph) {
    if constexpr (!BWD) return SdTaps{p.k, 0, 1, p.stride, -p.pad, 1};
    const int t0 = (ph + p.pad) % p.stride;
    return SdTaps{t0 < p.k ? (p.k - 1 - t0) / p.stride + 1 : 0, t0, p.stride, 1, (ph + p.pad - t0) / p.stride, -1};
}

// a tile behind its row: exact zeros inside the buffer, channels [c0, c0 + cols)
template <bool BWD>
__device__ __forceinline__ void sd_zero_tile(const SdConv& p, int b, int m0, int ph, int c0, int cols) {
    for (int idx = threadIdx.x; idx < SD_TILE * cols; idx += blockDim.x) {
        const int m = m0 + idx / cols;
        const int h = BWD ? m * p.stride + ph : m;
        if (h < p.Lo_max) p.out[((size_t)b * p.Lo_max + h) * p.NC + c0 + idx % cols] = 0.f;
    }
}

template <bool BWD>
__device__ __forceinline__ void sd_finish(const SdConv& p, int b, int h, int n, int Lo, float v) {
    if (h >= p.Lo_max) return;
    const size_t at = ((size_t)b * p.Lo_max + h) * p.NC + n;
    if (h >= Lo) { p.out[at] = 0.f; return; }
    if constexpr (BWD) {
        if (p.dfeat) v += p.dfeat[at];
        v = p.mask[at] > 0.f ? v : v * p.slope;
    } else {
        v += p.bias[n];
        if (p.act) v = v > 0.f ? v : v * p.slope;
    }
    p.out[at] = v;
}

// MF x MF tiles of the matrix instruction: 64 / MF waves on M, WN waves on N
template <bool BWD, int MF, int WN>
__global__ void __launch_bounds__(64 * (64 / MF) * WN) sd_mfma_kernel(const SdConv p) {
    constexpr int WM = 64 / MF, NT = MF * WN, THREADS = 64 * WM * WN, NACC = MF == 32 ? 16 : 4, KS = 64 / MF;
    using acc_t = __attribute__((ext_vector_type(NACC))) float;
    extern __shared__ __attribute__((aligned(16))) float win[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave % WM, wn = wave / WM, r = lane % MF, kq = lane / MF;
    const int b = blockIdx.z;
    const int groups = p.NC / p.NG;
    const int n_tiles = (p.NG + NT - 1) / NT;
    int y = blockIdx.y;
    const int nt = y % n_tiles;
    y /= n_tiles;
    const int g = y % groups, ph = y / groups;
    const int m0 = (int)blockIdx.x * SD_TILE;
    const int ns = sd_row_n(p, b);
    const int Ls = sd_length(ns, p.str, p.n_src), Lo = sd_length(ns, p.str, p.n_out);
    const int first = BWD ? m0 * p.stride + ph : m0;
    if (first >= Lo) {
        const int c0 = nt * NT;
        sd_zero_tile<BWD>(p, b, m0, ph, g * p.NG + c0, min(NT, p.NG - c0));
        return;
    }
    const SdTaps tp = sd_taps<BWD>(p, ph);
    const int cb = p.cb, ldw = cb + 1;   // an odd row: positions a stride apart fall on distinct banks
    const int row0 = BWD ? m0 + tp.base - (tp.n - 1) : m0 * p.stride - p.pad;
    const int wrows = BWD ? SD_TILE + tp.n - 1 : (SD_TILE - 1) * p.stride + p.k;
    const float* src_b = p.src + (size_t)b * p.Ls_max * p.KC + (size_t)g * p.KG;
    const int ml = wm * MF + r;   // this lane's position of the tile, as the A operand's row
    const int n_l = nt * NT + wn * MF + r;
    const bool n_ok = n_l < p.NG;
    const float* w_g = p.W + (size_t)g * p.k * p.KG * p.NG + (n_ok ? n_l : 0);
    acc_t acc, part;
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] = 0.f, part[e] = 0.f;
    for (int c0 = 0; c0 < p.KG; c0 += cb) {
        if (c0) __syncthreads();   // the products of the block before are done with the window
        for (int idx = tid; idx < wrows * cb; idx += THREADS) {
            const int w = idx / cb, c = idx % cb, hs = row0 + w;
            win[w * ldw + c] = (hs >= 0 && hs < Ls) ? src_b[(size_t)hs * p.KC + c0 + c] : 0.f;
        }
        __syncthreads();
        for (int j = 0; j < tp.n; ++j) {
            const int arow = BWD ? ml + tp.n - 1 - j : ml * p.stride + j;
            const float* a = &win[arow * ldw + kq];
            const float* wv = w_g + ((size_t)(tp.t0 + j * tp.tstep) * p.KG + c0 + kq) * p.NG;
            for (int k0 = 0; k0 < cb; k0 += 8) {   // cb is a multiple of 8: the fragments of 8 channels are in flight together
                float av[8 / KS], bv[8 / KS];
#pragma unroll
                for (int u = 0; u < 8 / KS; ++u) {
                    av[u] = a[k0 + u * KS];
                    bv[u] = n_ok ? wv[(size_t)(k0 + u * KS) * p.NG] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 8 / KS; ++u) {
                    if constexpr (MF == 32) part = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], part, 0, 0, 0);
                    else part = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], part, 0, 0, 0);
                }
            }
            if ((j & 7) == 7) {
#pragma unroll
                for (int e = 0; e < NACC; ++e) acc[e] += part[e], part[e] = 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < NACC; ++e) acc[e] += part[e], part[e] = 0.f;
    }
    // epilogue: a lane holds column r of rows (e & 3) + 8 (e >> 2) + 4 kq of its 32 x 32 tile, or of rows 4 kq + e of its 16 x 16 tile
    if (!n_ok) return;
#pragma unroll
    for (int e = 0; e < NACC; ++e) {
        const int row = MF == 32 ? (e & 3) + 8 * (e >> 2) + 4 * kq : 4 * kq + e;
        const int m = m0 + wm * MF + row;
        sd_finish<BWD>(p, b, BWD ? m * p.stride + ph : m, g * p.NG + n_l, Lo, acc[e]);
    }
}

// G lanes per output element (position, channel), channel fastest; the G partial sums are added by a fixed butterfly
template <int G, bool BWD>
__global__ void __launch_bounds__(256) sd_valu_kernel(const SdConv p) {
    const int b = blockIdx.z;
    const int n_tiles = (p.NC + SD_TILE_N - 1) / SD_TILE_N;
    const int n0 = ((int)blockIdx.y % n_tiles) * SD_TILE_N, ph = (int)blockIdx.y / n_tiles;
    const int cols = min(SD_TILE_N, p.NC - n0);
    const int m0 = (int)blockIdx.x * SD_TILE;
    const int ns = sd_row_n(p, b);
    const int Ls = sd_length(ns, p.str, p.n_src), Lo = sd_length(ns, p.str, p.n_out);
    const int first = BWD ? m0 * p.stride + ph : m0;
    if (first >= Lo) {
        sd_zero_tile<BWD>(p, b, m0, ph, n0, cols);
        return;
    }
    const SdTaps tp = sd_taps<BWD>(p, ph);
    const int K = p.k * p.KG;
    const float* src_b = p.src + (size_t)b * p.Ls_max * p.KC;
    const int total = SD_TILE * cols * G;   // G = 64: a multiple of 256, so the lanes of a wave stay together for the butterfly
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int gl = idx % G, el = idx / G, n = n0 + el % cols, m = m0 + el / cols;
        const int h = BWD ? m * p.stride + ph : m;
        float sum = 0.f;
        if (h < Lo) {
            const float* w = p.W + (size_t)n * K;
            const int xg = (n / p.NG) * p.KG;
            for (int j = 0; j < tp.n; ++j) {
                const int hs = m * tp.mul + tp.base + j * tp.hstep;
                if (hs < 0 || hs >= Ls) continue;
                const float* wt = w + (size_t)(tp.t0 + j * tp.tstep) * p.KG;
                const float* x = src_b + (size_t)hs * p.KC + xg;
                float run = 0.f;
                if constexpr (G > 1) {   // KG is a multiple of 4 here (sd_launch_conv): a lane takes whole float4s
                    for (int c = 4 * gl; c < p.KG; c += 4 * G) {
                        const float4 xv = *reinterpret_cast<const float4*>(x + c), wv = *reinterpret_cast<const float4*>(wt + c);
                        run = fmaf(xv.w, wv.w, fmaf(xv.z, wv.z, fmaf(xv.y, wv.y, fmaf(xv.x, wv.x, run))));
                    }
                } else {
                    for (int c = 0; c < p.KG; ++c) run = fmaf(x[c], wt[c], run);
                }
                sum += run;
            }
        }
#pragma unroll
        for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (gl == 0) sd_finish<BWD>(p, b, h, n, Lo, sum);
    }
}

// the positions [la, lb) of row b that a weight-gradient piece sums: rows dealt to pieces, or a row cut into runs
struct SdSpan { int b0, b1, chunk; };
__device__ __forceinline__ SdSpan sd_span(int piece, int B, int chunks, int rows_per_piece) {
    if (chunks > 1) return SdSpan{piece / chunks, piece / chunks + 1, piece % chunks};
    const int b0 = piece * rows_per_piece;
    return SdSpan{b0, b0 + rows_per_piece < B ? b0 + rows_per_piece : B, 0};
}

// one piece of dW[n][c][t] = sum over positions l of dY[l][n] X[l * stride + t - pad][c] inside a group: an MF x MF tile (n on M, c on
// N) of one tap per wave, positions on k; both operands are read as they lie, a position's channels being contiguous
template <int MF>
__global__ void __launch_bounds__(256) sd_wgrad_mfma_kernel(const SdConv p, float* parts, int B, int chunks, int rows_per_piece, int run) {
    constexpr int NACC = MF == 32 ? 16 : 4, KS = 64 / MF;
    using acc_t = __attribute__((ext_vector_type(NACC))) float;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane % MF, kq = lane / MF;
    const int t = (int)blockIdx.y * 4 + wave;
    if (t >= p.k) return;   // no barrier below
    const int nT = p.NG / MF, cT = (p.KG + MF - 1) / MF;
    int x = blockIdx.x;
    const int ct = x % cT;
    x /= cT;
    const int ntile = x % nT, g = x / nT;
    const int piece = blockIdx.z;
    const SdSpan sp = sd_span(piece, B, chunks, rows_per_piece);
    const int n = g * p.NG + ntile * MF + r, c_l = ct * MF + r;
    const bool c_ok = c_l < p.KG;
    const int c = g * p.KG + (c_ok ? c_l : 0);
    acc_t acc, part;
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] = 0.f, part[e] = 0.f;
    int since = 0;
    for (int b = sp.b0; b < sp.b1; ++b) {
        const int ns = sd_row_n(p, b);
        const int Ls = sd_length(ns, p.str, p.n_src), Lo = sd_length(ns, p.str, p.n_out);
        const int la = sp.chunk * run, lb = min(la + run, Lo);
        const float* dy_b = p.dy + (size_t)b * p.Lo_max * p.NC + n;
        const float* x_b = p.src + (size_t)b * p.Ls_max * p.KC + c;
        for (int l0 = la; l0 < lb; l0 += 4 * KS) {   // four k-steps' fragments in flight together; positions past the run multiply zeros
            float av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int l = l0 + u * KS + kq, hs = l * p.stride + t - p.pad;
                const bool live = l < lb;
                av[u] = live ? dy_b[(size_t)l * p.NC] : 0.f;
                bv[u] = (live && c_ok && hs >= 0 && hs < Ls) ? x_b[(size_t)hs * p.KC] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if constexpr (MF == 32) part = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], part, 0, 0, 0);
                else part = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], part, 0, 0, 0);
            }
            if (++since == 8) {   // 32 k-steps (64 or 128 positions) are summed apart, then added
                since = 0;
#pragma unroll
                for (int e = 0; e < NACC; ++e) acc[e] += part[e], part[e] = 0.f;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] += part[e];
    if (!c_ok) return;
    const size_t numel = (size_t)p.NC * p.KG * p.k;
#pragma unroll
    for (int e = 0; e < NACC; ++e) {
        const int row = MF == 32 ? (e & 3) + 8 * (e >> 2) + 4 * kq : 4 * kq + e;
        const int nn = g * p.NG + ntile * MF + row;
        parts[(size_t)piece * numel + ((size_t)nn * p.KG + c_l) * p.k + t] = acc[e];
    }
}

// the same piece in VALU code: a thread per (output channel, group input channel, tap), PyTorch's order
__global__ void __launch_bounds__(256) sd_wgrad_valu_kernel(const SdConv p, float* parts, int B, int chunks, int rows_per_piece, int run) {
    const size_t numel = (size_t)p.NC * p.KG * p.k;
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= numel) return;
    const int t = (int)(o % p.k), c_l = (int)((o / p.k) % p.KG), n = (int)(o / ((size_t)p.k * p.KG));
    const int c = (n / p.NG) * p.KG + c_l;
    const int piece = blockIdx.y;
    const SdSpan sp = sd_span(piece, B, chunks, rows_per_piece);
    float acc = 0.f;
    for (int b = sp.b0; b < sp.b1; ++b) {
        const int ns = sd_row_n(p, b);
        const int Ls = sd_length(ns, p.str, p.n_src), Lo = sd_length(ns, p.str, p.n_out);
        const int la = sp.chunk * run, lb = min(la + run, Lo);
        const float* dy_b = p.dy + (size_t)b * p.Lo_max * p.NC + n;
        const float* x_b = p.src + (size_t)b * p.Ls_max * p.KC + c;
        float part = 0.f;
        for (int l = la; l < lb; ++l) {
            const int hs = l * p.stride + t - p.pad;
            if (hs < 0 || hs >= Ls) continue;
            part = fmaf(dy_b[(size_t)l * p.NC], x_b[(size_t)hs * p.KC], part);
        }
        acc += part;
    }
    parts[(size_t)piece * numel + o] = acc;
}

// parts [pieces][numel] -> out [numel], both in PyTorch's layout: eight lanes per output take every eighth piece in order, and the
// eight sums are added by a fixed butterfly - the same order in every call
__global__ void __launch_bounds__(256) sd_reduce_kernel(const float* parts, float* out, size_t numel, int pieces) {
    const size_t o = ((size_t)blockIdx.x * 256 + threadIdx.x) / 8;
    const int ln = threadIdx.x & 7;
    float v = 0.f;
    if (o < numel)
        for (int i = ln; i < pieces; i += 8) v += parts[(size_t)i * numel + o];
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    if (ln == 0 && o < numel) out[o] = v;
}

// db[n] = sum over rows and positions of dy, in float64 (a bias gradient is a plain sum of cotangents that may cancel): a workgroup
// takes 32 channels and one slice of the flat positions [B][Lo_max]; eight lanes per channel stride the slice
__global__ void __launch_bounds__(256) sd_db_kernel(const SdConv p, double* db_parts, int B) {
    __shared__ double red[8][32];
    const int ch = threadIdx.x & 31, ln = threadIdx.x >> 5;
    const int n = (int)blockIdx.x * 32 + ch, slice = blockIdx.y;
    const long per_row = p.Lo_max, total = per_row * B;
    const long per = (total + SD_DB_SLICES - 1) / SD_DB_SLICES, lo = slice * per, hi = lo + per < total ? lo + per : total;
    double v = 0.0;
    int b_cur = -1, Lo = 0;
    for (long m = lo + ln; m < hi; m += 8) {
        const int b = (int)(m / per_row);
        if (b != b_cur) { b_cur = b; Lo = sd_length(sd_row_n(p, b), p.str, p.n_out); }
        if (m % per_row < Lo && n < p.NC) v += (double)p.dy[(size_t)m * p.NC + n];
    }
    red[ln][ch] = v;
    __syncthreads();
    if (ln == 0 && n < p.NC) {
        double sum = red[0][ch];
        for (int i = 1; i < 8; ++i) sum += red[i][ch];
        db_parts[(size_t)slice * p.NC + n] = sum;
    }
}

__global__ void __launch_bounds__(256) sd_db_reduce_kernel(const double* db_parts, float* out, int NC) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= NC) return;
    double v = 0.0;
    for (int i = 0; i < SD_DB_SLICES; ++i) v += db_parts[(size_t)i * NC + n];
    out[n] = (float)v;
}

// the waveform of scale s + 1 from that of scale s (rows [B][n_in_max] -> [B][n_out_max]): y[j] = (the sum of x[2j - 2 .. 2j + 1]
// inside the row) / 4 for j = 0 .. n / 2, zeros behind
__global__ void __launch_bounds__(256) sd_pool_kernel(const float* in, float* out, const int32_t* lens, int n_max, int s, int n_in_max, int n_out_max) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_out_max) return;
    int n = lens ? lens[b] : n_max;
    n = sd_scale_n(n > n_max ? n_max : n, s);
    float v = 0.f;
    if (n > 0 && j <= n / 2) {
        const float* x = in + (size_t)b * n_in_max;
        for (int i = 2 * j - 2; i <= 2 * j + 1; ++i)
            if (i >= 0 && i < n) v += x[i];
        v *= 0.25f;
    }
    out[(size_t)b * n_out_max + j] = v;
}

// gradient of the waveform of one scale: the first layer's data gradient, gathered by stride phase (p.dy: gradient of the first layer's
// pre-activation [B][Lo_max][NC]; p.W its weights [NC][k]), plus the pooling's adjoint of the next scale's waveform gradient `next`
// ([B][n_next_max], or NULL behind the last scale): sample i lies in the windows of the pooled positions i / 2 and i / 2 + 1.
// A wave takes SD_DWAV_RUN samples one after another, its lanes the channels (a position's channels are one contiguous read); a
// lane sums its channels over the taps, and the 64 sums are added by a fixed butterfly.
constexpr int SD_DWAV_RUN = 16;
__global__ void __launch_bounds__(256) sd_dwav_kernel(const SdConv p, const float* next, int n_next_max, float* out) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = ((int)blockIdx.x * 4 + wave) * SD_DWAV_RUN, i1 = min(i0 + SD_DWAV_RUN, p.Ls_max);
    const int ns = sd_row_n(p, b);
    const int Lo = sd_length(ns, p.str, p.n_out);
    const float* dy_b = p.dy + (size_t)b * p.Lo_max * p.NC;
    for (int i = i0; i < i1; ++i) {   // i and every test on it are the same in all lanes
        float v = 0.f;
        if (i < ns) {
            for (int t = 0; t < p.k; ++t) {
                const int num = i + p.pad - t;
                if (num < 0 || num % p.stride || num / p.stride >= Lo) continue;
                const float* d = dy_b + (size_t)(num / p.stride) * p.NC;
                for (int n = lane; n < p.NC; n += 64) v = fmaf(d[n], p.W[n * p.k + t], v);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane) continue;
        if (i < ns && next) {
            const float* g = next + (size_t)b * n_next_max;
            const int j = i / 2;
            float a = g[j];
            if (j + 1 <= ns / 2) a += g[j + 1];
            v += 0.25f * a;
        }
        out[(size_t)b * p.Ls_max + i] = i < ns ? v : 0.f;
    }
}

// W [n][c][t] (PyTorch, c inside the group) -> the forward's and the data gradient's operand.  VALU layers: wf [n][t][c], wb [c'][t][n']
// (c' the input channel of the whole layer, n' the output channel inside its group); matrix layers: wf [g][t][c][n'], wb [g][t][n'][c]
__global__ void __launch_bounds__(256) sd_pack_kernel(const float* W, float* wf, float* wb, int NC, int KG, int NG, int k, int mfma) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= (size_t)NC * KG * k) return;
    const int t = (int)(o % k), c = (int)((o / k) % KG), n = (int)(o / ((size_t)k * KG));
    const int g = n / NG, nl = n % NG;
    if (mfma) {
        wf[(((size_t)g * k + t) * KG + c) * NG + nl] = W[o];
        wb[(((size_t)g * k + t) * NG + nl) * KG + c] = W[o];
    } else {
        wf[((size_t)n * k + t) * KG + c] = W[o];
        wb[(((size_t)g * KG + c) * k + t) * NG + nl] = W[o];
    }
}

__global__ void __launch_bounds__(256) sd_copy_kernel(float* dst, const float* src, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

SdConv sd_conv(const gvx_hifigan_msd_dims& d, const SdLayer& l, const SdFeat& F, int s, int i, const int32_t* lens, int n_max) {
    SdConv p{};
    p.lens = lens; p.n_max = n_max; p.scale = s;
    p.KC = l.cin; p.NC = l.cout; p.KG = l.cin / l.groups; p.NG = l.cout / l.groups;
    p.k = l.k; p.stride = l.stride; p.pad = l.pad;
    p.Ls_max = i == 0 ? F.n_scale[s] : F.length[s][i - 1];
    p.Lo_max = F.length[s][i];
    p.n_src = i; p.n_out = i + 1;
    sd_strides(d, p.str);
    p.act = l.act; p.slope = d.slope;
    return p;
}

template <bool BWD, int MF, int WN>
void sd_launch_mfma(const SdConv& p, unsigned tiles, int phases, int B, size_t lds, hipStream_t s) {
    constexpr int NT = MF * WN, THREADS = 64 * (64 / MF) * WN;
    const int n_tiles = (p.NG + NT - 1) / NT, groups = p.NC / p.NG;
    sd_mfma_kernel<BWD, MF, WN><<<dim3(tiles, (unsigned)(n_tiles * groups * phases), (unsigned)B), THREADS, lds, s>>>(p);
}

// forward of layer (s, i), or with BWD its data gradient: there `q` already has the two sides exchanged
template <bool BWD>
int sd_launch_conv(const SdConv& q, int mfma, int B, hipStream_t s) {
    SdConv p = q;
    const int phases = BWD ? p.stride : 1;
    const int positions = BWD ? (p.Lo_max + p.stride - 1) / p.stride : p.Lo_max;
    const unsigned tiles = (unsigned)((positions + SD_TILE - 1) / SD_TILE);
    if (mfma) {
        const SdWin w = sd_window(p.KG, p.k, p.stride, BWD);
        p.cb = w.cb;
        if (mfma == 32 && p.NG % 64 == 0) sd_launch_mfma<BWD, 32, 2>(p, tiles, phases, B, w.bytes, s);
        else if (mfma == 32) sd_launch_mfma<BWD, 32, 1>(p, tiles, phases, B, w.bytes, s);
        else sd_launch_mfma<BWD, 16, 1>(p, tiles, phases, B, w.bytes, s);
    } else {
        const int n_tiles = (p.NC + SD_TILE_N - 1) / SD_TILE_N;
        const dim3 grid(tiles, (unsigned)(n_tiles * phases), (unsigned)B);
        if (p.KG >= 64 && p.KG % 4 == 0) sd_valu_kernel<64, BWD><<<grid, 256, 0, s>>>(p);   // a wave per output element
        else sd_valu_kernel<1, BWD><<<grid, 256, 0, s>>>(p);
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

bool sd_bad_shape(const gvx_hifigan_msd_dims* dims, int B, int n_max) {
    return sd_dims_problem(dims) || B < 1 || B > 65535 || n_max < 1 || n_max > GVX_HIFIGAN_MSD_MAX_SAMPLES;
}

int sd_check_call(const gvx_hifigan_msd* h, const float* wav, const void* features, int B, int n_max) {
    if (!h || !wav || !features) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (n_max < 1) return fail(GVX_ERR_INVALID_ARG, "n_max = %d: a row needs at least 1 sample", n_max);
    if (n_max > GVX_HIFIGAN_MSD_MAX_SAMPLES) return fail(GVX_ERR_UNSUPPORTED, "n_max = %d is beyond the limit of %d samples", n_max, GVX_HIFIGAN_MSD_MAX_SAMPLES);
    return GVX_OK;
}

// the next of a call's marks on the stream: (n_maps + 1) per scale, made on first use
int sd_mark(std::vector<hipEvent_t>& ev, size_t at, hipStream_t s) {
    while (ev.size() <= at) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
    }
    HIP_TRY(hipEventRecord(ev[at], s));
    return GVX_OK;
}

std::string sd_name(int s, int i, int nl) {
    return "discriminators." + std::to_string(s) + (i == nl - 1 ? std::string(".conv_post") : ".convs." + std::to_string(i));
}

// the waveforms of scales 1 .. into the workspace
int sd_pool_all(const gvx_hifigan_msd_dims& d, const SdFeat& F, const SdWs& wp, const float* wav, const int32_t* lens, int B, int n_max,
                void* workspace, hipStream_t s) {
    const float* in = wav;
    for (int sc = 1; sc < d.n_scales; ++sc) {
        float* out = gvx::ws_ptr<float>(workspace, wp.pooled[sc]);
        sd_pool_kernel<<<dim3((unsigned)((F.n_scale[sc] + 255) / 256), (unsigned)B), 256, 0, s>>>(in, out, lens, n_max, sc - 1, F.n_scale[sc - 1],
                                                                                               F.n_scale[sc]);
        HIP_TRY(hipGetLastError());
        in = out;
    }
    return GVX_OK;
}

}  // namespace

extern "C" {

size_t gvx_hifigan_msd_blob_floats(const gvx_hifigan_msd_dims* dims) {
    if (sd_dims_problem(dims)) return 0;
    SdLayer L[SD_MAX_MAPS];
    size_t per_scale = 0;
    sd_layers(*dims, L, &per_scale);
    return per_scale * dims->n_scales;
}

int gvx_hifigan_msd_layout(const gvx_hifigan_msd_dims* dims, int B, int n_max, gvx_hifigan_msd_entry* entries, int max_entries) {
    if (sd_bad_shape(dims, B, n_max)) return 0;
    const SdFeat F = sd_feat_layout(*dims, B, n_max);
    int n = 0;
    for (int s = 0; s < dims->n_scales; ++s)
        for (int i = 0; i < F.n_maps; ++i, ++n)
            if (entries && n < max_entries) {
                const int64_t C = F.channels[i], L = F.length[s][i];
                entries[n] = gvx_hifigan_msd_entry{(uint64_t)F.off[s][i], (int32_t)C, (int32_t)L, L * C, 1, C};
            }
    return n;
}

size_t gvx_hifigan_msd_features_bytes(const gvx_hifigan_msd_dims* dims, int B, int n_max) {
    if (sd_bad_shape(dims, B, n_max)) return 0;
    return sd_feat_layout(*dims, B, n_max).total;
}

size_t gvx_hifigan_msd_workspace_bytes(const gvx_hifigan_msd_dims* dims, int B, int n_max, int backward) {
    if (sd_bad_shape(dims, B, n_max)) return 0;
    return sd_ws_plan(*dims, B, n_max, backward != 0).total;
}

int gvx_hifigan_msd_pack_weights_device(const gvx_hifigan_msd_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = sd_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    SdLayer L[SD_MAX_MAPS];
    size_t per_scale = 0;
    const int nl = sd_layers(*dims, L, &per_scale);
    struct Job { int s, i; const float* w; const float* b; };
    std::vector<Job> jobs;
    int rc = GVX_OK;
    for (int s = 0; s < dims->n_scales; ++s)
        for (int i = 0; i < nl; ++i) {
            const std::string name = sd_name(s, i, nl);
            const gvx_weight_desc* w = gvx_mg::mg_find(table, n, name + ".weight", (size_t)L[i].cout * (L[i].cin / L[i].groups) * L[i].k, rc);
            if (!w) return rc;
            const gvx_weight_desc* bs = gvx_mg::mg_find(table, n, name + ".bias", (size_t)L[i].cout, rc);
            if (!bs) return rc;   // nothing was launched
            jobs.push_back({s, i, w->data, bs->data});
        }
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(device_blob, 0, per_scale * dims->n_scales * sizeof(float), st));   // the padding between the tensors
    for (const Job& jb : jobs) {
        const SdLayer& l = L[jb.i];
        float* base = device_blob + jb.s * per_scale;
        const int KG = l.cin / l.groups, NG = l.cout / l.groups;
        const size_t wn = (size_t)l.cout * KG * l.k;
        sd_pack_kernel<<<(unsigned)((wn + 255) / 256), 256, 0, st>>>(jb.w, base + l.wf_off, base + l.wb_off, l.cout, KG, NG, l.k, l.mfma);
        HIP_TRY(hipGetLastError());
        sd_copy_kernel<<<(unsigned)((l.cout + 255) / 256), 256, 0, st>>>(base + l.b_off, jb.b, (size_t)l.cout);
        HIP_TRY(hipGetLastError());
    }
    return GVX_OK;
}

int gvx_hifigan_msd_create(const gvx_hifigan_msd_dims* dims, gvx_hifigan_msd** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = sd_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_hifigan_msd* h = new gvx_hifigan_msd();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_hifigan_msd_destroy(gvx_hifigan_msd* h) {
    if (!h) return;
    for (hipEvent_t e : h->fwd_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->bwd_ev) (void)hipEventDestroy(e);
    delete h;
}

int gvx_hifigan_msd_timing_enable(gvx_hifigan_msd* h, int enable) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    h->timing = enable != 0;
    h->fwd_timed = h->bwd_timed = false;
    return GVX_OK;
}

int gvx_hifigan_msd_layer_times_ms(gvx_hifigan_msd* h, float* forward_ms, float* backward_ms, int* n_layers_out) {
    if (!h || !forward_ms || !backward_ms || !n_layers_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    SdLayer L[SD_MAX_MAPS];
    const int nl = sd_layers(h->d, L);
    *n_layers_out = nl;
    for (int i = 0; i < nl; ++i) forward_ms[i] = backward_ms[i] = 0.f;
    for (int s = 0; s < h->d.n_scales; ++s)
        for (int i = 0; i < nl; ++i) {
            const size_t at = (size_t)s * (nl + 1) + i;
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

int gvx_hifigan_msd_bind(gvx_hifigan_msd* h, const float* device_blob) {
    if (!h || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if ((uintptr_t)device_blob % 256) return fail(GVX_ERR_INVALID_ARG, "the blob must be 256-byte aligned");
    h->blob = device_blob;
    return GVX_OK;
}

int gvx_hifigan_msd_forward(gvx_hifigan_msd* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features,
                            size_t features_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = sd_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    const gvx_hifigan_msd_dims& d = h->d;
    const SdFeat F = sd_feat_layout(d, B, n_max);
    if ((uintptr_t)features % 256 || features_bytes < F.total)
        return fail(GVX_ERR_WORKSPACE, "the features buffer is misaligned or smaller than %zu bytes", F.total);
    const SdWs wp = sd_ws_plan(d, B, n_max, false);
    if (!workspace || (uintptr_t)workspace % 256 || workspace_bytes < wp.total)
        return fail(GVX_ERR_WORKSPACE, "the workspace is missing, misaligned or smaller than %zu bytes", wp.total);
    hipStream_t s = (hipStream_t)stream;
    SdLayer L[SD_MAX_MAPS];
    size_t per_scale = 0;
    const int nl = sd_layers(d, L, &per_scale);
    if ((rc = sd_pool_all(d, F, wp, wav, sample_lengths, B, n_max, workspace, s)) != GVX_OK) return rc;
    for (int sc = 0; sc < d.n_scales; ++sc) {
        const float* in = sc == 0 ? wav : gvx::ws_ptr<float>(workspace, wp.pooled[sc]);
        if (h->timing && (rc = sd_mark(h->fwd_ev, (size_t)sc * (nl + 1), s)) != GVX_OK) return rc;
        for (int i = 0; i < nl; ++i) {
            SdConv p = sd_conv(d, L[i], F, sc, i, sample_lengths, n_max);
            p.src = in; p.W = h->blob + sc * per_scale + L[i].wf_off; p.bias = h->blob + sc * per_scale + L[i].b_off;
            p.out = gvx::ws_ptr<float>(features, F.off[sc][i]);
            if ((rc = sd_launch_conv<false>(p, L[i].mfma, B, s)) != GVX_OK) return rc;
            in = p.out;
            if (h->timing && (rc = sd_mark(h->fwd_ev, (size_t)sc * (nl + 1) + i + 1, s)) != GVX_OK) return rc;
        }
    }
    h->fwd_timed = h->timing;
    return GVX_OK;
}

int gvx_hifigan_msd_backward(gvx_hifigan_msd* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, const void* features,
                             const void* d_features, const gvx_grad_desc* grads, int n_grads, float* d_wav,
                             void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = sd_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    if (!d_features) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_grads < 0 || (n_grads > 0 && !grads)) return fail(GVX_ERR_INVALID_ARG, "n_grads = %d without a table", n_grads);
    if (n_grads == 0 && !d_wav) return fail(GVX_ERR_INVALID_ARG, "neither parameter gradients nor d_wav are asked for");
    const gvx_hifigan_msd_dims& d = h->d;
    const SdFeat F = sd_feat_layout(d, B, n_max);
    if ((uintptr_t)features % 256 || (uintptr_t)d_features % 256) return fail(GVX_ERR_WORKSPACE, "features or d_features is not 256-byte aligned");
    const SdWs wp = sd_ws_plan(d, B, n_max, true);
    if (!workspace || (uintptr_t)workspace % 256 || workspace_bytes < wp.total)
        return fail(GVX_ERR_WORKSPACE, "the workspace is missing, misaligned or smaller than %zu bytes", wp.total);
    SdLayer L[SD_MAX_MAPS];
    size_t per_scale = 0;
    const int nl = sd_layers(d, L, &per_scale);
    float* gw[GVX_HIFIGAN_MSD_MAX_SCALES][SD_MAX_MAPS] = {};
    float* gb[GVX_HIFIGAN_MSD_MAX_SCALES][SD_MAX_MAPS] = {};
    if (n_grads > 0) {
        const gvx_weight_desc* table = reinterpret_cast<const gvx_weight_desc*>(grads);   // same fields, the data pointer writable
        static_assert(sizeof(gvx_weight_desc) == sizeof(gvx_grad_desc), "the two tables share a layout");
        for (int sc = 0; sc < d.n_scales; ++sc)
            for (int i = 0; i < nl; ++i) {
                const std::string name = sd_name(sc, i, nl);
                rc = GVX_OK;
                const gvx_weight_desc* w = gvx_mg::mg_find(table, n_grads, name + ".weight", (size_t)L[i].cout * (L[i].cin / L[i].groups) * L[i].k, rc);
                if (!w) return rc;
                gw[sc][i] = const_cast<float*>(w->data);
                w = gvx_mg::mg_find(table, n_grads, name + ".bias", (size_t)L[i].cout, rc);
                if (!w) return rc;
                gb[sc][i] = const_cast<float*>(w->data);
            }
    }
    hipStream_t s = (hipStream_t)stream;
    float* gbuf[2] = {gvx::ws_ptr<float>(workspace, wp.grad[0]), gvx::ws_ptr<float>(workspace, wp.grad[1])};
    float* parts = gvx::ws_ptr<float>(workspace, wp.parts);
    double* db_parts = gvx::ws_ptr<double>(workspace, wp.db_parts);
    auto feat = [&](const void* base, int sc, int i) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + F.off[sc][i]); };
    // the first layers' weight gradients read the pooled waveforms
    if (n_grads > 0 && (rc = sd_pool_all(d, F, wp, wav, sample_lengths, B, n_max, workspace, s)) != GVX_OK) return rc;
    for (int sc = d.n_scales - 1; sc >= 0; --sc) {   // the last scale first: its waveform gradient is pooled back into the one before it
        const float* blob = h->blob + sc * per_scale;
        const float* wav_s = sc == 0 ? wav : gvx::ws_ptr<float>(workspace, wp.pooled[sc]);
        const float* dcur = feat(d_features, sc, nl - 1);   // the score has no activation: its cotangent is its pre-activation's
        if (h->timing && (rc = sd_mark(h->bwd_ev, (size_t)sc * (nl + 1) + nl, s)) != GVX_OK) return rc;
        for (int i = nl - 1; i >= 0; --i) {
            SdConv p = sd_conv(d, L[i], F, sc, i, sample_lengths, n_max);
            if (n_grads > 0) {
                p.src = i == 0 ? wav_s : feat(features, sc, i - 1);
                p.dy = dcur;
                const SdPieces P = sd_pieces(L[i], B, p.Lo_max);
                if (L[i].mfma) {
                    const int MF = L[i].mfma;
                    const dim3 grid((unsigned)(L[i].groups * (p.NG / MF) * ((p.KG + MF - 1) / MF)), (unsigned)((p.k + 3) / 4), (unsigned)P.n);
                    if (MF == 32) sd_wgrad_mfma_kernel<32><<<grid, 256, 0, s>>>(p, parts, B, P.chunks, P.rows_per_piece, P.run);
                    else sd_wgrad_mfma_kernel<16><<<grid, 256, 0, s>>>(p, parts, B, P.chunks, P.rows_per_piece, P.run);
                } else {
                    sd_wgrad_valu_kernel<<<dim3((unsigned)((P.numel + 255) / 256), (unsigned)P.n), 256, 0, s>>>(p, parts, B, P.chunks, P.rows_per_piece, P.run);
                }
                HIP_TRY(hipGetLastError());
                sd_reduce_kernel<<<(unsigned)((P.numel + 31) / 32), 256, 0, s>>>(parts, gw[sc][i], P.numel, P.n);
                HIP_TRY(hipGetLastError());
                sd_db_kernel<<<dim3((unsigned)((p.NC + 31) / 32), SD_DB_SLICES), 256, 0, s>>>(p, db_parts, B);
                HIP_TRY(hipGetLastError());
                sd_db_reduce_kernel<<<(unsigned)((p.NC + 255) / 256), 256, 0, s>>>(db_parts, gb[sc][i], p.NC);
                HIP_TRY(hipGetLastError());
            }
            if (i > 0) {
                // the data gradient is a convolution with the sides exchanged: dY is the operand, the layer's input map the output
                SdConv q = p;
                q.src = dcur; q.W = blob + L[i].wb_off; q.bias = nullptr; q.dy = nullptr;
                q.KC = p.NC; q.NC = p.KC; q.KG = p.NG; q.NG = p.KG;
                q.Ls_max = p.Lo_max; q.Lo_max = p.Ls_max; q.n_src = p.n_out; q.n_out = p.n_src;
                q.mask = feat(features, sc, i - 1);
                q.dfeat = feat(d_features, sc, i - 1);
                q.out = gbuf[i & 1];
                if ((rc = sd_launch_conv<true>(q, L[i].mfma, B, s)) != GVX_OK) return rc;
                dcur = q.out;
            } else if (d_wav) {
                p.dy = dcur; p.W = blob + L[0].wf_off;
                const bool more = sc + 1 < d.n_scales;
                const float* next = more ? gvx::ws_ptr<float>(workspace, wp.dpool[sc + 1]) : nullptr;
                float* out = sc == 0 ? d_wav : gvx::ws_ptr<float>(workspace, wp.dpool[sc]);
                sd_dwav_kernel<<<dim3((unsigned)((p.Ls_max + 4 * SD_DWAV_RUN - 1) / (4 * SD_DWAV_RUN)), (unsigned)B), 256, 0, s>>>(
                    p, next, more ? F.n_scale[sc + 1] : 0, out);
                HIP_TRY(hipGetLastError());
            }
            if (h->timing && (rc = sd_mark(h->bwd_ev, (size_t)sc * (nl + 1) + i, s)) != GVX_OK) return rc;   // mark i: layer i is done
        }
    }
    h->bwd_timed = h->timing;
    return GVX_OK;
}

}  // C ABI
