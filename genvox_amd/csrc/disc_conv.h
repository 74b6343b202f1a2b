// The convolution core of the HiFi-GAN discriminators: what csrc/hifigan_disc.hip (period discriminators) and csrc/hifigan_msd.hip
// (scale discriminators) have in common.  Maps are channels-last; a row is a grid of [height][period] cells (GRID) or a plain run of
// positions (a grid of period 1, spelt without its divisions), and a convolution runs along the height.  The first part is host
// arithmetic that a stand-alone program can include without a device: the launch parameters, the row and length rules that host and
// kernels share, the pieces of a weight gradient and the backward's scratch.  The second part (hipcc only) holds the device helpers
// and the kernels that are the same in both: the VALU convolution, the VALU weight gradient, the piece reduction, the bias gradient
// and the copy.  A discriminator keeps its own matrix-instruction kernels, its planner of pieces and its waveform gradient.
#pragma once
#include <cstddef>
#include <cstdint>
#include "rounding.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DC_HD __host__ __device__
#else
#define DC_HD
#endif

namespace gvx_dc {

constexpr int DC_TILE = 64;        // positions per workgroup, every convolution kernel; a data gradient's are those of ONE stride phase
constexpr int DC_TILE_N = 64;      // output channels per workgroup of the VALU kernels
constexpr int DC_DB_SLICES = 64;   // slices of the bias-gradient sum, added in their order
constexpr int DC_MAX_MAPS = 9;     // the convolutions of one stack and its score
constexpr int DC_PART_FLOATS = 1 << 24;   // the weight-gradient partials of one layer stay below this many floats where the rows allow it

struct DcConv {
    const float* src;     // the operand: forward [B][Ls_max][period][KC] (wav_src: the waveform [B][n_max]); data gradient dY
    const float* W;       // VALU: [NC][taps][KG]; the matrix kernels: as their discriminator packs them
    const float* bias;    // forward
    float* out;           // [B][Lo_max][period][NC]
    const float* dfeat;   // data gradient: cotangent of the map that `out` is the gradient of (added before its mask)
    const float* mask;    // data gradient: that map itself, for its sign
    const float* dy;      // weight gradient: [B][Lo_max][period][NC] against src [B][Ls_max][period][KC]
    const int32_t* lens;
    int n_max, min_n, scale;   // the samples of a row: dc_samples
    int period;           // columns of the grid (1: no grid)
    int KC, NC, KG, NG;   // channels of the operand and of the output, in all and per group (a grid has one group)
    int k, stride, pad;
    int Ls_max, Lo_max;   // heights of the operand's and the output's buffers
    int n_src, n_out;     // how many of str[] lie in front of the operand's / the output's height
    int str[DC_MAX_MAPS];
    int act, wav_src;     // wav_src: a grid's first layer reads the waveform through the reshape and the reflection
    int cb;               // the scale discriminators' matrix kernels: their channel block
    float slope;
};

// samples of a row of n: fewer than min_n, or none, are 0 (a row the caller should have refused is silent, never a bad address); then
// `scale` poolings
DC_HD inline int dc_samples(int n, int min_n, int scale) {
    if (n < min_n || n <= 0) return 0;
    for (int i = 0; i < scale; ++i) n = n / 2 + 1;
    return n;
}

// height of a row of n samples on the period-p grid after the layers whose strides are str[0 .. count) (0 stays 0)
DC_HD inline int dc_length(int n, int period, const int* str, int count) {
    if (n <= 0) return 0;
    n = (n + period - 1) / period;
    for (int i = 0; i < count; ++i) n = (n - 1) / str[i] + 1;
    return n;
}


// pieces of one layer's weight gradient: rows are dealt `rows_per_piece` to a piece, or a row is cut into `chunks` runs of positions
struct DcPieces { int chunks, rows_per_piece, n, run; size_t numel; };

// the backward's scratch that every discriminator has, as byte offsets: two activation gradients of the largest map (the layers
// alternate), the partial weight gradients and the float64 partial bias gradients
struct DcWs { size_t grad[2], parts, db_parts; };

struct DcWsNeed {   // folded over every layer of every stack, then placed
    size_t act = 0, parts = 0, cmax = 1;
    void layer(int B, int cout, int positions, bool is_score, const DcPieces& P) {
        const size_t a = (size_t)B * cout * positions;
        if (!is_score && a > act) act = a;
        if (P.n * P.numel > parts) parts = P.n * P.numel;
        if ((size_t)cout > cmax) cmax = cout;
    }
    template <class Take>
    DcWs place(Take&& take) const {
        DcWs W{};
        W.grad[0] = take(act * sizeof(float));
        W.grad[1] = take(act * sizeof(float));
        W.parts = take(parts * sizeof(float));
        W.db_parts = take(DC_DB_SLICES * cmax * sizeof(double));
        return W;
    }
};

#if defined(__HIPCC__)

// the samples of row b.  WAVE_ROW: the caller states that every lane of its wave asks for the same row, and the count and the heights
// derived from it live in scalar registers (the period discriminators' matrix convolution has no vector registers to spare for them)
template <bool WAVE_ROW = false>
__device__ __forceinline__ int dc_row_n(const DcConv& p, int b) {
    int n = p.lens ? p.lens[b] : p.n_max;
    if constexpr (WAVE_ROW) n = __builtin_amdgcn_readfirstlane(n);
    n = n > p.n_max ? p.n_max : n;
    return dc_samples(n, p.min_n, p.scale);
}

// ---- geometry.  Position m of a row is the cell (u, col) = (m / period, m % period) of a grid, or m itself
template <bool GRID>
__device__ __forceinline__ int dc_len(const DcConv& p, int n, int count) { return dc_length(n, GRID ? p.period : 1, p.str, count); }
// the heights of a row's operand and output: they lie one layer apart, so one walk through the strides gives both (a division per
// stride: the workgroups of a score or a first layer do little more than this prologue)
struct DcHeights { int src, out; };
template <bool GRID>
__device__ __forceinline__ DcHeights dc_heights(const DcConv& p, int n) {
    const int near = min(p.n_src, p.n_out), h = dc_len<GRID>(p, n, near);
    const int far = h > 0 ? (h - 1) / p.str[near] + 1 : 0;
    return p.n_src < p.n_out ? DcHeights{h, far} : DcHeights{far, h};
}
template <bool GRID>
__device__ __forceinline__ int dc_u(const DcConv& p, int m) { if constexpr (GRID) return m / p.period; else return m; }
template <bool GRID>
__device__ __forceinline__ int dc_col(const DcConv& p, int m) { if constexpr (GRID) return m % p.period; else return 0; }
// the index of cell (h, col) in cells; with h = b * H_max + height, that of a whole buffer
template <bool GRID>
__device__ __forceinline__ size_t dc_cell(const DcConv& p, size_t h, int col) { if constexpr (GRID) return h * p.period + col; else return h; }

// how the taps of one workgroup walk the operand's heights: tap j (weight tap t0 + j * tstep) of position u reads height
// u * mul + base + j * hstep.  A data gradient's workgroup belongs to ONE stride phase ph: its output heights are u * stride + ph, and
// only the taps t = (ph + pad) mod stride, + stride, ... meet a dY height - the gather by stride phase
struct DcTaps { int n, t0, tstep, mul, base, hstep; };

template <bool BWD>
__device__ __forceinline__ DcTaps dc_taps(const DcConv& p, int ph) {
    if constexpr (!BWD) return DcTaps{p.k, 0, 1, p.stride, -p.pad, 1};
    const int t0 = (ph + p.pad) % p.stride;
    return DcTaps{t0 < p.k ? (p.k - 1 - t0) / p.stride + 1 : 0, t0, p.stride, 1, (ph + p.pad - t0) / p.stride, -1};
}

// a tile behind its row: exact zeros inside the buffer, channels [n0, n0 + cols)
template <bool GRID, bool BWD>
__device__ __forceinline__ void dc_zero_tile(const DcConv& p, int b, int m0, int ph, int n0, int cols) {
    for (int idx = threadIdx.x; idx < DC_TILE * cols; idx += blockDim.x) {
        const int m = m0 + idx / cols, u = dc_u<GRID>(p, m);
        const int h = BWD ? u * p.stride + ph : u;
        if (h < p.Lo_max) p.out[dc_cell<GRID>(p, (size_t)b * p.Lo_max + h, dc_col<GRID>(p, m)) * p.NC + n0 + idx % cols] = 0.f;
    }
}

// the epilogue of one output element: bias + LeakyReLU, or cotangent + mask, and the zeros behind the row
template <bool GRID, bool BWD>
__device__ __forceinline__ void dc_finish(const DcConv& p, int b, int h, int col, int n, int Lo, float v) {
    if (h >= p.Lo_max) return;
    const size_t at = dc_cell<GRID>(p, (size_t)b * p.Lo_max + h, col) * p.NC + n;
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

// forward (BWD = false) and data gradient (BWD = true) in fp32 VALU code: G lanes per output element (position, channel), channel
// fastest; the G partial sums are added by a fixed butterfly.  The first layer, the score (G = 64: the input channels dealt over a wave)
// and narrow layers
template <bool GRID, int G, bool BWD>
__global__ void __launch_bounds__(256) dc_valu_kernel(const DcConv p) {
    constexpr bool WAV = GRID && G == 1 && !BWD;   // the only form that a waveform operand is launched in
    const int b = blockIdx.z;
    const int n_tiles = (p.NC + DC_TILE_N - 1) / DC_TILE_N;
    const int n0 = ((int)blockIdx.y % n_tiles) * DC_TILE_N, ph = (int)blockIdx.y / n_tiles;
    const int cols = min(DC_TILE_N, p.NC - n0);
    const int m0 = (int)blockIdx.x * DC_TILE;
    const int nb = dc_row_n(p, b);
    const DcHeights hb = dc_heights<GRID>(p, nb);
    const int Ls = hb.src, Lo = hb.out;
    const int first = BWD ? dc_u<GRID>(p, m0) * p.stride + ph : dc_u<GRID>(p, m0);
    if (first >= Lo) {
        dc_zero_tile<GRID, BWD>(p, b, m0, ph, n0, cols);
        return;
    }
    const DcTaps tp = dc_taps<BWD>(p, ph);
    const int K = p.k * p.KG;
    const float* src_b = (WAV && p.wav_src) ? p.src + (size_t)b * p.n_max : p.src + dc_cell<GRID>(p, (size_t)b * p.Ls_max, 0) * p.KC;
    const int total = DC_TILE * cols * G;   // G = 64: a multiple of 256, so the lanes of a wave stay together for the butterfly
    for (int idx = threadIdx.x; idx < total; idx += 256) {
        const int g = idx % G, el = idx / G, n = n0 + el % cols, m = m0 + el / cols;
        const int u = dc_u<GRID>(p, m), col = dc_col<GRID>(p, m), h = BWD ? u * p.stride + ph : u;
        float sum = 0.f;
        if (h < Lo) {
            const float* w = p.W + (size_t)n * K;
            const int xg = GRID ? 0 : (n / p.NG) * p.KG;   // the group's first operand channel
            for (int j = 0; j < tp.n; ++j) {
                const int hs = u * tp.mul + tp.base + j * tp.hstep;
                if (hs < 0 || hs >= Ls) continue;
                const float* wt = w + (size_t)(tp.t0 + j * tp.tstep) * p.KG;
                float run = 0.f;
                if (WAV && p.wav_src) {   // the reshape and the reflection: cell (hs, col) is sample hs * period + col, mirrored behind the row
                    int i = hs * p.period + col;
                    i = i >= nb ? 2 * (nb - 1) - i : i;
                    if (g == 0 && i >= 0) run = src_b[i] * wt[0];
                } else {
                    const float* x = src_b + dc_cell<GRID>(p, (size_t)hs, col) * p.KC + xg;
                    if constexpr (G > 1) {   // KG is a multiple of 4 here (the launchers see to it): a lane takes whole float4s
                        for (int c = 4 * g; c < p.KG; c += 4 * G) {
                            const float4 xv = *reinterpret_cast<const float4*>(x + c), wv = *reinterpret_cast<const float4*>(wt + c);
                            run = fmaf(xv.w, wv.w, fmaf(xv.z, wv.z, fmaf(xv.y, wv.y, fmaf(xv.x, wv.x, run))));
                        }
                    } else {
                        for (int c = 0; c < p.KG; ++c) run = fmaf(x[c], wt[c], run);
                    }
                }
                sum += run;
            }
        }
#pragma unroll
        for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (g == 0) dc_finish<GRID, BWD>(p, b, h, col, n, Lo, sum);
    }
}

// the VALU kernel of a layer: a wave per output element where the operand's group channels fill its float4s
template <bool GRID, bool BWD>
inline void dc_launch_valu(const DcConv& p, unsigned tiles, int phases, int B, hipStream_t s) {
    const int n_tiles = (p.NC + DC_TILE_N - 1) / DC_TILE_N;
    const dim3 grid(tiles, (unsigned)(n_tiles * phases), (unsigned)B);
    if (p.KG >= 64 && p.KG % 4 == 0 && !p.wav_src) dc_valu_kernel<GRID, 64, BWD><<<grid, 256, 0, s>>>(p);
    else dc_valu_kernel<GRID, 1, BWD><<<grid, 256, 0, s>>>(p);
}

// the rows [b0, b1) and the run `chunk` of their positions that a weight-gradient piece sums: rows dealt to pieces, or a row cut into runs
struct DcSpan { int b0, b1, chunk; };
__device__ __forceinline__ DcSpan dc_span(int piece, int B, int chunks, int rows_per_piece) {
    if (chunks > 1) return DcSpan{piece / chunks, piece / chunks + 1, piece % chunks};
    const int b0 = piece * rows_per_piece;
    return DcSpan{b0, b0 + rows_per_piece < B ? b0 + rows_per_piece : B, 0};
}

// one piece of a weight gradient in VALU code: dW[n][c][t] = the sum over positions of dY[pos][n] X[source height of (pos, t)][c], a
// thread per element.  TAP_MAJOR numbers the threads, and lays the piece out, as [tap][n][c] with c fastest (the period discriminators:
// their matrix kernel writes that layout); otherwise in PyTorch's order [n][c][tap].  The bits are the same, the coalescing is not.
template <bool GRID, bool TAP_MAJOR>
__global__ void __launch_bounds__(256) dc_wgrad_valu_kernel(const DcConv p, float* parts, int B, int chunks, int rows_per_piece, int run) {
    const size_t numel = (size_t)p.NC * p.KG * p.k;
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= numel) return;
    int t, c_l, n;
    if constexpr (TAP_MAJOR) {
        c_l = (int)(o % p.KG), n = (int)((o / p.KG) % p.NC), t = (int)(o / ((size_t)p.KG * p.NC));
    } else {
        t = (int)(o % p.k), c_l = (int)((o / p.k) % p.KG), n = (int)(o / ((size_t)p.k * p.KG));
    }
    const int c = GRID ? c_l : (n / p.NG) * p.KG + c_l;
    const bool wav = GRID && p.wav_src;
    const int piece = blockIdx.y;
    const DcSpan sp = dc_span(piece, B, chunks, rows_per_piece);
    float acc = 0.f;
    for (int b = sp.b0; b < sp.b1; ++b) {
        const int nb = dc_row_n(p, b);
        const DcHeights hb = dc_heights<GRID>(p, nb);
        const int Ls = hb.src, Lo = hb.out;
        const int la = sp.chunk * run, lb = min(la + run, Lo * (GRID ? p.period : 1));
        const float* dy_b = p.dy + dc_cell<GRID>(p, (size_t)b * p.Lo_max, 0) * p.NC + n;
        const float* x_b = wav ? p.src + (size_t)b * p.n_max : p.src + dc_cell<GRID>(p, (size_t)b * p.Ls_max, 0) * p.KC + c;
        float part = 0.f;
        for (int m = la; m < lb; ++m) {
            const int col = dc_col<GRID>(p, m), hs = dc_u<GRID>(p, m) * p.stride + t - p.pad;
            if (hs < 0 || hs >= Ls) continue;
            float xv;
            if (wav) {
                int i = hs * p.period + col;
                i = i >= nb ? 2 * (nb - 1) - i : i;
                xv = i >= 0 ? x_b[i] : 0.f;
            } else {
                xv = x_b[dc_cell<GRID>(p, (size_t)hs, col) * p.KC];
            }
            part = fmaf(dy_b[(size_t)m * p.NC], xv, part);
        }
        acc += part;
    }
    parts[(size_t)piece * numel + o] = acc;
}

// parts [pieces][numel] (TAP_MAJOR: every piece [tap][n][c]) -> out [n][c][tap], PyTorch's layout: eight lanes per output take every
// eighth piece in order, and the eight sums are added by a fixed butterfly - the same order in every call
template <bool TAP_MAJOR>
__global__ void __launch_bounds__(256) dc_reduce_kernel(const float* parts, float* out, int NC, int KG, int k, int pieces) {
    const size_t numel = (size_t)NC * KG * k;
    const size_t o = ((size_t)blockIdx.x * 256 + threadIdx.x) / 8;
    const int ln = threadIdx.x & 7;
    float v = 0.f;
    if (o < numel) {
        size_t at = o;
        if constexpr (TAP_MAJOR) {
            const int t = (int)(o % k), c = (int)((o / k) % KG), n = (int)(o / ((size_t)k * KG));
            at = ((size_t)t * NC + n) * KG + c;
        }
        for (int i = ln; i < pieces; i += 8) v += parts[(size_t)i * numel + at];
    }
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    if (ln == 0 && o < numel) out[o] = v;
}

// db[n] = sum over rows and positions of dy, in float64 (a bias gradient is a plain sum of cotangents that may cancel): a workgroup
// takes 32 channels and one slice of the flat positions [B][Lo_max][period]; eight lanes per channel stride the slice
template <bool GRID>
__global__ void __launch_bounds__(256) dc_db_kernel(const DcConv p, double* db_parts, int B) {
    __shared__ double red[8][32];
    const int ch = threadIdx.x & 31, ln = threadIdx.x >> 5;
    const int n = (int)blockIdx.x * 32 + ch, slice = blockIdx.y;
    const long per_row = (long)p.Lo_max * (GRID ? p.period : 1), total = per_row * B;
    const long per = (total + DC_DB_SLICES - 1) / DC_DB_SLICES, lo = slice * per, hi = lo + per < total ? lo + per : total;
    double v = 0.0;
    int b_cur = -1, Lo = 0;
    for (long m = lo + ln; m < hi; m += 8) {
        const int b = (int)(m / per_row);
        if (b != b_cur) { b_cur = b; Lo = dc_len<GRID>(p, dc_row_n(p, b), p.n_out); }
        if (dc_u<GRID>(p, (int)(m % per_row)) < Lo && n < p.NC) v += (double)p.dy[(size_t)m * p.NC + n];
    }
    red[ln][ch] = v;
    __syncthreads();
    if (ln == 0 && n < p.NC) {
        double sum = red[0][ch];
        for (int i = 1; i < 8; ++i) sum += red[i][ch];
        db_parts[(size_t)slice * p.NC + n] = sum;
    }
}

static __global__ void __launch_bounds__(256) dc_db_reduce_kernel(const double* db_parts, float* out, int NC) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= NC) return;
    double v = 0.0;
    for (int i = 0; i < DC_DB_SLICES; ++i) v += db_parts[(size_t)i * NC + n];
    out[n] = (float)v;
}

static __global__ void __launch_bounds__(256) dc_copy_kernel(float* dst, const float* src, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

#endif   // __HIPCC__

}  // namespace gvx_dc
