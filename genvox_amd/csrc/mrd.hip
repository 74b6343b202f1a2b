// Multi-resolution spectrogram discriminator (include/genvox_amd.h, "Multi-resolution spectrogram discriminator"): forward, and the
// backward that reads the forward's own maps as its tape.  Maps are channels-last, [B][frames][bins][channels]; a position is a cell
// (frame w, bin f), numbered w * F + f.  A convolution mixes nine (three) frames and three bins: in this storage the three bins of one
// time tap are one contiguous run of 3 C floats, so a layer is an implicit GEMM with K = 3 C per time tap, and the zero padding in
// frequency is a test on the 32-channel block's bin.
//   mr_spec_kernel        a wave per frame: gather through the reflection, window, real transform in LDS (fft_lds.h), magnitude
//   mr_spec_grad_kernel   the same transform again, d_mag (re, im) / mag, the adjoint of the real transform, the window
//   mr_dwav_kernel        overlap-add as a gather, through the reflection, accumulated over the resolutions in their order
//   mr_mfma_kernel        the C -> C layers, forward (BWD = false) and data gradient (BWD = true, one stride phase per workgroup)
//   mr_narrow_in_kernel   one operand channel: the first layer's forward, the score's data gradient (VALU)
//   mr_narrow_out_kernel  one output channel: the score's forward, the first layer's data gradient (VALU, a wave per position)
//   mr_wgrad_mfma_kernel, mr_wgrad_valu_kernel   one piece of a weight gradient, laid out [tap][c_out][c_in]
// The handle, the marks, the name lookup, the argument checks, the piece reduction and the bias reduction are the shared host side's
// (disc_host.h).  No atomics anywhere: two calls give the same bits.
#include "disc_host.h"
#include "fft_lds.h"
#include "mrd_internal.h"

using gvx::fail;
using namespace gvx_mr;

static_assert(MR_TILE == GVX_MRD_TILE && MR_TILE_NARROW == GVX_MRD_TILE_NARROW && MR_PIECE_FRAMES == GVX_MRD_PIECE_FRAMES &&
                  MR_FRAMES_PER_WG == GVX_MRD_FRAMES_PER_WORKGROUP && MR_MAPS == GVX_MRD_MAPS,
              "the public header states the tile constants");
static_assert(GVX_MRD_MAX_RESOLUTIONS <= DC_MAX_STACKS && MR_MAPS <= DC_MAX_MAPS, "a resolution is a stack of the shared host side");

struct gvx_mrd : DcHandle {
    gvx_mrd_dims d;
};

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int MR_LD = 36;   // floats per LDS row of a 32-deep k-tile: the fragment reads of sixteen lanes fall on distinct 16-byte slots

struct MrConv {
    const float* src;     // the operand [B][Ls_max][F][KC]; data gradient: dY
    const float* W;       // [NC][kt][3][KC]
    const float* bias;    // forward
    float* out;           // [B][Lo_max][F][NC]
    const float* dfeat;   // data gradient: cotangent of the map that `out` is the gradient of (added before its mask), or null
    const float* mask;    // data gradient: that map itself, for its sign, or null (the spectrogram has no activation)
    const float* dy;      // weight gradient: [B][Lo_max][F][NC] against src
    const int32_t* lens;
    int n_max, min_n, n_fft, hop;
    int F, KC, NC, kt, stride, padt;
    int Ls_max, Lo_max;   // frames of the operand's and the output's buffers
    int n_src, n_out;     // how many layers lie in front of the operand's / the output's frames (mr_width)
    int act;
    float slope;
};

struct MrSpec {
    const float* win; const float2* tw; const float2* tw2;
    const int32_t* lens;
    int n_max, min_n, hop, W_max;
};

// the samples of row b: a row the caller should have refused is silent.  WAVE_ROW: every lane of the wave asks for the same row
template <bool WAVE_ROW = false>
__device__ __forceinline__ int mr_row_n(const int32_t* lens, int n_max, int min_n, int b) {
    int n = lens ? lens[b] : n_max;
    if constexpr (WAVE_ROW) n = __builtin_amdgcn_readfirstlane(n);
    n = n > n_max ? n_max : n;
    return n < min_n ? 0 : n;
}

__device__ __forceinline__ int mr_reflect(int i, int nb) {
    i = i < 0 ? -i : i;
    return i >= nb ? 2 * (nb - 1) - i : i;
}

// ---- the spectrogram and its adjoint

// frame t of row b, windowed, as H complex points in buf; then its complex transform
template <int H>
__device__ __forceinline__ void mr_frame_fft(const float* __restrict__ x, const MrSpec& p, int nb, int t, float2* buf, int j) {
    const int i0 = t * p.hop - (2 * H - p.hop) / 2;
#pragma unroll
    for (int q = 0; q < H / 64; ++q) {
        const int m = j + 64 * q;
        const float2 w = *reinterpret_cast<const float2*>(p.win + 2 * m);
        buf[fpad(m)] = make_float2(w.x * x[mr_reflect(i0 + 2 * m, nb)], w.y * x[mr_reflect(i0 + 2 * m + 1, nb)]);
    }
    wave_lds_fence();
    fft_lds_wave<H, false>(buf, p.tw, j);
}

template <int H>
__global__ __launch_bounds__(MR_FRAMES_PER_WG * 64) void mr_spec_kernel(const float* __restrict__ wav, const MrSpec p, float* __restrict__ mag) {
    constexpr int Q = H / 64, BINS = H + 1;
    __shared__ __attribute__((aligned(16))) float2 fsm[MR_FRAMES_PER_WG * fft_lds_words<H>()];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t = (int)blockIdx.x * MR_FRAMES_PER_WG + wave;
    const int nb = mr_row_n<true>(p.lens, p.n_max, p.min_n, b);
    if (t >= mr_frames(nb, 2 * H, p.hop)) return;   // nothing behind the row's frames is read by a layer
    float2* buf = fsm + wave * fft_lds_words<H>();
    mr_frame_fft<H>(wav + (size_t)b * p.n_max, p, nb, t, buf, j);
    float* out = mag + ((size_t)b * p.W_max + t) * BINS;
#pragma unroll
    for (int q = 0; q <= Q; ++q) {
        const int k = j + 64 * q;
        if (k <= H) {
            const float2 X = rfft_split(buf[fpad(k & (H - 1))], buf[fpad((H - k) & (H - 1))], p.tw2[k], k == 0 || k == H);
            out[k] = sqrtf(X.x * X.x + X.y * X.y);
        }
    }
}

// dL/dX = d_mag X / mag (0 where mag == 0), then as the STFT loss's gradient: the forward is X_k = sum_n x_n w_N^{kn} on bins 0 .. H,
// so dL/dx_n is the unnormalised complex-to-real inverse of Y with Y_0 = Re G_0, Y_H = Re G_H and Y_k = G_k / 2 between them; a lane
// makes the inverse's points k and H - k from the same two bins, which are also the only two points of the forward it reads
template <int H>
__global__ __launch_bounds__(MR_FRAMES_PER_WG * 64) void mr_spec_grad_kernel(const float* __restrict__ wav, const MrSpec p,
                                                                             const float* __restrict__ dmag, float* __restrict__ g) {
    constexpr int Q = H / 64, BINS = H + 1, N = 2 * H;
    __shared__ __attribute__((aligned(16))) float2 fsm[MR_FRAMES_PER_WG * fft_lds_words<H>()];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t = (int)blockIdx.x * MR_FRAMES_PER_WG + wave;
    const int nb = mr_row_n<true>(p.lens, p.n_max, p.min_n, b);
    if (t >= mr_frames(nb, N, p.hop)) return;
    float2* buf = fsm + wave * fft_lds_words<H>();
    mr_frame_fft<H>(wav + (size_t)b * p.n_max, p, nb, t, buf, j);
    const float* dm = dmag + ((size_t)b * p.W_max + t) * BINS;
    auto ybin = [&](float2 x, int k) -> float2 {
        const float m = sqrtf(x.x * x.x + x.y * x.y);
        float scale = m == 0.f ? 0.f : dm[k] / m;
        const bool end = k == 0 || k == H;
        if (!end) scale *= 0.5f;
        return make_float2(x.x * scale, end ? 0.f : x.y * scale);
    };
#pragma unroll
    for (int q = 0; q <= Q / 2; ++q) {
        const int k = j + 64 * q;
        if (k <= H / 2) {
            const float2 zk = buf[fpad(k & (H - 1))], zc = buf[fpad((H - k) & (H - 1))];
            const float2 ya = ybin(rfft_split(zk, zc, p.tw2[k], k == 0), k);
            const float2 yb = ybin(rfft_split(zc, zk, p.tw2[H - k], k == 0), H - k);
            const float2 e = make_float2(ya.x + yb.x, ya.y - yb.y), d = make_float2(ya.x - yb.x, ya.y + yb.y);
            const float2 w = p.tw2[k];
            const float2 o = cmul(make_float2(w.x, -w.y), d);
            buf[fpad(k)] = make_float2(e.x - o.y, e.y + o.x);
            if (k != 0 && k != H / 2) buf[fpad(H - k)] = make_float2(e.x + o.y, o.x - e.y);
        }
    }
    wave_lds_fence();
    fft_lds_wave<H, true>(buf, p.tw, j);
    float* gf = g + ((size_t)b * p.W_max + t) * N;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int m = j + 64 * q;
        const float2 z = buf[fpad(m)];
        const float2 w = *reinterpret_cast<const float2*>(p.win + 2 * m);
        *reinterpret_cast<float2*>(gf + 2 * m) = make_float2(w.x * z.x, w.y * z.y);
    }
}

// the transpose of padding and framing: sample i sums the frame gradients at the padded positions that read it - its own, i + pad,
// and its images under the left and the right reflection - over the frames that cover each, in ascending order.  accumulate: the
// resolutions before this one are already in d_wav
__global__ __launch_bounds__(256) void mr_dwav_kernel(const MrSpec p, int N, const float* __restrict__ g, float* __restrict__ d_wav, int accumulate) {
    const int b = blockIdx.y, i = (int)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n_max) return;
    const int nb = mr_row_n(p.lens, p.n_max, p.min_n, b);
    float v = 0.f;
    if (i < nb) {
        const int W = mr_frames(nb, N, p.hop), pad = (N - p.hop) / 2;
        const float* gb = g + (size_t)b * p.W_max * N;
#pragma unroll
        for (int img = 0; img < 3; ++img) {
            const int q = img == 0 ? i + pad : (img == 1 ? pad - i : pad + 2 * (nb - 1) - i);
            const bool ok = img == 0 || (img == 1 ? (i >= 1 && i <= pad) : (i <= nb - 2 && i >= nb - 1 - pad));
            if (ok) {
                const int t_lo = q >= N ? (q - N) / p.hop + 1 : 0;
                const int t_hi = min(W - 1, q / p.hop);
                for (int t = t_lo; t <= t_hi; ++t) v += gb[(size_t)t * N + (q - t * p.hop)];
            }
        }
    }
    float* o = d_wav + (size_t)b * p.n_max + i;
    *o = accumulate ? (i < nb ? *o + v : 0.f) : v;
}

// ---- the convolutions

// how the time taps of one workgroup walk the operand's frames: tap j (weight tap t0 + j * tstep) of position u reads frame
// u * mul + base + j * hstep.  A data gradient's workgroup belongs to ONE stride phase ph: its output frames are u * stride + ph, and
// only the taps t = (ph + pad) mod stride, + stride, ... meet a dY frame
struct MrTaps { int n, t0, tstep, mul, base, hstep; };

template <bool BWD>
__device__ __forceinline__ MrTaps mr_taps(const MrConv& p, int ph) {
    if constexpr (!BWD) return MrTaps{p.kt, 0, 1, p.stride, -p.padt, 1};
    const int t0 = (ph + p.padt) % p.stride;
    return MrTaps{t0 < p.kt ? (p.kt - 1 - t0) / p.stride + 1 : 0, t0, p.stride, 1, (ph + p.padt - t0) / p.stride, -1};
}

// a tile behind its row: exact zeros inside the buffer, channels [n0, n0 + cols)
template <bool BWD>
__device__ __forceinline__ void mr_zero_tile(const MrConv& p, int b, int m0, int tile, int ph, int n0, int cols) {
    for (int idx = threadIdx.x; idx < tile * cols; idx += blockDim.x) {
        const int m = m0 + idx / cols, u = m / p.F;
        const int h = BWD ? u * p.stride + ph : u;
        if (h < p.Lo_max) p.out[(((size_t)b * p.Lo_max + h) * p.F + m % p.F) * p.NC + n0 + idx % cols] = 0.f;
    }
}

// the epilogue of one output element: bias + LeakyReLU, or cotangent + mask, and the zeros behind the row
template <bool BWD>
__device__ __forceinline__ void mr_finish(const MrConv& p, int b, int h, int col, int n, int Wo, float v) {
    if (h >= p.Lo_max) return;
    const size_t at = (((size_t)b * p.Lo_max + h) * p.F + col) * p.NC + n;
    if (h >= Wo) { p.out[at] = 0.f; return; }
    if constexpr (BWD) {
        if (p.dfeat) v += p.dfeat[at];
        if (p.mask) v = p.mask[at] > 0.f ? v : v * p.slope;
    } else {
        v += p.bias[n];
        if (p.act) v = v > 0.f ? v : v * p.slope;
    }
    p.out[at] = v;
}

// 32 WR positions x 32 WC channels, a 32 x 32 v_mfma_f32_32x32x2_f32 tile per wave; k-steps of (one time tap, 32 of its 3 KC floats)
// through LDS; the products of a 32-float block are summed apart over the time taps and then added
template <bool BWD, int WR, int WC>
__global__ void __launch_bounds__(256) mr_mfma_kernel(const MrConv p) {
    static_assert(WR * WC == 4, "four waves");
    constexpr int TM = 32 * WR, BN = 32 * WC;
    __shared__ __attribute__((aligned(16))) float As[TM * MR_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * MR_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / WC, wc = wave % WC, r = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z;
    const int n_tiles = p.NC / BN;
    const int n0 = ((int)blockIdx.y % n_tiles) * BN, ph = (int)blockIdx.y / n_tiles;
    const int m0 = (int)blockIdx.x * TM;
    const int nb = mr_row_n<true>(p.lens, p.n_max, p.min_n, b);
    const int Ws = mr_width(nb, p.n_fft, p.hop, p.n_src), Wo = mr_width(nb, p.n_fft, p.hop, p.n_out);
    const int h_first = BWD ? (m0 / p.F) * p.stride + ph : m0 / p.F;
    if (h_first >= Wo) {
        mr_zero_tile<BWD>(p, b, m0, TM, ph, n0, BN);
        return;
    }
    const MrTaps tp = mr_taps<BWD>(p, ph);
    const int ld_row = tid >> 3, ld_c4 = tid & 7;
    const int K3 = MR_KF * p.KC, K = p.kt * K3;
    const float* src_b = p.src + (size_t)b * p.Ls_max * p.F * p.KC;
    int a_u[WR], a_col[WR];
    bool a_live[WR];
    const float* w_row[WC];
#pragma unroll
    for (int i = 0; i < WR; ++i) {
        const int m = m0 + ld_row + 32 * i;
        a_u[i] = m / p.F;
        a_col[i] = m % p.F;
        a_live[i] = (BWD ? a_u[i] * p.stride + ph : a_u[i]) < Wo;
    }
#pragma unroll
    for (int i = 0; i < WC; ++i) w_row[i] = p.W + (size_t)(n0 + ld_row + 32 * i) * K;   // NC is a multiple of BN
    float4 a_reg[WR], b_reg[WC];
    bool a_keep[WR];
#pragma unroll
    for (int i = 0; i < WR; ++i) a_keep[i] = false;
    auto load = [&](int cb, int j) {
        const int c3 = 32 * cb + 4 * ld_c4, tf = (32 * cb) / p.KC;   // KC is a multiple of 32: a block lies in one frequency tap
#pragma unroll
        for (int i = 0; i < WR; ++i) {
            const int hs = a_u[i] * tp.mul + tp.base + j * tp.hstep, cf = a_col[i] + tf - 1;
            a_keep[i] = a_live[i] && hs >= 0 && hs < Ws && cf >= 0 && cf < p.F;
            const size_t at = a_keep[i] ? ((size_t)hs * p.F + a_col[i]) * p.KC + c3 - p.KC : 0;   // the run starts one bin below
            a_reg[i] = *reinterpret_cast<const float4*>(src_b + at);
        }
#pragma unroll
        for (int i = 0; i < WC; ++i) b_reg[i] = *reinterpret_cast<const float4*>(w_row[i] + (size_t)(tp.t0 + j * tp.tstep) * K3 + c3);
    };
    f32x16 acc, part;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f, part[e] = 0.f;
    const int n_it = (K3 / 32) * tp.n;   // (32-float block, time tap) pairs, the tap fastest
    int cb = 0, j = 0;
    if (n_it > 0) load(0, 0);
    for (int it = 0; it < n_it; ++it) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < WR; ++i) *reinterpret_cast<float4*>(&As[(ld_row + 32 * i) * MR_LD + 4 * ld_c4]) = a_keep[i] ? a_reg[i] : z;
#pragma unroll
        for (int i = 0; i < WC; ++i) *reinterpret_cast<float4*>(&Bs[(ld_row + 32 * i) * MR_LD + 4 * ld_c4]) = b_reg[i];
        __syncthreads();
        int nj = j + 1, ncb = cb;
        if (nj == tp.n) { nj = 0; ++ncb; }
        if (it + 1 < n_it) load(ncb, nj);
        const float* a_base = &As[(wr * 32 + r) * MR_LD + 4 * hh];
        const float* b_base = &Bs[(wc * 32 + r) * MR_LD + 4 * hh];
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
            const float4 af = *reinterpret_cast<const float4*>(a_base + 8 * kg);
            const float4 bf = *reinterpret_cast<const float4*>(b_base + 8 * kg);
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, part, 0, 0, 0);
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, part, 0, 0, 0);
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, part, 0, 0, 0);
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, part, 0, 0, 0);
        }
        if (nj == 0) {   // a block is done
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] += part[e], part[e] = 0.f;
        }
        __syncthreads();
        j = nj;
        cb = ncb;
    }
    // epilogue: lane (r, hh) holds column r of rows (e & 3) + 8 (e >> 2) + 4 hh of its 32 x 32 tile
    const int n = n0 + wc * 32 + r;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int m = m0 + wr * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh, u = m / p.F;
        mr_finish<BWD>(p, b, BWD ? u * p.stride + ph : u, m % p.F, n, Wo, acc[e]);
    }
}

// one operand channel, stride 1: a thread per output element (position, channel), channel fastest; at most 27 taps x 128 channels
template <bool BWD>
__global__ void __launch_bounds__(256) mr_narrow_in_kernel(const MrConv p) {
    __shared__ float ws[27 * 128];   // the weights as [tap][n]: the lanes of a wave read consecutive words
    const int b = blockIdx.z, m0 = (int)blockIdx.x * MR_TILE;
    const int nb = mr_row_n(p.lens, p.n_max, p.min_n, b);
    const int Ws = mr_width(nb, p.n_fft, p.hop, p.n_src), Wo = mr_width(nb, p.n_fft, p.hop, p.n_out);
    if (m0 / p.F >= Wo) {
        mr_zero_tile<false>(p, b, m0, MR_TILE, 0, 0, p.NC);
        return;
    }
    const int taps = p.kt * MR_KF;
    for (int idx = threadIdx.x; idx < taps * p.NC; idx += 256) ws[(idx % taps) * p.NC + idx / taps] = p.W[idx];   // [n][tap] -> [tap][n]
    __syncthreads();
    const float* src_b = p.src + (size_t)b * p.Ls_max * p.F;
    for (int idx = threadIdx.x; idx < MR_TILE * p.NC; idx += 256) {
        const int n = idx % p.NC, m = m0 + idx / p.NC, u = m / p.F, col = m % p.F;
        float sum = 0.f;
        if (u < Wo) {
            for (int tt = 0; tt < p.kt; ++tt) {
                const int hs = BWD ? u + p.padt - tt : u - p.padt + tt;
                if (hs < 0 || hs >= Ws) continue;
                const float* x = src_b + (size_t)hs * p.F + col - 1;
                float run = 0.f;
#pragma unroll
                for (int tf = 0; tf < MR_KF; ++tf)
                    if (col + tf >= 1 && col + tf <= p.F) run = fmaf(x[tf], ws[(tt * MR_KF + tf) * p.NC + n], run);
                sum += run;
            }
        }
        mr_finish<BWD>(p, b, u, col, n, Wo, sum);
    }
}

// one output channel, stride 1: a wave per position, the kt * 3 KC products dealt over its lanes in float4s and added by a fixed butterfly
template <bool BWD>
__global__ void __launch_bounds__(256) mr_narrow_out_kernel(const MrConv p) {
    const int b = blockIdx.z, m0 = (int)blockIdx.x * MR_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb = mr_row_n<true>(p.lens, p.n_max, p.min_n, b);
    const int Ws = mr_width(nb, p.n_fft, p.hop, p.n_src), Wo = mr_width(nb, p.n_fft, p.hop, p.n_out);
    if (m0 / p.F >= Wo) {
        mr_zero_tile<false>(p, b, m0, MR_TILE, 0, 0, 1);
        return;
    }
    const float* src_b = p.src + (size_t)b * p.Ls_max * p.F * p.KC;
    const int run4 = MR_KF * p.KC / 4, total = p.kt * run4;
    for (int q = wave; q < MR_TILE; q += 4) {
        const int m = m0 + q, u = m / p.F, col = m % p.F;
        float sum = 0.f;
        if (u < Wo) {
            for (int it = lane; it < total; it += 64) {
                const int tt = it / run4, c3 = 4 * (it % run4), cf = col + c3 / p.KC - 1;
                const int hs = BWD ? u + p.padt - tt : u - p.padt + tt;
                if (hs < 0 || hs >= Ws || cf < 0 || cf >= p.F) continue;
                const float4 xv = *reinterpret_cast<const float4*>(src_b + ((size_t)hs * p.F + col) * p.KC + c3 - p.KC);
                const float4 wv = *reinterpret_cast<const float4*>(p.W + (size_t)tt * MR_KF * p.KC + c3);
                sum = fmaf(xv.w, wv.w, fmaf(xv.z, wv.z, fmaf(xv.y, wv.y, fmaf(xv.x, wv.x, sum))));
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
        if (lane == 0) mr_finish<BWD>(p, b, u, col, 0, Wo, sum);
    }
}

// the rows [b0, b1) and the frames [chunk * MR_PIECE_FRAMES, + MR_PIECE_FRAMES) of each that a weight-gradient piece sums
struct MrSpan { int b0, b1, chunk; };
__device__ __forceinline__ MrSpan mr_span(int piece, int B, int chunks, int rows_per_piece) {
    const int b0 = (piece / chunks) * rows_per_piece;
    return MrSpan{b0, b0 + rows_per_piece < B ? b0 + rows_per_piece : B, piece % chunks};
}

// one piece of dW[tap][n][c] = sum over positions of dY[w][f][n] X[w stride + tt - pad][f + tf - 1][c], tap = tf * kt + tt as PyTorch
// numbers a (3, kt) kernel: 32 n x 32 c of one tap, positions on k, 16 of every 64 to each wave; the four waves' sums are added in
// their order
__global__ void __launch_bounds__(256) mr_wgrad_mfma_kernel(const MrConv p, float* parts, int B, int chunks, int rows_per_piece) {
    __shared__ __attribute__((aligned(16))) float sm[2 * MR_WG_CHUNK * 32];
    float* As = sm;
    float* Bs = sm + MR_WG_CHUNK * 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int taps = p.kt * MR_KF;
    const int piece = (int)blockIdx.x / taps, tap = (int)blockIdx.x % taps, tf = tap / p.kt, tt = tap % p.kt;
    const int n0 = (int)blockIdx.y * 32, c0 = (int)blockIdx.z * 32;
    const MrSpan sp = mr_span(piece, B, chunks, rows_per_piece);
    const int ld_row = tid >> 3, ld_c4 = tid & 7;
    f32x16 acc, part;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f, part[e] = 0.f;
    int since = 0;
    for (int b = sp.b0; b < sp.b1; ++b) {
        const int nb = mr_row_n<true>(p.lens, p.n_max, p.min_n, b);
        const int Ws = mr_width(nb, p.n_fft, p.hop, p.n_src), Wo = mr_width(nb, p.n_fft, p.hop, p.n_out);
        const int la = sp.chunk * MR_PIECE_FRAMES * p.F, lb = min(sp.chunk * MR_PIECE_FRAMES + MR_PIECE_FRAMES, Wo) * p.F;
        const float* dy_b = p.dy + (size_t)b * p.Lo_max * p.F * p.NC + n0 + 4 * ld_c4;
        const float* x_b = p.src + (size_t)b * p.Ls_max * p.F * p.KC + c0 + 4 * ld_c4;
        for (int l0 = la; l0 < lb; l0 += MR_WG_CHUNK) {
            float4 a_reg[2], b_reg[2];
            bool a_keep[2], b_keep[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = l0 + ld_row + 32 * i, u = m / p.F, cf = m % p.F + tf - 1, hs = u * p.stride + tt - p.padt;
                a_keep[i] = m < lb;
                b_keep[i] = m < lb && hs >= 0 && hs < Ws && cf >= 0 && cf < p.F;
                a_reg[i] = *reinterpret_cast<const float4*>(dy_b + (a_keep[i] ? (size_t)m * p.NC : 0));
                b_reg[i] = *reinterpret_cast<const float4*>(x_b + (b_keep[i] ? ((size_t)hs * p.F + cf) * p.KC : 0));
            }
            __syncthreads();   // the products of the chunk before are done with the LDS
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
                *reinterpret_cast<float4*>(&As[(ld_row + 32 * i) * 32 + 4 * ld_c4]) = a_keep[i] ? a_reg[i] : z;
                *reinterpret_cast<float4*>(&Bs[(ld_row + 32 * i) * 32 + 4 * ld_c4]) = b_keep[i] ? b_reg[i] : z;
            }
            __syncthreads();
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) {
                const int k = 16 * wave + 2 * ks + hh;
                part = __builtin_amdgcn_mfma_f32_32x32x2f32(As[k * 32 + r], Bs[k * 32 + r], part, 0, 0, 0);
            }
            if (++since == 8) {   // a wave's 128 positions are summed apart, then added
                since = 0;
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] += part[e], part[e] = 0.f;
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] += part[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e) sm[wave * 1024 + e * 64 + lane] = acc[e];
    __syncthreads();
    for (int x = tid; x < 1024; x += 256) {
        const float s = ((sm[x] + sm[1024 + x]) + sm[2048 + x]) + sm[3072 + x];
        const int e = x >> 6, ln = x & 63;
        const int n = n0 + (e & 3) + 8 * (e >> 2) + 4 * (ln >> 5), c = c0 + (ln & 31);
        parts[(((size_t)piece * taps + tap) * p.NC + n) * p.KC + c] = s;
    }
}
static_assert(2 * MR_WG_CHUNK * 32 == 4 * 1024, "the weight gradient's LDS holds the four waves' tiles");

// the same piece in VALU code: the first layer's and the score's.  A thread per element of [tap][n][c], c fastest, so that a wave reads
// consecutive channels of whichever operand has them; the bins of the piece are dealt over MR_WG_VALU_SPLIT such threads, each of which
// leaves its own partial sum (the reduction adds frames-pieces x bin classes in a fixed order)
__global__ void __launch_bounds__(256) mr_wgrad_valu_kernel(const MrConv p, float* parts, int B, int chunks, int rows_per_piece) {
    const size_t numel = (size_t)p.NC * p.KC * p.kt * MR_KF;
    const size_t o = (size_t)blockIdx.y * 64 + (threadIdx.x & 63);
    if (o >= numel) return;
    const int fs = (int)blockIdx.z * 4 + (threadIdx.x >> 6);
    const int c = (int)(o % p.KC), n = (int)((o / p.KC) % p.NC), tap = (int)(o / ((size_t)p.KC * p.NC)), tf = tap / p.kt, tt = tap % p.kt;
    const int piece = blockIdx.x;
    const MrSpan sp = mr_span(piece, B, chunks, rows_per_piece);
    const int f_lo = tf == 0 ? 1 : 0, f_hi = tf == 2 ? p.F - 1 : p.F;   // the bins whose tap tf lies inside the map
    float acc = 0.f;
    for (int b = sp.b0; b < sp.b1; ++b) {
        const int nb = mr_row_n(p.lens, p.n_max, p.min_n, b);
        const int Ws = mr_width(nb, p.n_fft, p.hop, p.n_src), Wo = mr_width(nb, p.n_fft, p.hop, p.n_out);
        const int wa = sp.chunk * MR_PIECE_FRAMES, wb = min(wa + MR_PIECE_FRAMES, Wo);
        float part = 0.f;
        for (int w = wa; w < wb; ++w) {
            const int hs = w * p.stride + tt - p.padt;
            if (hs < 0 || hs >= Ws) continue;
            const float* dy = p.dy + (((size_t)b * p.Lo_max + w) * p.F) * p.NC + n;
            const float* x = p.src + (((size_t)b * p.Ls_max + hs) * p.F) * p.KC + c;
            for (int f = f_lo + fs; f < f_hi; f += MR_WG_VALU_SPLIT) part = fmaf(dy[(size_t)f * p.NC], x[(size_t)(f + tf - 1) * p.KC], part);
        }
        acc += part;
    }
    parts[((size_t)piece * MR_WG_VALU_SPLIT + fs) * numel + o] = acc;
}

// db[n] = sum over rows and positions of dy, in float64: a workgroup takes 32 channels and one slice of the flat positions
// [B][Lo_max][F]; eight lanes per channel stride the slice
__global__ void __launch_bounds__(256) mr_db_kernel(const MrConv p, double* db_parts, int B) {
    __shared__ double red[8][32];
    const int ch = threadIdx.x & 31, ln = threadIdx.x >> 5;
    const int n = (int)blockIdx.x * 32 + ch, slice = blockIdx.y;
    const long per_row = (long)p.Lo_max * p.F, total = per_row * B;
    const long per = (total + DC_DB_SLICES - 1) / DC_DB_SLICES, lo = slice * per, hi = lo + per < total ? lo + per : total;
    double v = 0.0;
    int b_cur = -1, Wo = 0;
    for (long m = lo + ln; m < hi; m += 8) {
        const int b = (int)(m / per_row);
        if (b != b_cur) { b_cur = b; Wo = mr_width(mr_row_n(p.lens, p.n_max, p.min_n, b), p.n_fft, p.hop, p.n_out); }
        if ((int)((m % per_row) / p.F) < Wo && n < p.NC) v += (double)p.dy[(size_t)m * p.NC + n];
    }
    red[ln][ch] = v;
    __syncthreads();
    if (ln == 0 && n < p.NC) {
        double sum = red[0][ch];
        for (int i = 1; i < 8; ++i) sum += red[i][ch];
        db_parts[(size_t)slice * p.NC + n] = sum;
    }
}

// W [n][c][tf][tt] (PyTorch) -> wf [n][tt][tf][c] and wb [c][tt][2 - tf][n]
__global__ void __launch_bounds__(256) mr_pack_kernel(const float* W, float* wf, float* wb, int NC, int KC, int kt) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= (size_t)NC * KC * kt * MR_KF) return;
    const int tt = (int)(o % kt), tf = (int)((o / kt) % MR_KF), c = (int)((o / ((size_t)kt * MR_KF)) % KC), n = (int)(o / ((size_t)kt * MR_KF * KC));
    wf[(((size_t)n * kt + tt) * MR_KF + tf) * KC + c] = W[o];
    wb[(((size_t)c * kt + tt) * MR_KF + (MR_KF - 1 - tf)) * NC + n] = W[o];
}

// the padded window and the twiddle factors w_H^m, w_N^k of one resolution, in double
__global__ void __launch_bounds__(256) mr_tables_kernel(float* win, float2* tw, float2* tw2, int N, int wl, int hann) {
    const int i = (int)blockIdx.x * 256 + threadIdx.x, H = N / 2, off = (N - wl) / 2;
    const double two_pi = 6.283185307179586476925286766559;
    if (i < N) {
        const int k = i - off;
        win[i] = (k >= 0 && k < wl) ? (hann ? (float)(0.5 - 0.5 * cos(two_pi * k / wl)) : 1.f) : 0.f;
    }
    if (i < H) tw[i] = make_float2((float)cos(two_pi * i / H), (float)-sin(two_pi * i / H));
    if (i <= H) tw2[i] = make_float2((float)cos(two_pi * i / N), (float)-sin(two_pi * i / N));
}

// ---- host

MrConv mr_conv(const gvx_mrd_dims& d, const MrLayer& l, const MrFeat& F, int r, int i, const int32_t* lens, int n_max) {
    MrConv p{};
    p.lens = lens; p.n_max = n_max; p.min_n = mr_min_samples(d); p.n_fft = d.n_fft[r]; p.hop = d.hop[r];
    p.F = F.bins[r]; p.KC = l.cin; p.NC = l.cout; p.kt = l.kt; p.stride = l.stride; p.padt = l.padt;
    p.Ls_max = i == 0 ? mr_frames(n_max, d.n_fft[r], d.hop[r]) : F.frames[r][i - 1];
    p.Lo_max = F.frames[r][i];
    p.n_src = i; p.n_out = i + 1;
    p.act = l.act; p.slope = d.slope;
    return p;
}

// the data gradient is a convolution with the sides exchanged: dY is the operand, the layer's input map (`mask`, its cotangent `dfeat`)
// the output, the weights the blob's second form
MrConv mr_exchanged(const MrConv& p, const float* dy, const float* wb, const float* mask, const float* dfeat, float* out) {
    MrConv q = p;
    q.src = dy; q.W = wb; q.bias = nullptr; q.dy = nullptr;
    q.KC = p.NC; q.NC = p.KC;
    q.Ls_max = p.Lo_max; q.Lo_max = p.Ls_max; q.n_src = p.n_out; q.n_out = p.n_src;
    q.mask = mask; q.dfeat = dfeat; q.out = out;
    return q;
}

// forward of a layer, or with BWD its data gradient: there `p` already has the two sides exchanged
template <bool BWD>
int mr_launch_conv(const MrConv& p, int B, hipStream_t s) {
    const int phases = BWD ? p.stride : 1;
    const int frames = BWD ? (p.Lo_max + p.stride - 1) / p.stride : p.Lo_max;
    const size_t positions = (size_t)frames * p.F;
    if (positions == 0) return GVX_OK;
    auto tiles = [&](int tile) { return (unsigned)((positions + tile - 1) / tile); };
    if (p.KC == 1) {   // stride 1: the first layer and the score
        mr_narrow_in_kernel<BWD><<<dim3(tiles(MR_TILE), 1, (unsigned)B), 256, 0, s>>>(p);
    } else if (p.NC == 1) {
        mr_narrow_out_kernel<BWD><<<dim3(tiles(MR_TILE), 1, (unsigned)B), 256, 0, s>>>(p);
    } else if (p.NC % 64 == 0) {
        mr_mfma_kernel<BWD, 2, 2><<<dim3(tiles(MR_TILE), (unsigned)(p.NC / 64 * phases), (unsigned)B), 256, 0, s>>>(p);
    } else {
        mr_mfma_kernel<BWD, 4, 1><<<dim3(tiles(MR_TILE_NARROW), (unsigned)(p.NC / 32 * phases), (unsigned)B), 256, 0, s>>>(p);
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

MrSpec mr_spec(const gvx_mrd* h, size_t per_res, int r, const int32_t* lens, int n_max) {
    const gvx_mrd_dims& d = h->d;
    const MrTables T = mr_tables(d, per_res, r);
    return MrSpec{h->blob + T.win, reinterpret_cast<const float2*>(h->blob + T.tw), reinterpret_cast<const float2*>(h->blob + T.tw2),
                  lens, n_max, mr_min_samples(d), d.hop[r], mr_frames(n_max, d.n_fft[r], d.hop[r])};
}

// grad: the frame gradients from d_mag; otherwise the magnitudes
int mr_launch_spec(const MrSpec& sp, int n_fft, const float* wav, int B, float* mag, const float* dmag, float* g, hipStream_t s) {
    if (sp.W_max == 0) return GVX_OK;
    const dim3 grid((unsigned)((sp.W_max + MR_FRAMES_PER_WG - 1) / MR_FRAMES_PER_WG), (unsigned)B);
    const int threads = MR_FRAMES_PER_WG * 64;
    switch (n_fft) {
        case 512:
            if (g) mr_spec_grad_kernel<256><<<grid, threads, 0, s>>>(wav, sp, dmag, g);
            else mr_spec_kernel<256><<<grid, threads, 0, s>>>(wav, sp, mag);
            break;
        case 1024:
            if (g) mr_spec_grad_kernel<512><<<grid, threads, 0, s>>>(wav, sp, dmag, g);
            else mr_spec_kernel<512><<<grid, threads, 0, s>>>(wav, sp, mag);
            break;
        default:
            if (g) mr_spec_grad_kernel<1024><<<grid, threads, 0, s>>>(wav, sp, dmag, g);
            else mr_spec_kernel<1024><<<grid, threads, 0, s>>>(wav, sp, mag);
            break;
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int mr_check_call(const gvx_mrd* h, const float* wav, const void* features, int B, int n_max) {
    if (const int rc = dc_check_call(h, wav, features, B)) return rc;
    if (n_max < mr_min_samples(h->d))
        return fail(GVX_ERR_INVALID_ARG, "n_max = %d: the widest reflection needs at least %d samples", n_max, mr_min_samples(h->d));
    if (n_max > GVX_MRD_MAX_SAMPLES) return fail(GVX_ERR_UNSUPPORTED, "n_max = %d is beyond the limit of %d samples", n_max, GVX_MRD_MAX_SAMPLES);
    if (mr_bad_shape(&h->d, B, n_max))
        return fail(GVX_ERR_UNSUPPORTED, "n_max = %d: a spectrogram would have more than %d cells in a row", n_max, GVX_MRD_MAX_POSITIONS);
    return GVX_OK;
}

}  // namespace

extern "C" {

size_t gvx_mrd_blob_floats(const gvx_mrd_dims* dims) {
    if (mr_dims_problem(dims)) return 0;
    return mr_blob_floats(*dims);
}

int gvx_mrd_layout(const gvx_mrd_dims* dims, int B, int n_max, gvx_mrd_entry* entries, int max_entries) {
    if (mr_bad_shape(dims, B, n_max)) return 0;
    const MrFeat F = mr_feat_layout(*dims, B, n_max);
    int n = 0;
    for (int r = 0; r < dims->n_resolutions; ++r)
        for (int i = 0; i < MR_MAPS; ++i, ++n)
            if (entries && n < max_entries) {
                const int64_t C = F.channels[i], W = F.frames[r][i], Fb = F.bins[r];
                entries[n] = gvx_mrd_entry{(uint64_t)F.off[r][i], (int32_t)C, (int32_t)W, (int32_t)Fb, 0, W * Fb * C, 1, Fb * C, C};
            }
    return n;
}

size_t gvx_mrd_features_bytes(const gvx_mrd_dims* dims, int B, int n_max) {
    if (mr_bad_shape(dims, B, n_max)) return 0;
    return mr_feat_layout(*dims, B, n_max).total;
}

size_t gvx_mrd_workspace_bytes(const gvx_mrd_dims* dims, int B, int n_max, int backward) {
    if (mr_bad_shape(dims, B, n_max)) return 0;
    return mr_ws_plan(*dims, B, n_max, backward != 0).total;
}

int gvx_mrd_pack_weights_device(const gvx_mrd_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = mr_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    MrLayer L[MR_MAPS];
    size_t per_res = 0;
    const int nl = mr_layers(*dims, L, &per_res);
    hipStream_t s = (hipStream_t)stream;
    const int rc = dc_pack_weights(table, n, dims->n_resolutions, L, nl, per_res, device_blob, s, [&](const MrLayer& l, const float* W, float* base) {
        mr_pack_kernel<<<(unsigned)((l.wn() + 255) / 256), 256, 0, s>>>(W, base + l.wf_off, base + l.wb_off, l.cout, l.cin, l.kt);
    });
    if (rc != GVX_OK) return rc;
    for (int r = 0; r < dims->n_resolutions; ++r) {
        const MrTables T = mr_tables(*dims, per_res, r);
        const int N = dims->n_fft[r];
        mr_tables_kernel<<<(unsigned)(N / 256 + 1), 256, 0, s>>>(device_blob + T.win, reinterpret_cast<float2*>(device_blob + T.tw),
                                                                reinterpret_cast<float2*>(device_blob + T.tw2), N, dims->win[r],
                                                                dims->window == GVX_MRD_WINDOW_HANN);
        HIP_TRY(hipGetLastError());
    }
    return GVX_OK;
}

int gvx_mrd_create(const gvx_mrd_dims* dims, gvx_mrd** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = mr_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_mrd* h = new gvx_mrd();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_mrd_destroy(gvx_mrd* h) { delete h; }

int gvx_mrd_timing_enable(gvx_mrd* h, int enable) { return dc_timing_enable(h, enable); }

int gvx_mrd_layer_times_ms(gvx_mrd* h, float* forward_ms, float* backward_ms, int* n_layers_out) {
    return dc_layer_times_ms(h, h ? h->d.n_resolutions : 0, h ? MR_MAPS : 0, forward_ms, backward_ms, n_layers_out);
}

int gvx_mrd_bind(gvx_mrd* h, const float* device_blob) { return gen_bind(h, device_blob); }

int gvx_mrd_forward(gvx_mrd* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features, size_t features_bytes,
                    void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = mr_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    const gvx_mrd_dims& d = h->d;
    const MrFeat F = mr_feat_layout(d, B, n_max);
    if ((rc = dc_check_features(features, features_bytes, F.total)) != GVX_OK) return rc;
    const MrWs wp = mr_ws_plan(d, B, n_max, false);
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    MrLayer L[MR_MAPS];
    size_t per_res = 0;
    const int nl = mr_layers(d, L, &per_res);
    float* mag = gvx::ws_ptr<float>(workspace, wp.mag);
    for (int r = 0; r < d.n_resolutions; ++r) {
        if ((rc = dc_mark(h, h->marks, (size_t)r * (nl + 1), s)) != GVX_OK) return rc;
        if ((rc = mr_launch_spec(mr_spec(h, per_res, r, sample_lengths, n_max), d.n_fft[r], wav, B, mag, nullptr, nullptr, s)) != GVX_OK) return rc;
        const float* in = mag;
        for (int i = 0; i < nl; ++i) {
            MrConv p = mr_conv(d, L[i], F, r, i, sample_lengths, n_max);
            p.src = in; p.W = h->blob + r * per_res + L[i].wf_off; p.bias = h->blob + r * per_res + L[i].b_off;
            p.out = gvx::ws_ptr<float>(features, F.off[r][i]);
            if ((rc = mr_launch_conv<false>(p, B, s)) != GVX_OK) return rc;
            in = p.out;
            if ((rc = dc_mark(h, h->marks, (size_t)r * (nl + 1) + i + 1, s)) != GVX_OK) return rc;
        }
    }
    h->fwd_timed = h->timing;
    return GVX_OK;
}

int gvx_mrd_backward(gvx_mrd* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, const void* features,
                     const void* d_features, const gvx_grad_desc* grads, int n_grads, float* d_wav, void* workspace,
                     size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = mr_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    if ((rc = dc_check_backward(features, d_features, grads, n_grads, d_wav)) != GVX_OK) return rc;
    const gvx_mrd_dims& d = h->d;
    const MrFeat F = mr_feat_layout(d, B, n_max);
    const MrWs wp = mr_ws_plan(d, B, n_max, true);
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    MrLayer L[MR_MAPS];
    size_t per_res = 0;
    const int nl = mr_layers(d, L, &per_res);
    DcParam g[DC_MAX_STACKS * DC_MAX_MAPS] = {};
    if ((rc = dc_find_grads(grads, n_grads, d.n_resolutions, L, nl, g)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    float* mag = gvx::ws_ptr<float>(workspace, wp.mag);
    float* dmag = gvx::ws_ptr<float>(workspace, wp.dmag);
    float* frame_grads = gvx::ws_ptr<float>(workspace, wp.g);
    float* gbuf[2] = {gvx::ws_ptr<float>(workspace, wp.grad[0]), gvx::ws_ptr<float>(workspace, wp.grad[1])};
    float* parts = gvx::ws_ptr<float>(workspace, wp.parts);
    double* db_parts = gvx::ws_ptr<double>(workspace, wp.db_parts);
    auto feat = [&](const void* base, int r, int i) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + F.off[r][i]); };
    for (int r = 0; r < d.n_resolutions; ++r) {
        const float* blob = h->blob + r * per_res;
        const MrSpec sp = mr_spec(h, per_res, r, sample_lengths, n_max);
        const float* dcur = feat(d_features, r, nl - 1);   // the score has no activation: its cotangent is its pre-activation's
        if ((rc = dc_mark(h, h->bwd_marks, (size_t)r * (nl + 1) + nl, s)) != GVX_OK) return rc;
        if (n_grads > 0 && (rc = mr_launch_spec(sp, d.n_fft[r], wav, B, mag, nullptr, nullptr, s)) != GVX_OK) return rc;   // the first layer's operand
        for (int i = nl - 1; i >= 0; --i) {
            MrConv p = mr_conv(d, L[i], F, r, i, sample_lengths, n_max);
            if (n_grads > 0) {
                p.src = i == 0 ? mag : feat(features, r, i - 1);
                p.dy = dcur;
                const MrPieces P = mr_pieces(L[i], B, p.Lo_max);
                if (L[i].mfma)
                    mr_wgrad_mfma_kernel<<<dim3((unsigned)(P.n * p.kt * MR_KF), (unsigned)(p.NC / 32), (unsigned)(p.KC / 32)), 256, 0, s>>>(
                        p, parts, B, P.chunks, P.rows_per_piece);
                else
                    mr_wgrad_valu_kernel<<<dim3((unsigned)P.n, (unsigned)((P.numel + 63) / 64), MR_WG_VALU_SPLIT / 4), 256, 0, s>>>(p, parts, B, P.chunks, P.rows_per_piece);
                HIP_TRY(hipGetLastError());
                dc_reduce_kernel<true><<<(unsigned)((P.numel + 31) / 32), 256, 0, s>>>(parts, g[r * nl + i].w, p.NC, p.KC, p.kt * MR_KF, P.n * P.split);
                HIP_TRY(hipGetLastError());
                mr_db_kernel<<<dim3((unsigned)((p.NC + 31) / 32), DC_DB_SLICES), 256, 0, s>>>(p, db_parts, B);
                HIP_TRY(hipGetLastError());
                dc_db_reduce_kernel<<<(unsigned)((p.NC + 255) / 256), 256, 0, s>>>(db_parts, g[r * nl + i].b, p.NC);
                HIP_TRY(hipGetLastError());
            }
            if (i > 0) {
                const MrConv q = mr_exchanged(p, dcur, blob + L[i].wb_off, feat(features, r, i - 1), feat(d_features, r, i - 1), gbuf[i & 1]);
                if ((rc = mr_launch_conv<true>(q, B, s)) != GVX_OK) return rc;
                dcur = q.out;
            } else if (d_wav) {
                const MrConv q = mr_exchanged(p, dcur, blob + L[0].wb_off, nullptr, nullptr, dmag);
                if ((rc = mr_launch_conv<true>(q, B, s)) != GVX_OK) return rc;
                if ((rc = mr_launch_spec(sp, d.n_fft[r], wav, B, nullptr, dmag, frame_grads, s)) != GVX_OK) return rc;
                mr_dwav_kernel<<<dim3((unsigned)((n_max + 255) / 256), (unsigned)B), 256, 0, s>>>(sp, d.n_fft[r], frame_grads, d_wav, r > 0);
                HIP_TRY(hipGetLastError());
            }
            if ((rc = dc_mark(h, h->bwd_marks, (size_t)r * (nl + 1) + i, s)) != GVX_OK) return rc;   // mark i: layer i is done
        }
    }
    h->bwd_timed = h->timing;
    return GVX_OK;
}

}  // C ABI
