// HiFi-GAN period discriminators (include/genvox_amd.h, "HiFi-GAN period discriminators"): forward, and the backward that reads the
// forward's own maps as its tape.  Maps are channels-last, [B][height][period][channels]: a grid cell's channels are contiguous, which
// is what an implicit GEMM with positions on M and channels on K wants.
//
// The tiles, the tap walk by stride phase, the VALU kernels (the first layer, which absorbs the reflection and the reshape: its operand
// is the waveform; the score; narrow layers), the piece reduction and the bias gradient are the shared core's (disc_conv.h, its GRID
// form; disc_host.h).  What is here:
//   pd_mfma_kernel     the wide layers, forward (BWD = false) and data gradient (BWD = true): 64 positions x 128 channels (64 where fewer
//                      than 128 are produced), four waves of two (one) 32 x 32 v_mfma_f32_32x32x2_f32 tiles each, k-steps of (one tap,
//                      32 channels) through LDS; the products of a channel block are summed apart and then added, so the 5 C_in terms
//                      never form one chain.
//   pd_wgrad_mfma_kernel   one piece (rows, or a run of positions of one row) of a weight gradient, laid out [tap][c_out][c_in], as the
//                      VALU pieces of this discriminator are (TAP_MAJOR).
//   pd_dwav_kernel     the adjoint of reshape + reflection as a gather, accumulated over the periods in their order.
// No atomics anywhere: two calls give the same bits.
#include "disc_host.h"
#include "hifigan_disc_internal.h"

using gvx::fail;
using namespace gvx_pd;

static_assert(PD_TILE == GVX_HIFIGAN_MPD_TILE && PD_TILE_N == GVX_HIFIGAN_MPD_TILE_N && PD_TILE_N_WIDE == GVX_HIFIGAN_MPD_TILE_N_WIDE &&
                  PD_MFMA_MULT == GVX_HIFIGAN_MPD_MFMA_MULT,
              "the public header states the tile constants");
static_assert(GVX_HIFIGAN_MPD_MAX_PERIODS <= DC_MAX_STACKS, "a period is a stack of the shared host side");

struct gvx_hifigan_mpd : DcHandle {
    gvx_hifigan_mpd_dims d;
};

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int PD_LD = 36;    // floats per LDS row of a 32-deep k-tile: the fragment reads of sixteen lanes fall on distinct 16-byte slots
constexpr int PD_WLD = 96;   // floats per LDS row of the weight gradient's 64-wide operands: the two k rows of a step 32 banks apart

// TN = 1: 64 positions x 64 channels, a 32 x 32 tile per wave; TN = 2: 64 x 128, two tiles per wave off one A fragment.  TN = 1
// states its five waves per SIMD: it sits at their edge (95 of 102 registers), and left to itself the register allocator falls to four
// with any change to the prologue's length arithmetic; TN = 2 states the default.  Both want the row's heights in scalar registers
template <bool BWD, int TN>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(TN == 1 ? 5 : 1))) pd_mfma_kernel(const DcConv p) {
    constexpr int BN = PD_TILE_N * TN;
    __shared__ __attribute__((aligned(16))) float As[PD_TILE * PD_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN * PD_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1, r = lane & 31, hh = lane >> 5;
    const int b = blockIdx.z;
    const int n_tiles = (p.NC + BN - 1) / BN;
    const int n0 = ((int)blockIdx.y % n_tiles) * BN, ph = (int)blockIdx.y / n_tiles;
    const int m0 = (int)blockIdx.x * PD_TILE;
    const int nb = dc_row_n<true>(p, b);
    const int Hs = dc_len<true>(p, nb, p.n_src), Ho = dc_len<true>(p, nb, p.n_out);
    const int h_first = BWD ? (m0 / p.period) * p.stride + ph : m0 / p.period;
    if (h_first >= Ho) {
        dc_zero_tile<true, BWD>(p, b, m0, ph, n0, min(BN, p.NC - n0));
        return;
    }
    const DcTaps tp = dc_taps<BWD>(p, ph);
    const int ld_row = tid >> 3, ld_c4 = tid & 7;
    const int K = p.k * p.KC;
    const float* src_b = p.src + (size_t)b * p.Ls_max * p.period * p.KC;
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
            dc_finish<true, BWD>(p, b, BWD ? u * p.stride + ph : u, col, n, Ho, acc[t][e]);
        }
    }
}

// one piece of dW[t][n][c] = sum over positions of dY[pos][n] X[source height of (pos, t)][c]: 64 n x 64 c of one tap, positions on k
__global__ void __launch_bounds__(256) pd_wgrad_mfma_kernel(const DcConv p, float* parts, int B, int chunks, int rows_per_piece, int run) {
    __shared__ __attribute__((aligned(16))) float As[PD_WG_CHUNK * PD_WLD];
    __shared__ __attribute__((aligned(16))) float Bs[PD_WG_CHUNK * PD_WLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1, r = lane & 31, hh = lane >> 5;
    const int n0 = (int)blockIdx.x * 64, c0 = (int)blockIdx.y * 64;
    const int piece = (int)blockIdx.z / p.k, t = (int)blockIdx.z % p.k;
    const DcSpan sp = dc_span(piece, B, chunks, rows_per_piece);
    const int ld_row = tid >> 4, ld_c4 = tid & 15;
    const bool n_ok = n0 + 4 * ld_c4 < p.NC, c_ok = c0 + 4 * ld_c4 < p.KC;   // both counts are multiples of 32: a float4 is whole
    f32x16 acc, part;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f, part[e] = 0.f;
    int since = 0;
    for (int b = sp.b0; b < sp.b1; ++b) {
        const int nb = dc_row_n(p, b);
        const int Hs = dc_len<true>(p, nb, p.n_src), Ho = dc_len<true>(p, nb, p.n_out);
        const int la = sp.chunk * run, lb = min(la + run, Ho * p.period);
        const float* dy_b = p.dy + (size_t)b * p.Lo_max * p.period * p.NC;
        const float* x_b = p.src + (size_t)b * p.Ls_max * p.period * p.KC;
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

// gradient of the waveform through one period: sample i collects its own cell and the cell behind the row that mirrors it; a cell's
// gradient is the first layer's data gradient, gathered by stride phase.  p.dy: gradient of the first layer's pre-activation
// [B][Lo_max][period][NC]; p.W its weights [NC][k].  accumulate: the periods before this one are already in d_wav.
__global__ void __launch_bounds__(256) pd_dwav_kernel(const DcConv p, float* d_wav, int accumulate) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n_max) return;
    const int nb = dc_row_n(p, b);
    float v = 0.f;
    if (i < nb) {
        const int H0 = dc_len<true>(p, nb, 0), Ho = dc_len<true>(p, nb, p.n_out);
        const int mirror = 2 * (nb - 1) - i;
        const int cell[2] = {i, (mirror >= nb && mirror < H0 * p.period) ? mirror : -1};
        const float* dy_b = p.dy + (size_t)b * p.Lo_max * p.period * p.NC;
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

DcConv pd_conv(const gvx_hifigan_mpd_dims& d, const PdLayer& l, const PdFeat& F, int j, int i, const int32_t* lens, int n_max) {
    DcConv p{};
    p.lens = lens; p.n_max = n_max; p.min_n = pd_min_samples(d);
    p.period = d.periods[j]; p.KC = p.KG = l.cin; p.NC = p.NG = l.cout; p.k = l.k; p.stride = l.stride; p.pad = l.pad;
    pd_strides(d, p.str);
    p.Ls_max = i == 0 ? dc_length(n_max, p.period, p.str, 0) : F.height[j][i - 1];
    p.Lo_max = F.height[j][i];
    p.n_src = i; p.n_out = i + 1;
    p.act = l.act; p.wav_src = i == 0; p.slope = d.slope;
    return p;
}

// forward of layer (j, i), or with BWD its data gradient: there `p` already has the two sides exchanged
template <bool BWD>
int pd_launch_conv(const DcConv& p, bool mfma, int B, hipStream_t s) {
    const int phases = BWD ? p.stride : 1;
    const int heights = BWD ? (p.Lo_max + p.stride - 1) / p.stride : p.Lo_max;
    const unsigned tiles = (unsigned)(((size_t)heights * p.period + PD_TILE - 1) / PD_TILE);
    if (mfma && p.NC >= PD_TILE_N_WIDE) {   // the wide N tile wherever a whole one fits
        const int n_tiles = (p.NC + PD_TILE_N_WIDE - 1) / PD_TILE_N_WIDE;
        pd_mfma_kernel<BWD, 2><<<dim3(tiles, (unsigned)(n_tiles * phases), (unsigned)B), 256, 0, s>>>(p);
    } else if (mfma) {
        const int n_tiles = (p.NC + PD_TILE_N - 1) / PD_TILE_N;
        pd_mfma_kernel<BWD, 1><<<dim3(tiles, (unsigned)(n_tiles * phases), (unsigned)B), 256, 0, s>>>(p);
    } else {
        dc_launch_valu<true, BWD>(p, tiles, phases, B, s);
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

bool pd_bad_shape(const gvx_hifigan_mpd_dims* dims, int B, int n_max) {
    return pd_dims_problem(dims) || B < 1 || B > 65535 || n_max < pd_min_samples(*dims) || n_max > GVX_HIFIGAN_MPD_MAX_SAMPLES;
}

int pd_check_call(const gvx_hifigan_mpd* h, const float* wav, const void* features, int B, int n_max) {
    if (const int rc = dc_check_call(h, wav, features, B)) return rc;
    if (n_max < pd_min_samples(h->d))
        return fail(GVX_ERR_INVALID_ARG, "n_max = %d: the largest period's reflection needs at least %d samples", n_max, pd_min_samples(h->d));
    if (n_max > GVX_HIFIGAN_MPD_MAX_SAMPLES) return fail(GVX_ERR_UNSUPPORTED, "n_max = %d is beyond the limit of %d samples", n_max, GVX_HIFIGAN_MPD_MAX_SAMPLES);
    return GVX_OK;
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
    PdLayer L[PD_MAX_MAPS];
    size_t per_period = 0;
    const int nl = pd_layers(*dims, L, &per_period);
    hipStream_t s = (hipStream_t)stream;
    return dc_pack_weights(table, n, dims->n_periods, L, nl, per_period, device_blob, s, [&](const PdLayer& l, const float* W, float* base) {
        pd_pack_kernel<<<(unsigned)((l.wn() + 255) / 256), 256, 0, s>>>(W, base + l.wf_off, base + l.wb_off, l.cout, l.cin, l.k);
    });
}

int gvx_hifigan_mpd_create(const gvx_hifigan_mpd_dims* dims, gvx_hifigan_mpd** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = pd_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_hifigan_mpd* h = new gvx_hifigan_mpd();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_hifigan_mpd_destroy(gvx_hifigan_mpd* h) { delete h; }

int gvx_hifigan_mpd_timing_enable(gvx_hifigan_mpd* h, int enable) { return dc_timing_enable(h, enable); }

int gvx_hifigan_mpd_layer_times_ms(gvx_hifigan_mpd* h, float* forward_ms, float* backward_ms, int* n_layers_out) {
    return dc_layer_times_ms(h, h ? h->d.n_periods : 0, h ? h->d.n_layers + 1 : 0, forward_ms, backward_ms, n_layers_out);
}

int gvx_hifigan_mpd_bind(gvx_hifigan_mpd* h, const float* device_blob) { return gen_bind(h, device_blob); }

int gvx_hifigan_mpd_forward(gvx_hifigan_mpd* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features,
                            size_t features_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = pd_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    const gvx_hifigan_mpd_dims& d = h->d;
    const PdFeat F = pd_feat_layout(d, B, n_max);
    if ((rc = dc_check_features(features, features_bytes, F.total)) != GVX_OK) return rc;
    if ((rc = gen_check_workspace(workspace, workspace_bytes, pd_ws_plan(d, B, n_max, false).total)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    PdLayer L[PD_MAX_MAPS];
    size_t per_period = 0;
    const int nl = pd_layers(d, L, &per_period);
    for (int j = 0; j < d.n_periods; ++j) {
        const float* in = wav;
        if ((rc = dc_mark(h, h->marks, (size_t)j * (nl + 1), s)) != GVX_OK) return rc;
        for (int i = 0; i < nl; ++i) {
            DcConv p = pd_conv(d, L[i], F, j, i, sample_lengths, n_max);
            p.src = in; p.W = h->blob + j * per_period + L[i].wf_off; p.bias = h->blob + j * per_period + L[i].b_off;
            p.out = gvx::ws_ptr<float>(features, F.off[j][i]);
            if ((rc = pd_launch_conv<false>(p, L[i].mfma != 0, B, s)) != GVX_OK) return rc;
            in = p.out;
            if ((rc = dc_mark(h, h->marks, (size_t)j * (nl + 1) + i + 1, s)) != GVX_OK) return rc;
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
    if ((rc = dc_check_backward(features, d_features, grads, n_grads, d_wav)) != GVX_OK) return rc;
    const gvx_hifigan_mpd_dims& d = h->d;
    const PdFeat F = pd_feat_layout(d, B, n_max);
    const PdWs wp = pd_ws_plan(d, B, n_max, true);
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    PdLayer L[PD_MAX_MAPS];
    size_t per_period = 0;
    const int nl = pd_layers(d, L, &per_period);
    DcParam g[DC_MAX_STACKS * DC_MAX_MAPS] = {};
    if ((rc = dc_find_grads(grads, n_grads, d.n_periods, L, nl, g)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    float* gbuf[2] = {gvx::ws_ptr<float>(workspace, wp.grad[0]), gvx::ws_ptr<float>(workspace, wp.grad[1])};
    float* parts = gvx::ws_ptr<float>(workspace, wp.parts);
    double* db_parts = gvx::ws_ptr<double>(workspace, wp.db_parts);
    auto feat = [&](const void* base, int j, int i) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + F.off[j][i]); };
    for (int j = 0; j < d.n_periods; ++j) {
        const float* blob = h->blob + j * per_period;
        const float* dcur = feat(d_features, j, nl - 1);   // the score has no activation: its cotangent is its pre-activation's
        if ((rc = dc_mark(h, h->bwd_marks, (size_t)j * (nl + 1) + nl, s)) != GVX_OK) return rc;
        for (int i = nl - 1; i >= 0; --i) {
            DcConv p = pd_conv(d, L[i], F, j, i, sample_lengths, n_max);
            if (n_grads > 0) {
                p.src = i == 0 ? wav : feat(features, j, i - 1);
                p.dy = dcur;
                const DcPieces P = pd_pieces(L[i], B, p.Lo_max * p.period);
                if (L[i].mfma)
                    pd_wgrad_mfma_kernel<<<dim3((unsigned)((p.NC + 63) / 64), (unsigned)((p.KC + 63) / 64), (unsigned)(P.n * p.k)), 256, 0, s>>>(
                        p, parts, B, P.chunks, P.rows_per_piece, P.run);
                else
                    dc_launch_wgrad_valu<true, true>(p, P, parts, B, s);
                if ((rc = dc_finish_param_grads<true, true>(p, P, parts, db_parts, g[j * nl + i], B, s)) != GVX_OK) return rc;
            }
            if (i > 0) {
                const DcConv q = dc_exchanged(p, dcur, blob + L[i].wb_off, feat(features, j, i - 1), feat(d_features, j, i - 1), gbuf[i & 1]);
                if ((rc = pd_launch_conv<true>(q, L[i].mfma != 0, B, s)) != GVX_OK) return rc;
                dcur = q.out;
            } else if (d_wav) {
                p.dy = dcur; p.W = blob + L[0].wf_off;
                pd_dwav_kernel<<<dim3((unsigned)((n_max + 255) / 256), (unsigned)B), 256, 0, s>>>(p, d_wav, j > 0);
                HIP_TRY(hipGetLastError());
            }
            if ((rc = dc_mark(h, h->bwd_marks, (size_t)j * (nl + 1) + i, s)) != GVX_OK) return rc;   // mark i: layer i is done
        }
    }
    h->bwd_timed = h->timing;
    return GVX_OK;
}

}  // C ABI
