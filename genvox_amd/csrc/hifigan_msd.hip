// HiFi-GAN scale discriminators (include/genvox_amd.h, "HiFi-GAN scale discriminators"): forward, and the backward that reads the
// forward's own maps as its tape.  Maps are channels-last, [B][length][channels]: a group's channels are contiguous at a position, which
// is what an implicit GEMM with positions on M and taps x group channels on K wants.  The waveform of a scale is such a map of 1 channel.
//
// The tiles, the tap walk by stride phase, the VALU kernels (the first layer, the score, narrow layers), the piece reduction and the
// bias gradient are the shared core's (disc_conv.h, its 1-D form; disc_host.h).  What is here:
//   sd_mfma_kernel    the grouped and the dense layers, forward (BWD = false) and data gradient (BWD = true): 64 positions x 16, 32 or 64
//                      channels of one group.  The window of the operand that the tile's taps touch - (SD_TILE - 1) * stride + k rows
//                      of a block of the group's channels, zeros outside the row - is staged into LDS once per channel block, and every
//                      tap runs off a row offset in it; the weights come as [group][tap][k channel][n channel], a coalesced read per
//                      fragment.  MF = 32: v_mfma_f32_32x32x2_f32, two waves on M; MF = 16: v_mfma_f32_16x16x4_f32, four waves on M.
//                      Eight taps are summed apart and then added, so the products never form one chain.
//   sd_wgrad_mfma_kernel   one piece (rows, or a run of positions of one row) of a weight gradient in PyTorch's layout, as the VALU
//                      pieces of this discriminator are: a per-group GEMM with positions on K, a wave per tap.
//   sd_pool_kernel    AvgPool1d(4, 2, 2) of a row at its own length; sd_dwav_kernel the first layer's data gradient plus the pooling's
//                      adjoint of the next scale's waveform gradient, both as gathers, the channels in the lanes of a wave.
// No atomics anywhere: two calls give the same bits.
#include "disc_host.h"
#include "hifigan_msd_internal.h"

using gvx::fail;
using namespace gvx_sd;

static_assert(SD_TILE == GVX_HIFIGAN_MSD_TILE && SD_MFMA_IN == GVX_HIFIGAN_MSD_MFMA_IN_MULT && SD_MFMA_OUT == GVX_HIFIGAN_MSD_MFMA_OUT_MULT &&
                  SD_WG_RUN == GVX_HIFIGAN_MSD_WG_RUN,
              "the public header states the tile constants");
static_assert(GVX_HIFIGAN_MSD_MAX_SCALES <= DC_MAX_STACKS, "a scale is a stack of the shared host side");

struct gvx_hifigan_msd : DcHandle {
    gvx_hifigan_msd_dims d;
};

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

// MF x MF tiles of the matrix instruction: 64 / MF waves on M, WN waves on N
template <bool BWD, int MF, int WN>
__global__ void __launch_bounds__(64 * (64 / MF) * WN) sd_mfma_kernel(const DcConv p) {
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
    const int ns = dc_row_n(p, b);
    const int Ls = dc_len<false>(p, ns, p.n_src), Lo = dc_len<false>(p, ns, p.n_out);
    const int first = BWD ? m0 * p.stride + ph : m0;
    if (first >= Lo) {
        const int c0 = nt * NT;
        dc_zero_tile<false, BWD>(p, b, m0, ph, g * p.NG + c0, min(NT, p.NG - c0));
        return;
    }
    const DcTaps tp = dc_taps<BWD>(p, ph);
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
        dc_finish<false, BWD>(p, b, BWD ? m * p.stride + ph : m, 0, g * p.NG + n_l, Lo, acc[e]);
    }
}

// one piece of dW[n][c][t] = sum over positions l of dY[l][n] X[l * stride + t - pad][c] inside a group: an MF x MF tile (n on M, c on
// N) of one tap per wave, positions on k; both operands are read as they lie, a position's channels being contiguous
template <int MF>
__global__ void __launch_bounds__(256) sd_wgrad_mfma_kernel(const DcConv p, float* parts, int B, int chunks, int rows_per_piece, int run) {
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
    const DcSpan sp = dc_span(piece, B, chunks, rows_per_piece);
    const int n = g * p.NG + ntile * MF + r, c_l = ct * MF + r;
    const bool c_ok = c_l < p.KG;
    const int c = g * p.KG + (c_ok ? c_l : 0);
    acc_t acc, part;
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] = 0.f, part[e] = 0.f;
    int since = 0;
    for (int b = sp.b0; b < sp.b1; ++b) {
        const int ns = dc_row_n(p, b);
        const int Ls = dc_len<false>(p, ns, p.n_src), Lo = dc_len<false>(p, ns, p.n_out);
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

// the waveform of scale s + 1 from that of scale s (rows [B][n_in_max] -> [B][n_out_max]): y[j] = (the sum of x[2j - 2 .. 2j + 1]
// inside the row) / 4 for j = 0 .. n / 2, zeros behind
__global__ void __launch_bounds__(256) sd_pool_kernel(const float* in, float* out, const int32_t* lens, int n_max, int s, int n_in_max, int n_out_max) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_out_max) return;
    int n = lens ? lens[b] : n_max;
    n = dc_samples(n > n_max ? n_max : n, 1, s);
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
__global__ void __launch_bounds__(256) sd_dwav_kernel(const DcConv p, const float* next, int n_next_max, float* out) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i0 = ((int)blockIdx.x * 4 + wave) * SD_DWAV_RUN, i1 = min(i0 + SD_DWAV_RUN, p.Ls_max);
    const int ns = dc_row_n(p, b);
    const int Lo = dc_len<false>(p, ns, p.n_out);
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

DcConv sd_conv(const gvx_hifigan_msd_dims& d, const SdLayer& l, const SdFeat& F, int s, int i, const int32_t* lens, int n_max) {
    DcConv p{};
    p.lens = lens; p.n_max = n_max; p.min_n = 1; p.scale = s; p.period = 1;
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
void sd_launch_mfma(const DcConv& p, unsigned tiles, int phases, int B, size_t lds, hipStream_t s) {
    constexpr int NT = MF * WN, THREADS = 64 * (64 / MF) * WN;
    const int n_tiles = (p.NG + NT - 1) / NT, groups = p.NC / p.NG;
    sd_mfma_kernel<BWD, MF, WN><<<dim3(tiles, (unsigned)(n_tiles * groups * phases), (unsigned)B), THREADS, lds, s>>>(p);
}

// forward of layer (s, i), or with BWD its data gradient: there `q` already has the two sides exchanged
template <bool BWD>
int sd_launch_conv(const DcConv& q, int mfma, int B, hipStream_t s) {
    DcConv p = q;
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
        dc_launch_valu<false, BWD>(p, tiles, phases, B, s);
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

bool sd_bad_shape(const gvx_hifigan_msd_dims* dims, int B, int n_max) {
    return sd_dims_problem(dims) || B < 1 || B > 65535 || n_max < 1 || n_max > GVX_HIFIGAN_MSD_MAX_SAMPLES;
}

int sd_check_call(const gvx_hifigan_msd* h, const float* wav, const void* features, int B, int n_max) {
    if (const int rc = dc_check_call(h, wav, features, B)) return rc;
    if (n_max < 1) return fail(GVX_ERR_INVALID_ARG, "n_max = %d: a row needs at least 1 sample", n_max);
    if (n_max > GVX_HIFIGAN_MSD_MAX_SAMPLES) return fail(GVX_ERR_UNSUPPORTED, "n_max = %d is beyond the limit of %d samples", n_max, GVX_HIFIGAN_MSD_MAX_SAMPLES);
    return GVX_OK;
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
    SdLayer L[SD_MAX_MAPS];
    size_t per_scale = 0;
    const int nl = sd_layers(*dims, L, &per_scale);
    hipStream_t s = (hipStream_t)stream;
    return dc_pack_weights(table, n, dims->n_scales, L, nl, per_scale, device_blob, s, [&](const SdLayer& l, const float* W, float* base) {
        sd_pack_kernel<<<(unsigned)((l.wn() + 255) / 256), 256, 0, s>>>(W, base + l.wf_off, base + l.wb_off, l.cout, l.cin / l.groups,
                                                                         l.cout / l.groups, l.k, l.mfma);
    });
}

int gvx_hifigan_msd_create(const gvx_hifigan_msd_dims* dims, gvx_hifigan_msd** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = sd_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_hifigan_msd* h = new gvx_hifigan_msd();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_hifigan_msd_destroy(gvx_hifigan_msd* h) { delete h; }

int gvx_hifigan_msd_timing_enable(gvx_hifigan_msd* h, int enable) { return dc_timing_enable(h, enable); }

int gvx_hifigan_msd_layer_times_ms(gvx_hifigan_msd* h, float* forward_ms, float* backward_ms, int* n_layers_out) {
    return dc_layer_times_ms(h, h ? h->d.n_scales : 0, h ? h->d.n_layers + 1 : 0, forward_ms, backward_ms, n_layers_out);
}

int gvx_hifigan_msd_bind(gvx_hifigan_msd* h, const float* device_blob) { return gen_bind(h, device_blob); }

int gvx_hifigan_msd_forward(gvx_hifigan_msd* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features,
                            size_t features_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = sd_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    const gvx_hifigan_msd_dims& d = h->d;
    const SdFeat F = sd_feat_layout(d, B, n_max);
    if ((rc = dc_check_features(features, features_bytes, F.total)) != GVX_OK) return rc;
    const SdWs wp = sd_ws_plan(d, B, n_max, false);
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    SdLayer L[SD_MAX_MAPS];
    size_t per_scale = 0;
    const int nl = sd_layers(d, L, &per_scale);
    if ((rc = sd_pool_all(d, F, wp, wav, sample_lengths, B, n_max, workspace, s)) != GVX_OK) return rc;
    for (int sc = 0; sc < d.n_scales; ++sc) {
        const float* in = sc == 0 ? wav : gvx::ws_ptr<float>(workspace, wp.pooled[sc]);
        if ((rc = dc_mark(h, h->marks, (size_t)sc * (nl + 1), s)) != GVX_OK) return rc;
        for (int i = 0; i < nl; ++i) {
            DcConv p = sd_conv(d, L[i], F, sc, i, sample_lengths, n_max);
            p.src = in; p.W = h->blob + sc * per_scale + L[i].wf_off; p.bias = h->blob + sc * per_scale + L[i].b_off;
            p.out = gvx::ws_ptr<float>(features, F.off[sc][i]);
            if ((rc = sd_launch_conv<false>(p, L[i].mfma, B, s)) != GVX_OK) return rc;
            in = p.out;
            if ((rc = dc_mark(h, h->marks, (size_t)sc * (nl + 1) + i + 1, s)) != GVX_OK) return rc;
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
    if ((rc = dc_check_backward(features, d_features, grads, n_grads, d_wav)) != GVX_OK) return rc;
    const gvx_hifigan_msd_dims& d = h->d;
    const SdFeat F = sd_feat_layout(d, B, n_max);
    const SdWs wp = sd_ws_plan(d, B, n_max, true);
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    SdLayer L[SD_MAX_MAPS];
    size_t per_scale = 0;
    const int nl = sd_layers(d, L, &per_scale);
    DcParam g[DC_MAX_STACKS * DC_MAX_MAPS] = {};
    if ((rc = dc_find_grads(grads, n_grads, d.n_scales, L, nl, g)) != GVX_OK) return rc;
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
        if ((rc = dc_mark(h, h->bwd_marks, (size_t)sc * (nl + 1) + nl, s)) != GVX_OK) return rc;
        for (int i = nl - 1; i >= 0; --i) {
            DcConv p = sd_conv(d, L[i], F, sc, i, sample_lengths, n_max);
            if (n_grads > 0) {
                p.src = i == 0 ? wav_s : feat(features, sc, i - 1);
                p.dy = dcur;
                const DcPieces P = sd_pieces(L[i], B, p.Lo_max);
                if (L[i].mfma) {
                    const int MF = L[i].mfma;
                    const dim3 grid((unsigned)(L[i].groups * (p.NG / MF) * ((p.KG + MF - 1) / MF)), (unsigned)((p.k + 3) / 4), (unsigned)P.n);
                    if (MF == 32) sd_wgrad_mfma_kernel<32><<<grid, 256, 0, s>>>(p, parts, B, P.chunks, P.rows_per_piece, P.run);
                    else sd_wgrad_mfma_kernel<16><<<grid, 256, 0, s>>>(p, parts, B, P.chunks, P.rows_per_piece, P.run);
                } else {
                    dc_launch_wgrad_valu<false, false>(p, P, parts, B, s);
                }
                if ((rc = dc_finish_param_grads<false, false>(p, P, parts, db_parts, g[sc * nl + i], B, s)) != GVX_OK) return rc;
            }
            if (i > 0) {
                const DcConv q = dc_exchanged(p, dcur, blob + L[i].wb_off, feat(features, sc, i - 1), feat(d_features, sc, i - 1), gbuf[i & 1]);
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
            if ((rc = dc_mark(h, h->bwd_marks, (size_t)sc * (nl + 1) + i, s)) != GVX_OK) return rc;   // mark i: layer i is done
        }
    }
    h->bwd_timed = h->timing;
    return GVX_OK;
}

}  // C ABI
