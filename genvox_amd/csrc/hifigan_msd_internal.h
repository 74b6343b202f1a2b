// What the host side of csrc/hifigan_msd.hip is built from: the layer table of one scale discriminator, the dims check, and the
// layouts of the blob, the features buffer and the workspaces; the length arithmetic that host and kernels share is disc_conv.h's.
// Host arithmetic only, so that a stand-alone program can check it without a device.
#pragma once
#include "../../include/genvox_amd.h"
#include "disc_conv.h"

namespace gvx_sd {

using namespace gvx_dc;

// Tile constants (the public header repeats them as GVX_HIFIGAN_MSD_*)
constexpr int SD_TILE = 64;          // positions per workgroup, every convolution kernel; a data gradient's are those of ONE stride phase
constexpr int SD_MFMA_IN = 8;        // a layer runs on the matrix instruction when its per-group input channels are a multiple of this
constexpr int SD_MFMA_OUT = 16;      // ... and its per-group output channels a multiple of this
constexpr int SD_WG_RUN = 256;       // positions per piece of a weight gradient where a row is cut into runs
constexpr int SD_WG_ALIGN = 32;      // a longer run (the partials' cap) is a multiple of this
constexpr int SD_MAX_MAPS = GVX_HIFIGAN_MSD_MAX_LAYERS + 1;
constexpr int SD_MAX_PIECES = 32768;
constexpr int SD_WIN_BYTES = 48 * 1024;   // the LDS window of the matrix kernels stays below this
static_assert(SD_TILE == DC_TILE && SD_MAX_MAPS == DC_MAX_MAPS, "the shared kernels' constants");

struct SdLayer {
    int cin, cout, k, stride, pad, groups;
    int act, mfma;           // mfma: 0 VALU, 32 the 32x32x2 instruction, 16 the 16x16x4 instruction
    size_t wf_off, wb_off, b_off;   // floats, inside one scale's part of the blob
    size_t wn() const { return (size_t)cout * (cin / groups) * k; }
};

inline const char* sd_dims_problem(const gvx_hifigan_msd_dims* d) {
    if (!d) return "null dims";
    if (d->n_scales < 1 || d->n_scales > GVX_HIFIGAN_MSD_MAX_SCALES) return "n_scales must be in [1, 4]";
    if (d->n_layers < 2 || d->n_layers > GVX_HIFIGAN_MSD_MAX_LAYERS) return "n_layers must be in [2, 8]";
    int cin = 1;
    for (int i = 0; i < d->n_layers; ++i) {
        const int c = d->channels[i], k = d->kernel_sizes[i], g = d->groups[i];
        if (c < 1 || c > 4096) return "a channel count must be in [1, 4096]";
        if (k < 1 || k > GVX_HIFIGAN_MSD_MAX_KERNEL || k % 2 == 0) return "a kernel size must be odd and in [1, 41]";
        if (d->strides[i] < 1 || d->strides[i] > 8) return "a stride must be in [1, 8]";
        if (g < 1 || cin % g || c % g) return "a group count must be at least 1 and divide both channel counts of its layer";
        cin = c;
    }
    if (!(d->slope >= 0.f && d->slope <= 1.f)) return "slope must be in [0, 1]";
    return nullptr;
}

inline int sd_mfma_kind(int cin_g, int cout_g) {
    if (cin_g % SD_MFMA_IN || cout_g % SD_MFMA_OUT) return 0;
    return (cin_g % 32 == 0 && cout_g % 32 == 0) ? 32 : 16;
}

// the n_layers convolutions and the score of one scale -> their count; *floats_out: one scale's part of the blob
inline int sd_layers(const gvx_hifigan_msd_dims& d, SdLayer* L, size_t* floats_out = nullptr, size_t* params_out = nullptr) {
    size_t at = 0, params = 0;
    int n = 0, cin = 1;
    auto add = [&](int ci, int co, int k, int stride, int groups, int act) {
        SdLayer& l = L[n++];
        l = SdLayer{ci, co, k, stride, k / 2, groups, act, sd_mfma_kind(ci / groups, co / groups), 0, 0, 0};
        l.wf_off = at; at += gvx::round64(l.wn());
        l.wb_off = at; at += gvx::round64(l.wn());
        l.b_off = at; at += gvx::round64((size_t)co);
        params += l.wn() + co;
    };
    for (int i = 0; i < d.n_layers; ++i) {
        add(cin, d.channels[i], d.kernel_sizes[i], d.strides[i], d.groups[i], 1);
        cin = d.channels[i];
    }
    add(cin, 1, 3, 1, 1, 0);
    if (floats_out) *floats_out = at;
    if (params_out) *params_out = params;
    return n;
}

// the strides in front of map i's length: those of layers 0 .. i (the score has stride 1)
inline void sd_strides(const gvx_hifigan_msd_dims& d, int* str) {
    for (int i = 0; i < SD_MAX_MAPS; ++i) str[i] = i < d.n_layers ? d.strides[i] : 1;
}

struct SdFeat {   // the features buffer: map (scale s, layer i) is [B][length][channels] at byte `off`
    size_t off[GVX_HIFIGAN_MSD_MAX_SCALES][SD_MAX_MAPS];
    int channels[SD_MAX_MAPS];
    int length[GVX_HIFIGAN_MSD_MAX_SCALES][SD_MAX_MAPS];
    int n_scale[GVX_HIFIGAN_MSD_MAX_SCALES];   // samples of a row of n_max at every scale
    int n_maps;
    size_t total;
};

inline SdFeat sd_feat_layout(const gvx_hifigan_msd_dims& d, int B, int n_max) {
    SdFeat F{};
    SdLayer L[SD_MAX_MAPS];
    int str[SD_MAX_MAPS];
    F.n_maps = sd_layers(d, L);
    sd_strides(d, str);
    size_t at = 0;
    for (int s = 0; s < d.n_scales; ++s) {
        F.n_scale[s] = dc_samples(n_max, 1, s);
        for (int i = 0; i < F.n_maps; ++i) {
            F.channels[i] = L[i].cout;
            F.length[s][i] = dc_length(F.n_scale[s], 1, str, i + 1);
            F.off[s][i] = at;
            at += gvx::round256((size_t)B * F.length[s][i] * L[i].cout * sizeof(float));
        }
    }
    F.total = at;
    return F;
}

// the pieces of one layer's weight gradient
inline DcPieces sd_pieces(const SdLayer& l, int B, int positions) {
    DcPieces P{};
    P.numel = l.wn();
    size_t cap = DC_PART_FLOATS / P.numel ? DC_PART_FLOATS / P.numel : 1;
    if (cap > (size_t)SD_MAX_PIECES) cap = SD_MAX_PIECES;
    if (cap >= (size_t)B) {
        const size_t most = cap / B, want = ((size_t)positions + SD_WG_RUN - 1) / SD_WG_RUN;
        P.rows_per_piece = 1;
        if (want <= most) {   // the usual case: runs of SD_WG_RUN positions
            P.chunks = want < 1 ? 1 : (int)want;
            P.run = SD_WG_RUN;
        } else {
            P.chunks = (int)most;
            P.run = (positions + P.chunks - 1) / P.chunks;
            P.run = (P.run + SD_WG_ALIGN - 1) / SD_WG_ALIGN * SD_WG_ALIGN;
        }
        P.n = B * P.chunks;
    } else {
        P.chunks = 1;
        P.rows_per_piece = (int)((B + cap - 1) / cap);
        P.n = (B + P.rows_per_piece - 1) / P.rows_per_piece;
        P.run = positions > 0 ? positions : 1;
    }
    return P;
}

// channel block and rows of the matrix kernels' LDS window: the K-side per-group channels kg (a multiple of 8) in blocks of the largest
// of 64, 32, 16, 8 that divides kg and keeps the window below SD_WIN_BYTES
struct SdWin { int cb, rows; size_t bytes; };

inline SdWin sd_window(int kg, int k, int stride, bool backward) {
    SdWin w{};
    w.rows = backward ? SD_TILE + (k + stride - 1) / stride - 1 : (SD_TILE - 1) * stride + k;
    for (int cb = 64; cb >= 8; cb >>= 1) {
        if (kg % cb) continue;
        w.cb = cb;
        w.bytes = (size_t)w.rows * (cb + 1) * sizeof(float);
        if (w.bytes <= (size_t)SD_WIN_BYTES) break;
    }
    return w;
}

struct SdWs : DcWs {   // byte offsets
    size_t pooled[GVX_HIFIGAN_MSD_MAX_SCALES];   // the waveform of scales 1 .., [B][n_scale]
    size_t dpool[GVX_HIFIGAN_MSD_MAX_SCALES];    // backward: the waveform gradient of scales 1 ..
    size_t total;
};

inline SdWs sd_ws_plan(const gvx_hifigan_msd_dims& d, int B, int n_max, bool backward) {
    SdWs W{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += gvx::round256(bytes); return o; };
    const SdFeat F = sd_feat_layout(d, B, n_max);
    for (int s = 1; s < d.n_scales; ++s) W.pooled[s] = take((size_t)B * F.n_scale[s] * sizeof(float));
    if (backward) {
        for (int s = 1; s < d.n_scales; ++s) W.dpool[s] = take((size_t)B * F.n_scale[s] * sizeof(float));
        SdLayer L[SD_MAX_MAPS];
        const int nl = sd_layers(d, L);
        DcWsNeed need;
        for (int s = 0; s < d.n_scales; ++s)
            for (int i = 0; i < nl; ++i) need.layer(B, L[i].cout, F.length[s][i], i == nl - 1, sd_pieces(L[i], B, F.length[s][i]));
        static_cast<DcWs&>(W) = need.place(take);
    }
    W.total = at < 256 ? 256 : at;
    return W;
}

}  // namespace gvx_sd
