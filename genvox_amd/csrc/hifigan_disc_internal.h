// What the host side of csrc/hifigan_disc.hip is built from: the layer table of one period discriminator, the dims check, and the
// layouts of the blob, the features buffer and the backward's workspace; the height arithmetic that host and kernels share is
// disc_conv.h's.  Host arithmetic only, so that a stand-alone program can check it without a device.
#pragma once
#include "../../include/genvox_amd.h"
#include "disc_conv.h"

namespace gvx_pd {

using namespace gvx_dc;

// Tile constants (the public header repeats them as GVX_HIFIGAN_MPD_*): every convolution kernel - matrix or VALU, forward or data
// gradient - gives a workgroup PD_TILE positions (h, column) of one row; the data gradient's positions are those of ONE stride phase.
constexpr int PD_TILE = 64;        // positions per workgroup, every kernel family
constexpr int PD_TILE_N = 64;      // output channels per workgroup: the VALU kernels, and the matrix kernels below 128 output channels
constexpr int PD_TILE_N_WIDE = 128;   // output channels per workgroup of the matrix kernels from 128 output channels on
constexpr int PD_MFMA_MULT = 32;   // a layer runs on the matrix instruction when both channel counts are multiples of this
constexpr int PD_WG_CHUNK = 32;    // positions per k-step of the matrix weight-gradient kernel
constexpr int PD_MAX_MAPS = GVX_HIFIGAN_MPD_MAX_LAYERS + 1;
static_assert(PD_TILE == DC_TILE && PD_TILE_N == DC_TILE_N && PD_MAX_MAPS == DC_MAX_MAPS, "the shared kernels' constants");

struct PdLayer {
    int cin, cout, k, stride, pad;
    int act, mfma;
    size_t wf_off, wb_off, b_off;   // floats, inside one period's part of the blob: W as [cout][k][cin], as [cin][k][cout], the bias
    size_t wn() const { return (size_t)cout * cin * k; }
};

inline int pd_min_samples(const gvx_hifigan_mpd_dims& d) {
    int m = 1;
    for (int j = 0; j < d.n_periods; ++j) m = d.periods[j] > m ? d.periods[j] : m;
    return m;
}

inline const char* pd_dims_problem(const gvx_hifigan_mpd_dims* d) {
    if (!d) return "null dims";
    if (d->n_periods < 1 || d->n_periods > GVX_HIFIGAN_MPD_MAX_PERIODS) return "n_periods must be in [1, 8]";
    for (int j = 0; j < d->n_periods; ++j)
        if (d->periods[j] < 1 || d->periods[j] > GVX_HIFIGAN_MPD_MAX_PERIOD) return "a period must be in [1, 64]";
    if (d->n_layers < 2 || d->n_layers > GVX_HIFIGAN_MPD_MAX_LAYERS) return "n_layers must be in [2, 8]";
    for (int i = 0; i < d->n_layers; ++i) {
        const int c = d->channels[i];
        if (c < 1 || c > 4096) return "a channel count must be in [1, 4096]";
        if (c > 64 && c % PD_MFMA_MULT) return "a channel count above 64 must be a multiple of 32 (the matrix kernels' k-tile)";
    }
    if (d->kernel_size < 1 || d->kernel_size > 15 || d->kernel_size % 2 == 0) return "kernel_size must be odd and in [1, 15]";
    if (d->stride < 1 || d->stride > 8) return "stride must be in [1, 8]";
    if (!(d->slope >= 0.f && d->slope <= 1.f)) return "slope must be in [0, 1]";
    return nullptr;
}

// the n_layers convolutions and the score of one period -> their count; *floats_out: one period's part of the blob
inline int pd_layers(const gvx_hifigan_mpd_dims& d, PdLayer* L, size_t* floats_out = nullptr, size_t* params_out = nullptr) {
    size_t at = 0, params = 0;
    int n = 0, cin = 1;
    auto add = [&](int ci, int co, int k, int stride, int act) {
        PdLayer& l = L[n++];
        l = PdLayer{ci, co, k, stride, k / 2, act, (ci % PD_MFMA_MULT == 0 && co % PD_MFMA_MULT == 0) ? 1 : 0, 0, 0, 0};
        l.wf_off = at; at += gvx::round64(l.wn());
        l.wb_off = at; at += gvx::round64(l.wn());
        l.b_off = at; at += gvx::round64((size_t)co);
        params += l.wn() + co;
    };
    for (int i = 0; i < d.n_layers; ++i) {
        add(cin, d.channels[i], d.kernel_size, i == d.n_layers - 1 ? 1 : d.stride, 1);   // the last convolution keeps the height
        cin = d.channels[i];
    }
    add(cin, 1, 3, 1, 0);
    if (floats_out) *floats_out = at;
    if (params_out) *params_out = params;
    return n;
}

// the strides in front of map i's height: those of layers 0 .. i
inline void pd_strides(const gvx_hifigan_mpd_dims& d, int* str) {
    for (int i = 0; i < PD_MAX_MAPS; ++i) str[i] = i < d.n_layers - 1 ? d.stride : 1;
}

struct PdFeat {   // the features buffer: map (period j, layer i) is [B][height][period][channels] at byte `off`
    size_t off[GVX_HIFIGAN_MPD_MAX_PERIODS][PD_MAX_MAPS];
    int channels[PD_MAX_MAPS];
    int height[GVX_HIFIGAN_MPD_MAX_PERIODS][PD_MAX_MAPS];
    int n_maps;
    size_t total;
};

inline PdFeat pd_feat_layout(const gvx_hifigan_mpd_dims& d, int B, int n_max) {
    PdFeat F{};
    PdLayer L[PD_MAX_MAPS];
    int str[PD_MAX_MAPS];
    F.n_maps = pd_layers(d, L);
    pd_strides(d, str);
    size_t at = 0;
    for (int j = 0; j < d.n_periods; ++j)
        for (int i = 0; i < F.n_maps; ++i) {
            F.channels[i] = L[i].cout;
            F.height[j][i] = dc_length(n_max, d.periods[j], str, i + 1);
            F.off[j][i] = at;
            at += gvx::round256((size_t)B * F.height[j][i] * d.periods[j] * L[i].cout * sizeof(float));
        }
    F.total = at;
    return F;
}

// the pieces of one layer's weight gradient
inline DcPieces pd_pieces(const PdLayer& l, int B, int positions) {
    DcPieces P{};
    P.numel = l.wn();
    const size_t out_blocks = l.mfma ? (size_t)((l.cout + 63) / 64) * ((l.cin + 63) / 64) * l.k : (P.numel + 255) / 256;
    // about 1024 workgroups per launch; the VALU kernel walks its run one position at a time, so it gets four times as many, shorter runs
    const size_t target = l.mfma ? 1024 : 4096, shortest = l.mfma ? 4 * PD_WG_CHUNK : PD_WG_CHUNK;
    size_t want = (target + out_blocks - 1) / out_blocks;
    const size_t cap = DC_PART_FLOATS / P.numel ? DC_PART_FLOATS / P.numel : 1;
    if (want > cap) want = cap;
    if (want >= (size_t)B) {
        size_t chunks = (want + B - 1) / B, most = ((size_t)positions + shortest - 1) / shortest;
        if (chunks > most) chunks = most;
        if (chunks < 1) chunks = 1;
        P.chunks = (int)chunks; P.rows_per_piece = 1; P.n = B * P.chunks;
    } else {
        P.chunks = 1; P.rows_per_piece = (int)((B + want - 1) / want); P.n = (B + P.rows_per_piece - 1) / P.rows_per_piece;
    }
    P.run = (positions + P.chunks - 1) / P.chunks;
    P.run = (P.run + PD_WG_CHUNK - 1) / PD_WG_CHUNK * PD_WG_CHUNK;
    return P;
}

struct PdWs : DcWs { size_t total; };   // byte offsets (backward only; the forward needs no scratch)

inline PdWs pd_ws_plan(const gvx_hifigan_mpd_dims& d, int B, int n_max, bool backward) {
    PdWs W{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += gvx::round256(bytes); return o; };
    if (backward) {
        PdLayer L[PD_MAX_MAPS];
        const int nl = pd_layers(d, L);
        const PdFeat F = pd_feat_layout(d, B, n_max);
        DcWsNeed need;
        for (int j = 0; j < d.n_periods; ++j)
            for (int i = 0; i < nl; ++i) {
                const int pos = F.height[j][i] * d.periods[j];
                need.layer(B, L[i].cout, pos, i == nl - 1, pd_pieces(L[i], B, pos));
            }
        static_cast<DcWs&>(W) = need.place(take);
    }
    W.total = at < 256 ? 256 : at;
    return W;
}

}  // namespace gvx_pd
