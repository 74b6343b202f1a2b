// What the host side of csrc/melgan_disc.hip is built from: the layer table of one discriminator scale, the dims check, the row-length
// arithmetic that host and kernels share, and the layouts of the blob, the features buffer and the workspaces.  Host arithmetic only, so
// that a stand-alone program can check it without a device.
#pragma once
#include "../../include/genvox_amd.h"
#include "rounding.h"

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MD_HD __host__ __device__
#else
#define MD_HD
#endif

namespace gvx_md {

constexpr int MD_TILE = 64;         // positions per workgroup of the convolution kernels (GVX_MELGAN_DISC_TILE)
constexpr int MD_MAX_LAYERS = 9;    // n_layers + 3 with n_layers <= 6
constexpr int MD_PART_FLOATS = 1 << 24;   // the weight-gradient partials of one layer stay below this many floats where the rows allow it

struct MdLayer {
    int cin, cout, k, stride, pad, groups, cig, cog;
    int down_in, down_out;   // how many strided layers lie in front of the input / the output: their lengths follow from the row's own n
    int reflect, act;
    size_t w_off, b_off;     // floats, inside one scale's part of the blob
    size_t wn() const { return (size_t)cout * cig * k; }
};

// length after `down` strided layers of a row of n samples at this scale (0 stays 0: a refused row is silent)
MD_HD inline int md_chain(int n, int s, int down) {
    for (int i = 0; i < down && n > 0; ++i) n = (n - 1) / s + 1;
    return n;
}

inline int md_min_samples(const gvx_melgan_disc_dims& d) { return 8 << (d.n_scales - 1); }

inline const char* md_dims_problem(const gvx_melgan_disc_dims* d) {
    if (!d) return "null dims";
    if (d->n_scales < 1 || d->n_scales > GVX_MELGAN_DISC_MAX_SCALES) return "n_scales must be in [1, 4]";
    if (d->base_channels < 4 || d->base_channels % 4) return "base_channels must be a positive multiple of 4";
    if (d->n_layers < 1 || d->n_layers > 6) return "n_layers must be in [1, 6]";
    if (d->downsampling_factor < 1 || d->downsampling_factor > 8) return "downsampling_factor must be in [1, 8]";
    if (d->max_channels < 4 || d->max_channels > (1 << 16)) return "max_channels must be in [4, 65536]";
    if (!(d->slope >= 0.f && d->slope <= 1.f)) return "slope must be in [0, 1]";
    long c = d->base_channels;
    for (int i = 1; i <= d->n_layers; ++i) {
        if (c % 4) return "a grouped layer's input channels are no multiple of 4";
        long cn = c * d->downsampling_factor;
        if (cn > d->max_channels) cn = d->max_channels;
        if (cn % (c / 4)) return "a grouped layer's output channels are not divisible by its group count";
        c = cn;
    }
    return nullptr;
}

// the n_layers + 3 layers of one scale -> their count; w_off / b_off rounded to 64 floats; *floats_out: one scale's part of the blob
inline int md_layers(const gvx_melgan_disc_dims& d, MdLayer* L, size_t* floats_out = nullptr, size_t* params_out = nullptr) {
    const int s = d.downsampling_factor;
    size_t at = 0, params = 0;
    int n = 0;
    auto add = [&](int cin, int cout, int k, int stride, int pad, int groups, int down_in, int down_out, int reflect, int act) {
        MdLayer& l = L[n++];
        l = MdLayer{cin, cout, k, stride, pad, groups, cin / groups, cout / groups, down_in, down_out, reflect, act, 0, 0};
        l.w_off = at; at += gvx::round64(l.wn());
        l.b_off = at; at += gvx::round64((size_t)cout);
        params += l.wn() + cout;
    };
    int c = d.base_channels;
    add(1, c, 15, 1, 7, 1, 0, 0, 1, 1);
    for (int i = 1; i <= d.n_layers; ++i) {
        const int cn = (long)c * s > d.max_channels ? d.max_channels : c * s;
        add(c, cn, 10 * s + 1, s, 5 * s, c / 4, i - 1, i, 0, 1);
        c = cn;
    }
    const int c2 = 2L * c > d.max_channels ? d.max_channels : 2 * c;
    add(c, c2, 5, 1, 2, 1, d.n_layers, d.n_layers, 0, 1);
    add(c2, 1, 3, 1, 1, 1, d.n_layers, d.n_layers, 0, 0);
    if (floats_out) *floats_out = at;
    if (params_out) *params_out = params;
    return n;
}

struct MdFeat {   // the features buffer: map (scale, layer) is [B][channels][positions] at byte `off`
    size_t off[GVX_MELGAN_DISC_MAX_SCALES][MD_MAX_LAYERS];
    int channels[MD_MAX_LAYERS];
    int positions[GVX_MELGAN_DISC_MAX_SCALES][MD_MAX_LAYERS];
    int n_layers;
    size_t total;
};

inline MdFeat md_feat_layout(const gvx_melgan_disc_dims& d, int B, int n_max) {
    MdFeat F{};
    MdLayer L[MD_MAX_LAYERS];
    F.n_layers = md_layers(d, L);
    size_t at = 0;
    for (int k = 0; k < d.n_scales; ++k)
        for (int i = 0; i < F.n_layers; ++i) {
            F.channels[i] = L[i].cout;
            F.positions[k][i] = md_chain(n_max >> k, d.downsampling_factor, L[i].down_out);
            F.off[k][i] = at;
            at += gvx::round256((size_t)B * L[i].cout * F.positions[k][i] * sizeof(float));
        }
    F.total = at;
    return F;
}

// pieces of one layer's weight gradient: rows are dealt `rows_per_piece` to a piece, or a row is cut into `chunks` runs of positions
struct MdPieces { int chunks, rows_per_piece, n; size_t numel; };

inline MdPieces md_pieces(const MdLayer& l, int B, int positions) {
    MdPieces P{};
    P.numel = l.wn();
    const size_t out_blocks = (P.numel / ((l.cog % 4) ? 1 : 4) + 255) / 256;
    size_t want = (1024 + out_blocks - 1) / out_blocks;            // about 1024 workgroups per launch
    const size_t cap = MD_PART_FLOATS / P.numel ? MD_PART_FLOATS / P.numel : 1;
    if (want > cap) want = cap;
    if (want >= (size_t)B) {
        size_t chunks = (want + B - 1) / B, most = ((size_t)positions + 31) / 32;
        if (chunks > most) chunks = most;
        if (chunks < 1) chunks = 1;
        P.chunks = (int)chunks; P.rows_per_piece = 1; P.n = B * P.chunks;
    } else {
        P.chunks = 1; P.rows_per_piece = (int)((B + want - 1) / want); P.n = (B + P.rows_per_piece - 1) / P.rows_per_piece;
    }
    return P;
}

struct MdWs {   // byte offsets
    size_t pooled[GVX_MELGAN_DISC_MAX_SCALES];   // the waveform of scale k >= 1, [B][n_max >> k]
    size_t d_pooled[GVX_MELGAN_DISC_MAX_SCALES]; // its gradient (backward only)
    size_t grad[2];                              // two activation gradients, the layers alternate (backward only)
    size_t parts;                                // partial weight gradients (backward only)
    size_t total;
};

inline MdWs md_ws_plan(const gvx_melgan_disc_dims& d, int B, int n_max, bool backward) {
    MdWs W{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += gvx::round256(bytes); return o; };
    for (int k = 1; k < d.n_scales; ++k) W.pooled[k] = take((size_t)B * (n_max >> k) * sizeof(float));
    if (backward) {
        for (int k = 1; k < d.n_scales; ++k) W.d_pooled[k] = take((size_t)B * (n_max >> k) * sizeof(float));
        MdLayer L[MD_MAX_LAYERS];
        const int nl = md_layers(d, L);
        size_t act = 0, parts = 0;
        for (int k = 0; k < d.n_scales; ++k)
            for (int i = 0; i < nl; ++i) {
                const int pos = md_chain(n_max >> k, d.downsampling_factor, L[i].down_out);
                const size_t a = (size_t)B * L[i].cout * pos;
                if (i < nl - 1 && a > act) act = a;
                const MdPieces P = md_pieces(L[i], B, pos);
                if (P.n * P.numel > parts) parts = P.n * P.numel;
            }
        W.grad[0] = take(act * sizeof(float));
        W.grad[1] = take(act * sizeof(float));
        W.parts = take(parts * sizeof(float));
    }
    W.total = at < 256 ? 256 : at;
    return W;
}

}  // namespace gvx_md
