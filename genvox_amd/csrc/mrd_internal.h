// What the host side of csrc/mrd.hip is built from: the frame and width rules that host and kernels share, the layer table of one
// resolution's sub-discriminator, the dims check, and the layouts of the blob, the features buffer and the workspace.  Host arithmetic
// only, so that a stand-alone program can check it without a device.
#pragma once
#include "../../include/genvox_amd.h"
#include "disc_conv.h"

namespace gvx_mr {

using namespace gvx_dc;

// Tile constants (the public header repeats them as GVX_MRD_*).  A position is a cell (frame w, bin f) of a map, numbered w * F + f
constexpr int MR_TILE = 64;           // positions per workgroup of the VALU kernels, and of the matrix kernels where c_out % 64 == 0
constexpr int MR_TILE_NARROW = 128;   // positions per workgroup of the matrix kernels otherwise (their tile is 128 x 32 channels)
constexpr int MR_PIECE_FRAMES = 16;   // output frames of one row that one piece of a weight gradient sums
constexpr int MR_WG_CHUNK = 64;       // positions per k-step of the matrix weight-gradient kernel, 16 to each wave
constexpr int MR_WG_VALU_SPLIT = 16;  // bin classes (f mod 16) that a piece of a VALU weight gradient is dealt into, four to a workgroup
constexpr int MR_FRAMES_PER_WG = 4;   // frames (waves) per workgroup of the spectrogram kernels
constexpr int MR_MAPS = 6;            // five convolutions and the score
constexpr int MR_KF = 3;              // frequency taps of every convolution

// frames of a row of n samples: reflection by p = (n_fft - hop) / 2 at both ends (needs n > p), no centring
DC_HD inline int mr_frames(int n, int n_fft, int hop) {
    const int p = (n_fft - hop) / 2;
    if (n <= p || n + 2 * p < n_fft) return 0;
    return 1 + (n + 2 * p - n_fft) / hop;
}

DC_HD inline int mr_stride(int layer) { return layer >= 1 && layer <= 3 ? 2 : 1; }

// frames of the row after `count` of the layers (count = 0: the spectrogram; map i: count = i + 1)
DC_HD inline int mr_width(int n, int n_fft, int hop, int count) {
    int w = mr_frames(n, n_fft, hop);
    for (int i = 0; i < count; ++i)
        if (w > 0) w = (w - 1) / mr_stride(i) + 1;
    return w;
}

struct MrLayer {
    int cin, cout, kt, stride, padt;   // kt taps along time, MR_KF along frequency
    int act, mfma;
    size_t wf_off, wb_off, b_off;      // floats inside one resolution's part of the blob: W as [cout][kt][3][cin], as [cin][kt][3 flipped][cout], bias
    size_t wn() const { return (size_t)cout * cin * kt * MR_KF; }
};

inline int mr_min_samples(const gvx_mrd_dims& d) {
    int m = 1;
    for (int r = 0; r < d.n_resolutions; ++r) {
        const int v = (d.n_fft[r] - d.hop[r]) / 2 + 1;
        m = v > m ? v : m;
    }
    return m;
}

inline const char* mr_dims_problem(const gvx_mrd_dims* d) {
    if (!d) return "null dims";
    if (d->n_resolutions < 1 || d->n_resolutions > GVX_MRD_MAX_RESOLUTIONS) return "n_resolutions must be in [1, 8]";
    for (int r = 0; r < d->n_resolutions; ++r) {
        if (d->n_fft[r] != 512 && d->n_fft[r] != 1024 && d->n_fft[r] != 2048) return "n_fft must be 512, 1024 or 2048";
        if (d->hop[r] < 1 || d->hop[r] > d->win[r] || d->win[r] > d->n_fft[r]) return "a resolution needs 1 <= hop <= win <= n_fft";
    }
    if (d->channels < 32 || d->channels > 128 || d->channels % 32) return "channels must be a multiple of 32 in [32, 128]";
    if (d->window != GVX_MRD_WINDOW_RECTANGULAR && d->window != GVX_MRD_WINDOW_HANN) return "window must be rectangular or hann";
    if (!(d->slope >= 0.f && d->slope <= 1.f)) return "slope must be in [0, 1]";
    return nullptr;
}

// the five convolutions and the score of one resolution; *floats_out: one resolution's part of the blob
inline int mr_layers(const gvx_mrd_dims& d, MrLayer* L, size_t* floats_out = nullptr) {
    size_t at = 0;
    const int C = d.channels;
    for (int i = 0; i < MR_MAPS; ++i) {
        MrLayer& l = L[i];
        const int kt = i < 4 ? 9 : 3;
        l = MrLayer{i == 0 ? 1 : C, i == MR_MAPS - 1 ? 1 : C, kt, mr_stride(i), kt / 2, i < MR_MAPS - 1, i > 0 && i < MR_MAPS - 1, 0, 0, 0};
        l.wf_off = at; at += gvx::round64(l.wn());
        l.wb_off = at; at += gvx::round64(l.wn());
        l.b_off = at; at += gvx::round64((size_t)l.cout);
    }
    if (floats_out) *floats_out = at;
    return MR_MAPS;
}

// behind the resolutions' weights the blob holds, per resolution, the padded window [n_fft], w_H^m [H] and w_N^k [H + 1] as float2
struct MrTables { size_t win, tw, tw2; };
inline size_t mr_table_floats(int n_fft) { return gvx::round64((size_t)n_fft) + gvx::round64((size_t)n_fft) + gvx::round64((size_t)n_fft + 2); }
inline MrTables mr_tables(const gvx_mrd_dims& d, size_t per_res, int r) {
    size_t at = per_res * d.n_resolutions;
    for (int q = 0; q < r; ++q) at += mr_table_floats(d.n_fft[q]);
    MrTables T{};
    T.win = at; at += gvx::round64((size_t)d.n_fft[r]);
    T.tw = at; at += gvx::round64((size_t)d.n_fft[r]);
    T.tw2 = at;
    return T;
}
inline size_t mr_blob_floats(const gvx_mrd_dims& d) {
    MrLayer L[MR_MAPS];
    size_t per_res = 0;
    mr_layers(d, L, &per_res);
    size_t at = per_res * d.n_resolutions;
    for (int r = 0; r < d.n_resolutions; ++r) at += mr_table_floats(d.n_fft[r]);
    return at;
}

// B, n_max and the largest map of every resolution are within what the kernels index with int
inline bool mr_bad_shape(const gvx_mrd_dims* d, int B, int n_max) {
    if (mr_dims_problem(d) || B < 1 || B > 65535 || n_max < mr_min_samples(*d) || n_max > GVX_MRD_MAX_SAMPLES) return true;
    for (int r = 0; r < d->n_resolutions; ++r)
        if ((long long)mr_frames(n_max, d->n_fft[r], d->hop[r]) * (d->n_fft[r] / 2 + 1) > GVX_MRD_MAX_POSITIONS) return true;
    return false;
}

struct MrFeat {   // the features buffer: map (resolution r, layer i) is [B][frames][bins][channels] at byte `off`
    size_t off[GVX_MRD_MAX_RESOLUTIONS][MR_MAPS];
    int channels[MR_MAPS];
    int frames[GVX_MRD_MAX_RESOLUTIONS][MR_MAPS];
    int bins[GVX_MRD_MAX_RESOLUTIONS];
    size_t total;
};

inline MrFeat mr_feat_layout(const gvx_mrd_dims& d, int B, int n_max) {
    MrFeat F{};
    MrLayer L[MR_MAPS];
    mr_layers(d, L);
    size_t at = 0;
    for (int r = 0; r < d.n_resolutions; ++r) {
        F.bins[r] = d.n_fft[r] / 2 + 1;
        for (int i = 0; i < MR_MAPS; ++i) {
            F.channels[i] = L[i].cout;
            F.frames[r][i] = mr_width(n_max, d.n_fft[r], d.hop[r], i + 1);
            F.off[r][i] = at;
            at += gvx::round256((size_t)B * F.frames[r][i] * F.bins[r] * L[i].cout * sizeof(float));
        }
    }
    F.total = at < 256 ? 256 : at;
    return F;
}

// the pieces of one layer's weight gradient: MR_PIECE_FRAMES output frames of `rows_per_piece` rows each; the rows are grouped only
// where the partial gradients would pass DC_PART_FLOATS
struct MrPieces { int chunks, rows_per_piece, n, split; size_t numel; };   // n * split partial sums of numel floats
inline MrPieces mr_pieces(const MrLayer& l, int B, int frames) {
    MrPieces P{};
    P.numel = l.wn();
    P.split = l.mfma ? 1 : MR_WG_VALU_SPLIT;
    P.chunks = (frames + MR_PIECE_FRAMES - 1) / MR_PIECE_FRAMES;
    if (P.chunks < 1) P.chunks = 1;
    size_t most = DC_PART_FLOATS / (P.numel * P.chunks * P.split);
    if (most < 1) most = 1;
    P.rows_per_piece = (int)(((size_t)B + most - 1) / most);
    P.n = ((B + P.rows_per_piece - 1) / P.rows_per_piece) * P.chunks;
    return P;
}

// byte offsets: the spectrogram of one resolution (forward and backward); the backward's gradient of it, the frame gradients
// [B][frames][n_fft], two activation gradients of the largest map, the partial weight and bias gradients
struct MrWs { size_t mag, dmag, g, grad[2], parts, db_parts, total; };

inline MrWs mr_ws_plan(const gvx_mrd_dims& d, int B, int n_max, bool backward) {
    MrWs W{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += gvx::round256(bytes); return o; };
    MrLayer L[MR_MAPS];
    mr_layers(d, L);
    const MrFeat F = mr_feat_layout(d, B, n_max);
    size_t mag = 0, g = 0, act = 0, parts = 0;
    for (int r = 0; r < d.n_resolutions; ++r) {
        const size_t w0 = (size_t)mr_frames(n_max, d.n_fft[r], d.hop[r]);
        if (B * w0 * F.bins[r] > mag) mag = B * w0 * F.bins[r];
        if (B * w0 * d.n_fft[r] > g) g = B * w0 * d.n_fft[r];
        for (int i = 0; i < MR_MAPS; ++i) {
            const size_t a = (size_t)B * F.frames[r][i] * F.bins[r] * L[i].cout;
            if (i < MR_MAPS - 1 && a > act) act = a;
            const MrPieces P = mr_pieces(L[i], B, F.frames[r][i]);
            if (P.n * P.split * P.numel > parts) parts = P.n * P.split * P.numel;
        }
    }
    W.mag = take(mag * sizeof(float));
    if (backward) {
        W.dmag = take(mag * sizeof(float));
        W.g = take(g * sizeof(float));
        W.grad[0] = take(act * sizeof(float));
        W.grad[1] = take(act * sizeof(float));
        W.parts = take(parts * sizeof(float));
        W.db_parts = take((size_t)DC_DB_SLICES * d.channels * sizeof(double));
    }
    W.total = at < 256 ? 256 : at;
    return W;
}

}  // namespace gvx_mr
