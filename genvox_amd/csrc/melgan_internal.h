// What csrc/melgan.hip (inference) and csrc/melgan_train.hip (tape forward, backward) share: the handle, the layer description of the
// implicit GEMM with its row arithmetic, the dims check and the blob layout.  The forward kernels live in melgan.hip and are reached
// through mg_launch.
#pragma once
#include "gen_host.h"

struct gvx_melgan : gvx_gen::GenHandle {
    gvx_melgan_dims d;
    bool lds_ready = false;
};

namespace gvx_mg {

using namespace gvx_gen;

struct MgLayer {
    const float* src0; const float* src1;   // tap sources (src1: tap 1 of the residual tail)
    const float* W; const float* bias; const float* bias2;
    float* out;
    const int32_t* lens;   // frames per row, or nullptr
    int T, in_mul;         // row b has T_b * in_mul input positions; tensors are strided by T * in_mul positions per row
    int Cin, Cout, K;      // K = taps * Cin
    int taps, dil, phases;
    int act_mask, two_src, zero_tail, tanh_out;
    float slope;
};

__device__ __forceinline__ int mg_frames(const int32_t* lens, int b, int T) { return gen_frames(lens, b, T, GVX_MELGAN_MIN_FRAMES); }

// source position of tap tau for output group q (q < len); zero: the tap lies outside the row and contributes nothing
__device__ __forceinline__ int mg_src_row(const MgLayer& p, int q, int tau, int phase, int len, bool& zero) {
    int s;
    if (p.phases == 1) {
        s = q + (tau - ((p.taps - 1) >> 1)) * p.dil;
        s = s < 0 ? -s : s;
        s = s >= len ? 2 * (len - 1) - s : s;
        zero = false;
    } else {
        s = tau == 0 ? q : (2 * phase < p.phases ? q - 1 : q + 1);
        zero = s < 0 || s >= len;
    }
    return s < 0 ? 0 : (s >= len ? len - 1 : s);
}

__device__ __forceinline__ float mg_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

inline int mg_cpad(const gvx_melgan_dims& d) { return (d.n_mels + 3) & ~3; }

inline const char* mg_dims_problem(const gvx_melgan_dims* d) {
    if (!d) return "null dims";
    if (d->n_mels < 1 || d->base_channels < 1) return "n_mels and base_channels must be >= 1";
    if (d->n_stages < 1 || d->n_stages > GVX_MELGAN_MAX_STAGES) return "n_stages must be in [1, GVX_MELGAN_MAX_STAGES]";
    long hop = 1;
    for (int i = 0; i < d->n_stages; ++i) {
        if (d->ratios[i] < 2 || (d->ratios[i] & 1)) return "every upsampling ratio must be even and >= 2";
        hop *= d->ratios[i];
        if (hop > GVX_MELGAN_MAX_HOP) return "the product of the ratios is beyond GVX_MELGAN_MAX_HOP";
    }
    if (d->base_channels % (1 << d->n_stages) != 0) return "base_channels must be divisible by 2^n_stages";
    if (d->n_residual_layers < 1 || d->n_residual_layers > 8) return "n_residual_layers must be in [1, 8]";
    if (d->dilation_base < 1) return "dilation_base must be >= 1";
    long dil = 1;
    for (int j = 1; j < d->n_residual_layers; ++j) dil *= d->dilation_base;
    if (dil >= (long)GVX_MELGAN_MIN_FRAMES * d->ratios[0]) return "the largest dilation must be below 4 * ratios[0], the shortest row of the first stage";
    if (!(d->slope >= 0.f && d->slope <= 1.f)) return "slope must be in [0, 1]";
    return nullptr;
}

struct MgBlob {   // offsets in floats
    size_t pre_w, pre_b, post_w, post_b;
    size_t up_w[GVX_MELGAN_MAX_STAGES], up_b[GVX_MELGAN_MAX_STAGES];
    size_t conv_w[GVX_MELGAN_MAX_STAGES][8], conv_b[GVX_MELGAN_MAX_STAGES][8], tail_w[GVX_MELGAN_MAX_STAGES][8], sc_b[GVX_MELGAN_MAX_STAGES][8],
        mix_b[GVX_MELGAN_MAX_STAGES][8];
    size_t total;
};

inline MgBlob mg_blob_layout(const gvx_melgan_dims& d) {
    MgBlob L{};
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t o = at; at += gvx::round64(floats); return o; };
    size_t C = d.base_channels;
    L.pre_w = take(C * 7 * mg_cpad(d));
    L.pre_b = take(C);
    for (int i = 0; i < d.n_stages; ++i) {
        const size_t Cn = C / 2;
        L.up_w[i] = take((size_t)d.ratios[i] * Cn * 2 * C);
        L.up_b[i] = take(Cn);
        for (int j = 0; j < d.n_residual_layers; ++j) {
            L.conv_w[i][j] = take(Cn * 3 * Cn);
            L.conv_b[i][j] = take(Cn);
            L.tail_w[i][j] = take(Cn * 2 * Cn);
            L.sc_b[i][j] = take(Cn);
            L.mix_b[i][j] = take(Cn);
        }
        C = Cn;
    }
    L.post_w = take(7 * C);
    L.post_b = take(1);
    L.total = at;
    return L;
}

// defined in melgan.hip
int mg_launch(const MgLayer& p, int B, hipStream_t s);   // one layer of the forward
int mg_mel_transpose(const float* mel, const int32_t* lens, int B, int M, int T, int Cp, float* out, hipStream_t s);
int mg_prepare(gvx_melgan* h);   // once per handle: the dynamic LDS size of the widest tile 

}  // namespace gvx_mg
