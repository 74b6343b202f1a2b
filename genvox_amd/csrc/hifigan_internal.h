// The HiFi-GAN generator's host-side description (csrc/hifigan.hip): the handle, the layer description of the windowed implicit GEMM
// with its row arithmetic, the dims check and the blob layout.  The model is defined in include/genvox_amd.h, "HiFi-GAN generator".
#pragma once
#include "gen_host.h"

#include <functional>

struct gvx_hifigan : gvx_gen::GenHandle {
    gvx_hifigan_dims d;
    bool lds_ready = false;        // hg_prepare
    gvx_gen::GenMarks bwd_marks;   // gvx_hifigan_backward's parts (hifigan_train.hip)
};

namespace gvx_hg {

using namespace gvx_gen;

// One layer:  out[b][phases * q + phase][n] = epilogue( bias[n] + sum over taps tau, channels c of
//                                                       act(src[b][q - left + off0 + tau * step][c]) * W[phase][n][tau * Cin + c] )
// with zeros for source positions outside [0, len_b).
//   convolution (phases = 1)      left = (taps - 1) dil / 2, off0 = 0, step = dil
//   transposed conv (phases = r)  kernel 2r, stride r, padding r/2: output r q + phase receives input q (tap 0) and input q - 1 (phase <
//                                 r/2) or q + 1 (tap 1):  phase < r/2: left = 1, off0 = 1, step = -1;  else left = 0, off0 = 0, step = 1
struct HgLayer {
    const float* src; const float* W; const float* bias;
    const float* res;      // added element by element after the bias (a residual block's own input), or nullptr
    float* out;
    const int32_t* lens;   // frames per row, or nullptr
    int T, in_mul;         // row b has T_b * in_mul input positions; tensors are strided by T * in_mul positions per row
    int Cin, Cout, K;      // K = taps * Cin
    int taps, dil, phases;
    int act;               // LeakyReLU(slope) on the operand
    int accumulate;        // the value is added to what out holds (the later residual blocks of a stage)
    float divide;          // > 0: the value is divided by it last (the stage's average)
    int zero_tail, tanh_out;
    float slope;
    // data gradients only (hifigan_kernels.h, BWD): the raw tape tensor whose LeakyReLU the gradient passes through, and a second tensor
    // added element by element after `res`; both [B][len][Cout] or nullptr
    const float* mask; const float* add2;
};

struct HgTaps { int halo, left, off0, step; };

__host__ __device__ __forceinline__ HgTaps hg_taps(int taps, int dil, int phases, int phase) {
    if (phases == 1) return {(taps - 1) * dil, (taps - 1) * dil / 2, 0, dil};
    return 2 * phase < phases ? HgTaps{1, 1, 1, -1} : HgTaps{1, 0, 0, 1};
}

__device__ __forceinline__ float hg_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

inline int hg_cpad(const gvx_hifigan_dims& d) { return (d.n_mels + 3) & ~3; }
inline int hg_convs_per_dilation(const gvx_hifigan_dims& d) { return d.resblock == 1 ? 2 : 1; }

inline const char* hg_dims_problem(const gvx_hifigan_dims* d) {
    if (!d) return "null dims";
    if (d->n_mels < 1) return "n_mels must be >= 1";
    if (d->n_stages < 1 || d->n_stages > GVX_HIFIGAN_MAX_STAGES) return "there must be 1 to GVX_HIFIGAN_MAX_STAGES upsampling stages";
    long hop = 1;
    for (int i = 0; i < d->n_stages; ++i) {
        if (d->upsample_rates[i] < 2 || (d->upsample_rates[i] & 1)) return "every upsampling rate must be even and >= 2";
        if (d->upsample_kernel_sizes[i] != 2 * d->upsample_rates[i])
            return "only upsample_kernel_sizes[i] == 2 * upsample_rates[i] is supported (the two-tap phase split of the transposed convolution)";
        hop *= d->upsample_rates[i];
        if (hop > GVX_HIFIGAN_MAX_HOP) return "the product of the rates is beyond GVX_HIFIGAN_MAX_HOP";
    }
    const int C0 = d->upsample_initial_channel;
    if (C0 < 1 || C0 % (1 << d->n_stages) != 0) return "upsample_initial_channel must be divisible by 2^n_stages";
    if ((C0 >> d->n_stages) < 4 || (C0 >> d->n_stages) % 4 != 0) return "every stage's channel count must be a multiple of 4 and at least 4";
    if (d->resblock != 1 && d->resblock != 2) return "resblock must be 1 or 2";
    if (d->n_dilations != (d->resblock == 1 ? 3 : 2)) return "resblock 1 has three dilations per block, resblock 2 has two";
    if (d->n_resblocks < 1 || d->n_resblocks > GVX_HIFIGAN_MAX_RESBLOCKS) return "there must be 1 to GVX_HIFIGAN_MAX_RESBLOCKS residual blocks per stage";
    for (int j = 0; j < d->n_resblocks; ++j) {
        const int k = d->resblock_kernel_sizes[j];
        if (k < 3 || k > 11 || !(k & 1)) return "every resblock kernel size must be odd and in [3, 11]";
        for (int m = 0; m < d->n_dilations; ++m) {
            const int dil = d->resblock_dilation_sizes[j][m];
            if (dil < 1) return "every dilation must be >= 1";
            if ((long)(k - 1) * dil > GVX_HIFIGAN_MAX_WINDOW) return "(kernel size - 1) * dilation must not pass GVX_HIFIGAN_MAX_WINDOW (72)";
        }
    }
    if (!(d->slope >= 0.f && d->slope <= 1.f) || !(d->post_slope >= 0.f && d->post_slope <= 1.f)) return "slope and post_slope must be in [0, 1]";
    return nullptr;
}

struct HgBlob {   // offsets in floats; conv_w[i][j][m][0 / 1]: convs1 / convs2 (resblock 2: only [0], its convs)
    size_t pre_w, pre_b, post_w, post_b;
    size_t up_w[GVX_HIFIGAN_MAX_STAGES], up_b[GVX_HIFIGAN_MAX_STAGES];
    size_t conv_w[GVX_HIFIGAN_MAX_STAGES][GVX_HIFIGAN_MAX_RESBLOCKS][GVX_HIFIGAN_MAX_DILATIONS][2];
    size_t conv_b[GVX_HIFIGAN_MAX_STAGES][GVX_HIFIGAN_MAX_RESBLOCKS][GVX_HIFIGAN_MAX_DILATIONS][2];
    size_t total;
};

inline HgBlob hg_blob_layout(const gvx_hifigan_dims& d) {
    HgBlob L{};
    size_t at = 0;
    auto take = [&](size_t floats) { const size_t o = at; at += gvx::round64(floats); return o; };
    size_t C = d.upsample_initial_channel;
    L.pre_w = take(C * 7 * hg_cpad(d));
    L.pre_b = take(C);
    for (int i = 0; i < d.n_stages; ++i) {
        const size_t Cn = C / 2;
        L.up_w[i] = take((size_t)d.upsample_rates[i] * Cn * 2 * C);
        L.up_b[i] = take(Cn);
        for (int j = 0; j < d.n_resblocks; ++j)
            for (int m = 0; m < d.n_dilations; ++m)
                for (int v = 0; v < hg_convs_per_dilation(d); ++v) {
                    L.conv_w[i][j][m][v] = take(Cn * d.resblock_kernel_sizes[j] * Cn);
                    L.conv_b[i][j][m][v] = take(Cn);
                }
        C = Cn;
    }
    L.post_w = take(7 * C);
    L.post_b = take(1);
    L.total = at;
    return L;
}

// the names of a residual block's convolutions: [m][0 / 1]
inline std::string hg_conv_name(const gvx_hifigan_dims& d, int block, int m, int v) {
    const std::string base = "resblocks." + std::to_string(block);
    if (d.resblock == 2) return base + ".convs." + std::to_string(m);
    return base + (v == 0 ? ".convs1." : ".convs2.") + std::to_string(m);
}

// hifigan.hip, for the training path and the generators built on these layers: one layer's launch, the dynamic-LDS sizes of its
// kernels (once per handle: *ready is the handle's flag), the mel transpose
int hg_launch(const HgLayer& p, int B, hipStream_t s);
int hg_prepare(bool* ready);
int hg_mel_transpose(const float* mel, const int32_t* lens, int B, int M, int T, int Cp, float* out, hipStream_t s);

// ---- the forward that HiFi-GAN and BigVGAN share (hifigan.hip)
constexpr int HG_MAX_BUFS = 5;
struct HgWs {   // byte offsets; n_bufs tensors of the widest activation's size behind the transposed mel
    size_t mel_t, buf[HG_MAX_BUFS], total;
};
HgWs hg_ws_plan(const gvx_hifigan_dims& d, int B, int T, int n_bufs);

// Where a layer of the forward stands.  A model's HgFront is called with every layer just before its launch, the layer's src being the
// tensor the network's activation applies to, and makes the operand: HiFi-GAN sets the kernel's LeakyReLU and its slope, BigVGAN
// launches its activation into a tensor of its own and points src there.  At HG_POST it also says what the output goes through.
enum HgSite { HG_PRE, HG_UPS, HG_CONV, HG_POST };
struct HgAt { HgSite site; int stage, block, act; };   // HG_UPS: stage; HG_CONV: the block's act-th activation
using HgFront = std::function<int(const HgAt& at, HgLayer& p)>;

// Everything of gvx_hifigan_forward but the last mark (n_stages + 2), which the caller records behind what it adds: the argument
// checks, hg_prepare, marks 0 .. n_stages + 1, the launches.  The stage walk uses buf[0 .. 3] of wp.
int hg_forward(const GenHandle* h, bool* lds_ready, const gvx_hifigan_dims& d, const HgWs& wp, const HgFront& front, const float* mel,
               const int32_t* frame_lengths, int B, int T, float* wav_out, float* const* stage_out, void* workspace, size_t workspace_bytes, hipStream_t s);

}  // namespace gvx_hg
