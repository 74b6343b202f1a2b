// The host side that all four discriminators share - csrc/melgan_disc.hip, hifigan_disc.hip, hifigan_msd.hip, mrd.hip: the handle on
// the generators' base (gen_host.h: blob, bind, timing flag, marks, the workspace check), the layer times of a forward and a backward,
// the lookup of every layer's (weight, bias) pair in a table, and the argument checks that the C ABIs word alike.  No kernels: what
// launches the HiFi-GAN family's shared convolution core is disc_host.h.  A "stack" is one period, scale or resolution: nl layers.
#pragma once
#include "gen_host.h"

#include <string>

namespace gvx_dc {

using gvx::fail;
using gvx_gen::gen_bind;
using gvx_gen::gen_check_workspace;

// the base's marks are the forward's; a timed call makes its events on first use: mark `at` of (nl + 1) per stack
struct DcHandle : gvx_gen::GenHandle {
    gvx_gen::GenMarks bwd_marks;
    bool fwd_timed = false, bwd_timed = false;   // that direction has run since timing was enabled
};

inline int dc_timing_enable(DcHandle* h, int enable) {
    if (h) h->fwd_timed = h->bwd_timed = false;
    return gvx_gen::gen_timing_enable(h, enable, 0);
}

inline int dc_mark(const DcHandle* h, gvx_gen::GenMarks& marks, size_t at, hipStream_t s) {
    if (!h->timing) return GVX_OK;
    if (const int rc = gvx_gen::gen_make_marks(marks, (int)at + 1)) return rc;
    return gvx_gen::gen_mark(h, (int)at, s, &marks);
}

// per layer, summed over the stacks: the time between the marks of the last timed forward and backward
inline int dc_layer_times_ms(DcHandle* h, int n_stacks, int nl, float* forward_ms, float* backward_ms, int* n_layers_out) {
    if (!h || !forward_ms || !backward_ms || !n_layers_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    *n_layers_out = nl;
    for (int i = 0; i < nl; ++i) forward_ms[i] = backward_ms[i] = 0.f;
    for (int j = 0; j < n_stacks; ++j)
        for (int i = 0; i < nl; ++i) {
            const size_t at = (size_t)j * (nl + 1) + i;
            float ms = 0.f;
            if (h->fwd_timed) {
                HIP_TRY(hipEventSynchronize(h->marks.ev[at + 1]));
                HIP_TRY(hipEventElapsedTime(&ms, h->marks.ev[at], h->marks.ev[at + 1]));
                forward_ms[i] += ms;
            }
            if (h->bwd_timed) {   // the backward walks down: mark i + 1 comes before mark i
                HIP_TRY(hipEventSynchronize(h->bwd_marks.ev[at]));
                HIP_TRY(hipEventElapsedTime(&ms, h->bwd_marks.ev[at + 1], h->bwd_marks.ev[at]));
                backward_ms[i] += ms;
            }
        }
    return GVX_OK;
}

// layer i of stack j as the HiFi-GAN family names it, the score last
inline std::string dc_name(int j, int i, int nl) {
    return "discriminators." + std::to_string(j) + (i == nl - 1 ? std::string(".conv_post") : ".convs." + std::to_string(i));
}

// the (weight, bias) pair of layer i of stack j in a table of weights or of gradients -> out[j * nl + i]; a Layer states its weight's
// elements as wn() and its bias's as cout; name(j, i, nl) is the layer's prefix
struct DcParam { float* w; float* b; };

template <class Layer, class Name = decltype(&dc_name)>
int dc_find_params(const gvx_weight_desc* table, int n, int n_stacks, const Layer* L, int nl, DcParam* out, Name name = dc_name) {
    int rc = GVX_OK;
    for (int j = 0; j < n_stacks; ++j)
        for (int i = 0; i < nl; ++i) {
            const std::string prefix = name(j, i, nl);
            const gvx_weight_desc* w = gvx_gen::gen_find(table, n, prefix + ".weight", L[i].wn(), rc);
            if (!w) return rc;
            const gvx_weight_desc* b = gvx_gen::gen_find(table, n, prefix + ".bias", (size_t)L[i].cout, rc);
            if (!b) return rc;
            out[j * nl + i] = DcParam{const_cast<float*>(w->data), const_cast<float*>(b->data)};
        }
    return GVX_OK;
}

// the gradients' table of a backward (no entries: none are asked for) -> out, as dc_find_params
template <class Layer, class Name = decltype(&dc_name)>
int dc_find_grads(const gvx_grad_desc* grads, int n_grads, int n_stacks, const Layer* L, int nl, DcParam* out, Name name = dc_name) {
    static_assert(sizeof(gvx_weight_desc) == sizeof(gvx_grad_desc), "the two tables share a layout");
    if (n_grads == 0) return GVX_OK;
    return dc_find_params(reinterpret_cast<const gvx_weight_desc*>(grads), n_grads, n_stacks, L, nl, out, name);   // same fields, the data pointer writable
}

// ---- the argument checks of forward and backward, in the order of the calls; the workspace's is gen_check_workspace
inline int dc_check_call(const gvx_gen::GenHandle* h, const float* wav, const void* features, int B) {
    if (!h || !wav || !features) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    return GVX_OK;
}

inline int dc_check_features(const void* features, size_t features_bytes, size_t need) {
    if ((uintptr_t)features % 256 || features_bytes < need)
        return fail(GVX_ERR_WORKSPACE, "the features buffer is misaligned or smaller than %zu bytes", need);
    return GVX_OK;
}

inline int dc_check_backward(const void* features, const void* d_features, const gvx_grad_desc* grads, int n_grads, const float* d_wav) {
    if (!d_features) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_grads < 0 || (n_grads > 0 && !grads)) return fail(GVX_ERR_INVALID_ARG, "n_grads = %d without a table", n_grads);
    if (n_grads == 0 && !d_wav) return fail(GVX_ERR_INVALID_ARG, "neither parameter gradients nor d_wav are asked for");
    if ((uintptr_t)features % 256 || (uintptr_t)d_features % 256) return fail(GVX_ERR_WORKSPACE, "features or d_features is not 256-byte aligned");
    return GVX_OK;
}

}  // namespace gvx_dc
