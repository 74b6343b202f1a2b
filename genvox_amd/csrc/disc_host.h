// The host side that csrc/hifigan_disc.hip and csrc/hifigan_msd.hip share: what a handle holds besides its dims, the event marks and the
// layer times read off them, the parameter names and their lookup in a table, the argument checks that the two C ABIs have in common,
// the pack loop, and the per-layer blocks of the backward walk.  A "stack" is one period or one scale: nl layers, the score last.
#pragma once
#include "disc_conv.h"
#include "gen_host.h"

#include <string>
#include <vector>

namespace gvx_dc {

using gvx::fail;

constexpr int DC_MAX_STACKS = 8;

struct DcHandle {
    const float* blob = nullptr;
    bool timing = false;                     // measurement only: events around every layer of the last forward / backward
    std::vector<hipEvent_t> fwd_ev, bwd_ev;  // per stack nl + 1 marks
    bool fwd_timed = false, bwd_timed = false;
    ~DcHandle() {
        for (hipEvent_t e : fwd_ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : bwd_ev) (void)hipEventDestroy(e);
    }
};

inline int dc_bind(DcHandle* h, const float* device_blob) {
    if (!h || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if ((uintptr_t)device_blob % 256) return fail(GVX_ERR_INVALID_ARG, "the blob must be 256-byte aligned");
    h->blob = device_blob;
    return GVX_OK;
}

inline int dc_timing_enable(DcHandle* h, int enable) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    h->timing = enable != 0;
    h->fwd_timed = h->bwd_timed = false;
    return GVX_OK;
}

// the next of a call's marks on the stream: mark `at` of (nl + 1) per stack, made on first use; nothing when the handle is not timed
inline int dc_mark(const DcHandle* h, std::vector<hipEvent_t>& ev, size_t at, hipStream_t s) {
    if (!h->timing) return GVX_OK;
    while (ev.size() <= at) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        ev.push_back(e);
    }
    HIP_TRY(hipEventRecord(ev[at], s));
    return GVX_OK;
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
                HIP_TRY(hipEventSynchronize(h->fwd_ev[at + 1]));
                HIP_TRY(hipEventElapsedTime(&ms, h->fwd_ev[at], h->fwd_ev[at + 1]));
                forward_ms[i] += ms;
            }
            if (h->bwd_timed) {   // the backward walks down: mark i + 1 comes before mark i
                HIP_TRY(hipEventSynchronize(h->bwd_ev[at]));
                HIP_TRY(hipEventElapsedTime(&ms, h->bwd_ev[at + 1], h->bwd_ev[at]));
                backward_ms[i] += ms;
            }
        }
    return GVX_OK;
}

inline std::string dc_name(int j, int i, int nl) {
    return "discriminators." + std::to_string(j) + (i == nl - 1 ? std::string(".conv_post") : ".convs." + std::to_string(i));
}

// the (weight, bias) pair of layer i of stack j in a table of weights or of gradients -> out[j * nl + i]; a Layer states its weight's
// elements as wn() and its bias's as cout
struct DcParam { float* w; float* b; };

template <class Layer>
int dc_find_params(const gvx_weight_desc* table, int n, int n_stacks, const Layer* L, int nl, DcParam* out) {
    int rc = GVX_OK;
    for (int j = 0; j < n_stacks; ++j)
        for (int i = 0; i < nl; ++i) {
            const std::string name = dc_name(j, i, nl);
            const gvx_weight_desc* w = gvx_gen::gen_find(table, n, name + ".weight", L[i].wn(), rc);
            if (!w) return rc;
            const gvx_weight_desc* b = gvx_gen::gen_find(table, n, name + ".bias", (size_t)L[i].cout, rc);
            if (!b) return rc;
            out[j * nl + i] = DcParam{const_cast<float*>(w->data), const_cast<float*>(b->data)};
        }
    return GVX_OK;
}

// every stack's part of the blob from a table of PyTorch-layout tensors: pack(layer, W, base) launches the discriminator's own kernel
// that writes the layer's two weight forms under `base`; nothing is launched when a tensor is missing
template <class Layer, class Pack>
int dc_pack_weights(const gvx_weight_desc* table, int n, int n_stacks, const Layer* L, int nl, size_t per_stack, float* device_blob,
                    hipStream_t s, Pack&& pack) {
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    DcParam src[DC_MAX_STACKS * DC_MAX_MAPS];
    if (const int rc = dc_find_params(table, n, n_stacks, L, nl, src)) return rc;
    HIP_TRY(hipMemsetAsync(device_blob, 0, per_stack * n_stacks * sizeof(float), s));   // the padding between the tensors
    for (int j = 0; j < n_stacks; ++j)
        for (int i = 0; i < nl; ++i) {
            float* base = device_blob + j * per_stack;
            pack(L[i], src[j * nl + i].w, base);
            HIP_TRY(hipGetLastError());
            dc_copy_kernel<<<(unsigned)((L[i].cout + 255) / 256), 256, 0, s>>>(base + L[i].b_off, src[j * nl + i].b, (size_t)L[i].cout);
            HIP_TRY(hipGetLastError());
        }
    return GVX_OK;
}

// ---- the argument checks of forward and backward, in the order of the calls
inline int dc_check_call(const DcHandle* h, const float* wav, const void* features, int B) {
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

inline int dc_check_workspace(const void* workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || (uintptr_t)workspace % 256 || workspace_bytes < need)
        return fail(GVX_ERR_WORKSPACE, "the workspace is missing, misaligned or smaller than %zu bytes", need);
    return GVX_OK;
}

// the gradients' table of a backward (no entries: none are asked for) -> out, as dc_find_params
template <class Layer>
int dc_find_grads(const gvx_grad_desc* grads, int n_grads, int n_stacks, const Layer* L, int nl, DcParam* out) {
    static_assert(sizeof(gvx_weight_desc) == sizeof(gvx_grad_desc), "the two tables share a layout");
    if (n_grads == 0) return GVX_OK;
    return dc_find_params(reinterpret_cast<const gvx_weight_desc*>(grads), n_grads, n_stacks, L, nl, out);   // same fields, the data pointer writable
}

// ---- the backward's blocks of one layer.  The two walks differ in the order of their stacks, in how a matrix weight gradient and a
// waveform gradient are launched and in what lies in front of a first layer, and stay with their discriminators.

// the pieces of a weight gradient that is not a matrix layer's
template <bool GRID, bool TAP_MAJOR>
void dc_launch_wgrad_valu(const DcConv& p, const DcPieces& P, float* parts, int B, hipStream_t s) {
    dc_wgrad_valu_kernel<GRID, TAP_MAJOR><<<dim3((unsigned)((P.numel + 255) / 256), (unsigned)P.n), 256, 0, s>>>(p, parts, B, P.chunks,
                                                                                                                  P.rows_per_piece, P.run);
}

// behind the launch of the pieces: their sum into the weight's gradient, and the bias's gradient
template <bool GRID, bool TAP_MAJOR>
int dc_finish_param_grads(const DcConv& p, const DcPieces& P, const float* parts, double* db_parts, const DcParam& g, int B, hipStream_t s) {
    HIP_TRY(hipGetLastError());
    dc_reduce_kernel<TAP_MAJOR><<<(unsigned)((P.numel + 31) / 32), 256, 0, s>>>(parts, g.w, p.NC, p.KG, p.k, P.n);
    HIP_TRY(hipGetLastError());
    dc_db_kernel<GRID><<<dim3((unsigned)((p.NC + 31) / 32), DC_DB_SLICES), 256, 0, s>>>(p, db_parts, B);
    HIP_TRY(hipGetLastError());
    dc_db_reduce_kernel<<<(unsigned)((p.NC + 255) / 256), 256, 0, s>>>(db_parts, g.b, p.NC);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// the data gradient is a convolution with the sides exchanged: dY is the operand, the layer's input map (`mask`, its cotangent `dfeat`)
// the output, the weights the blob's second form
inline DcConv dc_exchanged(const DcConv& p, const float* dy, const float* wb, const float* mask, const float* dfeat, float* out) {
    DcConv q = p;
    q.src = dy; q.W = wb; q.bias = nullptr; q.dy = nullptr;
    q.KC = p.NC; q.NC = p.KC; q.KG = p.NG; q.NG = p.KG;
    q.Ls_max = p.Lo_max; q.Lo_max = p.Ls_max; q.n_src = p.n_out; q.n_out = p.n_src;
    q.wav_src = 0;
    q.mask = mask; q.dfeat = dfeat; q.out = out;
    return q;
}

}  // namespace gvx_dc
