// The host side that csrc/hifigan_disc.hip, csrc/hifigan_msd.hip and csrc/mrd.hip share on top of disc_handle.h: what launches the
// kernels of their common convolution core (disc_conv.h) - the pack loop, and the per-layer blocks of the backward walk.
#pragma once
#include "disc_conv.h"
#include "disc_handle.h"

namespace gvx_dc {

constexpr int DC_MAX_STACKS = 8;

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
