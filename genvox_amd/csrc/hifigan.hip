// HiFi-GAN generator inference: mel [B][n_mels][T] -> waveform [B][T * hop].  The model is defined in include/genvox_amd.h ("HiFi-GAN
// generator"); the float64 restatement the tests hold these kernels to is tests/hifigan_ref64.py.
//
// Every layer is ONE launch over channels-last activations [B][len][C] of the form hifigan_internal.h states (HgLayer): a convolution
// with zero padding, or the r two-tap phases of a transposed convolution, with LeakyReLU on the operand and one of three epilogues -
// store, store with the residual block's own input added, or the multi-receptive-field accumulation into the stage's sum.
//
//   hg_mfma_kernel   Cout >= 32: 128 positions x 128 / 64 / 32 channels per workgroup of four waves on v_mfma_f32_32x32x2_f32.  Per block
//                    of 32 input channels the tile's WHOLE input window - its 128 positions and the (taps - 1) * dil halo rows - goes
//                    into LDS once (LeakyReLU and the zeros outside the row applied at that store), and every tap's products read it
//                    at a row offset of tau * dil: a tap moves every lane's row by the same amount, so the K-contiguous 36-float rows
//                    stay conflict-free.  The weights stream as one [BN][32] tile per (channel block, tap).  Both are double buffered
//                    through registers.  An activation row is read from global memory once per channel block, not once per tap.
//   hg_valu_kernel   Cout < 32 and the 1-channel output layer (with tanh): fmaf dot products, G lanes per output element
// A workgroup belongs to one batch row and computes nothing behind that row's length; tensors the caller sees are zero-filled there.
//
// The two kernels are in hifigan_kernels.h (the training path, hifigan_train.hip, runs its data gradients on them).
// Order of this file: the mel transpose, the launches, the forward that BigVGAN shares, the C ABI.
#include "hifigan_kernels.h"

using gvx::fail;
using namespace gvx_hg;

namespace {

// mel [B][M][T] -> channels-last [B][T][Cp] with the channels padded by zeros to a multiple of four; nothing behind a row's frames is read
__global__ void __launch_bounds__(256) hg_mel_transpose_kernel(const float* mel, const int32_t* lens, int M, int T, int Cp, float* out) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)T * Cp) return;
    const int t = (int)(idx % T), c = (int)(idx / T);
    const int Tb = gen_frames(lens, b, T);
    out[((size_t)b * T + t) * Cp + c] = (t < Tb && c < M) ? mel[((size_t)b * M + c) * T + t] : 0.f;
}

// ---- host side
template <int WR, int WC, int TM, int TN>
int hg_launch_mfma(const HgLayer& p, int B, hipStream_t s) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
    const dim3 grid((unsigned)((p.T * p.in_mul + BM - 1) / BM), (unsigned)(((p.Cout + BN - 1) / BN) * p.phases), (unsigned)B);
    hg_mfma_kernel<WR, WC, TM, TN><<<grid, 256, hg_lds_bytes(hg_taps(p.taps, p.dil, p.phases, 0).halo, BN), s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

}  // namespace

int gvx_hg::hg_launch(const HgLayer& p, int B, hipStream_t s) {
    if (p.Cout >= 32 && p.Cin % 4 == 0) {
        if (p.Cout >= 128) return hg_launch_mfma<2, 2, 2, 2>(p, B, s);
        if (p.Cout > 32) return hg_launch_mfma<4, 1, 1, 2>(p, B, s);
        return hg_launch_mfma<4, 1, 1, 1>(p, B, s);
    }
    const int G = p.Cout == 1 ? 8 : 1;
    const long threads = (long)p.T * p.in_mul * p.Cout * G;
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)p.phases, (unsigned)B);
    if (G == 8) hg_valu_kernel<8><<<grid, 256, 0, s>>>(p);
    else hg_valu_kernel<1><<<grid, 256, 0, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// once per handle: the dynamic LDS of the largest window any layer of any supported configuration asks for
int gvx_hg::hg_prepare(bool* ready) {
    if (!*ready) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(hg_mfma_kernel<2, 2, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)hg_lds_bytes(GVX_HIFIGAN_MAX_WINDOW, 128)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(hg_mfma_kernel<4, 1, 1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)hg_lds_bytes(GVX_HIFIGAN_MAX_WINDOW, 64)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(hg_mfma_kernel<4, 1, 1, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)hg_lds_bytes(GVX_HIFIGAN_MAX_WINDOW, 32)));
        *ready = true;
    }
    return GVX_OK;
}

int gvx_hg::hg_mel_transpose(const float* mel, const int32_t* lens, int B, int M, int T, int Cp, float* out, hipStream_t s) {
    const dim3 grid((unsigned)(((long)T * Cp + 255) / 256), (unsigned)B);
    hg_mel_transpose_kernel<<<grid, 256, 0, s>>>(mel, lens, M, T, Cp, out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

HgWs gvx_hg::hg_ws_plan(const gvx_hifigan_dims& d, int B, int T, int n_bufs) {
    size_t widest = d.upsample_initial_channel, mul = 1, C = d.upsample_initial_channel;   // floats per frame of the widest activation tensor
    for (int i = 0; i < d.n_stages; ++i) {
        mul *= d.upsample_rates[i];
        C /= 2;
        widest = std::max(widest, mul * C);
    }
    HgWs w{};
    GenRows ws{B};
    w.mel_t = ws.rows((size_t)T * hg_cpad(d));
    for (int i = 0; i < n_bufs; ++i) w.buf[i] = ws.rows((size_t)T * widest);
    w.total = ws.total;
    return w;
}

int gvx_hg::hg_forward(const GenHandle* h, bool* lds_ready, const gvx_hifigan_dims& d, const HgWs& wp, const HgFront& front, const float* mel,
                       const int32_t* frame_lengths, int B, int T, float* wav_out, float* const* stage_out, void* workspace, size_t workspace_bytes,
                       hipStream_t s) {
    if (!h || !mel || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (T < 1) return fail(GVX_ERR_INVALID_ARG, "T = %d: a row needs at least 1 frame", T);
    if (T > GVX_HIFIGAN_MAX_FRAMES) return fail(GVX_ERR_UNSUPPORTED, "T = %d is beyond the limit of %d frames", T, GVX_HIFIGAN_MAX_FRAMES);
    int rc;
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    if ((rc = gen_check_stage_out(stage_out, d.n_stages)) != GVX_OK) return rc;
    if ((rc = hg_prepare(lds_ready)) != GVX_OK) return rc;
    const HgBlob L = hg_blob_layout(d);
    const float* blob = h->blob;
    float* pool[4];
    for (int i = 0; i < 4; ++i) pool[i] = gvx::ws_ptr<float>(workspace, wp.buf[i]);
    int ev = 0;
    if ((rc = gen_mark(h, ev++, s)) != GVX_OK) return rc;

    const int Cp = hg_cpad(d);
    float* mel_t = gvx::ws_ptr<float>(workspace, wp.mel_t);
    if ((rc = hg_mel_transpose(mel, frame_lengths, B, d.n_mels, T, Cp, mel_t, s)) != GVX_OK) return rc;
    // p = one layer's description but for the operand's treatment, then the model's front on it; the caller adds what the site needs and launches
    HgLayer p;
    auto layer = [&](const HgAt& at, const float* src, size_t w, size_t bias, float* out, int in_mul, int Cin, int Cout, int taps, int dil, int phases) {
        p = HgLayer{};
        p.lens = frame_lengths; p.T = T;
        p.src = src; p.W = blob + w; p.bias = blob + bias; p.out = out;
        p.in_mul = in_mul; p.Cin = Cin; p.Cout = Cout; p.taps = taps; p.K = taps * Cin; p.dil = dil; p.phases = phases;
        return front(at, p);
    };
    int C = d.upsample_initial_channel, mul = 1;
    float* cur = pool[0];
    if ((rc = layer({HG_PRE, 0, 0, 0}, mel_t, L.pre_w, L.pre_b, cur, 1, Cp, C, 7, 1, 1)) != GVX_OK) return rc;
    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
    if ((rc = gen_mark(h, ev++, s)) != GVX_OK) return rc;

    const int nv = hg_convs_per_dilation(d);
    for (int i = 0; i < d.n_stages; ++i) {
        const int Cn = C / 2, r = d.upsample_rates[i];
        // the stage's tensors: x, its sum, and a block's two.  The stage's input is free once ups has run; it is a pool tensor unless
        // the caller's stage_out[i - 1] holds it, and then the sum is the caller's too and leaves a pool tensor over.
        float* rest[4];
        int n_rest = 0;
        for (float* c : pool)
            if (c != cur) rest[n_rest++] = c;
        float* x = rest[0];
        float* sum = stage_out ? stage_out[i] : rest[1];
        float* t0 = rest[2];
        float* t1 = n_rest == 3 ? cur : rest[1];
        if ((rc = layer({HG_UPS, i, 0, 0}, cur, L.up_w[i], L.up_b[i], x, mul, C, Cn, 2, 0, r)) != GVX_OK) return rc;
        if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
        mul *= r;
        for (int j = 0; j < d.n_resblocks; ++j) {
            const int k = d.resblock_kernel_sizes[j];
            const float* in = x;   // the block's running value
            for (int m = 0; m < d.n_dilations; ++m) {
                const bool last = m == d.n_dilations - 1;
                const int dil = d.resblock_dilation_sizes[j][m];
                const float* conv_in = in;
                int conv_dil = dil, v = 0;
                float* next;
                if (d.resblock == 1) {   // t1 = convs1(act(in)); next = in + convs2(act(t1)): next may be `in` itself once that is t0
                    if ((rc = layer({HG_CONV, i, j, nv * m}, in, L.conv_w[i][j][m][0], L.conv_b[i][j][m][0], t1, mul, Cn, Cn, k, dil, 1)) != GVX_OK) return rc;
                    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
                    conv_in = t1; conv_dil = 1; v = 1;
                    next = t0;
                } else {                 // next = in + convs(act(in)): the convolution reads its neighbours, so next is another tensor
                    next = in == t0 ? t1 : t0;
                }
                if ((rc = layer({HG_CONV, i, j, nv * m + v}, conv_in, L.conv_w[i][j][m][v], L.conv_b[i][j][m][v], last ? sum : next, mul, Cn, Cn, k, conv_dil,
                                1)) != GVX_OK) return rc;
                p.res = in;
                if (last) {   // y_j goes into the stage's sum: written by the first block, added by the later ones, the last divides
                    p.accumulate = j > 0;
                    p.divide = j == d.n_resblocks - 1 ? (float)d.n_resblocks : 0.f;
                    p.zero_tail = (stage_out && j == 0) ? 1 : 0;
                }
                if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
                in = next;
            }
        }
        cur = sum;
        C = Cn;
        if ((rc = gen_mark(h, ev++, s)) != GVX_OK) return rc;
    }
    if ((rc = layer({HG_POST, 0, 0, 0}, cur, L.post_w, L.post_b, wav_out, mul, C, 1, 7, 1, 1)) != GVX_OK) return rc;
    p.zero_tail = 1;
    return hg_launch(p, B, s);
}

extern "C" {

size_t gvx_hifigan_blob_floats(const gvx_hifigan_dims* dims) {
    if (hg_dims_problem(dims)) return 0;
    return hg_blob_layout(*dims).total;
}

size_t gvx_hifigan_workspace_bytes(const gvx_hifigan_dims* dims, int B, int T) {
    if (hg_dims_problem(dims) || B < 1 || T < 1 || T > GVX_HIFIGAN_MAX_FRAMES) return 0;
    return hg_ws_plan(*dims, B, T, 4).total;
}

int gvx_hifigan_pack_weights_device(const gvx_hifigan_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = hg_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_hifigan_dims& d = *dims;
    const HgBlob L = hg_blob_layout(d);
    GenConvPacker P{{table, n}};
    auto conv = [&](const std::string& name, size_t dst_w, size_t dst_b, int Cout, int Cin, int Cp, int k) {
        P.conv(name + ".weight", dst_w, Cout, Cin, Cp, k, k * Cp, 0);
        P.bias(name + ".bias", dst_b, Cout);
    };
    int C = d.upsample_initial_channel;
    conv("conv_pre", L.pre_w, L.pre_b, C, d.n_mels, hg_cpad(d), 7);
    for (int i = 0; i < d.n_stages; ++i) {
        const int Cn = C / 2;
        const std::string up = "ups." + std::to_string(i);
        P.tconv(up + ".weight", L.up_w[i], C, Cn, d.upsample_rates[i]);
        P.bias(up + ".bias", L.up_b[i], Cn);
        for (int j = 0; j < d.n_resblocks; ++j)
            for (int m = 0; m < d.n_dilations; ++m)
                for (int v = 0; v < hg_convs_per_dilation(d); ++v)
                    conv(hg_conv_name(d, i * d.n_resblocks + j, m, v), L.conv_w[i][j][m][v], L.conv_b[i][j][m][v], Cn, Cn, Cn, d.resblock_kernel_sizes[j]);
        C = Cn;
    }
    conv("conv_post", L.post_w, L.post_b, 1, C, C, 7);
    return P.run(device_blob, L.total, (hipStream_t)stream);
}

int gvx_hifigan_create(const gvx_hifigan_dims* dims, gvx_hifigan** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = hg_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_hifigan* h = new gvx_hifigan();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_hifigan_destroy(gvx_hifigan* h) { delete h; }

int gvx_hifigan_bind(gvx_hifigan* h, const float* device_blob) { return gen_bind(h, device_blob); }

int gvx_hifigan_timing_enable(gvx_hifigan* h, int enable) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const int need = h->d.n_stages + 3;
    if (enable)
        if (const int rc = gen_make_marks(h->bwd_marks, need + 1)) return rc;
    return gen_timing_enable(h, enable, need);
}

int gvx_hifigan_stage_times_ms(gvx_hifigan* h, float* ms_out, int* n_out) { return gen_stage_times_ms(h, h ? h->d.n_stages + 2 : 0, ms_out, n_out); }

int gvx_hifigan_forward(gvx_hifigan* h, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, float* const* stage_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_hifigan_dims& d = h->d;
    hipStream_t s = (hipStream_t)stream;
    // LeakyReLU on every operand but conv_pre's, in the kernel; conv_post has a slope of its own and tanh behind it
    const HgFront front = [&d](const HgAt& at, HgLayer& p) {
        p.slope = at.site == HG_POST ? d.post_slope : d.slope;
        p.act = at.site != HG_PRE;
        p.tanh_out = at.site == HG_POST;
        return (int)GVX_OK;
    };
    if (const int rc = hg_forward(h, &h->lds_ready, d, hg_ws_plan(d, B, T, 4), front, mel, frame_lengths, B, T, wav_out, stage_out, workspace, workspace_bytes, s))
        return rc;
    return gen_mark(h, d.n_stages + 2, s);
}

}  // C ABI
