// BigVGAN generator inference: mel [B][n_mels][T] -> waveform [B][T * hop].  The model is defined in include/genvox_amd.h ("BigVGAN
// generator"); the float64 restatement the tests hold this file to is tests/bigvgan_ref64.py.
//
// The network is HiFi-GAN's with every LeakyReLU replaced by the anti-aliased Snake activation A (2x Kaiser-sinc upsample, Snake, 2x
// low-pass downsample).  Every convolution is hg_launch (hifigan.hip) with act = 0 on the packed layouts of gvx_hifigan_pack_weights_device;
// what is new here is A as ONE launch in front of the convolution that reads it:
//
//   bv_snake_kernel<CB>   a workgroup of 256 threads owns BV_P = 32 positions of one row by CB channels (64, or the power of two that
//                         covers a narrower tensor), lanes along the channels: every global and LDS access of a wave is a run of
//                         consecutive floats.  x[t0 - 6 .. t0 + P + 5] goes into LDS once, both ends clamped to the row.  Then z in
//                         pairs (2 q, 2 q + 1) for q = t0 - 3 .. t0 + P + 2, each formed once: the two phases of u share seven values
//                         of x for their six taps each, then one sine each (bv_sin_sq); beyond the row's ends z is repeated as the definition
//                         asks.  Then the P outputs, twelve taps of z each.  (2 P + 12) / 2 P = 1.19 sines per upsampled position.
// Positions at and behind a row's length are written as zeros, and x is never read there.
//
// Order of this file: the activation, the clamp, the blob's activation part, the C ABI.
#include "hifigan_internal.h"

using gvx::fail;
using namespace gvx_hg;

struct gvx_bigvgan : gvx_gen::GenHandle {
    gvx_bigvgan_dims d;
    bool lds_ready = false;   // hg_prepare
};

namespace {

constexpr int BV_P = GVX_BIGVGAN_ACT_TILE;
constexpr int BV_TAPS = GVX_BIGVGAN_FILTER_TAPS;
constexpr int BV_XROWS = BV_P + 12;        // x[t0 - 6 .. t0 + P + 5]
constexpr int BV_QROWS = BV_P + 6;         // the pairs z[2 q], z[2 q + 1] of q = t0 - 3 .. t0 + P + 2

struct BvAct {
    const float* x; float* out;
    const int32_t* lens;   // per row: positions / mul, or nullptr
    int T, mul;            // row b has min(lens[b], T) * mul positions; tensors are strided by T * mul positions per row
    int C;
    const float* f; const float* a; const float* g;
};

// sin(t)^2 without the library's sine: sin^2 has period pi and no sign, so t is reduced to r = t - k pi in [-pi / 2, pi / 2] (pi in
// three parts, every step one fma: exact to an ulp of r for |t| < 8192) and sin(r) is its Taylor polynomial through r^13 (6.7e-10 at
// pi / 2) - no quadrant logic, no table.  15 % off the kernel against sinf (EXPERIMENTS.md); larger arguments take sinf.
__device__ __forceinline__ float bv_sin_sq(float t) {
    float s;
    if (fabsf(t) < 8192.f) {
        const float k = rintf(t * 0.318309886183790672f);
        float r = fmaf(-k, 3.140625f, t);
        r = fmaf(-k, 9.67502593994140625e-4f, r);
        r = fmaf(-k, 1.509957990978376432e-7f, r);
        const float r2 = r * r;
        float q = 1.6059043836821613e-10f;
        q = fmaf(q, r2, -2.5052108385441720e-8f);
        q = fmaf(q, r2, 2.7557319223985893e-6f);
        q = fmaf(q, r2, -1.9841269841269841e-4f);
        q = fmaf(q, r2, 8.3333333333333333e-3f);
        q = fmaf(q, r2, -1.6666666666666666e-1f);
        s = fmaf(r * r2, q, r);
    } else {
        s = sinf(t);
    }
    return s * s;
}

template <int CB>
__global__ void __launch_bounds__(256) bv_snake_kernel(const BvAct p) {
    constexpr int PG = 256 / CB;   // positions handled side by side
    __shared__ float xs[BV_XROWS * CB];
    __shared__ float zs[2 * BV_QROWS * CB];
    const int tid = threadIdx.x, cl = tid % CB, pg = tid / CB;
    const int b = blockIdx.z, c = (int)blockIdx.y * CB + cl, t0 = (int)blockIdx.x * BV_P;
    const bool c_ok = c < p.C;
    const int Lmax = p.T * p.mul;
    const int len = gen_frames(p.lens, b, p.T) * p.mul;
    const size_t row = (size_t)b * Lmax;
    const int t_end = min(t0 + BV_P, Lmax);
    if (t0 >= len) {   // nothing of this row here
        if (c_ok)
            for (int t = t0 + pg; t < t_end; t += PG) p.out[(row + t) * p.C + c] = 0.f;
        return;
    }
    constexpr int X_IT = (BV_XROWS + PG - 1) / PG;   // every load of a thread is issued before the first is waited for
    float xr[X_IT];
#pragma unroll
    for (int it = 0; it < X_IT; ++it) {
        const int i = pg + it * PG;
        const int pos = min(max(t0 - 6 + i, 0), len - 1);
        xr[it] = (c_ok && i < BV_XROWS) ? p.x[(row + pos) * p.C + c] : 0.f;
    }
#pragma unroll
    for (int it = 0; it < X_IT; ++it) {
        const int i = pg + it * PG;
        if (i < BV_XROWS) xs[i * CB + cl] = xr[it];
    }
    float f[BV_TAPS];
#pragma unroll
    for (int j = 0; j < BV_TAPS; ++j) f[j] = p.f[j];
    const float a = c_ok ? p.a[c] : 0.f, g = c_ok ? p.g[c] : 0.f;
    __syncthreads();

    // The z pair of q: z[2 q] from x[q - 3 .. q + 2] with f[11], f[9], .. f[1], z[2 q + 1] from x[q - 2 .. q + 3] with f[10], f[8], .. f[0]
    // (u[m] = 2 sum_i xp[i] f[m + 13 - 2 i], xp[i] = x[i - 4]): seven values of x for twelve products.  Beyond the row's ends z is
    // repeated, not recomputed: a pair in front of the row is z[0] twice, a pair behind it z[2 n - 1] twice.
#pragma unroll 2
    for (int qi = pg; qi < BV_QROWS; qi += PG) {
        const int q = t0 - 3 + qi;
        const int qc = min(max(q, 0), len - 1);
        const float* xw = &xs[(qc - t0 + 3) * CB + cl];   // x[qc - 3]
        float xv[7];
#pragma unroll
        for (int e = 0; e < 7; ++e) xv[e] = xw[e * CB];
        float ue = 0.f, uo = 0.f;
#pragma unroll
        for (int e = 0; e < 6; ++e) {
            ue = fmaf(xv[e], f[11 - 2 * e], ue);
            uo = fmaf(xv[e + 1], f[10 - 2 * e], uo);
        }
        ue *= 2.f;
        uo *= 2.f;
        const float ze = fmaf(g, bv_sin_sq(a * ue), ue), zo = fmaf(g, bv_sin_sq(a * uo), uo);
        zs[(2 * qi) * CB + cl] = q >= len ? zo : ze;
        zs[(2 * qi + 1) * CB + cl] = q < 0 ? ze : zo;
    }
    __syncthreads();

    // y[t] = sum_j f[j] z[2 t + j - 5]: zs row 2 (t - t0) + j + 1
    constexpr int Y_IT = (BV_P + PG - 1) / PG;
#pragma unroll
    for (int it = 0; it < Y_IT; ++it) {
        const int t = t0 + pg + it * PG;
        if (t >= t_end) break;
        float y = 0.f;
        if (t < len) {
            const float* zw = &zs[(2 * (t - t0) + 1) * CB + cl];
#pragma unroll
            for (int j = 0; j < BV_TAPS; ++j) y = fmaf(f[j], zw[j * CB], y);
        }
        if (c_ok) p.out[(row + t) * p.C + c] = y;
    }
}

int bv_snake(const BvAct& p, int B, hipStream_t s) {
    int CB = 64;
    while (CB > 4 && CB / 2 >= p.C) CB /= 2;   // the power of two that covers a tensor of fewer than 64 channels
    const dim3 grid((unsigned)(((long)p.T * p.mul + BV_P - 1) / BV_P), (unsigned)((p.C + CB - 1) / CB), (unsigned)B);
    switch (CB) {
        case 64: bv_snake_kernel<64><<<grid, 256, 0, s>>>(p); break;
        case 32: bv_snake_kernel<32><<<grid, 256, 0, s>>>(p); break;
        case 16: bv_snake_kernel<16><<<grid, 256, 0, s>>>(p); break;
        case 8: bv_snake_kernel<8><<<grid, 256, 0, s>>>(p); break;
        default: bv_snake_kernel<4><<<grid, 256, 0, s>>>(p); break;
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// use_tanh_at_final = false: the waveform clamped to [-1, 1], in place; the zeros behind a row stay zeros
__global__ void __launch_bounds__(256) bv_clamp_kernel(float* wav, long count) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx < count) wav[idx] = fminf(fmaxf(wav[idx], -1.f), 1.f);
}

// ---- the blob: gvx_hifigan_pack_weights_device's, then the filter and every activation's a and g
struct BvBlob {
    size_t filter;
    size_t act[GVX_HIFIGAN_MAX_STAGES][GVX_HIFIGAN_MAX_RESBLOCKS][2 * GVX_HIFIGAN_MAX_DILATIONS][2];   // [stage][block][p][a / g]
    size_t post[2];
    size_t total;
};

inline int bv_acts_per_block(const gvx_hifigan_dims& d) { return d.n_dilations * hg_convs_per_dilation(d); }

BvBlob bv_blob_layout(const gvx_hifigan_dims& d) {
    BvBlob L{};
    size_t at = hg_blob_layout(d).total;
    auto take = [&](size_t floats) { const size_t o = at; at += gvx::round64(floats); return o; };
    L.filter = take(BV_TAPS);
    size_t C = d.upsample_initial_channel;
    for (int i = 0; i < d.n_stages; ++i) {
        C /= 2;
        for (int j = 0; j < d.n_resblocks; ++j)
            for (int q = 0; q < bv_acts_per_block(d); ++q)
                for (int v = 0; v < 2; ++v) L.act[i][j][q][v] = take(C);
    }
    for (int v = 0; v < 2; ++v) L.post[v] = take(C);
    L.total = at;
    return L;
}

const char* bv_dims_problem(const gvx_bigvgan_dims* d) {
    if (!d) return "null dims";
    if (const char* why = hg_dims_problem(&d->net)) return why;
    for (int v : {d->snakebeta, d->tanh_at_final, d->bias_at_final})
        if (v != 0 && v != 1) return "snakebeta, tanh_at_final and bias_at_final must be 0 or 1";
    return nullptr;
}

constexpr int BV_BUFS = 5;   // HiFi-GAN's four tensors of a stage and the activation's output

}  // namespace

extern "C" {

int gvx_snake_antialiased(const float* x, const int32_t* lens, int B, int n_max, int C, const float* f, const float* a, const float* g,
                          float* out, void* stream) {
    if (!x || !f || !a || !g || !out || x == out) return fail(GVX_ERR_INVALID_ARG, "null argument, or out is x");
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (n_max < 1 || n_max > GVX_BIGVGAN_ACT_MAX_POSITIONS || C < 1)
        return fail(GVX_ERR_INVALID_ARG, "n_max must be in [1, %d] and C >= 1", (int)GVX_BIGVGAN_ACT_MAX_POSITIONS);
    if ((C + 63) / 64 > 65535) return fail(GVX_ERR_INVALID_ARG, "C = %d is beyond the grid", C);
    BvAct p{};
    p.x = x; p.out = out; p.lens = lens; p.T = n_max; p.mul = 1; p.C = C; p.f = f; p.a = a; p.g = g;
    return bv_snake(p, B, (hipStream_t)stream);
}

size_t gvx_bigvgan_blob_floats(const gvx_bigvgan_dims* dims) {
    if (bv_dims_problem(dims)) return 0;
    return bv_blob_layout(dims->net).total;
}

size_t gvx_bigvgan_workspace_bytes(const gvx_bigvgan_dims* dims, int B, int T) {
    if (bv_dims_problem(dims) || B < 1 || T < 1 || T > GVX_HIFIGAN_MAX_FRAMES) return 0;
    return hg_ws_plan(dims->net, B, T, BV_BUFS).total;
}

int gvx_bigvgan_pack_weights_device(const gvx_bigvgan_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = bv_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_hifigan_dims& d = dims->net;
    const BvBlob L = bv_blob_layout(d);
    GenPacker P{{table, n}};
    P.take("filter", L.filter, BV_TAPS);
    size_t C = d.upsample_initial_channel;
    static const char* const part[2] = {".a", ".g"};
    for (int i = 0; i < d.n_stages; ++i) {
        C /= 2;
        for (int j = 0; j < d.n_resblocks; ++j)
            for (int q = 0; q < bv_acts_per_block(d); ++q)
                for (int v = 0; v < 2; ++v)
                    P.take("resblocks." + std::to_string(i * d.n_resblocks + j) + ".activations." + std::to_string(q) + part[v], L.act[i][j][q][v], C);
    }
    for (int v = 0; v < 2; ++v) P.take(std::string("activation_post") + part[v], L.post[v], C);
    if (P.rc != GVX_OK) return P.rc;
    // the convolutions: HiFi-GAN's packer, which refuses before it launches and clears its own part of the blob
    if (const int rc = gvx_hifigan_pack_weights_device(&d, table, n, device_blob, stream)) return rc;
    return P.run(device_blob, hg_blob_layout(d).total, L.total, (hipStream_t)stream);
}

int gvx_bigvgan_create(const gvx_bigvgan_dims* dims, gvx_bigvgan** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = bv_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_bigvgan* h = new gvx_bigvgan();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_bigvgan_destroy(gvx_bigvgan* h) { delete h; }

int gvx_bigvgan_bind(gvx_bigvgan* h, const float* device_blob) { return gen_bind(h, device_blob); }

int gvx_bigvgan_timing_enable(gvx_bigvgan* h, int enable) { return gen_timing_enable(h, enable, h ? h->d.net.n_stages + 3 : 0); }

int gvx_bigvgan_stage_times_ms(gvx_bigvgan* h, float* ms_out, int* n_out) { return gen_stage_times_ms(h, h ? h->d.net.n_stages + 2 : 0, ms_out, n_out); }

int gvx_bigvgan_forward(gvx_bigvgan* h, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, float* const* stage_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_hifigan_dims& d = h->d.net;
    hipStream_t s = (hipStream_t)stream;
    const HgWs wp = hg_ws_plan(d, B, T, BV_BUFS);
    const BvBlob A = bv_blob_layout(d);
    // A in front of every convolution but conv_pre and ups: one launch into the fifth tensor, which the convolution then reads as it is
    const HgFront front = [&](const HgAt& at, HgLayer& p) -> int {
        if (at.site == HG_PRE || at.site == HG_UPS) return GVX_OK;
        if (at.site == HG_POST) p.tanh_out = h->d.tanh_at_final;
        const size_t* ag = at.site == HG_POST ? A.post : A.act[at.stage][at.block][at.act];
        BvAct a{};
        a.x = p.src; a.out = gvx::ws_ptr<float>(workspace, wp.buf[4]); a.lens = frame_lengths; a.T = T; a.mul = p.in_mul; a.C = p.Cin;
        a.f = h->blob + A.filter; a.a = h->blob + ag[0]; a.g = h->blob + ag[1];
        p.src = a.out;
        return bv_snake(a, B, s);
    };
    int rc;
    if ((rc = hg_forward(h, &h->lds_ready, d, wp, front, mel, frame_lengths, B, T, wav_out, stage_out, workspace, workspace_bytes, s)) != GVX_OK) return rc;
    if (!h->d.tanh_at_final) {
        long count = (long)B * T;
        for (int i = 0; i < d.n_stages; ++i) count *= d.upsample_rates[i];
        bv_clamp_kernel<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(wav_out, count);
        HIP_TRY(hipGetLastError());
    }
    return gen_mark(h, d.n_stages + 2, s);
}

}  // C ABI
