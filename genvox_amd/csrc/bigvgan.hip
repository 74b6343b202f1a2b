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

struct gvx_bigvgan {
    gvx_bigvgan_dims d;
    const float* blob = nullptr;
    gvx_hifigan core;   // what hg_prepare and the timing keep per handle: the dynamic-LDS flag and the events
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
    const int len = hg_frames(p.lens, b, p.T) * p.mul;
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
    auto take = [&](size_t floats) { const size_t o = at; at += hg_round64(floats); return o; };
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

size_t bv_widest(const gvx_hifigan_dims& d) {   // floats per frame of the widest activation tensor
    size_t widest = d.upsample_initial_channel, mul = 1, C = d.upsample_initial_channel;
    for (int i = 0; i < d.n_stages; ++i) {
        mul *= d.upsample_rates[i];
        C /= 2;
        widest = std::max(widest, mul * C);
    }
    return widest;
}

constexpr int BV_BUFS = 5;   // HiFi-GAN's four tensors of a stage and the activation's output
struct BvWs { size_t mel_t, buf[BV_BUFS], total; };

BvWs bv_ws_plan(const gvx_hifigan_dims& d, int B, int T) {
    BvWs w{};
    size_t at = 0;
    w.mel_t = at;
    at += (size_t)B * hg_round256((size_t)T * hg_cpad(d) * sizeof(float));
    for (int i = 0; i < BV_BUFS; ++i) {
        w.buf[i] = at;
        at += (size_t)B * hg_round256((size_t)T * bv_widest(d) * sizeof(float));
    }
    w.total = at;
    return w;
}

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
    return bv_ws_plan(dims->net, B, T).total;
}

int gvx_bigvgan_pack_weights_device(const gvx_bigvgan_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = bv_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_hifigan_dims& d = dims->net;
    const BvBlob L = bv_blob_layout(d);
    hipStream_t s = (hipStream_t)stream;
    struct Job { size_t dst; const float* src; size_t numel; };
    std::vector<Job> jobs;
    auto take = [&](const std::string& name, size_t dst, size_t numel) -> int {
        for (int i = 0; i < n; ++i)
            if (table[i].name && name == table[i].name) {
                if (!table[i].data || table[i].numel != (int64_t)numel)
                    return fail(GVX_ERR_SHAPE, "%s has %lld elements, the dims ask for %zu", name.c_str(), (long long)table[i].numel, numel);
                jobs.push_back({dst, table[i].data, numel});
                return GVX_OK;
            }
        return fail(GVX_ERR_MISSING_WEIGHT, "%s is missing", name.c_str());
    };
    int rc;
    if ((rc = take("filter", L.filter, BV_TAPS)) != GVX_OK) return rc;
    size_t C = d.upsample_initial_channel;
    static const char* const part[2] = {".a", ".g"};
    for (int i = 0; i < d.n_stages; ++i) {
        C /= 2;
        for (int j = 0; j < d.n_resblocks; ++j)
            for (int q = 0; q < bv_acts_per_block(d); ++q)
                for (int v = 0; v < 2; ++v) {
                    const std::string name = "resblocks." + std::to_string(i * d.n_resblocks + j) + ".activations." + std::to_string(q) + part[v];
                    if ((rc = take(name, L.act[i][j][q][v], C)) != GVX_OK) return rc;
                }
    }
    for (int v = 0; v < 2; ++v)
        if ((rc = take(std::string("activation_post") + part[v], L.post[v], C)) != GVX_OK) return rc;
    // the convolutions: HiFi-GAN's packer, which refuses before it launches and clears its own part of the blob
    if ((rc = gvx_hifigan_pack_weights_device(&d, table, n, device_blob, stream)) != GVX_OK) return rc;
    const size_t base = hg_blob_layout(d).total;
    HIP_TRY(hipMemsetAsync(device_blob + base, 0, (L.total - base) * sizeof(float), s));   // the padding between the tensors
    for (const Job& j : jobs) HIP_TRY(hipMemcpyAsync(device_blob + j.dst, j.src, j.numel * sizeof(float), hipMemcpyDeviceToDevice, s));
    return GVX_OK;
}

int gvx_bigvgan_create(const gvx_bigvgan_dims* dims, gvx_bigvgan** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = bv_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_bigvgan* h = new gvx_bigvgan();
    h->d = *dims;
    h->core.d = dims->net;
    *out = h;
    return GVX_OK;
}

void gvx_bigvgan_destroy(gvx_bigvgan* h) {
    if (!h) return;
    for (int i = 0; i < h->core.n_ev; ++i) (void)hipEventDestroy(h->core.ev[i]);
    delete h;
}

int gvx_bigvgan_bind(gvx_bigvgan* h, const float* device_blob) {
    if (!h || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if ((uintptr_t)device_blob % 256) return fail(GVX_ERR_INVALID_ARG, "the blob must be 256-byte aligned");
    h->blob = device_blob;
    return GVX_OK;
}

int gvx_bigvgan_timing_enable(gvx_bigvgan* h, int enable) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const int need = h->d.net.n_stages + 3;
    while (enable && h->core.n_ev < need) HIP_TRY(hipEventCreate(&h->core.ev[h->core.n_ev++]));
    h->core.timing = enable != 0;
    return GVX_OK;
}

int gvx_bigvgan_stage_times_ms(gvx_bigvgan* h, float* ms_out, int* n_out) {
    if (!h || !ms_out || !n_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->core.timing) return fail(GVX_ERR_STATE, "timing is not enabled");
    const int n = h->d.net.n_stages + 2;
    HIP_TRY(hipEventSynchronize(h->core.ev[n]));
    for (int i = 0; i < n; ++i) HIP_TRY(hipEventElapsedTime(&ms_out[i], h->core.ev[i], h->core.ev[i + 1]));
    *n_out = n;
    return GVX_OK;
}

int gvx_bigvgan_forward(gvx_bigvgan* h, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, float* const* stage_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !mel || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    const gvx_hifigan_dims& d = h->d.net;
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (T < 1) return fail(GVX_ERR_INVALID_ARG, "T = %d: a row needs at least 1 frame", T);
    if (T > GVX_HIFIGAN_MAX_FRAMES) return fail(GVX_ERR_UNSUPPORTED, "T = %d is beyond the limit of %d frames", T, GVX_HIFIGAN_MAX_FRAMES);
    const BvWs wp = bv_ws_plan(d, B, T);
    if (!workspace || (uintptr_t)workspace % 256 || workspace_bytes < wp.total)
        return fail(GVX_ERR_WORKSPACE, "the workspace is missing, misaligned or smaller than %zu bytes", wp.total);
    if (stage_out)
        for (int i = 0; i < d.n_stages; ++i)
            if (!stage_out[i] || (uintptr_t)stage_out[i] % 16) return fail(GVX_ERR_INVALID_ARG, "stage_out[%d] is null or not 16-byte aligned", i);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = hg_prepare(&h->core)) != GVX_OK) return rc;
    const HgBlob L = hg_blob_layout(d);
    const BvBlob A = bv_blob_layout(d);
    const float* blob = h->blob;
    float* pool[4];
    for (int i = 0; i < 4; ++i) pool[i] = gvx::ws_ptr<float>(workspace, wp.buf[i]);
    float* act = gvx::ws_ptr<float>(workspace, wp.buf[4]);   // A's output: written by one launch, read by the next
    int ev = 0;
    auto stamp = [&]() -> int {
        if (h->core.timing) HIP_TRY(hipEventRecord(h->core.ev[ev++], s));
        return GVX_OK;
    };
    if ((rc = stamp()) != GVX_OK) return rc;

    const int Cp = hg_cpad(d);
    float* mel_t = gvx::ws_ptr<float>(workspace, wp.mel_t);
    if ((rc = hg_mel_transpose(mel, frame_lengths, B, d.n_mels, T, Cp, mel_t, s)) != GVX_OK) return rc;
    auto layer = [&](const float* src, size_t w, size_t bias, float* out, int in_mul, int Cin, int Cout, int taps, int dil, int phases) {
        HgLayer p{};
        p.lens = frame_lengths; p.T = T;
        p.src = src; p.W = blob + w; p.bias = blob + bias; p.out = out;
        p.in_mul = in_mul; p.Cin = Cin; p.Cout = Cout; p.taps = taps; p.K = taps * Cin; p.dil = dil; p.phases = phases;
        return p;   // act = 0: the operand as it is
    };
    auto snake = [&](const float* src, const size_t* ag, int mul, int C) {   // act = A(src)
        BvAct p{};
        p.x = src; p.out = act; p.lens = frame_lengths; p.T = T; p.mul = mul; p.C = C;
        p.f = blob + A.filter; p.a = blob + ag[0]; p.g = blob + ag[1];
        return bv_snake(p, B, s);
    };
    int C = d.upsample_initial_channel, mul = 1;
    float* cur = pool[0];
    HgLayer p = layer(mel_t, L.pre_w, L.pre_b, cur, 1, Cp, C, 7, 1, 1);
    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
    if ((rc = stamp()) != GVX_OK) return rc;

    for (int i = 0; i < d.n_stages; ++i) {
        const int Cn = C / 2, r = d.upsample_rates[i];
        // the stage's tensors, as gvx_hifigan_forward assigns them: x, its sum, and a block's two
        float* rest[4];
        int n_rest = 0;
        for (float* c : pool)
            if (c != cur) rest[n_rest++] = c;
        float* x = rest[0];
        float* sum = stage_out ? stage_out[i] : rest[1];
        float* t0 = rest[2];
        float* t1 = n_rest == 3 ? cur : rest[1];
        p = layer(cur, L.up_w[i], L.up_b[i], x, mul, C, Cn, 2, 0, r);   // no activation in front of ups
        if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
        mul *= r;
        for (int j = 0; j < d.n_resblocks; ++j) {
            const int k = d.resblock_kernel_sizes[j];
            const float* in = x;   // the block's running value
            for (int m = 0; m < d.n_dilations; ++m) {
                const bool last = m == d.n_dilations - 1;
                const int dil = d.resblock_dilation_sizes[j][m];
                int conv_dil = dil, v = 0;
                float* next;
                if (d.resblock == 1) {   // t1 = convs1(A(in)); next = in + convs2(A(t1)): next may be `in` itself once that is t0
                    if ((rc = snake(in, A.act[i][j][2 * m], mul, Cn)) != GVX_OK) return rc;
                    p = layer(act, L.conv_w[i][j][m][0], L.conv_b[i][j][m][0], t1, mul, Cn, Cn, k, dil, 1);
                    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
                    if ((rc = snake(t1, A.act[i][j][2 * m + 1], mul, Cn)) != GVX_OK) return rc;
                    conv_dil = 1; v = 1;
                    next = t0;
                } else {                 // next = in + convs(A(in))
                    if ((rc = snake(in, A.act[i][j][m], mul, Cn)) != GVX_OK) return rc;
                    next = in == t0 ? t1 : t0;
                }
                p = layer(act, L.conv_w[i][j][m][v], L.conv_b[i][j][m][v], last ? sum : next, mul, Cn, Cn, k, conv_dil, 1);
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
        if ((rc = stamp()) != GVX_OK) return rc;
    }
    if ((rc = snake(cur, A.post, mul, C)) != GVX_OK) return rc;
    p = layer(act, L.post_w, L.post_b, wav_out, mul, C, 1, 7, 1, 1);
    p.tanh_out = h->d.tanh_at_final; p.zero_tail = 1;
    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
    if (!h->d.tanh_at_final) {
        const long count = (long)B * T * mul;
        bv_clamp_kernel<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(wav_out, count);
        HIP_TRY(hipGetLastError());
    }
    return stamp();
}

}  // C ABI
