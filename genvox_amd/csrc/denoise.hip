// Vocoder denoiser (include/genvox_amd.h, "Vocoder denoiser"): the STFT of a waveform, a gain per bin that takes strength x the
// vocoder's bias spectrum off every magnitude, and the inverse STFT with the phase kept.  dn_frame_kernel does everything of a frame in
// one wave: the samples gathered through the reflection and windowed, the real transform in LDS (fft_lds.h), magnitude and gain on the
// spectrum in registers, the inverse real transform and the window again; the windowed frame goes to the workspace and nothing of the
// spectrum does.  dn_gather_kernel is the overlap-add written as a gather: a thread per output sample sums the frames that cover it
// and the squared window under them, in ascending frame order, and divides.
// No atomics anywhere: two calls give the same bits, and a row's numbers never depend on another row's.
//
// Order of this file: kernels, workspace layout, the C ABI.
#include "fft_lds.h"
#include "stft_plan.h"

#include <algorithm>

using gvx::fail;
using namespace gvx_plan;

struct gvx_denoise_plan {
    int n_fft = 0, hop = 0;
    int pad = 0, n_min = 0;     // n_fft / 2; shortest legal row: pad + 1
    std::vector<float> host_tables;      // what create makes; the first call moves it to the device, so that a plan - and the
    float* tables = nullptr;             // workspace arithmetic with it - needs no device.  window [N], w_H^m [H], w_N^k [H + 1] as float2
    size_t tw_at = 0, tw2_at = 0;
};

namespace {

constexpr int DN_FRAMES = GVX_DENOISE_FRAMES_PER_WORKGROUP;   // frames (waves) per workgroup of the frame kernel
constexpr int DN_GATHER = GVX_DENOISE_GATHER_SAMPLES;         // output samples (threads) per workgroup of the gather

// ---- kernels ------------------------------------------------------------------------------------------------

struct DnArgs {
    const float* win; const float2* tw; const float2* tw2;
    const float* bias;    // [H + 1], or null: no gain
    float strength;
    int hop, f_max;       // frames of a row of n_max samples
    float* frames;        // windowed inverse frames [B][f_max][n_fft] (null: magnitudes alone)
    float* mag;           // [B][f_max][H + 1], or null
};

// a row the host refuses has no frames and no samples here: nothing of it is read, its outputs are zeros
__device__ __forceinline__ int dn_len(const int32_t* lens, int b, long n_max, int n_min) {
    const long n = lens ? (long)lens[b] : n_max;
    return n < n_min || n > n_max ? 0 : (int)n;
}

__device__ __forceinline__ int dn_reflect(int i, int nb) {
    i = i < 0 ? -i : i;
    return i >= nb ? 2 * (nb - 1) - i : i;
}

template <int H>
__global__ __launch_bounds__(DN_FRAMES * 64) void dn_frame_kernel(const float* __restrict__ wav, const int32_t* __restrict__ lens, long n_max,
                                                                  DnArgs p) {
    constexpr int Q = H / 64, N = 2 * H;
    __shared__ __attribute__((aligned(16))) float2 fsm[DN_FRAMES * fft_lds_words<H>()];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t = (int)blockIdx.x * DN_FRAMES + wave;
    const int nb = dn_len(lens, b, n_max, H + 1);
    const int F = nb ? 1 + nb / p.hop : 0;
    if (t >= p.f_max) return;
    const long f = (long)b * p.f_max + t;
    if (t >= F) {   // behind the row's frames: the magnitudes are zeros there, and no frame is read by the gather
        if (p.mag)
            for (int k = j; k <= H; k += 64) p.mag[f * (H + 1) + k] = 0.f;
        return;
    }
    float2* buf = fsm + wave * fft_lds_words<H>();
    const float* x = wav + (long)b * n_max;
    const int i0 = t * p.hop - H;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int m = j + 64 * q;
        const float2 w = *reinterpret_cast<const float2*>(p.win + 2 * m);
        buf[fpad(m)] = make_float2(w.x * x[dn_reflect(i0 + 2 * m, nb)], w.y * x[dn_reflect(i0 + 2 * m + 1, nb)]);
    }
    wave_lds_fence();
    fft_lds_wave<H, false>(buf, p.tw, j);
    float2 ys[Q + 1];
#pragma unroll
    for (int q = 0; q <= Q; ++q) {
        const int k = j + 64 * q;
        if (k <= H) {
            float2 X = rfft_split(buf[fpad(k & (H - 1))], buf[fpad((H - k) & (H - 1))], p.tw2[k], k == 0 || k == H);
            const float M = sqrtf(X.x * X.x + X.y * X.y);
            if (p.mag) p.mag[f * (H + 1) + k] = M;
            const float a = p.bias ? p.strength * p.bias[k] : 0.f;
            if (a != 0.f) {   // a == 0 leaves X as it is, bit for bit
                const float g = M > 0.f ? fmaxf(0.f, M - a) / M : 0.f;
                X = make_float2(X.x * g, X.y * g);
            }
            ys[q] = X;
        }
    }
    if (!p.frames) return;
    // ---- inverse: Y_k and Y_{H-k} meet through this wave's LDS row, unpadded at [k], k = 0 .. H (all reads of the transform are done)
    wave_lds_fence();
#pragma unroll
    for (int q = 0; q <= Q; ++q) {
        const int k = j + 64 * q;
        if (k <= H) buf[k] = ys[q];
    }
    wave_lds_fence();
    float2 z[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int k = j + 64 * q;
        z[q] = irfft_pack(ys[q], buf[H - k], p.tw2[k], k == 0);   // at k = 0 the partner is the Nyquist bin
    }
    wave_lds_fence();
#pragma unroll
    for (int q = 0; q < Q; ++q) buf[fpad(j + 64 * q)] = z[q];
    wave_lds_fence();
    fft_lds_wave<H, true>(buf, p.tw, j);
    float* g = p.frames + f * N;
    const float inv_n = 1.f / (float)N;   // a power of two: exact
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int m = j + 64 * q;
        const float2 v = buf[fpad(m)];
        const float2 w = *reinterpret_cast<const float2*>(p.win + 2 * m);
        *reinterpret_cast<float2*>(g + 2 * m) = make_float2(w.x * (v.x * inv_n), w.y * (v.y * inv_n));
    }
}

// overlap-add as a gather: a thread per sample of out sums, over the row's frames that cover its padded position p = i + pad in
// ascending frame order, the windowed inverse frames and the squared window, and divides.  Exact zeros at and behind the row's length
__global__ __launch_bounds__(DN_GATHER) void dn_gather_kernel(const int32_t* __restrict__ lens, long n_max, const float* __restrict__ frames,
                                                              const float* __restrict__ win, int N, int hop, int f_max, float* __restrict__ out) {
    const long i_long = (long)blockIdx.x * DN_GATHER + threadIdx.x;
    const int b = blockIdx.y;
    if (i_long >= n_max) return;
    const int i = (int)i_long;
    const int nb = dn_len(lens, b, n_max, N / 2 + 1);
    float r = 0.f;
    if (i < nb) {
        const int F = 1 + nb / hop;
        const float* g = frames + (long)b * f_max * N;
        const int p = i + N / 2;
        const int t_lo = p >= N ? (p - N) / hop + 1 : 0;
        const int t_hi = min(F - 1, p / hop);
        float num = 0.f, den = 0.f;
        for (int t = t_lo; t <= t_hi; ++t) {
            const int o = p - t * hop;
            const float w = win[o];
            num += g[(long)t * N + o];
            den += w * w;
        }
        r = num / den;
    }
    out[(long)b * n_max + i] = r;
}

// ---- workspace layout ---------------------------------------------------------------------------------------

struct DnLayout {
    int f_max, nwg;
    size_t frames, total;
};

DnLayout dn_layout(const gvx_denoise_plan* p, int B, long n_max) {
    DnLayout L{};
    L.f_max = (int)(1 + n_max / p->hop);
    L.nwg = (L.f_max + DN_FRAMES - 1) / DN_FRAMES;
    StftRegions ws;
    L.frames = ws.take((size_t)B * L.f_max * p->n_fft * sizeof(float));
    L.total = ws.total;
    return L;
}

const char* dn_shape_problem(const gvx_denoise_plan* p, int B, long n_max) {
    if (!p) return "null plan";
    if (B < 1 || B > GVX_DENOISE_MAX_ROWS) return "B must be in [1, GVX_DENOISE_MAX_ROWS]";
    if (n_max < 1 || n_max > GVX_DENOISE_MAX_SAMPLES) return "n_max must be in [1, GVX_DENOISE_MAX_SAMPLES]";
    return nullptr;
}

}  // namespace

extern "C" {

int gvx_denoise_create(int n_fft, int hop, gvx_denoise_plan** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_fft != 512 && n_fft != 1024 && n_fft != 2048) return fail(GVX_ERR_UNSUPPORTED, "n_fft = %d, supported are 512, 1024 and 2048", n_fft);
    if (hop < 1 || hop > n_fft / 2) return fail(GVX_ERR_INVALID_ARG, "hop = %d is outside [1, n_fft / 2 = %d]", hop, n_fft / 2);
    gvx_denoise_plan* p = new gvx_denoise_plan();
    p->n_fft = n_fft; p->hop = hop; p->pad = n_fft / 2; p->n_min = n_fft / 2 + 1;
    const StftTables t = stft_tables(p->host_tables, n_fft, n_fft);   // the window first: t.win = 0
    p->tw_at = t.tw; p->tw2_at = t.tw2;
    *out = p;
    return GVX_OK;
}

void gvx_denoise_destroy(gvx_denoise_plan* p) {
    if (!p) return;
    if (p->tables) (void)hipFree(p->tables);
    delete p;
}

size_t gvx_denoise_workspace_bytes(const gvx_denoise_plan* p, int B, long n_max) {
    if (const char* why = dn_shape_problem(p, B, n_max)) { (void)fail(GVX_ERR_INVALID_ARG, "%s", why); return 0; }
    return dn_layout(p, B, n_max).total;
}

int gvx_denoise(gvx_denoise_plan* p, const float* wav, const int32_t* sample_lengths, int B, long n_max, const float* bias, float strength,
                float* out, float* mag_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (const char* why = dn_shape_problem(p, B, n_max)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!wav) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!out && !mag_out) return fail(GVX_ERR_INVALID_ARG, "out and mag_out are both null: nothing to compute");
    if (!std::isfinite(strength) || strength < 0.f) return fail(GVX_ERR_INVALID_ARG, "strength must be finite and >= 0");
    if (strength > 0.f && !bias) return fail(GVX_ERR_INVALID_ARG, "strength = %g needs a bias spectrum", (double)strength);
    if (n_max < p->n_min) return fail(GVX_ERR_SHAPE, "n_max = %ld: a row needs at least n_fft / 2 + 1 = %d samples for the reflection", n_max, p->n_min);
    const DnLayout L = dn_layout(p, B, n_max);
    if (const int rc = stft_check_workspace(workspace, workspace_bytes, L.total)) return rc;
    if (!p->tables && !stft_upload(&p->tables, p->host_tables)) return fail(GVX_ERR_HIP, "window and twiddle table allocation failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(workspace);
    DnArgs a{};
    a.win = p->tables;
    a.tw = reinterpret_cast<const float2*>(p->tables + p->tw_at);
    a.tw2 = reinterpret_cast<const float2*>(p->tables + p->tw2_at);
    a.bias = strength > 0.f ? bias : nullptr;
    a.strength = strength;
    a.hop = p->hop; a.f_max = L.f_max;
    a.frames = out ? reinterpret_cast<float*>(ws + L.frames) : nullptr;
    a.mag = mag_out;
    const int rc = stft_dispatch(p->n_fft, [&](auto h) -> int {
        dn_frame_kernel<decltype(h)::value><<<dim3((unsigned)L.nwg, (unsigned)B), DN_FRAMES * 64, 0, s>>>(wav, sample_lengths, n_max, a);
        HIP_TRY(hipGetLastError());
        return GVX_OK;
    });
    if (rc != GVX_OK) return rc;
    if (out) {
        dn_gather_kernel<<<dim3((unsigned)((n_max + DN_GATHER - 1) / DN_GATHER), (unsigned)B), DN_GATHER, 0, s>>>(sample_lengths, n_max, a.frames, a.win,
                                                                                                                p->n_fft, p->hop, L.f_max, out);
        HIP_TRY(hipGetLastError());
    }
    return stft_check_lengths(sample_lengths, B, n_max, p->n_min, "n_fft / 2 + 1", nullptr, s);
}

}  // extern "C"
