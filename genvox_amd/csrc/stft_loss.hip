// Multi-resolution STFT loss of a predicted waveform against its target, value and gradient (include/genvox_amd.h, "Multi-resolution
// STFT loss").  Per resolution: sl_forward_kernel frames both signals through the reflection at the row's own length, transforms a
// frame per wave in LDS (fft_lds.h), takes magnitudes and leaves the three sums of its workgroup; sl_reduce_kernel adds the partial
// sums of every (row, resolution) in a fixed order and makes the loss, its parts and the two gradient coefficients of the pair;
// sl_grad_kernel turns the kept spectrum of pred into dL/dX, applies the adjoint of the real transform and the window; and
// sl_gather_kernel sums, per output sample, the frames of every resolution that cover the sample and its two reflected images.
// No atomics anywhere: two calls give the same bits, and a row's numbers never depend on another row's.
//
// Order of this file: kernels, workspace layout, the C ABI.
#include "fft_lds.h"
#include "stft_plan.h"

#include <algorithm>

using gvx::fail;
using namespace gvx_plan;

struct gvx_stft_loss_plan {
    int R = 0;
    gvx_stft_resolution res[GVX_STFT_LOSS_MAX_RESOLUTIONS] = {};
    float w_sc = 1.f, w_mag = 1.f, eps = 1e-7f;
    int n_min = 0;              // shortest legal row: n_fft_max / 2 + 1
    float* tables = nullptr;    // device, per resolution: window [N], w_H^m [H] and w_N^k [H + 1] as float2
    size_t win_at[GVX_STFT_LOSS_MAX_RESOLUTIONS] = {}, tw_at[GVX_STFT_LOSS_MAX_RESOLUTIONS] = {}, tw2_at[GVX_STFT_LOSS_MAX_RESOLUTIONS] = {};
};

namespace {

constexpr int SL_FRAMES = GVX_STFT_LOSS_FRAMES_PER_WORKGROUP;   // frames (waves) per workgroup of the forward and gradient kernels
constexpr int SL_GATHER = GVX_STFT_LOSS_GATHER_SAMPLES;         // output samples (threads) per workgroup of the gather
constexpr int SL_MAX_R = GVX_STFT_LOSS_MAX_RESOLUTIONS;

// ---- kernels ------------------------------------------------------------------------------------------------

struct SlRes {   // one resolution of one call
    const float* win; const float2* tw; const float2* tw2;
    int hop, r, R;
    int f_max, nwg;       // frames of a row of n_max samples, workgroups per row
    float2* X; float* Mt; float* g;   // kept spectrum of pred, magnitudes of target, frame gradients (all null: forward only)
    double* part;         // [B][nwg][3]
    float* dbg_p; float* dbg_t;
};

// a row the host refuses has no frames and no samples here: nothing of it is read, its gradient is zeros
__device__ __forceinline__ int sl_len(const int32_t* lens, int b, long n_max, int n_min) {
    const long n = lens ? (long)lens[b] : n_max;
    return n < n_min || n > n_max ? 0 : (int)n;
}

__device__ __forceinline__ int sl_reflect(int i, int nb) {
    i = i < 0 ? -i : i;
    return i >= nb ? 2 * (nb - 1) - i : i;
}

template <int H>
__global__ __launch_bounds__(SL_FRAMES * 64) void sl_forward_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                    const int32_t* __restrict__ lens, long n_max, int n_min, float eps, SlRes p) {
    constexpr int Q = H / 64, BINS = H + 1;
    __shared__ __attribute__((aligned(16))) float2 fsm[SL_FRAMES * fft_lds_words<H>()];
    __shared__ double wsum[SL_FRAMES][3];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t = (int)blockIdx.x * SL_FRAMES + wave;
    const int nb = sl_len(lens, b, n_max, n_min);
    const int F = nb ? 1 + nb / p.hop : 0;
    if ((int)blockIdx.x * SL_FRAMES >= F && !p.dbg_p && !p.dbg_t) return;   // the whole workgroup lies behind the row's frames
    float2* buf = fsm + wave * fft_lds_words<H>();
    const long f = (long)b * p.f_max + t;
    float sd = 0.f, st = 0.f, sl = 0.f;
    if (t < F) {
        float mp[Q + 1];
#pragma unroll
        for (int sig = 0; sig < 2; ++sig) {
            const float* x = (sig ? target : pred) + (long)b * n_max;
            const int i0 = t * p.hop - H;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int m = j + 64 * q;
                const float2 w = *reinterpret_cast<const float2*>(p.win + 2 * m);
                buf[fpad(m)] = make_float2(w.x * x[sl_reflect(i0 + 2 * m, nb)], w.y * x[sl_reflect(i0 + 2 * m + 1, nb)]);
            }
            wave_lds_fence();
            fft_lds_wave<H, false>(buf, p.tw, j);
#pragma unroll
            for (int q = 0; q <= Q; ++q) {
                const int k = j + 64 * q;
                if (k <= H) {
                    const float2 X = rfft_split(buf[fpad(k & (H - 1))], buf[fpad((H - k) & (H - 1))], p.tw2[k], k == 0 || k == H);
                    const float P = X.x * X.x + X.y * X.y;
                    const float M = sqrtf(fmaxf(P, eps));
                    if (sig == 0) {
                        mp[q] = M;
                        if (p.X) p.X[f * BINS + k] = X;
                        if (p.dbg_p) p.dbg_p[f * BINS + k] = M;
                    } else {
                        if (p.Mt) p.Mt[f * BINS + k] = M;
                        if (p.dbg_t) p.dbg_t[f * BINS + k] = M;
                        const float d = M - mp[q];
                        sd += d * d;
                        st += M * M;
                        sl += fabsf(logf(M) - logf(mp[q]));
                    }
                }
            }
            wave_lds_fence();
        }
    } else if (t < p.f_max) {
        const float nan = __uint_as_float(0x7fc00000u);
        for (int k = j; k < BINS; k += 64) {
            if (p.dbg_p) p.dbg_p[f * BINS + k] = nan;
            if (p.dbg_t) p.dbg_t[f * BINS + k] = nan;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        sd += __shfl_xor(sd, off);
        st += __shfl_xor(st, off);
        sl += __shfl_xor(sl, off);
    }
    if (j == 0) { wsum[wave][0] = (double)sd; wsum[wave][1] = (double)st; wsum[wave][2] = (double)sl; }
    __syncthreads();
    if (tid < 3 && (int)blockIdx.x * SL_FRAMES < F) {
        double s = 0.0;
        for (int w = 0; w < SL_FRAMES; ++w) s += wsum[w][tid];
        p.part[((long)b * p.nwg + blockIdx.x) * 3 + tid] = s;
    }
}

struct SlReduce {
    const double* part[SL_MAX_R];
    int nwg[SL_MAX_R], hop[SL_MAX_R], bins[SL_MAX_R];
    int R, B;
    float w_sc, w_mag;
    float* parts;     // [B][R][2] or null
    float2* coef;     // [B][R]: the factors of (M_p - M_t) and of sign / M_p in dL/dM_p
    double* terms;    // [B][R]
    float* loss;
};

// one workgroup: a wave per (row, resolution) adds the pair's partial sums (lane-strided, then a butterfly: a fixed order), then one
// thread adds the pairs' terms in order.  float64 here, in this one small kernel: the sums run over up to millions of bins
__global__ __launch_bounds__(256) void sl_reduce_kernel(const int32_t* __restrict__ lens, long n_max, int n_min, SlReduce q) {
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pairs = q.B * q.R;
    for (int pr = wave; pr < pairs; pr += 4) {
        const int b = pr / q.R, r = pr - b * q.R;
        const int nb = sl_len(lens, b, n_max, n_min);
        const int F = nb ? 1 + nb / q.hop[r] : 0;
        const int nw = (F + SL_FRAMES - 1) / SL_FRAMES;
        const double* part = q.part[r] + (long)b * q.nwg[r] * 3;
        double sd = 0.0, st = 0.0, sl = 0.0;
        for (int w = j; w < nw; w += 64) { sd += part[3 * w]; st += part[3 * w + 1]; sl += part[3 * w + 2]; }
        for (int off = 32; off >= 1; off >>= 1) {
            sd += __shfl_xor(sd, off);
            st += __shfl_xor(st, off);
            sl += __shfl_xor(sl, off);
        }
        if (j == 0) {
            const double nan = __longlong_as_double(0x7ff8000000000000LL);
            const double count = (double)F * (double)q.bins[r];
            const double nd = sqrt(sd), nt = sqrt(st);
            const double sc = F ? nd / nt : nan, mag = F ? sl / count : nan;
            const double share = 1.0 / ((double)q.B * (double)q.R);
            q.terms[pr] = (double)q.w_sc * sc + (double)q.w_mag * mag;
            q.coef[pr] = make_float2(F && sd > 0.0 ? (float)((double)q.w_sc * share / (nd * nt)) : 0.f,
                                     F ? (float)((double)q.w_mag * share / count) : 0.f);
            if (q.parts) { q.parts[2 * pr] = (float)sc; q.parts[2 * pr + 1] = (float)mag; }
        }
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int pr = 0; pr < pairs; ++pr) s += q.terms[pr];
        *q.loss = (float)(s / (double)pairs);
    }
}

// dL/dX of a frame from the kept spectrum, the adjoint of the real transform, the window.  The forward is X_k = sum_n x_n w_N^{kn}
// on bins 0 .. H, so dL/dx_n = sum_{k = 0}^{H} Re(G_k conj(w_N^{kn})): the unnormalised complex-to-real inverse of Y with
// Y_0 = Re G_0, Y_H = Re G_H and Y_k = G_k / 2 between them (that inverse counts the interior bins twice).  The inverse itself is a
// complex inverse of H points: Z_k = (Y_k + conj Y_{H-k}) + i conj(w_N^k) (Y_k - conj Y_{H-k}), z_m = x_{2m} + i x_{2m+1}; a lane
// makes Z_k and Z_{H-k} together from the same two bins
template <int H>
__global__ __launch_bounds__(SL_FRAMES * 64) void sl_grad_kernel(const int32_t* __restrict__ lens, long n_max, int n_min, float eps,
                                                                 const float2* __restrict__ coef, SlRes p) {
    constexpr int Q = H / 64, BINS = H + 1, N = 2 * H;
    __shared__ __attribute__((aligned(16))) float2 fsm[SL_FRAMES * fft_lds_words<H>()];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t = (int)blockIdx.x * SL_FRAMES + wave;
    const int nb = sl_len(lens, b, n_max, n_min);
    const int F = nb ? 1 + nb / p.hop : 0;
    if (t >= F) return;
    float2* buf = fsm + wave * fft_lds_words<H>();
    const long f = (long)b * p.f_max + t;
    const float2 ac = coef[b * p.R + p.r];
    const float2* X = p.X + f * BINS;
    const float* Mt = p.Mt + f * BINS;
    auto ybin = [&](int k) -> float2 {
        const float2 x = X[k];
        const float P = x.x * x.x + x.y * x.y;
        const float mp = sqrtf(fmaxf(P, eps)), mt = Mt[k];
        const float sgn = (float)((mt > mp) - (mt < mp));                  // sign(log M_t - log M_p): the logarithm is monotone
        const float gm = ac.x * (mp - mt) - ac.y * sgn / mp;               // dL/dM_p
        float scale = P < eps ? 0.f : gm / mp;                             // the clamp passes no gradient
        const bool end = k == 0 || k == H;
        if (!end) scale *= 0.5f;
        return make_float2(x.x * scale, end ? 0.f : x.y * scale);
    };
#pragma unroll
    for (int q = 0; q <= Q / 2; ++q) {
        const int k = j + 64 * q;
        if (k <= H / 2) {
            const float2 ya = ybin(k), yb = ybin(H - k);
            const float2 e = make_float2(ya.x + yb.x, ya.y - yb.y), d = make_float2(ya.x - yb.x, ya.y + yb.y);
            const float2 w = p.tw2[k];
            const float2 o = cmul(make_float2(w.x, -w.y), d);
            buf[fpad(k)] = make_float2(e.x - o.y, e.y + o.x);
            if (k != 0 && k != H / 2) buf[fpad(H - k)] = make_float2(e.x + o.y, o.x - e.y);
        }
    }
    wave_lds_fence();
    fft_lds_wave<H, true>(buf, p.tw, j);
    float* g = p.g + f * N;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int m = j + 64 * q;
        const float2 z = buf[fpad(m)];
        const float2 w = *reinterpret_cast<const float2*>(p.win + 2 * m);
        *reinterpret_cast<float2*>(g + 2 * m) = make_float2(w.x * z.x, w.y * z.y);
    }
}

struct SlGather {
    const float* g[SL_MAX_R];
    int n_fft[SL_MAX_R], hop[SL_MAX_R], f_max[SL_MAX_R];
    int R;
};

// overlap-add as a gather, the transpose of the framing: a thread per sample of d_pred sums the frame gradients at the padded
// positions that read the sample - its own, p = i + H, and its images under the left and right reflection - over the frames that
// cover each, in ascending frame order; the resolutions are added in their order.  Exact zeros at and behind the row's length
__global__ __launch_bounds__(SL_GATHER) void sl_gather_kernel(const int32_t* __restrict__ lens, long n_max, int n_min, SlGather q,
                                                              float* __restrict__ d_pred) {
    const long i_long = (long)blockIdx.x * SL_GATHER + threadIdx.x;
    const int b = blockIdx.y;
    if (i_long >= n_max) return;
    const int i = (int)i_long;
    const int nb = sl_len(lens, b, n_max, n_min);
    float acc = 0.f;
    if (i < nb) {
        for (int r = 0; r < q.R; ++r) {
            const int N = q.n_fft[r], H = N / 2, hop = q.hop[r];
            const int F = 1 + nb / hop;
            const float* g = q.g[r] + (long)b * q.f_max[r] * N;
            float s = 0.f;
#pragma unroll
            for (int img = 0; img < 3; ++img) {
                const int p = img == 0 ? i + H : (img == 1 ? H - i : 2 * (nb - 1) - i + H);
                const bool ok = img == 0 || (img == 1 ? (i >= 1 && i <= H) : (i <= nb - 2 && i >= nb - 1 - H));
                if (ok) {
                    const int t_lo = p >= N ? (p - N) / hop + 1 : 0;
                    const int t_hi = min(F - 1, p / hop);
                    for (int t = t_lo; t <= t_hi; ++t) s += g[(long)t * N + (p - t * hop)];
                }
            }
            acc += s;
        }
    }
    d_pred[(long)b * n_max + i] = acc;
}

// ---- workspace layout ---------------------------------------------------------------------------------------

struct SlLayout {
    int f_max[SL_MAX_R], nwg[SL_MAX_R];
    size_t X[SL_MAX_R], Mt[SL_MAX_R], g[SL_MAX_R], part[SL_MAX_R];
    size_t coef, terms, total;
};

SlLayout sl_layout(const gvx_stft_loss_plan* p, int B, long n_max) {
    SlLayout L{};
    StftRegions ws;
    for (int r = 0; r < p->R; ++r) {
        const size_t N = (size_t)p->res[r].n_fft, bins = N / 2 + 1;
        L.f_max[r] = (int)(1 + n_max / p->res[r].hop);
        L.nwg[r] = (L.f_max[r] + SL_FRAMES - 1) / SL_FRAMES;
        const size_t frames = (size_t)B * L.f_max[r];
        L.X[r] = ws.take(frames * bins * sizeof(float2));
        L.Mt[r] = ws.take(frames * bins * sizeof(float));
        L.g[r] = ws.take(frames * N * sizeof(float));
        L.part[r] = ws.take((size_t)B * L.nwg[r] * 3 * sizeof(double));
    }
    L.coef = ws.take((size_t)B * p->R * sizeof(float2));
    L.terms = ws.take((size_t)B * p->R * sizeof(double));
    L.total = ws.total;
    return L;
}

const char* sl_shape_problem(const gvx_stft_loss_plan* p, int B, long n_max) {
    if (!p) return "null plan";
    if (B < 1 || B > GVX_STFT_LOSS_MAX_ROWS) return "B must be in [1, GVX_STFT_LOSS_MAX_ROWS]";
    if (n_max < 1 || n_max > GVX_STFT_LOSS_MAX_SAMPLES) return "n_max must be in [1, GVX_STFT_LOSS_MAX_SAMPLES]";
    return nullptr;
}

}  // namespace

extern "C" {

int gvx_stft_loss_create(const gvx_stft_resolution* res, int R, float w_sc, float w_mag, float eps, gvx_stft_loss_plan** out) {
    if (!res || !out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (R < 1 || R > SL_MAX_R) return fail(GVX_ERR_INVALID_ARG, "R = %d resolutions: 1 .. %d are supported", R, SL_MAX_R);
    for (int r = 0; r < R; ++r) {
        const gvx_stft_resolution& q = res[r];
        if (q.n_fft != 512 && q.n_fft != 1024 && q.n_fft != 2048)
            return fail(GVX_ERR_UNSUPPORTED, "resolution %d: n_fft = %d, supported are 512, 1024 and 2048", r, q.n_fft);
        if (q.hop < 1 || q.hop > q.n_fft) return fail(GVX_ERR_INVALID_ARG, "resolution %d: hop = %d is outside [1, n_fft = %d]", r, q.hop, q.n_fft);
        if (q.win_length < 2 || q.win_length > q.n_fft)
            return fail(GVX_ERR_INVALID_ARG, "resolution %d: win_length = %d is outside [2, n_fft = %d]", r, q.win_length, q.n_fft);
    }
    if (!(w_sc >= 0.f) || !(w_mag >= 0.f) || std::isinf(w_sc) || std::isinf(w_mag))
        return fail(GVX_ERR_INVALID_ARG, "the weights must be finite and >= 0");
    if (!(eps > 0.f) || std::isinf(eps)) return fail(GVX_ERR_INVALID_ARG, "eps must be finite and > 0");
    gvx_stft_loss_plan* p = new gvx_stft_loss_plan();
    p->R = R; p->w_sc = w_sc; p->w_mag = w_mag; p->eps = eps;
    std::vector<float> h;
    for (int r = 0; r < R; ++r) {
        p->res[r] = res[r];
        p->n_min = std::max(p->n_min, res[r].n_fft / 2 + 1);
        const StftTables t = stft_tables(h, res[r].n_fft, res[r].win_length);
        p->win_at[r] = t.win; p->tw_at[r] = t.tw; p->tw2_at[r] = t.tw2;
        h.resize((h.size() + 3) & ~(size_t)3, 0.f);   // the next table starts on 16 bytes
    }
    if (!stft_upload(&p->tables, h)) {
        delete p;
        return fail(GVX_ERR_HIP, "window and twiddle table allocation failed");
    }
    *out = p;
    return GVX_OK;
}

void gvx_stft_loss_destroy(gvx_stft_loss_plan* p) {
    if (!p) return;
    if (p->tables) (void)hipFree(p->tables);
    delete p;
}

size_t gvx_stft_loss_workspace_bytes(const gvx_stft_loss_plan* p, int B, long n_max) {
    if (const char* why = sl_shape_problem(p, B, n_max)) { (void)fail(GVX_ERR_INVALID_ARG, "%s", why); return 0; }
    return sl_layout(p, B, n_max).total;
}

int gvx_stft_loss(gvx_stft_loss_plan* p, const float* pred, const float* target, const int32_t* sample_lengths, int B, long n_max,
                  float* loss_out, float* parts_out, float* d_pred, const gvx_stft_loss_debug* dbg, void* workspace, size_t workspace_bytes,
                  void* stream) {
    if (const char* why = sl_shape_problem(p, B, n_max)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!pred || !target || !loss_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_max < p->n_min)
        return fail(GVX_ERR_SHAPE, "n_max = %ld: a row needs at least n_fft / 2 + 1 = %d samples for the reflection", n_max, p->n_min);
    const SlLayout L = sl_layout(p, B, n_max);
    if (const int rc = stft_check_workspace(workspace, workspace_bytes, L.total)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(workspace);
    const bool grad = d_pred != nullptr;
    float2* coef = reinterpret_cast<float2*>(ws + L.coef);
    SlRes rr[SL_MAX_R];
    SlReduce red{};
    SlGather gat{};
    for (int r = 0; r < p->R; ++r) {
        SlRes& q = rr[r];
        q.win = p->tables + p->win_at[r];
        q.tw = reinterpret_cast<const float2*>(p->tables + p->tw_at[r]);
        q.tw2 = reinterpret_cast<const float2*>(p->tables + p->tw2_at[r]);
        q.hop = p->res[r].hop; q.r = r; q.R = p->R;
        q.f_max = L.f_max[r]; q.nwg = L.nwg[r];
        q.X = grad ? reinterpret_cast<float2*>(ws + L.X[r]) : nullptr;
        q.Mt = grad ? reinterpret_cast<float*>(ws + L.Mt[r]) : nullptr;
        q.g = grad ? reinterpret_cast<float*>(ws + L.g[r]) : nullptr;
        q.part = reinterpret_cast<double*>(ws + L.part[r]);
        q.dbg_p = dbg ? dbg->mag_pred[r] : nullptr;
        q.dbg_t = dbg ? dbg->mag_target[r] : nullptr;
        red.part[r] = q.part; red.nwg[r] = q.nwg; red.hop[r] = q.hop; red.bins[r] = p->res[r].n_fft / 2 + 1;
        gat.g[r] = q.g; gat.n_fft[r] = p->res[r].n_fft; gat.hop[r] = q.hop; gat.f_max[r] = q.f_max;
    }
    red.R = gat.R = p->R; red.B = B; red.w_sc = p->w_sc; red.w_mag = p->w_mag;
    red.parts = parts_out; red.coef = coef; red.terms = reinterpret_cast<double*>(ws + L.terms); red.loss = loss_out;
    auto pass = [&](bool grad_pass) {
        for (int r = 0; r < p->R; ++r) {
            const int rc = stft_dispatch(p->res[r].n_fft, [&](auto h) -> int {
                constexpr int H = decltype(h)::value;
                const dim3 grid((unsigned)rr[r].nwg, (unsigned)B);
                if (grad_pass) sl_grad_kernel<H><<<grid, SL_FRAMES * 64, 0, s>>>(sample_lengths, n_max, p->n_min, p->eps, coef, rr[r]);
                else sl_forward_kernel<H><<<grid, SL_FRAMES * 64, 0, s>>>(pred, target, sample_lengths, n_max, p->n_min, p->eps, rr[r]);
                HIP_TRY(hipGetLastError());
                return GVX_OK;
            });
            if (rc != GVX_OK) return rc;
        }
        return (int)GVX_OK;
    };
    int rc = pass(false);
    if (rc != GVX_OK) return rc;
    sl_reduce_kernel<<<1, 256, 0, s>>>(sample_lengths, n_max, p->n_min, red);
    HIP_TRY(hipGetLastError());
    if (grad) {
        rc = pass(true);
        if (rc != GVX_OK) return rc;
        sl_gather_kernel<<<dim3((unsigned)((n_max + SL_GATHER - 1) / SL_GATHER), (unsigned)B), SL_GATHER, 0, s>>>(sample_lengths, n_max, p->n_min, gat,
                                                                                                                d_pred);
        HIP_TRY(hipGetLastError());
    }
    return stft_check_lengths(sample_lengths, B, n_max, p->n_min, "n_fft / 2 + 1", d_pred, s);
}

}  // extern "C"
