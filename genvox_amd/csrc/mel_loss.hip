// Mel-spectrogram L1 loss of a predicted waveform against its target, value and gradient (include/genvox_amd.h, "Mel-spectrogram L1
// loss"): HiFi-GAN's spectral term.  ml_frame_kernel does everything of a frame in one wave: target's transform in LDS (fft_lds.h),
// its magnitudes staged in the transform's buffer, the banded mel product and the logarithm, the same for pred with its spectrum kept
// in registers, the cells' |l_t - l_p|, and - with d_pred - dm (its coefficient 1 / (B F n_mels) is known from the lengths alone, so
// no batch sum stands between the value and the gradient), the banded transposed product, dX = dS X / S, the adjoint of the real
// transform and the window.  ml_gather_kernel sums, per output sample, the frames that cover the sample and its two reflected images;
// ml_reduce_kernel adds the workgroups' partial sums per row and then the rows, in a fixed order in float64.
// No atomics anywhere: two calls give the same bits, and a row's numbers never depend on another row's.
//
// Order of this file: kernels, workspace layout, the C ABI.
#include "fft_lds.h"
#include "stft_plan.h"

#include <algorithm>

using gvx::fail;
using namespace gvx_plan;

struct gvx_mel_loss_plan {
    int n_fft = 0, hop = 0, win_length = 0, n_mels = 0;
    int pad = 0, n_min = 0;     // (n_fft - hop) / 2; shortest legal row: max(hop, pad + 1)
    float clamp = 1e-5f, mag_eps = 1e-9f;
    std::vector<int32_t> mel_lo, mel_hi, bin_lo, bin_hi;   // the bands, hi inclusive; an empty band is lo = 0, hi = -1
    std::vector<float> host_tables;      // what create makes; the first call moves both to the device, so that a plan - and the
    std::vector<int32_t> host_bands;     // workspace arithmetic with it - needs no device
    float* tables = nullptr;    // device: window [N], w_H^m [H] and w_N^k [H + 1] as float2, the mels' bands, the bins' bands
    int32_t* bands = nullptr;   // device: per mel (first bin, bins, offset of its values), then per bin (first mel, mels, offset)
    size_t tw_at = 0, tw2_at = 0, fwd_at = 0, bwd_at = 0;
};

namespace {

constexpr int ML_FRAMES = GVX_MEL_LOSS_FRAMES_PER_WORKGROUP;   // frames (waves) per workgroup of the frame kernel
constexpr int ML_GATHER = GVX_MEL_LOSS_GATHER_SAMPLES;         // output samples (threads) per workgroup of the gather
constexpr int ML_MAX_MELS = GVX_MEL_LOSS_MAX_MELS;
constexpr int ML_MEL_ROUNDS = ML_MAX_MELS / 64;                // mels of a lane

// ---- kernels ------------------------------------------------------------------------------------------------

struct MlArgs {
    const float* win; const float2* tw; const float2* tw2;
    const float* fwd; const float* bwd;              // basis[j][lo_j ..] per mel; basis[jlo_k ..][k] per bin
    const int32_t* mel_band; const int32_t* bin_band;   // [.][3]: first, count, offset into fwd / bwd
    int hop, pad, n_mels, B;
    int f_max, nwg;       // frames of a row of n_max samples, workgroups per row
    float clamp, mag_eps;
    float* g;             // frame gradients [B][f_max][n_fft] (null: the value alone)
    double* part;         // [B][nwg]
    float* dbg_p; float* dbg_t;
};

// a row the host refuses has no frames and no samples here: nothing of it is read, its gradient is zeros
__device__ __forceinline__ int ml_len(const int32_t* lens, int b, long n_max, int n_min) {
    const long n = lens ? (long)lens[b] : n_max;
    return n < n_min || n > n_max ? 0 : (int)n;
}

__device__ __forceinline__ int ml_reflect(int i, int nb) {
    i = i < 0 ? -i : i;
    return i >= nb ? 2 * (nb - 1) - i : i;
}

// The inverse side is sl_grad_kernel's (stft_loss.hip): dL/dx_n = sum_{k = 0}^{H} Re(G_k conj(w_N^{kn})) is the unnormalised
// complex-to-real inverse of Y with Y_0 = Re G_0, Y_H = Re G_H and Y_k = G_k / 2 between them, itself a complex inverse of H points:
// Z_k = (Y_k + conj Y_{H-k}) + i conj(w_N^k) (Y_k - conj Y_{H-k}); a lane makes Z_k and Z_{H-k} together from the same two bins.
template <int H>
__global__ __launch_bounds__(ML_FRAMES * 64) void ml_frame_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                  const int32_t* __restrict__ lens, long n_max, int n_min, MlArgs p) {
    constexpr int Q = H / 64, N = 2 * H;
    __shared__ __attribute__((aligned(16))) float2 fsm[ML_FRAMES * fft_lds_words<H>()];
    __shared__ float dmsm[ML_FRAMES][ML_MAX_MELS];
    __shared__ double wsum[ML_FRAMES];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, t = (int)blockIdx.x * ML_FRAMES + wave;
    const int nb = ml_len(lens, b, n_max, n_min);
    const int F = nb / p.hop;
    if ((int)blockIdx.x * ML_FRAMES >= F && !p.dbg_p && !p.dbg_t) return;   // the whole workgroup lies behind the row's frames
    float2* buf = fsm + wave * fft_lds_words<H>();
    float* sbuf = reinterpret_cast<float*>(buf);   // S_k at [k], k = 0 .. H, once the split has read the transform
    float* dm = dmsm[wave];
    const long f = (long)b * p.f_max + t;
    const bool grad = p.g != nullptr;
    float sl = 0.f;
    if (t < F) {
        const float coef = (float)(1.0 / ((double)p.B * (double)F * (double)p.n_mels));
        float lt[ML_MEL_ROUNDS];
        float2 xs[Q + 1];
        float ss[Q + 1];
#pragma unroll
        for (int sig = 0; sig < 2; ++sig) {   // target, then pred: what is kept across the second transform is two logarithms
            const float* x = (sig ? pred : target) + (long)b * n_max;
            const int i0 = t * p.hop - p.pad;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int m = j + 64 * q;
                const float2 w = *reinterpret_cast<const float2*>(p.win + 2 * m);
                buf[fpad(m)] = make_float2(w.x * x[ml_reflect(i0 + 2 * m, nb)], w.y * x[ml_reflect(i0 + 2 * m + 1, nb)]);
            }
            wave_lds_fence();
            fft_lds_wave<H, false>(buf, p.tw, j);
#pragma unroll
            for (int q = 0; q <= Q; ++q) {
                const int k = j + 64 * q;
                if (k <= H) {
                    const float2 X = rfft_split(buf[fpad(k & (H - 1))], buf[fpad((H - k) & (H - 1))], p.tw2[k], k == 0 || k == H);
                    xs[q] = X;
                    ss[q] = sqrtf(X.x * X.x + X.y * X.y + p.mag_eps);
                }
            }
            wave_lds_fence();
#pragma unroll
            for (int q = 0; q <= Q; ++q) {
                const int k = j + 64 * q;
                if (k <= H) sbuf[k] = ss[q];
            }
            wave_lds_fence();
#pragma unroll
            for (int r = 0; r < ML_MEL_ROUNDS; ++r) {
                const int mel = j + 64 * r;
                if (mel < p.n_mels) {
                    const int lo = p.mel_band[3 * mel], cnt = p.mel_band[3 * mel + 1];
                    const float* v = p.fwd + p.mel_band[3 * mel + 2];
                    float m = 0.f;
                    for (int c = 0; c < cnt; ++c) m = fmaf(v[c], sbuf[lo + c], m);
                    const float l = logf(fmaxf(m, p.clamp));
                    if (sig == 0) {
                        lt[r] = l;
                        if (p.dbg_t) p.dbg_t[f * p.n_mels + mel] = l;
                    } else {
                        if (p.dbg_p) p.dbg_p[f * p.n_mels + mel] = l;
                        sl += fabsf(lt[r] - l);
                        // d|l_t - l_p| / dl_p = sign(l_p - l_t), 0 at a tie; dl / dm = 1 / m where the clamp passes
                        const float sgn = (float)((l > lt[r]) - (l < lt[r]));
                        dm[mel] = m >= p.clamp ? coef * sgn / m : 0.f;
                    }
                }
            }
            wave_lds_fence();
        }
        if (grad) {
            float2 ya[Q / 2 + 1], yb[Q / 2 + 1];
            // Y_k of the lane's own bins from the spectrum it kept; S is no longer read by anyone (fence above)
#pragma unroll
            for (int q = 0; q <= Q; ++q) {
                const int k = j + 64 * q;
                if (k <= H) {
                    const int lo = p.bin_band[3 * k], cnt = p.bin_band[3 * k + 1];
                    const float* v = p.bwd + p.bin_band[3 * k + 2];
                    float ds = 0.f;
                    for (int c = 0; c < cnt; ++c) ds = fmaf(v[c], dm[lo + c], ds);
                    const bool end = k == 0 || k == H;
                    float scale = ds / ss[q];
                    if (!end) scale *= 0.5f;
                    buf[k] = make_float2(xs[q].x * scale, end ? 0.f : xs[q].y * scale);
                }
            }
            wave_lds_fence();
#pragma unroll
            for (int q = 0; q <= Q / 2; ++q) {
                const int k = j + 64 * q;
                if (k <= H / 2) { ya[q] = buf[k]; yb[q] = buf[H - k]; }
            }
            wave_lds_fence();
#pragma unroll
            for (int q = 0; q <= Q / 2; ++q) {
                const int k = j + 64 * q;
                if (k <= H / 2) {
                    const float2 e = make_float2(ya[q].x + yb[q].x, ya[q].y - yb[q].y), d = make_float2(ya[q].x - yb[q].x, ya[q].y + yb[q].y);
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
    } else if (t < p.f_max) {
        const float nan = __uint_as_float(0x7fc00000u);
        for (int mel = j; mel < p.n_mels; mel += 64) {
            if (p.dbg_p) p.dbg_p[f * p.n_mels + mel] = nan;
            if (p.dbg_t) p.dbg_t[f * p.n_mels + mel] = nan;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) sl += __shfl_xor(sl, off);
    if (j == 0) wsum[wave] = (double)sl;
    __syncthreads();
    if (tid == 0 && (int)blockIdx.x * ML_FRAMES < F) {
        double s = 0.0;
        for (int w = 0; w < ML_FRAMES; ++w) s += wsum[w];
        p.part[(long)b * p.nwg + blockIdx.x] = s;
    }
}

// overlap-add as a gather, the transpose of the framing: a thread per sample of d_pred sums the frame gradients at the padded
// positions that read the sample - its own, p = i + pad, and its images under the left and right reflection - over the frames that
// cover each, in ascending frame order.  Exact zeros at and behind the row's length and where no frame reaches
__global__ __launch_bounds__(ML_GATHER) void ml_gather_kernel(const int32_t* __restrict__ lens, long n_max, int n_min, const float* __restrict__ g_all,
                                                              int N, int hop, int pad, int f_max, float* __restrict__ d_pred) {
    const long i_long = (long)blockIdx.x * ML_GATHER + threadIdx.x;
    const int b = blockIdx.y;
    if (i_long >= n_max) return;
    const int i = (int)i_long;
    const int nb = ml_len(lens, b, n_max, n_min);
    float s = 0.f;
    if (i < nb) {
        const int F = nb / hop;
        const float* g = g_all + (long)b * f_max * N;
#pragma unroll
        for (int img = 0; img < 3; ++img) {
            const int p = img == 0 ? i + pad : (img == 1 ? pad - i : 2 * (nb - 1) - i + pad);
            const bool ok = img == 0 || (img == 1 ? (i >= 1 && i <= pad) : (i <= nb - 2 && i >= nb - 1 - pad));
            if (ok) {
                const int t_lo = p >= N ? (p - N) / hop + 1 : 0;
                const int t_hi = min(F - 1, p / hop);
                for (int t = t_lo; t <= t_hi; ++t) s += g[(long)t * N + (p - t * hop)];
            }
        }
    }
    d_pred[(long)b * n_max + i] = s;
}

// one workgroup: a wave per row adds the row's partial sums (lane-strided, then a butterfly: a fixed order), then one thread adds the
// rows in order.  float64 here, in this one small kernel
__global__ __launch_bounds__(256) void ml_reduce_kernel(const int32_t* __restrict__ lens, long n_max, int n_min, int B, int hop, int n_mels, int nwg,
                                                        const double* __restrict__ part, double* __restrict__ rows, float* __restrict__ parts,
                                                        float* __restrict__ loss) {
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int b = wave; b < B; b += 4) {
        const int nb = ml_len(lens, b, n_max, n_min);
        const int F = nb / hop;
        const int nw = (F + ML_FRAMES - 1) / ML_FRAMES;
        const double* mine = part + (long)b * nwg;
        double s = 0.0;
        for (int w = j; w < nw; w += 64) s += mine[w];
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        if (j == 0) {
            const double mean = F ? s / ((double)F * (double)n_mels) : __longlong_as_double(0x7ff8000000000000LL);
            rows[b] = mean;
            if (parts) parts[b] = (float)mean;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) s += rows[b];
        *loss = (float)(s / (double)B);
    }
}

// ---- workspace layout ---------------------------------------------------------------------------------------

struct MlLayout {
    int f_max, nwg;
    size_t g, part, rows, total;
};

MlLayout ml_layout(const gvx_mel_loss_plan* p, int B, long n_max) {
    MlLayout L{};
    StftRegions ws;
    L.f_max = (int)(n_max / p->hop);
    L.nwg = (L.f_max + ML_FRAMES - 1) / ML_FRAMES;
    L.g = ws.take((size_t)B * L.f_max * p->n_fft * sizeof(float));
    L.part = ws.take((size_t)B * L.nwg * sizeof(double));
    L.rows = ws.take((size_t)B * sizeof(double));
    L.total = ws.total;
    return L;
}

const char* ml_shape_problem(const gvx_mel_loss_plan* p, int B, long n_max) {
    if (!p) return "null plan";
    if (B < 1 || B > GVX_MEL_LOSS_MAX_ROWS) return "B must be in [1, GVX_MEL_LOSS_MAX_ROWS]";
    if (n_max < 1 || n_max > GVX_MEL_LOSS_MAX_SAMPLES) return "n_max must be in [1, GVX_MEL_LOSS_MAX_SAMPLES]";
    return nullptr;
}

}  // namespace

extern "C" {

// the bands: min .. max of the non-zero entries, per mel over the bins and per bin over the mels
int gvx_mel_loss_bands(const float* mel_basis, int n_mels, int bins, int32_t* mel_lo, int32_t* mel_hi, int32_t* bin_lo, int32_t* bin_hi) {
    if (!mel_basis || !mel_lo || !mel_hi || !bin_lo || !bin_hi) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_mels < 1 || bins < 1) return fail(GVX_ERR_INVALID_ARG, "n_mels and bins must be >= 1");
    for (int j = 0; j < n_mels; ++j) { mel_lo[j] = 0; mel_hi[j] = -1; }
    for (int k = 0; k < bins; ++k) { bin_lo[k] = 0; bin_hi[k] = -1; }
    for (int j = 0; j < n_mels; ++j)
        for (int k = 0; k < bins; ++k) {
            if (mel_basis[(size_t)j * bins + k] == 0.f) continue;
            if (mel_hi[j] < 0) mel_lo[j] = k;
            mel_hi[j] = k;
            if (bin_hi[k] < 0) bin_lo[k] = j;
            bin_hi[k] = j;
        }
    return GVX_OK;
}

int gvx_mel_loss_create(int n_fft, int hop, int win_length, int n_mels, const float* mel_basis, float clamp, float mag_eps,
                        gvx_mel_loss_plan** out) {
    if (!mel_basis || !out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_fft != 512 && n_fft != 1024 && n_fft != 2048) return fail(GVX_ERR_UNSUPPORTED, "n_fft = %d, supported are 512, 1024 and 2048", n_fft);
    if (hop < 1 || hop > n_fft) return fail(GVX_ERR_INVALID_ARG, "hop = %d is outside [1, n_fft = %d]", hop, n_fft);
    if ((n_fft - hop) & 1) return fail(GVX_ERR_INVALID_ARG, "n_fft - hop = %d is odd: the padding (n_fft - hop) / 2 must be whole", n_fft - hop);
    if (win_length < 2 || win_length > n_fft) return fail(GVX_ERR_INVALID_ARG, "win_length = %d is outside [2, n_fft = %d]", win_length, n_fft);
    if (n_mels < 1 || n_mels > ML_MAX_MELS) return fail(GVX_ERR_INVALID_ARG, "n_mels = %d is outside [1, %d]", n_mels, ML_MAX_MELS);
    if (!(clamp > 0.f) || std::isinf(clamp)) return fail(GVX_ERR_INVALID_ARG, "clamp must be finite and > 0");
    if (!(mag_eps > 0.f) || std::isinf(mag_eps)) return fail(GVX_ERR_INVALID_ARG, "mag_eps must be finite and > 0");
    const int bins = n_fft / 2 + 1;
    for (size_t i = 0; i < (size_t)n_mels * bins; ++i)
        if (!std::isfinite(mel_basis[i])) return fail(GVX_ERR_INVALID_ARG, "mel_basis[%zu][%zu] is not finite", i / bins, i % bins);
    gvx_mel_loss_plan* p = new gvx_mel_loss_plan();
    p->n_fft = n_fft; p->hop = hop; p->win_length = win_length; p->n_mels = n_mels;
    p->pad = (n_fft - hop) / 2; p->n_min = std::max(hop, p->pad + 1);
    p->clamp = clamp; p->mag_eps = mag_eps;
    p->mel_lo.assign(n_mels, 0); p->mel_hi.assign(n_mels, -1);
    p->bin_lo.assign(bins, 0); p->bin_hi.assign(bins, -1);
    (void)gvx_mel_loss_bands(mel_basis, n_mels, bins, p->mel_lo.data(), p->mel_hi.data(), p->bin_lo.data(), p->bin_hi.data());
    std::vector<float>& h = p->host_tables;
    std::vector<int32_t>& bands = p->host_bands;
    const StftTables t = stft_tables(h, n_fft, win_length);   // the window first: t.win = 0
    p->tw_at = t.tw; p->tw2_at = t.tw2;
    p->fwd_at = h.size();
    for (int j = 0; j < n_mels; ++j) {
        const int cnt = p->mel_hi[j] - p->mel_lo[j] + 1;
        bands.insert(bands.end(), {p->mel_lo[j], cnt, (int32_t)(h.size() - p->fwd_at)});
        for (int k = p->mel_lo[j]; k <= p->mel_hi[j]; ++k) h.push_back(mel_basis[(size_t)j * bins + k]);
    }
    p->bwd_at = h.size();
    for (int k = 0; k < bins; ++k) {
        const int cnt = p->bin_hi[k] - p->bin_lo[k] + 1;
        bands.insert(bands.end(), {p->bin_lo[k], cnt, (int32_t)(h.size() - p->bwd_at)});
        for (int j = p->bin_lo[k]; j <= p->bin_hi[k]; ++j) h.push_back(mel_basis[(size_t)j * bins + k]);
    }
    *out = p;
    return GVX_OK;
}

void gvx_mel_loss_destroy(gvx_mel_loss_plan* p) {
    if (!p) return;
    if (p->tables) (void)hipFree(p->tables);
    if (p->bands) (void)hipFree(p->bands);
    delete p;
}

size_t gvx_mel_loss_workspace_bytes(const gvx_mel_loss_plan* p, int B, long n_max) {
    if (const char* why = ml_shape_problem(p, B, n_max)) { (void)fail(GVX_ERR_INVALID_ARG, "%s", why); return 0; }
    return ml_layout(p, B, n_max).total;
}

int gvx_mel_loss(gvx_mel_loss_plan* p, const float* pred, const float* target, const int32_t* sample_lengths, int B, long n_max,
                 float* loss_out, float* parts_out, float* d_pred, const gvx_mel_loss_debug* dbg, void* workspace, size_t workspace_bytes,
                 void* stream) {
    if (const char* why = ml_shape_problem(p, B, n_max)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!pred || !target || !loss_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_max < p->n_min)
        return fail(GVX_ERR_SHAPE, "n_max = %ld: a row needs at least max(hop, (n_fft - hop) / 2 + 1) = %d samples", n_max, p->n_min);
    const MlLayout L = ml_layout(p, B, n_max);
    if (const int rc = stft_check_workspace(workspace, workspace_bytes, L.total)) return rc;
    if (!p->tables && (!stft_upload(&p->tables, p->host_tables) || !stft_upload(&p->bands, p->host_bands))) {
        if (p->tables) (void)hipFree(p->tables);   // the bands were refused
        p->tables = nullptr;
        return fail(GVX_ERR_HIP, "window, twiddle and band table allocation failed");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    char* ws = reinterpret_cast<char*>(workspace);
    const bool grad = d_pred != nullptr;
    MlArgs a{};
    a.win = p->tables;
    a.tw = reinterpret_cast<const float2*>(p->tables + p->tw_at);
    a.tw2 = reinterpret_cast<const float2*>(p->tables + p->tw2_at);
    a.fwd = p->tables + p->fwd_at; a.bwd = p->tables + p->bwd_at;
    a.mel_band = p->bands; a.bin_band = p->bands + 3 * p->n_mels;
    a.hop = p->hop; a.pad = p->pad; a.n_mels = p->n_mels; a.B = B;
    a.f_max = L.f_max; a.nwg = L.nwg;
    a.clamp = p->clamp; a.mag_eps = p->mag_eps;
    a.g = grad ? reinterpret_cast<float*>(ws + L.g) : nullptr;
    a.part = reinterpret_cast<double*>(ws + L.part);
    a.dbg_p = dbg ? dbg->log_mel_pred : nullptr;
    a.dbg_t = dbg ? dbg->log_mel_target : nullptr;
    const int rc = stft_dispatch(p->n_fft, [&](auto h) -> int {
        ml_frame_kernel<decltype(h)::value><<<dim3((unsigned)a.nwg, (unsigned)B), ML_FRAMES * 64, 0, s>>>(pred, target, sample_lengths, n_max, p->n_min, a);
        HIP_TRY(hipGetLastError());
        return GVX_OK;
    });
    if (rc != GVX_OK) return rc;
    ml_reduce_kernel<<<1, 256, 0, s>>>(sample_lengths, n_max, p->n_min, B, p->hop, p->n_mels, L.nwg, a.part, reinterpret_cast<double*>(ws + L.rows),
                                       parts_out, loss_out);
    HIP_TRY(hipGetLastError());
    if (grad) {
        ml_gather_kernel<<<dim3((unsigned)((n_max + ML_GATHER - 1) / ML_GATHER), (unsigned)B), ML_GATHER, 0, s>>>(sample_lengths, n_max, p->n_min, a.g,
                                                                                                                p->n_fft, p->hop, p->pad, L.f_max, d_pred);
        HIP_TRY(hipGetLastError());
    }
    return stft_check_lengths(sample_lengths, B, n_max, p->n_min, "max(hop, (n_fft - hop) / 2 + 1)", d_pred, s);
}

}  // extern "C"
