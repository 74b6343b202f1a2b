// Pitch tracking on the device: YIN F0 contours of a batch of waveforms, each row at its own length, and the comparison of two
// contours (voicing decision error, gross pitch error, F0 RMSE in cents).  The definitions are in include/genvox_amd.h; the float64
// restatement the tests hold these kernels to is tests/pitch_ref64.py.
//
// The difference function is computed as it is defined, d(tau) = sum_j (x[s+j] - x[s+j+tau])^2, one subtraction and one fused
// multiply-add per term.  The cheaper forms - energy minus autocorrelation, r(0) + r_tau(0) - 2 acf(tau), and any FFT route to the
// autocorrelation - form d as the difference of numbers of the size of the window's energy: on a nearly periodic signal, where d
// is orders of magnitude below that energy, float32 leaves them no correct digit, and that is exactly where the voicing decision
// is made (c(tau) < threshold) and where the parabola is laid.  A sum of squares of differences has no cancellation: every term is
// non-negative, so the relative error of d is (W + 1) 2^-24 whatever the signal.
//
// Order of this file: the plan, the tracker's kernel, the comparison's kernel, the C ABI.
#include "gvx_internal.h"

#include <algorithm>

using gvx::fail;

namespace {

constexpr int PY_THREADS = 256;
constexpr int PY_WAVES = PY_THREADS / 64;
constexpr int PY_LAGS = 3;                 // consecutive lags of a lane (odd: lanes 3 floats apart hit 32 different LDS banks)
constexpr int PY_PASS = 64 * PY_LAGS;      // lags a wave covers at a time
constexpr int PY_MAX_TILE = 16;            // frames of a workgroup, at most
constexpr int PY_MAX_CHUNK = (GVX_PITCH_MAX_LAG + 63) / 64;   // lags of a lane in the running sum
constexpr size_t PY_LDS_BYTES = 64 * 1024;

// What a call with these parameters does: a workgroup takes `tile` consecutive frames of one row, PY_WAVES at a time, and stages the
// `region` = W + lag_max + (tile - 1) hop samples they span into LDS once; behind them one table of lag_max + 1 floats per wave.
// tile is the largest count up to PY_MAX_TILE whose region fits 64 KiB beside the tables (a hop beyond the window leaves one).
struct PitchPlan {
    int tile, region;
    size_t lds_bytes;
};
inline PitchPlan pitch_plan(const gvx_pitch_params& p) {
    const long span = (long)p.window + p.lag_max, tables = (long)PY_WAVES * (p.lag_max + 1);
    const long room = (long)(PY_LDS_BYTES / sizeof(float)) - tables - span;   // >= 0 inside the limits: 16384 - 4100 - 3072
    PitchPlan pl;
    pl.tile = (int)std::min<long>(PY_MAX_TILE, 1 + room / p.hop);
    pl.region = (int)(span + (long)(pl.tile - 1) * p.hop);
    pl.lds_bytes = (size_t)(pl.region + tables) * sizeof(float);
    return pl;
}

__device__ __forceinline__ float py_bcast(float v, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); }

// One block of up to 64 terms j0 .. j0 + n - 1 of the three sums of a lane.  The lane's 64 x[s + j] arrive with one LDS read (lane i
// holds term i) and are handed round as scalars; of the other operand every term needs one new sample: x[s + j + tau0 + 2], the two
// before it are still in registers from the terms before.  One LDS read per three differences.
template <bool FULL>
__device__ __forceinline__ void py_block(const float* xs, const float* xt, int j0, int n, int lane, float& w0, float& w1, float& a0, float& a1,
                                         float& a2) {
    const float mine = (FULL || lane < n) ? xs[j0 + lane] : 0.f;
    auto term = [&](int i) {
        const float x = py_bcast(mine, i), w2 = xt[j0 + i + 2];
        const float e0 = x - w0, e1 = x - w1, e2 = x - w2;
        a0 = fmaf(e0, e0, a0);
        a1 = fmaf(e1, e1, a1);
        a2 = fmaf(e2, e2, a2);
        w0 = w1;
        w1 = w2;
    };
    if constexpr (FULL) {
#pragma unroll
        for (int i = 0; i < 64; ++i) term(i);
    } else {
        for (int i = 0; i < n; ++i) term(i);   // n is the same for every lane
    }
}

// grid (ceil(F / tile), B), PY_THREADS threads.  Per frame, one wave:
//   d     lane l of pass p owns the lags 3 (64 p + l) + {0, 1, 2}, clamped so that the last lane of the table ends on lag_max (it
//         recomputes a neighbour's lags with the same operations, hence the same bits); every sum runs over j ascending.
//   sum   lane l owns the lags 1 + l C .. (l + 1) C of the running sum, C = ceil(lag_max / 64): its own total, an inclusive scan of
//         the totals across the wave (strides 1, 2, .. 32), then its lags in ascending order on top of the lanes before it.
//   scan  the first lag under the threshold by ballot, 64 lags at a time; the walk down to the local minimum and the parabola are
//         a handful of LDS reads.
// The waves of a workgroup meet at barriers only because they share the staged samples; all of them run every round.
__global__ void __launch_bounds__(PY_THREADS)
pitch_yin_kernel(const float* wav, const int32_t* sample_lengths, long N, int F, gvx_pitch_params p, int tile, int region, float* f0_out,
                 int32_t* lag_out, float* ap_out, float* cmnd_out) {
    extern __shared__ __attribute__((aligned(16))) float py_lds[];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fb0 = blockIdx.x * tile, f_end = min(fb0 + tile, F);
    long nb = sample_lengths ? (long)sample_lengths[b] : N;
    nb = nb < 0 ? 0 : (nb > N ? N : nb);
    const int Fb = (int)((nb + p.hop - 1) / p.hop);
    const int f_in = min(f_end, Fb);   // frames fb0 .. f_in - 1 are tracked, f_in .. f_end - 1 lie behind the row
    float* f0_b = f0_out + (long)b * F;
    int32_t* lag_b = lag_out + (long)b * F;
    float* ap_b = ap_out + (long)b * F;
    for (int f = max(fb0, f_in) + tid; f < f_end; f += PY_THREADS) {
        f0_b[f] = 0.f;
        lag_b[f] = -1;
        ap_b[f] = 1.f;
    }
    if (fb0 >= f_in) return;   // the whole workgroup: no barrier is left half attended, nothing of the row is read

    const int W = p.window, lag_max = p.lag_max, n_lags = lag_max + 1;
    float* xs = py_lds;                                  // [region]
    float* table = py_lds + region + wave * n_lags;      // [n_lags] of this wave
    const long g0 = (long)p.first_centre + (long)fb0 * p.hop - (W + lag_max) / 2;   // the sample xs[0] holds
    const float* row = wav + (long)b * N;
    for (int i = tid; i < region; i += PY_THREADS) {
        const long g = g0 + i;
        xs[i] = (g >= 0 && g < nb) ? row[g] : 0.f;
    }
    __syncthreads();

    const int chunk = (lag_max + 63) / 64;
    for (int f = fb0 + wave; f - wave < f_in; f += PY_WAVES) {   // every wave runs every round
        const bool live = f < f_in;
        if (live) {
            const float* xf = xs + (long)(f - fb0) * p.hop;
            for (int t0 = 0; t0 < n_lags; t0 += PY_PASS) {
                const int tau = t0 + lane * PY_LAGS, tau0 = min(tau, lag_max - (PY_LAGS - 1));
                const float* xt = xf + tau0;
                float w0 = xt[0], w1 = xt[1], a0 = 0.f, a1 = 0.f, a2 = 0.f;
                int j0 = 0;
                for (; j0 + 64 <= W; j0 += 64) py_block<true>(xf, xt, j0, 64, lane, w0, w1, a0, a1, a2);
                if (j0 < W) py_block<false>(xf, xt, j0, W - j0, lane, w0, w1, a0, a1, a2);
                if (tau <= lag_max) {
                    table[tau0] = a0;
                    table[tau0 + 1] = a1;
                    table[tau0 + 2] = a2;
                }
            }
        }
        __syncthreads();
        if (live) {   // d -> c in place: every lane reads and writes its own lags only
            float d[PY_MAX_CHUNK];
            const int first = 1 + lane * chunk;
            float total = 0.f;
#pragma unroll
            for (int i = 0; i < PY_MAX_CHUNK; ++i) {
                d[i] = (i < chunk && first + i <= lag_max) ? table[first + i] : 0.f;
                total += d[i];
            }
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float up = __shfl_up(total, off);
                if (lane >= off) total += up;
            }
            float run = __shfl_up(total, 1);
            if (lane == 0) {
                run = 0.f;
                table[0] = 1.f;
            }
#pragma unroll
            for (int i = 0; i < PY_MAX_CHUNK; ++i) {
                if (i < chunk && first + i <= lag_max) {
                    run += d[i];
                    table[first + i] = run > 0.f ? d[i] * (float)(first + i) / run : 1.f;
                }
            }
        }
        __syncthreads();
        if (live) {
            if (cmnd_out) {
                float* out = cmnd_out + ((long)b * F + f) * n_lags;
                for (int t = lane; t < n_lags; t += 64) out[t] = table[t];
            }
            int lag = -1;
            float lowest = INFINITY;
            for (int t0 = p.lag_min; t0 < lag_max; t0 += 64) {
                const int t = t0 + lane;
                const float c = t < lag_max ? table[t] : INFINITY;
                lowest = fminf(lowest, c);
                const unsigned long long under = __ballot(t < lag_max && c < p.threshold);
                if (under) {
                    lag = t0 + __builtin_ctzll(under);
                    break;   // the same for every lane
                }
            }
            if (lag >= 0) {
                while (lag + 1 <= lag_max - 1 && table[lag + 1] < table[lag]) ++lag;
                if (lane == 0) {
                    const float cm = table[lag - 1], c0 = table[lag], cp = table[lag + 1];
                    const float den = cm - 2.f * c0 + cp;
                    float shift = 0.f;
                    if (den > 0.f) shift = fminf(1.f, fmaxf(-1.f, (cm - cp) / (2.f * den)));
                    f0_b[f] = (float)p.sampling_rate / ((float)lag + shift);
                    lag_b[f] = lag;
                    ap_b[f] = c0;
                }
            } else {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) lowest = fminf(lowest, __shfl_xor(lowest, off));
                if (lane == 0) {
                    f0_b[f] = 0.f;
                    lag_b[f] = -1;
                    ap_b[f] = lowest;
                }
            }
        }
        __syncthreads();   // the table is the next round's
    }
}

// ---- comparison of two contours ------------------------------------------------------------------------------------------------

constexpr int FC_THREADS = 256;

// One workgroup per row.  Thread i counts the frames i, i + 256, ... in ascending order and sums their squared cents in double (the
// ratio, its logarithm and the sum: the result is then the float32 nearest to the exact one but for the last rounding); the 256
// partial results are added pairwise at strides 128, 64, ..., 1.
__global__ void __launch_bounds__(FC_THREADS)
f0_compare_kernel(const float* fa, const float* fb, const int32_t* frames_a, const int32_t* frames_b, int F, int32_t* counts, float* vde,
                  float* gpe, float* rmse) {
    __shared__ int s_both[FC_THREADS], s_one[FC_THREADS], s_gross[FC_THREADS];
    __shared__ double s_sq[FC_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    int na = frames_a ? frames_a[b] : F, nb = frames_b ? frames_b[b] : F;
    na = na < 0 ? 0 : (na > F ? F : na);
    nb = nb < 0 ? 0 : (nb > F ? F : nb);
    const int n = min(na, nb);
    int both = 0, one = 0, gross = 0;
    double sq = 0.0;
    for (int f = tid; f < n; f += FC_THREADS) {
        const float a = fa[(long)b * F + f], c = fb[(long)b * F + f];
        const bool va = a > 0.f, vc = c > 0.f;
        if (va != vc) ++one;
        if (va && vc) {
            ++both;
            const double r = (double)a / (double)c;
            if (fabs(r - 1.0) > 0.2) {
                ++gross;
            } else {
                const double cents = 1200.0 * log2(r);
                sq += cents * cents;
            }
        }
    }
    s_both[tid] = both, s_one[tid] = one, s_gross[tid] = gross, s_sq[tid] = sq;
    __syncthreads();
    for (int stride = FC_THREADS / 2; stride > 0; stride >>= 1) {
        if (tid < stride) {
            s_both[tid] += s_both[tid + stride];
            s_one[tid] += s_one[tid + stride];
            s_gross[tid] += s_gross[tid + stride];
            s_sq[tid] += s_sq[tid + stride];
        }
        __syncthreads();
    }
    if (tid == 0) {
        both = s_both[0], one = s_one[0], gross = s_gross[0];
        int32_t* c = counts + (long)b * GVX_F0_ROW_INTS;
        c[GVX_F0_FRAMES] = n;
        c[GVX_F0_VOICED_BOTH] = both;
        c[GVX_F0_VOICED_ONE] = one;
        c[GVX_F0_GROSS] = gross;
        vde[b] = n > 0 ? (float)one / (float)n : NAN;
        gpe[b] = both > 0 ? (float)gross / (float)both : NAN;
        rmse[b] = both - gross > 0 ? (float)sqrt(s_sq[0] / (double)(both - gross)) : NAN;
    }
}

int pitch_check(const gvx_pitch_params* p, int B, long N) {
    if (!p) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (B < 1 || N < 1) return fail(GVX_ERR_INVALID_ARG, "B and N must be >= 1");
    if (p->sampling_rate < 1 || p->hop < 1 || p->window < 1) return fail(GVX_ERR_INVALID_ARG, "sampling_rate, hop and window must be >= 1");
    if (p->lag_min < 1 || p->lag_min >= p->lag_max)
        return fail(GVX_ERR_INVALID_ARG, "lag_min = %d, lag_max = %d: 1 <= lag_min < lag_max is required", p->lag_min, p->lag_max);
    if (!(p->threshold > 0.f && p->threshold <= 1.f)) return fail(GVX_ERR_INVALID_ARG, "threshold = %g is outside (0, 1]", (double)p->threshold);
    if (p->window < GVX_PITCH_MIN_WINDOW || p->window > GVX_PITCH_MAX_WINDOW || p->lag_max > GVX_PITCH_MAX_LAG)
        return fail(GVX_ERR_UNSUPPORTED, "window = %d / lag_max = %d is beyond the pitch tracker's limits (window %d .. %d, lag_max <= %d)", p->window,
                    p->lag_max, GVX_PITCH_MIN_WINDOW, GVX_PITCH_MAX_WINDOW, GVX_PITCH_MAX_LAG);
    if (B > GVX_PITCH_MAX_ROWS) return fail(GVX_ERR_UNSUPPORTED, "B = %d is above %d rows", B, GVX_PITCH_MAX_ROWS);
    if ((N + p->hop - 1) / p->hop > GVX_PITCH_MAX_FRAMES)
        return fail(GVX_ERR_UNSUPPORTED, "%ld samples at hop %d are more than %d frames", N, p->hop, GVX_PITCH_MAX_FRAMES);
    return GVX_OK;
}

}  // namespace

extern "C" {

int gvx_pitch_frames(long n, int hop) {
    if (n <= 0 || hop < 1) return 0;
    const long frames = (n + hop - 1) / hop;
    return frames > INT32_MAX ? INT32_MAX : (int)frames;
}

int gvx_pitch_tile_frames(const gvx_pitch_params* params) {
    if (pitch_check(params, 1, 1) != GVX_OK) return -1;
    return pitch_plan(*params).tile;
}

int gvx_pitch_yin(const float* wav, const int32_t* sample_lengths, int B, long N, const gvx_pitch_params* params, float* f0_out,
                  int32_t* lag_out, float* aperiodicity_out, float* cmnd_out, void* stream) {
    const int rc = pitch_check(params, B, N);
    if (rc != GVX_OK) return rc;
    if (!wav || !f0_out || !lag_out || !aperiodicity_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const PitchPlan pl = pitch_plan(*params);
    const int F = gvx_pitch_frames(N, params->hop);
    const dim3 grid((F + pl.tile - 1) / pl.tile, B);
    pitch_yin_kernel<<<grid, PY_THREADS, pl.lds_bytes, (hipStream_t)stream>>>(wav, sample_lengths, N, F, *params, pl.tile, pl.region, f0_out, lag_out,
                                                                             aperiodicity_out, cmnd_out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int gvx_f0_compare(const float* f0_a, const float* f0_b, const int32_t* frames_a, const int32_t* frames_b, int B, int F, int32_t* counts_out,
                   float* vde_out, float* gpe_out, float* rmse_cents_out, void* stream) {
    if (B < 1 || F < 1) return fail(GVX_ERR_INVALID_ARG, "B and F must be >= 1");
    if (!f0_a || !f0_b || !counts_out || !vde_out || !gpe_out || !rmse_cents_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (F > GVX_PITCH_MAX_FRAMES) return fail(GVX_ERR_UNSUPPORTED, "F = %d is above %d frames", F, GVX_PITCH_MAX_FRAMES);
    f0_compare_kernel<<<B, FC_THREADS, 0, (hipStream_t)stream>>>(f0_a, f0_b, frames_a, frames_b, F, counts_out, vde_out, gpe_out, rmse_cents_out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

}  // C ABI
