// Pitch control on the device: TD-PSOLA in two calls - the plan (gvx_psola_plan: the pitch marks of a waveform from the tracker's lag
// contour, and where the grains of the output go for a ratio per frame) and the synthesis (gvx_psola_synth: the overlap-add).  The
// definitions are in include/genvox_amd.h; the numpy restatement the tests hold these kernels to is tests/psola_ref.py.
//
// Order of this file: what both kernels share, the plan's kernel, the synthesis' kernel, the C ABI.
#include "gvx_internal.h"

#include <algorithm>
#include <climits>

using gvx::fail;

namespace {

constexpr int PS_STAGE = 4096;                     // samples a row's wave holds in LDS at a time
constexpr int PS_STAGE_FRAMES = PS_STAGE + 4;      // their frames at hop 1, and the clamp at both ends
constexpr int PS_MARKS = PS_STAGE_FRAMES / 2;      // marks the second walk holds at a time (it reuses the first walk's LDS)
constexpr int PS_TILE = GVX_PSOLA_TILE;            // output samples of a workgroup of the synthesis: one per thread
static_assert(2 * GVX_PITCH_MAX_LAG <= PS_STAGE / 2, "a restaged chunk holds a candidate's whole neighbourhood and moves on by half a chunk at least");

struct PsGrid {   // the frame grid of a row
    int hop, first_centre, Fb;
    double inv_hop;
    __device__ PsGrid(int hop_, int first_centre_, int Fb_) : hop(hop_), first_centre(first_centre_), Fb(Fb_), inv_hop(1.0 / hop_) {}
    // floor((t - first_centre + hop / 2) / hop) without a 64-bit division: |a| is below 2^34, so a * (1 / hop) in double is within one
    // of the quotient, and the remainder says which way
    __device__ __forceinline__ int frame_of(long long t) const {
        const long long a = t - first_centre + hop / 2;
        long long f = (long long)floor((double)a * inv_hop);
        const long long rem = a - f * hop;
        if (rem < 0) --f;
        else if (rem >= hop) ++f;
        return f < 0 ? 0 : (f > Fb - 1 ? Fb - 1 : (int)f);
    }
};

__device__ __forceinline__ long ps_len(const int32_t* lens, int b, long N) {
    if (!lens) return N;
    const long v = lens[b];
    return v < 0 ? 0 : (v > N ? N : v);
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------

// One wave per row; control flow is the same in every lane.
//
// Analysis walk.  LDS holds x[cb .. cb + PS_STAGE) and the signed period (p, or -U where unvoiced) of the frames those samples fall
// in.  Before a candidate c is handled the chunk is moved to cb = c - P, P = max(lag_max, U), unless it holds [c - P, c + P] already:
// everything the step looks at - the window c +- r, r <= P / 4, and the frames of c and of the new mark - lies in there.  The window
// is searched by all lanes, each a run of consecutive samples: the wave's maximum by six exchanges, its lowest index by a ballot.
//
// Synthesis walk.  The same LDS now holds the ratios of the frames of [sb, sb + PS_STAGE) and PS_MARKS marks with their periods from
// kb on, read back from what the first walk stored; both chunks move forward when the walk reaches their ends.
//
// Marks and grains go out 64 at a time: lane (k mod 64) keeps entry k until the 64 are complete.
__global__ void __launch_bounds__(64)
psola_plan_kernel(const float* wav, const int32_t* sample_lengths, const int32_t* lag, const float* ratio, long N, int F, gvx_psola_params p, int K,
                  int J, int32_t* marks_out, int32_t* periods_out, int32_t* syn_pos_out, int32_t* syn_src_out, int32_t* counts_out,
                  int32_t* status_out) {
    __shared__ float xs[PS_STAGE_FRAMES];     // walk 1: samples; walk 2: ratios per frame
    __shared__ int32_t ps[PS_STAGE_FRAMES];   // walk 1: signed periods per frame; walk 2: marks [PS_MARKS] | signed periods [PS_MARKS]
    const int b = blockIdx.x, lane = threadIdx.x;
    const long n = ps_len(sample_lengths, b, N);
    if (n == 0) {
        if (lane == 0) {
            counts_out[(size_t)b * GVX_PSOLA_ROW_INTS + GVX_PSOLA_MARKS] = 0;
            counts_out[(size_t)b * GVX_PSOLA_ROW_INTS + GVX_PSOLA_GRAINS] = 0;
            status_out[b] = GVX_PSOLA_EMPTY;
        }
        return;
    }
    const PsGrid g(p.hop, p.first_centre, (int)((n + p.hop - 1) / p.hop));
    const float* x = wav + (size_t)b * N;
    const int32_t* lag_b = lag + (size_t)b * F;
    const float* ratio_b = ratio + (size_t)b * F;
    int32_t* marks_b = marks_out + (size_t)b * K;
    int32_t* periods_b = periods_out + (size_t)b * K;
    const int U = p.unvoiced_period, P = max(p.lag_max, U);

    int bad = 0;
    for (int f = lane; f < g.Fb; f += 64) {
        const float q = ratio_b[f];
        bad |= !(q >= GVX_PSOLA_RATIO_MIN && q <= GVX_PSOLA_RATIO_MAX);   // a NaN fails both comparisons
    }
    bad = __any(bad);

    // ---- analysis marks
    long cb = 0;          // the sample xs[0] holds
    int fbase = 0;        // the frame ps[0] holds
    bool staged = false;
    int k = 0, keep_m = 0, keep_p = 0;
    long m_prev = -1;
    int p_prev = 0;       // signed period at m_prev
    for (; k < K; ++k) {
        const long c = k == 0 ? 0 : m_prev + abs(p_prev);
        if (c >= n) break;
        if (!staged || c + P >= cb + PS_STAGE) {
            __syncthreads();   // the reads of the chunk before
            cb = c - P;
            fbase = g.frame_of(cb);
            const int flast = g.frame_of(cb + PS_STAGE - 1);
            for (int i = lane; i < PS_STAGE; i += 64) {
                const long t = cb + i;
                xs[i] = (t >= 0 && t < n) ? x[t] : 0.f;
            }
            for (int f = fbase + lane; f <= flast; f += 64) {   // at most (PS_STAGE - 1) / hop + 2 frames
                const int l = lag_b[f];
                ps[f - fbase] = l >= 1 ? min(max(l, p.lag_min), p.lag_max) : -U;
            }
            staged = true;
            __syncthreads();
        }
        long m = c;
        const int pc = ps[g.frame_of(c) - fbase];
        if (pc > 0) {
            const int r = (k == 0 ? pc : min(pc, abs(p_prev))) / 4;
            const long lo = max(c - r, m_prev + 1), hi = min(c + r, n - 1);
            // lane l owns the l-th run of ceil(length / 64) consecutive samples: the lowest lane that holds the wave's maximum holds
            // its lowest index
            const int run = ((int)(hi - lo) + 64) >> 6;
            const long i0 = lo + (long)lane * run, i1 = min(i0 + run - 1, hi);
            float best = -INFINITY;
            int at = INT_MAX;   // N is at most 2^25
            for (long i = i0; i <= i1; ++i) {
                const float v = xs[i - cb];
                if (v > best) {
                    best = v;
                    at = (int)i;
                }
            }
            float top = best;   // never NaN: only a sample that compared greater replaced -inf
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) top = fmaxf(top, __shfl_xor(top, off));
            const unsigned long long holders = __ballot(at != INT_MAX && best == top);
            if (holders) m = __shfl(at, __builtin_ctzll(holders));
        }
        const int pm = m == c ? pc : ps[g.frame_of(m) - fbase];
        if (lane == (k & 63)) {
            keep_m = (int)m;
            keep_p = pm;
        }
        if ((k & 63) == 63) {
            marks_b[k - 63 + lane] = keep_m;
            periods_b[k - 63 + lane] = keep_p;
        }
        m_prev = m;
        p_prev = pm;
    }
    const int n_marks = k;
    if (lane < (n_marks & 63)) {
        marks_b[(n_marks & ~63) + lane] = keep_m;
        periods_b[(n_marks & ~63) + lane] = keep_p;
    }
    __syncthreads();   // the marks are read back below; the chunks of walk 1 are done with

    // ---- synthesis marks
    int j = 0;
    if (!bad && n_marks > 0) {
        int32_t* pos_b = syn_pos_out + (size_t)b * J;
        int32_t* src_b = syn_src_out + (size_t)b * J;
        int32_t* mk = ps;
        int32_t* pk = ps + PS_MARKS;
        long sb = 0;
        int kb = 0, a = 0, keep_s = 0, keep_a = 0;
        bool ratios_staged = false, marks_staged = false;
        auto need_marks = [&]() {   // marks a and a + 1 (where it exists) are in LDS
            if (marks_staged && a + 1 < kb + PS_MARKS) return;
            __syncthreads();
            kb = a;
            for (int i = lane; i < PS_MARKS && kb + i < n_marks; i += 64) {
                mk[i] = marks_b[kb + i];
                pk[i] = periods_b[kb + i];
            }
            marks_staged = true;
            __syncthreads();
        };
        long s = 0;
        for (; j < J; ++j) {
            need_marks();
            if (j == 0) s = mk[0];
            if (!ratios_staged || s >= sb + PS_STAGE) {
                __syncthreads();
                sb = s;
                fbase = g.frame_of(sb);
                const int flast = g.frame_of(sb + PS_STAGE - 1);
                for (int f = fbase + lane; f <= flast; f += 64) xs[f - fbase] = ratio_b[f];
                ratios_staged = true;
                __syncthreads();
            }
            const int pa = pk[a - kb];
            if (lane == (j & 63)) {
                keep_s = (int)s;
                keep_a = a;
            }
            if ((j & 63) == 63) {
                pos_b[j - 63 + lane] = keep_s;
                src_b[j - 63 + lane] = keep_a;
            }
            const double q = pa > 0 ? (double)xs[g.frame_of(s) - fbase] : 1.0;
            const int step = max(1, (int)floor((double)abs(pa) / q + 0.5));
            const long s2 = s + step;
            if (s2 >= n) {
                ++j;
                break;
            }
            while (a + 1 < n_marks) {   // |m_k - s2| falls and then rises along k: stop at the first k that is not closer
                need_marks();
                const long here = mk[a - kb], next = mk[a + 1 - kb];
                if (!(labs(next - s2) < labs(here - s2))) break;
                ++a;
            }
            s = s2;
        }
        if (lane < (j & 63)) {
            pos_b[(j & ~63) + lane] = keep_s;
            src_b[(j & ~63) + lane] = keep_a;
        }
    }
    if (lane == 0) {
        counts_out[(size_t)b * GVX_PSOLA_ROW_INTS + GVX_PSOLA_MARKS] = n_marks;
        counts_out[(size_t)b * GVX_PSOLA_ROW_INTS + GVX_PSOLA_GRAINS] = j;
        status_out[b] = bad ? GVX_PSOLA_BAD_RATIO : GVX_PSOLA_OK;
    }
}

// ---- the synthesis -------------------------------------------------------------------------------------------------------------

// A workgroup owns row b and the PS_TILE output samples from tile * PS_TILE, one per thread.
//
// Grains.  Grain j reaches a sample of the tile only if t0 - P < s_j < t0 + PS_TILE + P, P = max(lag_max, U): s ascends strictly, so
// these are consecutive and at most PS_TILE + 2 P - 1.  Thread 0 finds the first of them and thread 64 the first behind them by
// bisection (26 halvings cover the largest row); all threads copy their (s, m, p) into LDS.
//
// Samples.  Every thread walks the grains in ascending j - LDS reads that are the same address for the whole wave - and gathers
// x[m + u] from global memory: consecutive threads read consecutive samples.
// LDS: range int32 [2] | s int32 [cap] | m int32 [cap] | p int32 [cap], cap = PS_TILE + 2 P.
__global__ void __launch_bounds__(PS_TILE)
psola_synth_kernel(const float* wav, const int32_t* sample_lengths, const int32_t* marks, const int32_t* periods, const int32_t* syn_pos,
                   const int32_t* syn_src, const int32_t* counts, const int32_t* status, long N, int tiles, int P, int K, int J, float* wav_out) {
    extern __shared__ __attribute__((aligned(16))) int32_t ps_lds[];
    const int cap = PS_TILE + 2 * P;
    int32_t* range = ps_lds;
    int32_t* gs = ps_lds + 2;
    int32_t* gm = gs + cap;
    int32_t* gp = gm + cap;
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles, tid = threadIdx.x;
    const long n = ps_len(sample_lengths, b, N);
    const long t0 = (long)tile * PS_TILE, t = t0 + tid;
    const float* x = wav + (size_t)b * N;
    float* y = wav_out + (size_t)b * N;
    const int n_marks = min(max(counts[(size_t)b * GVX_PSOLA_ROW_INTS + GVX_PSOLA_MARKS], 0), K);
    const int n_grains = min(max(counts[(size_t)b * GVX_PSOLA_ROW_INTS + GVX_PSOLA_GRAINS], 0), J);
    if (t0 >= n || status[b] != GVX_PSOLA_OK || n_grains == 0 || n_marks == 0) {   // the whole workgroup: no barrier is left half attended
        if (t < N) y[t] = t < n ? x[t] : 0.f;
        return;
    }
    const int32_t* pos_b = syn_pos + (size_t)b * J;
    const int32_t* src_b = syn_src + (size_t)b * J;
    if (tid == 0 || tid == 64) {
        const long bound = tid == 0 ? t0 - P : t0 + PS_TILE + P - 1;   // the first j with s_j > bound
        int lo = 0, hi = n_grains;
        for (int it = 0; it < 26 && lo < hi; ++it) {
            const int mid = (lo + hi) >> 1;
            if ((long)pos_b[mid] > bound) hi = mid;
            else lo = mid + 1;
        }
        range[tid >> 6] = lo;
    }
    __syncthreads();
    const int j0 = range[0], G = min(range[1] - j0, cap);
    for (int i = tid; i < G; i += PS_TILE) {
        const int a = min(max(src_b[j0 + i], 0), n_marks - 1);
        gs[i] = pos_b[j0 + i];
        gm[i] = marks[(size_t)b * K + a];
        gp[i] = min(max(abs(periods[(size_t)b * K + a]), 1), P);
    }
    __syncthreads();
    if (t >= N) return;   // no barrier follows
    if (t >= n) {
        y[t] = 0.f;
        return;
    }
    float num = 0.f, den = 0.f;
    for (int i = 0; i < G; ++i) {
        const long u = t - gs[i];
        const int pg = gp[i];
        const long au = u < 0 ? -u : u;
        if (au < pg) {
            const float v = 1.f - (float)au / (float)pg;
            const float w = (v * v) * (3.f - 2.f * v);
            const long at = (long)gm[i] + u;
            const float xv = (at >= 0 && at < n) ? x[at] : 0.f;
            num = fmaf(w, xv, num);
            den = den + w;
        }
    }
    const long s_first = pos_b[0], s_last = pos_b[n_grains - 1];
    float out;
    if (t >= s_first && t <= s_last) out = num / fmaxf(den, 0.5f);
    else out = den >= 1.f ? num / den : fmaf(1.f - den, x[t], num);
    y[t] = out;
}

int psola_check(const gvx_psola_params* p, int B, long N) {
    if (!p) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (B < 1 || N < 1) return fail(GVX_ERR_INVALID_ARG, "B and N must be >= 1");
    if (p->hop < 1 || p->lag_min < 1 || p->unvoiced_period < 1 || p->lag_max < p->lag_min)
        return fail(GVX_ERR_INVALID_ARG, "hop = %d, lag_min = %d, lag_max = %d, unvoiced_period = %d: all must be >= 1 and lag_min <= lag_max", p->hop,
                    p->lag_min, p->lag_max, p->unvoiced_period);
    if (p->lag_max > GVX_PITCH_MAX_LAG || p->unvoiced_period > GVX_PITCH_MAX_LAG)
        return fail(GVX_ERR_UNSUPPORTED, "lag_max = %d / unvoiced_period = %d is beyond the limit of %d samples", p->lag_max, p->unvoiced_period,
                    GVX_PITCH_MAX_LAG);
    if (B > GVX_PITCH_MAX_ROWS) return fail(GVX_ERR_UNSUPPORTED, "B = %d is above %d rows", B, GVX_PITCH_MAX_ROWS);
    if ((N + p->hop - 1) / p->hop > GVX_PITCH_MAX_FRAMES)
        return fail(GVX_ERR_UNSUPPORTED, "%ld samples at hop %d are more than %d frames", N, p->hop, GVX_PITCH_MAX_FRAMES);
    if (N > (long)GVX_PITCH_MAX_FRAMES * GVX_PITCH_MAX_LAG)
        return fail(GVX_ERR_UNSUPPORTED, "%ld samples are more than %ld", N, (long)GVX_PITCH_MAX_FRAMES * GVX_PITCH_MAX_LAG);
    return GVX_OK;
}

}  // namespace

extern "C" {

long gvx_psola_max_marks(long N, int p_min) {
    if (N < 1 || p_min < 1) return 0;
    return N / ((3 * (long)p_min + 3) / 4) + 1;
}

long gvx_psola_max_grains(long N, int p_min) {
    if (N < 1 || p_min < 1) return 0;
    return N / std::max(1L, ((long)p_min + 1) / 2) + 1;
}

int gvx_psola_plan(const float* wav, const int32_t* sample_lengths, const int32_t* lag, const float* ratio, int B, long N,
                   const gvx_psola_params* params, int32_t* marks_out, int32_t* periods_out, int32_t* syn_pos_out, int32_t* syn_src_out,
                   int32_t* counts_out, int32_t* row_status_out, void* stream) {
    const int rc = psola_check(params, B, N);
    if (rc != GVX_OK) return rc;
    if (!wav || !lag || !ratio || !marks_out || !periods_out || !syn_pos_out || !syn_src_out || !counts_out || !row_status_out)
        return fail(GVX_ERR_INVALID_ARG, "null argument");
    const int p_min = std::min(params->lag_min, params->unvoiced_period);
    const int K = (int)gvx_psola_max_marks(N, p_min), J = (int)gvx_psola_max_grains(N, p_min);   // N <= 2^25: both fit
    psola_plan_kernel<<<B, 64, 0, (hipStream_t)stream>>>(wav, sample_lengths, lag, ratio, N, gvx_pitch_frames(N, params->hop), *params, K, J,
                                                         marks_out, periods_out, syn_pos_out, syn_src_out, counts_out, row_status_out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int gvx_psola_synth(const float* wav, const int32_t* sample_lengths, const int32_t* marks, const int32_t* periods, const int32_t* syn_pos,
                    const int32_t* syn_src, const int32_t* counts, const int32_t* row_status, int B, long N, const gvx_psola_params* params,
                    float* wav_out, void* stream) {
    const int rc = psola_check(params, B, N);
    if (rc != GVX_OK) return rc;
    if (!wav || !marks || !periods || !syn_pos || !syn_src || !counts || !row_status || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const int p_min = std::min(params->lag_min, params->unvoiced_period), P = std::max(params->lag_max, params->unvoiced_period);
    const int K = (int)gvx_psola_max_marks(N, p_min), J = (int)gvx_psola_max_grains(N, p_min);
    const long tiles = (N + PS_TILE - 1) / PS_TILE;
    if ((long)B * tiles > 0x7fffffffL) return fail(GVX_ERR_UNSUPPORTED, "B = %d rows of %ld tiles are beyond one launch's grid", B, tiles);
    const size_t lds = (2 + 3 * (size_t)(PS_TILE + 2 * P)) * sizeof(int32_t);
    psola_synth_kernel<<<(unsigned)(B * tiles), PS_TILE, lds, (hipStream_t)stream>>>(wav, sample_lengths, marks, periods, syn_pos, syn_src, counts,
                                                                                    row_status, N, (int)tiles, P, K, J, wav_out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

}  // C ABI
