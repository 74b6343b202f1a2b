// Speaking rate control on the device: the plan (gvx_duration_scale: how many frames every token gets at a speed and per-token
// rates) and the warp (gvx_mel_time_warp: the mel resampled token by token, centre to centre).  The definitions are in
// include/genvox_amd.h; the numpy restatements the tests hold these kernels to are in tests/warp_ref.py.
//
// Order of this file: the plan's kernel, the warp's kernel, the C ABI.
#include "gvx_internal.h"

using gvx::fail;

namespace {

constexpr int TW_THREADS = 256;
constexpr int TW_WAVES = TW_THREADS / 64;
constexpr int TW_TILE = GVX_WARP_TILE_FRAMES;   // output frames of a workgroup: one per lane of a wave
constexpr int TW_UNROLL = 4;                    // channels a wave has in flight
constexpr int TW_SAT = 1 << 30;                 // a start that no frame index reaches: 64-bit sums are stored saturated at it
static_assert(TW_TILE == 64, "a wave's lanes are the frames of a tile");
static_assert(GVX_MAS_MAX_FRAMES < TW_SAT, "a saturated start lies behind every frame");

__device__ __forceinline__ int tw_len(const int32_t* lens, int b, int full) {
    if (!lens) return full;
    const int v = lens[b];
    return v < 0 ? 0 : (v > full ? full : v);
}
__device__ __forceinline__ int tw_sat(long long v) { return v > TW_SAT ? TW_SAT : (int)v; }

// One workgroup per row.  All threads form the quotients d_l / e_l into LDS and look for a bad token; thread 0 walks the sum in
// ascending l (the order is the definition: every add rounds) and leaves the starts in LDS; all threads write the outputs.
// LDS: q double [L] | starts int32 [L + 1] | result int32 [2] (status, T').
__global__ void __launch_bounds__(TW_THREADS)
duration_scale_kernel(const int32_t* durations, const int32_t* token_lengths, const float* rates, int L, double speed, int32_t* target_durations,
                      int32_t* target_starts, int32_t* out_lengths, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tw_lds[];
    double* q = reinterpret_cast<double*>(tw_lds);
    int32_t* S = reinterpret_cast<int32_t*>(tw_lds + (size_t)L * sizeof(double));
    int32_t* result = S + (L + 1);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Lb = tw_len(token_lengths, b, L);
    const int32_t* d_b = durations + (size_t)b * L;
    const float* r_b = rates ? rates + (size_t)b * L : nullptr;

    int bad = 0;
    for (int l = tid; l < Lb; l += TW_THREADS) {
        const int d = d_b[l];
        const double e = speed * (double)(r_b ? r_b[l] : 1.f);
        const bool ok = d >= 0 && e >= (double)GVX_RATE_MIN && e <= (double)GVX_RATE_MAX;   // a NaN fails both comparisons
        bad |= !ok;
        q[l] = ok ? (double)d / e : 0.0;   // > 0 exactly when d > 0: e is at most 8
    }
    bad = __syncthreads_or(bad);   // also: q is complete
    if (tid == 0) {
        int st = GVX_WARP_OK;
        long long Sl = 0;
        if (Lb == 0) {
            st = GVX_WARP_EMPTY;
        } else if (bad) {
            st = GVX_WARP_BAD;
        } else {
            double E = 0.0;
#pragma unroll 8
            for (int l = 0; l < Lb; ++l) {
                const double ql = q[l];
                E = E + ql;
                const long long c = (long long)__builtin_rint(E);   // llrint: to nearest, half to even
                S[l] = tw_sat(Sl);
                const long long step = Sl + (ql > 0.0 ? 1 : 0);
                Sl = step > c ? step : c;
            }
            S[Lb] = tw_sat(Sl);
            if (Sl == 0) st = GVX_WARP_EMPTY;
            else if (Sl > GVX_MAS_MAX_FRAMES) st = GVX_WARP_BAD;
        }
        result[0] = st;
        result[1] = st == GVX_WARP_OK ? (int)Sl : 0;
    }
    __syncthreads();
    const bool ok = result[0] == GVX_WARP_OK;
    int32_t* td_b = target_durations + (size_t)b * L;
    int32_t* ts_b = target_starts ? target_starts + (size_t)b * L : nullptr;
    for (int l = tid; l < L; l += TW_THREADS) {
        const bool in = ok && l < Lb;
        td_b[l] = in ? S[l + 1] - S[l] : 0;
        if (ts_b) ts_b[l] = in ? S[l] : -1;
    }
    if (tid == 0) {
        out_lengths[b] = result[1];
        status[b] = result[0];
    }
}

// A workgroup owns row b and the TW_TILE output frames from tile * TW_TILE, for all M channels.
//
// Sums.  The row's tokens are dealt to the threads in runs of `chunk` consecutive ones; a thread copies its run of d and d' into
// LDS while it adds them up (64 bits) and checks them, the run totals are scanned (shuffles inside a wave, four wave totals through
// LDS), and the thread turns its own run into starts in place.  Every workgroup of a row does this for itself - L ints against
// M * TW_TILE floats - so that no workgroup waits for another; tile 0 reports the row's status.
//
// Frames.  Wave 0: lane i finds the token of frame u = tile * TW_TILE + i by bisection over the target starts (the last token
// whose start is <= u: of tokens that share a start, the one that has frames) and computes i0 and frac in integers, once per frame.
//
// Channels.  Wave w streams channels w, w + 4, ...: lane i reads x[m][i0] (and x[m][i0 + 1] where frac != 0) - addresses that
// ascend with the lane - and stores out[m][u], 64 consecutive floats per wave.
// LDS: wave totals int64 [2][TW_WAVES] | i0 int32 [TW_TILE] | frac fp32 [TW_TILE] | S int32 [L + 1] | S' int32 [L + 1].
__global__ void __launch_bounds__(TW_THREADS)
mel_time_warp_kernel(const float* mel, const int32_t* durations, const int32_t* target_durations, const int32_t* token_lengths, int M, int T, int L,
                     int T_out, int tiles, float* mel_out, int32_t* src_frame, float* src_frac, int32_t* status) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tw_lds[];
    long long* wtot = reinterpret_cast<long long*>(tw_lds);
    int32_t* fr_i0 = reinterpret_cast<int32_t*>(wtot + 2 * TW_WAVES);
    float* fr_frac = reinterpret_cast<float*>(fr_i0 + TW_TILE);
    int32_t* S = reinterpret_cast<int32_t*>(fr_frac + TW_TILE);
    int32_t* Sp = S + (L + 1);
    const int b = blockIdx.x / tiles, tile = blockIdx.x - b * tiles;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Lb = tw_len(token_lengths, b, L);
    const int32_t* d_b = durations + (size_t)b * L;
    const int32_t* dp_b = target_durations + (size_t)b * L;

    // ---- sums
    const int chunk = (Lb + TW_THREADS - 1) / TW_THREADS;
    const int lo = min(tid * chunk, Lb), hi = min(lo + chunk, Lb);
    long long sum_d = 0, sum_p = 0;
    int bad = 0;
    for (int l = lo; l < hi; ++l) {   // at most GVX_MAS_MAX_TOKENS / TW_THREADS = 16 tokens
        const int d = d_b[l], p = dp_b[l];
        bad |= (d < 0) | (p < 0) | ((d > 0) != (p > 0));
        S[l] = d;
        Sp[l] = p;
        sum_d += d;
        sum_p += p;
    }
    long long inc_d = sum_d, inc_p = sum_p;   // inclusive scan over the wave's 64 run totals
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long od = __shfl_up(inc_d, off), op = __shfl_up(inc_p, off);
        if (lane >= off) {
            inc_d += od;
            inc_p += op;
        }
    }
    if (lane == 63) {
        wtot[wave] = inc_d;
        wtot[TW_WAVES + wave] = inc_p;
    }
    bad = __syncthreads_or(bad);   // also: the wave totals are there
    long long run_d = inc_d - sum_d, run_p = inc_p - sum_p, Tb = 0, Tpb = 0;
#pragma unroll
    for (int w = 0; w < TW_WAVES; ++w) {
        const long long wd = wtot[w], wp = wtot[TW_WAVES + w];
        if (w < wave) {
            run_d += wd;
            run_p += wp;
        }
        Tb += wd;
        Tpb += wp;
    }
    for (int l = lo; l < hi; ++l) {   // the thread's own run, in place: counts -> starts
        const int d = S[l], p = Sp[l];
        S[l] = tw_sat(run_d);
        Sp[l] = tw_sat(run_p);
        run_d += d;
        run_p += p;
    }
    if (tid == 0) {
        S[Lb] = tw_sat(Tb);
        Sp[Lb] = tw_sat(Tpb);
    }
    bad |= Tb > T;
    const bool empty = Lb == 0 || Tpb == 0;
    const int Tlen = (bad || empty) ? 0 : (int)(Tpb < T_out ? Tpb : T_out);   // frames of this row that are computed
    if (tile == 0 && tid == 0) status[b] = bad ? GVX_WARP_BAD : empty ? GVX_WARP_EMPTY : Tpb > T_out ? GVX_WARP_CUT : GVX_WARP_OK;
    __syncthreads();

    // ---- frames
    const int u0 = tile * TW_TILE;
    if (wave == 0) {
        const int u = u0 + lane;
        int i0 = -1;
        float frac = 0.f;
        if (u < Tlen) {
            int l = 0, end = Lb;   // S'[l] <= u < S'[end]
            for (int it = 0; it < 13 && end - l > 1; ++it) {   // 13 halvings cover GVX_MAS_MAX_TOKENS
                const int mid = (l + end) >> 1;
                if (Sp[mid] <= u) l = mid;
                else end = mid;
            }
            const long long d = d_b[l], p = dp_b[l];   // the counts themselves: a saturated start would falsify a difference
            const long long n = (2ll * (u - Sp[l]) + 1) * d - p, den = 2 * p;
            long long quo = n / den, rem = n - quo * den;
            if (rem < 0) {   // floor, not truncation
                rem += den;
                quo -= 1;
            }
            const long long i = S[l] + quo;
            frac = (float)((double)rem / (double)den);
            i0 = (int)i;
            if (i < 0) {
                i0 = 0;
                frac = 0.f;
            }
            if (i >= Tb - 1) {
                i0 = (int)Tb - 1;
                frac = 0.f;
            }
        }
        fr_i0[lane] = i0;
        fr_frac[lane] = frac;
        if (u < T_out) {
            if (src_frame) src_frame[(size_t)b * T_out + u] = i0;
            if (src_frac) src_frac[(size_t)b * T_out + u] = frac;
        }
    }
    __syncthreads();

    // ---- channels
    const int u = u0 + lane;
    if (u >= T_out) return;   // no barrier follows
    const int i0 = fr_i0[lane];
    const float frac = fr_frac[lane];
    const bool valid = u < Tlen, two = frac != 0.f;
    const float* x_b = mel + (size_t)b * M * T;
    float* o_b = mel_out + (size_t)b * M * T_out + u;
    for (int m0 = wave; m0 < M; m0 += TW_WAVES * TW_UNROLL) {
        float x0[TW_UNROLL], x1[TW_UNROLL];
#pragma unroll
        for (int k = 0; k < TW_UNROLL; ++k) {
            const int m = m0 + k * TW_WAVES;
            x0[k] = x1[k] = 0.f;
            if (m < M && valid) {
                const float* x = x_b + (size_t)m * T + i0;
                x0[k] = x[0];
                if (two) x1[k] = x[1];
            }
        }
#pragma unroll
        for (int k = 0; k < TW_UNROLL; ++k) {
            const int m = m0 + k * TW_WAVES;
            if (m < M) o_b[(size_t)m * T_out] = two ? fmaf(frac, x1[k] - x0[k], x0[k]) : x0[k];
        }
    }
}

int tw_check_tokens(int B, int L) {
    if (B < 1 || L < 1) return fail(GVX_ERR_INVALID_ARG, "B and L must be >= 1");
    if (L > GVX_MAS_MAX_TOKENS) return fail(GVX_ERR_UNSUPPORTED, "L = %d is beyond the limit of %d tokens", L, GVX_MAS_MAX_TOKENS);
    return GVX_OK;
}

}  // namespace

extern "C" {

int gvx_duration_scale(const int32_t* durations, const int32_t* token_lengths, const float* rates, int B, int L, float speed,
                       int32_t* target_durations_out, int32_t* target_starts_out, int32_t* out_lengths_out, int32_t* row_status_out, void* stream) {
    const int rc = tw_check_tokens(B, L);
    if (rc != GVX_OK) return rc;
    if (!durations || !target_durations_out || !out_lengths_out || !row_status_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!(speed >= GVX_RATE_MIN && speed <= GVX_RATE_MAX))
        return fail(GVX_ERR_INVALID_ARG, "speed = %g is outside [%g, %g]", (double)speed, (double)GVX_RATE_MIN, (double)GVX_RATE_MAX);
    const size_t lds = (size_t)L * sizeof(double) + (size_t)(L + 1 + 2) * sizeof(int32_t);
    duration_scale_kernel<<<B, TW_THREADS, lds, (hipStream_t)stream>>>(durations, token_lengths, rates, L, (double)speed, target_durations_out,
                                                                      target_starts_out, out_lengths_out, row_status_out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int gvx_mel_time_warp(const float* mel, const int32_t* durations, const int32_t* target_durations, const int32_t* token_lengths, int B, int M, int T,
                      int L, int T_out, float* mel_out, int32_t* src_frame_out, float* src_frac_out, int32_t* row_status_out, void* stream) {
    if (M < 1 || T < 1 || T_out < 1) return fail(GVX_ERR_INVALID_ARG, "M, T and T_out must be >= 1");
    const int rc = tw_check_tokens(B, L);
    if (rc != GVX_OK) return rc;
    if (T > GVX_MAS_MAX_FRAMES || T_out > GVX_MAS_MAX_FRAMES)
        return fail(GVX_ERR_UNSUPPORTED, "T = %d / T_out = %d is beyond the limit of %d frames", T, T_out, GVX_MAS_MAX_FRAMES);
    if (!mel || !durations || !target_durations || !mel_out || !row_status_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const int tiles = (T_out + TW_TILE - 1) / TW_TILE;
    if ((long long)B * tiles > 0x7fffffffll) return fail(GVX_ERR_UNSUPPORTED, "B = %d rows of %d tiles are beyond one launch's grid", B, tiles);
    const size_t lds = 2 * TW_WAVES * sizeof(long long) + TW_TILE * (sizeof(int32_t) + sizeof(float)) + 2 * (size_t)(L + 1) * sizeof(int32_t);
    mel_time_warp_kernel<<<B * tiles, TW_THREADS, lds, (hipStream_t)stream>>>(mel, durations, target_durations, token_lengths, M, T, L, T_out, tiles,
                                                                             mel_out, src_frame_out, src_frac_out, row_status_out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

}  // C ABI
