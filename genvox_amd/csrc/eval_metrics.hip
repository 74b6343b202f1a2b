// Evaluation by synthesis on the device: statistics of an attention alignment (is it a sharp, monotonic diagonal?) and the distance
// between a free-running mel and its target under dynamic time warping.  The definitions are in include/genvox_amd.h; the float64
// restatement the tests hold these kernels to is tests/metrics_ref64.py.
//
// Order of this file: alignment statistics, the projection, the warp, the C ABI.
#include "gvx_internal.h"

#include <algorithm>
#include <climits>

using gvx::fail;

namespace {

__device__ __forceinline__ int em_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int em_len(const int32_t* lens, int b, int full) { return lens ? em_clamp(lens[b], full) : full; }

// ---- alignment statistics ---------------------------------------------------------------------------------------------------

constexpr int AL_THREADS = 256;
constexpr int AL_WAVES = AL_THREADS / 64;
constexpr int AL_HIST = 4096;   // tokens whose frame counts a workgroup holds in LDS at a time

// (v2, p2) replaces (v1, p1) when it is the larger value, or the same value at a lower index.  A lane that saw nothing holds
// (-inf, INT_MAX); a NaN is never v2 here (the scan below does not take one) and never wins a comparison.
__device__ __forceinline__ void al_take(float& v1, int& p1, float v2, int p2) {
    if (v2 > v1 || (v2 == v1 && p2 < p1)) { v1 = v2; p1 = p2; }
}

// One wave per frame: peak[b][t] = max_l a[b][t][l] over l < L_b, pos[b][t] = the lowest l that attains it.  Comparisons only.
// Frames t >= T_b (and every frame of a row with L_b == 0) get pos -1, peak 0 and are not read.
__global__ void __launch_bounds__(AL_THREADS)
align_frames_kernel(const float* a, const int32_t* mel_lengths, const int32_t* token_lengths, int T, int L, int32_t* positions, float* peaks) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int Tb = em_len(mel_lengths, b, T), Lb = em_len(token_lengths, b, L);
    for (int t = blockIdx.x * AL_WAVES + (threadIdx.x >> 6); t < T; t += gridDim.x * AL_WAVES) {
        const long o = (long)b * T + t;
        if (t >= Tb || Lb == 0) {
            if (lane == 0) { positions[o] = -1; peaks[o] = 0.f; }
            continue;
        }
        const float* row = a + o * L;
        float best = -INFINITY;
        int pos = INT_MAX;
        for (int l = lane; l < Lb; l += 64) {
            const float v = row[l];
            if (v > best || (v == best && pos == INT_MAX)) { best = v; pos = l; }   // ascending l: a tie keeps the lower index
        }
        for (int off = 32; off > 0; off >>= 1) al_take(best, pos, __shfl_xor(best, off), __shfl_xor(pos, off));
        if (lane == 0) {
            const bool none = pos == INT_MAX;   // every entry of the frame is a NaN
            positions[o] = none ? 0 : pos;
            peaks[o] = none ? NAN : best;
        }
    }
}

// One workgroup per row, over the frames' positions and peaks: the frames-per-token table, and the row's numbers.
// row_ints[b] = {monotonic, max_jump, covered, first_pos, last_pos}.  The peaks are summed in a fixed order: thread i adds frames
// i, i + 256, ... in ascending order, then the 256 partial sums are added pairwise at strides 128, 64, ..., 1.
__global__ void __launch_bounds__(AL_THREADS)
align_rows_kernel(const int32_t* positions, const float* peaks, const int32_t* mel_lengths, const int32_t* token_lengths, int T, int L,
                  int32_t* durations, int32_t* row_ints, float* focus) {
    __shared__ int hist[AL_HIST];
    __shared__ float part[AL_THREADS];
    __shared__ int counts[3];   // monotonic, max_jump, covered
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tb = em_len(mel_lengths, b, T), Lb = em_len(token_lengths, b, L);
    const int32_t* pos = positions + (long)b * T;
    int32_t* dur = durations + (long)b * L;
    const bool empty = Tb == 0 || Lb == 0;
    if (tid < 3) counts[tid] = 0;
    __syncthreads();
    // frames per token, AL_HIST tokens at a time (integer counts: the order of the additions does not show)
    for (int l0 = 0; l0 < L; l0 += AL_HIST) {
        const int n = min(AL_HIST, L - l0);
        for (int l = tid; l < n; l += AL_THREADS) hist[l] = 0;
        __syncthreads();
        if (!empty)
            for (int t = tid; t < Tb; t += AL_THREADS) {
                const int p = pos[t] - l0;
                if (p >= 0 && p < n) atomicAdd(&hist[p], 1);
            }
        __syncthreads();
        int cov = 0;
        for (int l = tid; l < n; l += AL_THREADS) {
            dur[l0 + l] = hist[l];
            cov += hist[l] > 0;
        }
        if (cov) atomicAdd(&counts[2], cov);
        __syncthreads();
    }
    int mono = 0, jump = 0;
    float s = 0.f;
    if (!empty) {
        for (int t = tid; t < Tb; t += AL_THREADS) s += peaks[(long)b * T + t];
        for (int t = 1 + tid; t < Tb; t += AL_THREADS) {
            const int d = pos[t] - pos[t - 1];
            mono += d >= 0;
            jump = max(jump, d < 0 ? -d : d);
        }
    }
    if (mono) atomicAdd(&counts[0], mono);
    if (jump) atomicMax(&counts[1], jump);
    part[tid] = s;
    __syncthreads();
    for (int stride = AL_THREADS / 2; stride > 0; stride >>= 1) {
        if (tid < stride) part[tid] += part[tid + stride];
        __syncthreads();
    }
    if (tid == 0) {
        int32_t* r = row_ints + (long)b * GVX_ALIGN_ROW_INTS;
        r[0] = counts[0];
        r[1] = counts[1];
        r[2] = counts[2];
        r[3] = empty ? 0 : pos[0];
        r[4] = empty ? 0 : pos[Tb - 1];
        focus[b] = empty ? NAN : part[0] / (float)Tb;
    }
}

// ---- projection: c[b][t][k] = sum_m P[k][m] * mel[b][m][t] ----------------------------------------------------------------------

constexpr size_t EM_LDS_BYTES = 160 * 1024;   // a CU's LDS: what a workgroup of the two kernels below may ask for
constexpr int PJ_THREADS = 256;
constexpr int PJ_FRAMES = 64;   // frames of a tile: a wave reads 64 consecutive frames of one mel channel

// A workgroup takes PJ_FRAMES frames of one row: the tile mel[b][:, t0 .. t0 + 63] and P go to LDS (P at a row stride of M + 1,
// so that threads on neighbouring k do not share a bank), then thread o computes output element o of the tile's [frames][K] block,
// which is contiguous in c.  Every sum runs in ascending m, one fused multiply-add per term.
__global__ void __launch_bounds__(PJ_THREADS)
mel_project_kernel(const float* mel, const float* P, int M, int T, int K, float* c) {
    extern __shared__ __attribute__((aligned(16))) float pj_lds[];
    float* Ps = pj_lds;                    // [K][M + 1]
    float* tile = pj_lds + (size_t)K * (M + 1);   // [M][PJ_FRAMES]
    const int b = blockIdx.y, t0 = blockIdx.x * PJ_FRAMES, nt = min(PJ_FRAMES, T - t0);
    for (int i = threadIdx.x; i < K * M; i += PJ_THREADS) Ps[(i / M) * (M + 1) + i % M] = P[i];
    for (int i = threadIdx.x; i < M * PJ_FRAMES; i += PJ_THREADS) {
        const int m = i / PJ_FRAMES, t = i % PJ_FRAMES;
        tile[i] = t < nt ? mel[((long)b * M + m) * T + t0 + t] : 0.f;
    }
    __syncthreads();
    float* out = c + ((long)b * T + t0) * K;
    for (int o = threadIdx.x; o < nt * K; o += PJ_THREADS) {
        const int t = o / K, k = o % K;
        float acc = 0.f;
        for (int m = 0; m < M; ++m) acc = fmaf(Ps[k * (M + 1) + m], tile[m * PJ_FRAMES + t], acc);
        out[o] = acc;
    }
}

// ---- the warp -------------------------------------------------------------------------------------------------------------------

constexpr int DTW_MAX_THREADS = 1024;


// Row stride of a feature table's LDS image: odd, so that the lanes of a wave, which sit on consecutive frames, read 64 banks.
__host__ __device__ constexpr int dtw_stride(int K) { return K | 1; }

// What a call on (Tp_max, Tg_max, K) does.  lds: both feature tables and the three diagonals fit the CU's LDS.  Otherwise the
// features are read through the cache and the diagonals live in the workspace (3 * Tp_max floats per row): no size limit.
struct DtwPlan {
    bool lds;
    size_t lds_bytes, ws_bytes;
    int threads;
};
inline DtwPlan dtw_plan(int B, int Tp_max, int Tg_max, int K) {
    DtwPlan p;
    const size_t diag = 3 * (size_t)Tp_max * sizeof(float);
    const size_t all = diag + ((size_t)Tp_max + (size_t)Tg_max) * dtw_stride(K) * sizeof(float);
    p.lds = all <= EM_LDS_BYTES;
    p.lds_bytes = p.lds ? all : 0;
    p.ws_bytes = p.lds ? 0 : (((size_t)B * diag + 255) & ~(size_t)255);
    p.threads = std::min(DTW_MAX_THREADS, std::max(64, (std::min(Tp_max, Tg_max) + 63) / 64 * 64));
    return p;
}

// One workgroup per row.  Anti-diagonal s = i + j needs s - 1 and s - 2 only: three rotating diagonals indexed by i, one barrier per
// diagonal (diagonal s + 1 overwrites the buffer of s - 2, which nobody reads after the barrier that ends s).  The cells of a
// diagonal, at most min(Tp, Tg), are dealt to the threads in ascending i; a neighbour outside the rectangle counts as +inf, which
// gives the first row and column of the recurrence.  The loop runs Tp + Tg - 1 times and waits for nothing but its own barrier.
template <bool LDS>
__global__ void __launch_bounds__(DTW_MAX_THREADS)
dtw_kernel(const float* cp, const float* cg, const int32_t* pred_lengths, const int32_t* target_lengths, int Tp_max, int Tg_max, int K,
           float* diag_ws, float* dist, float* acc_out) {
    extern __shared__ __attribute__((aligned(16))) float dtw_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int Tp = em_len(pred_lengths, b, Tp_max), Tg = em_len(target_lengths, b, Tg_max);
    if (Tp == 0 || Tg == 0) {   // the whole workgroup leaves: no barrier is left half attended
        if (tid == 0) dist[b] = NAN;
        return;
    }
    const float* P = cp + (long)b * Tp_max * K;
    const float* G = cg + (long)b * Tg_max * K;
    float* diag = LDS ? dtw_lds : diag_ws + (long)b * 3 * Tp_max;
    int ks = K;
    if constexpr (LDS) {
        ks = dtw_stride(K);
        float* Ps = dtw_lds + 3 * (size_t)Tp_max;
        float* Gs = Ps + (size_t)Tp_max * ks;
        for (int i = tid; i < Tp * K; i += nthr) Ps[(i / K) * ks + i % K] = P[i];
        for (int i = tid; i < Tg * K; i += nthr) Gs[(i / K) * ks + i % K] = G[i];
        P = Ps;
        G = Gs;
        __syncthreads();
    }
    float* acc = acc_out ? acc_out + (long)b * Tp_max * Tg_max : nullptr;
    for (int s = 0; s < Tp + Tg - 1; ++s) {
        float* cur = diag + (size_t)(s % 3) * Tp_max;
        const float* d1 = diag + (size_t)((s + 2) % 3) * Tp_max;   // diagonal s - 1
        const float* d2 = diag + (size_t)((s + 1) % 3) * Tp_max;   // diagonal s - 2
        const int i_lo = max(0, s - Tg + 1), i_hi = min(Tp - 1, s);
        for (int i = i_lo + tid; i <= i_hi; i += nthr) {
            const int j = s - i;
            const float* x = P + (size_t)i * ks;
            const float* y = G + (size_t)j * ks;
            float q = 0.f;
            for (int k = 0; k < K; ++k) {
                const float e = x[k] - y[k];
                q = fmaf(e, e, q);
            }
            const float d = sqrtf(q);
            float v;
            if (s == 0) {
                v = d + d;
            } else {
                const float up = i > 0 ? d1[i - 1] + d : INFINITY;            // from (i - 1, j)
                const float left = j > 0 ? d1[i] + d : INFINITY;              // from (i, j - 1)
                const float both = (i > 0 && j > 0) ? d2[i - 1] + (d + d) : INFINITY;   // from (i - 1, j - 1)
                v = fminf(fminf(up, left), both);
            }
            cur[i] = v;
            if (acc) acc[(size_t)i * Tg_max + j] = v;
        }
        if constexpr (!LDS) __threadfence_block();
        __syncthreads();
    }
    if (tid == 0) dist[b] = diag[(size_t)((Tp + Tg - 2) % 3) * Tp_max + Tp - 1] / (float)(Tp + Tg);
}

int dtw_check_shape(int B, int Tp_max, int Tg_max, int K) {
    if (B < 1 || Tp_max < 1 || Tg_max < 1 || K < 1) return fail(GVX_ERR_INVALID_ARG, "B, Tp_max, Tg_max and K must be >= 1");
    if (Tp_max > GVX_DTW_MAX_FRAMES || Tg_max > GVX_DTW_MAX_FRAMES || K > GVX_DTW_MAX_FEATURES)
        return fail(GVX_ERR_UNSUPPORTED, "Tp_max = %d / Tg_max = %d / K = %d is beyond the warp's limits (%d frames, %d features)", Tp_max, Tg_max, K,
                    GVX_DTW_MAX_FRAMES, GVX_DTW_MAX_FEATURES);
    return GVX_OK;
}

}  // namespace

extern "C" {

int gvx_alignment_stats(const float* alignments, const int32_t* mel_lengths, const int32_t* token_lengths, int B, int T, int L,
                        int32_t* positions_out, int32_t* durations_out, float* peaks_out, int32_t* row_ints_out, float* focus_out, void* stream) {
    if (!alignments || !positions_out || !durations_out || !peaks_out || !row_ints_out || !focus_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (B < 1 || T < 1 || L < 1) return fail(GVX_ERR_INVALID_ARG, "B, T and L must be >= 1");
    if (B > 65535) return fail(GVX_ERR_UNSUPPORTED, "B = %d is above the 65535 rows of one call", B);
    hipStream_t s = (hipStream_t)stream;
    const unsigned gx = (unsigned)std::min(4096, (T + AL_WAVES - 1) / AL_WAVES);
    align_frames_kernel<<<dim3(gx, B), AL_THREADS, 0, s>>>(alignments, mel_lengths, token_lengths, T, L, positions_out, peaks_out);
    HIP_TRY(hipGetLastError());
    align_rows_kernel<<<B, AL_THREADS, 0, s>>>(positions_out, peaks_out, mel_lengths, token_lengths, T, L, durations_out, row_ints_out, focus_out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int gvx_mel_project(const float* mel, int B, int M, int T, const float* P, int K, float* out, void* stream) {
    if (!mel || !P || !out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (B < 1 || M < 1 || T < 1) return fail(GVX_ERR_INVALID_ARG, "B, M and T must be >= 1");
    if (K < 1 || K > M) return fail(GVX_ERR_INVALID_ARG, "K = %d is outside [1, M = %d]", K, M);
    if (B > 65535) return fail(GVX_ERR_UNSUPPORTED, "B = %d is above the 65535 rows of one call", B);
    const size_t bytes = ((size_t)K * (M + 1) + (size_t)M * PJ_FRAMES) * sizeof(float);
    if (bytes > EM_LDS_BYTES) return fail(GVX_ERR_UNSUPPORTED, "a projection of %d x %d does not fit the kernel's LDS tile", K, M);
    if (bytes > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mel_project_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    mel_project_kernel<<<dim3((T + PJ_FRAMES - 1) / PJ_FRAMES, B), PJ_THREADS, bytes, (hipStream_t)stream>>>(mel, P, M, T, K, out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

size_t gvx_dtw_workspace_bytes(int B, int Tp_max, int Tg_max, int K) {
    if (dtw_check_shape(B, Tp_max, Tg_max, K) != GVX_OK) return 0;
    return dtw_plan(B, Tp_max, Tg_max, K).ws_bytes;
}

int gvx_dtw_uses_lds_tables(int Tp_max, int Tg_max, int K) {
    if (dtw_check_shape(1, Tp_max, Tg_max, K) != GVX_OK) return -1;
    return dtw_plan(1, Tp_max, Tg_max, K).lds ? 1 : 0;
}

int gvx_dtw_distance(const float* cp, const float* cg, const int32_t* pred_lengths, const int32_t* target_lengths, int B, int Tp_max,
                     int Tg_max, int K, float* dist_out, float* acc_out, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = dtw_check_shape(B, Tp_max, Tg_max, K);
    if (rc != GVX_OK) return rc;
    if (!cp || !cg || !dist_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const DtwPlan p = dtw_plan(B, Tp_max, Tg_max, K);
    if (p.ws_bytes) {
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255)) return fail(GVX_ERR_WORKSPACE, "workspace must be non-null and 256-byte aligned");
        if (workspace_bytes < p.ws_bytes) return fail(GVX_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, p.ws_bytes);
    }
    hipStream_t s = (hipStream_t)stream;
    if (p.lds) {
        if (p.lds_bytes > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(dtw_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
        dtw_kernel<true><<<B, p.threads, p.lds_bytes, s>>>(cp, cg, pred_lengths, target_lengths, Tp_max, Tg_max, K, nullptr, dist_out, acc_out);
    } else {
        dtw_kernel<false><<<B, p.threads, 0, s>>>(cp, cg, pred_lengths, target_lengths, Tp_max, Tg_max, K, static_cast<float*>(workspace), dist_out, acc_out);
    }
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

}  // C ABI
