// Monotonic alignment search on the device: the best path through an attention alignment that starts on the first token, ends on
// the last and stays or advances by one token per frame - which frames belong to which token.  The definition is in
// include/genvox_amd.h; the numpy restatements the tests hold this kernel to are in tests/mas_ref.py.
//
// Order of this file: the plan, the kernel (forward recurrence, backtrack, row outputs), the C ABI.
#include "gvx_internal.h"

#include <algorithm>

using gvx::fail;

namespace {

constexpr size_t MAS_LDS_BYTES = 160 * 1024;   // a CU's LDS
constexpr int MAS_MAX_THREADS = 1024;
constexpr int MAS_MAX_DEAL = 4;   // tokens of a thread: GVX_MAS_MAX_TOKENS over MAS_MAX_THREADS
// frames of alignment weights a thread holds in registers ahead of the frame it computes: 8 with the bit table in LDS, 4 with the
// table in the workspace (its 64-bit store addresses take the registers: 8 there spills under the 128 of a 1024-thread workgroup)
constexpr int MAS_DEPTH_LDS = 8, MAS_DEPTH_WS = 4;
static_assert(MAS_MAX_THREADS * MAS_MAX_DEAL >= GVX_MAS_MAX_TOKENS, "a workgroup holds a whole row of tokens");

__device__ __forceinline__ int mas_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int mas_len(const int32_t* lens, int b, int full) { return lens ? mas_clamp(lens[b], full) : full; }

// What a call on (B, T, L) does.  Token l belongs to thread l % threads, one token per thread up to 1024 tokens and up to four
// beyond; the back-pointers of a frame are words = ceil(L / 64) 64-bit masks.  lds: the two Q rows and the T x words back-pointer
// table fit the CU's LDS; otherwise the table lives in the workspace.  (One wave with four tokens per lane for L <= 256, which has
// no barrier to wait at, was measured and is slower: the four cells of a lane run one after the other - EXPERIMENTS.md,
// "Monotonic alignment search".)
struct MasPlan {
    bool lds;
    int threads, deal, words;
    size_t lds_bytes, ws_bytes;
};
inline MasPlan mas_plan(int B, int T, int L) {
    MasPlan p;
    p.words = (L + 63) / 64;
    p.threads = std::min(MAS_MAX_THREADS, (L + 63) / 64 * 64);
    p.deal = (L + p.threads - 1) / p.threads;
    const size_t q = 2 * (size_t)L * sizeof(float), table = (size_t)T * p.words * sizeof(uint64_t);
    p.lds = q + table <= MAS_LDS_BYTES;
    p.lds_bytes = p.lds ? q + table : q;
    p.ws_bytes = p.lds ? 0 : (((size_t)B * table + 255) & ~(size_t)255);
    return p;
}

// One workgroup per row.
//
// Forward.  Q of frame t - 1 and of frame t are two rows in LDS; a thread computes its cells of frame t from the first and writes
// them to the second, one barrier per frame.  Only reachable cells (l <= t) are read, computed or written: what a cell reads from
// an unreachable neighbour is taken as -inf without looking.  "Advance wins" is one bit per cell: a wave's ballot is the 64-bit
// word of its 64 tokens (thread counts are multiples of 64, so token l sits in bit l % 64 of word l / 64), written by lane 0.  The
// weights of the next MAS_DEPTH (8 or 4) frames wait in registers: the load of frame t + MAS_DEPTH is issued when frame t is used, so that
// the row walks at the pace of its arithmetic, not of a trip to memory per frame.
//
// Backtrack, by wave 0 alone, 64 frames at a time.  The path descends by at most one token per frame, so over 64 frames it stays
// inside the 64 tokens that end at its current one: lane i fetches, for frame t0 - i, that 64-bit window of the table (all 64
// trips to the table at once), and the walk itself is 64 scalar steps over registers.  `adv` collects the frames at which the
// path advanced; lane i then knows its token from the count of the bits below i.
//
// Row outputs.  starts live in LDS over the Q rows (dead by then); durations are their differences.
template <bool LDS, bool SCORES>
__global__ void __launch_bounds__(MAS_MAX_THREADS)
mas_kernel(const float* a, const int32_t* mel_lengths, const int32_t* token_lengths, int T, int L, int deal, int words, float floor_,
           uint64_t* table_ws, int32_t* path, int32_t* durations, int32_t* starts, float* score, int32_t* status, float* scores) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mas_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63;
    const int Tb = mas_len(mel_lengths, b, T), Lb = mas_len(token_lengths, b, L);
    int32_t* path_b = path ? path + (long)b * T : nullptr;
    int32_t* dur_b = durations + (long)b * L;
    int32_t* st_b = starts ? starts + (long)b * L : nullptr;
    if (Tb == 0 || Lb == 0 || Tb < Lb) {   // the whole workgroup leaves: no barrier is left half attended, nothing of `a` is read
        if (path_b)
            for (int t = tid; t < T; t += nthr) path_b[t] = -1;
        for (int l = tid; l < L; l += nthr) {
            dur_b[l] = 0;
            if (st_b) st_b[l] = -1;
        }
        if (tid == 0) {
            status[b] = (Tb == 0 || Lb == 0) ? GVX_MAS_EMPTY : GVX_MAS_INFEASIBLE;
            if (score) score[b] = NAN;
        }
        return;
    }
    float* Q = reinterpret_cast<float*>(mas_lds);   // [2][L]
    uint64_t* table = LDS ? reinterpret_cast<uint64_t*>(mas_lds + 2 * (size_t)L * sizeof(float)) : table_ws + (size_t)b * T * words;
    const float* row = a + (long)b * T * L;
    float* sc_row = SCORES ? scores + (long)b * T * L : nullptr;

    // a cell's weight is wanted if it is inside the row and reachable (with scores_out: every cell inside the row)
    // (addresses as a frame pointer every thread shares plus the thread's own 32-bit token index: no pointer pair per load)
    auto fetch = [&](int t, int l) -> float {
        const float* frame = row + (long)t * L;
        return (t < Tb && l < Lb && (SCORES || l <= t)) ? frame[(unsigned)l] : 0.f;
    };
    constexpr int MAS_DEPTH = LDS ? MAS_DEPTH_LDS : MAS_DEPTH_WS;
    float ahead[MAS_DEPTH][MAS_MAX_DEAL];
#pragma unroll
    for (int j = 0; j < MAS_DEPTH; ++j)
#pragma unroll
        for (int k = 0; k < MAS_MAX_DEAL; ++k) ahead[j][k] = k < deal ? fetch(j, tid + k * nthr) : 0.f;

    for (int t0 = 0; t0 < Tb; t0 += MAS_DEPTH) {
#pragma unroll
        for (int j = 0; j < MAS_DEPTH; ++j) {
            const int t = t0 + j;
            if (t >= Tb) break;   // the same for every thread of the workgroup
            float* cur = Q + (size_t)(t & 1) * L;
            const float* prev = Q + (size_t)((t + 1) & 1) * L;
            uint64_t* words_t = table + (size_t)t * words;
            float* sc_t = SCORES ? sc_row + (long)t * L : nullptr;
#pragma unroll
            for (int k = 0; k < MAS_MAX_DEAL; ++k) {
                const int l = tid + k * nthr;
                if (k >= deal || l - lane >= Lb) break;   // the same for every lane of the wave: the ballot below sees all 64
                const float w = ahead[j][k];
                ahead[j][k] = fetch(t + MAS_DEPTH, l);
                bool advance = false;
                if (l < Lb && (SCORES || l <= t)) {
                    const float s = logf(fmaxf(w, floor_));
                    if (SCORES) sc_t[(unsigned)l] = s;
                    if (l <= t) {
                        if (t > 0) {
                            const float stay = l < t ? prev[l] : -INFINITY;
                            const float up = l > 0 ? prev[l - 1] : -INFINITY;
                            advance = up > stay;   // a tie stays
                            cur[l] = s + (advance ? up : stay);
                        } else {
                            cur[l] = s;   // the one reachable cell of frame 0 is (0, 0)
                        }
                    }
                }
                const uint64_t word = __ballot(advance);
                if (lane == 0) words_t[(unsigned)__builtin_amdgcn_readfirstlane(l >> 6)] = word;
            }
            __syncthreads();
        }
    }
    if constexpr (!LDS) {
        __threadfence_block();
        __syncthreads();
    }

    int32_t* S = reinterpret_cast<int32_t*>(mas_lds);   // starts [L], over the Q rows
    if (tid < 64) {
        if (tid == 0) {
            const float total = Q[(size_t)((Tb - 1) & 1) * L + Lb - 1];   // read before S overwrites it
            if (score) score[b] = total;
            status[b] = GVX_MAS_OK;
            S[0] = 0;
        }
        int cur_l = Lb - 1;   // the path's token at frame t0: the same in every lane
        for (int t0 = Tb - 1; t0 >= 0; t0 -= 64) {
            const int t = t0 - lane;
            const int hi_word = cur_l >> 6, shift = (cur_l & 63) + 1;   // the window's bit 63 is token cur_l
            uint64_t hi = 0, lo = 0;
            if (t >= 0) {
                hi = table[(size_t)t * words + hi_word];
                if (hi_word > 0 && shift < 64) lo = table[(size_t)t * words + hi_word - 1];
            }
            const uint64_t window = shift == 64 ? hi : ((hi << (64 - shift)) | (lo >> shift));
            const int w_lo = (int)(uint32_t)window, w_hi = (int)(uint32_t)(window >> 32);
            uint64_t adv = 0;
            int pos = 63;
#pragma unroll
            for (int i = 0; i < 64; ++i) {   // frame t0 - i (a frame below 0 has an empty window: the path stays)
                const uint64_t wi = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(w_hi, i) << 32) | (uint32_t)__builtin_amdgcn_readlane(w_lo, i);
                const uint64_t bit = (wi >> pos) & 1;
                adv |= bit << i;
                pos -= (int)bit;
            }
            const int tok = max(0, cur_l - __popcll(adv & ((1ull << lane) - 1)));
            if (t >= 0) {
                if (path_b) path_b[t] = tok;
                if ((adv >> lane) & 1) S[tok] = t;   // the path came up to tok at frame t
            }
            cur_l = max(0, cur_l - __popcll(adv));
        }
    }
    __syncthreads();
    for (int l = tid; l < L; l += nthr) {
        const bool in = l < Lb;
        dur_b[l] = in ? (l + 1 < Lb ? S[l + 1] : Tb) - S[l] : 0;
        if (st_b) st_b[l] = in ? S[l] : -1;
    }
    if (path_b)
        for (int t = Tb + tid; t < T; t += nthr) path_b[t] = -1;
}

int mas_check_shape(int B, int T, int L) {
    if (B < 1 || T < 1 || L < 1) return fail(GVX_ERR_INVALID_ARG, "B, T and L must be >= 1");
    if (T > GVX_MAS_MAX_FRAMES || L > GVX_MAS_MAX_TOKENS)
        return fail(GVX_ERR_UNSUPPORTED, "T = %d / L = %d is beyond the alignment search's limits (%d frames, %d tokens)", T, L, GVX_MAS_MAX_FRAMES,
                    GVX_MAS_MAX_TOKENS);
    return GVX_OK;
}

template <bool LDS, bool SCORES>
int mas_launch(const MasPlan& p, const float* a, const int32_t* mel_lengths, const int32_t* token_lengths, int B, int T, int L, float floor_,
               void* workspace, int32_t* path, int32_t* durations, int32_t* starts, float* score, int32_t* status, float* scores, hipStream_t s) {
    if (p.lds_bytes > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mas_kernel<LDS, SCORES>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes));
    mas_kernel<LDS, SCORES><<<B, p.threads, p.lds_bytes, s>>>(a, mel_lengths, token_lengths, T, L, p.deal, p.words, floor_,
                                                             static_cast<uint64_t*>(workspace), path, durations, starts, score, status, scores);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

}  // namespace

extern "C" {

size_t gvx_monotonic_align_workspace_bytes(int B, int T, int L) {
    if (mas_check_shape(B, T, L) != GVX_OK) return 0;
    return mas_plan(B, T, L).ws_bytes;
}

int gvx_monotonic_align_uses_lds(int T, int L) {
    if (mas_check_shape(1, T, L) != GVX_OK) return -1;
    return mas_plan(1, T, L).lds ? 1 : 0;
}

int gvx_monotonic_align(const float* alignments, const int32_t* mel_lengths, const int32_t* token_lengths, int B, int T, int L, float floor,
                        int32_t* path_out, int32_t* durations_out, int32_t* starts_out, float* score_out, int32_t* row_status_out,
                        float* scores_out, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = mas_check_shape(B, T, L);
    if (rc != GVX_OK) return rc;
    if (!alignments || !durations_out || !row_status_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!(floor > 0.f && floor <= 1.f)) return fail(GVX_ERR_INVALID_ARG, "floor = %g is outside (0, 1]", (double)floor);
    const MasPlan p = mas_plan(B, T, L);
    if (p.ws_bytes) {
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255)) return fail(GVX_ERR_WORKSPACE, "workspace must be non-null and 256-byte aligned");
        if (workspace_bytes < p.ws_bytes) return fail(GVX_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", workspace_bytes, p.ws_bytes);
    }
    hipStream_t s = (hipStream_t)stream;
#define MAS_GO(LDS_, SC_) \
    mas_launch<LDS_, SC_>(p, alignments, mel_lengths, token_lengths, B, T, L, floor, workspace, path_out, durations_out, starts_out, score_out, \
                          row_status_out, scores_out, s)
    if (p.lds) return scores_out ? MAS_GO(true, true) : MAS_GO(true, false);
    return scores_out ? MAS_GO(false, true) : MAS_GO(false, false);
#undef MAS_GO
}

}  // C ABI
