// Sample-rate conversion and channel mix-down of ragged PCM batches on the GPU: the first stage of the reference's data path
// (format_audio2wav: mono mix-down and resampling to config.sampling_rate, there an ffmpeg process per file), and the way
// synthesised audio leaves at a rate other than the model's.  The resampler is a polyphase FIR over a caller-designed table
// (genvox_amd/resample.py designs this project's Kaiser-windowed sinc); the library only fixes the table's layout, stated in
// include/genvox_amd.h.
//
// Order of this file: kernels, the plan of a call (block shape, which table path), the C ABI.
#include "vocoder_internal.h"

#include <algorithm>

using namespace gvx::voc;

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_SAME_PHASE = 4;        // outputs m, m + S, m + 2S, m + 3S of a thread (S a multiple of up) share one tap row
constexpr int RS_TILE_SAMPLES = 6144;   // input samples a workgroup stages per output block: 24 KiB as float32, 48 KiB as float64
constexpr int RS_LDS_BYTES = 160 * 1024;
constexpr int RS_CHUNK = 4;             // taps a thread holds in registers at a time (taps_per_phase is a multiple of it)

// ---- kernels ------------------------------------------------------------------------------------------------

__device__ __forceinline__ float rs_fma(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double rs_fma(double a, double b, double c) { return fma(a, b, c); }

// four consecutive taps from a 16-byte aligned address (LDS: ds_read_b128, one for float32 and two for float64)
__device__ __forceinline__ void rs_load_taps(const float* p, float (&h)[RS_CHUNK]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    h[0] = v.x; h[1] = v.y; h[2] = v.z; h[3] = v.w;
}
__device__ __forceinline__ void rs_load_taps(const double* p, double (&h)[RS_CHUNK]) {
    const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
    h[0] = a.x; h[1] = a.y; h[2] = b.x; h[3] = b.y;
}

// Row stride of the table's LDS image in elements: the K taps padded so that the stride counts an ODD number of 16-byte slots.  The
// lanes of a wave sit on different phases p and read 16 bytes at p * stride + k; an even slot count would fold the 16 lanes that
// share an LDS cycle onto half (or fewer) of the 16 slots of a bank row whatever their phases are.
template <typename T>
__host__ __device__ constexpr int rs_row_stride(int K) {
    const int per = 16 / (int)sizeof(T);
    int slots = K / per;
    if ((slots & 1) == 0) ++slots;
    return slots * per;
}

__device__ __forceinline__ long rs_clamp(long v, long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// y[b][m] = sum_k table[p][k] * x[b][left_b + q - (K/2 - 1) + k],  q, p = divmod(m * down, up), x zero outside [left_b, right_b)
//
// The table ([up][K], tens of KB) is what a workgroup stages: once, into LDS, before it walks output blocks w = blockIdx.x,
// blockIdx.x + gridDim.x, ... of the (row, block) grid; a block's input span (block * down / up + K samples, at most RS_TILE_SAMPLES)
// is staged per block, converted to Out and zero-filled outside the row's bounds, so nothing behind a row's bounds reaches a sum.
// A block is R * S consecutive outputs, S = c * up: thread o takes outputs m0 + o + r * S, r < R.  They share the phase p (S * down
// is a multiple of up) and their inputs lie c * down apart, so a chunk of four taps is read once and used for R outputs.  Every
// output is one thread's sum in ascending tap order: it does not depend on the grid, the block shape aside, and the block shape is
// a function of (up, down, K) only - never of the batch.
// LDS_TABLE = false (the table does not fit beside the tile): the tap rows are read through the cache from global memory.
template <typename In, typename Out, bool LDS_TABLE>
__global__ __launch_bounds__(RS_THREADS) void resample_ragged_kernel(const In* __restrict__ pcm, long n_max, const int32_t* __restrict__ bounds,
                                                                     int B, int up, int down, const Out* __restrict__ table, int K, int S, int R,
                                                                     Out* __restrict__ out, long n_out_stride, int32_t* __restrict__ out_lengths,
                                                                     long blocks_per_row) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    Out* tile = reinterpret_cast<Out*>(rs_lds);    // [RS_TILE_SAMPLES]
    Out* tab_lds = tile + RS_TILE_SAMPLES;         // [up][stride]
    const int tid = threadIdx.x;
    const Out* tab = table;
    int ts = K;
    if constexpr (LDS_TABLE) {
        constexpr int per = 16 / (int)sizeof(Out);
        using V = std::conditional_t<sizeof(Out) == 4, float4, double2>;
        ts = rs_row_stride<Out>(K);
        const int per_row = K / per, chunks = up * per_row;
        for (int c = tid; c < chunks; c += RS_THREADS) {
            const int row = c / per_row, col = (c - row * per_row) * per;
            *reinterpret_cast<V*>(tab_lds + (long)row * ts + col) = *reinterpret_cast<const V*>(table + (long)row * K + col);
        }
        tab = tab_lds;   // made visible by the barrier in front of the first block's tile
    }
    const long block = (long)R * S, total = (long)B * blocks_per_row;
    const int koff = K / 2 - 1, step = (S / up) * down;
    for (long w = blockIdx.x; w < total; w += gridDim.x) {
        const int b = (int)(w / blocks_per_row);
        const long m0 = (w - (long)b * blocks_per_row) * block;
        const long left = rs_clamp(bounds[2 * b], n_max), right = rs_clamp(bounds[2 * b + 1], n_max);
        const long n = right > left ? right - left : 0;
        long n_out = (n * up + down - 1) / down;
        if (n_out > n_out_stride) n_out = n_out_stride;
        if (m0 == 0 && tid == 0) out_lengths[b] = (int32_t)n_out;
        Out* ob = out + (long)b * n_out_stride;
        const long m_end = m0 + block < n_out_stride ? m0 + block : n_out_stride;   // this block writes [m0, m_end)
        if (m0 >= n_out) {   // wholly behind the row's end (the whole workgroup takes this branch)
            for (long m = m0 + tid; m < m_end; m += RS_THREADS) ob[m] = (Out)0;
            continue;
        }
        const long m_last = (m0 + block < n_out ? m0 + block : n_out) - 1;
        const long q0 = (m0 * down) / up;
        const int span = (int)((m_last * down) / up - q0) + K;   // <= RS_TILE_SAMPLES by the plan
        const In* x = pcm + (long)b * n_max + left;
        __syncthreads();   // the previous block's sums have read the tile
        for (int i = tid; i < span; i += RS_THREADS) {
            const long j = q0 - koff + i;
            tile[i] = j >= 0 && j < n ? (Out)x[j] : (Out)0;
        }
        __syncthreads();
        for (int o = tid; o < S; o += RS_THREADS) {
            const long md = (m0 + o) * down, q = md / up;
            const int p = (int)(md - q * up);
            int xo[RS_SAME_PHASE];
            Out acc[RS_SAME_PHASE];
#pragma unroll
            for (int r = 0; r < RS_SAME_PHASE; ++r) {
                const bool live = r < R && m0 + o + (long)r * S <= m_last;
                xo[r] = live ? (int)(q - q0) + r * step : 0;   // a dead slot sums tile[0, K): never stored
                acc[r] = (Out)0;
            }
            const Out* trow = tab + (long)p * ts;
            for (int k = 0; k < K; k += RS_CHUNK) {
                Out h[RS_CHUNK];
                rs_load_taps(trow + k, h);
#pragma unroll
                for (int r = 0; r < RS_SAME_PHASE; ++r) {
                    const Out* xr = tile + xo[r] + k;
#pragma unroll
                    for (int i = 0; i < RS_CHUNK; ++i) acc[r] = rs_fma(xr[i], h[i], acc[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < RS_SAME_PHASE; ++r) {
                const long m = m0 + o + (long)r * S;
                if (r < R && m <= m_last) ob[m] = acc[r];
            }
        }
        for (long m = m_last + 1 + tid; m < m_end; m += RS_THREADS) ob[m] = (Out)0;
    }
}

// mono[i] = float32(sum_c double(frame i's channel c) / C), the sum in ascending channel order and rounded once; pcm is
// interleaved [frames][C].  VEC: C == 2 or C == 4 with an aligned batch - one load per frame.
template <typename In, int VEC>
__global__ void mixdown_kernel(const In* __restrict__ pcm, long frames, int C, float* __restrict__ mono) {
    struct alignas(sizeof(In) * (VEC ? VEC : 1)) Frame { In v[VEC ? VEC : 1]; };
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < frames; i += (long)gridDim.x * blockDim.x) {
        double s = 0.0;
        if constexpr (VEC != 0) {
            const Frame f = reinterpret_cast<const Frame*>(pcm)[i];
#pragma unroll
            for (int c = 0; c < VEC; ++c) s += (double)f.v[c];
        } else {
            const In* f = pcm + i * C;
            for (int c = 0; c < C; ++c) s += (double)f[c];
        }
        mono[i] = (float)(s / (double)C);
    }
}

// ---- the plan of a call --------------------------------------------------------------------------------------

inline size_t rs_sample_bytes(int pcm_kind) { return pcm_kind == GVX_PCM_INT16 ? 2 : (pcm_kind == GVX_PCM_FLOAT32 ? 4 : 8); }
inline bool rs_kind_ok(int pcm_kind) { return pcm_kind == GVX_PCM_INT16 || pcm_kind == GVX_PCM_FLOAT32 || pcm_kind == GVX_PCM_FLOAT64; }
inline bool rs_taps_ok(int K) { return K >= 4 && K <= GVX_RESAMPLE_MAX_TAPS && (K & 3) == 0; }

// Does the table's LDS image fit beside the input tile?  A function of (up, K, output type) alone.
template <typename Out>
bool rs_table_fits(int up, int K) {
    return ((size_t)up * rs_row_stride<Out>(K) + RS_TILE_SAMPLES) * sizeof(Out) <= (size_t)RS_LDS_BYTES;
}

struct RsShape { int S, R; };

// Block shape of (up, down, K): R same-phase outputs per thread, as many as a tile of one phase sweep allows; then S = c * up, c the
// largest that keeps a workgroup's 256 threads busy (c * up about 256) and the block's input span inside the tile.
inline RsShape rs_shape(int up, int down, int K) {
    auto span = [&](long outputs) { return ((outputs - 1) * down) / up + 1 + K; };
    int R = RS_SAME_PHASE;
    while (R > 1 && span((long)R * up) > RS_TILE_SAMPLES) R >>= 1;
    int c = std::max(1, (RS_THREADS + up - 1) / up);
    while (c > 1 && span((long)R * c * up) > RS_TILE_SAMPLES) --c;
    return RsShape{c * up, R};
}

template <typename In, typename Out>
int resample_launch(const In* pcm, int B, long n_max, const int32_t* bounds, int up, int down, const Out* table, int K, Out* out,
                    long n_out_stride, int32_t* out_lengths, hipStream_t s) {
    const RsShape sh = rs_shape(up, down, K);
    const long block = (long)sh.R * sh.S, blocks_per_row = (n_out_stride + block - 1) / block, total = (long)B * blocks_per_row;
    const bool lds = rs_table_fits<Out>(up, K);
    const size_t bytes = ((lds ? (size_t)up * rs_row_stride<Out>(K) : 0) + RS_TILE_SAMPLES) * sizeof(Out);
    int dev = 0, cus = 0;
    GL_HIP(hipGetDevice(&dev));
    GL_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    // a few workgroups per CU at most, each staging the table once: as many as its LDS image lets a CU hold, up to 4
    const long per_cu = std::min<long>(4, RS_LDS_BYTES / (long)bytes);
    const unsigned grid = (unsigned)std::max<long>(1, std::min<long>(total, per_cu * std::max(cus, 1)));
    auto kern = lds ? resample_ragged_kernel<In, Out, true> : resample_ragged_kernel<In, Out, false>;
    if (bytes > 64 * 1024) GL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    kern<<<grid, RS_THREADS, bytes, s>>>(pcm, n_max, bounds, B, up, down, table, K, sh.S, sh.R, out, n_out_stride, out_lengths, blocks_per_row);
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

template <typename In>
int mixdown_launch(const In* pcm, long frames, int C, float* mono, hipStream_t s) {
    const int grid = blocks_for(frames, 256, 4096);
    const bool aligned = (reinterpret_cast<uintptr_t>(pcm) % (sizeof(In) * (size_t)C)) == 0;
    if (C == 2 && aligned) mixdown_kernel<In, 2><<<grid, 256, 0, s>>>(pcm, frames, C, mono);
    else if (C == 4 && aligned) mixdown_kernel<In, 4><<<grid, 256, 0, s>>>(pcm, frames, C, mono);
    else mixdown_kernel<In, 0><<<grid, 256, 0, s>>>(pcm, frames, C, mono);
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

int rs_check_batch(const void* pcm, int pcm_kind, int B, long n_max) {
    if (!pcm) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!rs_kind_ok(pcm_kind)) return gl_fail(GVX_ERR_INVALID_ARG, "pcm_kind %d is none of int16 (0), float32 (1), float64 (2)", pcm_kind);
    if (B < 1 || n_max < 1 || n_max > 0x7fffffffL) return gl_fail(GVX_ERR_INVALID_ARG, "B and n_max must be >= 1 (n_max below 2^31)");
    if (reinterpret_cast<uintptr_t>(pcm) & (rs_sample_bytes(pcm_kind) - 1)) return gl_fail(GVX_ERR_INVALID_ARG, "pcm is not aligned to its sample type");
    return GVX_OK;
}

}  // namespace

extern "C" {

int gvx_resample_uses_lds_table(int up, int taps_per_phase, int pcm_kind) {
    if (up < 1 || up > GVX_RESAMPLE_MAX_UP || !rs_taps_ok(taps_per_phase) || !rs_kind_ok(pcm_kind)) return -1;
    return (pcm_kind == GVX_PCM_FLOAT64 ? rs_table_fits<double>(up, taps_per_phase) : rs_table_fits<float>(up, taps_per_phase)) ? 1 : 0;
}

int gvx_resample_block_shape(int up, int down, int taps_per_phase, int* S_out, int* R_out) {
    if (up < 1 || up > GVX_RESAMPLE_MAX_UP || down < 1 || down > GVX_RESAMPLE_MAX_DOWN || !rs_taps_ok(taps_per_phase) || !S_out || !R_out) return -1;
    const RsShape sh = rs_shape(up, down, taps_per_phase);
    *S_out = sh.S;
    *R_out = sh.R;
    return 0;
}

int gvx_wav_mixdown(const void* pcm, int pcm_kind, int B, long n_max, int channels, float* mono_out, void* stream) {
    const int rc = rs_check_batch(pcm, pcm_kind, B, n_max);
    if (rc != GVX_OK) return rc;
    if (!mono_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (channels < 2 || channels > 8) return gl_fail(GVX_ERR_INVALID_ARG, "channels = %d is outside [2, 8] (a mono batch needs no mix-down)", channels);
    hipStream_t s = (hipStream_t)stream;
    const long frames = (long)B * n_max;
    if (pcm_kind == GVX_PCM_INT16) return mixdown_launch(static_cast<const int16_t*>(pcm), frames, channels, mono_out, s);
    if (pcm_kind == GVX_PCM_FLOAT32) return mixdown_launch(static_cast<const float*>(pcm), frames, channels, mono_out, s);
    return mixdown_launch(static_cast<const double*>(pcm), frames, channels, mono_out, s);
}

int gvx_wav_resample_ragged(const void* pcm, int pcm_kind, int B, long n_max, const int32_t* bounds, int up, int down, const void* table,
                            int taps_per_phase, void* out, long n_out_stride, int32_t* out_lengths, void* stream) {
    const int rc = rs_check_batch(pcm, pcm_kind, B, n_max);
    if (rc != GVX_OK) return rc;
    if (!bounds || !table || !out || !out_lengths) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (up < 1 || down < 1) return gl_fail(GVX_ERR_INVALID_ARG, "up = %d and down = %d must be >= 1", up, down);
    if (up > GVX_RESAMPLE_MAX_UP || down > GVX_RESAMPLE_MAX_DOWN)
        return gl_fail(GVX_ERR_UNSUPPORTED, "up = %d / down = %d is beyond the resampler's limits (%d / %d)", up, down, GVX_RESAMPLE_MAX_UP, GVX_RESAMPLE_MAX_DOWN);
    if (!rs_taps_ok(taps_per_phase))
        return gl_fail(GVX_ERR_INVALID_ARG, "taps_per_phase = %d is no multiple of 4 in [4, %d]", taps_per_phase, GVX_RESAMPLE_MAX_TAPS);
    const size_t out_bytes = pcm_kind == GVX_PCM_FLOAT64 ? 8 : 4;
    if ((reinterpret_cast<uintptr_t>(table) & 15) || (reinterpret_cast<uintptr_t>(out) & (out_bytes - 1)))
        return gl_fail(GVX_ERR_INVALID_ARG, "table must be 16-byte aligned and out aligned to its sample type");
    const long need = (n_max * up + down - 1) / down;
    if (n_out_stride < need) return gl_fail(GVX_ERR_INVALID_ARG, "n_out_stride = %ld is below the %ld samples a row of n_max can become", n_out_stride, need);
    if (n_out_stride > 0x7fffffffL) return gl_fail(GVX_ERR_UNSUPPORTED, "n_out_stride = %ld does not fit the int32 row lengths", n_out_stride);
    hipStream_t s = (hipStream_t)stream;
    if (pcm_kind == GVX_PCM_INT16)
        return resample_launch(static_cast<const int16_t*>(pcm), B, n_max, bounds, up, down, static_cast<const float*>(table), taps_per_phase,
                               static_cast<float*>(out), n_out_stride, out_lengths, s);
    if (pcm_kind == GVX_PCM_FLOAT32)
        return resample_launch(static_cast<const float*>(pcm), B, n_max, bounds, up, down, static_cast<const float*>(table), taps_per_phase,
                               static_cast<float*>(out), n_out_stride, out_lengths, s);
    return resample_launch(static_cast<const double*>(pcm), B, n_max, bounds, up, down, static_cast<const double*>(table), taps_per_phase,
                           static_cast<double*>(out), n_out_stride, out_lengths, s);
}

}  // C ABI
