// Batched mel -> waveform vocoder on the GPU: dB->amplitude + pseudo-inverse mel projection, fast Griffin-Lim, overlap-add
// inverse STFT.  Replaces the mel->wav half of the reference's NumPy audio library, which is strictly per utterance with Python
// loops over frames (utils/audio/base.py:38-88, :143-169; core/processors.py:81-96).  Its clip / trim / normalise / Butterworth
// tail is wav_finalize.hip, the wav -> mel half is wav_to_mel.hip; what the three share is vocoder_internal.h.
//
// Layouts: the reference's spectrogram layout is [bins][frames]; internally everything is frame-major
// ([B*T][bins] complex, [B*T][n_fft] real) because that is what a batched 1-D FFT wants (one contiguous transform
// per frame).  The C ABI takes and returns the reference's layout and transposes once on the way in / out.
//
// A Griffin-Lim iteration takes one of four paths (gl_path picks one per call; all fp32 / complex64, all HBM-bound):
//   one launch, two frames per wave  the default for n_fft 1024 / hop 256, the reference's vocoder setting: FFTs in LDS (fft512_lds.h:
//                                    the transform, the even/odd split of the real transform and its inverse-side pack), only
//                                    the signal and the previous rebuilt spectrum cross iterations (gl_iteration_kernel<2>)
//   one launch, one frame per wave   the same kernel for sequences too short for the larger workgroup, or GVX_GL_ONE_FRAME=1
//   two launches                     GVX_GL_TWO_KERNELS=1: gl_inverse_ola_kernel + gl_forward_update_kernel (A/B runs, cross-checks)
//   rocFFT                           every other n_fft / hop, or GVX_GL_ROCFFT=1: C2R (rocFFT, batch B*T) -> overlap-add + window-sum
//                                    normalisation (gather form, frames added in ascending order like the reference) -> re-framing
//                                    * window -> R2C (rocFFT) -> momentum update / magnitude projection
// gvx_stft and gvx_istft are rocFFT at every size.  Below: kernels, what vocoder_internal.h declares, the calls' host side, the C ABI.
#include "fft512_lds.h"
#include "vocoder_internal.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <vector>

using namespace gvx::voc;

namespace {

// ---- kernels ------------------------------------------------------------------------------------------------

// amp_t[(b*T + t)][m] = inv_log(mel_db[b][m][t] + log(max(amin, ref)))     (utils/audio/base.py:38-52, power=False, scale=1)
__global__ void db_to_amp_transpose_kernel(const float* mel_db, float* amp_t, int M, int T, int log10_kind, float log_ref) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, m0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int r = ty; r < 32; r += 8) {
        const int m = m0 + r, t = t0 + tx;
        float v = 0.f;
        if (m < M && t < T) {
            const float db = mel_db[((long)b * M + m) * T + t] + log_ref;
            v = log10_kind ? powf(10.f, db) : expf(db);
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, m = m0 + tx;
        if (m < M && t < T) amp_t[((long)b * T + t) * M + m] = tile[tx][r];
    }
}

// generic [B][ni][nj] -> [B][nj][ni] for float (scale 1) or float2 elements
template <typename E>
__global__ void transpose_kernel(const E* src, E* dst, int ni, int nj) {
    __shared__ E tile[32][33];
    const int b = blockIdx.z, i0 = blockIdx.y * 32, j0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    for (int r = ty; r < 32; r += 8) {
        const int i = i0 + r, j = j0 + tx;
        if (i < ni && j < nj) tile[r][tx] = src[((long)b * ni + i) * nj + j];
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int j = j0 + r, i = i0 + tx;
        if (i < ni && j < nj) dst[((long)b * nj + j) * ni + i] = tile[tx][r];
    }
}

template <typename E>
hipError_t launch_transpose(const E* src, E* dst, int B, int ni, int nj, hipStream_t s) {
    dim3 grid((nj + 31) / 32, (ni + 31) / 32, B);
    transpose_kernel<E><<<grid, dim3(32, 8), 0, s>>>(src, dst, ni, nj);
    return hipGetLastError();
}

// window sum of squares along the signal (utils/audio/base.py:81-84), frames added in ascending order, float32
__global__ void wss_kernel(const float* win, float* wss, int n_fft, int hop, int T, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long t_lo = (i - n_fft + hop) / hop;  // ceil((i - n_fft + 1) / hop) for i - n_fft + 1 > 0
    if (i - n_fft + 1 <= 0) t_lo = 0;
    long t_hi = i / hop;
    if (t_hi > T - 1) t_hi = T - 1;
    float s = 0.f;
    for (long t = t_lo; t <= t_hi; ++t) {
        const float w = win[i - t * hop];
        s += w * w;
    }
    wss[i] = s;
}

// The window sum of squares of a row of T_b frames equals the padded table wss[i] for i < T_b*hop (there only the clip at frame
// 0 matters); its last n_fft - hop samples, where the frames t >= T_b of the padded table are missing, come from this per-row
// table: tail[b][q] = wss of sample T_b*hop + q at T = T_b, frames added in ascending order exactly as wss_kernel adds them
// (rows shorter than the overlap, whose head and tail meet, included: the clip at frame 0 is the same expression).
__global__ void wss_tail_kernel(const float* win, const int32_t* lens, float* tail, int n_fft, int hop, int T) {
    const int b = blockIdx.y;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_fft - hop) return;
    const int Tb = row_frames(lens, b, T);
    const long i = (long)Tb * hop + q;
    long t_lo = (i - n_fft + hop) / hop;
    if (i - n_fft + 1 <= 0) t_lo = 0;
    float s = 0.f;
    for (long t = t_lo; t <= Tb - 1; ++t) {
        const float w = win[i - t * hop];
        s += w * w;
    }
    tail[(long)b * (n_fft - hop) + q] = s;
}

// angles = (mag, 0)   (utils/audio/base.py:151-154)
__global__ void gl_init_kernel(const float* mag, float2* ang, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) ang[i] = make_float2(mag[i], 0.f);
}

// y[b][i] = (sum_t win[i - t*hop] * fr[b][t][i - t*hop] / n_fft) / wss[i]      (utils/audio/base.py:71-88)
// RAGGED: frames t >= T_b are skipped, samples i >= n_b are left unwritten, the divisor of the last n_fft - hop samples is the row's
template <bool RAGGED>
__global__ void gl_ola_kernel(const float* fr, const float* win, const float* wss, float* y, int n_fft, int hop, int T, long n,
                              const int32_t* lens, const float* wss_tail) {
    const int b = blockIdx.y;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int Tb = T;
    if (RAGGED) {
        Tb = row_frames(lens, b, T);
        if (Tb == 0 || i >= (long)n_fft + (long)(Tb - 1) * hop) return;
    }
    long t_lo = (i - n_fft + hop) / hop;
    if (i - n_fft + 1 <= 0) t_lo = 0;
    long t_hi = i / hop;
    if (t_hi > Tb - 1) t_hi = Tb - 1;
    const float inv_n = 1.f / (float)n_fft;
    const float* frb = fr + (long)b * T * n_fft;
    float s = 0.f;
    for (long t = t_lo; t <= t_hi; ++t) {
        const long k = i - t * hop;
        s += win[k] * (frb[t * n_fft + k] * inv_n);
    }
    const float w = (RAGGED && i >= (long)Tb * hop) ? wss_tail[(long)b * (n_fft - hop) + (i - (long)Tb * hop)] : wss[i];
    y[(long)b * n + i] = w > 1.17549435e-38f ? s / w : s;
}

// angles = rebuilt - c*prev; angles /= |angles| + tiny; angles *= mag      (utils/audio/base.py:158-160)
__global__ void gl_update_kernel(const float2* reb, const float2* prev, const float* mag, float2* ang, float c, int first, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float2 r = reb[i];
        float2 a = r;
        if (!first) {
            const float2 p = prev[i];
            a.x = r.x - c * p.x;
            a.y = r.y - c * p.y;
        }
        const float d = hypotf(a.x, a.y) + 1.17549435e-38f;
        const float m = mag[i];
        ang[i] = make_float2(a.x / d * m, a.y / d * m);
    }
}

// phase = angle(angles); spec = mag * (cos phase + i sin phase)     (base.py:162, :54-56; core/processors.py:89-90)
// RAGGED: one grid row per utterance, n = T * bins elements each (frame-major, so a row's valid frames are a prefix);
// phase and final spectrum of frames t >= T_b are 0
template <bool RAGGED>
__global__ void gl_final_kernel(const float2* ang, const float* mag, float2* spec, float* phase_t, long n, int bins, int T,
                                const int32_t* lens) {
    long n_valid = n;
    if (RAGGED) {
        const long off = (long)blockIdx.y * n;
        ang += off; mag += off;
        if (spec) spec += off;
        if (phase_t) phase_t += off;
        n_valid = (long)row_frames(lens, blockIdx.y, T) * bins;
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        if (RAGGED && i >= n_valid) {
            if (phase_t) phase_t[i] = 0.f;
            if (spec) spec[i] = make_float2(0.f, 0.f);
            continue;
        }
        const float2 a = ang[i];
        const float ph = atan2f(a.y, a.x);
        const float m = mag[i];
        if (phase_t) phase_t[i] = ph;
        if (spec) spec[i] = make_float2(m * cosf(ph), m * sinf(ph));
    }
}

// ragged result rows: dst[b][i] = src[b][i] for i < n_b, 0 behind (src is not valid there)
__global__ void copy_rows_ragged_kernel(const float* src, float* dst, long n, int n_fft, int hop, const int32_t* lens) {
    const int b = blockIdx.y;
    const long nb = row_samples(lens, b, n_fft, hop, n);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dst[(long)b * n + i] = i < nb ? src[(long)b * n + i] : 0.f;
}

// =====================================================================================================
// Fused Griffin-Lim iteration for n_fft = 1024, hop = 256 (the reference's vocoder setting).
// The rocFFT pipeline moves each frame through HBM seven times per iteration (c2r pre/post kernels, raw frames, overlap-add,
// re-framing, r2c, update: 8.6 GB per iteration at 256 x 800 frames).  Here an iteration is two kernels:
//   gl_inverse_ola_kernel   spectrum -> 512-point complex inverse FFT per frame in LDS (one wave per frame, 16 frames per
//                           workgroup) -> window -> overlap-add of the workgroup's 13 hop blocks -> y        (reads S, writes y)
//   gl_forward_update_kernel  y -> window -> FFT -> rebuilt spectrum -> momentum update -> new S and tprev in place
//                                                                     (reads y, tprev, mag; writes S, tprev)
// = 3.9 GB per iteration, the minimum for an iteration that keeps S and tprev in HBM.
// FFT: a 1024-point real transform as a 512-point complex Stockham radix-8 (3 passes, 8 points per lane, exchange through
// LDS) plus the even/odd split; unnormalised inverse like rocFFT's c2r, so the 1/n_fft of istft stays where it was.
// Summation order of the overlap-add (ascending frame index) and every elementwise formula are those of the unfused
// kernels above; only the FFT's internal rounding differs (fp32, table twiddles computed in double).
// =====================================================================================================

constexpr int GLI_FRAMES = 16;                 // frames (waves) per workgroup of the inverse kernel
constexpr int GLI_BLOCKS = GLI_FRAMES - 3;     // hop blocks it completes (n_fft / hop - 1 = 3 halo frames)
constexpr int GLI_TAB_WIN = FN + 520;          // LDS tables of gl_iteration_kernel, in float2: twiddles [FN + 513], pad, window [512]
constexpr int GLI_TAB = GLI_TAB_WIN + 512;

// ---- the steps of a frame that the kernels below share.  Lane j of the frame's wave holds samples 2 (j + 64 r), 2 (j + 64 r) + 1
// in v[r] (the complex points j + 64 r of fft512_wave) and owns bins j + 64 r and, on lane 0, bin 512.
// (The prefetch of the update's operands is not among them: gl_forward_update_kernel loads its twiddles in the same loop, and with
// the loop shared it needs 98 VGPRs instead of 96, a wave less per SIMD.)

// v = win * frame at yb
__device__ __forceinline__ void load_windowed_frame(float2 v[8], const float* __restrict__ yb, const float* __restrict__ win, int j) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n2 = 2 * (j + 64 * r);
        const float2 x = *reinterpret_cast<const float2*>(yb + n2);
        const float2 w = *reinterpret_cast<const float2*>(win + n2);
        v[r] = make_float2(w.x * x.x, w.y * x.y);
    }
}

// the inverse transform's v, windowed, into the frame's LDS row of 1024 floats
// (same operation order as gl_ola_kernel: win[k] * (fr[k] * (1/n_fft)))
__device__ __forceinline__ void store_windowed_frame(float* frow, const float2 v[8], const float* __restrict__ win, int j) {
    const float inv_n = 1.f / 1024.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int n2 = 2 * (j + 64 * r);
        const float2 w = *reinterpret_cast<const float2*>(win + n2);
        *reinterpret_cast<float2*>(frow + n2) = make_float2(w.x * (v[r].x * inv_n), w.y * (v[r].y * inv_n));
    }
}

// Overlap-add of the workgroup's hop blocks h0 .. h0+NBL-1 from its NBL + 3 windowed frame rows in LDS (`rows`; frame h0-3 is row
// 0), frames added in ascending order, divided by the window sum of squares (v_rcp_f32: 1 ulp).  Called by every thread, behind
// the barrier that ends the rows' writes.  RAGGED: frames t >= Tb do not exist, the row ends at (Tb+3)*256, its last three hop
// blocks are divided by the row's own wss_tail [B][768]
template <int NBL, bool RAGGED>
__device__ __forceinline__ void overlap_add_blocks(const float* rows, const float* __restrict__ wss, const float* __restrict__ wss_tail,
                                                   float* __restrict__ y, int b, int h0, int T, int Tb, int tid) {
    const long n = (long)(T + 3) * 256;
    const long n_row = RAGGED ? (long)(Tb + 3) * 256 : n;
    for (int idx = tid; idx < NBL * 256; idx += GLI_FRAMES * 64) {
        const int hb = idx >> 8, q = idx & 255;
        const int h = h0 + hb;
        const long i = (long)h * 256 + q;
        if (i >= n_row) break;
        float sacc = 0.f;
#pragma unroll
        for (int d = 3; d >= 0; --d) {           // frames t = h-3 .. h  ->  rows hb .. hb+3
            const int tt = h - d;
            if (tt >= 0 && tt < Tb) sacc += rows[(long)(hb + 3 - d) * (FPAD * 2) + d * 256 + q];
        }
        const float w = (RAGGED && h >= Tb) ? wss_tail[(long)b * 768 + (h - Tb) * 256 + q] : wss[i];
        y[(long)b * n + i] = w > 1.17549435e-38f ? sacc * __builtin_amdgcn_rcpf(w) : sacc;
    }
}

// S [B*T][513] (frame-major) -> y [B][(T+3)*256]: y[i] = (sum_t win[k] * (irfft(S_t)[k] / 1024)) / wss[i], k = i - 256 t
// RAGGED: only the frames t < T_b of row b exist; its samples i < (T_b+3)*256 are written (the last three hop blocks divided by the
// row's own wss_tail [B][768]), the rest of the padded row is left as it was; a workgroup behind the row's end leaves at once
template <bool RAGGED>
__global__ __launch_bounds__(GLI_FRAMES * 64) void gl_inverse_ola_kernel(const float2* __restrict__ spec, const float* __restrict__ win,
                                                                         const float* __restrict__ wss, const float2* __restrict__ tw,
                                                                         float* __restrict__ y, int T, const int32_t* __restrict__ lens,
                                                                         const float* __restrict__ wss_tail) {
    extern __shared__ __attribute__((aligned(16))) float2 fsm[];   // [GLI_FRAMES][FPAD] float2; reused as [GLI_FRAMES][1024] float
    const int b = blockIdx.y, h0 = blockIdx.x * GLI_BLOCKS;
    int Tb = T;
    if (RAGGED) {
        Tb = row_frames(lens, b, T);
        if (Tb == 0 || h0 >= Tb + 3) return;   // uniform over the workgroup, before any barrier
    }
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t = h0 - 3 + wave;
    const bool valid = t >= 0 && t < Tb;      // wave-uniform; every wave still joins the barriers
    float2* buf = fsm + wave * FPAD;
    float2 v[8];
    if (valid) {
        const float2* S = spec + ((long)b * T + t) * 513;
        const float2* tw2 = tw + FN;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k = j + 64 * r;
            v[r] = irfft_pack(S[k], S[512 - k], tw2[k], k == 0);
        }
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = make_float2(0.f, 0.f);
    }
    fft512_wave<true>(v, buf, tw, j, false);
    // the windowed frame goes into this wave's LDS row: 1024 floats inside the wave's FPAD*2 floats; all exchanges above are done
    __syncthreads();
    if (valid) store_windowed_frame(reinterpret_cast<float*>(buf), v, win, j);
    __syncthreads();
    overlap_add_blocks<GLI_BLOCKS, RAGGED>(reinterpret_cast<const float*>(fsm), wss, wss_tail, y, b, h0, T, Tb, tid);
}

// One whole Griffin-Lim iteration per launch (n_fft 1024 / hop 256):
//   y_in (the signal of the current angles) -> frames -> FFT -> rebuilt -> momentum update -> new spectrum S
//   -> inverse FFT of S -> window -> overlap-add -> y_out (the signal of the new angles)
// so the state that crosses iterations is the signal (1 KB per frame) and tprev (4 KB per frame); the spectrum itself never
// goes to HBM except in the last iteration.  Per frame and iteration this moves 1 216 B (y_in incl. the 3-frame halo) +
// 4 104 (tprev in) + 2 052 (mag) + 4 104 (tprev out) + 1 024 (y_out) = 12.5 KB (x 16/13 for the reads of halo frames: 14.1 KB)
// against 21.5 KB of the forward / inverse kernel pair above (S written, then read x 1.23) and 20 516 B of SURVEY 8d's
// "minimal" count, which assumed the spectrum has to make the round trip.
// Workgroup = 16 waves x FPW frames each = the 16 FPW - 3 hop blocks they complete + 3 halo frames; frames h0 .. are OWNED by
// the workgroup (it writes their tprev / spectrum), the halo frames h0-3 .. h0-1 are recomputed from y_in and tprev_in, which
// is why both are double buffered (a neighbour may still be reading what this workgroup would overwrite).  FPW = 2 (32 frames,
// 29 blocks, 144 KB of rows + 12 KB of tables in LDS) recomputes 10 % of the frames instead of 23 %.
// RAGGED: as in gl_inverse_ola_kernel - frames t >= T_b are neither transformed nor added, samples of y_out past (T_b+3)*256 stay
// unwritten (no valid frame reads them), and a workgroup whose hop blocks all lie behind the row's end returns before it loads the
// tables, so the padding of a batch with spread lengths costs a launch slot and nothing else.
template <int FPW, bool RAGGED>   // frames per wave: a workgroup covers 16 FPW frames = 16 FPW - 3 hop blocks (halo share 3/16 or 3/32)
__global__ __launch_bounds__(GLI_FRAMES * 64) void gl_iteration_kernel(const float* __restrict__ y_in, float* __restrict__ y_out,
                                                                       const float* __restrict__ win_g, const float* __restrict__ wss,
                                                                       const float2* __restrict__ tw_g, const float* __restrict__ mag,
                                                                       const float2* __restrict__ tprev_in, float2* __restrict__ tprev_out,
                                                                       float2* __restrict__ spec_out, float c, int first, int do_inverse,
                                                                       int T, const int32_t* __restrict__ lens,
                                                                       const float* __restrict__ wss_tail) {
    constexpr int NFR = GLI_FRAMES * FPW, NBL = NFR - 3;
    extern __shared__ __attribute__((aligned(16))) float2 fsm[];   // [NFR][FPAD] float2; reused as [NFR][1024+] float; then the tables
    const int b = blockIdx.y, h0 = blockIdx.x * NBL;
    int Tb = T;
    if (RAGGED) {
        Tb = row_frames(lens, b, T);
        if (Tb == 0 || h0 >= Tb + 3) return;   // uniform over the workgroup, before the tables and any barrier
    }
    const int tid = threadIdx.x, jj = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // twiddle and window tables live in LDS behind the frame rows: a table read from global memory costs the wave a
    // round trip through L1 at every FFT pass (60 % of the wave cycles were s_waitcnt before this)
    float2* tab = fsm + NFR * FPAD;
    for (int i = tid; i < GLI_TAB; i += GLI_FRAMES * 64)
        tab[i] = i < FN ? tw_g[FN + 513 + i]      // per-pass twiddles
                        : (i < FN + 513 ? tw_g[i] : (i < GLI_TAB_WIN ? make_float2(0.f, 0.f) : reinterpret_cast<const float2*>(win_g)[i - GLI_TAB_WIN]));
    __syncthreads();
    const float2* tw_ = tab;
    const float* win_ = reinterpret_cast<const float*>(tab + GLI_TAB_WIN);
#pragma unroll 1
    for (int f = 0; f < FPW; ++f) {
        const int slot = wave + GLI_FRAMES * f;   // the wave's frames are 16 apart so that all waves stay busy in the last group
        const int t = h0 - 3 + slot;
        if (t < 0 || t >= Tb) continue;           // wave-uniform; the barrier below is outside the loop
        const bool owner = slot >= 3;             // frames h0 .. h0+NBL-1
        float2* buf = fsm + slot * FPAD;
        float2 v[8];
        // the tables are frame independent: without this the compiler hoists their loads out of the frame loop and spills
        const float* win = win_;
        const float2 *tw = tw_, *tw2 = tw_ + FN;
        int j = jj;
        if (FPW > 1) asm volatile("" : "+v"(j));
        // ---- forward: frame of y_in, windowed
        load_windowed_frame(v, y_in + (long)b * ((long)(T + 3) * 256) + (long)t * 256, win, j);
        // the update's operands do not depend on the FFT: fetch them now so their latency hides under it.  (Measured the other
        // way round as well: loading them after the FFT and capping the kernel at 64 VGPRs puts two workgroups on a CU, but the
        // kernel is bound by instruction issue and LDS traffic, not by latency - 81 ms instead of 72 ms for 60 iterations.)
        const long base = ((long)b * T + t) * 513;
        float2 pv[9];
        float mg[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int k = r < 8 ? j + 64 * r : 512;
            const bool mine = r < 8 || j == 0;
            pv[r] = (mine && !first) ? tprev_in[base + k] : make_float2(0.f, 0.f);
            mg[r] = mine ? mag[base + k] : 0.f;
        }
        fft512_wave<false, true>(v, buf, tw, j, true);
        wave_lds_fence();        // ---- rebuilt spectrum, momentum update, projection onto the magnitudes: bins k = j + 64 r and, on lane 0, k = 512
        float2 S[9];
        // row addresses: bin k = j + 64 r sits at fpad(j) + 72 r and its mirror 512 - k at fpad(512 - j) - 72 r (both linear in r,
        // so they fold into the LDS instructions' offsets); only k = 0 (lane 0, r = 0) mirrors onto itself
        const int a_fwd = fpad(j), a_rev = fpad(512 - j);
        auto update_bin = [&](const int r, float2 pvk, float mgk) -> float2 {   // r is a constant after unrolling
            const int k = r < 8 ? j + 64 * r : 512;
            const bool edge = r == 8 || (r == 0 && j == 0);       // DC / Nyquist
            const float2 zk = buf[r < 8 ? a_fwd + 72 * r : 0];
            const float2 zc = buf[r == 8 ? 0 : (r == 0 && j == 0 ? 0 : a_rev - 72 * r)];
            const float2 reb = rfft_split(zk, zc, tw2[k], edge);
            float2 a = reb;
            if (!first) {
                a.x = reb.x - c * pvk.x;
                a.y = reb.y - c * pvk.y;
            }
            // a / (|a| + tiny) * mag with v_sqrt_f32 / v_rcp_f32; the operands are pre-scaled on the rare path where their
            // squares would underflow (|a| < 1e-15), like the hypot behind the reference's abs().  This is (a * rcp) * mag;
            // gl_forward_update_kernel computes a * (rcp * mag), which rounds differently and can form 0 * inf for a == 0 under a
            // large mag.  The two are kept apart on purpose: making one into the other changes what a path computes
            float dd = __builtin_amdgcn_sqrtf(a.x * a.x + a.y * a.y);
            if (fmaxf(fabsf(a.x), fabsf(a.y)) < 1e-15f) {
                const float ax = a.x * 1.8446744e19f, ay = a.y * 1.8446744e19f;   // 2^64
                dd = __builtin_amdgcn_sqrtf(ax * ax + ay * ay) * 5.4210109e-20f;  // 2^-64
            }
            const float q = __builtin_amdgcn_rcpf(dd + 1.17549435e-38f);
            const float2 Sk = make_float2(a.x * q * mgk, a.y * q * mgk);   // unit vector first: 0 * (mag / tiny) would be NaN
            if (owner) {
                tprev_out[base + k] = reb;
                if (spec_out) spec_out[base + k] = Sk;
            }
            return Sk;
        };
#pragma unroll
        for (int r = 0; r < 8; ++r) S[r] = update_bin(r, pv[r], mg[r]);
        S[8] = make_float2(0.f, 0.f);
        if (j == 0) S[8] = update_bin(8, pv[8], mg[8]);
        if (!do_inverse) continue;   // uniform: the last iteration only needs the spectrum
        // ---- inverse: S[k] and S[512-k] meet through this wave's LDS row (all reads of Z above are done)
        wave_lds_fence();
#pragma unroll
        for (int r = 0; r < 8; ++r) buf[a_fwd + 72 * r] = S[r];
        wave_lds_fence();
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const bool dc = r == 0 && j == 0;
            v[r] = irfft_pack(S[r], dc ? S[8] : buf[a_rev - 72 * r], tw2[j + 64 * r], dc);   // lane 0 holds the Nyquist bin itself
        }
        wave_lds_fence();
        fft512_wave<true, true>(v, buf, tw, j, false);
        // the windowed frame goes into this frame's LDS row, which only this wave touches until the barrier (the FFT's last
        // exchange ended with a fence)
        store_windowed_frame(reinterpret_cast<float*>(buf), v, win, j);
    }
    if (!do_inverse) return;
    __syncthreads();
    overlap_add_blocks<NBL, RAGGED>(reinterpret_cast<const float*>(fsm), wss, wss_tail, y_out, b, h0, T, Tb, tid);
}


// y -> rebuilt = rfft(win * frame); ang' = rebuilt - c*tprev; S = mag * ang' / (|ang'| + tiny); tprev = rebuilt  (in place)
__global__ __launch_bounds__(GLF_FRAMES * 64) void gl_forward_update_kernel(const float* __restrict__ y, const float* __restrict__ win,
                                                                            const float2* __restrict__ tw, const float* __restrict__ mag,
                                                                            float2* __restrict__ tprev, float2* __restrict__ spec,
                                                                            float c, int first, int T, long frames) {
    __shared__ __attribute__((aligned(16))) float2 fsm[GLF_FRAMES * FPAD];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long f = (long)blockIdx.x * GLF_FRAMES + wave;
    const bool valid = f < frames;
    float2* buf = fsm + wave * FPAD;
    float2 v[8];
    if (valid) {
        const unsigned fu = (unsigned)f;   // frames < 2^32 (checked on the host): 32-bit division, the 64-bit one is ~150 instructions
        const int b = (int)(fu / (unsigned)T), t = (int)(fu - (unsigned)b * (unsigned)T);
        load_windowed_frame(v, y + (long)b * (long)(T + 3) * 256 + (long)t * 256, win, j);
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = make_float2(0.f, 0.f);
    }
    // the update's operands do not depend on the FFT: fetch them now so their latency hides under it
    const float2* tw2 = tw + FN;
    const long base = f * 513;
    float2 pv[9], wk[9];
    float mg[9];
    if (valid) {
#pragma unroll
        for (int r = 0; r < 9; ++r) {
            const int k = r < 8 ? j + 64 * r : 512;
            const bool mine = r < 8 || j == 0;
            pv[r] = (mine && !first) ? tprev[base + k] : make_float2(0.f, 0.f);
            mg[r] = mine ? mag[base + k] : 0.f;
            wk[r] = tw2[k];
        }
    }
    fft512_wave<false>(v, buf, tw, j, true);
    wave_lds_fence();
    if (!valid) return;
    // bins k = j + 64 r (r = 0..7) and, on lane 0, k = 512
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const int k = r < 8 ? j + 64 * r : 512;
        if (r == 8 && j != 0) break;
        const float2 reb = rfft_split(buf[fpad(k & (FN - 1))], buf[fpad((512 - k) & (FN - 1))], wk[r], k == 0 || k == 512);
        float2 a = reb;
        if (!first) {
            a.x = reb.x - c * pv[r].x;
            a.y = reb.y - c * pv[r].y;
        }
        // a / (|a| + tiny) * mag with v_sqrt_f32 / v_rcp_f32 (1 ulp each) instead of libm hypotf and two IEEE divisions,
        // which together were half of this kernel's vector instructions.  Operands are pre-scaled by a power of two when
        // they are so small that their squares would underflow (hypotf's only advantage here), so tiny bins keep their phase.
        // This is a * (rcp * mag); gl_iteration_kernel computes (a * rcp) * mag, the unit vector first, which rounds differently
        // and never forms 0 * inf.  The two are kept apart on purpose: making one into the other changes what a path computes
        const float big = fmaxf(fabsf(a.x), fabsf(a.y));
        const float sc = big < 1e-15f ? 1.8446744e19f : 1.f;         // 2^64 (exact)
        const float isc = big < 1e-15f ? 5.4210109e-20f : 1.f;       // 2^-64
        const float ax = a.x * sc, ay = a.y * sc;
        const float d = __builtin_amdgcn_sqrtf(ax * ax + ay * ay) * isc + 1.17549435e-38f;
        const float q = __builtin_amdgcn_rcpf(d) * mg[r];
        spec[base + k] = make_float2(a.x * q, a.y * q);
        tprev[base + k] = reb;
    }
}

}  // namespace

// ---- what vocoder_internal.h declares ------------------------------------------------------------------------
namespace gvx { namespace voc {

int gl_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return gvx::set_error(code, buf);
}

int get_plans(gvx_gl_plan* p, long batch, FftPair** out) {
    auto it = p->plans.find(batch);
    if (it != p->plans.end()) { *out = &it->second; return GVX_OK; }
    FftPair fp;
    const size_t len[1] = {(size_t)p->n_fft};
    const size_t one[1] = {1};
    const size_t off[1] = {0};
    rocfft_plan_description d1 = nullptr, d2 = nullptr;
    GL_FFT(rocfft_plan_description_create(&d1));
    GL_FFT(rocfft_plan_description_set_data_layout(d1, rocfft_array_type_real, rocfft_array_type_hermitian_interleaved, off, off,
                                                   1, one, (size_t)p->n_fft, 1, one, (size_t)p->bins));
    GL_FFT(rocfft_plan_create(&fp.r2c, rocfft_placement_notinplace, rocfft_transform_type_real_forward, rocfft_precision_single, 1,
                              len, (size_t)batch, d1));
    GL_FFT(rocfft_plan_description_create(&d2));
    GL_FFT(rocfft_plan_description_set_data_layout(d2, rocfft_array_type_hermitian_interleaved, rocfft_array_type_real, off, off,
                                                   1, one, (size_t)p->bins, 1, one, (size_t)p->n_fft));
    GL_FFT(rocfft_plan_create(&fp.c2r, rocfft_placement_notinplace, rocfft_transform_type_real_inverse, rocfft_precision_single, 1,
                              len, (size_t)batch, d2));
    rocfft_plan_description_destroy(d1);
    rocfft_plan_description_destroy(d2);
    size_t w1 = 0, w2 = 0;
    GL_FFT(rocfft_plan_get_work_buffer_size(fp.r2c, &w1));
    GL_FFT(rocfft_plan_get_work_buffer_size(fp.c2r, &w2));
    fp.work_bytes = w1 > w2 ? w1 : w2;
    auto ins = p->plans.emplace(batch, fp);
    *out = &ins.first->second;
    return GVX_OK;
}

int run_fft(gvx_gl_plan* p, rocfft_plan plan, void* in, void* out, void* work, size_t work_bytes, hipStream_t s) {
    if (!p->info) GL_FFT(rocfft_execution_info_create(&p->info));
    if (work_bytes) GL_FFT(rocfft_execution_info_set_work_buffer(p->info, work, work_bytes));
    GL_FFT(rocfft_execution_info_set_stream(p->info, s));
    void* ib[1] = {in};
    void* ob[1] = {out};
    GL_FFT(rocfft_execute(plan, ib, ob, p->info));
    return GVX_OK;
}

GlPath gl_path(const gvx_gl_plan* p, const int32_t* lens, int n_iter, int T) {
    if (p->tw == nullptr || getenv_flag("GVX_GL_ROCFFT")) return GlPath::rocfft;
    // a ragged call always takes the one-launch iteration: the two-launch A/B variant walks all B*T frames.  (No iteration at all
    // is the two-launch path as well: its loop is empty, the one-launch path would start with an inverse nobody reads.)
    if (n_iter <= 0 || (!lens && getenv_flag("GVX_GL_TWO_KERNELS"))) return GlPath::two_launch;
    // two frames per wave (29 hop blocks per workgroup, 147 KB of LDS) unless the sequence is short
    return T + 3 > GLI_BLOCKS && !getenv_flag("GVX_GL_ONE_FRAME") ? GlPath::one_launch_two_frames : GlPath::one_launch_one_frame;
}

// basis: the mel basis of the wav -> mel calls in rows padded for the GEMM (its size does not depend on the frame count, so it
// has a region of its own: no call with M mels is too short for it).  What a WsKind adds lies behind everything else (the uniform
// layout is a prefix of both)
int gl_layout(gvx_gl_plan* p, int B, int T, int M, WsKind kind, bool plans_when_fused, GlCall* c) {
    c->fp = nullptr;
    if (plans_when_fused || !gl_fused(p)) {
        const int rc = get_plans(p, (long)B * T, &c->fp);
        if (rc != GVX_OK) return rc;
    }
    GlWs& w = c->w;
    w = GlWs{};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t frames = (size_t)B * T;
    const size_t n = (size_t)p->n_fft + (size_t)(T - 1) * p->hop;
    w.mag = take(frames * p->bins * sizeof(float));
    w.ang = take(frames * p->bins * sizeof(float2));
    w.reb0 = take(frames * p->bins * sizeof(float2));
    w.reb1 = take(frames * p->bins * sizeof(float2));
    w.fr = take(frames * p->n_fft * sizeof(float));
    w.y = take((size_t)B * n * sizeof(float));
    w.wss = take(n * sizeof(float));
    w.amp = take(frames * (size_t)(M > 0 ? M : 1) * sizeof(float));
    w.fft_work = take(c->fp ? c->fp->work_bytes : 0);
    w.basis = take((size_t)(M > 0 ? M : 0) * (size_t)((p->bins + 3) & ~3) * sizeof(float));
    if (kind == WsKind::ragged_gl) w.wss_tail = take((size_t)B * (p->n_fft - p->hop) * sizeof(float));
    if (kind == WsKind::wav_rows) {
        w.rows = take((size_t)B * 2 * sizeof(int32_t));
        w.peak = take((size_t)B * sizeof(double));
        w.peak_bits = take((size_t)B * sizeof(unsigned int));
    }
    w.total = off;
    return GVX_OK;
}

int gl_open(gvx_gl_plan* p, int B, int T, int M, WsKind kind, bool plans_when_fused, void* ws, size_t ws_bytes, void* stream, GlCall* c) {
    const int rc = gl_layout(p, B, T, M, kind, plans_when_fused, c);
    if (rc != GVX_OK) return rc;
    if (B < 1 || T < 1) return gl_fail(GVX_ERR_INVALID_ARG, "B and T must be >= 1");
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return gl_fail(GVX_ERR_WORKSPACE, "workspace must be non-null and 256-byte aligned");
    if (ws_bytes < c->w.total) return gl_fail(GVX_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, c->w.total);
    c->ws = ws;
    c->s = (hipStream_t)stream;
    return GVX_OK;
}

}}  // namespace gvx::voc

// ---- host side of the calls ------------------------------------------------------------------------------------
namespace {

// what the stages of one gvx_griffin_lim* call share
struct GlRun {
    gvx_gl_plan* p; GlCall c; const float* window; int B, T, n_iter;
    const int32_t* lens;   // per-row frame counts of a ragged batch, or null: every launch is the uniform one, unchanged
    const float* tail;     // the rows' own window-sum tails (wss_tail_kernel) when lens, else null
    float* mag_t; float2 *ang, *reb[2]; float coef;   // coef = momentum / (1 + momentum)
};

// frame-major spectrum -> signal: C2R + overlap-add
// (ragged: every frame is transformed either way, the overlap-add skips the padded ones)
int istft_frames(const GlRun& r, float2* spec_t) {
    const gvx_gl_plan* p = r.p;
    const GlWs& w = r.c.w;
    const long n = (long)p->n_fft + (long)(r.T - 1) * p->hop;
    int rc = run_fft(r.p, r.c.fp->c2r, spec_t, r.c.at<float>(w.fr), r.c.at<char>(w.fft_work), r.c.fp->work_bytes, r.c.s);
    if (rc != GVX_OK) return rc;
    ragged_dispatch(r.lens != nullptr, [&](auto R) {
        gl_ola_kernel<decltype(R)::value><<<dim3((unsigned)((n + 255) / 256), r.B), 256, 0, r.c.s>>>(
            r.c.at<float>(w.fr), r.window, r.c.at<float>(w.wss), r.c.at<float>(w.y), p->n_fft, p->hop, r.T, n, r.lens, r.tail);
    });
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

// y = istft(spec) in LDS
int inverse_ola(const GlRun& r, const float2* spec) {
    const dim3 grid((unsigned)((r.T + 3 + GLI_BLOCKS - 1) / GLI_BLOCKS), r.B);
    ragged_dispatch(r.lens != nullptr, [&](auto R) {
        gl_inverse_ola_kernel<decltype(R)::value><<<grid, GLI_FRAMES * 64, GLI_FRAMES * FPAD * sizeof(float2), r.c.s>>>(
            spec, r.window, r.c.at<float>(r.c.w.wss), r.p->tw, r.c.at<float>(r.c.w.y), r.T, r.lens, r.tail);
    });
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

// one launch per iteration: signal -> rebuilt -> update -> new spectrum -> its signal (gl_iteration_kernel); the signal
// and tprev ping-pong between two buffers each (the framed-signal region of the rocFFT pipeline serves as the second y)
template <int FPW>
int iterate_one_launch(const GlRun& r) {
    constexpr int nbl = FPW * GLI_FRAMES - 3;
    constexpr size_t lds_bytes = (FPW * GLI_FRAMES * FPAD + GLI_TAB) * sizeof(float2);
    float* ybuf[2] = {r.c.at<float>(r.c.w.y), r.c.at<float>(r.c.w.fr)};
    const int rc = inverse_ola(r, r.ang);                       // signal of the initial angles
    if (rc != GVX_OK) return rc;
    const dim3 grid((unsigned)((r.T + 3 + nbl - 1) / nbl), r.B);
    for (int it = 0; it < r.n_iter; ++it) {
        const bool last = it == r.n_iter - 1;
        ragged_dispatch(r.lens != nullptr, [&](auto R) {
            gl_iteration_kernel<FPW, decltype(R)::value><<<grid, GLI_FRAMES * 64, lds_bytes, r.c.s>>>(
                ybuf[it & 1], ybuf[(it + 1) & 1], r.window, r.c.at<float>(r.c.w.wss), r.p->tw, r.mag_t, r.reb[it & 1], r.reb[(it + 1) & 1],
                last ? r.ang : nullptr, r.coef, it == 0, !last, r.T, r.lens, r.tail);
        });
        GL_HIP(hipGetLastError());
    }
    return GVX_OK;
}

// GVX_GL_TWO_KERNELS=1: the two-launch iteration (A/B runs)
int iterate_two_launch(const GlRun& r) {
    const long frames = (long)r.B * r.T;
    for (int it = 0; it < r.n_iter; ++it) {
        const int rc = inverse_ola(r, r.ang);                   // inverse = istft(angles)
        if (rc != GVX_OK) return rc;
        // rebuilt = stft(inverse); momentum update; tprev = rebuilt
        gl_forward_update_kernel<<<dim3((unsigned)((frames + GLF_FRAMES - 1) / GLF_FRAMES)), GLF_FRAMES * 64, 0, r.c.s>>>(
            r.c.at<float>(r.c.w.y), r.window, r.p->tw, r.mag_t, r.reb[0], r.ang, r.coef, it == 0, r.T, frames);
        GL_HIP(hipGetLastError());
    }
    return GVX_OK;
}

int iterate_rocfft(const GlRun& r) {
    const gvx_gl_plan* p = r.p;
    const GlWs& w = r.c.w;
    const long n = (long)p->n_fft + (long)(r.T - 1) * p->hop;
    const long nbin = (long)r.B * r.T * p->bins;
    for (int it = 0; it < r.n_iter; ++it) {
        int rc = istft_frames(r, r.ang);                        // inverse = istft(angles)
        if (rc != GVX_OK) return rc;
        gl_frame_kernel<false, float><<<dim3((unsigned)((long)r.B * r.T)), 256, 0, r.c.s>>>(r.c.at<float>(w.y), r.window, r.c.at<float>(w.fr), p->n_fft,
                                                                                            p->hop, r.T, n, WavRows{});
        GL_HIP(hipGetLastError());
        float2* cur = r.reb[it & 1];
        rc = run_fft(r.p, r.c.fp->r2c, r.c.at<float>(w.fr), cur, r.c.at<char>(w.fft_work), r.c.fp->work_bytes, r.c.s);  // rebuilt = stft(inverse)
        if (rc != GVX_OK) return rc;
        gl_update_kernel<<<blocks_for(nbin), 256, 0, r.c.s>>>(cur, r.reb[(it + 1) & 1], r.mag_t, r.ang, r.coef, it == 0, nbin);
        GL_HIP(hipGetLastError());
    }
    return GVX_OK;
}

// gvx_griffin_lim (lens == nullptr) and gvx_griffin_lim_ragged
int griffin_lim_impl(gvx_gl_plan* p, const float* mag, const float* window, int B, int T, const int32_t* lens, int n_iter, float momentum,
                     float* phase_out, float* wav_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !mag || !window) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_iter < 0) return gl_fail(GVX_ERR_INVALID_ARG, "n_iter must be >= 0");
    if (B < 1 || T < 1) return gl_fail(GVX_ERR_INVALID_ARG, "B and T must be >= 1");
    GlRun r{p, {}, window, B, T, n_iter, lens};
    int rc = gl_open(p, B, T, 0, lens ? WsKind::ragged_gl : WsKind::uniform, true, ws, ws_bytes, stream, &r.c);
    if (rc != GVX_OK) return rc;
    const GlWs& w = r.c.w;
    hipStream_t s = r.c.s;
    r.tail = lens ? r.c.at<float>(w.wss_tail) : nullptr;
    r.mag_t = r.c.at<float>(w.mag);
    r.ang = r.c.at<float2>(w.ang);
    r.reb[0] = r.c.at<float2>(w.reb0);
    r.reb[1] = r.c.at<float2>(w.reb1);
    r.coef = momentum / (1.f + momentum);
    if (lens && p->n_fft > p->hop) {
        wss_tail_kernel<<<dim3((unsigned)((p->n_fft - p->hop + 255) / 256), B), 256, 0, s>>>(window, lens, r.c.at<float>(w.wss_tail), p->n_fft,
                                                                                           p->hop, T);
        GL_HIP(hipGetLastError());
    }
    const long n = (long)p->n_fft + (long)(T - 1) * p->hop;
    const long nbin = (long)B * T * p->bins;
    GL_HIP(launch_transpose<float>(mag, r.mag_t, B, p->bins, T, s));
    wss_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(window, r.c.at<float>(w.wss), p->n_fft, p->hop, T, n);
    GL_HIP(hipGetLastError());
    gl_init_kernel<<<blocks_for(nbin), 256, 0, s>>>(r.mag_t, r.ang, nbin);
    GL_HIP(hipGetLastError());
    const GlPath path = gl_path(p, lens, n_iter, T);
    switch (path) {
        case GlPath::one_launch_two_frames: rc = iterate_one_launch<2>(r); break;
        case GlPath::one_launch_one_frame: rc = iterate_one_launch<1>(r); break;
        case GlPath::two_launch: rc = iterate_two_launch(r); break;
        case GlPath::rocfft: rc = iterate_rocfft(r); break;
    }
    if (rc != GVX_OK) return rc;
    // phase = angle(angles); final spectrum = mag * exp(i phase) (not `angles` itself: they differ where mag < 0)
    float2* spec_t = r.reb[1];
    float* phase_t = r.c.at<float>(w.fr);   // frames * n_fft floats >= frames * bins
    // ragged: one grid row per utterance over its T * bins elements; uniform: one flat grid over all of them
    const long n_final = lens ? (long)T * p->bins : nbin;
    const dim3 grid_final = lens ? dim3(blocks_for(n_final, 256, 1024), B) : dim3(blocks_for(nbin));
    ragged_dispatch(lens != nullptr, [&](auto R) {
        gl_final_kernel<decltype(R)::value><<<grid_final, 256, 0, s>>>(r.ang, r.mag_t, wav_out ? spec_t : nullptr, phase_out ? phase_t : nullptr,
                                                                       n_final, p->bins, T, lens);
    });
    GL_HIP(hipGetLastError());
    if (phase_out) GL_HIP(launch_transpose<float>(phase_t, phase_out, B, T, p->bins, s));
    if (wav_out) {
        rc = path != GlPath::rocfft ? inverse_ola(r, spec_t) : istft_frames(r, spec_t);
        if (rc != GVX_OK) return rc;
        if (lens) {   // the signal buffer is valid up to each row's n_b only: zeros behind it in the result
            copy_rows_ragged_kernel<<<dim3(blocks_for(n, 256, 1024), B), 256, 0, s>>>(r.c.at<float>(w.y), wav_out, n, p->n_fft, p->hop, lens);
            GL_HIP(hipGetLastError());
        } else {
            GL_HIP(hipMemcpyAsync(wav_out, r.c.at<float>(w.y), (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    return GVX_OK;
}

}  // namespace

extern "C" {

int gvx_gl_plan_create(int n_fft, int hop, gvx_gl_plan** out) {
    if (!out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_fft < 8 || (n_fft & 3) || hop < 4 || (hop & 3) || hop > n_fft)
        return gl_fail(GVX_ERR_UNSUPPORTED, "n_fft = %d, hop = %d: both must be multiples of 4 with hop <= n_fft", n_fft, hop);
    static bool setup_done = false;
    if (!setup_done) {
        GL_FFT(rocfft_setup());
        setup_done = true;
    }
    gvx_gl_plan* p = new gvx_gl_plan();
    p->n_fft = n_fft; p->hop = hop; p->bins = n_fft / 2 + 1;
    if (n_fft == 1024 && hop == 256) {   // tables of the fused Griffin-Lim path
        std::vector<float2> h(FN + 513 + FN);   // w_512^m, w_1024^k, and gl_iteration_kernel's per-pass gather of the first table
        const double two_pi = 6.283185307179586476925286766559;
        for (int m = 0; m < FN; ++m) h[m] = make_float2((float)std::cos(two_pi * m / 512.0), (float)-std::sin(two_pi * m / 512.0));
        for (int k = 0; k <= 512; ++k) h[FN + k] = make_float2((float)std::cos(two_pi * k / 1024.0), (float)-std::sin(two_pi * k / 1024.0));
        float2* g = h.data() + FN + 513;
        for (int i = 0; i < FN; ++i) g[i] = make_float2(1.f, 0.f);
        for (int r = 1; r < 8; ++r) {
            for (int k = 0; k < 8; ++k) g[(r - 1) * 8 + k] = h[(r * k * 8) & (FN - 1)];
            for (int k = 0; k < 64; ++k) g[64 + (r - 1) * 64 + k] = h[(r * k) & (FN - 1)];
        }
        if (hipMalloc(&p->tw, h.size() * sizeof(float2)) != hipSuccess ||
            hipMemcpy(p->tw, h.data(), h.size() * sizeof(float2), hipMemcpyHostToDevice) != hipSuccess) {
            delete p;
            return gl_fail(GVX_ERR_HIP, "twiddle table allocation failed");
        }
        const int lds_inv = GLI_FRAMES * FPAD * (int)sizeof(float2), lds_it1 = (GLI_FRAMES * FPAD + GLI_TAB) * (int)sizeof(float2),
                  lds_it2 = (2 * GLI_FRAMES * FPAD + GLI_TAB) * (int)sizeof(float2);
        auto lds = [](auto* kernel, int bytes) {
            return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
        };
        if (!lds(gl_inverse_ola_kernel<false>, lds_inv) || !lds(gl_inverse_ola_kernel<true>, lds_inv) ||
            !lds(gl_iteration_kernel<1, false>, lds_it1) || !lds(gl_iteration_kernel<1, true>, lds_it1) ||
            !lds(gl_iteration_kernel<2, false>, lds_it2) || !lds(gl_iteration_kernel<2, true>, lds_it2)) {
            delete p;
            return gl_fail(GVX_ERR_HIP, "hipFuncSetAttribute failed");
        }
    }
    *out = p;
    return GVX_OK;
}

void gvx_gl_plan_destroy(gvx_gl_plan* p) {
    if (!p) return;
    for (auto& kv : p->plans) {
        if (kv.second.r2c) rocfft_plan_destroy(kv.second.r2c);
        if (kv.second.c2r) rocfft_plan_destroy(kv.second.c2r);
    }
    if (p->info) rocfft_execution_info_destroy(p->info);
    if (p->tw) (void)hipFree(p->tw);
    delete p;
}

size_t gvx_gl_workspace_bytes(gvx_gl_plan* p, int B, int T, int n_mels) {
    GlCall c;
    if (!p || B < 1 || T < 1 || gl_layout(p, B, T, n_mels, WsKind::uniform, true, &c) != GVX_OK) return 0;
    return c.w.total;
}

size_t gvx_gl_workspace_bytes_ragged(gvx_gl_plan* p, int B, int T, int n_mels) {
    GlCall c;
    if (!p || B < 1 || T < 1 || gl_layout(p, B, T, n_mels, WsKind::ragged_gl, true, &c) != GVX_OK) return 0;
    return c.w.total;
}

int gvx_stft(gvx_gl_plan* p, const float* signal, const float* window, int B, long n_samples, float* spec_out, void* ws, size_t ws_bytes,
             void* stream) {
    if (!p || !signal || !window || !spec_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_samples < p->n_fft) return gl_fail(GVX_ERR_INVALID_ARG, "signal shorter than one frame");
    const int T = (int)((n_samples - p->n_fft) / p->hop + 1);
    GlCall c;
    int rc = gl_open(p, B, T, 0, WsKind::uniform, true, ws, ws_bytes, stream, &c);
    if (rc != GVX_OK) return rc;
    const GlWs& w = c.w;
    gl_frame_kernel<false, float><<<dim3((unsigned)((long)B * T)), 256, 0, c.s>>>(signal, window, c.at<float>(w.fr), p->n_fft, p->hop, T, n_samples, WavRows{});
    GL_HIP(hipGetLastError());
    rc = run_fft(p, c.fp->r2c, c.at<float>(w.fr), c.at<float2>(w.reb0), c.at<char>(w.fft_work), c.fp->work_bytes, c.s);
    if (rc != GVX_OK) return rc;
    GL_HIP(launch_transpose<float2>(c.at<float2>(w.reb0), reinterpret_cast<float2*>(spec_out), B, T, p->bins, c.s));
    return GVX_OK;
}

int gvx_istft(gvx_gl_plan* p, const float* spec, const float* window, int B, int T, float* signal_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !spec || !window || !signal_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    GlRun r{p, {}, window, B, T};
    int rc = gl_open(p, B, T, 0, WsKind::uniform, true, ws, ws_bytes, stream, &r.c);
    if (rc != GVX_OK) return rc;
    const GlWs& w = r.c.w;
    const long n = (long)p->n_fft + (long)(T - 1) * p->hop;
    GL_HIP(launch_transpose<float2>(reinterpret_cast<const float2*>(spec), r.c.at<float2>(w.ang), B, p->bins, T, r.c.s));
    wss_kernel<<<(unsigned)((n + 255) / 256), 256, 0, r.c.s>>>(window, r.c.at<float>(w.wss), p->n_fft, p->hop, T, n);
    GL_HIP(hipGetLastError());
    rc = istft_frames(r, r.c.at<float2>(w.ang));
    if (rc != GVX_OK) return rc;
    GL_HIP(hipMemcpyAsync(signal_out, r.c.at<float>(w.y), (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, r.c.s));
    return GVX_OK;
}

int gvx_mel_to_magnitude(gvx_gl_plan* p, const float* mel_db, const float* inv_basis, int B, int n_mels, int T, int log10_kind, float ref,
                         float* mag_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !mel_db || !inv_basis || !mag_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_mels & 3) return gl_fail(GVX_ERR_UNSUPPORTED, "n_mels must be a multiple of 4");
    GlCall c;
    const int rc = gl_open(p, B, T, n_mels, WsKind::uniform, true, ws, ws_bytes, stream, &c);
    if (rc != GVX_OK) return rc;
    const GlWs& w = c.w;
    const float refc = ref > 1e-5f ? ref : 1e-5f;
    const float log_ref = log10_kind ? log10f(refc) : logf(refc);
    db_to_amp_transpose_kernel<<<dim3((T + 31) / 32, (n_mels + 31) / 32, B), dim3(32, 8), 0, c.s>>>(mel_db, c.at<float>(w.amp), n_mels, T,
                                                                                                   log10_kind, log_ref);
    GL_HIP(hipGetLastError());
    // mel2fft (utils/audio/base.py:143-145): mag_t[(b,t)][bin] = sum_m inv_basis[bin][m] * amp_t[(b,t)][m]
    gvx::GemmParams g{};
    g.A = c.at<float>(w.amp); g.amap = gvx::RowMap{B * T, 0, (long)n_mels};
    g.W = inv_basis; g.ldw = n_mels;
    g.C = c.at<float>(w.mag); g.cmap = gvx::RowMap{B * T, 0, (long)p->bins};
    g.M = B * T; g.N = p->bins; g.K = n_mels; g.act = gvx::ACT_NONE;
    GL_HIP(gvx::launch_gemm(g, c.s));
    GL_HIP(launch_transpose<float>(c.at<float>(w.mag), mag_out, B, T, p->bins, c.s));
    return GVX_OK;
}

int gvx_griffin_lim(gvx_gl_plan* p, const float* mag, const float* window, int B, int T, int n_iter, float momentum, float* phase_out,
                    float* wav_out, void* ws, size_t ws_bytes, void* stream) {
    return griffin_lim_impl(p, mag, window, B, T, nullptr, n_iter, momentum, phase_out, wav_out, ws, ws_bytes, stream);
}

int gvx_griffin_lim_ragged(gvx_gl_plan* p, const float* mag, const float* window, int B, int T, const int32_t* frame_lengths, int n_iter,
                           float momentum, float* phase_out, float* wav_out, void* ws, size_t ws_bytes, void* stream) {
    if (!frame_lengths) return gl_fail(GVX_ERR_INVALID_ARG, "null frame_lengths (gvx_griffin_lim is the call for rows of one length)");
    return griffin_lim_impl(p, mag, window, B, T, frame_lengths, n_iter, momentum, phase_out, wav_out, ws, ws_bytes, stream);
}

}  // C ABI
