// Batched waveform -> mel (dB) front-end on the GPU: the reference's convert_wav2mel chain (core/processors.py:70-79: stft, abs,
// fft2mel, amplitude_to_db) for rows of one length (gvx_wav_to_mel) and for PCM recordings of different lengths that are trimmed
// of silence and peak-normalised per row on the way (gvx_wav_trim_bounds, gvx_wav_to_mel_ragged).  Both calls run one chain,
// wav_to_mel_chain; n_fft 1024 / hop 256 frames, windows, transforms and takes magnitudes in one kernel (fft512_lds.h), every other
// size - and GVX_GL_ROCFFT=1 - goes through rocFFT.  The plan, the workspace and the path choice are those of the mel -> wav half
// (griffinlim.hip, vocoder_internal.h); the even/odd split of the real transform is fft512_lds.h's rfft_split.
//
// Order of this file: kernels, the host side of the calls, the C ABI.
#include "fft512_lds.h"
#include "vocoder_internal.h"

#include <cmath>

using namespace gvx::voc;

namespace {

// ---- kernels ------------------------------------------------------------------------------------------------

// |spec| of a frame-major complex spectrum into rows padded to kp floats (kp % 4 == 0, pad = 0) for the GEMM
__global__ void magnitude_kernel(const float2* spec_t, float* mag, int bins, int kp, long frames) {
    const long total = frames * kp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long fr = i / kp;
        const int k = (int)(i - fr * kp);
        float v = 0.f;
        if (k < bins) { const float2 z = spec_t[fr * bins + k]; v = hypotf(z.x, z.y); }
        mag[i] = v;
    }
}

// basis [n_mels][bins] -> padded [n_mels][kp]
__global__ void pad_rows_kernel(const float* src, float* dst, int rows, int cols, int kp) {
    const int total = rows * kp;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int r = i / kp, c = i - r * kp;
        dst[i] = c < cols ? src[r * cols + c] : 0.f;
    }
}

// mel_db[b][m][t] = log(max(amin, mel_t[(b,t)][m])) - log(max(amin, ref))      (utils/audio/base.py:24-36, power=False, scale=1)
// RAGGED: frames t >= T_b = rows[b][1] of mel_db are exact zeros (the collate's padding, not log(amin)), and the workgroups of the
// first mel tile also write the gate target of the batch: gate[b][t] = 1 from the row's last frame on, 0 before (gate may be null)
template <bool RAGGED>
__global__ void amp_to_db_transpose_kernel(const float* mel_t, float* mel_db, int M, int T, int log10_kind, float log_ref,
                                           const int32_t* rows, float* gate) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, t0 = blockIdx.y * 32, m0 = blockIdx.x * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int Tb = RAGGED ? rows[2 * b + 1] : T;
    for (int r = ty; r < 32; r += 8) {
        const int t = t0 + r, m = m0 + tx;
        float v = 0.f;
        if (t < Tb && m < M) {
            const float a = fmaxf(1e-5f, mel_t[((long)b * T + t) * M + m]);
            v = (log10_kind ? log10f(a) : logf(a)) - log_ref;
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int m = m0 + r, t = t0 + tx;
        if (t < T && m < M) mel_db[((long)b * M + m) * T + t] = tile[tx][r];
    }
    if (RAGGED && gate && m0 == 0 && ty == 0 && t0 + tx < T) gate[(long)b * T + t0 + tx] = t0 + tx >= Tb - 1 ? 1.f : 0.f;
}

// frames of a signal -> |rfft(win * frame)| into rows padded to kp floats (kp >= 513, pad = 0): the magnitude input of the
// mel GEMM (convert_wav2mel: stft + abs, core/processors.py:70-79) without the framed-signal and complex-spectrum round trips
// RAGGED: grid (ceil(T / 4), B), so a workgroup's four frames belong to one row; row b's frame t starts at sample left_b + t*256 of
// its PCM row and is read through pcm_sample (the division by the peak happens in the load: no normalised copy of the batch exists).
// Whether a frame exists is a test per wave (a frame is a wave): one with t >= T_b writes its padded magnitude row as zeros - the
// GEMM reads every row - and leaves before it touches the twiddle table, so a workgroup wholly behind its row's end costs one store
template <bool RAGGED, typename PCM>
__global__ __launch_bounds__(GLF_FRAMES * 64) void stft_magnitude_kernel(const PCM* __restrict__ x, long n_samples, const float* __restrict__ win,
                                                                         const float2* __restrict__ tw, float* __restrict__ mag, int kp,
                                                                         int T, long frames, WavRows wr) {
    __shared__ __attribute__((aligned(16))) float2 fsm[GLF_FRAMES * FPAD];
    const int tid = threadIdx.x, j = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float2* buf = fsm + wave * FPAD;
    // the frame f of this wave, whether it is transformed, and where its samples start
    long f;
    bool valid = true, norm = false;
    const PCM* xb = x;
    double peak = 1.0;
    if constexpr (RAGGED) {
        const int b = blockIdx.y, t = (int)blockIdx.x * GLF_FRAMES + wave;
        if (t >= T) return;
        f = (long)b * T + t;
        if (t >= wr.rows[2 * b + 1]) {
            float* row = mag + f * kp;
            for (int k = j; k < kp; k += 64) row[k] = 0.f;
            return;
        }
        xb = x + (long)b * n_samples + wr.rows[2 * b] + (long)t * 256;
        peak = wr.peak[b];
        norm = wr.normalize != 0;
    } else {
        f = (long)blockIdx.x * GLF_FRAMES + wave;
        valid = f < frames;   // a wave behind the last frame still takes part in the transform, on zeros
        if (valid) {
            const unsigned fu = (unsigned)f;
            const int b = (int)(fu / (unsigned)T), t = (int)(fu - (unsigned)b * (unsigned)T);
            xb = x + (long)b * n_samples + (long)t * 256;
        }
    }
    // scalar loads: a PCM row, and a float row as well, need not be 8-byte aligned (n_samples is arbitrary)
    auto sample = [&](int i) -> float { if constexpr (RAGGED) return pcm_sample(xb[i], peak, norm); else return xb[i]; };
    float2 v[8] = {};
    if (valid) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n2 = 2 * (j + 64 * r);
            const float2 w = *reinterpret_cast<const float2*>(win + n2);
            v[r] = make_float2(w.x * sample(n2), w.y * sample(n2 + 1));
        }
    }
    fft512_wave<false>(v, buf, tw, j, true);
    wave_lds_fence();
    if (!valid) return;
    const float2* tw2 = tw + FN;
    float* row = mag + f * kp;
    for (int k = j; k < kp; k += 64) {
        float out = 0.f;
        if (k <= 512) {
            const float2 X = rfft_split(buf[fpad(k & (FN - 1))], buf[fpad((512 - k) & (FN - 1))], tw2[k], k == 0 || k == 512);
            out = hypotf(X.x, X.y);
        }
        row[k] = out;
    }
}

// ---- silence bounds, peak and row plan of the ragged front-end --------------------------------------------------------------
__device__ __forceinline__ long clamp_len(long v, long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// Is the chunk x[0, len) at or above the silence threshold?  dBFS (utils/__init__.py:44-54) is 20 log10(rms / full scale), so
// dBFS >= trim_dbfs  <=>  sum x^2 >= len * thr with thr = full_scale^2 * 10^(trim_dbfs / 10).  int16: the sum is an exact 64-bit
// integer (order independent) and the comparison is made once in double; float32 (full scale 1.0): double partial sums per lane,
// added in a fixed butterfly.  One wave, every lane returns the same answer.
template <typename PCM>
__device__ __forceinline__ bool chunk_is_loud(const PCM* x, int len, double thr, int lane) {
    if constexpr (sizeof(PCM) == 2) {
        long long s = 0;
        for (int i = lane; i < len; i += 64) { const int v = x[i]; s += (long long)(v * v); }
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        return (double)s >= (double)len * thr;
    } else {
        double s = 0.0;
        for (int i = lane; i < len; i += 64) { const double v = (double)x[i]; s += v * v; }
        for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
        return s >= (double)len * thr;
    }
}

// get_non_silent_boundary (utils/__init__.py:56-76) per row, one workgroup of four waves per row: chunks of `chunk` samples are
// walked from the row's start and - aligned to its last sample, as the reference walks the flipped signal - from its end, four at
// a time (a wave takes a chunk of each walk), until both walks have met a chunk at or above the threshold.  bounds[b] = {start of
// the first such chunk from the left, n_b - start of the first such chunk from the right}.  When no chunk passes, a walk ends on its
// last chunk start like the reference's loop variable does (left >= right then: the caller's "empty row").  thr NaN: no trimming.
template <typename PCM>
__global__ __launch_bounds__(256) void wav_trim_bounds_kernel(const PCM* __restrict__ pcm, long n_max, const int32_t* __restrict__ sample_lengths,
                                                              int chunk, double thr, int32_t* __restrict__ bounds) {
    __shared__ int first[2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long n = clamp_len(sample_lengths[b], n_max);
    if (thr != thr || n == 0) {
        if (tid == 0) { bounds[2 * b] = 0; bounds[2 * b + 1] = (int32_t)n; }
        return;
    }
    const PCM* x = pcm + (long)b * n_max;
    const int nch = (int)((n + chunk - 1) / chunk);
    if (tid < 2) first[tid] = nch;
    __syncthreads();
    bool done_l = false, done_r = false;
    for (int c0 = 0; c0 < nch && !(done_l && done_r); c0 += 4) {
        const int c = c0 + wave;
        if (c < nch) {
            const long lo = (long)c * chunk;
            const int len = (int)(n - lo < chunk ? n - lo : chunk);
            if (!done_l && chunk_is_loud(x + lo, len, thr, lane) && lane == 0) atomicMin(&first[0], c);
            if (!done_r && chunk_is_loud(x + (n - lo - len), len, thr, lane) && lane == 0) atomicMin(&first[1], c);
        }
        __syncthreads();
        done_l = first[0] < nch;
        done_r = first[1] < nch;
        __syncthreads();
    }
    if (tid == 0) {
        const int cl = first[0] < nch ? first[0] : nch - 1, cr = first[1] < nch ? first[1] : nch - 1;
        bounds[2 * b] = (int32_t)((long)cl * chunk);
        bounds[2 * b + 1] = (int32_t)(n - (long)cr * chunk);
    }
}

// max |sample| of row b over its clamped bounds (normalize_signal's max(|min|, |max|), utils/audio/base.py:20-22, without the
// reference's int16 wrap of |-32768|): int16 as the integer, float32 as its bit pattern - both order like unsigned integers
template <typename PCM>
__global__ void wav_peak_bounds_kernel(const PCM* __restrict__ pcm, long n_max, const int32_t* __restrict__ bounds, unsigned int* peak_bits) {
    const int b = blockIdx.y;
    const long left = clamp_len(bounds[2 * b], n_max), right = clamp_len(bounds[2 * b + 1], n_max);
    const PCM* x = pcm + (long)b * n_max;
    unsigned int m = 0;
    for (long i = left + (long)blockIdx.x * blockDim.x + threadIdx.x; i < right; i += (long)gridDim.x * blockDim.x) {
        unsigned int a;
        if constexpr (sizeof(PCM) == 2) { const int v = x[i]; a = (unsigned int)(v < 0 ? -v : v); }
        else { const float v = fabsf(x[i]); a = v == v ? __float_as_uint(v) : 0u; }
        m = a > m ? a : m;
    }
    for (int off = 32; off >= 1; off >>= 1) { const unsigned int o = __shfl_xor(m, off); m = o > m ? o : m; }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(peak_bits + b, m);
}

// one thread per row: bounds + peak -> rows[b] = {left, T_b}, the peak as a double, the frame count and the status word of the
// row (GVX_WAV_ROW_* of the header).  A row with any of the first three bits has T_b = 0: nothing of it is read again.
template <typename PCM>
__global__ void wav_row_plan_kernel(const int32_t* __restrict__ bounds, const unsigned int* __restrict__ peak_bits, long n_max, int n_fft, int hop,
                                    int T, int B, int32_t* __restrict__ rows, double* __restrict__ peak, int32_t* __restrict__ frame_lengths,
                                    int32_t* __restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long left = clamp_len(bounds[2 * b], n_max), right = clamp_len(bounds[2 * b + 1], n_max);
    double pk;
    if constexpr (sizeof(PCM) == 2) pk = (double)peak_bits[b]; else pk = (double)__uint_as_float(peak_bits[b]);
    int32_t st = 0;
    long Tb = 0;
    if (left >= right) st = GVX_WAV_ROW_EMPTY;
    else if (right - left < n_fft) st = GVX_WAV_ROW_SHORT;
    else if (!(pk > 0.0)) st = GVX_WAV_ROW_SILENT;
    else {
        Tb = (right - left - n_fft) / hop + 1;
        if (Tb > T) { Tb = T; st = GVX_WAV_ROW_CUT; }
    }
    rows[2 * b] = (int32_t)left;
    rows[2 * b + 1] = (int32_t)Tb;
    peak[b] = Tb > 0 ? pk : 1.0;
    frame_lengths[b] = (int32_t)Tb;
    status[b] = st;
}

// ---- host side of the calls ------------------------------------------------------------------------------------

// STFT -> magnitude -> padded basis -> GEMM -> dB of B rows of T frames, behind the entry points' checks.  Uniform: x is [B][n_row]
// float32, wr is empty, gate_out null.  RAGGED: x is the PCM batch, wr says where each row's frames start and how many it has.
template <bool RAGGED, typename PCM>
int wav_to_mel_chain(gvx_gl_plan* p, const GlCall& c, const PCM* x, long n_row, WavRows wr, const float* window,
                     const float* mel_basis, int B, int T, int n_mels, int log10_kind, float ref, float* mel_db_out, float* gate_out) {
    const GlWs& w = c.w;
    hipStream_t s = c.s;
    const long frames = (long)B * T;
    const int kp = (p->bins + 3) & ~3;                     // GEMM K must be a multiple of 4: 513 -> 516, zero padded
    // workspace reuse: fr = framed signal, reb0 = spectrum, ang = padded magnitudes (kp floats per frame inside bins float2: kp <= 2 bins
    // for every n_fft), amp = mel amplitudes; the padded basis has its own region
    float* mag_p = c.at<float>(w.ang);
    float* basis_p = c.at<float>(w.basis);
    if (gl_fused(p)) {   // n_fft 1024 / hop 256: framing + window + FFT + magnitude in one kernel
        const dim3 grid = RAGGED ? dim3((unsigned)((T + GLF_FRAMES - 1) / GLF_FRAMES), B) : dim3((unsigned)((frames + GLF_FRAMES - 1) / GLF_FRAMES));
        stft_magnitude_kernel<RAGGED, PCM><<<grid, GLF_FRAMES * 64, 0, s>>>(x, n_row, window, p->tw, mag_p, kp, T, frames, wr);
        GL_HIP(hipGetLastError());
    } else {
        const dim3 grid = RAGGED ? dim3((unsigned)T, B) : dim3((unsigned)frames);
        gl_frame_kernel<RAGGED, PCM><<<grid, 256, 0, s>>>(x, window, c.at<float>(w.fr), p->n_fft, p->hop, T, n_row, wr);
        GL_HIP(hipGetLastError());
        const int rc = run_fft(p, c.fp->r2c, c.at<float>(w.fr), c.at<float2>(w.reb0), c.at<char>(w.fft_work), c.fp->work_bytes, s);
        if (rc != GVX_OK) return rc;
        magnitude_kernel<<<blocks_for(frames * kp), 256, 0, s>>>(c.at<float2>(w.reb0), mag_p, p->bins, kp, frames);
        GL_HIP(hipGetLastError());
    }
    pad_rows_kernel<<<blocks_for((long)n_mels * kp), 256, 0, s>>>(mel_basis, basis_p, n_mels, p->bins, kp);
    GL_HIP(hipGetLastError());
    // fft2mel (utils/audio/base.py:139-141): mel_t[(b,t)][m] = sum_k basis[m][k] * |S|[(b,t)][k], over every padded frame (the rows
    // of frames that do not exist are zeros)
    gvx::GemmParams g{};
    g.A = mag_p; g.amap = gvx::RowMap{(int)frames, 0, (long)kp};
    g.W = basis_p; g.ldw = kp;
    g.C = c.at<float>(w.amp); g.cmap = gvx::RowMap{(int)frames, 0, (long)n_mels};
    g.M = (int)frames; g.N = n_mels; g.K = kp; g.act = gvx::ACT_NONE;
    GL_HIP(gvx::launch_gemm(g, s));
    const float refc = ref > 1e-5f ? ref : 1e-5f;
    const float log_ref = log10_kind ? log10f(refc) : logf(refc);
    amp_to_db_transpose_kernel<RAGGED><<<dim3((n_mels + 31) / 32, (T + 31) / 32, B), dim3(32, 8), 0, s>>>(c.at<float>(w.amp), mel_db_out, n_mels,
                                                                                                         T, log10_kind, log_ref, wr.rows, gate_out);
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

// peak and row plan of every row, then the chain
template <typename PCM>
int wav_to_mel_ragged_impl(gvx_gl_plan* p, const GlCall& c, const PCM* pcm, const float* window, const float* mel_basis, int B,
                           long n_max, const int32_t* bounds, int normalize, int n_mels, int log10_kind, float ref, int T, float* mel_db_out,
                           float* gate_out, int32_t* frame_lengths_out, int32_t* row_status_out) {
    unsigned int* peak_bits = c.at<unsigned int>(c.w.peak_bits);
    int32_t* rows = c.at<int32_t>(c.w.rows);
    GL_HIP(hipMemsetAsync(peak_bits, 0, (size_t)B * sizeof(unsigned int), c.s));
    wav_peak_bounds_kernel<PCM><<<dim3(64, B), 256, 0, c.s>>>(pcm, n_max, bounds, peak_bits);
    GL_HIP(hipGetLastError());
    wav_row_plan_kernel<PCM><<<(B + 63) / 64, 64, 0, c.s>>>(bounds, peak_bits, n_max, p->n_fft, p->hop, T, B, rows, c.at<double>(c.w.peak),
                                                           frame_lengths_out, row_status_out);
    GL_HIP(hipGetLastError());
    const WavRows wr{rows, c.at<double>(c.w.peak), normalize};
    return wav_to_mel_chain<true, PCM>(p, c, pcm, n_max, wr, window, mel_basis, B, T, n_mels, log10_kind, ref, mel_db_out, gate_out);
}

int check_pcm(const void* pcm, int pcm_kind, int B, long n_max) {
    if (!pcm) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (pcm_kind != GVX_PCM_INT16 && pcm_kind != GVX_PCM_FLOAT32) return gl_fail(GVX_ERR_INVALID_ARG, "pcm_kind %d is neither int16 (0) nor float32 (1)", pcm_kind);
    if (B < 1 || n_max < 1 || n_max > 0x7fffffffL) return gl_fail(GVX_ERR_INVALID_ARG, "B and n_max must be >= 1 (n_max below 2^31)");
    if (reinterpret_cast<uintptr_t>(pcm) & (pcm_kind == GVX_PCM_INT16 ? 1 : 3)) return gl_fail(GVX_ERR_INVALID_ARG, "pcm is not aligned to its sample type");
    return GVX_OK;
}

inline int wav_frames_of(const gvx_gl_plan* p, long n) { return n >= p->n_fft ? (int)((n - p->n_fft) / p->hop + 1) : 1; }

}  // namespace

extern "C" {

int gvx_wav_to_mel(gvx_gl_plan* p, const float* signal, const float* window, const float* mel_basis, int B, long n_samples, int n_mels,
                   int log10_kind, float ref, float* mel_db_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !signal || !window || !mel_basis || !mel_db_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_samples < p->n_fft) return gl_fail(GVX_ERR_INVALID_ARG, "signal shorter than one frame");
    if (n_mels < 1) return gl_fail(GVX_ERR_INVALID_ARG, "n_mels must be >= 1");
    const int T = (int)((n_samples - p->n_fft) / p->hop + 1);
    GlCall c;
    const int rc = gl_open(p, B, T, n_mels, WsKind::uniform, true, ws, ws_bytes, stream, &c);
    if (rc != GVX_OK) return rc;
    return wav_to_mel_chain<false, float>(p, c, signal, n_samples, WavRows{}, window, mel_basis, B, T, n_mels, log10_kind, ref, mel_db_out,
                                          nullptr);
}

size_t gvx_wav_to_mel_ragged_workspace_bytes(gvx_gl_plan* p, int B, long n_max, int n_mels) {
    GlCall c;
    if (!p || B < 1 || n_max < 1 || n_mels < 1 || gl_layout(p, B, wav_frames_of(p, n_max), n_mels, WsKind::wav_rows, false, &c) != GVX_OK) return 0;
    return c.w.total;
}

int gvx_wav_trim_bounds(const void* pcm, int pcm_kind, int B, long n_max, const int32_t* sample_lengths, int fs, float trim_dbfs,
                        int32_t* bounds_out, void* stream) {
    int rc = check_pcm(pcm, pcm_kind, B, n_max);
    if (rc != GVX_OK) return rc;
    if (!sample_lengths || !bounds_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    const int chunk = (int)(20 * 0.001 * fs);   // the reference's expression (utils/__init__.py:60-61)
    if (fs < 1 || chunk < 1) return gl_fail(GVX_ERR_INVALID_ARG, "fs = %d gives no 20 ms chunk", fs);
    if (trim_dbfs > 0.f) return gl_fail(GVX_ERR_INVALID_ARG, "trim_dbfs = %g is above full scale", (double)trim_dbfs);
    hipStream_t s = (hipStream_t)stream;
    // NaN stays NaN: no trimming.  Full scale is the reference's np.iinfo(int16).max, 1.0 for float32 samples.
    const double rel = std::pow(10.0, (double)trim_dbfs / 10.0);
    if (pcm_kind == GVX_PCM_INT16)
        wav_trim_bounds_kernel<int16_t><<<dim3((unsigned)B), 256, 0, s>>>(static_cast<const int16_t*>(pcm), n_max, sample_lengths, chunk,
                                                                          32767.0 * 32767.0 * rel, bounds_out);
    else
        wav_trim_bounds_kernel<float><<<dim3((unsigned)B), 256, 0, s>>>(static_cast<const float*>(pcm), n_max, sample_lengths, chunk, rel, bounds_out);
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

int gvx_wav_to_mel_ragged(gvx_gl_plan* p, const void* pcm, int pcm_kind, const float* window, const float* mel_basis, int B, long n_max,
                          const int32_t* bounds, int normalize, int n_mels, int log10_kind, float ref, int T_out, float* mel_db_out,
                          float* gate_out, int32_t* frame_lengths_out, int32_t* row_status_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !window || !mel_basis || !bounds || !mel_db_out || !frame_lengths_out || !row_status_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    int rc = check_pcm(pcm, pcm_kind, B, n_max);
    if (rc != GVX_OK) return rc;
    if (n_mels < 1 || T_out < 1) return gl_fail(GVX_ERR_INVALID_ARG, "n_mels and T_out must be >= 1");
    if ((long)B * T_out > 0x7fffffffL / ((p->bins + 3) & ~3)) return gl_fail(GVX_ERR_UNSUPPORTED, "%d x %d frames are too many for one call", B, T_out);
    GlCall c;
    rc = gl_open(p, B, T_out, n_mels, WsKind::wav_rows, false, ws, ws_bytes, stream, &c);
    if (rc != GVX_OK) return rc;
    if (pcm_kind == GVX_PCM_INT16)
        return wav_to_mel_ragged_impl(p, c, static_cast<const int16_t*>(pcm), window, mel_basis, B, n_max, bounds, normalize, n_mels, log10_kind,
                                      ref, T_out, mel_db_out, gate_out, frame_lengths_out, row_status_out);
    return wav_to_mel_ragged_impl(p, c, static_cast<const float*>(pcm), window, mel_basis, B, n_max, bounds, normalize, n_mels, log10_kind, ref,
                                  T_out, mel_db_out, gate_out, frame_lengths_out, row_status_out);
}

}  // C ABI
