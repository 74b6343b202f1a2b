// Batched mel -> waveform vocoder on the GPU: dB->amplitude + pseudo-inverse mel projection, fast Griffin-Lim on
// rocFFT batched real transforms, overlap-add inverse STFT, and the clip / trim / normalise / Butterworth tail.
// Replaces the mel->wav half of the reference's NumPy audio library, which is strictly per utterance with Python
// loops over frames (utils/audio/base.py:38-88, :143-169; core/processors.py:81-96).
//
// Layouts: the reference's spectrogram layout is [bins][frames]; internally everything is frame-major
// ([B*T][bins] complex, [B*T][n_fft] real) because that is what a batched 1-D FFT wants (one contiguous transform
// per frame).  The C ABI takes and returns the reference's layout and transposes once on the way in / out.
//
// Per Griffin-Lim iteration (all HBM-bound, fp32 / complex64):
//   C2R (rocFFT, batch B*T)  ->  overlap-add + window-sum normalisation (gather form, frames added in ascending
//   order like the reference)  ->  re-framing * window  ->  R2C (rocFFT)  ->  momentum update / magnitude projection.
#include "../../include/genvox_amd.h"
#include "gvx_kernels.h"

#include <rocfft/rocfft.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

int gl_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return gvx::set_error(code, buf);
}
#define GL_HIP(expr)                                                                                   \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess) return gl_fail(GVX_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define GL_FFT(expr)                                                                          \
    do {                                                                                      \
        rocfft_status _s = (expr);                                                            \
        if (_s != rocfft_status_success) return gl_fail(GVX_ERR_HIP, "%s failed: rocfft status %d", #expr, (int)_s); \
    } while (0)

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

struct FftPair {
    rocfft_plan r2c = nullptr, c2r = nullptr;
    size_t work_bytes = 0;
};

}  // namespace

struct gvx_gl_plan {
    int n_fft, hop, bins;
    float2* tw = nullptr;   // fused 1024-point path: [0,512) e^{-2 pi i m/512}, [512, 512+513) e^{-2 pi i k/1024}
    std::map<long, FftPair> plans;  // keyed by batch count (B*T)
    rocfft_execution_info info = nullptr;
};

namespace {

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

struct GlWs {  // byte offsets
    size_t mag, ang, reb0, reb1, fr, y, wss, amp, fft_work, basis, wss_tail, total;
};

// basis: the mel basis of the wav -> mel calls in rows padded for the GEMM (its size does not depend on the frame count, so it
// has a region of its own: no call with M mels is too short for it).  ragged: room for the per-row tail of the window sum of
// squares behind everything else (the uniform layout is a prefix)
GlWs gl_plan_ws(const gvx_gl_plan* p, int B, int T, int M, size_t fft_work, bool ragged = false) {
    GlWs w{};
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
    w.fft_work = take(fft_work);
    w.basis = take((size_t)(M > 0 ? M : 0) * (size_t)((p->bins + 3) & ~3) * sizeof(float));
    w.wss_tail = ragged ? take((size_t)B * (p->n_fft - p->hop) * sizeof(float)) : 0;
    w.total = off;
    return w;
}

template <typename T>
T* wsp(void* ws, size_t off) { return reinterpret_cast<T*>(reinterpret_cast<char*>(ws) + off); }

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

// ---- ragged batches: row b has T_b = frame_lengths[b] frames (clamped to [0, T], never trusted) and n_b = n_fft + (T_b-1)*hop
// samples inside buffers that keep the strides of the padded T.  Kernels that know about lengths are the RAGGED = true
// instantiation of the uniform kernel's body; RAGGED = false never touches `lens` and compiles to the uniform kernel.
__device__ __forceinline__ int row_frames(const int32_t* __restrict__ lens, int b, int T) {
    const int v = lens[b];
    return v < 0 ? 0 : (v > T ? T : v);
}
__device__ __forceinline__ long row_samples(const int32_t* __restrict__ lens, int b, int n_fft, int hop, long n_cap) {
    const long v = lens[b];
    if (v < 1) return 0;
    const long nb = (long)n_fft + (v - 1) * hop;
    return nb < n_cap ? nb : n_cap;
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

// ---- rows of the ragged wav -> mel front-end (gvx_wav_to_mel_ragged) ------------------------------------------------------
// A PCM row is int16 or float32.  wav_row_plan_kernel turns each row's bounds into rows[b] = {first sample, frames T_b} and its
// peak into a double; every later kernel reads those, so all of them agree on which frames exist.
struct WavRows {
    const int32_t* rows;   // [B][2]: left_b, T_b (0 for a row that has no frame)
    const double* peak;    // [B]: max |sample| over [left_b, right_b), as the divisor of normalize_signal
    int normalize;
};

// normalize_signal (utils/audio/base.py:20-22): float32(double(y) / double(peak)); without it the sample as float32
template <typename PCM>
__device__ __forceinline__ float pcm_sample(PCM v, double peak, bool normalize) {
    return normalize ? (float)((double)v / peak) : (float)v;
}

// xf[b][t][k] = win[k] * y[b][t*hop + k]      (utils/audio/base.py:58-69)
// RAGGED: grid (T, B); row b's frame t starts at sample left_b + t*hop and is read through pcm_sample; frames t >= T_b are zeros
template <bool RAGGED, typename PCM>
__global__ void gl_frame_kernel(const PCM* y, const float* win, float* xf, int n_fft, int hop, int T, long n, WavRows wr) {
    if constexpr (RAGGED) {
        const int b = blockIdx.y, t = blockIdx.x;
        float* o = xf + ((long)b * T + t) * n_fft;
        if (t >= wr.rows[2 * b + 1]) {
            for (int k = threadIdx.x; k < n_fft; k += blockDim.x) o[k] = 0.f;
            return;
        }
        const PCM* yb = y + (long)b * n + wr.rows[2 * b] + (long)t * hop;
        const double peak = wr.peak[b];
        for (int k = threadIdx.x; k < n_fft; k += blockDim.x) o[k] = win[k] * pcm_sample(yb[k], peak, wr.normalize != 0);
        return;
    } else {
    const long bt = blockIdx.x;  // b*T + t
    const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
    const float* yb = y + (long)b * n + (long)t * hop;
    float* o = xf + bt * n_fft;
    if ((n & 3) || (reinterpret_cast<uintptr_t>(y) & 15)) {  // rows not 16-byte aligned: scalar path
        for (int k = threadIdx.x; k < n_fft; k += blockDim.x) o[k] = win[k] * yb[k];
        return;
    }
    for (int k = threadIdx.x * 4; k < n_fft; k += blockDim.x * 4) {
        const float4 w = *reinterpret_cast<const float4*>(win + k);
        const float4 v = *reinterpret_cast<const float4*>(yb + k);  // hop % 4 == 0 and n_fft % 4 == 0 keep this aligned
        *reinterpret_cast<float4*>(o + k) = make_float4(w.x * v.x, w.y * v.y, w.z * v.z, w.w * v.w);
    }
    }
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

// clip spurious samples, trim, peak, normalise to float32, IIR low-pass in float64 (core/processors.py:91-95,
// utils/audio/base.py:20-22, :164-169; scipy.signal.lfilter = direct form II transposed)
// RAGGED: n is the row stride; row b holds n_b = n_fft + (T_b-1)*hop samples (row_samples) and everything - trim at both ends, peak,
// filter, the chunks' warm-up positions - is counted within them, as in a call on that row alone; out is 0 past n_b - 2*trim
template <bool RAGGED>
__global__ void wav_peak_kernel(const float* y, long n, int trim, unsigned int* peak_bits, const int32_t* lens, int n_fft, int hop) {
    const int b = blockIdx.y;
    const long n_out = (RAGGED ? row_samples(lens, b, n_fft, hop, n) : n) - 2L * trim;
    float m = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += (long)gridDim.x * blockDim.x) {
        float v = y[(long)b * n + trim + i];
        if (v > 1.f || v < -1.f) v = 0.f;
        m = fmaxf(m, fabsf(v));
    }
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) atomicMax(peak_bits + b, __float_as_uint(m));  // non-negative floats order like their bit patterns
}

struct IirCoef { double b[8], a[8]; int order; };

template <bool RAGGED>
__global__ void wav_filter_kernel(const float* y, long n, int trim, const unsigned int* peak_bits, IirCoef c, double* out, int B,
                                  const int32_t* lens, int n_fft, int hop) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const long n_stride = n - 2L * trim;
    long n_out = n_stride;
    if (RAGGED) {
        n_out = row_samples(lens, b, n_fft, hop, n) - 2L * trim;
        if (n_out < 0) n_out = 0;
        for (long i = n_out; i < n_stride; ++i) out[(long)b * n_stride + i] = 0.0;
    }
    const float peak = __uint_as_float(peak_bits[b]);
    double z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const float* yb = y + (long)b * n + trim;
    double* ob = out + (long)b * n_stride;
    // the recurrence is strictly sequential per utterance; the loads are not: fetch the next 16 samples while the
    // current 16 go through the filter (one thread = one utterance, a wave = 64 utterances in lock step)
    constexpr int CH = 16;
    float cur[CH], nxt[CH];
#pragma unroll
    for (int k = 0; k < CH; ++k) cur[k] = k < n_out ? yb[k] : 0.f;
    for (long i0 = 0; i0 < n_out; i0 += CH) {
#pragma unroll
        for (int k = 0; k < CH; ++k) nxt[k] = (i0 + CH + k) < n_out ? yb[i0 + CH + k] : 0.f;
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            if (i0 + k < n_out) {
                float v = cur[k];
                if (v > 1.f || v < -1.f) v = 0.f;
                const double x = (double)(v / peak);  // float32 division, then float64 filtering, like the reference
                const double yo = c.b[0] * x + z[0];
#pragma unroll
                for (int q = 1; q < 8; ++q) {
                    if (q <= c.order) z[q - 1] = c.b[q] * x + (q < c.order ? z[q] : 0.0) - c.a[q] * yo;
                }
                ob[i0 + k] = yo;
            }
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) cur[k] = nxt[k];
    }
}

// The same filter, parallel over chunks of every utterance.  The recurrence is linear and stable: a chunk started W samples
// early from a zero state differs from the sequential filter by |M^W| (M = state transition matrix), and the host picks W
// so that this is below 1e-18 - far under a float64 ulp of the output - so the warm-up samples are simply filtered and
// discarded (overlap-discard).  One thread = one chunk; no cross-chunk exchange, no extra buffers; a row's result does
// not depend on the batch it is in.  Reference: scipy.signal.lfilter in butter_lowpass_filter (utils/audio/base.py:164-166).
template <bool RAGGED>
__global__ void wav_filter_chunked_kernel(const float* y, long n, int trim, const unsigned int* peak_bits, IirCoef c, double* out,
                                          int chunk, int warm, int nch, const int32_t* lens, int n_fft, int hop) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int b = blockIdx.y;
    if (k >= nch) return;
    const long n_stride = n - 2L * trim;
    long n_out = n_stride;
    const long i_begin = (long)k * chunk;
    double* ob = out + (long)b * n_stride;
    if (RAGGED) {
        n_out = row_samples(lens, b, n_fft, hop, n) - 2L * trim;
        if (n_out < 0) n_out = 0;
        for (long i = max(i_begin, n_out); i < min(n_stride, i_begin + chunk); ++i) ob[i] = 0.0;   // the chunk's share of the padding
        if (i_begin >= n_out) return;
    }
    const float peak = __uint_as_float(peak_bits[b]);
    const long i_end = min(n_out, i_begin + chunk);
    const long i_start = max(0L, i_begin - warm);
    double z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const float* yb = y + (long)b * n + trim;
    constexpr int CH = 16;
    float cur[CH], nxt[CH];
#pragma unroll
    for (int q = 0; q < CH; ++q) cur[q] = (i_start + q) < i_end ? yb[i_start + q] : 0.f;
    for (long i0 = i_start; i0 < i_end; i0 += CH) {
#pragma unroll
        for (int q = 0; q < CH; ++q) nxt[q] = (i0 + CH + q) < i_end ? yb[i0 + CH + q] : 0.f;
#pragma unroll
        for (int q = 0; q < CH; ++q) {
            if (i0 + q < i_end) {
                float v = cur[q];
                if (v > 1.f || v < -1.f) v = 0.f;
                const double x = (double)(v / peak);
                const double yo = c.b[0] * x + z[0];
#pragma unroll
                for (int r = 1; r < 8; ++r) {
                    if (r <= c.order) z[r - 1] = c.b[r] * x + (r < c.order ? z[r] : 0.0) - c.a[r] * yo;
                }
                if (i0 + q >= i_begin) ob[i0 + q] = yo;
            }
        }
#pragma unroll
        for (int q = 0; q < CH; ++q) cur[q] = nxt[q];
    }
}

// smallest W with max|M^W| < 1e-18 for the filter's state transition matrix (direct form II transposed), or -1 if the
// filter decays too slowly (or not at all) for the overlap-discard scheme
int iir_warmup_length(const IirCoef& c, int cap) {
    const int n = c.order;
    double P[8][8] = {}, M[8][8] = {}, R[8][8];
    for (int q = 1; q <= n; ++q) {
        M[q - 1][0] = -c.a[q];
        if (q < n) M[q - 1][q] = 1.0;
    }
    for (int i = 0; i < n; ++i) P[i][i] = 1.0;
    for (int w = 1; w <= cap; ++w) {
        double mx = 0.0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                double acc = 0.0;
                for (int k = 0; k < n; ++k) acc += P[i][k] * M[k][j];
                R[i][j] = acc;
                mx = std::fmax(mx, std::fabs(acc));
            }
        std::memcpy(P, R, sizeof P);
        if (!(mx < 1e300)) return -1;
        if (mx < 1e-18) return w;
    }
    return -1;
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
constexpr int FN = 512;              // complex points
constexpr int FPAD = FN + FN / 8;    // LDS words (float2) per frame: index i lives at i + (i >> 3)
__device__ __forceinline__ int fpad(int i) { return i + (i >> 3); }
// (Measured: an XOR swizzle of the row instead of the padding removes the last two-way conflicts of the j + 64 r accesses, but
// its addresses no longer fold into the instructions' immediate offsets; the extra VALU work costs more than the conflicts.)

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
template <bool INV> __device__ __forceinline__ float2 rot90(float2 a) {   // a * (-i) forward, a * (+i) inverse
    return INV ? make_float2(-a.y, a.x) : make_float2(a.y, -a.x);
}

template <bool INV>
__device__ __forceinline__ void dft4(float2& a, float2& b, float2& c, float2& d) {
    const float2 t0 = cadd(a, c), t1 = csub(a, c), t2 = cadd(b, d), t3 = rot90<INV>(csub(b, d));
    a = cadd(t0, t2); b = cadd(t1, t3); c = csub(t0, t2); d = csub(t1, t3);
}

template <bool INV>
__device__ __forceinline__ void dft8(float2 v[8]) {
    float2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6], o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
    dft4<INV>(e0, e1, e2, e3);
    dft4<INV>(o0, o1, o2, o3);
    const float h = 0.70710678118654752f;
    // o_k *= w8^k, w8 = e^{-+ i pi/4}
    const float2 w1 = INV ? make_float2(h * (o1.x - o1.y), h * (o1.x + o1.y)) : make_float2(h * (o1.x + o1.y), h * (o1.y - o1.x));
    const float2 w2 = rot90<INV>(o2);
    const float2 w3 = INV ? make_float2(-h * (o3.x + o3.y), h * (o3.x - o3.y)) : make_float2(h * (o3.y - o3.x), -h * (o3.x + o3.y));
    v[0] = cadd(e0, o0); v[4] = csub(e0, o0);
    v[1] = cadd(e1, w1); v[5] = csub(e1, w1);
    v[2] = cadd(e2, w2); v[6] = csub(e2, w2);
    v[3] = cadd(e3, w3); v[7] = csub(e3, w3);
}

// 512-point complex FFT of one frame by one wave.  In: lane j holds x[j + 64 r] in v[r].  Out: lane j holds X[j + 64 r]
// in v[r] (natural order); if to_lds, the result is also left in `buf` (padded indexing) for the caller.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// CTW: per-pass twiddle tables (tw[(r-1)*8 + k] for the second pass, tw[64 + (r-1)*64 + j] for the third: the same values as
// tw[(r k mult) & 511] of the plain table, gathered so that a half wave reads consecutive LDS words)
template <bool INV, bool CTW = false>
__device__ __forceinline__ void fft512_wave(float2 v[8], float2* buf, const float2* __restrict__ tw, int j, bool to_lds) {
#pragma unroll
    for (int stage = 0; stage < 3; ++stage) {
        const int Ns = stage == 0 ? 1 : (stage == 1 ? 8 : 64);
        const int k = j & (Ns - 1);
        if (stage > 0) {
            const int mult = 64 / Ns;   // twiddle w_{Ns*8}^{r k} = w_512^{r k mult}
#pragma unroll
            for (int r = 1; r < 8; ++r) {
                float2 w = CTW ? tw[(stage == 1 ? 0 : 64) + (r - 1) * Ns + k] : tw[(r * k * mult) & (FN - 1)];
                if (INV) w.y = -w.y;
                v[r] = cmul(v[r], w);
            }
        }
        dft8<INV>(v);
        if (stage < 2 || to_lds) {
            const int j0 = (j / Ns) * Ns * 8 + k;
#pragma unroll
            for (int r = 0; r < 8; ++r) buf[fpad(j0 + r * Ns)] = v[r];
        }
        if (stage < 2) {
            // the exchange stays inside this wave's LDS row and a wave's LDS instructions execute in order: a wave-level
            // fence (no instruction, only ordering for the compiler) is all the synchronisation the pass needs
            wave_lds_fence();
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] = buf[fpad(j + 64 * r)];
            wave_lds_fence();
        }
    }
}

constexpr int GLI_FRAMES = 16;                 // frames (waves) per workgroup of the inverse kernel
constexpr int GLI_BLOCKS = GLI_FRAMES - 3;     // hop blocks it completes (n_fft / hop - 1 = 3 halo frames)
constexpr int GLI_TAB_WIN = FN + 520;          // LDS tables of gl_iteration_kernel, in float2: twiddles [FN + 513], pad, window [512]
constexpr int GLI_TAB = GLI_TAB_WIN + 512;

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
            float2 a = S[k], c = S[512 - k];
            if (k == 0) { a.y = 0.f; c.y = 0.f; }          // c2r ignores the imaginary parts of the DC and Nyquist bins
            c.y = -c.y;                                     // conj(S[512 - k])
            const float2 w = tw2[k];                        // e^{-2 pi i k/1024}; need e^{+...}
            const float2 d = csub(a, c);
            const float2 id = make_float2(-d.y, d.x);       // i * d
            v[r] = cadd(cadd(a, c), cmul(id, make_float2(w.x, -w.y)));
        }
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = make_float2(0.f, 0.f);
    }
    fft512_wave<true>(v, buf, tw, j, false);
    // windowed frame (same operation order as gl_ola_kernel: win[k] * (fr[k] * (1/n_fft))) into this wave's LDS row
    float* frow = reinterpret_cast<float*>(buf);   // 1024 floats inside the wave's FPAD*2 floats; all exchanges above are done
    __syncthreads();
    if (valid) {
        const float inv_n = 1.f / 1024.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n2 = 2 * (j + 64 * r);
            const float2 w = *reinterpret_cast<const float2*>(win + n2);
            *reinterpret_cast<float2*>(frow + n2) = make_float2(w.x * (v[r].x * inv_n), w.y * (v[r].y * inv_n));
        }
    }
    __syncthreads();
    // overlap-add of hop blocks h0 .. h0+12 (ascending frame order), divide by the window sum of squares
    const long n = (long)(T + 3) * 256;
    const long n_row = RAGGED ? (long)(Tb + 3) * 256 : n;
    const float* fall = reinterpret_cast<const float*>(fsm);
    for (int idx = tid; idx < GLI_BLOCKS * 256; idx += GLI_FRAMES * 64) {
        const int hb = idx >> 8, q = idx & 255;
        const int h = h0 + hb;
        const long i = (long)h * 256 + q;
        if (i >= n_row) break;
        float sacc = 0.f;
#pragma unroll
        for (int d = 3; d >= 0; --d) {           // frames t = h-3 .. h  ->  waves hb .. hb+3
            const int tt = h - d;
            if (tt >= 0 && tt < Tb) sacc += fall[(long)(hb + 3 - d) * (FPAD * 2) + d * 256 + q];
        }
        const float w = (RAGGED && h >= Tb) ? wss_tail[(long)b * 768 + (h - Tb) * 256 + q] : wss[i];
        y[(long)b * n + i] = w > 1.17549435e-38f ? sacc * __builtin_amdgcn_rcpf(w) : sacc;   // v_rcp_f32: 1 ulp
    }
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
    const long n = (long)(T + 3) * 256;
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
        const float* yb = y_in + (long)b * n + (long)t * 256;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n2 = 2 * (j + 64 * r);
            const float2 x = *reinterpret_cast<const float2*>(yb + n2);
            const float2 w = *reinterpret_cast<const float2*>(win + n2);
            v[r] = make_float2(w.x * x.x, w.y * x.y);
        }
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
            float2 zc = buf[r == 8 ? 0 : (r == 0 && j == 0 ? 0 : a_rev - 72 * r)];
            zc.y = -zc.y;
            const float2 sm = cadd(zk, zc), df = csub(zk, zc);
            const float2 wd = cmul(tw2[k], df);                  // W^k (Z[k] - conj Z[512-k])
            float2 reb = make_float2(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x));   // 0.5*sm - 0.5i*wd
            if ((r == 0 || r == 8) && edge) reb.y = 0.f;         // exactly real for a real signal
            float2 a = reb;
            if (!first) {
                a.x = reb.x - c * pvk.x;
                a.y = reb.y - c * pvk.y;
            }
            // a / (|a| + tiny) * mag with v_sqrt_f32 / v_rcp_f32; the operands are pre-scaled on the rare path where their
            // squares would underflow (|a| < 1e-15), like the hypot behind the reference's abs()
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
            const int k = j + 64 * r;
            const bool dc = r == 0 && j == 0;
            float2 a = S[r];
            float2 cj = dc ? S[8] : buf[a_rev - 72 * r];       // lane 0 holds the Nyquist bin itself
            if (dc) { a.y = 0.f; cj.y = 0.f; }                 // c2r ignores the imaginary parts of the DC and Nyquist bins
            cj.y = -cj.y;                                      // conj(S[512 - k])
            const float2 w = tw2[k];                           // e^{-2 pi i k/1024}; need e^{+...}
            const float2 d = csub(a, cj);
            const float2 id = make_float2(-d.y, d.x);          // i * d
            v[r] = cadd(cadd(a, cj), cmul(id, make_float2(w.x, -w.y)));
        }
        wave_lds_fence();
        fft512_wave<true, true>(v, buf, tw, j, false);
        // windowed frame (same operation order as gl_ola_kernel: win[k] * (fr[k] * (1/n_fft))) into this frame's LDS row, which
        // only this wave touches until the barrier (the FFT's last exchange ended with a fence)
        float* frow = reinterpret_cast<float*>(buf);
        const float inv_n = 1.f / 1024.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n2 = 2 * (j + 64 * r);
            const float2 w = *reinterpret_cast<const float2*>(win + n2);
            *reinterpret_cast<float2*>(frow + n2) = make_float2(w.x * (v[r].x * inv_n), w.y * (v[r].y * inv_n));
        }
    }
    if (!do_inverse) return;
    __syncthreads();
    // overlap-add of hop blocks h0 .. h0+NBL-1 (ascending frame order), divide by the window sum of squares
    const float* fall = reinterpret_cast<const float*>(fsm);
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
            if (tt >= 0 && tt < Tb) sacc += fall[(long)(hb + 3 - d) * (FPAD * 2) + d * 256 + q];
        }
        const float w = (RAGGED && h >= Tb) ? wss_tail[(long)b * 768 + (h - Tb) * 256 + q] : wss[i];
        y_out[(long)b * n + i] = w > 1.17549435e-38f ? sacc * __builtin_amdgcn_rcpf(w) : sacc;
    }
}

constexpr int GLF_FRAMES = 4;   // frames (waves) per workgroup of the forward kernel

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
        const float* yb = y + (long)b * (long)(T + 3) * 256 + (long)t * 256;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n2 = 2 * (j + 64 * r);
            const float2 x = *reinterpret_cast<const float2*>(yb + n2);
            const float2 w = *reinterpret_cast<const float2*>(win + n2);
            v[r] = make_float2(w.x * x.x, w.y * x.y);
        }
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
        const float2 zk = buf[fpad(k & (FN - 1))];
        float2 zc = buf[fpad((512 - k) & (FN - 1))];
        zc.y = -zc.y;
        const float2 sm = cadd(zk, zc), df = csub(zk, zc);
        const float2 wd = cmul(wk[r], df);                   // W^k (Z[k] - conj Z[512-k])
        float2 reb = make_float2(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x));   // 0.5*sm - 0.5i*wd
        if (k == 0 || k == 512) reb.y = 0.f;                 // exactly real for a real signal
        float2 a = reb;
        if (!first) {
            a.x = reb.x - c * pv[r].x;
            a.y = reb.y - c * pv[r].y;
        }
        // a / (|a| + tiny) * mag with v_sqrt_f32 / v_rcp_f32 (1 ulp each) instead of libm hypotf and two IEEE divisions,
        // which together were half of this kernel's vector instructions.  Operands are pre-scaled by a power of two when
        // they are so small that their squares would underflow (hypotf's only advantage here), so tiny bins keep their phase.
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
    long f;
    bool valid;
    float2* buf = fsm + wave * FPAD;
    float2 v[8];
    if constexpr (RAGGED) {
        const int b = blockIdx.y, t = (int)blockIdx.x * GLF_FRAMES + wave;
        if (t >= T) return;
        f = (long)b * T + t;
        if (t >= wr.rows[2 * b + 1]) {
            float* row = mag + f * kp;
            for (int k = j; k < kp; k += 64) row[k] = 0.f;
            return;
        }
        valid = true;
        const PCM* xb = x + (long)b * n_samples + wr.rows[2 * b] + (long)t * 256;
        const double peak = wr.peak[b];
        const bool norm = wr.normalize != 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n2 = 2 * (j + 64 * r);
            const float2 w = *reinterpret_cast<const float2*>(win + n2);
            v[r] = make_float2(w.x * pcm_sample(xb[n2], peak, norm), w.y * pcm_sample(xb[n2 + 1], peak, norm));
        }
    } else {
    f = (long)blockIdx.x * GLF_FRAMES + wave;
    valid = f < frames;
    if (valid) {
        const unsigned fu = (unsigned)f;
        const int b = (int)(fu / (unsigned)T), t = (int)(fu - (unsigned)b * (unsigned)T);
        const float* xb = x + (long)b * n_samples + (long)t * 256;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int n2 = 2 * (j + 64 * r);
            const float2 w = *reinterpret_cast<const float2*>(win + n2);
            v[r] = make_float2(w.x * xb[n2], w.y * xb[n2 + 1]);   // rows need not be 8-byte aligned (n_samples is arbitrary)
        }
    } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] = make_float2(0.f, 0.f);
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
            const float2 zk = buf[fpad(k & (FN - 1))];
            float2 zc = buf[fpad((512 - k) & (FN - 1))];
            zc.y = -zc.y;
            const float2 sm = cadd(zk, zc), df = csub(zk, zc);
            const float2 wd = cmul(tw2[k], df);
            float2 X = make_float2(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x));
            if (k == 0 || k == 512) X.y = 0.f;
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

bool getenv_flag(const char* name) {
    const char* e = std::getenv(name);
    return e && e[0] == '1';
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

inline int blocks_for(long n, int per = 256, int cap = 8192) {
    long b = (n + per - 1) / per;
    return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

// frame-major spectrum -> signal: C2R + overlap-add
// (lens: per-row frame counts of a ragged batch, or null - every frame is transformed either way, the overlap-add skips the padded ones)
int istft_frames(gvx_gl_plan* p, FftPair* fp, float2* spec_t, const float* win, int B, int T, void* ws, const GlWs& w, hipStream_t s,
                 const int32_t* lens = nullptr) {
    const long n = (long)p->n_fft + (long)(T - 1) * p->hop;
    int rc = run_fft(p, fp->c2r, spec_t, wsp<float>(ws, w.fr), wsp<char>(ws, w.fft_work), fp->work_bytes, s);
    if (rc != GVX_OK) return rc;
    const dim3 grid((unsigned)((n + 255) / 256), B);
    if (lens)
        gl_ola_kernel<true><<<grid, 256, 0, s>>>(wsp<float>(ws, w.fr), win, wsp<float>(ws, w.wss), wsp<float>(ws, w.y), p->n_fft, p->hop, T, n,
                                                 lens, wsp<float>(ws, w.wss_tail));
    else
        gl_ola_kernel<false><<<grid, 256, 0, s>>>(wsp<float>(ws, w.fr), win, wsp<float>(ws, w.wss), wsp<float>(ws, w.y), p->n_fft, p->hop, T, n,
                                                  nullptr, nullptr);
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

int check_gl(const gvx_gl_plan* p, int B, int T, const void* ws, size_t ws_bytes, size_t need) {
    if (!p) return gl_fail(GVX_ERR_INVALID_ARG, "null plan");
    if (B < 1 || T < 1) return gl_fail(GVX_ERR_INVALID_ARG, "B and T must be >= 1");
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 255)) return gl_fail(GVX_ERR_WORKSPACE, "workspace must be non-null and 256-byte aligned");
    if (ws_bytes < need) return gl_fail(GVX_ERR_WORKSPACE, "workspace too small: %zu < %zu bytes", ws_bytes, need);
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
    if (!p || B < 1 || T < 1) return 0;
    FftPair* fp = nullptr;
    if (get_plans(p, (long)B * T, &fp) != GVX_OK) return 0;
    return gl_plan_ws(p, B, T, n_mels, fp->work_bytes).total;
}

int gvx_stft(gvx_gl_plan* p, const float* signal, const float* window, int B, long n_samples, float* spec_out, void* ws, size_t ws_bytes,
             void* stream) {
    if (!p || !signal || !window || !spec_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_samples < p->n_fft) return gl_fail(GVX_ERR_INVALID_ARG, "signal shorter than one frame");
    const int T = (int)((n_samples - p->n_fft) / p->hop + 1);
    FftPair* fp = nullptr;
    int rc = get_plans(p, (long)B * T, &fp);
    if (rc != GVX_OK) return rc;
    const GlWs w = gl_plan_ws(p, B, T, 0, fp->work_bytes);
    rc = check_gl(p, B, T, ws, ws_bytes, w.total);
    if (rc != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    gl_frame_kernel<false, float><<<dim3((unsigned)((long)B * T)), 256, 0, s>>>(signal, window, wsp<float>(ws, w.fr), p->n_fft, p->hop, T, n_samples, WavRows{});
    GL_HIP(hipGetLastError());
    rc = run_fft(p, fp->r2c, wsp<float>(ws, w.fr), wsp<float2>(ws, w.reb0), wsp<char>(ws, w.fft_work), fp->work_bytes, s);
    if (rc != GVX_OK) return rc;
    GL_HIP(launch_transpose<float2>(wsp<float2>(ws, w.reb0), reinterpret_cast<float2*>(spec_out), B, T, p->bins, s));
    return GVX_OK;
}

int gvx_istft(gvx_gl_plan* p, const float* spec, const float* window, int B, int T, float* signal_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !spec || !window || !signal_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    FftPair* fp = nullptr;
    int rc = get_plans(p, (long)B * T, &fp);
    if (rc != GVX_OK) return rc;
    const GlWs w = gl_plan_ws(p, B, T, 0, fp->work_bytes);
    rc = check_gl(p, B, T, ws, ws_bytes, w.total);
    if (rc != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long n = (long)p->n_fft + (long)(T - 1) * p->hop;
    GL_HIP(launch_transpose<float2>(reinterpret_cast<const float2*>(spec), wsp<float2>(ws, w.ang), B, p->bins, T, s));
    wss_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(window, wsp<float>(ws, w.wss), p->n_fft, p->hop, T, n);
    GL_HIP(hipGetLastError());
    rc = istft_frames(p, fp, wsp<float2>(ws, w.ang), window, B, T, ws, w, s);
    if (rc != GVX_OK) return rc;
    GL_HIP(hipMemcpyAsync(signal_out, wsp<float>(ws, w.y), (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return GVX_OK;
}

int gvx_mel_to_magnitude(gvx_gl_plan* p, const float* mel_db, const float* inv_basis, int B, int n_mels, int T, int log10_kind, float ref,
                         float* mag_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !mel_db || !inv_basis || !mag_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_mels & 3) return gl_fail(GVX_ERR_UNSUPPORTED, "n_mels must be a multiple of 4");
    FftPair* fp = nullptr;
    int rc = get_plans(p, (long)B * T, &fp);
    if (rc != GVX_OK) return rc;
    const GlWs w = gl_plan_ws(p, B, T, n_mels, fp->work_bytes);
    rc = check_gl(p, B, T, ws, ws_bytes, w.total);
    if (rc != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const float refc = ref > 1e-5f ? ref : 1e-5f;
    const float log_ref = log10_kind ? log10f(refc) : logf(refc);
    db_to_amp_transpose_kernel<<<dim3((T + 31) / 32, (n_mels + 31) / 32, B), dim3(32, 8), 0, s>>>(mel_db, wsp<float>(ws, w.amp), n_mels, T,
                                                                                                 log10_kind, log_ref);
    GL_HIP(hipGetLastError());
    // mel2fft (utils/audio/base.py:143-145): mag_t[(b,t)][bin] = sum_m inv_basis[bin][m] * amp_t[(b,t)][m]
    gvx::GemmParams g{};
    g.A = wsp<float>(ws, w.amp); g.amap = gvx::RowMap{B * T, 0, (long)n_mels};
    g.W = inv_basis; g.ldw = n_mels;
    g.C = wsp<float>(ws, w.mag); g.cmap = gvx::RowMap{B * T, 0, (long)p->bins};
    g.M = B * T; g.N = p->bins; g.K = n_mels; g.act = gvx::ACT_NONE;
    GL_HIP(gvx::launch_gemm(g, s));
    GL_HIP(launch_transpose<float>(wsp<float>(ws, w.mag), mag_out, B, T, p->bins, s));
    return GVX_OK;
}

}  // extern "C"

namespace {

// gvx_griffin_lim (lens == nullptr: every launch is the uniform one, unchanged) and gvx_griffin_lim_ragged
int griffin_lim_impl(gvx_gl_plan* p, const float* mag, const float* window, int B, int T, const int32_t* lens, int n_iter, float momentum,
                     float* phase_out, float* wav_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !mag || !window) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_iter < 0) return gl_fail(GVX_ERR_INVALID_ARG, "n_iter must be >= 0");
    if (B < 1 || T < 1) return gl_fail(GVX_ERR_INVALID_ARG, "B and T must be >= 1");
    FftPair* fp = nullptr;
    int rc = get_plans(p, (long)B * T, &fp);
    if (rc != GVX_OK) return rc;
    const GlWs w = gl_plan_ws(p, B, T, 0, fp->work_bytes, lens != nullptr);
    rc = check_gl(p, B, T, ws, ws_bytes, w.total);
    if (rc != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const float* tail = lens ? wsp<float>(ws, w.wss_tail) : nullptr;
    if (lens && p->n_fft > p->hop) {
        wss_tail_kernel<<<dim3((unsigned)((p->n_fft - p->hop + 255) / 256), B), 256, 0, s>>>(window, lens, wsp<float>(ws, w.wss_tail), p->n_fft,
                                                                                           p->hop, T);
        GL_HIP(hipGetLastError());
    }
    const long n = (long)p->n_fft + (long)(T - 1) * p->hop;
    const long nbin = (long)B * T * p->bins;
    float* mag_t = wsp<float>(ws, w.mag);
    float2* ang = wsp<float2>(ws, w.ang);
    float2* reb[2] = {wsp<float2>(ws, w.reb0), wsp<float2>(ws, w.reb1)};
    GL_HIP(launch_transpose<float>(mag, mag_t, B, p->bins, T, s));
    wss_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(window, wsp<float>(ws, w.wss), p->n_fft, p->hop, T, n);
    GL_HIP(hipGetLastError());
    gl_init_kernel<<<blocks_for(nbin), 256, 0, s>>>(mag_t, ang, nbin);
    GL_HIP(hipGetLastError());
    const float c = momentum / (1.f + momentum);
    const bool fused = p->tw != nullptr && !getenv_flag("GVX_GL_ROCFFT");
    auto inverse_ola = [&](const float2* spec) -> int {   // y = istft(spec), fused path
        const dim3 grid((unsigned)((T + 3 + GLI_BLOCKS - 1) / GLI_BLOCKS), B);
        if (lens)
            gl_inverse_ola_kernel<true><<<grid, GLI_FRAMES * 64, GLI_FRAMES * FPAD * sizeof(float2), s>>>(
                spec, window, wsp<float>(ws, w.wss), p->tw, wsp<float>(ws, w.y), T, lens, tail);
        else
            gl_inverse_ola_kernel<false><<<grid, GLI_FRAMES * 64, GLI_FRAMES * FPAD * sizeof(float2), s>>>(
                spec, window, wsp<float>(ws, w.wss), p->tw, wsp<float>(ws, w.y), T, nullptr, nullptr);
        GL_HIP(hipGetLastError());
        return GVX_OK;
    };
    // (a ragged call always takes the one-launch iteration: the two-launch A/B variant walks all B*T frames)
    if (fused && n_iter > 0 && (lens || !getenv_flag("GVX_GL_TWO_KERNELS"))) {
        // one launch per iteration: signal -> rebuilt -> update -> new spectrum -> its signal (gl_iteration_kernel); the signal
        // and tprev ping-pong between two buffers each (the framed-signal region of the rocFFT pipeline serves as the second y)
        float* ybuf[2] = {wsp<float>(ws, w.y), wsp<float>(ws, w.fr)};
        rc = inverse_ola(ang);                                  // signal of the initial angles
        if (rc != GVX_OK) return rc;
        // two frames per wave (29 hop blocks per workgroup, 147 KB of LDS) unless the sequence is short
        const bool two = T + 3 > GLI_BLOCKS && !getenv_flag("GVX_GL_ONE_FRAME");
        const int nbl = two ? 2 * GLI_FRAMES - 3 : GLI_BLOCKS;
        const dim3 grid((unsigned)((T + 3 + nbl - 1) / nbl), B);
        for (int it = 0; it < n_iter; ++it) {
            const bool last = it == n_iter - 1;
            auto launch = [&](auto* kernel, size_t lds_bytes) {
                kernel<<<grid, GLI_FRAMES * 64, lds_bytes, s>>>(ybuf[it & 1], ybuf[(it + 1) & 1], window, wsp<float>(ws, w.wss), p->tw, mag_t,
                                                                reb[it & 1], reb[(it + 1) & 1], last ? ang : nullptr, c, it == 0, !last, T,
                                                                lens, tail);
            };
            if (two) {
                const size_t lds_bytes = (2 * GLI_FRAMES * FPAD + GLI_TAB) * sizeof(float2);
                if (lens) launch(gl_iteration_kernel<2, true>, lds_bytes); else launch(gl_iteration_kernel<2, false>, lds_bytes);
            } else {
                const size_t lds_bytes = (GLI_FRAMES * FPAD + GLI_TAB) * sizeof(float2);
                if (lens) launch(gl_iteration_kernel<1, true>, lds_bytes); else launch(gl_iteration_kernel<1, false>, lds_bytes);
            }
            GL_HIP(hipGetLastError());
        }
    } else
    for (int it = 0; fused && it < n_iter; ++it) {              // GVX_GL_TWO_KERNELS=1: the two-launch iteration (A/B runs)
        rc = inverse_ola(ang);                                  // inverse = istft(angles)
        if (rc != GVX_OK) return rc;
        const long frames = (long)B * T;                        // rebuilt = stft(inverse); momentum update; tprev = rebuilt
        gl_forward_update_kernel<<<dim3((unsigned)((frames + GLF_FRAMES - 1) / GLF_FRAMES)), GLF_FRAMES * 64, 0, s>>>(
            wsp<float>(ws, w.y), window, p->tw, mag_t, reb[0], ang, c, it == 0, T, frames);
        GL_HIP(hipGetLastError());
    }
    for (int it = 0; !fused && it < n_iter; ++it) {
        rc = istft_frames(p, fp, ang, window, B, T, ws, w, s, lens);  // inverse = istft(angles)
        if (rc != GVX_OK) return rc;
        gl_frame_kernel<false, float><<<dim3((unsigned)((long)B * T)), 256, 0, s>>>(wsp<float>(ws, w.y), window, wsp<float>(ws, w.fr), p->n_fft, p->hop, T, n, WavRows{});
        GL_HIP(hipGetLastError());
        float2* cur = reb[it & 1];
        rc = run_fft(p, fp->r2c, wsp<float>(ws, w.fr), cur, wsp<char>(ws, w.fft_work), fp->work_bytes, s);  // rebuilt = stft(inverse)
        if (rc != GVX_OK) return rc;
        gl_update_kernel<<<blocks_for(nbin), 256, 0, s>>>(cur, reb[(it + 1) & 1], mag_t, ang, c, it == 0, nbin);
        GL_HIP(hipGetLastError());
    }
    // phase = angle(angles); final spectrum = mag * exp(i phase) (not `angles` itself: they differ where mag < 0)
    float2* spec_t = reb[1];
    float* phase_t = wsp<float>(ws, w.fr);   // frames * n_fft floats >= frames * bins
    if (lens)
        gl_final_kernel<true><<<dim3(blocks_for((long)T * p->bins, 256, 1024), B), 256, 0, s>>>(
            ang, mag_t, wav_out ? spec_t : nullptr, phase_out ? phase_t : nullptr, (long)T * p->bins, p->bins, T, lens);
    else
        gl_final_kernel<false><<<blocks_for(nbin), 256, 0, s>>>(ang, mag_t, wav_out ? spec_t : nullptr, phase_out ? phase_t : nullptr, nbin,
                                                                p->bins, T, nullptr);
    GL_HIP(hipGetLastError());
    if (phase_out) GL_HIP(launch_transpose<float>(phase_t, phase_out, B, T, p->bins, s));
    if (wav_out) {
        rc = fused ? inverse_ola(spec_t) : istft_frames(p, fp, spec_t, window, B, T, ws, w, s, lens);
        if (rc != GVX_OK) return rc;
        if (lens) {   // the signal buffer is valid up to each row's n_b only: zeros behind it in the result
            copy_rows_ragged_kernel<<<dim3(blocks_for(n, 256, 1024), B), 256, 0, s>>>(wsp<float>(ws, w.y), wav_out, n, p->n_fft, p->hop, lens);
            GL_HIP(hipGetLastError());
        } else {
            GL_HIP(hipMemcpyAsync(wav_out, wsp<float>(ws, w.y), (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
    }
    return GVX_OK;
}

// shared by gvx_wav_finalize (lens == nullptr) and gvx_wav_finalize_ragged
int wav_finalize_impl(const float* wav, int B, long n_samples, const int32_t* lens, int n_fft, int hop, int trim, const double* b_coef,
                      const double* a_coef, int order, double* out, unsigned int* scratch_B, void* stream) {
    if (!wav || !b_coef || !a_coef || !out || !scratch_B) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (order < 1 || order > 7) return gl_fail(GVX_ERR_UNSUPPORTED, "filter order %d not in [1, 7]", order);
    if (n_samples <= 2L * trim) return gl_fail(GVX_ERR_INVALID_ARG, "signal shorter than the trim");
    hipStream_t s = (hipStream_t)stream;
    IirCoef c{};
    c.order = order;
    for (int k = 0; k <= order; ++k) { c.b[k] = b_coef[k] / a_coef[0]; c.a[k] = a_coef[k] / a_coef[0]; }
    GL_HIP(hipMemsetAsync(scratch_B, 0, (size_t)B * sizeof(unsigned int), s));
    if (lens)
        wav_peak_kernel<true><<<dim3(64, B), 256, 0, s>>>(wav, n_samples, trim, scratch_B, lens, n_fft, hop);
    else
        wav_peak_kernel<false><<<dim3(64, B), 256, 0, s>>>(wav, n_samples, trim, scratch_B, nullptr, 0, 0);
    GL_HIP(hipGetLastError());
    const int warm = iir_warmup_length(c, 4096);
    if (warm > 0) {
        int chunk = 1024;
        while (chunk < 8 * warm) chunk *= 2;   // warm-up work <= 1/8 of the total
        const long n_out = n_samples - 2L * trim;
        const int nch = (int)((n_out + chunk - 1) / chunk);
        const dim3 grid((nch + 63) / 64, B);
        if (lens)
            wav_filter_chunked_kernel<true><<<grid, 64, 0, s>>>(wav, n_samples, trim, scratch_B, c, out, chunk, warm, nch, lens, n_fft, hop);
        else
            wav_filter_chunked_kernel<false><<<grid, 64, 0, s>>>(wav, n_samples, trim, scratch_B, c, out, chunk, warm, nch, nullptr, 0, 0);
    } else if (lens) {                          // slowly decaying filter: sequential
        wav_filter_kernel<true><<<(B + 63) / 64, 64, 0, s>>>(wav, n_samples, trim, scratch_B, c, out, B, lens, n_fft, hop);
    } else {
        wav_filter_kernel<false><<<(B + 63) / 64, 64, 0, s>>>(wav, n_samples, trim, scratch_B, c, out, B, nullptr, 0, 0);
    }
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

}  // namespace

extern "C" {

int gvx_griffin_lim(gvx_gl_plan* p, const float* mag, const float* window, int B, int T, int n_iter, float momentum, float* phase_out,
                    float* wav_out, void* ws, size_t ws_bytes, void* stream) {
    return griffin_lim_impl(p, mag, window, B, T, nullptr, n_iter, momentum, phase_out, wav_out, ws, ws_bytes, stream);
}

size_t gvx_gl_workspace_bytes_ragged(gvx_gl_plan* p, int B, int T, int n_mels) {
    if (!p || B < 1 || T < 1) return 0;
    FftPair* fp = nullptr;
    if (get_plans(p, (long)B * T, &fp) != GVX_OK) return 0;
    return gl_plan_ws(p, B, T, n_mels, fp->work_bytes, true).total;
}

int gvx_griffin_lim_ragged(gvx_gl_plan* p, const float* mag, const float* window, int B, int T, const int32_t* frame_lengths, int n_iter,
                           float momentum, float* phase_out, float* wav_out, void* ws, size_t ws_bytes, void* stream) {
    if (!frame_lengths) return gl_fail(GVX_ERR_INVALID_ARG, "null frame_lengths (gvx_griffin_lim is the call for rows of one length)");
    return griffin_lim_impl(p, mag, window, B, T, frame_lengths, n_iter, momentum, phase_out, wav_out, ws, ws_bytes, stream);
}

int gvx_wav_finalize_ragged(const float* wav, int B, long n_samples, const int32_t* frame_lengths, int n_fft, int hop, int trim,
                            const double* b_coef, const double* a_coef, int order, double* out, unsigned int* scratch_B, void* stream) {
    if (!frame_lengths) return gl_fail(GVX_ERR_INVALID_ARG, "null frame_lengths (gvx_wav_finalize is the call for rows of one length)");
    if (B < 1 || n_fft < 1 || hop < 1 || trim < 0) return gl_fail(GVX_ERR_INVALID_ARG, "B, n_fft, hop must be >= 1 and trim >= 0");
    return wav_finalize_impl(wav, B, n_samples, frame_lengths, n_fft, hop, trim, b_coef, a_coef, order, out, scratch_B, stream);
}

int gvx_wav_finalize(const float* wav, int B, long n_samples, int trim, const double* b_coef, const double* a_coef, int order,
                     double* out, unsigned int* scratch_B, void* stream) {
    return wav_finalize_impl(wav, B, n_samples, nullptr, 0, 0, trim, b_coef, a_coef, order, out, scratch_B, stream);
}

int gvx_wav_to_mel(gvx_gl_plan* p, const float* signal, const float* window, const float* mel_basis, int B, long n_samples, int n_mels,
                   int log10_kind, float ref, float* mel_db_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !signal || !window || !mel_basis || !mel_db_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    if (n_samples < p->n_fft) return gl_fail(GVX_ERR_INVALID_ARG, "signal shorter than one frame");
    if (n_mels < 1) return gl_fail(GVX_ERR_INVALID_ARG, "n_mels must be >= 1");
    const int T = (int)((n_samples - p->n_fft) / p->hop + 1);
    FftPair* fp = nullptr;
    int rc = get_plans(p, (long)B * T, &fp);
    if (rc != GVX_OK) return rc;
    const GlWs w = gl_plan_ws(p, B, T, n_mels, fp->work_bytes);
    rc = check_gl(p, B, T, ws, ws_bytes, w.total);
    if (rc != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const long frames = (long)B * T;
    const int kp = (p->bins + 3) & ~3;                     // GEMM K must be a multiple of 4: 513 -> 516, zero padded
    // workspace reuse: fr = framed signal, reb0 = spectrum, ang = padded magnitudes (kp floats per frame inside bins float2: kp <= 2 bins
    // for every n_fft), amp = mel amplitudes; the padded basis has its own region
    float* mag_p = wsp<float>(ws, w.ang);
    float* basis_p = wsp<float>(ws, w.basis);
    if (p->tw && !getenv_flag("GVX_GL_ROCFFT")) {   // n_fft 1024 / hop 256: framing + window + FFT + magnitude in one kernel
        stft_magnitude_kernel<false, float><<<dim3((unsigned)((frames + GLF_FRAMES - 1) / GLF_FRAMES)), GLF_FRAMES * 64, 0, s>>>(
            signal, n_samples, window, p->tw, mag_p, kp, T, frames, WavRows{});
        GL_HIP(hipGetLastError());
    } else {
        gl_frame_kernel<false, float><<<dim3((unsigned)frames), 256, 0, s>>>(signal, window, wsp<float>(ws, w.fr), p->n_fft, p->hop, T, n_samples, WavRows{});
        GL_HIP(hipGetLastError());
        rc = run_fft(p, fp->r2c, wsp<float>(ws, w.fr), wsp<float2>(ws, w.reb0), wsp<char>(ws, w.fft_work), fp->work_bytes, s);
        if (rc != GVX_OK) return rc;
        magnitude_kernel<<<blocks_for(frames * kp), 256, 0, s>>>(wsp<float2>(ws, w.reb0), mag_p, p->bins, kp, frames);
        GL_HIP(hipGetLastError());
    }
    pad_rows_kernel<<<blocks_for((long)n_mels * kp), 256, 0, s>>>(mel_basis, basis_p, n_mels, p->bins, kp);
    GL_HIP(hipGetLastError());
    // fft2mel (utils/audio/base.py:139-141): mel_t[(b,t)][m] = sum_k basis[m][k] * |S|[(b,t)][k]
    gvx::GemmParams g{};
    g.A = mag_p; g.amap = gvx::RowMap{(int)frames, 0, (long)kp};
    g.W = basis_p; g.ldw = kp;
    g.C = wsp<float>(ws, w.amp); g.cmap = gvx::RowMap{(int)frames, 0, (long)n_mels};
    g.M = (int)frames; g.N = n_mels; g.K = kp; g.act = gvx::ACT_NONE;
    GL_HIP(gvx::launch_gemm(g, s));
    const float refc = ref > 1e-5f ? ref : 1e-5f;
    const float log_ref = log10_kind ? log10f(refc) : logf(refc);
    amp_to_db_transpose_kernel<false><<<dim3((n_mels + 31) / 32, (T + 31) / 32, B), dim3(32, 8), 0, s>>>(wsp<float>(ws, w.amp), mel_db_out, n_mels,
                                                                                                        T, log10_kind, log_ref, nullptr, nullptr);
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

}  // extern "C"

// ---- ragged wav -> mel: PCM rows of different lengths, trimmed and normalised per row, one launch set per batch ------------------
namespace {

struct WavWs {   // the uniform layout of T frames per row (the padded mel basis included), then the per-row words
    GlWs g;
    size_t rows, peak, peak_bits, total;
};

WavWs wav_plan_ws(const gvx_gl_plan* p, int B, int T, int M, size_t fft_work) {
    WavWs w{};
    w.g = gl_plan_ws(p, B, T, M, fft_work);
    size_t off = w.g.total;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    w.rows = take((size_t)B * 2 * sizeof(int32_t));
    w.peak = take((size_t)B * sizeof(double));
    w.peak_bits = take((size_t)B * sizeof(unsigned int));
    w.total = off;
    return w;
}

inline bool wav_fused(const gvx_gl_plan* p) { return p->tw != nullptr && !getenv_flag("GVX_GL_ROCFFT"); }

// the fused n_fft 1024 / hop 256 path needs no rocFFT plan (and so no plan per batch size)
int wav_fft_plans(gvx_gl_plan* p, int B, int T, FftPair** fp) {
    *fp = nullptr;
    return wav_fused(p) ? GVX_OK : get_plans(p, (long)B * T, fp);
}

template <typename PCM>
int wav_trim_bounds_impl(const PCM* pcm, int B, long n_max, const int32_t* sample_lengths, int chunk, double thr, int32_t* bounds_out,
                         hipStream_t s) {
    wav_trim_bounds_kernel<PCM><<<dim3((unsigned)B), 256, 0, s>>>(pcm, n_max, sample_lengths, chunk, thr, bounds_out);
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

template <typename PCM>
int wav_to_mel_ragged_impl(gvx_gl_plan* p, FftPair* fp, const PCM* pcm, const float* window, const float* mel_basis, int B, long n_max,
                           const int32_t* bounds, int normalize, int n_mels, int log10_kind, float ref, int T, float* mel_db_out,
                           float* gate_out, int32_t* frame_lengths_out, int32_t* row_status_out, void* ws, const WavWs& w, hipStream_t s) {
    const long frames = (long)B * T;
    const int kp = (p->bins + 3) & ~3;
    unsigned int* peak_bits = wsp<unsigned int>(ws, w.peak_bits);
    int32_t* rows = wsp<int32_t>(ws, w.rows);
    GL_HIP(hipMemsetAsync(peak_bits, 0, (size_t)B * sizeof(unsigned int), s));
    wav_peak_bounds_kernel<PCM><<<dim3(64, B), 256, 0, s>>>(pcm, n_max, bounds, peak_bits);
    GL_HIP(hipGetLastError());
    wav_row_plan_kernel<PCM><<<(B + 63) / 64, 64, 0, s>>>(bounds, peak_bits, n_max, p->n_fft, p->hop, T, B, rows, wsp<double>(ws, w.peak),
                                                         frame_lengths_out, row_status_out);
    GL_HIP(hipGetLastError());
    const WavRows wr{rows, wsp<double>(ws, w.peak), normalize};
    // workspace reuse as in gvx_wav_to_mel: fr = framed signal, reb0 = spectrum, ang = padded magnitudes, amp = mel amplitudes
    float* mag_p = wsp<float>(ws, w.g.ang);
    float* basis_p = wsp<float>(ws, w.g.basis);
    if (wav_fused(p)) {
        stft_magnitude_kernel<true, PCM><<<dim3((unsigned)((T + GLF_FRAMES - 1) / GLF_FRAMES), B), GLF_FRAMES * 64, 0, s>>>(
            pcm, n_max, window, p->tw, mag_p, kp, T, frames, wr);
        GL_HIP(hipGetLastError());
    } else {
        gl_frame_kernel<true, PCM><<<dim3((unsigned)T, B), 256, 0, s>>>(pcm, window, wsp<float>(ws, w.g.fr), p->n_fft, p->hop, T, n_max, wr);
        GL_HIP(hipGetLastError());
        const int rc = run_fft(p, fp->r2c, wsp<float>(ws, w.g.fr), wsp<float2>(ws, w.g.reb0), wsp<char>(ws, w.g.fft_work), fp->work_bytes, s);
        if (rc != GVX_OK) return rc;
        magnitude_kernel<<<blocks_for(frames * kp), 256, 0, s>>>(wsp<float2>(ws, w.g.reb0), mag_p, p->bins, kp, frames);
        GL_HIP(hipGetLastError());
    }
    pad_rows_kernel<<<blocks_for((long)n_mels * kp), 256, 0, s>>>(mel_basis, basis_p, n_mels, p->bins, kp);
    GL_HIP(hipGetLastError());
    gvx::GemmParams g{};   // fft2mel over every padded frame: the rows of frames that do not exist are zeros
    g.A = mag_p; g.amap = gvx::RowMap{(int)frames, 0, (long)kp};
    g.W = basis_p; g.ldw = kp;
    g.C = wsp<float>(ws, w.g.amp); g.cmap = gvx::RowMap{(int)frames, 0, (long)n_mels};
    g.M = (int)frames; g.N = n_mels; g.K = kp; g.act = gvx::ACT_NONE;
    GL_HIP(gvx::launch_gemm(g, s));
    const float refc = ref > 1e-5f ? ref : 1e-5f;
    const float log_ref = log10_kind ? log10f(refc) : logf(refc);
    amp_to_db_transpose_kernel<true><<<dim3((n_mels + 31) / 32, (T + 31) / 32, B), dim3(32, 8), 0, s>>>(wsp<float>(ws, w.g.amp), mel_db_out, n_mels,
                                                                                                       T, log10_kind, log_ref, rows, gate_out);
    GL_HIP(hipGetLastError());
    return GVX_OK;
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

size_t gvx_wav_to_mel_ragged_workspace_bytes(gvx_gl_plan* p, int B, long n_max, int n_mels) {
    if (!p || B < 1 || n_max < 1 || n_mels < 1) return 0;
    const int T = wav_frames_of(p, n_max);
    FftPair* fp = nullptr;
    if (wav_fft_plans(p, B, T, &fp) != GVX_OK) return 0;
    return wav_plan_ws(p, B, T, n_mels, fp ? fp->work_bytes : 0).total;
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
        return wav_trim_bounds_impl(static_cast<const int16_t*>(pcm), B, n_max, sample_lengths, chunk, 32767.0 * 32767.0 * rel, bounds_out, s);
    return wav_trim_bounds_impl(static_cast<const float*>(pcm), B, n_max, sample_lengths, chunk, rel, bounds_out, s);
}

int gvx_wav_to_mel_ragged(gvx_gl_plan* p, const void* pcm, int pcm_kind, const float* window, const float* mel_basis, int B, long n_max,
                          const int32_t* bounds, int normalize, int n_mels, int log10_kind, float ref, int T_out, float* mel_db_out,
                          float* gate_out, int32_t* frame_lengths_out, int32_t* row_status_out, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !window || !mel_basis || !bounds || !mel_db_out || !frame_lengths_out || !row_status_out) return gl_fail(GVX_ERR_INVALID_ARG, "null argument");
    int rc = check_pcm(pcm, pcm_kind, B, n_max);
    if (rc != GVX_OK) return rc;
    if (n_mels < 1 || T_out < 1) return gl_fail(GVX_ERR_INVALID_ARG, "n_mels and T_out must be >= 1");
    if ((long)B * T_out > 0x7fffffffL / ((p->bins + 3) & ~3)) return gl_fail(GVX_ERR_UNSUPPORTED, "%d x %d frames are too many for one call", B, T_out);
    FftPair* fp = nullptr;
    rc = wav_fft_plans(p, B, T_out, &fp);
    if (rc != GVX_OK) return rc;
    const WavWs w = wav_plan_ws(p, B, T_out, n_mels, fp ? fp->work_bytes : 0);
    rc = check_gl(p, B, T_out, ws, ws_bytes, w.total);
    if (rc != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (pcm_kind == GVX_PCM_INT16)
        return wav_to_mel_ragged_impl(p, fp, static_cast<const int16_t*>(pcm), window, mel_basis, B, n_max, bounds, normalize, n_mels, log10_kind, ref,
                                      T_out, mel_db_out, gate_out, frame_lengths_out, row_status_out, ws, w, s);
    return wav_to_mel_ragged_impl(p, fp, static_cast<const float*>(pcm), window, mel_basis, B, n_max, bounds, normalize, n_mels, log10_kind, ref,
                                  T_out, mel_db_out, gate_out, frame_lengths_out, row_status_out, ws, w, s);
}

}  // extern "C"
