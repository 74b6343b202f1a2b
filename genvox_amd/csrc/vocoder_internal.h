// Internal to the vocoder sources (griffinlim.hip: mel -> wav, wav_finalize.hip: its clip / trim / normalise / Butterworth tail,
// wav_to_mel.hip: wav -> mel); not installed.  The plan handle, the workspace layout, the opening every call shares, the choice of
// the Griffin-Lim path, and the device code more than one source uses.
#pragma once
#include "../../include/genvox_amd.h"
#include "gvx_kernels.h"

#include <rocfft/rocfft.h>

#include <cstdlib>
#include <map>
#include <type_traits>

namespace gvx { namespace voc {

struct FftPair {
    rocfft_plan r2c = nullptr, c2r = nullptr;
    size_t work_bytes = 0;
};

}}  // namespace gvx::voc

struct gvx_gl_plan {
    int n_fft, hop, bins;
    float2* tw = nullptr;   // fused 1024-point path: [0,512) e^{-2 pi i m/512}, [512, 512+513) e^{-2 pi i k/1024}
    std::map<long, gvx::voc::FftPair> plans;  // keyed by batch count (B*T)
    rocfft_execution_info info = nullptr;
};

namespace gvx { namespace voc {

int gl_fail(int code, const char* fmt, ...);   // sets gvx_last_error() of this thread, returns `code`
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

inline bool getenv_flag(const char* name) {
    const char* e = std::getenv(name);
    return e && e[0] == '1';
}

inline int blocks_for(long n, int per = 256, int cap = 8192) {
    long b = (n + per - 1) / per;
    return (int)(b < cap ? (b < 1 ? 1 : b) : cap);
}

int get_plans(gvx_gl_plan* p, long batch, FftPair** out);   // the rocFFT plan pair of `batch` transforms, created on first use
int run_fft(gvx_gl_plan* p, rocfft_plan plan, void* in, void* out, void* work, size_t work_bytes, hipStream_t s);

// Which Griffin-Lim runs.  n_fft 1024 / hop 256 (the plan has twiddle tables) runs in LDS: one launch per iteration, two frames
// per wave or - short sequences, GVX_GL_ONE_FRAME=1 - one; GVX_GL_TWO_KERNELS=1 is the two-launch iteration of A/B runs.  Every
// other size, and GVX_GL_ROCFFT=1, takes the rocFFT pipeline.  The flags are read at every call.
enum class GlPath { one_launch_two_frames, one_launch_one_frame, two_launch, rocfft };
GlPath gl_path(const gvx_gl_plan* p, const int32_t* lens, int n_iter, int T);
inline bool gl_fused(const gvx_gl_plan* p) { return gl_path(p, nullptr, 0, 1) != GlPath::rocfft; }   // the wav -> mel calls' question

// uniform: rows of one length; ragged_gl: + the rows' tails of the window sum of squares; wav_rows: + gvx_wav_to_mel_ragged's row words
enum class WsKind { uniform, ragged_gl, wav_rows };
struct GlWs {  // byte offsets
    size_t mag, ang, reb0, reb1, fr, y, wss, amp, fft_work, basis, wss_tail, rows, peak, peak_bits, total;
};

// what a call holds once it is open: its rocFFT plans (null: none were made, see gl_layout), its workspace and layout, its stream
struct GlCall {
    FftPair* fp = nullptr;
    GlWs w{};
    void* ws = nullptr;
    hipStream_t s = nullptr;
    template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }
};

// Plans and layout of a call on B rows of T frames and M mels (0: none).  plans_when_fused: the uniform calls create their rocFFT
// plan pair even when they run in LDS and count its work buffer in the workspace; gvx_wav_to_mel_ragged does not.  The asymmetry
// shows in the byte counts the size functions return and in the cost of the first call on a batch size, so it is kept as it is.
int gl_layout(gvx_gl_plan* p, int B, int T, int M, WsKind kind, bool plans_when_fused, GlCall* c);
// The opening of every call behind its own argument checks: gl_layout, the workspace check, the stream.
int gl_open(gvx_gl_plan* p, int B, int T, int M, WsKind kind, bool plans_when_fused, void* ws, size_t ws_bytes, void* stream, GlCall* c);

// f(std::true_type) for a ragged batch, f(std::false_type) for rows of one length: a launch is written once and instantiated twice
template <typename F>
void ragged_dispatch(bool ragged, F&& f) {
    if (ragged) f(std::true_type{}); else f(std::false_type{});
}

}}  // namespace gvx::voc

// ---- device code of more than one source (file-local in each) --------------------------------------------------------------------
namespace {

constexpr int GLF_FRAMES = 4;   // frames (waves) per workgroup of the forward kernels (gl_forward_update_kernel, stft_magnitude_kernel)

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

}  // namespace
