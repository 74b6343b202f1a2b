// The tail of the mel -> waveform vocoder (griffinlim.hip): clip / trim / peak-normalise / Butterworth low-pass of the waveforms that
// Griffin-Lim or a neural vocoder left, for rows of one length (gvx_wav_finalize) and for rows of their own lengths
// (gvx_wav_finalize_ragged).  Needs no plan, no FFT and no workspace beyond the caller's B words; what it shares with the other
// vocoder sources is vocoder_internal.h.
//
// Order of this file: kernels, the host side of the calls, the C ABI.
#include "vocoder_internal.h"

#include <cmath>
#include <cstring>

using namespace gvx::voc;

namespace {

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

// gvx_wav_finalize (lens == nullptr, n_fft = hop = 0) and gvx_wav_finalize_ragged
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
    ragged_dispatch(lens != nullptr, [&](auto R) {
        wav_peak_kernel<decltype(R)::value><<<dim3(64, B), 256, 0, s>>>(wav, n_samples, trim, scratch_B, lens, n_fft, hop);
    });
    GL_HIP(hipGetLastError());
    const int warm = iir_warmup_length(c, 4096);
    ragged_dispatch(lens != nullptr, [&](auto R) {
        constexpr bool ragged = decltype(R)::value;
        if (warm > 0) {
            int chunk = 1024;
            while (chunk < 8 * warm) chunk *= 2;   // warm-up work <= 1/8 of the total
            const long n_out = n_samples - 2L * trim;
            const int nch = (int)((n_out + chunk - 1) / chunk);
            wav_filter_chunked_kernel<ragged><<<dim3((nch + 63) / 64, B), 64, 0, s>>>(wav, n_samples, trim, scratch_B, c, out, chunk, warm, nch,
                                                                                     lens, n_fft, hop);
        } else {                                    // slowly decaying filter: sequential
            wav_filter_kernel<ragged><<<(B + 63) / 64, 64, 0, s>>>(wav, n_samples, trim, scratch_B, c, out, B, lens, n_fft, hop);
        }
    });
    GL_HIP(hipGetLastError());
    return GVX_OK;
}

}  // namespace

extern "C" {

int gvx_wav_finalize(const float* wav, int B, long n_samples, int trim, const double* b_coef, const double* a_coef, int order,
                     double* out, unsigned int* scratch_B, void* stream) {
    return wav_finalize_impl(wav, B, n_samples, nullptr, 0, 0, trim, b_coef, a_coef, order, out, scratch_B, stream);
}

int gvx_wav_finalize_ragged(const float* wav, int B, long n_samples, const int32_t* frame_lengths, int n_fft, int hop, int trim,
                            const double* b_coef, const double* a_coef, int order, double* out, unsigned int* scratch_B, void* stream) {
    if (!frame_lengths) return gl_fail(GVX_ERR_INVALID_ARG, "null frame_lengths (gvx_wav_finalize is the call for rows of one length)");
    if (B < 1 || n_fft < 1 || hop < 1 || trim < 0) return gl_fail(GVX_ERR_INVALID_ARG, "B, n_fft, hop must be >= 1 and trim >= 0");
    return wav_finalize_impl(wav, B, n_samples, frame_lengths, n_fft, hop, trim, b_coef, a_coef, order, out, scratch_B, stream);
}

}  // C ABI
