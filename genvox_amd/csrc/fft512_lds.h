// 512-point complex FFT of one frame by one wave, in LDS: the transform under every n_fft = 1024 / hop = 256 vocoder kernel
// (griffinlim.hip: gl_inverse_ola_kernel, gl_iteration_kernel, gl_forward_update_kernel; wav_to_mel.hip: stft_magnitude_kernel).
// A 1024-point real transform is a 512-point complex Stockham radix-8 (3 passes, 8 points per lane, exchange through LDS) plus
// the even/odd split; the inverse is unnormalised like rocFFT's c2r.  fp32, table twiddles computed in double on the host
// (gvx_gl_plan_create).  The split and its inverse-side pack are written once, here, for every size (rfft_split, irfft_pack: on
// values, the callers keep their own LDS addressing); fft_lds.h builds the 256- and 1024-point transforms on the same pieces.
#pragma once
#include <hip/hip_runtime.h>

namespace {

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

// Real transform of 2H samples from the complex transform Z of its H even/odd pairs: bin k from zk = Z[k mod H] and zc = Z[(H - k)
// mod H], both as stored, and w = e^{-2 pi i k/2H}.  edge: k is 0 or H, the two bins that are exactly real for a real signal
__device__ __forceinline__ float2 rfft_split(float2 zk, float2 zc, float2 w, bool edge) {
    zc.y = -zc.y;
    const float2 sm = cadd(zk, zc), df = csub(zk, zc);
    const float2 wd = cmul(w, df);                       // W^k (Z[k] - conj Z[H-k])
    float2 X = make_float2(0.5f * (sm.x + wd.y), 0.5f * (sm.y - wd.x));   // 0.5*sm - 0.5i*wd
    if (edge) X.y = 0.f;
    return X;
}

// The way back: point k of the H-point complex input of the unnormalised inverse real transform from a = S[k], c = S[H - k] as
// stored and the same w.  dc: k is 0 (c is then the Nyquist bin); c2r ignores the imaginary parts of the DC and Nyquist bins
__device__ __forceinline__ float2 irfft_pack(float2 a, float2 c, float2 w, bool dc) {
    if (dc) { a.y = 0.f; c.y = 0.f; }
    c.y = -c.y;                                          // conj(S[H - k])
    const float2 d = csub(a, c);
    const float2 id = make_float2(-d.y, d.x);            // i * d
    return cadd(cadd(a, c), cmul(id, make_float2(w.x, -w.y)));   // w is e^{-...}; need e^{+...}
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

}  // namespace
