// 256-, 512- and 1024-point complex FFT of one frame by one wave, in LDS: the transforms under the multi-resolution STFT loss
// (stft_loss.hip), whose real transforms of 512, 1024 and 2048 samples are complex transforms of half the size plus the even/odd
// split (fft512_lds.h's rfft_split; the gradient kernel packs its inverse side for itself, two points from one pair of bins).
// Stockham passes like fft512_lds.h's (whose butterflies, padding and wave fence this header reuses, and whose own 512-point
// instantiations it leaves alone), but from LDS to LDS: the caller writes point i to buf[fpad(i)], the result is left there in
// natural order, and every pass reads all of a lane's points into registers before it writes any - the exchange is in place.
// Radices: 256 = 4.4.4.4, 512 = 8.8.8, 1024 = 8.8.4.4, so that every pass keeps all 64 lanes busy (a radix-8 pass over 256 points
// has 32 butterflies).  fp32, table twiddles tw[m] = w_H^m computed in double on the host; the inverse is unnormalised.
#pragma once
#include "fft512_lds.h"

namespace {

template <int H> constexpr int fft_lds_words() { return H + H / 8 + 8; }   // float2 words per frame: fpad(H) is a valid index

// one pass of radix R over H points whose sub-transforms so far have NS points: butterfly i (of H / R) takes x[i + r H/R], turns
// input r by w_{NS R}^{r k} with k = i mod NS, and leaves output r at (i - k) R + k + r NS
template <int H, int R, int NS, bool INV>
__device__ __forceinline__ void fft_lds_pass(float2* buf, const float2* __restrict__ tw, int j) {
    constexpr int T = H / R, V = T / 64;
    static_assert(V >= 1 && (R == 4 || R == 8), "every pass keeps the 64 lanes busy");
    float2 v[V][R];
#pragma unroll
    for (int m = 0; m < V; ++m)
#pragma unroll
        for (int r = 0; r < R; ++r) v[m][r] = buf[fpad(j + 64 * m + r * T)];
    wave_lds_fence();
#pragma unroll
    for (int m = 0; m < V; ++m) {
        const int i = j + 64 * m, k = i & (NS - 1);
        if (NS > 1) {
#pragma unroll
            for (int r = 1; r < R; ++r) {
                float2 w = tw[r * k * (H / (NS * R))];
                if (INV) w.y = -w.y;
                v[m][r] = cmul(v[m][r], w);
            }
        }
        if constexpr (R == 8) dft8<INV>(v[m]);
        else dft4<INV>(v[m][0], v[m][1], v[m][2], v[m][3]);
        const int j0 = (i - k) * R + k;
#pragma unroll
        for (int r = 0; r < R; ++r) buf[fpad(j0 + r * NS)] = v[m][r];
    }
    wave_lds_fence();
}

template <int H, bool INV>
__device__ __forceinline__ void fft_lds_wave(float2* buf, const float2* __restrict__ tw, int j) {
    static_assert(H == 256 || H == 512 || H == 1024, "supported sizes");
    if constexpr (H == 256) {
        fft_lds_pass<H, 4, 1, INV>(buf, tw, j);
        fft_lds_pass<H, 4, 4, INV>(buf, tw, j);
        fft_lds_pass<H, 4, 16, INV>(buf, tw, j);
        fft_lds_pass<H, 4, 64, INV>(buf, tw, j);
    } else if constexpr (H == 512) {
        fft_lds_pass<H, 8, 1, INV>(buf, tw, j);
        fft_lds_pass<H, 8, 8, INV>(buf, tw, j);
        fft_lds_pass<H, 8, 64, INV>(buf, tw, j);
    } else {
        fft_lds_pass<H, 8, 1, INV>(buf, tw, j);
        fft_lds_pass<H, 8, 8, INV>(buf, tw, j);
        fft_lds_pass<H, 4, 64, INV>(buf, tw, j);
        fft_lds_pass<H, 4, 256, INV>(buf, tw, j);
    }
}

}  // namespace
