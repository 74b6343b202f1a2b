// Winograd / Toom-Cook F(4,5) along time: 4 output frames of a k = 5 correlation from 8 products per (cin, cout) pair,
//   y[0..3] = A^T [ (G g) .* (B^T d) ],   y[i] = sum_k g[k] d[i + k],  d = 8 input frames, g = 5 taps,
// with the evaluation points {0, 1, -1, 2, -2, 1/2, -1/2, infinity}.  Each row's scale sits in G (applied once, in double, when
// the weights are packed), so that B^T is a matrix of small integers and A^T of powers of two: both are exact in fp32.
// Used by gvx_pack.hip (U = G w), winograd_conv.hip (the two transforms) and gvx_debug_winograd_constants (tests).
#pragma once
#include <hip/hip_runtime.h>

namespace gvx {

constexpr int WINO_OUT = 4;    // output frames per tile
constexpr int WINO_TAPS = 5;   // filter taps
constexpr int WINO_PTS = 8;    // products per tile = input frames per tile

__host__ __device__ inline double wino_G(int s, int k) {
    constexpr double G[WINO_PTS][WINO_TAPS] = {
        {1.0 / 4.0, 0, 0, 0, 0},
        {1.0 / 18.0, 1.0 / 18.0, 1.0 / 18.0, 1.0 / 18.0, 1.0 / 18.0},
        {1.0 / 18.0, -1.0 / 18.0, 1.0 / 18.0, -1.0 / 18.0, 1.0 / 18.0},
        {1.0 / 360.0, 1.0 / 180.0, 1.0 / 90.0, 1.0 / 45.0, 2.0 / 45.0},
        {1.0 / 360.0, -1.0 / 180.0, 1.0 / 90.0, -1.0 / 45.0, 2.0 / 45.0},
        {16.0 / 45.0, 8.0 / 45.0, 4.0 / 45.0, 2.0 / 45.0, 1.0 / 45.0},
        {16.0 / 45.0, -8.0 / 45.0, 4.0 / 45.0, -2.0 / 45.0, 1.0 / 45.0},
        {0, 0, 0, 0, 1.0 / 4.0},
    };
    return G[s][k];
}

__host__ __device__ inline float wino_BT(int s, int i) {
    constexpr float BT[WINO_PTS][WINO_PTS] = {
        {4, 0, -21, 0, 21, 0, -4, 0},
        {0, -4, -4, 17, 17, -4, -4, 0},
        {0, 4, -4, -17, 17, 4, -4, 0},
        {0, 2, 1, -10, -5, 8, 4, 0},
        {0, -2, 1, 10, -5, -8, 4, 0},
        {0, 4, 8, -5, -10, 1, 2, 0},
        {0, -4, 8, 5, -10, -1, 2, 0},
        {0, -4, 0, 21, 0, -21, 0, 4},
    };
    return BT[s][i];
}

__host__ __device__ inline float wino_AT(int i, int s) {
    constexpr float AT[WINO_OUT][WINO_PTS] = {
        {1, 1, 1, 1, 1, 1, 1, 0},
        {0, 1, -1, 2, -2, 0.5f, -0.5f, 0},
        {0, 1, 1, 4, 4, 0.25f, 0.25f, 0},
        {0, 1, -1, 8, -8, 0.125f, -0.125f, 1},
    };
    return AT[i][s];
}

// U[s] = sum_k G[s][k] * (w[k] * scale) in double, k ascending - the one expression both packers (host and device) evaluate, so
// that a blob re-packed on the device equals the host's bit for bit.  w: the 5 taps of one (cout, cin) pair, stride `ws`.
__host__ __device__ inline float wino_weight(const float* w, long ws, double scale, int s) {
    double u = 0.0;
    for (int k = 0; k < WINO_TAPS; ++k) u += wino_G(s, k) * ((double)w[k * ws] * scale);
    return (float)u;
}

}  // namespace gvx
