// The two streaming transforms of a k = 5 convolution along time computed as Winograd F(4,5) (winograd_f45.h): between them
// the eight products per tile of four frames run as ONE batched launch of the fp32 GEMM (gemm_f32.hip, GemmParams::slices)
// against the weights' transform U = G w, which the packers keep in the blob (gvx_pack.hip).
//
//   input   x[B][T + 4][C]  channels-last, two zero halo rows on either side of each sequence (what the direct form reads too)
//   V[s][b * tiles + j][c] = sum_i BT[s][i] x[b][4 j + i][c]          tiles = ceil(T / 4), tile j = frames 4 j .. 4 j + 3
//   M[s][m][n]             = sum_c V[s][m][c] U[s][n][c]              (the GEMM, K = C)
//   y[b][4 j + i][n]       = act(bias[n] + sum_s AT[i][s] M[s][b * tiles + j][n])     Postnet: tanh, zero at or behind row_len[b];
//                                                                                      encoder: ReLU, every position of the sequence
//
// Tiles start at frame 0 of each sequence, so a row's values do not depend on the batch it runs in, on T, or on how the batch's
// tiles are cut into groups (a group is any range of tiles: the caller sizes it to the scratch it has); rows of x past the
// sequence's own halo (a last tile that sticks out: the next sequence follows in memory) are zeros by predicate.
// Both kernels: one thread per (tile, four channels), 16-byte accesses, lanes along the channels - every load and store of a
// wave is contiguous.  No LDS, no reuse beyond the cache (an input row is read by two tiles): both are bound by the bytes
// they move, V and M written / read once each.  The sums are fmaf chains in a fixed order: deterministic, shape independent.
#include "gvx_kernels.h"
#include "winograd_f45.h"

namespace gvx {

namespace {

__device__ __forceinline__ float4 f4_fma(float a, const float4& x, const float4& y) {
    return make_float4(fmaf(a, x.x, y.x), fmaf(a, x.y, y.y), fmaf(a, x.z, y.z), fmaf(a, x.w, y.w));
}

// A launch covers the tiles [mt0, mt0 + nmt) of the batch (tile b * tiles + j = tile j of sequence b): a group of tiles whose V and
// M fit the scratch.  x: the batch's buffer (front halo of sequence 0); rows per sequence T + 4.  V: [8][nmt][C], this group's.
__global__ void __launch_bounds__(256) winograd_input_kernel(const float* __restrict__ x, float* __restrict__ V, long mt0, long nmt, int T, int C) {
    const int tiles = (T + WINO_OUT - 1) / WINO_OUT, c4n = C >> 2;
    const long total = nmt * c4n;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % c4n) * 4;
    const long lt = idx / c4n, mt = mt0 + lt;
    const int b = (int)(mt / tiles), j = (int)(mt - (long)b * tiles);
    const int rows = T + WINO_TAPS - 1;   // the sequence's rows with both halos
    const float* src = x + ((long)b * rows + 4 * j) * C + c;
    float4 d[WINO_PTS];
#pragma unroll
    for (int i = 0; i < WINO_PTS; ++i)
        d[i] = 4 * j + i < rows ? *reinterpret_cast<const float4*>(src + (long)i * C) : make_float4(0.f, 0.f, 0.f, 0.f);
    const long slice = nmt * C;
    float* dst = V + lt * C + c;
#pragma unroll
    for (int s = 0; s < WINO_PTS; ++s) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 0; i < WINO_PTS; ++i)
            if (wino_BT(s, i) != 0.f) v = f4_fma(wino_BT(s, i), d[i], v);
        *reinterpret_cast<float4*>(dst + s * slice) = v;
    }
}

// y: the batch's next halo buffer (front halo of sequence 0), row_len: the batch's; the thread of a sequence's first / last tile
// also writes the two front / back halo rows (zeros), so the buffer may hold anything before.
// ACT: the layer's activation.  ACT_TANH is the Postnet's form: frames at or behind row_len[b] are zeros.  ACT_RELU is the encoder's:
// no row_len (its convolutions see the padding tokens' embeddings, as the reference's do), every frame of the sequence is computed.
template <int ACT>
__global__ void __launch_bounds__(256) winograd_output_kernel(const float* __restrict__ Mm, const float* __restrict__ bias, const int32_t* __restrict__ row_len,
                                                              float* __restrict__ y, long mt0, long nmt, int T, int C) {
    const int tiles = (T + WINO_OUT - 1) / WINO_OUT, c4n = C >> 2;
    const long total = nmt * c4n;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % c4n) * 4;
    const long lt = idx / c4n, mt = mt0 + lt;
    const int b = (int)(mt / tiles), j = (int)(mt - (long)b * tiles);
    const long slice = nmt * C;
    const float* src = Mm + lt * C + c;
    float4 m[WINO_PTS];
#pragma unroll
    for (int s = 0; s < WINO_PTS; ++s) m[s] = *reinterpret_cast<const float4*>(src + s * slice);
    const float4 bv = *reinterpret_cast<const float4*>(bias + c);
    [[maybe_unused]] const int len = row_len ? row_len[b] : T;
    constexpr int HALO = (WINO_TAPS - 1) / 2;
    const int rows = T + 2 * HALO;
    float* dst = y + ((long)b * rows + HALO) * C + c;   // frame 0 of the sequence
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < WINO_OUT; ++i) {
        const int t = 4 * j + i;
        float4 v = zero;
#pragma unroll
        for (int s = 0; s < WINO_PTS; ++s)
            if (wino_AT(i, s) != 0.f) v = f4_fma(wino_AT(i, s), m[s], v);
        if constexpr (ACT == ACT_TANH) {
            const bool live = t < len;   // (selected per component: a float4 select makes LLVM build a lookup table in scratch)
            v = make_float4(live ? tanhf(v.x + bv.x) : 0.f, live ? tanhf(v.y + bv.y) : 0.f, live ? tanhf(v.z + bv.z) : 0.f, live ? tanhf(v.w + bv.w) : 0.f);
        } else {
            v = make_float4(fmaxf(v.x + bv.x, 0.f), fmaxf(v.y + bv.y, 0.f), fmaxf(v.z + bv.z, 0.f), fmaxf(v.w + bv.w, 0.f));
        }
        if (t < T) *reinterpret_cast<float4*>(dst + (long)t * C) = v;
    }
    if (j == 0) {
#pragma unroll
        for (int h = 1; h <= HALO; ++h) *reinterpret_cast<float4*>(dst - (long)h * C) = zero;
    }
    if (j == tiles - 1) {
#pragma unroll
        for (int h = 0; h < HALO; ++h) *reinterpret_cast<float4*>(dst + (long)(T + h) * C) = zero;
    }
}

unsigned blocks_of(long nmt, int C) { return (unsigned)((nmt * (C >> 2) + 255) / 256); }
// (the range must lie inside the batch's B * ceil(T / 4) tiles: the kernels address x, y and row_len from the tile index)
bool bad_shape(int B, long mt0, long nmt, int T, int C) {
    if (B < 1 || T < 1 || C < 4 || (C & 3) || mt0 < 0 || nmt < 1) return true;
    return mt0 + nmt > (long)B * ((T + WINO_OUT - 1) / WINO_OUT) || nmt * (C >> 2) > ((long)1 << 38);
}

}  // namespace

hipError_t launch_winograd_input(const float* x, float* V, int B, long mt0, long nmt, int T, int C, hipStream_t s) {
    if (bad_shape(B, mt0, nmt, T, C)) return hipErrorInvalidValue;
    winograd_input_kernel<<<dim3(blocks_of(nmt, C)), dim3(256), 0, s>>>(x, V, mt0, nmt, T, C);
    return hipGetLastError();
}

hipError_t launch_winograd_output(const float* Mm, const float* bias, const int32_t* row_len, float* y, int B, long mt0, long nmt, int T, int C, int act, hipStream_t s) {
    if (bad_shape(B, mt0, nmt, T, C) || (act != ACT_TANH && (act != ACT_RELU || row_len))) return hipErrorInvalidValue;
    if (act == ACT_TANH) winograd_output_kernel<ACT_TANH><<<dim3(blocks_of(nmt, C)), dim3(256), 0, s>>>(Mm, bias, row_len, y, mt0, nmt, T, C);
    else winograd_output_kernel<ACT_RELU><<<dim3(blocks_of(nmt, C)), dim3(256), 0, s>>>(Mm, bias, nullptr, y, mt0, nmt, T, C);
    return hipGetLastError();
}

}  // namespace gvx
