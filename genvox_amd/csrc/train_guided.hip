// Diagonal guided attention loss (Tachibana et al. 2017, as ESPnet's Tacotron2 recipe masks and averages it) and its gradient on
// the alignments, in ONE pass over A [B][T][L] (gvx_guided_attention_loss):
//   G[b][t][l] = 1 - exp(-(l / L_b - t / T_b)^2 / (2 sigma^2))   for t < T_b and l < L_b,   N = sum_b T_b L_b,
//   loss = sum G A / N,   dalign = alpha G / N,   cells outside a row's T_b x L_b skipped (A is not looked at there), dalign 0.
// G goes to 0 on the diagonal, where l / L_b - t / T_b cancels: two rounded quotients would leave an error of an ulp of 1 in a
// difference of 1e-3 and smaller.  The difference is formed from the exact integer l T_b - t L_b, divided once by L_b T_b, and
// G = -expm1f(-x): every element carries a few roundings of ITSELF (9 u, u = 2^-24, counted at guide() below) and is exactly 0
// where l T_b = t L_b.
// The sum: a wave takes whole (b, t) rows in a fixed assignment, a lane adds its cells as float64 in ascending l, the wave's
// shuffle tree, the workgroup's four waves and the GA_BLOCKS partials are each added in one fixed order: two runs are bit-equal,
// no atomics.  N is a sum of integers (exact in any order), so every wave adds it up for itself from the two length arrays and
// nothing waits for the host.
#include "train_internal.h"

namespace gvx {
namespace {

constexpr int GA_BLOCKS = 256, GA_THREADS = 256, GA_WAVES = GA_THREADS / 64;

__device__ __forceinline__ int clampi(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// G of one live cell.  num = l T_b - t L_b is exact; (float)num and den = (float)(L_b T_b) are exact below 2^24 (a rounding each
// beyond).  d = num / den: 1 rounding (u); d d: 2 u + u; times inv2s2 (itself rounded once): + 2 u -> x is good to 5 u, and
// G' x / G = x / (e^x - 1) <= 1 passes that on as at most 5 u of G; expm1f is good to 1 ulp (2 u): 7 u.  The caller's scale
// alpha / N (rounded once) and the product add 2 u: 9 u for an element of dalign.
__device__ __forceinline__ float guide(long num, float den, float inv2s2) {
    const float d = (float)num / den;
    return -expm1f(-((d * d) * inv2s2));
}

template <bool GRAD>
__global__ __launch_bounds__(GA_THREADS) void guided_attention_kernel(const float* __restrict__ A, const int* __restrict__ token_lengths,
                                                                      const int* __restrict__ mel_lengths, int B, int T, int L, float inv2s2,
                                                                      float alpha, float* __restrict__ dalign, double* partial,
                                                                      long long* n_out) {
    __shared__ double red[GA_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long n = 0;
    for (int b = lane; b < B; b += 64) n += (long long)clampi(token_lengths[b], L) * clampi(mel_lengths[b], T);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    const float scale = n > 0 ? (float)((double)alpha / (double)n) : 0.f;
    double acc = 0.0;
    const long rows = (long)B * T;
    for (long r = (long)blockIdx.x * GA_WAVES + wave; r < rows; r += (long)GA_BLOCKS * GA_WAVES) {
        const int b = (int)(r / T), t = (int)(r - (long)b * T);
        const int Lb = clampi(token_lengths[b], L), Tb = clampi(mel_lengths[b], T);
        const int live = t < Tb ? Lb : 0;   // cells [0, live) of this row count
        const float den = (float)((long)Lb * Tb);
        const long tLb = (long)t * Lb;
        const float* arow = A + r * L;
        float* drow = GRAD ? dalign + r * L : nullptr;
        // float4 along the row where its first element sits on 16 bytes in both tensors (every row when L % 4 == 0)
        const bool vec = ((reinterpret_cast<uintptr_t>(arow) | (GRAD ? reinterpret_cast<uintptr_t>(drow) : 0)) & 15) == 0;
        const int Lv = vec ? (L & ~3) : 0;
        for (int l0 = lane * 4; l0 < Lv; l0 += 256) {
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if (l0 < live) {
                const float4 a = *reinterpret_cast<const float4*>(arow + l0);   // (may reach past `live`, never past L: those lanes are not used)
                g.x = guide((long)l0 * Tb - tLb, den, inv2s2);
                acc += (double)g.x * (double)a.x;
                if (l0 + 1 < live) { g.y = guide((long)(l0 + 1) * Tb - tLb, den, inv2s2); acc += (double)g.y * (double)a.y; }
                if (l0 + 2 < live) { g.z = guide((long)(l0 + 2) * Tb - tLb, den, inv2s2); acc += (double)g.z * (double)a.z; }
                if (l0 + 3 < live) { g.w = guide((long)(l0 + 3) * Tb - tLb, den, inv2s2); acc += (double)g.w * (double)a.w; }
            }
            if (GRAD) *reinterpret_cast<float4*>(drow + l0) = make_float4(scale * g.x, scale * g.y, scale * g.z, scale * g.w);
        }
        for (int l = Lv + lane; l < L; l += 64) {
            float g = 0.f;
            if (l < live) { g = guide((long)l * Tb - tLb, den, inv2s2); acc += (double)g * (double)arow[l]; }
            if (GRAD) drow[l] = scale * g;
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < GA_WAVES; ++w) s += red[w];
        partial[blockIdx.x] = s;
        if (blockIdx.x == 0) *n_out = n;
    }
}

__global__ void guided_attention_final_kernel(const double* partial, const long long* n_in, float* loss_out) {
    double s = 0.0;
    for (int b = 0; b < GA_BLOCKS; ++b) s += partial[b];
    const long long n = *n_in;
    loss_out[0] = n > 0 ? (float)(s / (double)n) : 0.f;
}

constexpr size_t GA_SCRATCH_BYTES = (size_t)(GA_BLOCKS + 1) * sizeof(double);   // the partials, then N

}  // namespace
}  // namespace gvx

using namespace gvx;

extern "C" {

size_t gvx_guided_attention_loss_scratch_bytes(int B, int T, int L) {
    if (B < 1 || T < 1 || L < 1) { tfail(GVX_ERR_INVALID_ARG, "guided_attention_loss: B, T and L must be >= 1"); return 0; }
    return GA_SCRATCH_BYTES;
}

int gvx_guided_attention_loss(const float* align, const int32_t* token_lengths, const int32_t* mel_lengths, int B, int T, int L, float sigma,
                              float alpha, float* loss_out, float* dalign, void* scratch, size_t scratch_bytes, void* stream) {
    if (!align || !token_lengths || !mel_lengths || !loss_out) return tfail(GVX_ERR_INVALID_ARG, "guided_attention_loss: null pointer argument");
    if (B < 1 || T < 1 || L < 1) return tfail(GVX_ERR_INVALID_ARG, "guided_attention_loss: B, T and L must be >= 1");
    if (!(sigma > 0.f) || !(sigma <= 3.4e38f)) return tfail(GVX_ERR_INVALID_ARG, "guided_attention_loss: sigma must be positive and finite");
    if (!(alpha >= 0.f) || !(alpha <= 3.4e38f)) return tfail(GVX_ERR_INVALID_ARG, "guided_attention_loss: alpha must be non-negative and finite");
    if (!scratch || scratch_bytes < GA_SCRATCH_BYTES || (reinterpret_cast<uintptr_t>(scratch) & 7))
        return tfail(GVX_ERR_WORKSPACE, "guided_attention_loss: scratch too small (gvx_guided_attention_loss_scratch_bytes) or not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    double* partial = reinterpret_cast<double*>(scratch);
    long long* n = reinterpret_cast<long long*>(partial + GA_BLOCKS);
    const float inv2s2 = (float)(1.0 / (2.0 * (double)sigma * (double)sigma));
    if (!(inv2s2 <= 3.4e38f)) return tfail(GVX_ERR_INVALID_ARG, "guided_attention_loss: sigma too small (1 / (2 sigma^2) is not a finite float)");
    if (dalign)
        hipLaunchKernelGGL(guided_attention_kernel<true>, dim3(GA_BLOCKS), dim3(GA_THREADS), 0, s, align, token_lengths, mel_lengths, B, T, L, inv2s2, alpha,
                           dalign, partial, n);
    else
        hipLaunchKernelGGL(guided_attention_kernel<false>, dim3(GA_BLOCKS), dim3(GA_THREADS), 0, s, align, token_lengths, mel_lengths, B, T, L, inv2s2, alpha,
                           dalign, partial, n);
    TR_TRY(hipGetLastError());
    hipLaunchKernelGGL(guided_attention_final_kernel, dim3(1), dim3(1), 0, s, partial, n, loss_out);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}

}  // extern "C"
