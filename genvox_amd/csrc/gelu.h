// nn.GELU() in its erf form, once for the GEMM's EPI_GELU epilogue (gemm_f32.hip), the tape forward's separate launch and the GELU
// backward (vocos_train.hip): the three see the same function, so h = gelu(p) has the same bits wherever it is formed.
#pragma once
#include <hip/hip_runtime.h>

// x Phi(x) with the library's erff (1 ulp; the 1 + erf cancellation for x < 0 costs an absolute 6e-8 |x|, below an ulp of the
// tensor's scale)
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752f)); }

// d gelu / d v = Phi(v) + v phi(v)
__device__ __forceinline__ float gelu_erf_grad(float v) {
    const float cdf = 0.5f * (1.f + erff(v * 0.70710678118654752f));
    const float pdf = 0.3989422804014327f * expf(-0.5f * v * v);
    return cdf + v * pdf;
}
