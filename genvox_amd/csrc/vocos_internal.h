// What csrc/vocos.hip (inference) and csrc/vocos_train.hip (tape forward, backward) share: the handle, the arguments of the
// forward's launches, the blob and workspace layouts and the checks of dims and shapes.  Defined in vocos.hip.
#pragma once
#include "gen_host.h"

struct gvx_vocos : gvx_gen::GenHandle {
    gvx_vocos_dims d;
    gvx_gen::GenMarks bwd_marks;   // gvx_vocos_backward's parts (vocos_train.hip)
};

namespace gvx { hipError_t gemm_init(); }

namespace gvx_vc {

constexpr int VC_P = GVX_VOCOS_TILE;
constexpr int VC_WAVES = 4;          // waves per workgroup of the filter + LayerNorm kernel and of the frame kernel
constexpr float VC_LN_EPS = 1e-6f;
constexpr float VC_MAG_MAX = 100.f;

#if defined(__HIPCC__)
__device__ __forceinline__ float vc_wave_sum(float v) {   // a butterfly: every lane ends with the same bits
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
#endif

struct VcNorm {
    const float* x; float* out;
    const int32_t* lens;
    int T, C, taps;
    const float* w; const float* b; const float* ln_w; const float* ln_b;
    float eps;
};

struct VcIstft {
    const float* coeffs;   // [B][T][N + 2]: m[0 .. H], p[0 .. H]
    const int32_t* lens;
    int T;
    const float* win; const float2* tw; const float2* tw2;
    float* frames;         // [B][T][N]
};

struct VcLayer { size_t dw_w, dw_b, ln_w, ln_b, pw1_w, pw1_b, pw2_w, pw2_b; };
struct VcBlob {
    size_t embed_w, embed_b, norm_w, norm_b;
    VcLayer layer[GVX_VOCOS_MAX_LAYERS];
    size_t fin_w, fin_b, head_w, head_b, window, tw, tw2, total;
};
struct VcWs { size_t mel_t, x, a, h, coeffs, frames, total; };

inline int vc_cpad(const gvx_vocos_dims& d) { return (d.n_mels + 3) & ~3; }

int vc_norm(const VcNorm& p, int B, hipStream_t s);
int vc_istft(const VcIstft& a, int B, int N, int hop, int center, float* wav, hipStream_t s);
// window [N] (NULL: none), w_H^m [H] and w_N^k [H + 1], in float64
int vc_tables(float* win, float2* tw, float2* tw2, int N, hipStream_t s);
// mel [B][M][T] -> out [B][T + 6][Cp]: frame t at row t + 3, zeros in the halo rows, at and behind the row's length and in the padding
int vc_mel_transpose(const float* mel, const int32_t* lens, int B, int M, int T, int Cp, float* out, hipStream_t s);
const char* vc_fft_problem(int n_fft, int hop, int center);
const char* vc_dims_problem(const gvx_vocos_dims* d);
const char* vc_shape_problem(int B, int T);
VcBlob vc_blob_layout(const gvx_vocos_dims& d);
VcWs vc_ws_plan(const gvx_vocos_dims& d, int B, int T);
// C [B][T][N] = epilogue(A W^T + bias): rows grouped by T for row_len
int vc_gemm(const float* A, const gvx::RowMap& amap, int K, const float* W, const float* bias, float* out, int N, int B, int T, const int32_t* lens,
            int act, const float* res, hipStream_t s);

}  // namespace gvx_vc
