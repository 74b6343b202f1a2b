// Whole-sequence pieces of the backward pass: generic primitives for the host side (genvox_amd/training.py) - dense products
// on the exact-fp32 MFMA GEMM, transposes, column sums, elementwise updates, Adam.  All tensors row-major fp32 with an
// explicit leading dimension where slices are taken.  The two recurrences are in train_bptt_decoder.hip and
// train_bptt_encoder.hip.
#include "train_internal.h"

#include <cmath>
#include <cstdio>

namespace gvx {
namespace {

// column sums over the rows of X [rows][C] (and of X * Y when Y != nullptr), double accumulation, fixed order.
// Workgroup = 32 columns x 32 row lanes; a lane walks its rows four at a time with independent partial sums, so that the
// loads of a pass are in flight together (the first version walked 8 lanes x rows / 8 dependent iterations: 290 us for the
// 6 400 x 4 096 gate-gradient matrices of a 32 x 200 step).
__global__ __launch_bounds__(1024) void col_reduce_kernel(const float* X, const float* Y, long rows, int C, float* sum_x, float* sum_xy) {
    __shared__ double sx[CR_LANES][33], sxy[CR_LANES][33];
    const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
    if (c < C) {
        long r = rl;
        for (; r + 3 * CR_LANES < rows; r += 4 * CR_LANES) {
            const float x0 = X[r * C + c], x1 = X[(r + CR_LANES) * C + c], x2 = X[(r + 2 * CR_LANES) * C + c], x3 = X[(r + 3 * CR_LANES) * C + c];
            a0 += x0; a1 += x1; a2 += x2; a3 += x3;
            if (Y) {
                b0 += (double)x0 * (double)Y[r * C + c]; b1 += (double)x1 * (double)Y[(r + CR_LANES) * C + c];
                b2 += (double)x2 * (double)Y[(r + 2 * CR_LANES) * C + c]; b3 += (double)x3 * (double)Y[(r + 3 * CR_LANES) * C + c];
            }
        }
        for (; r < rows; r += CR_LANES) {
            const double x = X[r * C + c];
            a0 += x;
            if (Y) b0 += x * (double)Y[r * C + c];
        }
    }
    sx[rl][cl] = (a0 + a1) + (a2 + a3); sxy[rl][cl] = (b0 + b1) + (b2 + b3);
    __syncthreads();
    if (rl == 0 && c < C) {
        double ta = 0.0, tb = 0.0;
        for (int i = 0; i < CR_LANES; ++i) { ta += sx[i][cl]; tb += sxy[i][cl]; }
        sum_x[c] = (float)ta;
        if (Y && sum_xy) sum_xy[c] = (float)tb;
    }
}

// dst[c][r] = src[r][c]  for r < rows; columns of dst are padded with zeros up to rows_p.  32 x 32 tiles through LDS: both the
// reads and the writes are row-contiguous.  grid (ceil(rows_p / 32), ceil(C / 32)), 256 threads
__global__ __launch_bounds__(256) void transpose_pad_kernel(const float* src, float* dst, long rows, int C, long rows_p) {
    __shared__ float tile[32][33];
    const long r0 = (long)blockIdx.x * 32;
    const int c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long r = r0 + ty + 8 * i;
        const int c = c0 + tx;
        tile[ty + 8 * i][tx] = (r < rows && c < C) ? src[r * C + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = c0 + ty + 8 * i;
        const long r = r0 + tx;
        if (c < C && r < rows_p) dst[(long)c * rows_p + r] = tile[tx][ty + 8 * i];
    }
}
// generic elementwise: y[r][c] = alpha * a[r][c] + beta * b[r][c]   (b may be null), each with its own leading dimension
__global__ void axpby_kernel(const float* a, long lda, float alpha, const float* b, long ldb, float beta, float* y, long ldy, long rows, int cols) {
    const long n = rows * cols;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % cols);
        const long r = i / cols;
        float v = alpha * a[r * lda + c];
        if (b) v += beta * b[r * ldb + c];
        y[r * ldy + c] = v;
    }
}
// dz = dy * keep * scale * (act_out > 0)      (Prenet: relu then dropout)
__global__ void relu_drop_bwd_kernel(const float* dy, const float* act_out, const uint8_t* keep, float scale, long n, float* dz) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dz[i] = (keep[i] && act_out[i] > 0.f) ? dy[i] * scale : 0.f;
}
// k-group-blocked vector [K/8][B][8] -> row-major [B][K]  (slots: n_slots consecutive vectors)
__global__ void unblock_kernel(const float* src, float* dst, long n_slots, int B, int K) {
    const long n = n_slots * B * K;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % K);
        const long sb = i / K;
        const int b = (int)(sb % B);
        const long s = sb / B;
        dst[i] = src[s * B * K + (long)(k >> 3) * B * 8 + b * 8 + (k & 7)];
    }
}
// d embedding[row][e] = sum over the batch positions that hold token `row`, added in position order (no atomics: the result
// does not depend on the launch's scheduling).  One workgroup per table row, threads over the channels.  The positions that hold
// the row's token are first compacted, in order, into LDS (chunks of EMB_CHUNK tokens: every thread looks at a contiguous
// segment, an exclusive scan over the threads places its matches) - walking all positions one by one, as the first version
// did, took 0.32 ms for 4096 positions; the sums themselves then run over ~1 % of them with independent loads.
constexpr int EMB_CHUNK = 8192;
__global__ __launch_bounds__(256) void embedding_bwd_kernel(const int64_t* tokens, const float* dx, long n_tok, int E, int n_rows, float* demb) {
    __shared__ int list[EMB_CHUNK];
    __shared__ int cnt[257];
    const int row = blockIdx.x, tid = threadIdx.x;
    for (int pass = 0; pass * 1024 < E; ++pass) {   // (E <= 1024: one pass; every thread takes part in the barriers of every pass)
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        const int e0 = pass * 1024 + tid, e1 = e0 + 256, e2 = e0 + 512, e3 = e0 + 768;
        for (long base = 0; base < n_tok; base += EMB_CHUNK) {
            const int n = (int)((n_tok - base) < EMB_CHUNK ? (n_tok - base) : EMB_CHUNK), seg = (n + 255) / 256;
            const int lo = tid * seg, hi = lo + seg < n ? lo + seg : n;
            int mine = 0;
            for (int t = lo; t < hi; ++t) mine += tokens[base + t] == row;
            __syncthreads();   // (the list of the previous chunk / pass has been consumed)
            cnt[tid + 1] = mine;
            if (tid == 0) cnt[0] = 0;
            __syncthreads();
            if (tid == 0) for (int i = 1; i <= 256; ++i) cnt[i] += cnt[i - 1];
            __syncthreads();
            int at = cnt[tid];
            for (int t = lo; t < hi; ++t) if (tokens[base + t] == row) list[at++] = t;
            __syncthreads();
            const int m = cnt[256];
            for (int k = 0; k < m; ++k) {   // position order; the loads of later positions do not wait for the adds
                const float* r = dx + (base + list[k]) * E;
                if (e0 < E) a0 += r[e0];
                if (e1 < E) a1 += r[e1];
                if (e2 < E) a2 += r[e2];
                if (e3 < E) a3 += r[e3];
            }
        }
        if (e0 < E) demb[(long)row * E + e0] = a0;
        if (e1 < E) demb[(long)row * E + e1] = a1;
        if (e2 < E) demb[(long)row * E + e2] = a2;
        if (e3 < E) demb[(long)row * E + e3] = a3;
    }
}
// sum of squares of MANY tensors in one launch: workgroup (x, tensor) writes its partial (double) to partials[tensor][x]; a
// second tiny launch adds all partials in index order - the total does not depend on the launch's scheduling (torch's
// clip_grad_norm_ on the reference side is a tree of its own; this one is at least reproducible)
constexpr int SQN_BLOCKS = 64;
__global__ __launch_bounds__(256) void sqnorm_many_kernel(const gvx_tensor_ref* refs, double* partials) {
    __shared__ double red[256];
    const gvx_tensor_ref r = refs[blockIdx.y];
    double s0 = 0.0, s1 = 0.0;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long stride = (long)SQN_BLOCKS * 256;
    for (; i + stride < r.numel; i += 2 * stride) {
        const double a = r.data[i], b = r.data[i + stride];
        s0 += a * a; s1 += b * b;
    }
    if (i < r.numel) { const double a = r.data[i]; s0 += a * a; }
    red[threadIdx.x] = s0 + s1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) partials[(long)blockIdx.y * SQN_BLOCKS + blockIdx.x] = red[0];
}
__global__ __launch_bounds__(256) void sqnorm_finish_kernel(const double* partials, int n, double* out) {
    // 256 strided sums, then a tree: a fixed order (one thread walking all ~6 000 partials took 0.2 ms)
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[0] = red[0];
}
// torch.optim.Adam (L2 weight decay folded into the gradient, bias-corrected), gradient pre-scaled by gscale (clipping),
// for MANY tensors in one launch: workgroup (x, tensor) walks its share of the tensor
__global__ void adam_many_kernel(const gvx_adam_ref* refs, float gscale, float lr, float wd, float b1, float b2, float eps, float bc1,
                                 float bc2_sqrt) {
    const gvx_adam_ref r = refs[blockIdx.y];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < r.numel; i += (long)gridDim.x * blockDim.x) {
        const float gi = r.grad[i] * gscale + wd * r.param[i];
        const float mi = b1 * r.exp_avg[i] + (1.f - b1) * gi;
        const float vi = b2 * r.exp_avg_sq[i] + (1.f - b2) * gi * gi;
        r.exp_avg[i] = mi; r.exp_avg_sq[i] = vi;
        r.param[i] -= (lr / bc1) * mi / (sqrtf(vi) / bc2_sqrt + eps);
    }
}

// The split gvx_train_gemm_nt / _tn ask launch_gemm_splitk for: what choose_splitk wants for the product's 64 x 128 tiles, as far
// as the caller's scratch holds the partial tiles (1 = no split; no scratch, no split)
inline int train_gemm_splitk(int M, int N, int K, bool have_scratch, size_t scratch_bytes) {
    const long tiles = (long)((M + 63) / 64) * ((N + 127) / 128);
    int splitk = have_scratch ? choose_splitk(tiles, K) : 1;
    while (splitk > 1 && (size_t)splitk * M * N * sizeof(float) > scratch_bytes) --splitk;
    return splitk;
}

}  // namespace

int tfail_hip(const char* expr, hipError_t e) {
    thread_local char msg[256];
    snprintf(msg, sizeof msg, "%s failed: %s", expr, hipGetErrorString(e));
    return set_error(GVX_ERR_HIP, msg);
}

void launch_col_reduce(const float* X, const float* Y, long rows, int C, float* sum_x, float* sum_xy, hipStream_t s) {
    hipLaunchKernelGGL(col_reduce_kernel, dim3((C + 31) / 32), dim3(1024), 0, s, X, Y, rows, C, sum_x, sum_xy);
}

}  // namespace gvx

using namespace gvx;

extern "C" {

// Host-only query for the tests (not part of the public header; touches no device): how gvx_train_gemm_nt (kmajor == 0) or
// gvx_train_gemm_tn (kmajor != 0, K = rows) runs an M x N x K product with dense leading dimensions - plan_gemm's tile shape and
// two-launch split, and the number of K pieces (1 = no split-K).  Returns the status launch_gemm would return for the shape.
int gvx_debug_gemm_plan(int M, int N, int K, int kmajor, int have_scratch, size_t scratch_bytes, int* tile_out, int* rows_big_out, int* k_pieces_out) {
    if (!tile_out || !rows_big_out || !k_pieces_out || M < 1 || N < 1 || K < 1) return GVX_ERR_INVALID_ARG;
    GemmParams g{};
    g.kmajor = kmajor != 0;
    g.amap = kmajor ? RowMap{K, 0, (long)M} : RowMap{M, 0, (long)K};
    g.wmap = RowMap{K, 0, (long)N};
    g.M = M; g.N = N; g.K = K;
    const int splitk = train_gemm_splitk(M, N, K, have_scratch != 0, scratch_bytes);
    if (splitk > 1) set_splitk(g, splitk);   // (what launch_gemm_splitk does before it plans)
    const GemmPlan pl = plan_gemm(g);
    *tile_out = pl.tile; *rows_big_out = pl.rows_big; *k_pieces_out = g.splitk;
    return pl.err == hipSuccess ? GVX_OK : GVX_ERR_INVALID_ARG;
}

// ... and of a batch of `slices` row-major products of that shape in one launch (GemmParams::slices: the Winograd layers of the
// Postnet); slices = 1 is the plain product.  Host arithmetic only, not in the public header.
int gvx_debug_gemm_plan_batched(int M, int N, int K, int slices, int* tile_out, int* rows_big_out) {
    if (!tile_out || !rows_big_out || M < 1 || N < 1 || K < 1 || slices < 1) return GVX_ERR_INVALID_ARG;
    GemmParams g{};
    g.amap = RowMap{M, 0, (long)K};
    g.M = M; g.N = N; g.K = K;
    g.slices = slices; g.a_slice = (long)M * K; g.w_slice = (long)N * K; g.c_slice = (long)M * N;
    const GemmPlan pl = plan_gemm(g);
    *tile_out = pl.tile; *rows_big_out = pl.rows_big;
    return pl.err == hipSuccess ? GVX_OK : GVX_ERR_INVALID_ARG;
}

// C[m][n] = sum_k A[m*lda + k] * W[n*ldw + k] (+ bias[n]);  K % 4 == 0
int gvx_train_gemm_nt(const float* A, long lda, const float* W, long ldw, float* C, long ldc, int M, int N, int K, const float* bias,
                      float* scratch, size_t scratch_bytes, void* stream) {
    if (!A || !W || !C || M < 1 || N < 1 || K < 4 || (K & 3)) return tfail(GVX_ERR_INVALID_ARG, "gemm_nt: null argument or K not a positive multiple of 4");
    GemmParams g{};
    g.A = A; g.amap = RowMap{M, 0, lda};
    g.W = W; g.ldw = ldw;
    g.C = C; g.cmap = RowMap{M, 0, ldc};
    g.bias = bias; g.M = M; g.N = N; g.K = K; g.act = ACT_NONE;
    // few output tiles and a long K (the per-step products of the backward: 32 rows x thousands of columns): split K over
    // enough workgroups to fill the chip, partial tiles in the caller's scratch, added in split order (deterministic)
    TR_TRY(launch_gemm_splitk(g, train_gemm_splitk(M, N, K, scratch != nullptr, scratch_bytes), scratch, (hipStream_t)stream));
    return GVX_OK;
}
// C[m][n] = sum_r A[r * lda + m] * Bm[r * ldb + n]: the weight-gradient form, both operands as they lie in memory
int gvx_train_gemm_tn(const float* A, long lda, const float* Bm, long ldb, float* C, long ldc, int M, int N, long rows, float* scratch,
                      size_t scratch_bytes, void* stream) {
    if (!A || !Bm || !C || M < 1 || N < 1 || rows < 1 || rows > (1L << 30)) return tfail(GVX_ERR_INVALID_ARG, "gemm_tn: bad argument");
    GemmParams g{};
    g.kmajor = true;
    g.A = A; g.amap = RowMap{(int)rows, 0, lda};
    g.W = Bm; g.wmap = RowMap{(int)rows, 0, ldb};
    g.C = C; g.cmap = RowMap{M, 0, ldc};
    g.M = M; g.N = N; g.K = (int)rows; g.act = ACT_NONE;
    TR_TRY(launch_gemm_splitk(g, train_gemm_splitk(M, N, (int)rows, scratch != nullptr, scratch_bytes), scratch, (hipStream_t)stream));
    return GVX_OK;
}
// dst[c][r] = src[r * ld_src + c] for r < rows (0 for rows <= r < rows_p);  dst rows are rows_p long
int gvx_train_transpose(const float* src, long ld_src, float* dst, long rows, int cols, long rows_p, void* stream) {
    if (!src || !dst || rows < 1 || cols < 1 || rows_p < rows) return tfail(GVX_ERR_INVALID_ARG, "transpose: bad argument");
    if (ld_src != cols) return tfail(GVX_ERR_UNSUPPORTED, "transpose: source must be dense (ld == cols)");
    hipLaunchKernelGGL(transpose_pad_kernel, dim3((unsigned)((rows_p + 31) / 32), (cols + 31) / 32), dim3(256), 0, (hipStream_t)stream, src, dst, rows, cols, rows_p);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}
int gvx_train_colsum(const float* X, long rows, int C, float* out, void* stream) {
    if (!X || !out || rows < 1 || C < 1) return tfail(GVX_ERR_INVALID_ARG, "colsum: bad argument");
    launch_col_reduce(X, nullptr, rows, C, out, nullptr, (hipStream_t)stream);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}
int gvx_train_axpby(const float* a, long lda, float alpha, const float* b, long ldb, float beta, float* y, long ldy, long rows, int cols, void* stream) {
    if (!a || !y || rows < 1 || cols < 1) return tfail(GVX_ERR_INVALID_ARG, "axpby: bad argument");
    hipLaunchKernelGGL(axpby_kernel, dim3(blocks_for(rows * cols)), dim3(256), 0, (hipStream_t)stream, a, lda, alpha, b, ldb, beta, y, ldy, rows, cols);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}
int gvx_train_relu_dropout_backward(const float* dy, const float* act_out, const uint8_t* keep, float scale, long n, float* dz, void* stream) {
    if (!dy || !act_out || !keep || !dz || n < 1) return tfail(GVX_ERR_INVALID_ARG, "relu_dropout_backward: bad argument");
    hipLaunchKernelGGL(relu_drop_bwd_kernel, dim3(blocks_for(n)), dim3(256), 0, (hipStream_t)stream, dy, act_out, keep, scale, n, dz);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}
int gvx_train_unblock(const float* blocked, float* rows_out, long n_slots, int B, int K, void* stream) {
    if (!blocked || !rows_out || n_slots < 1 || B < 1 || K < 8 || (K & 7)) return tfail(GVX_ERR_INVALID_ARG, "unblock: bad argument");
    hipLaunchKernelGGL(unblock_kernel, dim3(blocks_for(n_slots * B * K)), dim3(256), 0, (hipStream_t)stream, blocked, rows_out, n_slots, B, K);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}
int gvx_train_embedding_backward(const int64_t* tokens, const float* dx, long n_tokens_in_batch, int E, int n_rows, float* demb, void* stream) {
    if (!tokens || !dx || !demb || n_tokens_in_batch < 1 || E < 1 || n_rows < 1) return tfail(GVX_ERR_INVALID_ARG, "embedding_backward: bad argument");
    hipLaunchKernelGGL(embedding_bwd_kernel, dim3(n_rows), dim3(256), 0, (hipStream_t)stream, tokens, dx, n_tokens_in_batch, E, n_rows, demb);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}
int gvx_train_sqnorm_many(const gvx_tensor_ref* refs_device, int n_tensors, double* scratch, double* sumsq_out, void* stream) {
    if (!refs_device || !scratch || !sumsq_out || n_tensors < 1) return tfail(GVX_ERR_INVALID_ARG, "sqnorm_many: bad argument");
    hipLaunchKernelGGL(sqnorm_many_kernel, dim3(SQN_BLOCKS, n_tensors), dim3(256), 0, (hipStream_t)stream, refs_device, scratch);
    hipLaunchKernelGGL(sqnorm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, SQN_BLOCKS * n_tensors, sumsq_out);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}
size_t gvx_train_sqnorm_scratch_bytes(int n_tensors) { return n_tensors < 1 ? 0 : (size_t)SQN_BLOCKS * n_tensors * sizeof(double); }
int gvx_train_adam_step_many(const gvx_adam_ref* refs_device, int n_tensors, float grad_scale, float lr, float weight_decay, float beta1,
                             float beta2, float eps, int step, void* stream) {
    if (!refs_device || n_tensors < 1 || step < 1) return tfail(GVX_ERR_INVALID_ARG, "adam_step_many: bad argument");
    // (bias corrections in double, as torch.optim.Adam computes them in Python: 1 - 0.999f in fp32 is 1.3e-5 off at step 1)
    const float bc1 = (float)(1.0 - std::pow((double)beta1, (double)step)), bc2s = (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step));
    hipLaunchKernelGGL(adam_many_kernel, dim3(128, n_tensors), dim3(256), 0, (hipStream_t)stream, refs_device, grad_scale, lr, weight_decay, beta1, beta2,
                       eps, bc1, bc2s);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}

}  // extern "C"
