// Internal to the training sources (train_conv.hip: conv + BatchNorm layer and criterion backward; train_ops.hip: the whole-sequence
// primitives; train_bptt_decoder.hip / train_bptt_encoder.hip: the two recurrences); not installed.  What more than one of them
// uses, and nothing else.
#pragma once
#include "../../include/genvox_amd.h"
#include "gvx_kernels.h"

namespace gvx {

inline int tfail(int code, const char* msg) { return set_error(code, msg); }
// "<expr> failed: <HIP's error string>" as this thread's error, returns GVX_ERR_HIP (the message buffer lives in train_ops.hip)
int tfail_hip(const char* expr, hipError_t e);
#define TR_TRY(expr)                                              \
    do {                                                          \
        hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return gvx::tfail_hip(#expr, _e);   \
    } while (0)

#define TR_STAMP(flag, k, i) do { if (flag) GVX_STAMP(k, i); } while (0)

inline int blocks_for(long n) { long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }

// Split-K factor for a product with `tiles` output tiles of 64 x 128 and a long K (weight gradients: few outputs, thousands of
// rows to sum over): the tiles run in rounds of 256 (one per CU), so the time goes like ceil(tiles * s / 256) / s - the
// smallest s <= 8 that minimises it, pieces of at least 256 k.  1 = no split.
inline int choose_splitk(long tiles, int K) {
    if (tiles >= 256 || K < 512) return 1;
    int best = 1;
    double best_t = 1.0;   // (tiles < 256: one round at s = 1)
    for (int sp = 2; sp <= 8 && K / sp >= 256; ++sp) {
        const double t = (double)((tiles * sp + 255) / 256) / sp;
        if (t < best_t - 1e-9) { best_t = t; best = sp; }
    }
    return best;
}

// Row lanes of the 32-column x 32-row-lane walk that col_reduce_kernel (train_ops.hip) and bn_stats_kernel (train_conv.hip) share.
constexpr int CR_LANES = 32;
// sum_x[c] = sum over the rows of X [rows][C]; with Y and sum_xy also sum_xy[c] = sum of X * Y.  Double accumulation, fixed order
// (col_reduce_kernel, train_ops.hip).  A launch only: the caller looks at hipGetLastError().
void launch_col_reduce(const float* X, const float* Y, long rows, int C, float* sum_x, float* sum_xy, hipStream_t s);

#if defined(__HIPCC__)
// One LSTM cell backwards from its gate pre-activations (torch gate order i, f, g, o) and previous cell state: both BPTT walks.
__device__ __forceinline__ void lstm_cell_bwd_one(float dh, float dcn, float pi, float pf, float pg, float po, float cp, float& gi, float& gf,
                                                  float& gg_, float& go, float& dc_prev) {
    const float ig = 1.f / (1.f + expf(-pi)), fg = 1.f / (1.f + expf(-pf)), gg = tanhf(pg), og = 1.f / (1.f + expf(-po));
    const float c = fg * cp + ig * gg, tc = tanhf(c);
    const float d_o = dh * tc;
    const float dc = dh * og * (1.f - tc * tc) + dcn;
    gi = dc * gg * ig * (1.f - ig);
    gf = dc * cp * fg * (1.f - fg);
    gg_ = dc * ig * (1.f - gg * gg);
    go = d_o * og * (1.f - og);
    dc_prev = dc * fg;
}
#endif

#ifdef GVX_STAMPS
// diagnostic build only: gvx_stamps is file-local, and the two walks stamp different rows of it in different sources (row 0:
// bptt_attention_kernel, row 1: the encoder walk).  train_bptt_decoder.hip hands out its row 0; gvx_debug_read_stamps_train
// (train_bptt_encoder.hip) puts it in front of its own row 1
hipError_t read_stamps_decoder_bptt(unsigned long long* host32);
#endif

}  // namespace gvx
