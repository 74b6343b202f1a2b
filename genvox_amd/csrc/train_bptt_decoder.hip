// Back-propagation through the decoder loop in ONE call (gvx_train_decoder_bptt): three launches per step, issued from
// here - not ~20 primitives per step strung together by the host mirror (round 3, first version: 2.2 ms per step of
// launch overhead and small-kernel time).  Step t, walking down from T - 1:
//   A  bptt_attention_kernel  (G position chunks x B rows): gradient of the context -> attention weights -> energies ->
//      query / processed memory / location layers, and through the location convolution into the previous and cumulative
//      weights.  Everything of a row is local to its positions except a few sums over positions, which leave the kernel as
//      per-chunk partials that their consumers add in chunk order (deterministic, no atomics).
//   B  bptt_cells_kernel: attention-LSTM cell of step t and decoder-LSTM cell of step t - 1 backwards (the decoder cell of
//      step t - 1 only needs the decoder cell of step t: the two recurrences overlap exactly like in the forward loop).
//   C  the two products dgates x [W_ih | W_hh] on the weight-streaming skinny kernel of the forward path (skinny.hip,
//      mode 2) with the matrices transposed and packed in MFMA-fragment order on the device at the start of the call; K
//      is cut in two so that the default layer sizes give 256 equal tiles (48 + 80 row tiles x 2 K halves, 256 KB each).
// The softmax term sum_l w_l dw_l is taken as  w . (dw_next + G) + dctx . ctx(t)  (ctx(t) = sum_l w_l memory_l is on the
// tape): a chunk does not need the other chunks' dw.  A loss that looks at the alignments themselves (the guided attention loss,
// train_guided.hip) hands its d loss / d w_t to gvx_train_decoder_bptt_ext, where it joins dw_next + G of step t - in the softmax
// backward only, not in what the location convolution passes to earlier steps.  The context path of the memory gradient,
// sum_t w_t (x) dctx_t, is one kernel after the loop.  What is not on the recurrence - the Prenet columns of the attention LSTM, all weight gradients -
// stays with the host mirror as whole-sequence GEMMs.
#include "train_internal.h"

#include <cstring>

namespace gvx {
namespace {

constexpr int BP_THREADS = 256;
constexpr int BP_GMAX = 8;   // position chunks per batch row

inline int bptt_chunks(int L) { int g = (L + 3) / 4; return g < 1 ? 1 : (g > BP_GMAX ? BP_GMAX : g); }
inline int round32(int x) { return (x + 31) / 32 * 32; }

struct BpttAttn {
    int B, L, E, a, F, kl, G;
    const float* dhc_ctx; long dhc_ld;        // d loss / d ctx(t) through the projection: row b at dhc_ctx + b * dhc_ld
    const float* yd0; const float* yd1; int yd_ld, yd_ctx;   // decoder-cell products of step t (two K halves): context columns at yd_ctx
    const float* ya0; const float* ya1; int ya_ld;           // attention-cell products of step t + 1 (nullptr at t = T - 1): context columns at 0
    const float* ctx; long ctx_bs;            // ctx(t), row b at ctx + b * ctx_bs
    const float* w; const float* w_prev; const float* wcum;   // alignments of step t, t - 1 (nullptr at t = 0), cumulative before t: [B][L]
    const float* q;                           // [B][a] query of step t
    const float* memory; const float* pm; const float* v; const float* lw; const float* ld;
    const float* dw_in; const float* gc_in;   // [B][G][L] partials written by step t + 1
    float* dw_out; float* gc_out;             // [B][G][L] partials of this step
    float* dq_part;                           // [B][G][a]
    float* dctx_out;                          // [B][E] (dctx_all[t])
    float* dpm;                               // [B][L][a]  accumulated
    float* dv_acc; float* dld_acc; float* dlw_acc;   // [B][G][a], [B][G][a][F], [B][G][F * 2 * kl]  accumulated
    int stamp;                                // stamps build: this launch records its phase times
    const float* dw_ext; long dw_ext_bs;      // bptt_attention_kernel<true> only: d loss / d w_t taken directly on the alignments, row b at dw_ext + b * dw_ext_bs
};

// LDS rows of the location filters are FS = 32 floats whatever F is (zeros past F): every loop over filters is a compile-time
// 32-iteration loop, its operands in registers / consecutive LDS words
constexpr int BA_THREADS = 512;
constexpr int BA_FS = 32;
// items a thread of bptt_attention_kernel takes per pass: energies, dense-gradient groups (8 filters of one attention dim),
// convolution-gradient items.  More than BA_NB* x BA_THREADS items: further passes, which reload their operands
constexpr int BA_NBE = 8, BA_NBD = 2, BA_NBC = 4;
inline size_t bptt_attn_lds_floats(int L, int E, int a, int F, int kl, int G) {
    const int CH = (L + G - 1) / G;
    return (size_t)E + 2 * L + BA_THREADS + 2 * (CH + kl - 1) + (size_t)2 * kl * (BA_FS + 1) + (size_t)a * (BA_FS + 1) + (size_t)CH * BA_FS + CH +
           (size_t)2 * CH * a + (size_t)CH * BA_FS + (size_t)CH * 2 * kl + 8;
}

constexpr size_t BA_LDS_LIMIT = 160 * 1024;

__device__ __forceinline__ float fast_tanh(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * x) + 1.f); }

// EXT: a gradient on the alignments themselves (gvx_train_decoder_bptt_ext) joins dw_next + G.  A template parameter, not a branch:
// the instantiation without it is the kernel as it was, instruction for instruction.
template <bool EXT>
__global__ __launch_bounds__(BA_THREADS) void bptt_attention_kernel(BpttAttn p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int L = p.L, E = p.E, a = p.a, F = p.F, kl = p.kl, G = p.G, pad = (kl - 1) / 2;
    constexpr int FS = BA_FS, LDF = BA_FS + 1;
    const int CH = (L + G - 1) / G, l0 = g * CH;
    const int n = max(0, min(L, l0 + CH) - l0);   // positions of this chunk (0: the chunk only passes its partial buffers on)
    const int LW = CH + kl - 1;
    float* locf = sm;                  // [CH][FS]        zeros past F          (16-byte aligned rows: read as float4)
    float* dlocf = locf + CH * FS;     // [CH][FS]
    float* dc = dlocf + CH * FS;       // [E]
    float* dwg = dc + E;               // [L]   dw_next + G (+ the external term) of the whole row
    float* wrow = dwg + L;             // [L]   alignment of step t
    float* red = wrow + L;             // [BA_THREADS]
    float* win = red + BA_THREADS;     // [2][LW] previous / cumulative weights at positions l0 - pad ...
    float* lws = win + 2 * LW;         // [2 kl][FS + 1]  lw[f][c][j] at (c kl + j, f), zeros past F
    float* lds_ = lws + 2 * kl * LDF;  // [a][FS + 1]     zeros past F
    float* des = lds_ + a * LDF;       // [CH]
    float* du = des + CH;              // [CH][a]
    float* dvt = du + CH * a;          // [CH][a]
    float* t1 = dvt + CH * a;          // [CH][2][kl]
    TR_STAMP(p.stamp, 0, 0);

    // ---- every global operand that does not depend on this launch's arithmetic is requested up front (a dependent round trip
    // to memory the previous launch wrote costs ~1 us; the first version of this kernel had a dozen of them in a row)
    constexpr int NBE = BA_NBE, NBD = BA_NBD, NBC = BA_NBC;   // items per thread and batch: energies, dense-gradient groups, conv-gradient items
    const int n_en = n * a, n_dg = a * (FS / 8), n_cv = F * 2 * kl;
    float e_pm[NBE], e_dpm[NBE];
#pragma unroll
    for (int u = 0; u < NBE; ++u) {
        const int i = tid + u * BA_THREADS;
        e_pm[u] = e_dpm[u] = 0.f;
        if (i < n_en) { const int li = i / a, d = i - li * a; const long o = ((long)b * L + l0 + li) * a + d; e_pm[u] = p.pm[o]; e_dpm[u] = p.dpm[o]; }
    }
    float* dldb = p.dld_acc + ((long)b * G + g) * a * F;
    float d_old[NBD][8];
#pragma unroll
    for (int u = 0; u < NBD; ++u) {
        const int grp = tid + u * BA_THREADS, d = grp >> 2, f0 = (grp & 3) * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) d_old[u][k] = (grp < n_dg && f0 + k < F) ? dldb[(long)d * F + f0 + k] : 0.f;
    }
    float* dlwb = p.dlw_acc + ((long)b * G + g) * F * 2 * kl;
    float c_old[NBC];
#pragma unroll
    for (int u = 0; u < NBC; ++u) { const int i = tid + u * BA_THREADS; c_old[u] = i < n_cv ? dlwb[i] : 0.f; }
    const long part_o = ((long)b * G + g) * L;
    float dv_old = 0.f, gq_ = 0.f, gv_ = 0.f;
    if (tid < a) { dv_old = p.dv_acc[((long)b * G + g) * a + tid]; }
    if (BA_THREADS % a == 0) { gq_ = p.q[(long)b * a + tid % a]; gv_ = p.v[tid % a]; }
    for (int e = tid; e < E; e += BA_THREADS) {
        float v = p.dhc_ctx[(long)b * p.dhc_ld + e] + p.yd0[(long)b * p.yd_ld + p.yd_ctx + e] + p.yd1[(long)b * p.yd_ld + p.yd_ctx + e];
        if (p.ya0) v += p.ya0[(long)b * p.ya_ld + e] + p.ya1[(long)b * p.ya_ld + e];
        dc[e] = v;
        if (g == 0) p.dctx_out[(long)b * E + e] = v;
    }
    for (int l = tid; l < L; l += BA_THREADS) {
        float pd[BP_GMAX], pg[BP_GMAX];
#pragma unroll
        for (int gg = 0; gg < BP_GMAX; ++gg) {
            pd[gg] = gg < G ? p.dw_in[((long)b * G + gg) * L + l] : 0.f;
            pg[gg] = gg < G ? p.gc_in[((long)b * G + gg) * L + l] : 0.f;
        }
        float ex = 0.f;
        if (EXT) ex = p.dw_ext[(long)b * p.dw_ext_bs + l];
        float s = 0.f;
#pragma unroll
        for (int gg = 0; gg < BP_GMAX; ++gg) s += pd[gg] + pg[gg];
        // the external term enters here and nowhere else: ssum and des read dwg, dw_out / gc_out (the location convolution's
        // gradient to earlier steps) do not
        if (EXT) s += ex;
        dwg[l] = s;
        wrow[l] = p.w[(long)b * L + l];
    }
    for (int i = tid; i < 2 * LW; i += BA_THREADS) {
        const int c = i / LW, ii = i - c * LW, l = l0 + ii - pad;
        float v = 0.f;
        if (l >= 0 && l < L) v = c == 0 ? (p.w_prev ? p.w_prev[(long)b * L + l] : 0.f) : p.wcum[(long)b * L + l];
        win[i] = v;
    }
    for (int i = tid; i < 2 * kl * FS; i += BA_THREADS) {   // lw [F][2][kl] -> rows (c, j), filters along the row
        const int f = i & (FS - 1), cj = i >> 5;
        lws[cj * LDF + f] = f < F ? p.lw[(long)f * 2 * kl + cj] : 0.f;
    }
    for (int i = tid; i < a * FS; i += BA_THREADS) {
        const int f = i & (FS - 1), d = i >> 5;
        lds_[d * LDF + f] = f < F ? p.ld[(long)d * F + f] : 0.f;
    }
    __syncthreads();
    TR_STAMP(p.stamp, 0, 1);
    // s = sum_l w_l dw_l = w . (dw_next + G) + dctx . ctx(t)
    {
        float part = 0.f;
        for (int e = tid; e < E; e += BA_THREADS) part += dc[e] * p.ctx[(long)b * p.ctx_bs + e];
        for (int l = tid; l < L; l += BA_THREADS) part += wrow[l] * dwg[l];
        red[tid] = part;
        __syncthreads();
        for (int o = BA_THREADS / 2; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    }
    const float ssum = red[0];
    TR_STAMP(p.stamp, 0, 2);
    // dw and de of the chunk's positions: one wave per position, lanes over the memory channels
    {
        const int wave = tid >> 6, lane = tid & 63;
        for (int li = wave; li < n; li += BA_THREADS / 64) {
            const float* mrow = p.memory + ((long)b * L + l0 + li) * E;
            float acc = 0.f;
#pragma unroll 8
            for (int e = lane; e < E; e += 64) acc += dc[e] * mrow[e];
            for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
            if (lane == 0) des[li] = wrow[l0 + li] * (acc + dwg[l0 + li] - ssum);
        }
    }
    TR_STAMP(p.stamp, 0, 3);
    // location features of the chunk (recomputed): locf[l][f] = sum_{c,j} in_c[l + j - pad] lw[f][c][j]
    for (int i = tid; i < n * FS; i += BA_THREADS) {
        const int li = i >> 5, f = i & (FS - 1);
        float acc = 0.f;
        for (int c = 0; c < 2; ++c) {
#pragma unroll 8
            for (int j = 0; j < kl; ++j) acc += win[c * LW + li + j] * lws[(c * kl + j) * LDF + f];
        }
        locf[i] = acc;   // (filters past F: zero weights -> 0)
    }
    __syncthreads();
    TR_STAMP(p.stamp, 0, 4);
    // energies backwards: u = q + locf ld^T + pm, th = tanh(u), du = de v (1 - th^2).  A thread keeps the dense row of its
    // attention dim in registers while that dim does not change (a | 512: never)
    {
        float ldr[FS];
        int d_have = -1;
        float qd = gq_, vd = gv_;
        for (int i0 = tid; i0 < n_en; i0 += NBE * BA_THREADS) {
            if (i0 != tid) {   // later batches (more than 8 items per thread): their operands are requested here
#pragma unroll
                for (int u = 0; u < NBE; ++u) {
                    const int i = i0 + u * BA_THREADS;
                    if (i < n_en) { const int li = i / a, d = i - li * a; const long o = ((long)b * L + l0 + li) * a + d; e_pm[u] = p.pm[o]; e_dpm[u] = p.dpm[o]; }
                }
            }
#pragma unroll
            for (int u = 0; u < NBE; ++u) {
                const int i = i0 + u * BA_THREADS;
                if (i < n_en) {
                    const int li = i / a, d = i - li * a;
                    if (d != d_have) {
#pragma unroll
                        for (int f = 0; f < FS; ++f) ldr[f] = lds_[d * LDF + f];
                        if (BA_THREADS % a != 0) { qd = p.q[(long)b * a + d]; vd = p.v[d]; }
                        d_have = d;
                    }
                    float locd = 0.f;
#pragma unroll
                    for (int f = 0; f < FS; ++f) locd += locf[li * FS + f] * ldr[f];
                    const float th = fast_tanh(qd + locd + e_pm[u]);
                    const float e_ = des[li];
                    const float gq = e_ * vd * (1.f - th * th);
                    du[i] = gq;
                    dvt[i] = e_ * th;
                    p.dpm[((long)b * L + l0 + li) * a + d] = e_dpm[u] + gq;
                }
            }
        }
    }
    __syncthreads();
    TR_STAMP(p.stamp, 0, 5);
    for (int d = tid; d < a; d += BA_THREADS) {
        if (d != tid) dv_old = p.dv_acc[((long)b * G + g) * a + d];
        float sq = 0.f, sv = 0.f;
#pragma unroll 4
        for (int li = 0; li < n; ++li) { sq += du[li * a + d]; sv += dvt[li * a + d]; }
        p.dq_part[((long)b * G + g) * a + d] = sq;
        p.dv_acc[((long)b * G + g) * a + d] = dv_old + sv;
    }
    TR_STAMP(p.stamp, 0, 6);
    // d location_dense[d][f] += sum_l du[l][d] locf[l][f]: a thread owns 8 consecutive filters of one attention dim
    for (int g0 = tid; g0 < n_dg; g0 += NBD * BA_THREADS) {
#pragma unroll
        for (int u = 0; u < NBD; ++u) {
            const int grp = g0 + u * BA_THREADS;
            if (grp < n_dg) {
                const int d = grp >> 2, f0 = (grp & 3) * 8;
                if (g0 != tid) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) d_old[u][k] = f0 + k < F ? dldb[(long)d * F + f0 + k] : 0.f;
                }
                float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
                for (int li = 0; li < n; ++li) {
                    const float dv_ = du[li * a + d];
                    const float4 x0 = *reinterpret_cast<const float4*>(locf + li * FS + f0), x1 = *reinterpret_cast<const float4*>(locf + li * FS + f0 + 4);
                    acc[0] += dv_ * x0.x; acc[1] += dv_ * x0.y; acc[2] += dv_ * x0.z; acc[3] += dv_ * x0.w;
                    acc[4] += dv_ * x1.x; acc[5] += dv_ * x1.y; acc[6] += dv_ * x1.z; acc[7] += dv_ * x1.w;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (f0 + k < F) dldb[(long)d * F + f0 + k] = d_old[u][k] + acc[k];
            }
        }
    }
    TR_STAMP(p.stamp, 0, 7);
    for (int i = tid; i < n * FS; i += BA_THREADS) {   // dlocf[l][f] = sum_d du[l][d] ld[d][f]
        const int li = i >> 5, f = i & (FS - 1);
        float acc = 0.f;
#pragma unroll 8
        for (int d = 0; d < a; ++d) acc += du[li * a + d] * lds_[d * LDF + f];
        dlocf[i] = acc;
    }
    __syncthreads();
    TR_STAMP(p.stamp, 0, 8);
    for (int i = tid; i < n * 2 * kl; i += BA_THREADS) {   // t1[l][c][j] = sum_f dlocf[l][f] lw[f][c][j]
        const int li = i / (2 * kl), cj = i - li * 2 * kl;
        float acc = 0.f;
#pragma unroll
        for (int f = 0; f < FS; ++f) acc += dlocf[li * FS + f] * lws[cj * LDF + f];
        t1[i] = acc;
    }
    TR_STAMP(p.stamp, 0, 9);
    // d location_conv[f][c][j] += sum_l dlocf[l][f] in_c[l + j - pad]
    for (int i0 = tid; i0 < n_cv; i0 += NBC * BA_THREADS) {
#pragma unroll
        for (int u = 0; u < NBC; ++u) {
            const int i = i0 + u * BA_THREADS;
            if (i < n_cv) {
                if (i0 != tid) c_old[u] = dlwb[i];
                const int f = i / (2 * kl), cj = i - f * 2 * kl, c = cj / kl, j = cj - c * kl;
                float acc = 0.f;
#pragma unroll 4
                for (int li = 0; li < n; ++li) acc += dlocf[li * FS + f] * win[c * LW + li + j];
                dlwb[i] = c_old[u] + acc;
            }
        }
    }
    __syncthreads();
    TR_STAMP(p.stamp, 0, 10);
    // d in_c[l'] = sum over the chunk's l of t1[l][c][l' - l + pad]: c = 0 -> previous weights (next step's dw_next),
    // c = 1 -> cumulative weights (added to G for all earlier steps)
    for (int i = tid; i < 2 * L; i += BA_THREADS) {
        const int c = i / L, lt = i - c * L;
        const float old = c == 0 ? 0.f : p.gc_in[part_o + lt];
        float acc = 0.f;
        const int li_lo = max(0, lt + pad - (kl - 1) - l0), li_hi = min(n, lt + pad - l0 + 1);   // 0 <= lt - (l0 + li) + pad < kl
        for (int li = li_lo; li < li_hi; ++li) acc += t1[(li * 2 + c) * kl + lt - (l0 + li) + pad];
        if (c == 0) p.dw_out[part_o + lt] = acc;
        else p.gc_out[part_o + lt] = old + acc;
    }
    TR_STAMP(p.stamp, 0, 11);
}

struct BpttCells {
    int B, A, D, E, a, G;
    // attention cell of step t (att == 0: skipped)
    int att;
    const float* yd0; const float* yd1; int yd_ld;      // decoder-cell products of step t: h_a columns at 0, h_d columns at A + E
    const float* ya0; const float* ya1; int ya_ld;      // attention-cell products of step t + 1 (nullptr at t = T - 1): h_a columns at E
    const float* dq_part; const float* wq;              // [B][G][a], [a][A]
    const float* pre_a; const float* c_a; const uint8_t* keep_a; float scale_a;   // step t: [B][A][4], [B][A], [B][A]
    float* dc_a;                                        // [B][A] state
    float* dga; float* xa_blk; float* dq_out;           // dga_all[t] [B][4A], blocked copy, dq_all[t] [B][a]
    // decoder cell of step t - 1 (dec == 0: skipped)
    int dec; int have_yd;                               // have_yd == 0: no later step (t - 1 = T - 1)
    const float* dhc_hd; long dhc_ld;                   // dhc_all[t - 1], h_d columns at 0
    const float* pre_d; const float* c_d; const uint8_t* keep_d; float scale_d;
    float* dc_d;
    float* dgd; float* xd_blk;
};


__global__ __launch_bounds__(BP_THREADS) void bptt_cells_kernel(BpttCells p) {
    __shared__ float dq[256];
    const int b = blockIdx.y, tid = threadIdx.x, j = blockIdx.x * BP_THREADS + tid;
    const int A = p.A, D = p.D, B = p.B;
    const bool att_block = p.att && (int)blockIdx.x * BP_THREADS < A;   // block-uniform
    if (att_block) {
        for (int d = tid; d < p.a; d += BP_THREADS) {
            float s = 0.f;
            for (int g = 0; g < p.G; ++g) s += p.dq_part[((long)b * p.G + g) * p.a + d];
            dq[d] = s;
            if (blockIdx.x == 0) p.dq_out[(long)b * p.a + d] = s;
        }
        __syncthreads();
    }
    if (j < A) {
        if (!p.att) return;
        float dh = p.yd0[(long)b * p.yd_ld + j] + p.yd1[(long)b * p.yd_ld + j];
        if (p.ya0) dh += p.ya0[(long)b * p.ya_ld + p.E + j] + p.ya1[(long)b * p.ya_ld + p.E + j];
        float hq = 0.f;
#pragma unroll 16
        for (int d = 0; d < p.a; ++d) hq += dq[d] * p.wq[(long)d * A + j];
        dh += hq;
        dh = p.keep_a[(long)b * A + j] ? dh * p.scale_a : 0.f;
        const float4 pr = *reinterpret_cast<const float4*>(p.pre_a + ((long)b * A + j) * 4);
        float gi, gf, gg, go, dcp;
        lstm_cell_bwd_one(dh, p.dc_a[(long)b * A + j], pr.x, pr.y, pr.z, pr.w, p.c_a[(long)b * A + j], gi, gf, gg, go, dcp);
        p.dc_a[(long)b * A + j] = dcp;
        const float gv[4] = {gi, gf, gg, go};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = q * A + j;
            p.dga[(long)b * 4 * A + k] = gv[q];
            p.xa_blk[(long)(k >> 3) * B * 8 + b * 8 + (k & 7)] = gv[q];
        }
    } else if (j < A + D) {
        if (!p.dec) return;
        const int jd = j - A;
        float dh = p.dhc_hd[(long)b * p.dhc_ld + jd];
        if (p.have_yd) dh += p.yd0[(long)b * p.yd_ld + A + p.E + jd] + p.yd1[(long)b * p.yd_ld + A + p.E + jd];
        dh = p.keep_d[(long)b * D + jd] ? dh * p.scale_d : 0.f;
        const float4 pr = *reinterpret_cast<const float4*>(p.pre_d + ((long)b * D + jd) * 4);
        float gi, gf, gg, go, dcp;
        lstm_cell_bwd_one(dh, p.dc_d[(long)b * D + jd], pr.x, pr.y, pr.z, pr.w, p.c_d[(long)b * D + jd], gi, gf, gg, go, dcp);
        p.dc_d[(long)b * D + jd] = dcp;
        const float gv[4] = {gi, gf, gg, go};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int k = q * D + jd;
            p.dgd[(long)b * 4 * D + k] = gv[q];
            p.xd_blk[(long)(k >> 3) * B * 8 + b * 8 + (k & 7)] = gv[q];
        }
    }
}

// Transposed recurrent matrix in MFMA-fragment order: logical row n (< N, zero rows up to Np) = column col0 + n of
// [W_ih | W_hh] ([K][Kin], [K][H]), logical column k = gate row k (torch order).  out [Np/32][K/8][64][4]
__global__ void pack_transposed_frag_kernel(const float* w_ih, int Kin, const float* w_hh, int H, int col0, int N, int Np, int K, float* out) {
    const long total = (long)(Np / 32) * (K / 8) * 64;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int lane = (int)(i & 63);
        const long tk = i >> 6;
        const int kg = (int)(tk % (K / 8)), tile = (int)(tk / (K / 8));
        const int n = tile * 32 + (lane & 31), k0 = 8 * kg + 4 * (lane >> 5);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n < N) {
            const int col = col0 + n;
            const float* src = col < Kin ? w_ih + col : w_hh + (col - Kin);
            const long ld = col < Kin ? Kin : H;
            v.x = src[(long)(k0 + 0) * ld]; v.y = src[(long)(k0 + 1) * ld]; v.z = src[(long)(k0 + 2) * ld]; v.w = src[(long)(k0 + 3) * ld];
        }
        reinterpret_cast<float4*>(out)[i] = v;
    }
}

// wcum[t][b][l] = sum_{s < t} w[s][b][l], added in ascending order like the forward loop does
__global__ void cumulative_weights_kernel(const float* w, int T, long BL, float* wcum) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < BL; i += (long)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) { wcum[(long)t * BL + i] = s; s += w[(long)t * BL + i]; }
    }
}

// dmemory[b][l][e] = sum_t w[t][b][l] dctx[t][b][e]   (8 positions per workgroup)
__global__ __launch_bounds__(BP_THREADS) void memory_context_grad_kernel(const float* w, const float* dctx, int T, int B, int L, int E, float* dmemory) {
    const int b = blockIdx.y, l0 = blockIdx.x * 8, tid = threadIdx.x;
    for (int e = tid; e < E; e += BP_THREADS) {
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < T; ++t) {
            const float dv = dctx[((long)t * B + b) * E + e];
            const float* wr = w + ((long)t * B + b) * L;
#pragma unroll
            for (int i = 0; i < 8; ++i) acc[i] += wr[min(l0 + i, L - 1)] * dv;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (l0 + i < L) dmemory[((long)b * L + l0 + i) * E + e] = acc[i];
    }
}

struct BpttPlan {   // float offsets into the workspace
    size_t wa_t, wd_t, xa, xd, ya, yd, dc_a, dc_d, dwp, gcp, dqp, wcum, dv_acc, dld_acc, dlw_acc, total;
    int Na, Nd, G;
};
BpttPlan bptt_plan(const gvx_bptt_decoder_args& a) {
    BpttPlan p{};
    p.Na = round32(a.E + a.A); p.Nd = round32(a.A + a.E + a.D); p.G = bptt_chunks(a.L);
    size_t o = 0;
    auto take = [&](size_t floats) { size_t r = o; o += (floats + 63) / 64 * 64; return r; };
    p.wa_t = take((size_t)p.Na * 4 * a.A);
    p.wd_t = take((size_t)p.Nd * 4 * a.D);
    p.xa = take((size_t)a.B * 4 * a.A);
    p.xd = take((size_t)a.B * 4 * a.D);
    p.ya = take((size_t)2 * a.B * p.Na);
    p.yd = take((size_t)2 * a.B * p.Nd);
    p.dc_a = take((size_t)a.B * a.A);
    p.dc_d = take((size_t)a.B * a.D);
    p.dwp = take((size_t)2 * a.B * p.G * a.L);
    p.gcp = take((size_t)2 * a.B * p.G * a.L);
    p.dqp = take((size_t)a.B * p.G * a.a);
    p.wcum = take((size_t)a.T * a.B * a.L);
    p.dv_acc = take((size_t)a.B * p.G * a.a);
    p.dld_acc = take((size_t)a.B * p.G * a.a * a.F);
    p.dlw_acc = take((size_t)a.B * p.G * a.F * 2 * a.kl);
    p.total = o;
    return p;
}

int check_bptt_args(const gvx_bptt_decoder_args* a) {
    if (!a) return tfail(GVX_ERR_INVALID_ARG, "decoder_bptt: null argument block");
    if (a->B < 1 || a->B > 32 || a->L < 1 || a->T < 1) return tfail(GVX_ERR_UNSUPPORTED, "decoder_bptt: 1 <= B <= 32, L >= 1, T >= 1");
    if (a->A < 8 || a->D < 8 || (a->A % 8) || (a->D % 8) || (a->E % 8) || (a->P % 4) || a->a < 1 || a->a > 256 || a->F < 1 || a->F > 32 || a->kl < 1 || !(a->kl & 1))
        return tfail(GVX_ERR_UNSUPPORTED, "decoder_bptt: unsupported layer sizes");
    const void* need[] = {a->dhc_all, a->pre_a, a->pre_d, a->c_a_all, a->c_d_all, a->att_keep, a->dec_keep, a->q_all, a->ctx_all, a->w_all, a->memory, a->pm,
                          a->w_ih_a, a->w_hh_a, a->w_ih_d, a->w_hh_d, a->wq, a->v, a->loc_conv, a->loc_dense, a->dga_all, a->dgd_all, a->dq_all,
                          a->dctx_all, a->dpm, a->dmemory, a->dv, a->dloc_dense, a->dloc_conv};
    for (const void* q : need)
        if (!q) return tfail(GVX_ERR_INVALID_ARG, "decoder_bptt: null pointer in the argument block");
    const size_t lds = bptt_attn_lds_floats(a->L, a->E, a->a, a->F, a->kl, bptt_chunks(a->L)) * sizeof(float);
    if (lds > BA_LDS_LIMIT) return tfail(GVX_ERR_UNSUPPORTED, "decoder_bptt: a row's attention chunk does not fit the LDS (L or E too large)");
    return GVX_OK;
}

}  // namespace

#ifdef GVX_STAMPS
// diagnostic build only: row 0 of this source's stamp array (bptt_attention_kernel), for gvx_debug_read_stamps_train
hipError_t read_stamps_decoder_bptt(unsigned long long* host32) {
    return hipMemcpyFromSymbol(host32, HIP_SYMBOL(gvx_stamps), sizeof(unsigned long long) * 32);
}
#endif

}  // namespace gvx

using namespace gvx;

extern "C" {

// Host-only query for the tests (not part of the public header; touches no device): where gvx_train_decoder_bptt's kernels
// land for an argument block, from the functions and constants the launches use.  out[0..9] = position chunks G, positions per
// chunk CH, chunks that hold positions, passes of bptt_attention_kernel over the energies of a full chunk / over the
// dense-gradient groups / over the convolution-gradient items, 1 if a thread keeps its query and v element in registers
// (BA_THREADS % a == 0), Na, Nd, LDS bytes of the attention launch.  Returns the status gvx_train_decoder_bptt's argument check
// gives (out is filled whenever the sizes are positive, so that both sides of a limit can be read).
int gvx_debug_bptt_plan(const gvx_bptt_decoder_args* a, int* out) {
    if (!out) return GVX_ERR_INVALID_ARG;
    for (int i = 0; i < 10; ++i) out[i] = 0;
    const int rc = check_bptt_args(a);
    if (!a || a->L < 1 || a->a < 1 || a->F < 1 || a->kl < 1 || a->E < 0 || a->A < 1 || a->D < 1) return rc;
    auto passes = [](long items, int per_thread) { return (int)((items + (long)per_thread * BA_THREADS - 1) / ((long)per_thread * BA_THREADS)); };
    const int G = bptt_chunks(a->L), CH = (a->L + G - 1) / G;
    out[0] = G; out[1] = CH; out[2] = (a->L + CH - 1) / CH;
    out[3] = passes((long)(CH < a->L ? CH : a->L) * a->a, BA_NBE);
    out[4] = passes((long)a->a * (BA_FS / 8), BA_NBD);
    out[5] = passes((long)a->F * 2 * a->kl, BA_NBC);
    out[6] = BA_THREADS % a->a == 0 ? 1 : 0;
    out[7] = round32(a->E + a->A); out[8] = round32(a->A + a->E + a->D);
    out[9] = (int)(bptt_attn_lds_floats(a->L, a->E, a->a, a->F, a->kl, G) * sizeof(float));
    return rc;
}
size_t gvx_train_decoder_bptt_workspace_bytes(const gvx_bptt_decoder_args* a) {
    if (check_bptt_args(a) != GVX_OK) return 0;
    return bptt_plan(*a).total * sizeof(float);
}

int gvx_train_decoder_bptt(const gvx_bptt_decoder_args* ap, void* workspace, size_t workspace_bytes, void* stream) {
    return gvx_train_decoder_bptt_ext(ap, nullptr, 0, 0, workspace, workspace_bytes, stream);
}

int gvx_train_decoder_bptt_ext(const gvx_bptt_decoder_args* ap, const float* dw_ext, int64_t dw_ext_ts, int64_t dw_ext_bs, void* workspace,
                               size_t workspace_bytes, void* stream) {
    int rc = check_bptt_args(ap);
    if (rc != GVX_OK) return rc;
    const gvx_bptt_decoder_args& a = *ap;
    // (rows of dw_ext may not overlap: a stride below L between two steps or two batch rows is a mistake of the caller's)
    if (dw_ext && ((a.T > 1 && dw_ext_ts < a.L) || (a.B > 1 && dw_ext_bs < a.L) || dw_ext_ts < 0 || dw_ext_bs < 0))
        return tfail(GVX_ERR_INVALID_ARG, "decoder_bptt: dw_ext strides must be >= L between steps and between batch rows");
    const BpttPlan pl = bptt_plan(a);
    if (!workspace || workspace_bytes < pl.total * sizeof(float)) return tfail(GVX_ERR_WORKSPACE, "decoder_bptt: workspace too small");
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return tfail(GVX_ERR_WORKSPACE, "decoder_bptt: workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* ws = reinterpret_cast<float*>(workspace);
    const int B = a.B, L = a.L, T = a.T, A = a.A, D = a.D, E = a.E, P = a.P, G = pl.G, Na = pl.Na, Nd = pl.Nd;
    const int Ka = 4 * A, Kd = 4 * D;
    // (per call, not once per process: the attribute belongs to the current device)
    auto attention_kernel = dw_ext ? bptt_attention_kernel<true> : bptt_attention_kernel<false>;
    TR_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(attention_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const size_t lds_attn = bptt_attn_lds_floats(L, E, a.a, a.F, a.kl, G) * sizeof(float);

    // ---- before the loop: transposed matrices in fragment order, cumulative weights, cleared state and accumulators
    float* wa_t = ws + pl.wa_t; float* wd_t = ws + pl.wd_t;
    hipLaunchKernelGGL(pack_transposed_frag_kernel, dim3(blocks_for((long)(Na / 32) * (Ka / 8) * 64)), dim3(256), 0, s, a.w_ih_a, P + E, a.w_hh_a, A, P,
                       E + A, Na, Ka, wa_t);
    hipLaunchKernelGGL(pack_transposed_frag_kernel, dim3(blocks_for((long)(Nd / 32) * (Kd / 8) * 64)), dim3(256), 0, s, a.w_ih_d, A + E, a.w_hh_d, D, 0,
                       A + E + D, Nd, Kd, wd_t);
    float* wcum = ws + pl.wcum;
    hipLaunchKernelGGL(cumulative_weights_kernel, dim3(blocks_for((long)B * L)), dim3(256), 0, s, a.w_all, T, (long)B * L, wcum);
    TR_TRY(hipMemsetAsync(ws + pl.dc_a, 0, (pl.dqp - pl.dc_a) * sizeof(float), s));               // dc_a, dc_d, dw / G partials (both parities)
    TR_TRY(hipMemsetAsync(ws + pl.dv_acc, 0, (pl.total - pl.dv_acc) * sizeof(float), s));         // dv, dld, dlw accumulators
    TR_TRY(hipMemsetAsync(a.dpm, 0, (size_t)B * L * a.a * sizeof(float), s));
    float* ya0 = ws + pl.ya; float* ya1 = ya0 + (size_t)B * Na;
    float* yd0 = ws + pl.yd; float* yd1 = yd0 + (size_t)B * Nd;
    float* xa = ws + pl.xa; float* xd = ws + pl.xd;
    const size_t part = (size_t)B * G * L;

    // ---- slot t = T ... 0: attention chain of step t (t < T) and decoder cell of step t - 1 (t > 0)
    for (int t = T; t >= 0; --t) {
        const bool att = t < T, dec = t > 0;
        const int par = t & 1;   // partial buffers: step t reads parity (t + 1) & 1, writes parity t & 1
        if (att) {
            BpttAttn q{};
            q.B = B; q.L = L; q.E = E; q.a = a.a; q.F = a.F; q.kl = a.kl; q.G = G;
            q.dhc_ctx = a.dhc_all + (size_t)t * B * (D + E) + D; q.dhc_ld = D + E;
            q.yd0 = yd0; q.yd1 = yd1; q.yd_ld = Nd; q.yd_ctx = A;
            q.ya0 = t < T - 1 ? ya0 : nullptr; q.ya1 = ya1; q.ya_ld = Na;
            q.ctx = a.ctx_all + (long)t * (long)a.ctx_ts; q.ctx_bs = (long)a.ctx_bs;
            q.w = a.w_all + (size_t)t * B * L;
            q.w_prev = t > 0 ? a.w_all + (size_t)(t - 1) * B * L : nullptr;
            q.wcum = wcum + (size_t)t * B * L;
            q.q = a.q_all + (size_t)t * B * a.a;
            q.memory = a.memory; q.pm = a.pm; q.v = a.v; q.lw = a.loc_conv; q.ld = a.loc_dense;
            q.dw_in = ws + pl.dwp + (size_t)(par ^ 1) * part; q.gc_in = ws + pl.gcp + (size_t)(par ^ 1) * part;
            q.dw_out = ws + pl.dwp + (size_t)par * part; q.gc_out = ws + pl.gcp + (size_t)par * part;
            q.dq_part = ws + pl.dqp;
            q.dctx_out = a.dctx_all + (size_t)t * B * E;
            q.dpm = a.dpm; q.dv_acc = ws + pl.dv_acc; q.dld_acc = ws + pl.dld_acc; q.dlw_acc = ws + pl.dlw_acc;
            q.stamp = t == T / 2;
            if (dw_ext) { q.dw_ext = dw_ext + (long)t * (long)dw_ext_ts; q.dw_ext_bs = (long)dw_ext_bs; }
            hipLaunchKernelGGL(attention_kernel, dim3(G, B), dim3(BA_THREADS), lds_attn, s, q);
        }
        {
            BpttCells c{};
            c.B = B; c.A = A; c.D = D; c.E = E; c.a = a.a; c.G = G;
            c.att = att ? 1 : 0; c.dec = dec ? 1 : 0;
            c.yd0 = yd0; c.yd1 = yd1; c.yd_ld = Nd;
            c.ya0 = t < T - 1 ? ya0 : nullptr; c.ya1 = ya1; c.ya_ld = Na;
            c.dq_part = ws + pl.dqp; c.wq = a.wq;
            c.dc_a = ws + pl.dc_a; c.xa_blk = xa; c.scale_a = a.att_scale;
            if (att) {
                c.pre_a = a.pre_a + (size_t)t * B * Ka; c.c_a = a.c_a_all + (size_t)t * B * A; c.keep_a = a.att_keep + (size_t)t * B * A;
                c.dga = a.dga_all + (size_t)t * B * Ka; c.dq_out = a.dq_all + (size_t)t * B * a.a;
            }
            c.have_yd = t < T ? 1 : 0;
            c.dc_d = ws + pl.dc_d; c.xd_blk = xd; c.scale_d = a.dec_scale;
            if (dec) {
                c.dhc_hd = a.dhc_all + (size_t)(t - 1) * B * (D + E); c.dhc_ld = D + E;
                c.pre_d = a.pre_d + (size_t)(t - 1) * B * Kd; c.c_d = a.c_d_all + (size_t)(t - 1) * B * D; c.keep_d = a.dec_keep + (size_t)(t - 1) * B * D;
                c.dgd = a.dgd_all + (size_t)(t - 1) * B * Kd;
            }
            hipLaunchKernelGGL(bptt_cells_kernel, dim3((A + D + BP_THREADS - 1) / BP_THREADS, B), dim3(BP_THREADS), 0, s, c);
        }
        if (t == 0) break;   // the products of step 0's attention cell feed nothing on the recurrence
        {
            SkinnyJob jobs[4];
            std::memset(jobs, 0, sizeof jobs);
            int nj = 0;
            auto add = [&](const float* wt, const float* x, int K, int N, float* y0, float* y1) {
                const int nkg = K / 8, h0 = (nkg / 2 + 0), h1 = nkg - h0;
                const int kg0[2] = {0, h0}, nk[2] = {h0, h1};
                float* ys[2] = {y0, y1};
                for (int hh = 0; hh < 2; ++hh) {
                    SkinnyJob& J = jobs[nj++];
                    J.Wp = wt; J.N = N; J.nkg = nk[hh]; J.kg0 = kg0[hh]; J.nkg_w = nkg; J.mode = 2; J.B = B;
                    J.x[0] = XSeg{x + (size_t)kg0[hh] * B * 8, nk[hh] * 8};
                    J.y = ys[hh];
                }
            };
            if (att) add(wa_t, xa, Ka, Na, ya0, ya1);
            add(wd_t, xd, Kd, Nd, yd0, yd1);
            TR_TRY(launch_skinny(jobs, nj, SK_TRAIN, s));
        }
    }
    TR_TRY(hipGetLastError());
    // ---- after the loop: per-chunk accumulators summed in (row, chunk) order; context path of the memory gradient
    launch_col_reduce(ws + pl.dv_acc, nullptr, (long)B * G, a.a, a.dv, nullptr, s);
    launch_col_reduce(ws + pl.dld_acc, nullptr, (long)B * G, a.a * a.F, a.dloc_dense, nullptr, s);
    launch_col_reduce(ws + pl.dlw_acc, nullptr, (long)B * G, a.F * 2 * a.kl, a.dloc_conv, nullptr, s);
    hipLaunchKernelGGL(memory_context_grad_kernel, dim3((L + 7) / 8, B), dim3(BP_THREADS), 0, s, a.w_all, a.dctx_all, T, B, L, E, a.dmemory);
    TR_TRY(hipGetLastError());
    return GVX_OK;
}

}  // extern "C"
