// Back-propagation through the encoder BiLSTM in one call (gvx_train_encoder_lstm_bptt: one launch per time step for both
// directions; gvx_train_encoder_lstm_bptt_resident: the same walk as ONE resident launch), packed-sequence semantics as in the
// forward (a row takes part in step s while s < its length; the reverse direction walks each row from its own last token).
// Workgroup = (4 hidden units, direction); thread = (batch row, lane r of 8) - the 8 lanes of a row split the K of every dot
// product and combine with DPP-free shuffles.  Launch s first finishes dh(s) = dgates(s + 1) W_hh + pass-through for its units
// (the previous launch wrote dgates(s + 1)), recomputes the gate pre-activations from the tape (x-projection + h_prev W_hh^T)
// and runs the cell backwards.
#include "train_internal.h"

#include <cstdlib>
#include <cstring>

namespace gvx {
namespace {

constexpr int EB_UJ = 4;   // hidden units per workgroup

struct EncBptt {
    int B, L, H, s;
    const float* xg;         // [2][B][L][4H]  W_ih x + b_ih + b_hh per direction, torch gate order
    const float* memory;     // [B][L][2H]     BiLSTM outputs (forward direction in channels [0, H))
    const float* c_enc;      // [B][L][2H]     cell states
    const float* dmemory;    // [B][L][2H]     d loss / d memory
    const float* w_hh;       // [2][4H][H]
    const float* w_hh_t;     // [2][H][4H]
    const int32_t* lengths;  // [B]
    const float* dg_in; const float* dpass_in;   // [2][B][4H], [2][B][H] written by step s + 1
    float* dg_out; float* dpass_out;
    float* dc;               // [2][B][H] state
    float* dg_pos;           // [2][B][L][4H]  gate gradients filed under the position they belong to (zeros elsewhere)
    float* hprev_pos;        // [2][B][L][H]   the previous hidden state of that position
    int stamp;
};

// staging of a workgroup's weights (EB_UJ columns and 4 EB_UJ rows of W_hh) into LDS
__device__ __forceinline__ void enc_bptt_stage(const EncBptt& p, float* sm, int dir, int j0, int tid) {
    const int H = p.H, H4 = 4 * H;
    const float* whh = p.w_hh + (size_t)dir * H4 * H;
    const float* whht = p.w_hh_t + (size_t)dir * H * H4;
    // staging: rows of 4H / H floats are contiguous on both sides -> 16-byte pieces, all requested before the first LDS store
    {
        constexpr int NV = 8;
        const int nc4 = EB_UJ * H4 / 4, nr4 = 4 * EB_UJ * H / 4;
        for (int i0 = tid; i0 < nc4 + nr4; i0 += NV * 256) {
            float4 v[NV];
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const int i = i0 + u * 256;
                v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (i < nc4) {
                    const int jl = i / (H4 / 4), n4 = i - jl * (H4 / 4);
                    if (j0 + jl < H) v[u] = reinterpret_cast<const float4*>(whht + (size_t)(j0 + jl) * H4)[n4];
                } else if (i < nc4 + nr4) {
                    const int ii = i - nc4, qj = ii / (H / 4), k4 = ii - qj * (H / 4), jl = qj % EB_UJ, q = qj / EB_UJ;
                    if (j0 + jl < H) v[u] = reinterpret_cast<const float4*>(whh + ((size_t)q * H + j0 + jl) * H)[k4];
                }
            }
#pragma unroll
            for (int u = 0; u < NV; ++u) {
                const int i = i0 + u * 256;
                if (i < nc4 + nr4) reinterpret_cast<float4*>(sm)[i] = v[u];   // (wrow starts right behind wcol)
            }
        }
    }
    __syncthreads();
}

// One time step of the walk for this workgroup's units.  RES: the step runs inside the resident kernel - the vectors other
// workgroups wrote in the previous step of the same launch (dg_in) and this workgroup's own state words are read and written
// write-through / past the L1 (sc1), as every handed-off byte of the resident loops is.
template <bool RES>
__device__ __forceinline__ void enc_bptt_step(const EncBptt& p, const float* sm, int dir, int j0, int tid) {
    const int H = p.H, H4 = 4 * H, L = p.L, B = p.B;
    const int r = tid & 7, b0 = tid >> 3;
    const float* wcol = sm;                    // [UJ][4H]  column j of W_hh = row j of its transpose
    const float* wrow = sm + EB_UJ * H4;       // [4][UJ][H] rows (q H + j) of W_hh
    const __amdgpu_buffer_rsrc_t r_dgi = make_rsrc(p.dg_in), r_dgo = make_rsrc(p.dg_out), r_pi = make_rsrc(p.dpass_in),
                                 r_po = make_rsrc(p.dpass_out), r_dc = make_rsrc(p.dc);
    // thread = (batch row, lane r of 8).  The 8 lanes of a row split K in float4 pieces: lane r takes the floats
    // 32 i + 4 r ... + 3, so that a row's 8 lanes read 128 contiguous bytes per instruction (global and LDS alike)
    const bool vec_h = (H & 31) == 0;
    for (int b = b0; b < B; b += 32) {
        const int len = p.lengths[b];
        const bool active = p.s < len;
        const int t_idx = dir == 0 ? p.s : max(len - 1 - p.s, 0);
        const int p_idx = dir == 0 ? t_idx - 1 : t_idx + 1;
        const bool has_prev = active && p.s > 0;
        const float* hp = p.memory + ((size_t)b * L + min(max(p_idx, 0), L - 1)) * 2 * H + dir * H;
        const float* dgi = p.dg_in + ((size_t)dir * B + b) * H4;
        const unsigned dgi_off = (unsigned)(((size_t)dir * B + b) * H4 * sizeof(float));
        // operands of the cell (lanes r < UJ own unit j0 + r): requested now, used after the dot products
        const int j = j0 + r;
        const bool own = r < EB_UJ && j < H;
        const size_t sj = ((size_t)dir * B + b) * H + (own ? j : 0);
        float o_pass = 0.f, o_dmem = 0.f, o_dc = 0.f, o_cp = 0.f, o_hp = 0.f, o_x0 = 0.f, o_x1 = 0.f, o_x2 = 0.f, o_x3 = 0.f;
        if (own) {
            if (RES) { o_pass = load_sc1_f32(r_pi, (unsigned)(sj * 4)); o_dc = load_sc1_f32(r_dc, (unsigned)(sj * 4)); }
            else { o_pass = p.dpass_in[sj]; o_dc = p.dc[sj]; }
            if (active) {
                o_dmem = p.dmemory[((size_t)b * L + t_idx) * 2 * H + dir * H + j];
                const float* xg = p.xg + (((size_t)dir * B + b) * L + t_idx) * H4;
                o_x0 = xg[j]; o_x1 = xg[H + j]; o_x2 = xg[2 * H + j]; o_x3 = xg[3 * H + j];
                if (has_prev) { o_cp = p.c_enc[((size_t)b * L + p_idx) * 2 * H + dir * H + j]; o_hp = hp[j]; }
            }
        }
        float sdh[EB_UJ], sp[4][EB_UJ];
#pragma unroll
        for (int jl = 0; jl < EB_UJ; ++jl) { sdh[jl] = 0.f; sp[0][jl] = sp[1][jl] = sp[2][jl] = sp[3][jl] = 0.f; }
        constexpr int NX = 16;   // float4 pieces of the row requested together
        for (int ib = 0; ib < H4 / 32; ib += NX) {
            float4 x[NX];
#pragma unroll
            for (int u = 0; u < NX; ++u)
                x[u] = ib + u >= H4 / 32 ? make_float4(0.f, 0.f, 0.f, 0.f)
                       : (RES ? load_sc1(r_dgi, dgi_off + (unsigned)(32 * (ib + u) + 4 * r) * 4u) : *reinterpret_cast<const float4*>(dgi + 32 * (ib + u) + 4 * r));
#pragma unroll
            for (int u = 0; u < NX; ++u) {
                if (ib + u < H4 / 32) {
#pragma unroll
                    for (int jl = 0; jl < EB_UJ; ++jl) {
                        const float4 w = *reinterpret_cast<const float4*>(wcol + jl * H4 + 32 * (ib + u) + 4 * r);
                        sdh[jl] += x[u].x * w.x + x[u].y * w.y + x[u].z * w.z + x[u].w * w.w;
                    }
                }
            }
        }
        TR_STAMP(p.stamp, 1, 2);
        if (has_prev) {
            if (vec_h) {
                constexpr int NHX = 8;
                for (int ib = 0; ib < H / 32; ib += NHX) {
                    float4 x[NHX];
#pragma unroll
                    for (int u = 0; u < NHX; ++u) x[u] = ib + u < H / 32 ? *reinterpret_cast<const float4*>(hp + 32 * (ib + u) + 4 * r) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int u = 0; u < NHX; ++u) {
                        if (ib + u < H / 32) {
#pragma unroll
                            for (int q = 0; q < 4; ++q)
#pragma unroll
                                for (int jl = 0; jl < EB_UJ; ++jl) {
                                    const float4 w = *reinterpret_cast<const float4*>(wrow + (q * EB_UJ + jl) * H + 32 * (ib + u) + 4 * r);
                                    sp[q][jl] += x[u].x * w.x + x[u].y * w.y + x[u].z * w.z + x[u].w * w.w;
                                }
                        }
                    }
                }
            } else {
                for (int k = r; k < H; k += 8) {
                    const float hv = hp[k];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int jl = 0; jl < EB_UJ; ++jl) sp[q][jl] += hv * wrow[(q * EB_UJ + jl) * H + k];
                }
            }
        }
        TR_STAMP(p.stamp, 1, 3);
        float my_dh = 0.f, my_pre[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int jl = 0; jl < EB_UJ; ++jl) {
            float v0 = sdh[jl], v1 = sp[0][jl], v2 = sp[1][jl], v3 = sp[2][jl], v4 = sp[3][jl];
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {
                v0 += __shfl_xor(v0, o, 64); v1 += __shfl_xor(v1, o, 64); v2 += __shfl_xor(v2, o, 64);
                v3 += __shfl_xor(v3, o, 64); v4 += __shfl_xor(v4, o, 64);
            }
            if (r == jl) { my_dh = v0; my_pre[0] = v1; my_pre[1] = v2; my_pre[2] = v3; my_pre[3] = v4; }
        }
        TR_STAMP(p.stamp, 1, 4);
        if (own) {
            const float dh = my_dh + o_pass + o_dmem;
            float* dgo = p.dg_out + ((size_t)dir * B + b) * H4;
            const unsigned dgo_off = (unsigned)((((size_t)dir * B + b) * H4 + j) * sizeof(float));
            auto put = [&](float* ptr, __amdgpu_buffer_rsrc_t rs, unsigned off, float v) {
                if (RES) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (int)off, 0, 16); else *ptr = v;
            };
            if (!active) {
                for (int q = 0; q < 4; ++q) put(dgo + q * H + j, r_dgo, dgo_off + (unsigned)(q * H) * 4u, 0.f);
                put(p.dpass_out + sj, r_po, (unsigned)(sj * 4), dh);   // (dc stays)
            } else {
                float gi, gf, gg, go, dcp;
                lstm_cell_bwd_one(dh, o_dc, o_x0 + my_pre[0], o_x1 + my_pre[1], o_x2 + my_pre[2], o_x3 + my_pre[3], o_cp, gi, gf, gg, go, dcp);
                put(p.dc + sj, r_dc, (unsigned)(sj * 4), dcp);
                put(p.dpass_out + sj, r_po, (unsigned)(sj * 4), 0.f);
                put(dgo + j, r_dgo, dgo_off, gi); put(dgo + H + j, r_dgo, dgo_off + (unsigned)H * 4u, gf);
                put(dgo + 2 * H + j, r_dgo, dgo_off + (unsigned)(2 * H) * 4u, gg); put(dgo + 3 * H + j, r_dgo, dgo_off + (unsigned)(3 * H) * 4u, go);
                float* dgp = p.dg_pos + (((size_t)dir * B + b) * L + t_idx) * H4;
                dgp[j] = gi; dgp[H + j] = gf; dgp[2 * H + j] = gg; dgp[3 * H + j] = go;
                p.hprev_pos[(((size_t)dir * B + b) * L + t_idx) * H + j] = o_hp;
            }
        }
    }
}

__global__ __launch_bounds__(256) void encoder_bptt_step_kernel(EncBptt p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int dir = blockIdx.y, j0 = blockIdx.x * EB_UJ, tid = threadIdx.x;
    TR_STAMP(p.stamp, 1, 0);
    enc_bptt_stage(p, sm, dir, j0, tid);
    TR_STAMP(p.stamp, 1, 1);
    enc_bptt_step<false>(p, sm, dir, j0, tid);
    TR_STAMP(p.stamp, 1, 5);
}

// The whole walk as ONE resident launch (the launch per time step: 128 x 22 us for ~2 us of work each, and at the end of a
// training step it runs alone on the GPU).  Same grid, same arithmetic in the same order; the weights are staged once; step s
// starts when every workgroup of the direction has published step s + 1 (one flag word per workgroup, each on a 128-byte line
// of its own, value = steps published; stores drained and a barrier in front of the flag, cdna_hip_programming.md guideline
// 16).  Parity buffers as in the launch-per-step walk: step s writes what step s + 1's readers have left - they all published
// s + 1 before anybody could start s.  Every wait is bounded: after a time-out all waits return at once, the grid drains and
// the caller's last launch overwrites the outputs with NaN and raises the status word of the workspace.
struct EncBpttRes {
    EncBptt q;               // (s, dg_in / dg_out, dpass_in / dpass_out are set per step inside)
    float* dg; float* dpass; // [2 parities][2][B][4H] / [2 parities][2][B][H]
    unsigned* flags;         // [2][nwg] x 32 words
    unsigned* tmo;           // the call's time-out word
    unsigned spin_limit;
    int nwg;                 // workgroups per direction
    int debug_skip_block;    // tests: this workgroup leaves at once
};
__global__ __launch_bounds__(256) void encoder_bptt_resident_kernel(EncBpttRes a) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int dir = blockIdx.y, j0 = blockIdx.x * EB_UJ, tid = threadIdx.x;
    if ((int)(blockIdx.y * gridDim.x + blockIdx.x) == a.debug_skip_block) return;   // (uniform per workgroup)
    EncBptt p = a.q;
    enc_bptt_stage(p, sm, dir, j0, tid);
    const int B = p.B, H = p.H, L = p.L;
    const unsigned* fl = a.flags + (size_t)dir * a.nwg * 32;
    const unsigned limit = (a.spin_limit ? a.spin_limit : HANDOFF_SPIN_LIMIT) * 16u;
    for (int st = L - 1; st >= 0; --st) {
        const int par = st & 1;
        p.s = st;
        p.dg_in = a.dg + (size_t)(par ^ 1) * 2 * B * 4 * H; p.dg_out = a.dg + (size_t)par * 2 * B * 4 * H;
        p.dpass_in = a.dpass + (size_t)(par ^ 1) * 2 * B * H; p.dpass_out = a.dpass + (size_t)par * 2 * B * H;
        if (st < L - 1) {   // everybody has published step st + 1 = (L - 1 - st) steps
            if (tid < 64) {
                const unsigned want = (unsigned)(L - 1 - st);
                unsigned spins = 0;
                while (true) {
                    bool ok = true;
                    for (int w = tid; w < a.nwg; w += 64) ok = ok && __hip_atomic_load(fl + (size_t)w * 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= want;
                    if (__all(ok)) break;
                    if ((++spins & 127u) == 1u) {   // (after a time-out every wait gives up at its first look)
                        if (__hip_atomic_load(a.tmo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
                        if (spins > limit) { if (tid == 0) __hip_atomic_store(a.tmo, 0x600u + (unsigned)dir, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); break; }
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            __syncthreads();
        }
        enc_bptt_step<true>(p, sm, dir, j0, tid);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's write-through stores have left
        __syncthreads();
        if (tid == 0) __hip_atomic_store(a.flags + ((size_t)dir * a.nwg + blockIdx.x) * 32, (unsigned)(L - st), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// dst[d][c][r] = src[d][r][c]
__global__ void transpose_batched_kernel(const float* src, float* dst, int n, int rows, int cols) {
    const long per = (long)rows * cols, total = per * n;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long d = i / per, rc = i - d * per;
        const int c = (int)(rc / rows), r = (int)(rc - (long)c * rows);
        dst[i] = src[d * per + (long)r * cols + c];
    }
}

inline int enc_bptt_workgroups(int H) { return (H + EB_UJ - 1) / EB_UJ; }                       // per direction
inline size_t enc_bptt_lds_bytes(int H) { return (size_t)(EB_UJ * 4 * H * 2) * sizeof(float); }   // EB_UJ columns and 4 EB_UJ rows of W_hh
constexpr size_t EB_LDS_LIMIT = 160 * 1024;
// one resident launch for the whole walk where all its workgroups fit on the GPU at once (default layer size: 128 of 256 CUs)
inline bool enc_bptt_resident_serves(int H) { return 2 * enc_bptt_workgroups(H) <= 192 && enc_bptt_lds_bytes(H) <= 64 * 1024; }

struct EncBpttPlan { size_t wt, dg, dpass, dc, sync, total; };
constexpr int EB_SYNC_STATUS = 0, EB_SYNC_TMO = 32, EB_SYNC_FLAGS = 64;   // words inside the sync region (a 128-byte line each)
EncBpttPlan enc_bptt_plan(int B, int H) {
    EncBpttPlan p{};
    size_t o = 0;
    auto take = [&](size_t floats) { size_t r = o; o += (floats + 63) / 64 * 64; return r; };
    p.wt = take((size_t)2 * H * 4 * H);
    p.dg = take((size_t)2 * 2 * B * 4 * H);      // two parities
    p.dpass = take((size_t)2 * 2 * B * H);
    p.dc = take((size_t)2 * B * H);
    p.sync = take((size_t)EB_SYNC_FLAGS + (size_t)2 * ((H + EB_UJ - 1) / EB_UJ) * 32);   // status word, time-out word, a flag line per workgroup
    p.total = o;
    return p;
}

}  // namespace
}  // namespace gvx

using namespace gvx;

extern "C" {

// Host-only query for the tests, like gvx_debug_bptt_plan: out[0..3] = workgroups per direction, LDS bytes, 1 if the entry point (resident != 0:
// gvx_train_encoder_lstm_bptt_resident) takes the one resident launch, trips of the kernels' loop over batch rows.
int gvx_debug_enc_bptt_plan(int B, int H, int resident, int* out) {
    if (!out) return GVX_ERR_INVALID_ARG;
    for (int i = 0; i < 4; ++i) out[i] = 0;
    if (B < 1 || H < 8 || (H % 8)) return GVX_ERR_UNSUPPORTED;
    out[0] = enc_bptt_workgroups(H); out[1] = (int)enc_bptt_lds_bytes(H);
    out[2] = resident && enc_bptt_resident_serves(H) ? 1 : 0; out[3] = (B + 31) / 32;
    return enc_bptt_lds_bytes(H) > EB_LDS_LIMIT ? GVX_ERR_UNSUPPORTED : GVX_OK;
}

size_t gvx_train_encoder_lstm_bptt_workspace_bytes(int B, int H) {
    if (B < 1 || H < 1) return 0;
    return enc_bptt_plan(B, H).total * sizeof(float);
}

static int encoder_lstm_bptt_impl(const float* xg, const float* memory, const float* cell_states, const float* dmemory, const float* w_hh,
                                  const int32_t* lengths, int B, int L, int H, float* dg_pos, float* hprev_pos, void* workspace,
                                  size_t workspace_bytes, void* stream, bool resident) {
    if (!xg || !memory || !cell_states || !dmemory || !w_hh || !lengths || !dg_pos || !hprev_pos || !workspace)
        return tfail(GVX_ERR_INVALID_ARG, "encoder_lstm_bptt: null argument");
    if (B < 1 || L < 1 || H < 8 || (H % 8)) return tfail(GVX_ERR_UNSUPPORTED, "encoder_lstm_bptt: B, L >= 1, H a positive multiple of 8");
    const EncBpttPlan pl = enc_bptt_plan(B, H);
    if (workspace_bytes < pl.total * sizeof(float)) return tfail(GVX_ERR_WORKSPACE, "encoder_lstm_bptt: workspace too small");
    const size_t lds = enc_bptt_lds_bytes(H);
    if (lds > EB_LDS_LIMIT) return tfail(GVX_ERR_UNSUPPORTED, "encoder_lstm_bptt: H too large for the LDS");
    hipStream_t s = (hipStream_t)stream;
    float* ws = reinterpret_cast<float*>(workspace);
    TR_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(encoder_bptt_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    hipLaunchKernelGGL(transpose_batched_kernel, dim3(blocks_for((long)2 * 4 * H * H)), dim3(256), 0, s, w_hh, ws + pl.wt, 2, 4 * H, H);
    TR_TRY(hipMemsetAsync(ws + pl.dg, 0, (pl.total - pl.dg) * sizeof(float), s));
    TR_TRY(hipMemsetAsync(dg_pos, 0, (size_t)2 * B * L * 4 * H * sizeof(float), s));
    TR_TRY(hipMemsetAsync(hprev_pos, 0, (size_t)2 * B * L * H * sizeof(float), s));
    const int nwg = enc_bptt_workgroups(H);
    if (resident && enc_bptt_resident_serves(H)) {
        TR_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(encoder_bptt_resident_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        unsigned* sync = reinterpret_cast<unsigned*>(ws + pl.sync);
        EncBpttRes a{};
        a.q.B = B; a.q.L = L; a.q.H = H;
        a.q.xg = xg; a.q.memory = memory; a.q.c_enc = cell_states; a.q.dmemory = dmemory; a.q.w_hh = w_hh; a.q.w_hh_t = ws + pl.wt; a.q.lengths = lengths;
        a.q.dc = ws + pl.dc; a.q.dg_pos = dg_pos; a.q.hprev_pos = hprev_pos;
        a.dg = ws + pl.dg; a.dpass = ws + pl.dpass; a.flags = sync + EB_SYNC_FLAGS; a.tmo = sync + EB_SYNC_TMO; a.nwg = nwg;
        { const char* e = std::getenv("GVX_HANDOFF_SPIN_LIMIT"); a.spin_limit = e ? (unsigned)std::strtoul(e, nullptr, 10) : 0u; }
        { const char* e = std::getenv("GVX_DEBUG_ENC_BPTT_SKIP_BLOCK"); a.debug_skip_block = e ? std::atoi(e) : -1; }   // (tests: forced time-out)
        hipLaunchKernelGGL(encoder_bptt_resident_kernel, dim3(nwg, 2), dim3(256), lds, s, a);
        // a hand-off that timed out must not look like a result: NaN over both outputs, the code into the workspace's status word
        float* outs[2] = {dg_pos, hprev_pos};
        const size_t counts[2] = {(size_t)2 * B * L * 4 * H, (size_t)2 * B * L * H};
        TR_TRY(launch_poison_on_timeout(sync + EB_SYNC_TMO, reinterpret_cast<int*>(sync + EB_SYNC_STATUS), outs, counts, 2, s));
        TR_TRY(hipGetLastError());
        return GVX_OK;
    }
    for (int st = L - 1; st >= 0; --st) {
        EncBptt q{};
        q.B = B; q.L = L; q.H = H; q.s = st;
        q.xg = xg; q.memory = memory; q.c_enc = cell_states; q.dmemory = dmemory; q.w_hh = w_hh; q.w_hh_t = ws + pl.wt; q.lengths = lengths;
        const int par = st & 1;
        q.dg_in = ws + pl.dg + (size_t)(par ^ 1) * 2 * B * 4 * H; q.dg_out = ws + pl.dg + (size_t)par * 2 * B * 4 * H;
        q.dpass_in = ws + pl.dpass + (size_t)(par ^ 1) * 2 * B * H; q.dpass_out = ws + pl.dpass + (size_t)par * 2 * B * H;
        q.dc = ws + pl.dc; q.dg_pos = dg_pos; q.hprev_pos = hprev_pos;
        q.stamp = st == L / 2;
        hipLaunchKernelGGL(encoder_bptt_step_kernel, dim3(nwg, 2), dim3(256), lds, s, q);
    }
    TR_TRY(hipGetLastError());
    return GVX_OK;
}

int gvx_train_encoder_lstm_bptt(const float* xg, const float* memory, const float* cell_states, const float* dmemory, const float* w_hh,
                                const int32_t* lengths, int B, int L, int H, float* dg_pos, float* hprev_pos, void* workspace,
                                size_t workspace_bytes, void* stream) {
    return encoder_lstm_bptt_impl(xg, memory, cell_states, dmemory, w_hh, lengths, B, L, H, dg_pos, hprev_pos, workspace, workspace_bytes, stream, false);
}
int gvx_train_encoder_lstm_bptt_resident(const float* xg, const float* memory, const float* cell_states, const float* dmemory, const float* w_hh,
                                         const int32_t* lengths, int B, int L, int H, float* dg_pos, float* hprev_pos, void* workspace,
                                         size_t workspace_bytes, void* stream) {
    return encoder_lstm_bptt_impl(xg, memory, cell_states, dmemory, w_hh, lengths, B, L, H, dg_pos, hprev_pos, workspace, workspace_bytes, stream, true);
}
int gvx_train_encoder_lstm_bptt_status(const void* workspace, size_t workspace_bytes, int B, int H, int* code_out, void* stream) {
    if (!workspace || !code_out || B < 1 || H < 8) return tfail(GVX_ERR_INVALID_ARG, "encoder_lstm_bptt_status: bad argument");
    const EncBpttPlan pl = enc_bptt_plan(B, H);
    if (workspace_bytes < pl.total * sizeof(float)) return tfail(GVX_ERR_WORKSPACE, "encoder_lstm_bptt_status: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    TR_TRY(hipMemcpyAsync(code_out, reinterpret_cast<const float*>(workspace) + pl.sync + EB_SYNC_STATUS, sizeof(int), hipMemcpyDeviceToHost, s));
    TR_TRY(hipStreamSynchronize(s));
    return GVX_OK;
}

}  // extern "C"

#ifdef GVX_STAMPS
// diagnostic build only: phase timestamps of the flagged BPTT launches (tools/stamps_train.py) as one [3][32] image - row 0 from
// the decoder walk's source, row 1 from this one's array, row 2 not stamped by either
extern "C" int gvx_debug_read_stamps_train(unsigned long long* host96) {
    constexpr size_t row = sizeof(unsigned long long) * 32;
    std::memset(host96 + 64, 0, row);
    return read_stamps_decoder_bptt(host96) == hipSuccess && hipMemcpyFromSymbol(host96 + 32, HIP_SYMBOL(gvx::gvx_stamps), row, row) == hipSuccess ? 0 : 1;
}
#endif
