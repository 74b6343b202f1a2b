// HiFi-GAN generator inference: mel [B][n_mels][T] -> waveform [B][T * hop].  The model is defined in include/genvox_amd.h ("HiFi-GAN
// generator"); the float64 restatement the tests hold these kernels to is tests/hifigan_ref64.py.
//
// Every layer is ONE launch over channels-last activations [B][len][C] of the form hifigan_internal.h states (HgLayer): a convolution
// with zero padding, or the r two-tap phases of a transposed convolution, with LeakyReLU on the operand and one of three epilogues -
// store, store with the residual block's own input added, or the multi-receptive-field accumulation into the stage's sum.
//
//   hg_mfma_kernel   Cout >= 32: 128 positions x 128 / 64 / 32 channels per workgroup of four waves on v_mfma_f32_32x32x2_f32.  Per block
//                    of 32 input channels the tile's WHOLE input window - its 128 positions and the (taps - 1) * dil halo rows - goes
//                    into LDS once (LeakyReLU and the zeros outside the row applied at that store), and every tap's products read it
//                    at a row offset of tau * dil: a tap moves every lane's row by the same amount, so the K-contiguous 36-float rows
//                    stay conflict-free.  The weights stream as one [BN][32] tile per (channel block, tap).  Both are double buffered
//                    through registers.  An activation row is read from global memory once per channel block, not once per tap.
//   hg_valu_kernel   Cout < 32 and the 1-channel output layer (with tanh): fmaf dot products, G lanes per output element
// A workgroup belongs to one batch row and computes nothing behind that row's length; tensors the caller sees are zero-filled there.
//
// Order of this file: the two kernels, the mel transpose, the weight packer, the host walk, the C ABI.
#include "hifigan_internal.h"

using gvx::fail;
using namespace gvx_hg;

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int HG_LD = 36;    // floats per LDS row of a 32-deep k-tile: the fragment reads of sixteen lanes fall on distinct 16-byte slots
constexpr int HG_BM = 128;   // positions per workgroup
constexpr int HG_A_PASS = (HG_BM + GVX_HIFIGAN_MAX_WINDOW + 31) / 32;   // 32 window rows per pass of the 256 threads
inline size_t hg_lds_bytes(int halo, int BN) { return (size_t)2 * (HG_BM + halo + BN) * HG_LD * sizeof(float); }

__device__ __forceinline__ float hg_finish(const HgLayer& p, float v, const float* res, float* o) {
    if (res) v += *res;
    if (p.accumulate) v = *o + v;
    if (p.divide > 0.f) v = v / p.divide;
    return v;
}

template <int WR, int WC, int TM, int TN>
__global__ void __launch_bounds__(256) hg_mfma_kernel(const HgLayer p) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32, B_V4 = BN / 32;
    static_assert(WR * WC == 4 && BM == HG_BM, "four waves, 128 positions");
    extern __shared__ __attribute__((aligned(16))) float hg_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / WC, wc = wave % WC, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z;
    const int n_tiles = (p.Cout + BN - 1) / BN;
    const int nt = (int)blockIdx.y % n_tiles, phase = (int)blockIdx.y / n_tiles;
    const int q0 = (int)blockIdx.x * BM, n0 = nt * BN;
    const int Lmax = p.T * p.in_mul;
    const int len = hg_frames(p.lens, b, p.T) * p.in_mul;
    float* out_b = p.out + (size_t)b * Lmax * p.phases * p.Cout;
    if (q0 >= len) {   // nothing of this row here
        if (p.zero_tail) {
            const int rows = min(BM, Lmax - q0), cols = min(BN, p.Cout - n0);
            for (int i = tid; i < rows * cols; i += 256) {
                const int q = q0 + i / cols, n = n0 + i % cols;
                out_b[((size_t)q * p.phases + phase) * p.Cout + n] = 0.f;
            }
        }
        return;
    }
    const HgTaps tp = hg_taps(p.taps, p.dil, p.phases, phase);
    const int win = BM + tp.halo;              // window rows: source positions q0 - left .. q0 - left + win - 1
    float* As = hg_smem;                       // [2][win][HG_LD]
    float* Bs = hg_smem + 2 * win * HG_LD;     // [2][BN][HG_LD]
    const float* src_b = p.src + (size_t)b * Lmax * p.Cin;

    const int ld_row = tid >> 3, ld_c4 = tid & 7;
    const float* w_row[B_V4];
#pragma unroll
    for (int i = 0; i < B_V4; ++i) {
        const int n = n0 + ld_row + 32 * i;
        w_row[i] = p.W + ((size_t)phase * p.Cout + (n < p.Cout ? n : 0)) * p.K;   // columns past Cout read row 0 and are never stored
    }
    float4 a_reg[HG_A_PASS], b_reg[B_V4];
    int a_keep = 0;               // bit i: a_reg[i] lies inside the row and inside the channels
    bool a_c_ok = false, b_c_ok = false;

    // global -> registers; what is zeroed is decided here and applied, with the activation, at the LDS stores, so that nothing waits
    // for the loads while the products of the current tile run
#define HG_LOAD_A(CB)                                                                                                \
    {                                                                                                                \
        const int c_ = 32 * (CB) + 4 * ld_c4;                                                                        \
        a_c_ok = c_ < p.Cin;                                                                                         \
        const float* s_ = src_b + (a_c_ok ? c_ : 0);                                                                 \
        a_keep = 0;                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < HG_A_PASS; ++i) {                                                      \
            const int w_ = ld_row + 32 * i;                                                                          \
            if (w_ < win) {                                                                                          \
                const int pos_ = q0 - tp.left + w_;                                                                  \
                const bool in_ = pos_ >= 0 && pos_ < len;                                                            \
                a_keep |= (int)(in_ && a_c_ok) << i;                                                                 \
                a_reg[i] = *reinterpret_cast<const float4*>(s_ + (size_t)(in_ ? pos_ : 0) * p.Cin);                  \
            }                                                                                                        \
        }                                                                                                            \
    }
#define HG_STORE_A(BUF)                                                                                              \
    {                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < HG_A_PASS; ++i) {                                                      \
            const int w_ = ld_row + 32 * i;                                                                          \
            if (w_ < win) {                                                                                          \
                const bool keep_ = (a_keep >> i) & 1;                                                                \
                float4 v_ = a_reg[i];                                                                                \
                if (p.act) v_ = make_float4(hg_lrelu(v_.x, p.slope), hg_lrelu(v_.y, p.slope), hg_lrelu(v_.z, p.slope), hg_lrelu(v_.w, p.slope)); \
                *reinterpret_cast<float4*>(&As[((BUF) * win + w_) * HG_LD + 4 * ld_c4]) =                            \
                    make_float4(keep_ ? v_.x : 0.f, keep_ ? v_.y : 0.f, keep_ ? v_.z : 0.f, keep_ ? v_.w : 0.f);     \
            }                                                                                                        \
        }                                                                                                            \
    }
#define HG_LOAD_B(TAU, CB)                                                                                           \
    {                                                                                                                \
        const int c_ = 32 * (CB) + 4 * ld_c4;                                                                        \
        b_c_ok = c_ < p.Cin;                                                                                         \
        const int k_ = b_c_ok ? (TAU) * p.Cin + c_ : 0;                                                              \
        _Pragma("unroll") for (int i = 0; i < B_V4; ++i) b_reg[i] = *reinterpret_cast<const float4*>(w_row[i] + k_); \
    }
#define HG_STORE_B(BUF)                                                                                              \
    {                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < B_V4; ++i)                                                             \
            *reinterpret_cast<float4*>(&Bs[((BUF) * BN + ld_row + 32 * i) * HG_LD + 4 * ld_c4]) =                    \
                make_float4(b_c_ok ? b_reg[i].x : 0.f, b_c_ok ? b_reg[i].y : 0.f, b_c_ok ? b_reg[i].z : 0.f, b_c_ok ? b_reg[i].w : 0.f); \
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int n_it = ((p.Cin + 31) / 32) * p.taps;   // (channel block, tap) pairs, the tap fastest
    HG_LOAD_A(0)
    HG_LOAD_B(0, 0)
    HG_STORE_A(0)
    HG_STORE_B(0)
    __syncthreads();
    int tau = 0, cb = 0;
    for (int it = 0; it < n_it; ++it) {
        int ntau = tau + 1, ncb = cb;
        if (ntau == p.taps) { ntau = 0; ++ncb; }
        const bool more = it + 1 < n_it, new_a = more && ntau == 0;
        if (more) HG_LOAD_B(ntau, ncb)
        if (new_a) HG_LOAD_A(ncb)
        const float* a_base = &As[((cb & 1) * win + tp.off0 + tau * tp.step + wr * TM * 32 + r) * HG_LD + 4 * h];
        const float* b_base = &Bs[((it & 1) * BN + wc * TN * 32 + r) * HG_LD + 4 * h];
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4*>(a_base + i * 32 * HG_LD + 8 * kg);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const float4*>(b_base + j * 32 * HG_LD + 8 * kg);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
                }
        }
        if (more) HG_STORE_B((it + 1) & 1)
        if (new_a) HG_STORE_A(ncb & 1)
        __syncthreads();
        tau = ntau;
        cb = ncb;
    }
#undef HG_LOAD_A
#undef HG_STORE_A
#undef HG_LOAD_B
#undef HG_STORE_B

    // epilogue: lane (r, h) holds column r of rows (e & 3) + 8 (e >> 2) + 4 h of every 32 x 32 tile
    const float* res_b = p.res ? p.res + (size_t)b * Lmax * p.Cout : nullptr;   // a residual comes with phases = 1 only
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + (wc * TN + j) * 32 + r;
        if (col >= p.Cout) continue;
        const float bias = p.bias[col];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int q = q0 + (wr * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                float* o = out_b + ((size_t)q * p.phases + phase) * p.Cout + col;
                if (q < len) *o = hg_finish(p, acc[i][j][e] + bias, res_b ? res_b + (size_t)q * p.Cout + col : nullptr, o);
                else if (p.zero_tail && q < Lmax) *o = 0.f;
            }
    }
}

// G lanes per output element (position, channel), channel fastest; the G partial sums are added by shuffles.
template <int G>
__global__ void __launch_bounds__(256) hg_valu_kernel(const HgLayer p) {
    const int b = blockIdx.z, phase = blockIdx.y;
    const int Lmax = p.T * p.in_mul;
    const int len = hg_frames(p.lens, b, p.T) * p.in_mul;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int g = (int)(idx % G);
    const long e = idx / G;
    const int n = (int)(e % p.Cout);
    const long ql = e / p.Cout;
    const bool inside = ql < Lmax, live = ql < len;
    const int q = (int)ql;
    float sum = 0.f;
    if (live) {
        const HgTaps tp = hg_taps(p.taps, p.dil, p.phases, phase);
        const float* w = p.W + ((size_t)phase * p.Cout + n) * p.K;
        for (int tau = 0; tau < p.taps; ++tau) {
            const int pos = q - tp.left + tp.off0 + tau * tp.step;
            if (pos < 0 || pos >= len) continue;
            const float* x = p.src + ((size_t)b * Lmax + pos) * p.Cin;
            const float* wt = w + tau * p.Cin;
            for (int c = g; c < p.Cin; c += G) {
                float v = x[c];
                if (p.act) v = hg_lrelu(v, p.slope);
                sum = fmaf(v, wt[c], sum);
            }
        }
    }
#pragma unroll
    for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (g == 0 && inside) {
        float* o = p.out + (((size_t)b * Lmax + q) * p.phases + phase) * p.Cout + n;
        if (live) {
            float v = hg_finish(p, sum + p.bias[n], p.res ? p.res + ((size_t)b * Lmax + q) * p.Cout + n : nullptr, o);
            if (p.tanh_out) v = tanhf(v);
            *o = v;
        } else if (p.zero_tail) {
            *o = 0.f;
        }
    }
}

// mel [B][M][T] -> channels-last [B][T][Cp] with the channels padded by zeros to a multiple of four; nothing behind a row's frames is read
__global__ void __launch_bounds__(256) hg_mel_transpose_kernel(const float* mel, const int32_t* lens, int M, int T, int Cp, float* out) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)T * Cp) return;
    const int t = (int)(idx % T), c = (int)(idx / T);
    const int Tb = hg_frames(lens, b, T);
    out[((size_t)b * T + t) * Cp + c] = (t < Tb && c < M) ? mel[((size_t)b * M + c) * T + t] : 0.f;
}

// Conv1d weight [Cout][Cin][k] -> dst[n][tau * Cp + c], zeros for the padded channels c >= Cin (a bias: Cin = Cp = k = 1)
__global__ void __launch_bounds__(256) hg_pack_conv_kernel(float* dst, const float* src, int Cout, int Cin, int Cp, int k) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)Cout * k * Cp) return;
    const int c = (int)(idx % Cp), tau = (int)((idx / Cp) % k), n = (int)(idx / ((long)Cp * k));
    dst[idx] = c < Cin ? src[((size_t)n * Cin + c) * k + tau] : 0.f;
}

// ConvTranspose1d weight [Cin][Cout][2r] -> dst[phase][n][tau * Cin + c]: the kernel tap that connects output r q + phase with its tap-tau input
__global__ void __launch_bounds__(256) hg_pack_tconv_kernel(float* dst, const float* src, int Cin, int Cout, int r) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)r * Cout * 2 * Cin) return;
    const int c = (int)(idx % Cin), tau = (int)((idx / Cin) % 2), n = (int)((idx / (2l * Cin)) % Cout), phase = (int)(idx / (2l * Cin * Cout));
    const int half = r / 2;
    const int tap = tau == 0 ? phase + half : (phase < half ? phase + half + r : phase + half - r);
    dst[idx] = src[((size_t)c * Cout + n) * (2 * r) + tap];
}

// ---- host side
struct HgWs {   // byte offsets; every region is B times a per-row size that is a multiple of 256
    size_t mel_t, buf[4], total;
};

HgWs hg_ws_plan(const gvx_hifigan_dims& d, int B, int T) {
    size_t widest = d.upsample_initial_channel, mul = 1, C = d.upsample_initial_channel;   // floats per frame of the widest activation tensor
    for (int i = 0; i < d.n_stages; ++i) {
        mul *= d.upsample_rates[i];
        C /= 2;
        widest = std::max(widest, mul * C);
    }
    HgWs w{};
    size_t at = 0;
    w.mel_t = at;
    at += (size_t)B * hg_round256((size_t)T * hg_cpad(d) * sizeof(float));
    for (int i = 0; i < 4; ++i) {
        w.buf[i] = at;
        at += (size_t)B * hg_round256((size_t)T * widest * sizeof(float));
    }
    w.total = at;
    return w;
}

template <int WR, int WC, int TM, int TN>
int hg_launch_mfma(const HgLayer& p, int B, hipStream_t s) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
    const dim3 grid((unsigned)((p.T * p.in_mul + BM - 1) / BM), (unsigned)(((p.Cout + BN - 1) / BN) * p.phases), (unsigned)B);
    hg_mfma_kernel<WR, WC, TM, TN><<<grid, 256, hg_lds_bytes(hg_taps(p.taps, p.dil, p.phases, 0).halo, BN), s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int hg_launch(const HgLayer& p, int B, hipStream_t s) {
    if (p.Cout >= 32 && p.Cin % 4 == 0) {
        if (p.Cout >= 128) return hg_launch_mfma<2, 2, 2, 2>(p, B, s);
        if (p.Cout > 32) return hg_launch_mfma<4, 1, 1, 2>(p, B, s);
        return hg_launch_mfma<4, 1, 1, 1>(p, B, s);
    }
    const int G = p.Cout == 1 ? 8 : 1;
    const long threads = (long)p.T * p.in_mul * p.Cout * G;
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)p.phases, (unsigned)B);
    if (G == 8) hg_valu_kernel<8><<<grid, 256, 0, s>>>(p);
    else hg_valu_kernel<1><<<grid, 256, 0, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

// once per handle: the dynamic LDS of the largest window any layer of any supported configuration asks for
int hg_prepare(gvx_hifigan* h) {
    if (!h->lds_ready) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(hg_mfma_kernel<2, 2, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)hg_lds_bytes(GVX_HIFIGAN_MAX_WINDOW, 128)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(hg_mfma_kernel<4, 1, 1, 2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)hg_lds_bytes(GVX_HIFIGAN_MAX_WINDOW, 64)));
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(hg_mfma_kernel<4, 1, 1, 1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)hg_lds_bytes(GVX_HIFIGAN_MAX_WINDOW, 32)));
        h->lds_ready = true;
    }
    return GVX_OK;
}

const gvx_weight_desc* hg_find(const gvx_weight_desc* table, int n, const std::string& name, size_t numel, int& rc) {
    for (int i = 0; i < n; ++i)
        if (table[i].name && name == table[i].name) {
            if (!table[i].data || table[i].numel != (int64_t)numel) {
                rc = fail(GVX_ERR_SHAPE, "%s has %lld elements, the dims ask for %zu", name.c_str(), (long long)table[i].numel, numel);
                return nullptr;
            }
            return &table[i];
        }
    rc = fail(GVX_ERR_MISSING_WEIGHT, "%s is missing", name.c_str());
    return nullptr;
}

// the names of a residual block's convolutions: [m][0 / 1]
std::string hg_conv_name(const gvx_hifigan_dims& d, int block, int m, int v) {
    const std::string base = "resblocks." + std::to_string(block);
    if (d.resblock == 2) return base + ".convs." + std::to_string(m);
    return base + (v == 0 ? ".convs1." : ".convs2.") + std::to_string(m);
}

}  // namespace

extern "C" {

size_t gvx_hifigan_blob_floats(const gvx_hifigan_dims* dims) {
    if (hg_dims_problem(dims)) return 0;
    return hg_blob_layout(*dims).total;
}

size_t gvx_hifigan_workspace_bytes(const gvx_hifigan_dims* dims, int B, int T) {
    if (hg_dims_problem(dims) || B < 1 || T < 1 || T > GVX_HIFIGAN_MAX_FRAMES) return 0;
    return hg_ws_plan(*dims, B, T).total;
}

int gvx_hifigan_pack_weights_device(const gvx_hifigan_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = hg_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_hifigan_dims& d = *dims;
    const HgBlob L = hg_blob_layout(d);
    hipStream_t s = (hipStream_t)stream;
    struct Job { int kind; size_t dst; const float* src; int a, b, c, k; };   // kind 0: conv (Cout a, Cin b, Cp c), 1: tconv (Cin a, Cout b, r c)
    std::vector<Job> jobs;
    int rc = GVX_OK;
    auto conv = [&](const std::string& name, size_t dst_w, size_t dst_b, int Cout, int Cin, int Cp, int k) {
        if (rc != GVX_OK) return;
        if (const gvx_weight_desc* w = hg_find(table, n, name + ".weight", (size_t)Cout * Cin * k, rc)) jobs.push_back({0, dst_w, w->data, Cout, Cin, Cp, k});
        if (rc != GVX_OK) return;
        if (const gvx_weight_desc* w = hg_find(table, n, name + ".bias", (size_t)Cout, rc)) jobs.push_back({0, dst_b, w->data, Cout, 1, 1, 1});
    };
    int C = d.upsample_initial_channel;
    conv("conv_pre", L.pre_w, L.pre_b, C, d.n_mels, hg_cpad(d), 7);
    for (int i = 0; i < d.n_stages && rc == GVX_OK; ++i) {
        const int Cn = C / 2;
        const std::string up = "ups." + std::to_string(i);
        if (const gvx_weight_desc* w = hg_find(table, n, up + ".weight", (size_t)C * Cn * 2 * d.upsample_rates[i], rc))
            jobs.push_back({1, L.up_w[i], w->data, C, Cn, d.upsample_rates[i], 0});
        if (rc != GVX_OK) break;
        if (const gvx_weight_desc* w = hg_find(table, n, up + ".bias", (size_t)Cn, rc)) jobs.push_back({0, L.up_b[i], w->data, Cn, 1, 1, 1});
        for (int j = 0; j < d.n_resblocks; ++j)
            for (int m = 0; m < d.n_dilations; ++m)
                for (int v = 0; v < hg_convs_per_dilation(d); ++v)
                    conv(hg_conv_name(d, i * d.n_resblocks + j, m, v), L.conv_w[i][j][m][v], L.conv_b[i][j][m][v], Cn, Cn, Cn, d.resblock_kernel_sizes[j]);
        C = Cn;
    }
    conv("conv_post", L.post_w, L.post_b, 1, C, C, 7);
    if (rc != GVX_OK) return rc;   // nothing was launched
    HIP_TRY(hipMemsetAsync(device_blob, 0, L.total * sizeof(float), s));   // the padding between the tensors
    for (const Job& j : jobs) {
        if (j.kind == 0) {
            const long count = (long)j.a * j.k * j.c;
            hg_pack_conv_kernel<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(device_blob + j.dst, j.src, j.a, j.b, j.c, j.k);
        } else {
            const long count = (long)j.c * j.b * 2 * j.a;
            hg_pack_tconv_kernel<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(device_blob + j.dst, j.src, j.a, j.b, j.c);
        }
        HIP_TRY(hipGetLastError());
    }
    return GVX_OK;
}

int gvx_hifigan_create(const gvx_hifigan_dims* dims, gvx_hifigan** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = hg_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_hifigan* h = new gvx_hifigan();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_hifigan_destroy(gvx_hifigan* h) {
    if (!h) return;
    for (int i = 0; i < h->n_ev; ++i) (void)hipEventDestroy(h->ev[i]);
    delete h;
}

int gvx_hifigan_bind(gvx_hifigan* h, const float* device_blob) {
    if (!h || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if ((uintptr_t)device_blob % 256) return fail(GVX_ERR_INVALID_ARG, "the blob must be 256-byte aligned");
    h->blob = device_blob;
    return GVX_OK;
}

int gvx_hifigan_timing_enable(gvx_hifigan* h, int enable) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const int need = h->d.n_stages + 3;
    while (enable && h->n_ev < need) HIP_TRY(hipEventCreate(&h->ev[h->n_ev++]));
    h->timing = enable != 0;
    return GVX_OK;
}

int gvx_hifigan_stage_times_ms(gvx_hifigan* h, float* ms_out, int* n_out) {
    if (!h || !ms_out || !n_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->timing) return fail(GVX_ERR_STATE, "timing is not enabled");
    const int n = h->d.n_stages + 2;
    HIP_TRY(hipEventSynchronize(h->ev[n]));
    for (int i = 0; i < n; ++i) HIP_TRY(hipEventElapsedTime(&ms_out[i], h->ev[i], h->ev[i + 1]));
    *n_out = n;
    return GVX_OK;
}

int gvx_hifigan_forward(gvx_hifigan* h, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, float* const* stage_out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !mel || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    const gvx_hifigan_dims& d = h->d;
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (T < 1) return fail(GVX_ERR_INVALID_ARG, "T = %d: a row needs at least 1 frame", T);
    if (T > GVX_HIFIGAN_MAX_FRAMES) return fail(GVX_ERR_UNSUPPORTED, "T = %d is beyond the limit of %d frames", T, GVX_HIFIGAN_MAX_FRAMES);
    const HgWs wp = hg_ws_plan(d, B, T);
    if (!workspace || (uintptr_t)workspace % 256 || workspace_bytes < wp.total)
        return fail(GVX_ERR_WORKSPACE, "the workspace is missing, misaligned or smaller than %zu bytes", wp.total);
    if (stage_out)
        for (int i = 0; i < d.n_stages; ++i)
            if (!stage_out[i] || (uintptr_t)stage_out[i] % 16) return fail(GVX_ERR_INVALID_ARG, "stage_out[%d] is null or not 16-byte aligned", i);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = hg_prepare(h)) != GVX_OK) return rc;
    const HgBlob L = hg_blob_layout(d);
    const float* blob = h->blob;
    float* pool[4];
    for (int i = 0; i < 4; ++i) pool[i] = gvx::ws_ptr<float>(workspace, wp.buf[i]);
    int ev = 0;
    auto stamp = [&]() -> int {
        if (h->timing) HIP_TRY(hipEventRecord(h->ev[ev++], s));
        return GVX_OK;
    };
    if ((rc = stamp()) != GVX_OK) return rc;

    const int Cp = hg_cpad(d);
    float* mel_t = gvx::ws_ptr<float>(workspace, wp.mel_t);
    {
        const dim3 grid((unsigned)(((long)T * Cp + 255) / 256), (unsigned)B);
        hg_mel_transpose_kernel<<<grid, 256, 0, s>>>(mel, frame_lengths, d.n_mels, T, Cp, mel_t);
        HIP_TRY(hipGetLastError());
    }
    auto layer = [&](const float* src, size_t w, size_t bias, float* out, int in_mul, int Cin, int Cout, int taps, int dil, int phases, int act) {
        HgLayer p{};
        p.lens = frame_lengths; p.T = T; p.slope = d.slope;
        p.src = src; p.W = blob + w; p.bias = blob + bias; p.out = out;
        p.in_mul = in_mul; p.Cin = Cin; p.Cout = Cout; p.taps = taps; p.K = taps * Cin; p.dil = dil; p.phases = phases; p.act = act;
        return p;
    };
    int C = d.upsample_initial_channel, mul = 1;
    float* cur = pool[0];
    HgLayer p = layer(mel_t, L.pre_w, L.pre_b, cur, 1, Cp, C, 7, 1, 1, 0);   // conv_pre: no activation in front of it
    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
    if ((rc = stamp()) != GVX_OK) return rc;

    for (int i = 0; i < d.n_stages; ++i) {
        const int Cn = C / 2, r = d.upsample_rates[i];
        // the stage's tensors: x, its sum, and a block's two.  The stage's input is free once ups has run; it is a pool tensor unless
        // the caller's stage_out[i - 1] holds it, and then the sum is the caller's too and leaves a pool tensor over.
        float* rest[4];
        int n_rest = 0;
        for (float* c : pool)
            if (c != cur) rest[n_rest++] = c;
        float* x = rest[0];
        float* sum = stage_out ? stage_out[i] : rest[1];
        float* t0 = rest[2];
        float* t1 = n_rest == 3 ? cur : rest[1];
        p = layer(cur, L.up_w[i], L.up_b[i], x, mul, C, Cn, 2, 0, r, 1);
        if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
        mul *= r;
        for (int j = 0; j < d.n_resblocks; ++j) {
            const int k = d.resblock_kernel_sizes[j];
            const float* in = x;   // the block's running value
            for (int m = 0; m < d.n_dilations; ++m) {
                const bool last = m == d.n_dilations - 1;
                const int dil = d.resblock_dilation_sizes[j][m];
                const float* conv_in = in;
                int conv_dil = dil, v = 0;
                float* next;
                if (d.resblock == 1) {   // t1 = convs1(lrelu(in)); next = in + convs2(lrelu(t1)): next may be `in` itself once that is t0
                    p = layer(in, L.conv_w[i][j][m][0], L.conv_b[i][j][m][0], t1, mul, Cn, Cn, k, dil, 1, 1);
                    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
                    conv_in = t1; conv_dil = 1; v = 1;
                    next = t0;
                } else {                 // next = in + convs(lrelu(in)): the convolution reads its neighbours, so next is another tensor
                    next = in == t0 ? t1 : t0;
                }
                p = layer(conv_in, L.conv_w[i][j][m][v], L.conv_b[i][j][m][v], last ? sum : next, mul, Cn, Cn, k, conv_dil, 1, 1);
                p.res = in;
                if (last) {   // y_j goes into the stage's sum: written by the first block, added by the later ones, the last divides
                    p.accumulate = j > 0;
                    p.divide = j == d.n_resblocks - 1 ? (float)d.n_resblocks : 0.f;
                    p.zero_tail = (stage_out && j == 0) ? 1 : 0;
                }
                if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
                in = next;
            }
        }
        cur = sum;
        C = Cn;
        if ((rc = stamp()) != GVX_OK) return rc;
    }
    p = layer(cur, L.post_w, L.post_b, wav_out, mul, C, 1, 7, 1, 1, 1);
    p.slope = d.post_slope; p.tanh_out = 1; p.zero_tail = 1;
    if ((rc = hg_launch(p, B, s)) != GVX_OK) return rc;
    return stamp();
}

}  // C ABI
