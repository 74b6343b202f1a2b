// MelGAN generator inference: mel [B][n_mels][T] -> waveform [B][T * hop].  The model is defined in include/genvox_amd.h; the float64
// restatement the tests hold these kernels to is tests/melgan_ref64.py.
//
// Every layer of the stack is ONE launch of the same implicit GEMM over channels-last activations [B][len][C]:
//
//     out[b][phases * q + phase][n] = bias[n] (+ bias2[n]) + sum over taps tau, channels c of  act_tau(src_tau[b][row(q, tau, phase)][c]) * W[phase][n][tau * Cin + c]
//
//   convolution (phases = 1)      row = reflect(q + (tau - (taps - 1) / 2) * dil) at the row's OWN length; taps = 7 or 3
//   residual tail (phases = 1)    two taps at row q from two tensors: tap 0 = x as it is against W_s, tap 1 = lrelu(h) against W_m - the
//                                 block's shortcut(x) + mix(lrelu(h)) as one product with K = 2 C
//   transposed conv (phases = r)  kernel 2r, stride r, padding r/2: output r q + phase receives input q through kernel tap phase + r/2 and
//                                 input q - 1 (phase < r/2, tap phase + r/2 + r) or q + 1 (else, tap phase + r/2 - r); outside the row: zero.
//                                 r two-tap products with K = 2 Cin whose outputs interleave; the weight is packed per phase at pack time.
//
// LeakyReLU is applied to the operand on its way into LDS (act_mask: one bit per tap).  Two kernels take that form:
//   mg_mfma_kernel   Cout >= 32: 128 positions x 128 / 64 / 32 channels per workgroup of four waves on v_mfma_f32_32x32x2_f32, k-tiles of 32
//                    double buffered through registers; both operands K-contiguous in LDS rows of 36 floats, one float4 per lane feeding
//                    four k-steps (the layout of gemm_f32.hip)
//   mg_valu_kernel   Cout < 32 (and the 1-channel output layer, with tanh): fmaf dot products, G lanes per output element
// A workgroup belongs to one batch row and computes nothing behind that row's length; tensors the caller sees are zero-filled there.
//
// Order of this file: layer description, the two kernels, the mel transpose, the weight packer, the C ABI.
#include "melgan_internal.h"

using gvx::fail;
using namespace gvx_mg;

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int MG_LD = 36;   // floats per LDS row of a 32-deep k-tile: the fragment reads of sixteen lanes fall on distinct 16-byte slots
template <int BM, int BN>
constexpr size_t mg_lds_bytes() { return (size_t)2 * (BM + BN) * MG_LD * sizeof(float); }

template <int WR, int WC, int TM, int TN>
__global__ void __launch_bounds__(256) mg_mfma_kernel(const MgLayer p) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32, A_V4 = BM / 32, B_V4 = BN / 32;
    static_assert(WR * WC == 4, "four waves");
    extern __shared__ __attribute__((aligned(16))) float mg_smem[];
    float* As = mg_smem;                   // [2][BM][MG_LD]
    float* Bs = mg_smem + 2 * BM * MG_LD;  // [2][BN][MG_LD]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave / WC, wc = wave % WC, r = lane & 31, h = lane >> 5;
    const int b = blockIdx.z;
    const int n_tiles = (p.Cout + BN - 1) / BN;
    const int nt = (int)blockIdx.y % n_tiles, phase = (int)blockIdx.y / n_tiles;
    const int q0 = (int)blockIdx.x * BM, n0 = nt * BN;
    const int Lmax = p.T * p.in_mul;
    const int len = mg_frames(p.lens, b, p.T) * p.in_mul;
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

    const int ld_row = tid >> 3, ld_c4 = tid & 7;
    const float* w_row[B_V4];
#pragma unroll
    for (int i = 0; i < B_V4; ++i) {
        const int n = n0 + ld_row + 32 * i;
        w_row[i] = p.W + ((size_t)phase * p.Cout + (n < p.Cout ? n : 0)) * p.K;   // columns past Cout read row 0 and are never stored
    }
    float4 a_reg[A_V4], b_reg[B_V4];
    int a_zero = 0;          // bit i: the tap of a_reg[i] lies outside the row
    bool k_ok = false, act = false;

    // global -> registers for the k-tile at K0; what is zeroed or activated is decided here and applied at the LDS stores, so that nothing
    // waits for the loads while the products of the current tile run
#define MG_LOAD(K0)                                                                                                  \
    {                                                                                                                \
        const int k_ = (K0) + 4 * ld_c4;                                                                             \
        k_ok = k_ < p.K;                                                                                             \
        const int kk_ = k_ok ? k_ : 0;                                                                               \
        const int tau_ = kk_ / p.Cin, c_ = kk_ - tau_ * p.Cin;                                                       \
        act = (p.act_mask >> tau_) & 1;                                                                              \
        const float* s_ = ((p.two_src && tau_) ? p.src1 : p.src0) + (size_t)b * Lmax * p.Cin + c_;                   \
        a_zero = 0;                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < A_V4; ++i) {                                                           \
            bool z_;                                                                                                 \
            const int q_ = min(q0 + ld_row + 32 * i, len - 1);   /* positions past the row repeat its last one; never stored */ \
            const int row_ = mg_src_row(p, q_, tau_, phase, len, z_);                                                \
            a_zero |= (int)z_ << i;                                                                                  \
            a_reg[i] = *reinterpret_cast<const float4*>(s_ + (size_t)row_ * p.Cin);                                  \
        }                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < B_V4; ++i) b_reg[i] = *reinterpret_cast<const float4*>(w_row[i] + kk_); \
    }
#define MG_STORE(BUF)                                                                                                \
    {                                                                                                                \
        _Pragma("unroll") for (int i = 0; i < A_V4; ++i) {                                                           \
            const bool keep_ = k_ok && !((a_zero >> i) & 1);                                                         \
            float4 v_ = a_reg[i];                                                                                    \
            if (act) v_ = make_float4(mg_lrelu(v_.x, p.slope), mg_lrelu(v_.y, p.slope), mg_lrelu(v_.z, p.slope), mg_lrelu(v_.w, p.slope)); \
            *reinterpret_cast<float4*>(&As[((BUF) * BM + ld_row + 32 * i) * MG_LD + 4 * ld_c4]) =                    \
                make_float4(keep_ ? v_.x : 0.f, keep_ ? v_.y : 0.f, keep_ ? v_.z : 0.f, keep_ ? v_.w : 0.f);         \
        }                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < B_V4; ++i)                                                             \
            *reinterpret_cast<float4*>(&Bs[((BUF) * BN + ld_row + 32 * i) * MG_LD + 4 * ld_c4]) =                    \
                make_float4(k_ok ? b_reg[i].x : 0.f, k_ok ? b_reg[i].y : 0.f, k_ok ? b_reg[i].z : 0.f, k_ok ? b_reg[i].w : 0.f); \
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int nk = (p.K + 31) / 32;
    MG_LOAD(0)
    MG_STORE(0)
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int buf = kt & 1;
        if (kt + 1 < nk) MG_LOAD((kt + 1) * 32)
        const float* a_base = &As[(buf * BM + wr * TM * 32 + r) * MG_LD + 4 * h];
        const float* b_base = &Bs[(buf * BN + wc * TN * 32 + r) * MG_LD + 4 * h];
#pragma unroll
        for (int kg = 0; kg < 4; ++kg) {
            float4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4*>(a_base + i * 32 * MG_LD + 8 * kg);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const float4*>(b_base + j * 32 * MG_LD + 8 * kg);
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
        if (kt + 1 < nk) MG_STORE(buf ^ 1)
        __syncthreads();
    }
#undef MG_LOAD
#undef MG_STORE

    // epilogue: lane (r, h) holds column r of rows (e & 3) + 8 (e >> 2) + 4 h of every 32 x 32 tile
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int col = n0 + (wc * TN + j) * 32 + r;
        if (col >= p.Cout) continue;
        const float bias = p.bias[col] + (p.bias2 ? p.bias2[col] : 0.f);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int q = q0 + (wr * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * h;
                float* o = out_b + ((size_t)q * p.phases + phase) * p.Cout + col;
                if (q < len) *o = acc[i][j][e] + bias;
                else if (p.zero_tail && q < Lmax) *o = 0.f;
            }
    }
}

// G lanes per output element (position, channel), channel fastest; the G partial sums are added by shuffles.
template <int G>
__global__ void __launch_bounds__(256) mg_valu_kernel(const MgLayer p) {
    const int b = blockIdx.z, phase = blockIdx.y;
    const int Lmax = p.T * p.in_mul;
    const int len = mg_frames(p.lens, b, p.T) * p.in_mul;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int g = (int)(idx % G);
    const long e = idx / G;
    const int n = (int)(e % p.Cout);
    const long ql = e / p.Cout;
    const bool inside = ql < Lmax, live = ql < len;
    const int q = (int)ql;
    float sum = 0.f;
    if (live) {
        const float* w = p.W + ((size_t)phase * p.Cout + n) * p.K;
        for (int tau = 0; tau < p.taps; ++tau) {
            bool zero;
            const int row = mg_src_row(p, q, tau, phase, len, zero);
            if (zero) continue;
            const float* x = ((p.two_src && tau) ? p.src1 : p.src0) + ((size_t)b * Lmax + row) * p.Cin;
            const bool act = (p.act_mask >> tau) & 1;
            const float* wt = w + tau * p.Cin;
            for (int c = g; c < p.Cin; c += G) {
                float v = x[c];
                if (act) v = mg_lrelu(v, p.slope);
                sum = fmaf(v, wt[c], sum);
            }
        }
    }
#pragma unroll
    for (int off = G >> 1; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    if (g == 0 && inside) {
        float v = 0.f;
        if (live) {
            v = sum + (p.bias[n] + (p.bias2 ? p.bias2[n] : 0.f));
            if (p.tanh_out) v = tanhf(v);
        }
        if (live || p.zero_tail) p.out[(((size_t)b * Lmax + q) * p.phases + phase) * p.Cout + n] = v;
    }
}

// mel [B][M][T] -> channels-last [B][T][Cp] with the channels padded by zeros to a multiple of four; nothing behind a row's frames is read
__global__ void __launch_bounds__(256) mg_mel_transpose_kernel(const float* mel, const int32_t* lens, int M, int T, int Cp, float* out) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)T * Cp) return;
    const int t = (int)(idx % T), c = (int)(idx / T);
    const int Tb = mg_frames(lens, b, T);
    out[((size_t)b * T + t) * Cp + c] = (t < Tb && c < M) ? mel[((size_t)b * M + c) * T + t] : 0.f;
}

// Conv1d weight [Cout][Cin][k] -> dst[n * ld + off + tau * Cp + c], zeros for the padded channels c >= Cin (a bias: Cin = Cp = k = ld = 1)
__global__ void __launch_bounds__(256) mg_pack_conv_kernel(float* dst, const float* src, int Cout, int Cin, int Cp, int k, int ld, int off) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)Cout * k * Cp) return;
    const int c = (int)(idx % Cp), tau = (int)((idx / Cp) % k), n = (int)(idx / ((long)Cp * k));
    dst[(size_t)n * ld + off + tau * Cp + c] = c < Cin ? src[((size_t)n * Cin + c) * k + tau] : 0.f;
}

// ConvTranspose1d weight [Cin][Cout][2r] -> dst[phase][n][tau * Cin + c]: the kernel tap that connects output r q + phase with its tap-tau input
__global__ void __launch_bounds__(256) mg_pack_tconv_kernel(float* dst, const float* src, int Cin, int Cout, int r) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)r * Cout * 2 * Cin) return;
    const int c = (int)(idx % Cin), tau = (int)((idx / Cin) % 2), n = (int)((idx / (2l * Cin)) % Cout), phase = (int)(idx / (2l * Cin * Cout));
    const int half = r / 2;
    const int tap = tau == 0 ? phase + half : (phase < half ? phase + half + r : phase + half - r);
    dst[idx] = src[((size_t)c * Cout + n) * (2 * r) + tap];
}

// ---- host side
struct MgWs {   // byte offsets; every region is B times a per-row size that is a multiple of 256
    size_t mel_t, buf[3], total;
};

MgWs mg_ws_plan(const gvx_melgan_dims& d, int B, int T) {
    size_t widest = d.base_channels, mul = 1, C = d.base_channels;   // floats per frame of the widest activation tensor
    for (int i = 0; i < d.n_stages; ++i) {
        mul *= d.ratios[i];
        C /= 2;
        widest = std::max(widest, mul * C);
    }
    MgWs w{};
    GenRows ws{B};
    w.mel_t = ws.rows((size_t)T * mg_cpad(d));
    for (size_t& buf : w.buf) buf = ws.rows((size_t)T * widest);
    w.total = ws.total;
    return w;
}

template <int WR, int WC, int TM, int TN>
int mg_launch_mfma(const MgLayer& p, int B, hipStream_t s) {
    constexpr int BM = WR * TM * 32, BN = WC * TN * 32;
    const dim3 grid((unsigned)((p.T * p.in_mul + BM - 1) / BM), (unsigned)(((p.Cout + BN - 1) / BN) * p.phases), (unsigned)B);
    mg_mfma_kernel<WR, WC, TM, TN><<<grid, 256, mg_lds_bytes<BM, BN>(), s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

}  // namespace

namespace gvx_mg {

int mg_launch(const MgLayer& p, int B, hipStream_t s) {
    if (p.Cout >= 32 && p.Cin % 4 == 0) {
        if (p.Cout >= 128) return mg_launch_mfma<2, 2, 2, 2>(p, B, s);
        if (p.Cout > 32) return mg_launch_mfma<4, 1, 1, 2>(p, B, s);
        return mg_launch_mfma<4, 1, 1, 1>(p, B, s);
    }
    const int G = p.Cout == 1 ? 8 : 1;
    const long threads = (long)p.T * p.in_mul * p.Cout * G;
    const dim3 grid((unsigned)((threads + 255) / 256), (unsigned)p.phases, (unsigned)B);
    if (G == 8) mg_valu_kernel<8><<<grid, 256, 0, s>>>(p);
    else mg_valu_kernel<1><<<grid, 256, 0, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int mg_mel_transpose(const float* mel, const int32_t* lens, int B, int M, int T, int Cp, float* out, hipStream_t s) {
    const dim3 grid((unsigned)(((long)T * Cp + 255) / 256), (unsigned)B);
    mg_mel_transpose_kernel<<<grid, 256, 0, s>>>(mel, lens, M, T, Cp, out);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int mg_prepare(gvx_melgan* h) {
    if (!h->lds_ready) {
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(mg_mfma_kernel<2, 2, 2, 2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)mg_lds_bytes<128, 128>()));
        h->lds_ready = true;
    }
    return GVX_OK;
}

}  // namespace gvx_mg

// the relayouts of MelGAN's and HiFi-GAN's packers
int gvx_gen::GenConvPacker::run(float* device_blob, size_t total, hipStream_t s) const {
    if (rc != GVX_OK) return rc;   // nothing was launched
    HIP_TRY(hipMemsetAsync(device_blob, 0, total * sizeof(float), s));   // the padding between the tensors
    for (const Job& j : jobs) {
        if (!j.tconv) {
            const long count = (long)j.a * j.k * j.c;
            mg_pack_conv_kernel<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(device_blob + j.dst, j.src, j.a, j.b, j.c, j.k, j.ld, j.off);
        } else {
            const long count = (long)j.c * j.b * 2 * j.a;
            mg_pack_tconv_kernel<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(device_blob + j.dst, j.src, j.a, j.b, j.c);
        }
        HIP_TRY(hipGetLastError());
    }
    return GVX_OK;
}

extern "C" {

size_t gvx_melgan_blob_floats(const gvx_melgan_dims* dims) {
    if (mg_dims_problem(dims)) return 0;
    return mg_blob_layout(*dims).total;
}

size_t gvx_melgan_workspace_bytes(const gvx_melgan_dims* dims, int B, int T) {
    if (mg_dims_problem(dims) || B < 1 || T < GVX_MELGAN_MIN_FRAMES || T > GVX_MELGAN_MAX_FRAMES) return 0;
    return mg_ws_plan(*dims, B, T).total;
}

int gvx_melgan_pack_weights_device(const gvx_melgan_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = mg_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    const gvx_melgan_dims& d = *dims;
    const MgBlob L = mg_blob_layout(d);
    GenConvPacker P{{table, n}};
    int C = d.base_channels;
    P.conv("pre.weight", L.pre_w, C, d.n_mels, mg_cpad(d), 7, 7 * mg_cpad(d), 0);
    P.bias("pre.bias", L.pre_b, C);
    for (int i = 0; i < d.n_stages; ++i) {
        const int Cn = C / 2;
        const std::string up = "ups." + std::to_string(i);
        P.tconv(up + ".weight", L.up_w[i], C, Cn, d.ratios[i]);
        P.bias(up + ".bias", L.up_b[i], Cn);
        for (int j = 0; j < d.n_residual_layers; ++j) {
            const std::string res = "res." + std::to_string(i) + "." + std::to_string(j);
            P.conv(res + ".conv.weight", L.conv_w[i][j], Cn, Cn, Cn, 3, 3 * Cn, 0);
            P.bias(res + ".conv.bias", L.conv_b[i][j], Cn);
            P.conv(res + ".shortcut.weight", L.tail_w[i][j], Cn, Cn, Cn, 1, 2 * Cn, 0);
            P.conv(res + ".mix.weight", L.tail_w[i][j], Cn, Cn, Cn, 1, 2 * Cn, Cn);
            P.bias(res + ".shortcut.bias", L.sc_b[i][j], Cn);
            P.bias(res + ".mix.bias", L.mix_b[i][j], Cn);
        }
        C = Cn;
    }
    P.conv("post.weight", L.post_w, 1, C, C, 7, 7 * C, 0);
    P.bias("post.bias", L.post_b, 1);
    return P.run(device_blob, L.total, (hipStream_t)stream);
}

int gvx_melgan_create(const gvx_melgan_dims* dims, gvx_melgan** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = mg_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_melgan* h = new gvx_melgan();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_melgan_destroy(gvx_melgan* h) { delete h; }

int gvx_melgan_bind(gvx_melgan* h, const float* device_blob) { return gen_bind(h, device_blob); }

int gvx_melgan_timing_enable(gvx_melgan* h, int enable) { return gen_timing_enable(h, enable, h ? h->d.n_stages + 3 : 0); }

int gvx_melgan_stage_times_ms(gvx_melgan* h, float* ms_out, int* n_out) { return gen_stage_times_ms(h, h ? h->d.n_stages + 2 : 0, ms_out, n_out); }

int gvx_melgan_forward(gvx_melgan* h, const float* mel, const int32_t* frame_lengths, int B, int T, float* wav_out, float* const* stage_out,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!h || !mel || !wav_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->blob) return fail(GVX_ERR_STATE, "no weight blob is bound");
    const gvx_melgan_dims& d = h->d;
    if (B < 1 || B > 65535) return fail(GVX_ERR_INVALID_ARG, "B must be in [1, 65535]");
    if (T < GVX_MELGAN_MIN_FRAMES) return fail(GVX_ERR_INVALID_ARG, "T = %d: the first convolution's reflection needs at least %d frames", T, GVX_MELGAN_MIN_FRAMES);
    if (T > GVX_MELGAN_MAX_FRAMES) return fail(GVX_ERR_UNSUPPORTED, "T = %d is beyond the limit of %d frames", T, GVX_MELGAN_MAX_FRAMES);
    const MgWs wp = mg_ws_plan(d, B, T);
    int rc;
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    if ((rc = gen_check_stage_out(stage_out, d.n_stages)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = mg_prepare(h)) != GVX_OK) return rc;
    const MgBlob L = mg_blob_layout(d);
    const float* blob = h->blob;
    float* pool[3] = {gvx::ws_ptr<float>(workspace, wp.buf[0]), gvx::ws_ptr<float>(workspace, wp.buf[1]), gvx::ws_ptr<float>(workspace, wp.buf[2])};
    auto other = [&](const float* a, const float* b2) {   // a pool buffer that is neither
        for (float* c : pool)
            if (c != a && c != b2) return c;
        return pool[0];
    };
    int ev = 0;
    auto stamp = [&] { return gen_mark(h, ev++, s); };
    if ((rc = stamp()) != GVX_OK) return rc;

    const int Cp = mg_cpad(d);
    float* mel_t = gvx::ws_ptr<float>(workspace, wp.mel_t);
    if ((rc = mg_mel_transpose(mel, frame_lengths, B, d.n_mels, T, Cp, mel_t, s)) != GVX_OK) return rc;
    MgLayer p{};
    p.lens = frame_lengths;
    p.T = T;
    p.slope = d.slope;
    int C = d.base_channels, mul = 1;
    float* cur = pool[0];
    // the first convolution: no activation in front of it
    p.src0 = mel_t; p.W = blob + L.pre_w; p.bias = blob + L.pre_b; p.out = cur;
    p.in_mul = 1; p.Cin = Cp; p.Cout = C; p.taps = 7; p.K = 7 * Cp; p.dil = 1; p.phases = 1; p.act_mask = 0;
    if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
    if ((rc = stamp()) != GVX_OK) return rc;

    for (int i = 0; i < d.n_stages; ++i) {
        const int Cn = C / 2, r = d.ratios[i];
        float* x = other(cur, nullptr);
        p = MgLayer{};
        p.lens = frame_lengths; p.T = T; p.slope = d.slope;
        p.src0 = cur; p.W = blob + L.up_w[i]; p.bias = blob + L.up_b[i]; p.out = x;
        p.in_mul = mul; p.Cin = C; p.Cout = Cn; p.taps = 2; p.K = 2 * C; p.dil = 0; p.phases = r; p.act_mask = 3;
        if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
        mul *= r;
        int dil = 1;
        for (int j = 0; j < d.n_residual_layers; ++j, dil *= d.dilation_base) {
            float* hbuf = other(x, nullptr);
            const bool last = j == d.n_residual_layers - 1;
            float* y = (last && stage_out) ? stage_out[i] : other(x, hbuf);
            p = MgLayer{};
            p.lens = frame_lengths; p.T = T; p.slope = d.slope;
            p.src0 = x; p.W = blob + L.conv_w[i][j]; p.bias = blob + L.conv_b[i][j]; p.out = hbuf;
            p.in_mul = mul; p.Cin = Cn; p.Cout = Cn; p.taps = 3; p.K = 3 * Cn; p.dil = dil; p.phases = 1; p.act_mask = 7;
            if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
            p.src1 = hbuf; p.two_src = 1; p.W = blob + L.tail_w[i][j]; p.bias = blob + L.sc_b[i][j]; p.bias2 = blob + L.mix_b[i][j]; p.out = y;
            p.taps = 2; p.K = 2 * Cn; p.dil = 0; p.act_mask = 2; p.zero_tail = (last && stage_out) ? 1 : 0;
            if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
            x = y;
        }
        cur = x;
        C = Cn;
        if ((rc = stamp()) != GVX_OK) return rc;
    }
    p = MgLayer{};
    p.lens = frame_lengths; p.T = T; p.slope = d.slope;
    p.src0 = cur; p.W = blob + L.post_w; p.bias = blob + L.post_b; p.out = wav_out;
    p.in_mul = mul; p.Cin = C; p.Cout = 1; p.taps = 7; p.K = 7 * C; p.dil = 1; p.phases = 1; p.act_mask = 0x7f; p.tanh_out = 1; p.zero_tail = 1;
    if ((rc = mg_launch(p, B, s)) != GVX_OK) return rc;
    return stamp();
}

}  // C ABI
