// MelGAN multi-scale discriminator (include/genvox_amd.h, "MelGAN discriminators"): forward, and the backward that reads the forward's
// own maps as its tape.  Maps are [B][C][L] with positions contiguous, as the Python surface returns them.
//
// Every convolution - the reflected first layer, the grouped strided layers (4 input channels per group), the dense k = 5 layer and the
// score layer - is one of three fp32 kernels, a workgroup per tile of MD_TILE = 64 positions of one row:
//   md_fwd_kernel  a thread owns one position and CPT output channels of one group; the strided input window of the tile goes through
//                  LDS once and serves every tap; weights are wave-uniform reads.
//                  (md_fwd_one_kernel: the score's single output channel, the input channels dealt to four waves.)
//   md_dx_kernel   the data gradient as a gather: a thread owns one input position and CPT input channels; the dY window and the
//                  group's weights go through LDS; the epilogue adds the cotangent of the map below and applies its LeakyReLU mask,
//                  which it reads off the map itself (y > 0 exactly where the pre-activation is).
//   md_dw_kernel   the weight gradient in pieces of rows / runs of positions, a thread per (4 output channels, input channel, tap);
//                  md_reduce_kernel adds the pieces in their order.  No atomics anywhere: two calls give the same bits.
// Dot products are summed in runs of at most 32 input channels whose sums are then added, so the dense layer's 5120 terms never form one
// chain.  Rows are ragged: every length derives from the row's own n_b, and a map is exact zeros behind it.
#include "disc_handle.h"
#include "melgan_disc_internal.h"

#include <climits>

using gvx::fail;
using namespace gvx_md;
using namespace gvx_dc;

struct gvx_melgan_disc : gvx_gen::GenHandle {
    gvx_melgan_disc_dims d;
};

namespace {

struct MdConv {
    const float* x;       // input  [B][cin][lin_max]   (forward, dW);  the map below, for its sign (dX)
    const float* W;
    const float* bias;
    float* y;             // output [B][cout][lout_max] (forward);  dX: the gradient that leaves, [B][cin][lin_max]
    const float* dy;      // dX, dW: gradient of this layer's pre-activation [B][cout][lout_max]
    const float* dfeat;   // dX: cotangent of the map below (added before its mask), or nullptr
    const int32_t* lens;
    int n_max, min_n, shift, s;
    int lin_max, lout_max;
    int cin, cout, cig, cog, k, stride, pad, down_in, down_out, reflect, act;
    float slope;
};

__device__ __forceinline__ int md_row_n(const MdConv& p, int b) {
    int n = p.lens ? p.lens[b] : p.n_max;
    n = n > p.n_max ? p.n_max : n;
    return n < p.min_n ? 0 : (n >> p.shift);   // rows the caller should have refused are silent, never a bad address
}

__device__ __forceinline__ int md_src(int q, int n, bool reflect) {   // source index of padded position q, -1: zero
    if (reflect) {
        q = q < 0 ? -q : q;
        q = q >= n ? 2 * (n - 1) - q : q;
    }
    return (q < 0 || q >= n) ? -1 : q;
}

constexpr int FWD_WIN_FLOATS = 2400;   // 4 channels x (63 * 8 + 81) or 32 channels x (63 + 5)

template <int CPT>
__global__ void __launch_bounds__(256) md_fwd_kernel(const MdConv p) {
    __shared__ float win[FWD_WIN_FLOATS];
    const int b = blockIdx.z, tid = threadIdx.x, pos = tid & 63;
    const int lane = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cob = (blockDim.x >> 6) * CPT, tiles = (p.cog + cob - 1) / cob;
    const int g = blockIdx.y / tiles, co0 = (blockIdx.y % tiles) * cob + lane * CPT;   // co0: inside the group
    const int nb = md_row_n(p, b);
    const int lin = md_chain(nb, p.s, p.down_in), lout = md_chain(nb, p.s, p.down_out);
    const int l0 = blockIdx.x * MD_TILE, l = l0 + pos;
    float* yrow = p.y + ((size_t)b * p.cout + (size_t)g * p.cog) * p.lout_max;
    if (l0 >= lout) {   // the whole tile lies behind the row
        if (l < p.lout_max)
            for (int j = 0; j < CPT; ++j)
                if (co0 + j < p.cog) yrow[(size_t)(co0 + j) * p.lout_max + l] = 0.f;
        return;
    }
    const int width = (MD_TILE - 1) * p.stride + p.k, q0 = l0 * p.stride - p.pad;
    const int cic = p.cig < 32 ? p.cig : 32;
    const float* xrow = p.x + ((size_t)b * p.cin + (size_t)g * p.cig) * p.lin_max;
    const float* w[CPT];
    float acc[CPT];
    for (int j = 0; j < CPT; ++j) {
        const int co = g * p.cog + (co0 + j < p.cog ? co0 + j : p.cog - 1);
        w[j] = p.W + (size_t)co * p.cig * p.k;
        acc[j] = p.bias[co];
    }
    for (int c0 = 0; c0 < p.cig; c0 += cic) {
        const int cn = p.cig - c0 < cic ? p.cig - c0 : cic;
        __syncthreads();
        for (int idx = tid; idx < cn * width; idx += blockDim.x) {
            const int ci = idx / width, q = md_src(q0 + idx % width, lin, p.reflect);
            win[idx] = q < 0 ? 0.f : xrow[(size_t)(c0 + ci) * p.lin_max + q];
        }
        __syncthreads();
        float part[CPT];
        for (int j = 0; j < CPT; ++j) part[j] = 0.f;
        for (int ci = 0; ci < cn; ++ci) {
            const float* wr = win + ci * width + pos * p.stride;
            const int wo = (c0 + ci) * p.k;
            for (int t = 0; t < p.k; ++t) {
                const float xv = wr[t];
#pragma unroll
                for (int j = 0; j < CPT; ++j) part[j] = fmaf(xv, w[j][wo + t], part[j]);
            }
        }
        for (int j = 0; j < CPT; ++j) acc[j] += part[j];
    }
    if (l < p.lout_max)
        for (int j = 0; j < CPT; ++j)
            if (co0 + j < p.cog) {
                float v = acc[j];
                if (p.act) v = v > 0.f ? v : v * p.slope;
                yrow[(size_t)(co0 + j) * p.lout_max + l] = l < lout ? v : 0.f;
            }
}

// a layer with ONE output channel (the score): a thread per position would walk all 3 C_in products alone, so the input channels are
// dealt to the four waves of the workgroup and the four sums are added in a fixed order
__global__ void __launch_bounds__(256) md_fwd_one_kernel(const MdConv p) {
    __shared__ float red[4][MD_TILE];
    const int b = blockIdx.z, tid = threadIdx.x, pos = tid & 63;
    const int part = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nb = md_row_n(p, b);
    const int lin = md_chain(nb, p.s, p.down_in), lout = md_chain(nb, p.s, p.down_out);
    const int l0 = blockIdx.x * MD_TILE, l = l0 + pos;
    float* yrow = p.y + (size_t)b * p.lout_max;
    if (l0 >= lout) {
        if (part == 0 && l < p.lout_max) yrow[l] = 0.f;
        return;
    }
    const int per = (p.cig + 3) / 4, c_lo = part * per, c_hi = c_lo + per < p.cig ? c_lo + per : p.cig;
    const float* xrow = p.x + (size_t)b * p.cin * p.lin_max;
    float acc = 0.f;
    for (int c0 = c_lo; c0 < c_hi; c0 += 32) {
        const int c1 = c0 + 32 < c_hi ? c0 + 32 : c_hi;
        float run = 0.f;
        for (int ci = c0; ci < c1; ++ci)
            for (int t = 0; t < p.k; ++t) {
                const int q = md_src(l * p.stride + t - p.pad, lin, p.reflect);
                run = fmaf(q < 0 ? 0.f : xrow[(size_t)ci * p.lin_max + q], p.W[ci * p.k + t], run);
            }
        acc += run;
    }
    red[part][pos] = acc;
    __syncthreads();
    if (part == 0 && l < p.lout_max) {
        float v = p.bias[0] + ((red[0][pos] + red[1][pos]) + (red[2][pos] + red[3][pos]));
        if (p.act) v = v > 0.f ? v : v * p.slope;
        yrow[l] = l < lout ? v : 0.f;
    }
}

constexpr int DX_LW = 80;           // dY positions a tile of 64 input positions can reach: (63 + k - 1) / stride + 2 <= 75
constexpr int DX_W_FLOATS = 10368;  // 32 output channels x 4 input channels x 81 taps, or 32 x 32 x 5

// gradient that leaves through the input of a zero-padded layer: out = (sum + dfeat) * mask(x), 0 at and behind the row's input length
template <int CPT>
__global__ void __launch_bounds__(256) md_dx_kernel(const MdConv p) {
    __shared__ float dwin[32 * DX_LW];
    __shared__ float wl[DX_W_FLOATS];
    const int b = blockIdx.z, tid = threadIdx.x, pos = tid & 63, lane = tid >> 6;
    const int cib = (blockDim.x >> 6) * CPT, tiles = (p.cig + cib - 1) / cib;
    const int g = blockIdx.y / tiles, cb0 = (blockIdx.y % tiles) * cib, ci0 = cb0 + lane * CPT;   // inside the group
    const int nb = md_row_n(p, b);
    const int lin = md_chain(nb, p.s, p.down_in), lout = md_chain(nb, p.s, p.down_out);
    const int p0 = blockIdx.x * MD_TILE, pp = p0 + pos;
    float* orow = p.y + ((size_t)b * p.cin + (size_t)g * p.cig) * p.lin_max;
    if (p0 >= lin) {
        if (pp < p.lin_max)
            for (int j = 0; j < CPT; ++j)
                if (ci0 + j < p.cig) orow[(size_t)(ci0 + j) * p.lin_max + pp] = 0.f;
        return;
    }
    int lbase = p0 + p.pad - (p.k - 1);
    lbase = lbase <= 0 ? 0 : (lbase + p.stride - 1) / p.stride;
    const int coc = p.cog < 32 ? p.cog : 32;
    const int r = (pp + p.pad) % p.stride, ltop = (pp + p.pad) / p.stride;
    const float* dyrow = p.dy + ((size_t)b * p.cout + (size_t)g * p.cog) * p.lout_max;
    float acc[CPT];
    for (int j = 0; j < CPT; ++j) acc[j] = 0.f;
    for (int c0 = 0; c0 < p.cog; c0 += coc) {
        const int cn = p.cog - c0 < coc ? p.cog - c0 : coc;
        __syncthreads();
        for (int idx = tid; idx < cn * DX_LW; idx += blockDim.x) {
            const int co = idx / DX_LW, l = lbase + idx % DX_LW;
            dwin[idx] = l < lout ? dyrow[(size_t)(c0 + co) * p.lout_max + l] : 0.f;
        }
        for (int idx = tid; idx < cn * cib * p.k; idx += blockDim.x) {
            const int t = idx % p.k, ci = (idx / p.k) % cib, co = idx / (p.k * cib);
            wl[idx] = cb0 + ci < p.cig ? p.W[((size_t)(g * p.cog + c0 + co) * p.cig + cb0 + ci) * p.k + t] : 0.f;
        }
        __syncthreads();
        float part[CPT];
        for (int j = 0; j < CPT; ++j) part[j] = 0.f;
        for (int co = 0; co < cn; ++co) {
            const float* wr = wl + (co * cib + lane * CPT) * p.k;
            for (int t = r, l = ltop; t < p.k && l >= 0; t += p.stride, --l) {
                if (l - lbase >= DX_LW) continue;   // cannot happen for the layers of this model; never an address outside dwin
                const float d = dwin[co * DX_LW + l - lbase];
#pragma unroll
                for (int j = 0; j < CPT; ++j) part[j] = fmaf(d, wr[j * p.k + t], part[j]);
            }
        }
        for (int j = 0; j < CPT; ++j) acc[j] += part[j];
    }
    if (pp < p.lin_max)
        for (int j = 0; j < CPT; ++j)
            if (ci0 + j < p.cig) {
                const size_t at = ((size_t)b * p.cin + (size_t)g * p.cig + ci0 + j) * p.lin_max + pp;
                float v = 0.f;
                if (pp < lin) {
                    v = acc[j] + (p.dfeat ? p.dfeat[at] : 0.f);
                    v = p.x[at] > 0.f ? v : v * p.slope;
                }
                p.y[at] = v;
            }
}

// y[j] = mean of x[2j-1 .. 2j+2] inside [0, n), j < n / 2
__global__ void __launch_bounds__(256) md_pool_kernel(const float* x, float* y, const int32_t* lens, int n_max, int min_n, int shift, int xs, int ys) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    int n = lens ? lens[b] : n_max;
    n = n > n_max ? n_max : n;
    n = n < min_n ? 0 : (n >> shift);
    if (j >= (n >> 1)) return;
    const int lo = 2 * j - 1 < 0 ? 0 : 2 * j - 1, hi = 2 * j + 2 > n - 1 ? n - 1 : 2 * j + 2;
    float sum = 0.f;
    for (int i = lo; i <= hi; ++i) sum += x[(size_t)b * xs + i];
    y[(size_t)b * ys + j] = sum / (float)(hi - lo + 1);
}

// gradient of a scale's waveform: the adjoint of the reflected first convolution (its gradient dy is [B][c0][n]) plus the adjoint of the
// pooling applied to the gradient of the next scale's waveform (d_next [B][ns], or nullptr); 0 at and behind the row's samples
__global__ void __launch_bounds__(256) md_dx0_kernel(const MdConv p, const float* d_next, int ns) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.lin_max) return;
    const int n = md_row_n(p, b);
    float v = 0.f;
    if (i < n) {
        const float* dyrow = p.dy + (size_t)b * p.cout * p.lout_max;
        // the padded positions whose source is sample i: i itself, its mirror at the front, its mirror at the end
        const int img[3] = {i, (i >= 1 && i <= p.pad) ? -i : INT_MIN, (2 * (n - 1) - i >= n && 2 * (n - 1) - i < n + p.pad) ? 2 * (n - 1) - i : INT_MIN};
        for (int co = 0; co < p.cout; ++co) {
            float part = 0.f;
            for (int m = 0; m < 3; ++m) {
                if (img[m] == INT_MIN) continue;
                for (int t = 0; t < p.k; ++t) {
                    const int l = img[m] + p.pad - t;
                    if (l >= 0 && l < n) part = fmaf(dyrow[(size_t)co * p.lout_max + l], p.W[co * p.k + t], part);
                }
            }
            v += part;
        }
        if (d_next) {
            const int m = n >> 1;
            int jlo = i - 2 <= 0 ? 0 : (i - 1) / 2, jhi = (i + 1) / 2;   // ceil((i - 2) / 2) .. floor((i + 1) / 2)
            jhi = jhi > m - 1 ? m - 1 : jhi;
            float pool = 0.f;
            for (int j = jlo; j <= jhi; ++j) {
                const int lo = 2 * j - 1 < 0 ? 0 : 2 * j - 1, hi = 2 * j + 2 > n - 1 ? n - 1 : 2 * j + 2;
                pool += d_next[(size_t)b * ns + j] / (float)(hi - lo + 1);
            }
            v += pool;
        }
    }
    p.y[(size_t)b * p.lin_max + i] = v;
}

// one piece of dW: thread -> (CPT output channels of a group, one input channel, one tap), summed over the piece's rows and positions
template <int CPT>
__global__ void __launch_bounds__(256) md_dw_kernel(const MdConv p, float* parts, int B, int chunks, int rows_per_piece) {
    const size_t numel = (size_t)p.cout * p.cig * p.k;
    const int per_co = p.cig * p.k;
    const long o = (long)blockIdx.x * 256 + threadIdx.x;
    if (o >= (long)(p.cout / CPT) * per_co) return;
    const int cob = (int)(o / per_co), rem = (int)(o % per_co), ci = rem / p.k, t = rem % p.k;
    const int co = cob * CPT, g = co / p.cog;
    const int piece = blockIdx.y;
    int b0, b1, chunk;
    if (chunks > 1) { b0 = piece / chunks; b1 = b0 + 1; chunk = piece % chunks; }
    else { b0 = piece * rows_per_piece; b1 = b0 + rows_per_piece < B ? b0 + rows_per_piece : B; chunk = 0; }
    const int run = (p.lout_max + chunks - 1) / chunks;
    float acc[CPT];
    for (int j = 0; j < CPT; ++j) acc[j] = 0.f;
    for (int b = b0; b < b1; ++b) {
        const int nb = md_row_n(p, b);
        const int lin = md_chain(nb, p.s, p.down_in), lout = md_chain(nb, p.s, p.down_out);
        const int la = chunk * run, lb = la + run < lout ? la + run : lout;
        const float* xr = p.x + ((size_t)b * p.cin + (size_t)g * p.cig + ci) * p.lin_max;
        const float* dr = p.dy + ((size_t)b * p.cout + co) * p.lout_max;
        float part[CPT];
        for (int j = 0; j < CPT; ++j) part[j] = 0.f;
        for (int l = la; l < lb; ++l) {
            const int q = md_src(l * p.stride + t - p.pad, lin, p.reflect);
            if (q < 0) continue;
            const float xv = xr[q];
#pragma unroll
            for (int j = 0; j < CPT; ++j) part[j] = fmaf(dr[(size_t)j * p.lout_max + l], xv, part[j]);
        }
        for (int j = 0; j < CPT; ++j) acc[j] += part[j];
    }
    for (int j = 0; j < CPT; ++j) parts[(size_t)piece * numel + (size_t)(co + j) * per_co + rem] = acc[j];
}

__global__ void __launch_bounds__(256) md_reduce_kernel(const float* parts, float* out, size_t numel, int n) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= numel) return;
    float v = 0.f;
    for (int i = 0; i < n; ++i) v += parts[(size_t)i * numel + o];
    out[o] = v;
}

// db[co] = sum over rows and positions of dy: a workgroup per channel, threads stride the positions, one tree in LDS.  Summed in
// float64 and rounded once: a bias gradient is a plain sum of cotangents that may cancel (the hinge loss's real and fake halves do),
// and a tensor of one element - the score's bias - has no larger neighbour to set its scale, so float32 partial sums would leave an
// error of an ulp of the TERMS in a result far smaller than they are
__global__ void __launch_bounds__(256) md_db_kernel(const MdConv p, float* out, int B) {
    __shared__ double red[256];
    const int co = blockIdx.x;
    double v = 0.0;
    for (int b = 0; b < B; ++b) {
        const int lout = md_chain(md_row_n(p, b), p.s, p.down_out);
        const float* dr = p.dy + ((size_t)b * p.cout + co) * p.lout_max;
        for (int l = threadIdx.x; l < lout; l += 256) v += (double)dr[l];
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[co] = (float)red[0];
}

MdConv md_conv(const gvx_melgan_disc_dims& d, const MdLayer& l, const MdFeat& F, int k, int i, const int32_t* lens, int n_max) {
    MdConv p{};
    p.lens = lens; p.n_max = n_max; p.min_n = md_min_samples(d); p.shift = k; p.s = d.downsampling_factor;
    p.lin_max = i == 0 ? (n_max >> k) : F.positions[k][i - 1];
    p.lout_max = F.positions[k][i];
    p.cin = l.cin; p.cout = l.cout; p.cig = l.cig; p.cog = l.cog; p.k = l.k; p.stride = l.stride; p.pad = l.pad;
    p.down_in = l.down_in; p.down_out = l.down_out; p.reflect = l.reflect; p.act = l.act; p.slope = d.slope;
    return p;
}

int md_launch_fwd(const MdConv& p, const MdLayer& l, int B, hipStream_t s) {
    if (l.cout == 1) {
        md_fwd_one_kernel<<<dim3((unsigned)((p.lout_max + MD_TILE - 1) / MD_TILE), 1, (unsigned)B), 256, 0, s>>>(p);
        HIP_TRY(hipGetLastError());
        return GVX_OK;
    }
    const int cpt = (l.groups == 1 && l.cog >= 32) ? 8 : (l.cog >= 4 ? 4 : 1);
    int lanes = (l.cog + cpt - 1) / cpt;
    lanes = lanes > 4 ? 4 : lanes;
    const int cob = lanes * cpt;
    const dim3 grid((unsigned)((p.lout_max + MD_TILE - 1) / MD_TILE), (unsigned)(l.groups * ((l.cog + cob - 1) / cob)), (unsigned)B);
    if (grid.y > 65535) return fail(GVX_ERR_UNSUPPORTED, "a layer of %d channels has too many channel tiles", l.cout);
    if (cpt == 8) md_fwd_kernel<8><<<grid, 64 * lanes, 0, s>>>(p);
    else if (cpt == 4) md_fwd_kernel<4><<<grid, 64 * lanes, 0, s>>>(p);
    else md_fwd_kernel<1><<<grid, 64 * lanes, 0, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int md_launch_dx(const MdConv& p, const MdLayer& l, int B, hipStream_t s) {
    const int cpt = l.cig >= 32 ? 8 : 4;
    int lanes = (l.cig + cpt - 1) / cpt;
    lanes = lanes > 4 ? 4 : lanes;
    const int cib = lanes * cpt;
    const dim3 grid((unsigned)((p.lin_max + MD_TILE - 1) / MD_TILE), (unsigned)(l.groups * ((l.cig + cib - 1) / cib)), (unsigned)B);
    if (grid.y > 65535) return fail(GVX_ERR_UNSUPPORTED, "a layer of %d channels has too many channel tiles", l.cin);
    if (cpt == 8) md_dx_kernel<8><<<grid, 64 * lanes, 0, s>>>(p);
    else md_dx_kernel<4><<<grid, 64 * lanes, 0, s>>>(p);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int md_launch_pool(const float* x, float* y, const int32_t* lens, int B, int n_max, int min_n, int k, hipStream_t s) {
    // scale k's waveform from scale k - 1's
    const int xs = n_max >> (k - 1), ys = n_max >> k;
    md_pool_kernel<<<dim3((unsigned)((ys + 255) / 256), (unsigned)B), 256, 0, s>>>(x, y, lens, n_max, min_n, k - 1, xs, ys);
    HIP_TRY(hipGetLastError());
    return GVX_OK;
}

int md_check_call(const gvx_melgan_disc* h, const float* wav, const void* features, int B, int n_max) {
    if (const int rc = dc_check_call(h, wav, features, B)) return rc;
    if (n_max < md_min_samples(h->d))
        return fail(GVX_ERR_INVALID_ARG, "n_max = %d: the last scale's reflection needs at least %d samples", n_max, md_min_samples(h->d));
    if (n_max > GVX_MELGAN_DISC_MAX_SAMPLES) return fail(GVX_ERR_UNSUPPORTED, "n_max = %d is beyond the limit of %d samples", n_max, GVX_MELGAN_DISC_MAX_SAMPLES);
    return GVX_OK;
}

std::string md_name(int k, int i, int) { return "scales." + std::to_string(k) + ".layers." + std::to_string(i); }

bool md_shape_ok(const gvx_melgan_disc_dims* d, int B, int n_max) {
    return !md_dims_problem(d) && B >= 1 && B <= 65535 && n_max >= md_min_samples(*d) && n_max <= GVX_MELGAN_DISC_MAX_SAMPLES;
}

}  // namespace

extern "C" {

size_t gvx_melgan_disc_blob_floats(const gvx_melgan_disc_dims* dims) {
    if (md_dims_problem(dims)) return 0;
    MdLayer L[MD_MAX_LAYERS];
    size_t per_scale = 0;
    md_layers(*dims, L, &per_scale);
    return per_scale * dims->n_scales;
}

int gvx_melgan_disc_layout(const gvx_melgan_disc_dims* dims, int B, int n_max, gvx_melgan_disc_entry* entries, int max_entries) {
    if (!md_shape_ok(dims, B, n_max)) return 0;
    const MdFeat F = md_feat_layout(*dims, B, n_max);
    int n = 0;
    for (int k = 0; k < dims->n_scales; ++k)
        for (int i = 0; i < F.n_layers; ++i, ++n)
            if (entries && n < max_entries) entries[n] = gvx_melgan_disc_entry{(uint64_t)F.off[k][i], F.channels[i], F.positions[k][i]};
    return n;
}

size_t gvx_melgan_disc_features_bytes(const gvx_melgan_disc_dims* dims, int B, int n_max) {
    if (!md_shape_ok(dims, B, n_max)) return 0;
    return md_feat_layout(*dims, B, n_max).total;
}

size_t gvx_melgan_disc_workspace_bytes(const gvx_melgan_disc_dims* dims, int B, int n_max, int backward) {
    if (!md_shape_ok(dims, B, n_max)) return 0;
    return md_ws_plan(*dims, B, n_max, backward != 0).total;
}

int gvx_melgan_disc_pack_weights_device(const gvx_melgan_disc_dims* dims, const gvx_weight_desc* table, int n, float* device_blob, void* stream) {
    if (const char* why = md_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    if (!table || n < 1 || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    MdLayer L[MD_MAX_LAYERS];
    size_t per_scale = 0;
    const int nl = md_layers(*dims, L, &per_scale);
    gvx_gen::GenPacker P{{table, n}};
    for (int k = 0; k < dims->n_scales; ++k)
        for (int i = 0; i < nl; ++i) {
            const std::string name = md_name(k, i, nl);
            P.take(name + ".weight", k * per_scale + L[i].w_off, L[i].wn());
            P.take(name + ".bias", k * per_scale + L[i].b_off, (size_t)L[i].cout);
        }
    return P.run(device_blob, 0, per_scale * dims->n_scales, (hipStream_t)stream);
}

int gvx_melgan_disc_create(const gvx_melgan_disc_dims* dims, gvx_melgan_disc** out) {
    if (!out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (const char* why = md_dims_problem(dims)) return fail(GVX_ERR_INVALID_ARG, "%s", why);
    gvx_melgan_disc* h = new gvx_melgan_disc();
    h->d = *dims;
    *out = h;
    return GVX_OK;
}

void gvx_melgan_disc_destroy(gvx_melgan_disc* h) { delete h; }

int gvx_melgan_disc_bind(gvx_melgan_disc* h, const float* device_blob) { return gen_bind(h, device_blob); }

int gvx_melgan_disc_forward(gvx_melgan_disc* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, void* features,
                            size_t features_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = md_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    const gvx_melgan_disc_dims& d = h->d;
    const MdFeat F = md_feat_layout(d, B, n_max);
    if ((rc = dc_check_features(features, features_bytes, F.total)) != GVX_OK) return rc;
    const MdWs wp = md_ws_plan(d, B, n_max, false);
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    MdLayer L[MD_MAX_LAYERS];
    size_t per_scale = 0;
    const int nl = md_layers(d, L, &per_scale);
    const float* x = wav;
    for (int k = 0; k < d.n_scales; ++k) {
        if (k > 0) {
            float* pooled = gvx::ws_ptr<float>(workspace, wp.pooled[k]);
            if ((rc = md_launch_pool(x, pooled, sample_lengths, B, n_max, md_min_samples(d), k, s)) != GVX_OK) return rc;
            x = pooled;
        }
        const float* in = x;
        for (int i = 0; i < nl; ++i) {
            MdConv p = md_conv(d, L[i], F, k, i, sample_lengths, n_max);
            p.x = in; p.W = h->blob + k * per_scale + L[i].w_off; p.bias = h->blob + k * per_scale + L[i].b_off;
            p.y = gvx::ws_ptr<float>(features, F.off[k][i]);
            if ((rc = md_launch_fwd(p, L[i], B, s)) != GVX_OK) return rc;
            in = p.y;
        }
    }
    return GVX_OK;
}

int gvx_melgan_disc_backward(gvx_melgan_disc* h, const float* wav, const int32_t* sample_lengths, int B, int n_max, const void* features,
                             const void* d_features, const gvx_grad_desc* grads, int n_grads, float* d_wav,
                             void* workspace, size_t workspace_bytes, void* stream) {
    int rc;
    if ((rc = md_check_call(h, wav, features, B, n_max)) != GVX_OK) return rc;
    if ((rc = dc_check_backward(features, d_features, grads, n_grads, d_wav)) != GVX_OK) return rc;
    const gvx_melgan_disc_dims& d = h->d;
    const MdFeat F = md_feat_layout(d, B, n_max);
    const MdWs wp = md_ws_plan(d, B, n_max, true);
    if ((rc = gen_check_workspace(workspace, workspace_bytes, wp.total)) != GVX_OK) return rc;
    MdLayer L[MD_MAX_LAYERS];
    size_t per_scale = 0;
    const int nl = md_layers(d, L, &per_scale);
    DcParam g[GVX_MELGAN_DISC_MAX_SCALES * MD_MAX_LAYERS] = {};
    if ((rc = dc_find_grads(grads, n_grads, d.n_scales, L, nl, g, md_name)) != GVX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int min_n = md_min_samples(d);
    for (int k = 1; k < d.n_scales; ++k)   // the pooled waveforms again: the forward's workspace is not the backward's
        if ((rc = md_launch_pool(k == 1 ? wav : gvx::ws_ptr<float>(workspace, wp.pooled[k - 1]), gvx::ws_ptr<float>(workspace, wp.pooled[k]),
                                 sample_lengths, B, n_max, min_n, k, s)) != GVX_OK)
            return rc;
    float* gbuf[2] = {gvx::ws_ptr<float>(workspace, wp.grad[0]), gvx::ws_ptr<float>(workspace, wp.grad[1])};
    float* parts = gvx::ws_ptr<float>(workspace, wp.parts);
    auto feat = [&](const void* base, int k, int i) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + F.off[k][i]); };
    for (int k = d.n_scales - 1; k >= 0; --k) {
        const float* xk = k == 0 ? wav : gvx::ws_ptr<float>(workspace, wp.pooled[k]);
        const float* dcur = feat(d_features, k, nl - 1);   // the score has no activation: its cotangent is its pre-activation's
        for (int i = nl - 1; i >= 0; --i) {
            MdConv p = md_conv(d, L[i], F, k, i, sample_lengths, n_max);
            p.W = h->blob + k * per_scale + L[i].w_off;
            p.dy = dcur;
            if (n_grads > 0) {
                p.x = i == 0 ? xk : feat(features, k, i - 1);
                const MdPieces P = md_pieces(L[i], B, p.lout_max);
                const int cpt = (L[i].cog % 4) ? 1 : 4;
                const dim3 grid((unsigned)((P.numel / cpt + 255) / 256), (unsigned)P.n);
                if (cpt == 4) md_dw_kernel<4><<<grid, 256, 0, s>>>(p, parts, B, P.chunks, P.rows_per_piece);
                else md_dw_kernel<1><<<grid, 256, 0, s>>>(p, parts, B, P.chunks, P.rows_per_piece);
                HIP_TRY(hipGetLastError());
                md_reduce_kernel<<<(unsigned)((P.numel + 255) / 256), 256, 0, s>>>(parts, g[k * nl + i].w, P.numel, P.n);
                HIP_TRY(hipGetLastError());
                md_db_kernel<<<(unsigned)L[i].cout, 256, 0, s>>>(p, g[k * nl + i].b, B);
                HIP_TRY(hipGetLastError());
            }
            if (i > 0) {
                p.x = feat(features, k, i - 1);
                p.dfeat = feat(d_features, k, i - 1);
                p.y = gbuf[i & 1];
                if ((rc = md_launch_dx(p, L[i], B, s)) != GVX_OK) return rc;
                dcur = p.y;
            } else if (d_wav) {
                p.y = k == 0 ? d_wav : gvx::ws_ptr<float>(workspace, wp.d_pooled[k]);
                const float* d_next = k + 1 < d.n_scales ? gvx::ws_ptr<float>(workspace, wp.d_pooled[k + 1]) : nullptr;
                md_dx0_kernel<<<dim3((unsigned)((p.lin_max + 255) / 256), (unsigned)B), 256, 0, s>>>(p, d_next, n_max >> (k + 1));
                HIP_TRY(hipGetLastError());
            }
        }
    }
    return GVX_OK;
}

}  // C ABI
