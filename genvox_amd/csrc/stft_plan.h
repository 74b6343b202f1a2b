// The plan host of the STFT-framed calls - csrc/stft_loss.hip, csrc/mel_loss.hip, csrc/denoise.hip - beside the transforms of
// fft_lds.h: the window and twiddle tables in float64, their upload, the workspace's regions and checks, the dispatch on n_fft, and the
// read-back of the rows' lengths behind the launches.  When a plan uploads (at create, or at its first call), what it pads its tables
// to and how it words a row's range stay with the plan.
#pragma once
#include "gvx_internal.h"
#include "rounding.h"

#include <cmath>
#include <type_traits>
#include <vector>

namespace gvx_plan {

using gvx::fail;

// appended to h: a Hann window of win_length centred in n_fft floats, then w_H^m (m < H = n_fft / 2) and w_N^k (k <= H) as float2
struct StftTables { size_t win, tw, tw2; };   // offsets in floats

inline StftTables stft_tables(std::vector<float>& h, int n_fft, int win_length) {
    const double two_pi = 6.283185307179586476925286766559;
    const int N = n_fft, H = N / 2, off = (N - win_length) / 2;
    StftTables t{};
    t.win = h.size();
    h.resize(h.size() + N, 0.f);
    for (int k = 0; k < win_length; ++k) h[t.win + off + k] = (float)(0.5 - 0.5 * std::cos(two_pi * k / win_length));
    t.tw = h.size();
    for (int m = 0; m < H; ++m) { h.push_back((float)std::cos(two_pi * m / H)); h.push_back((float)-std::sin(two_pi * m / H)); }
    t.tw2 = h.size();
    for (int k = 0; k <= H; ++k) { h.push_back((float)std::cos(two_pi * k / N)); h.push_back((float)-std::sin(two_pi * k / N)); }
    return t;
}

// host -> a new device array; false, with nothing allocated and *dev null, when the device refuses
template <class T>
bool stft_upload(T** dev, const std::vector<T>& host) {
    if (hipMalloc(dev, host.size() * sizeof(T)) == hipSuccess && hipMemcpy(*dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice) == hipSuccess)
        return true;
    if (*dev) (void)hipFree(*dev);
    *dev = nullptr;
    return false;
}

struct StftRegions {   // a workspace's regions, each rounded to 256 bytes: take() gives a region's byte offset
    size_t total = 0;
    size_t take(size_t bytes) { const size_t o = total; total += gvx::round256(bytes); return o; }
};

inline int stft_check_workspace(const void* workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || ((uintptr_t)workspace & 255)) return fail(GVX_ERR_WORKSPACE, "the workspace must be non-null and 256-byte aligned");
    if (workspace_bytes < need) return fail(GVX_ERR_WORKSPACE, "workspace too small: %zu bytes, %zu needed", workspace_bytes, need);
    return GVX_OK;
}

// f(std::integral_constant<int, n_fft / 2>) for the three sizes a plan accepts
template <class F>
int stft_dispatch(int n_fft, F&& f) {
    switch (n_fft) {
        case 512: return f(std::integral_constant<int, 256>{});
        case 1024: return f(std::integral_constant<int, 512>{});
        default: return f(std::integral_constant<int, 1024>{});
    }
}

// The rows' lengths live on the device: the kernels gave a refused row no frames, and the host learns of it here, behind the launches,
// so that its wait overlaps their run.  The first row outside [n_min, n_max] is named, `least` being the plan's words for n_min, after
// d_pred [B][n_max] (nullptr: the call has none) is zeroed.
inline int stft_check_lengths(const int32_t* lens, int B, long n_max, int n_min, const char* least, float* d_pred, hipStream_t s) {
    if (!lens) return GVX_OK;
    std::vector<int32_t> host(B);
    HIP_TRY(hipMemcpyAsync(host.data(), lens, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int b = 0; b < B; ++b) {
        if (host[b] >= n_min && host[b] <= n_max) continue;
        if (d_pred) HIP_TRY(hipMemsetAsync(d_pred, 0, (size_t)B * n_max * sizeof(float), s));
        return fail(GVX_ERR_SHAPE, "row %d has %d samples: outside [%s = %d, n_max = %ld]", b, host[b], least, n_min, n_max);
    }
    return GVX_OK;
}

}  // namespace gvx_plan
