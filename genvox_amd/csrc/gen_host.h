// The host side that the generators share - csrc/melgan.hip, hifigan.hip, bigvgan.hip, vocos.hip, univnet.hip, fastpitch.hip: what a
// handle holds besides its dims, the event marks and the stage times read off them, a row's own length (the roundings of the layouts
// are rounding.h's), the lookup of a tensor by name and the two packers built on it, and the argument checks that every forward
// makes with the same words.  What only one model needs stays in that model's file.
#pragma once
#include "gvx_internal.h"
#include "rounding.h"

#include <string>
#include <vector>

namespace gvx_gen {

using gvx::fail;


// frames of row b: lens[b] (nullptr: T) clamped to T; a row of fewer than `least` produces silence, never a bad address
__device__ __forceinline__ int gen_frames(const int32_t* lens, int b, int T, int least = 1) {
    int v = lens ? lens[b] : T;
    v = v > T ? T : v;
    return v < least ? 0 : v;
}

// ---- the handle: every gvx_<model> derives from GenHandle and adds its dims
struct GenMarks {   // events on the caller's stream, made by gen_timing_enable, destroyed with the handle
    std::vector<hipEvent_t> ev;
    GenMarks() = default;
    GenMarks(const GenMarks&) = delete;
    GenMarks& operator=(const GenMarks&) = delete;
    ~GenMarks() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

struct GenHandle {
    const float* blob = nullptr;
    bool timing = false;   // measurement only: marks around every stage of the last forward
    GenMarks marks;
    GenHandle() = default;
    GenHandle(const GenHandle&) = delete;   // the marks are the handle's own
    GenHandle& operator=(const GenHandle&) = delete;
};

inline int gen_bind(GenHandle* h, const float* device_blob) {
    if (!h || !device_blob) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if ((uintptr_t)device_blob % 256) return fail(GVX_ERR_INVALID_ARG, "the blob must be 256-byte aligned");
    h->blob = device_blob;
    return GVX_OK;
}

inline int gen_make_marks(GenMarks& m, int n_marks) {   // never fewer than there are: disabling keeps them for the next enabling
    while ((int)m.ev.size() < n_marks) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        m.ev.push_back(e);
    }
    return GVX_OK;
}

inline int gen_timing_enable(GenHandle* h, int enable, int n_marks) {
    if (!h) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (enable)
        if (const int rc = gen_make_marks(h->marks, n_marks)) return rc;
    h->timing = enable != 0;
    return GVX_OK;
}

// mark `at` of a call on the stream; nothing when the handle is not timed.  `marks`: a second list of the handle's (a backward's)
inline int gen_mark(const GenHandle* h, int at, hipStream_t s, const GenMarks* marks = nullptr) {
    if (h->timing) HIP_TRY(hipEventRecord((marks ? marks : &h->marks)->ev[at], s));
    return GVX_OK;
}

// the n times between n + 1 consecutive marks of the last timed call
inline int gen_stage_times_ms(const GenHandle* h, int n, float* ms_out, int* n_out, const GenMarks* marks = nullptr) {
    if (!h || !ms_out || !n_out) return fail(GVX_ERR_INVALID_ARG, "null argument");
    if (!h->timing) return fail(GVX_ERR_STATE, "timing is not enabled");
    const std::vector<hipEvent_t>& ev = (marks ? marks : &h->marks)->ev;
    HIP_TRY(hipEventSynchronize(ev[n]));
    for (int i = 0; i < n; ++i) HIP_TRY(hipEventElapsedTime(&ms_out[i], ev[i], ev[i + 1]));
    *n_out = n;
    return GVX_OK;
}

// ---- weights by name
// the entry `name` of a weight (or gradient) table, which must hold `numel` elements; NULL with rc set to the failure otherwise
inline const gvx_weight_desc* gen_find(const gvx_weight_desc* table, int n, const std::string& name, size_t numel, int& rc) {
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

// The lookups of one pack call: the first miss stays in rc, and every later find() does nothing and gives nullptr
struct GenLookup {
    const gvx_weight_desc* table;
    int n;
    int rc = GVX_OK;
    const float* find(const std::string& name, size_t numel) {
        if (rc != GVX_OK) return nullptr;
        const gvx_weight_desc* e = gen_find(table, n, name, numel, rc);
        return e ? e->data : nullptr;
    }
};

// A blob of tensors copied as they are.  take() looks a name up and launches nothing; run() returns the first miss, or clears
// blob[from, to) - the padding between the tensors - and copies.
struct GenPacker : GenLookup {
    struct Job { size_t dst; const float* src; size_t numel; };
    std::vector<Job> jobs;

    void take(const std::string& name, size_t dst, size_t numel) {
        if (const float* src = find(name, numel)) jobs.push_back({dst, src, numel});
    }
    int run(float* device_blob, size_t from, size_t to, hipStream_t s) const {
        if (rc != GVX_OK) return rc;
        HIP_TRY(hipMemsetAsync(device_blob + from, 0, (to - from) * sizeof(float), s));
        for (const Job& j : jobs) HIP_TRY(hipMemcpyAsync(device_blob + j.dst, j.src, j.numel * sizeof(float), hipMemcpyDeviceToDevice, s));
        return GVX_OK;
    }
};

// A blob of convolution weights in the implicit GEMM's order (MelGAN, HiFi-GAN), under GenPacker's rules.  run() is in melgan.hip,
// beside its two relayout kernels.
//   conv    Conv1d weight [Cout][Cin][k] -> dst[n * ld + off + tau * Cp + c], zeros for the padded channels c >= Cin
//   tconv   ConvTranspose1d weight [Cin][Cout][2r] -> dst[phase][n][tau * Cin + c]: the kernel tap that connects output r q + phase with
//           its tap-tau input
struct GenConvPacker : GenLookup {
    struct Job { bool tconv; size_t dst; const float* src; int a, b, c, k, ld, off; };   // conv: Cout a, Cin b, Cp c; tconv: Cin a, Cout b, r c
    std::vector<Job> jobs;

    void conv(const std::string& name, size_t dst, int Cout, int Cin, int Cp, int k, int ld, int off) {
        if (const float* src = find(name, (size_t)Cout * Cin * k)) jobs.push_back({false, dst, src, Cout, Cin, Cp, k, ld, off});
    }
    void bias(const std::string& name, size_t dst, int Cout) { conv(name, dst, Cout, 1, 1, 1, 1, 0); }
    void tconv(const std::string& name, size_t dst, int Cin, int Cout, int r) {
        if (const float* src = find(name, (size_t)Cin * Cout * 2 * r)) jobs.push_back({true, dst, src, Cin, Cout, r, 0, 0, 0});
    }
    int run(float* device_blob, size_t total, hipStream_t s) const;
};

// ---- workspaces: regions of B rows, every row rounded to 256 bytes; rows() gives a region's byte offset, `total` the bytes so far
struct GenRows {
    int B;
    size_t total = 0;
    size_t rows(size_t floats_per_row) {
        const size_t o = total;
        total += (size_t)B * gvx::round256(floats_per_row * sizeof(float));
        return o;
    }
};

// ---- the argument checks every forward makes
inline int gen_check_workspace(const void* workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || (uintptr_t)workspace % 256 || workspace_bytes < need)
        return fail(GVX_ERR_WORKSPACE, "the workspace is missing, misaligned or smaller than %zu bytes", need);
    return GVX_OK;
}

inline int gen_check_stage_out(float* const* stage_out, int n) {   // stage_out may be nullptr: no stage tensors are asked for
    if (stage_out)
        for (int i = 0; i < n; ++i)
            if (!stage_out[i] || (uintptr_t)stage_out[i] % 16) return fail(GVX_ERR_INVALID_ARG, "stage_out[%d] is null or not 16-byte aligned", i);
    return GVX_OK;
}

}  // namespace gvx_gen
