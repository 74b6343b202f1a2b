// What the generators' backwards share - csrc/melgan_train.hip, csrc/hifigan_train.hip: a gradient's destination by name, the tape's
// slots and their export, the tape check (the workspace's is gen_check_workspace), and the two kernels at the ends of the walk.  The
// plans, the pieces, the reduce and weight-gradient kernels differ and stay with their models.
#pragma once
#include "gen_host.h"

namespace gvx_gen {

// where the gradient of `name` goes, which must hold `numel` elements; after a first miss (rc) every call does nothing
inline float* gen_grad(const gvx_grad_desc* table, int n, const std::string& name, size_t numel, int& rc) {
    if (rc != GVX_OK) return nullptr;
    for (int i = 0; i < n; ++i)
        if (table[i].name && name == table[i].name) {
            if (!table[i].data || table[i].numel != (int64_t)numel) {
                rc = fail(GVX_ERR_SHAPE, "the gradient of %s has %lld elements, the dims ask for %zu", name.c_str(), (long long)table[i].numel, numel);
                return nullptr;
            }
            return table[i].data;
        }
    rc = fail(GVX_ERR_MISSING_WEIGHT, "the gradient of %s has no destination", name.c_str());
    return nullptr;
}

// ---- the tape: every slot is [B][T * mul][C] at `off` floats
struct GenTapeSlot { size_t off; int mul, C; };

template <class Entry>   // a model's gvx_<model>_tape_entry -> the number of slots
int gen_tape_layout(const std::vector<GenTapeSlot>& slots, Entry* entries, int max_entries) {
    const int n = (int)slots.size();
    for (int i = 0; entries && i < n && i < max_entries; ++i) {
        entries[i].byte_offset = slots[i].off * sizeof(float);
        entries[i].positions_per_frame = slots[i].mul;
        entries[i].channels = slots[i].C;
    }
    return n;
}

inline int gen_check_tape(const void* tape, size_t tape_bytes, size_t need) {
    if (!tape || (uintptr_t)tape % 256 || tape_bytes < need) return fail(GVX_ERR_WORKSPACE, "the tape is missing, misaligned or smaller than %zu bytes", need);
    return GVX_OK;
}

// ---- the walk's first and last kernel; LEAST: the model's least frame count (gen_frames)
// dz = d_wav * (1 - wav^2) inside a row, 0 behind it (d_wav is not read there)
template <int LEAST>
__global__ void __launch_bounds__(256) gen_tanh_bwd_kernel(const float* d_wav, const float* wav, const int32_t* lens, int T, int hop, float* dz) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)T * hop) return;
    const size_t at = (size_t)b * T * hop + idx;
    float v = 0.f;
    if (idx < (long)gen_frames(lens, b, T, LEAST) * hop) {
        const float w = wav[at];
        v = d_wav[at] * (1.f - w * w);
    }
    dz[at] = v;
}

// d_mel [B][M][T] from its channels-last form [B][T][Cp]; exactly 0 at and behind a row's frames
template <int LEAST>
__global__ void __launch_bounds__(256) gen_dmel_kernel(const float* dmel_t, const int32_t* lens, int M, int T, int Cp, float* d_mel) {
    const int b = blockIdx.y;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)M * T) return;
    const int t = (int)(idx % T), c = (int)(idx / T);
    d_mel[(size_t)b * M * T + idx] = t < gen_frames(lens, b, T, LEAST) ? dmel_t[((size_t)b * T + t) * Cp + c] : 0.f;
}

}  // namespace gvx_gen
