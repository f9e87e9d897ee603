// selection_write.h — how a select call of the model operations writes the selection (gsx_model_select_range / _neighbors /
// _clusters / _knn), written once: k_property<., kPropSelect>, k_nb_select, k_cl_select and k_knn_select decide a lane's `hit` and
// call select_write; what follows — who owns a word, the op, the tail, the counts, the partial and its sum — is here.  Device code
// and its launch; the host side of a select is gsx_state.h's select_begin / select_end.
#pragma once
#include "edit_math.h"
#include "gsx_internal.h"
#include "wave_reduce.h"

namespace gsx {

struct SelectCounts {  // of the words a lane wrote: lanes 0 and 32 of a wave
    uint32_t hit = 0, selected = 0;
};

// Gaussian i (i < n or not) is hit or not: the wave's 64 hits are balloted into its two selection words; lanes 0 and 32 apply the op
// to the word they read — nothing, where the buffer stands for "none selected" — clear the tail and store.  A wave's 64 consecutive
// Gaussians start at a multiple of 64, so this lane reads and writes the word of its 32 and no other wave touches it; the wave's
// lanes have read what they need of the words before (prop_keep: the selection as it was before the call).  Called by all 64 lanes.
__device__ inline void select_write(const SelectionWrite& sel, bool hit, uint64_t i, uint64_t n, SelectCounts& c) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long hits64 = __ballot(hit);
    if ((lane & 31u) == 0u && i < n) {
        const uint64_t w = i >> 5;
        const uint32_t hits = (uint32_t)(hits64 >> lane);
        const uint32_t old = sel.valid ? sel.words[w] : 0u;
        const uint32_t now = prop_apply_op(sel.op, old, hits) & extract_tail_mask(n, w);
        sel.words[w] = now;
        c.hit += extract_popc(hits);
        c.selected += extract_popc(now);
    }
}

__device__ inline SelectCounts select_fold(SelectCounts c) {
    c.hit = wave_sum(c.hit);
    c.selected = wave_sum(c.selected);
    return group_fold(c, [](SelectCounts a, const SelectCounts& b) { return SelectCounts{a.hit + b.hit, a.selected + b.selected}; });
}

// The workgroup's partial, plain stores ("Model properties": atomics on a few words cost more than the stream).
// Called by every thread of the workgroup of 256.
__device__ inline void select_store_partial(const SelectionWrite& sel, SelectCounts c) {
    c = select_fold(c);
    if (threadIdx.x == 0u) {
        uint32_t* p = sel.partials + (size_t)blockIdx.x * kSelectPartialWords;
        p[0] = c.hit;
        p[1] = c.selected;
    }
}

// One workgroup: the partials' sums (integer adds: the same bits in any order).  One copy per translation unit that launches it.
static __global__ __launch_bounds__(256) void k_select_finish(const uint32_t* __restrict__ partials, uint32_t n_partials, uint32_t* __restrict__ hit_out,
                                                              uint32_t* __restrict__ selected_out) {
    SelectCounts c;
    for (uint32_t j = threadIdx.x; j < n_partials; j += 256u) {
        c.hit += partials[(size_t)j * kSelectPartialWords + 0u];
        c.selected += partials[(size_t)j * kSelectPartialWords + 1u];
    }
    c = select_fold(c);
    if (threadIdx.x == 0u) {
        *hit_out = c.hit;
        *selected_out = c.selected;
    }
}
inline hipError_t launch_select_finish(hipStream_t s, const SelectionWrite& sel, uint32_t n_partials, uint32_t* hit_out, uint32_t* selected_out) {
    GSX_LAUNCH(k_select_finish, dim3(1), dim3(256), 0, s, sel.partials, n_partials, hit_out, selected_out);
    return hipGetLastError();
}

}  // namespace gsx
