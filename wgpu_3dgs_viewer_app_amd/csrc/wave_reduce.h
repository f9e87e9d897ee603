// wave_reduce.h — the reductions of the model operations' kernels (kernels_property / _neighbors / _clusters / _knn / _nearest /
// _decimate / _plane.hip), written once: a value over the 64 lanes of a wave, the four waves' values over a workgroup of 256, and the wave's
// append to a list (kernels_knn / _nearest.hip).  Device code only.  The frame pipeline's kernels keep their own, tuned per kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsx {

// Over the wave: an xor butterfly, offsets 32 down to 1.  Every lane ends with the same value, the same on every call: both lanes of
// a pair compute the same f(a, b), so a double sum's bits depend on the offset order alone.  Called by all 64 lanes.
template <class T, class F>
__device__ inline T wave_fold(T x, F f) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = f(x, (T)__shfl_xor(x, o, 64));
    return x;
}
__device__ inline uint32_t wave_sum(uint32_t x) { return wave_fold(x, [](uint32_t a, uint32_t b) { return a + b; }); }
__device__ inline double wave_sum(double x) { return wave_fold(x, [](double a, double b) { return a + b; }); }
__device__ inline float wave_min(float x) { return wave_fold(x, [](float a, float b) { return fminf(a, b); }); }
__device__ inline float wave_max(float x) { return wave_fold(x, [](float a, float b) { return fmaxf(a, b); }); }
__device__ inline uint32_t wave_min(uint32_t x) { return wave_fold(x, [](uint32_t a, uint32_t b) { return b < a ? b : a; }); }
__device__ inline uint32_t wave_max(uint32_t x) { return wave_fold(x, [](uint32_t a, uint32_t b) { return b > a ? b : a; }); }
__device__ inline uint64_t wave_min(uint64_t x) { return wave_fold(x, [](uint64_t a, uint64_t b) { return b < a ? b : a; }); }
__device__ inline uint64_t wave_max(uint64_t x) { return wave_fold(x, [](uint64_t a, uint64_t b) { return b > a ? b : a; }); }

// The wave's lanes with `on` draw consecutive slots of a list with one returning add (ballot, popcount, lane 0 adds, shuffle) and
// store their 16-byte entry there; a slot at or beyond `capacity` is not written.  The list's order differs from call to call.  Called
// by all 64 lanes.
__device__ inline void wave_append(bool on, const uint4& entry, uint4* __restrict__ list, uint32_t* __restrict__ list_count, uint64_t capacity) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long pending = __ballot(on);
    if (pending) {
        uint32_t slot0 = 0;
        if (lane == 0u) slot0 = atomicAdd(list_count, (uint32_t)__popcll(pending));
        slot0 = __shfl(slot0, 0, 64);
        if (on) {
            const uint32_t slot = slot0 + (uint32_t)__popcll(pending & ((1ull << lane) - 1ull));
            if (slot < capacity) list[slot] = entry;  // (always: a list takes at most as many entries as it has room for)
        }
    }
}

// Over the workgroup of 256: `mine` is already reduced over the wave.  Lane 0 of the waves 1..3 stores it to LDS (wave 0's stays in
// thread 0's registers), one barrier, and thread 0 folds the waves 0..3 in wave order: merge(merge(merge(wave 0, wave 1), wave 2),
// wave 3).  The result is valid in thread 0 alone.  Called by every thread, once per kernel and P: the LDS is 3 x sizeof(P) (P is
// copied as bytes: it may have member initialisers, which a __shared__ variable may not).
template <class P, class F>
__device__ inline P group_fold(P mine, F merge) {
    static_assert(__is_trivially_copyable(P), "copied through LDS as bytes");
    __shared__ __attribute__((aligned(alignof(P)))) unsigned char s_wave[3][sizeof(P)];
    const uint32_t t = threadIdx.x;
    if ((t & 63u) == 0u && t != 0u) __builtin_memcpy(s_wave[(t >> 6) - 1u], &mine, sizeof(P));
    __syncthreads();
    if (t == 0u) {
        for (uint32_t w = 0; w < 3u; ++w) {
            P theirs;
            __builtin_memcpy(&theirs, s_wave[w], sizeof(P));
            mine = merge(mine, theirs);
        }
    }
    return mine;
}

// T double sums a lane, folded over the wave and then over the workgroup's four waves in a fixed order (kernels_nearest.hip's align
// passes, kernels_plane.hip's moments): valid in thread 0 alone.  Called by every thread.
template <uint32_t T>
struct DoubleTerms {
    double v[T];
};
template <uint32_t T>
__device__ inline DoubleTerms<T> combine_terms(DoubleTerms<T> p) {
#pragma unroll
    for (uint32_t k = 0; k < T; ++k) p.v[k] = wave_sum(p.v[k]);
    return group_fold(p, [](DoubleTerms<T> a, const DoubleTerms<T>& b) {
#pragma unroll
        for (uint32_t k = 0; k < T; ++k) a.v[k] += b.v[k];
        return a;
    });
}

}  // namespace gsx
