// kernels_plane.hip — the plane of a model for gfx950 (spec/RENDER_SPEC.md §28, "Model plane"): gsx_model_fit_plane and
// gsx_model_select_plane.  The rules — the hash, the probe, the candidates, the residual, the inlier rule — are plane_math.h's.
//   k_plane_participants  k_property's chunk frame (a workgroup of 256 takes chunks of kExtractGroup = 1024 consecutive Gaussians, grid
//                         stride, the grid capped at kPropMaxGroups): the filter (prop_keep) and three finite coordinates, as bits;
//                         the participants and the filtered Gaussians without a finite position counted by integer adds;
//   k_plane_candidates    one lane per candidate: the probes against the participant bits, the plane of a triple or of a kept normal,
//                         or the caller's plane checked; an invalid candidate is stored with a NaN offset, so that nothing is its inlier;
//   k_plane_score         THE HOT PATH: N x H plane tests.  The same chunk frame.  A lane holds the chunk's four Gaussians it owns in
//                         registers (position; with min_cos the kept normal and the variation) and the wave's participant bits of
//                         each of the four rounds as a 64-bit mask in scalar registers.  The planes are read in the inner loop
//                         through a wave-uniform index into a kernel-argument pointer (scalar loads: 16 B serve 256 tests of the
//                         wave); a test is six float32 operations and one compare that writes the wave's ballot; the count of a
//                         plane over the wave's 256 Gaussians is four masked popcounts, scalar.  It is put into lane (h mod 64) of
//                         one register (a compare and a select), and after 64 planes every lane adds its plane's count to the workgroup's LDS
//                         counters: one LDS add a wave and 64 planes.  The counters are flushed once a workgroup, the non-zero ones
//                         by non-returning global integer adds, as kPropHist's bins are.  Integers: any order gives the same bits.
//   k_plane_moments       index order, one workgroup a chunk, twice a refine round: over the inliers of a plane, pass 0 the count, sum p
//                         and sum r^2, pass 1 about the float32 centre the six products of the float32 differences, taken and summed
//                         in double; one partial a workgroup (wave_sum, group_fold: combine_terms), folded in index order by
//                         k_plane_moments_finish, one workgroup: no float atomics, the same bits every call;
//   k_plane_select        k_property's select shape with the signed residual rule (select_write, k_select_finish).
// Every loop is bounded by n, by H <= 1024 or by 64 probes; no lane waits for another's progress.  Bounds: a Gaussian's index is
// checked against n before a load by it, a plane's index against H (<= kPlaneMaxCandidates, the planes', the counters' and the LDS
// array's length) before a load or an add by it.  Built with -ffp-contract=off.  Nothing of the model but the selection (k_plane_select)
// is written.
#include "gsx_internal.h"
#include "plane_math.h"
#include "selection_write.h"
#include "wave_reduce.h"

namespace gsx {

namespace {
__device__ inline Plane plane_of(const float4& q) { return Plane{{q.x, q.y, q.z}, q.w}; }
__device__ inline bool plane_bit(const uint32_t* __restrict__ words, uint64_t i) { return (words[i >> 5] >> (uint32_t)(i & 31u)) & 1u; }
constexpr uint32_t kMomentTerms = 6;  // pass 0 uses 5: count, sum p, sum r^2; pass 1 all: xx xy xz yy yz zz
static_assert(kMomentTerms <= kPlanePartialDoubles && 8u + kMomentTerms <= kPlaneSumDoubles, "the partials and the sums hold every term");
static_assert(kPlaneMaxCandidates % 64u == 0u && kPlaneMaxCandidates == GSX_PLANE_MAX_CANDIDATES, "whole waves of counters");
}  // namespace

__global__ __launch_bounds__(256) void k_plane_participants(uint64_t n, ModelFilter f, PlaneJob job) {
    const uint32_t t = threadIdx.x, lane = t & 63u;
    uint32_t count = 0, nonfinite = 0;
    const uint64_t chunks = extract_groups(n);
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t base = c * kExtractGroup;
#pragma unroll 1
        for (uint32_t k = 0; k < 4u; ++k) {
            if (base + k * 256u >= n) break;  // (uniform: the round holds no Gaussian)
            const uint64_t i = base + k * 256u + t;
            bool part = prop_keep(f, n, i, t);  // (every lane of the wave makes the call: a ballot inside)
            if (part) {
                const uint4 e = job.pc[i];
                part = pl_finite3(__uint_as_float(e.x), __uint_as_float(e.y), __uint_as_float(e.z));
                if (part) count += 1u;
                else nonfinite += 1u;
            }
            const unsigned long long part64 = __ballot(part);
            if (i < n && (lane & 31u) == 0u) job.participants[i >> 5] = (uint32_t)(part64 >> lane);  // (bits at and above n are clear)
        }
    }
    count = wave_sum(count);
    nonfinite = wave_sum(nonfinite);
    if (lane == 0u) {  // (integer sums: the same in any order)
        if (count) atomicAdd(job.words + kPlaneCount, count);
        if (nonfinite) atomicAdd(job.words + kPlaneNonfinite, nonfinite);
    }
}

__global__ __launch_bounds__(256) void k_plane_candidates(uint64_t n, PlaneJob job) {
    const uint32_t h = blockIdx.x * 256u + threadIdx.x;
    if (h >= job.n_candidates || h >= kPlaneMaxCandidates) return;
    const auto position = [&](uint32_t i, float p[3]) {
        const uint4 e = job.pc[i];
        p[0] = __uint_as_float(e.x);
        p[1] = __uint_as_float(e.y);
        p[2] = __uint_as_float(e.z);
    };
    Plane pl = pl_invalid();
    bool ok = false;
    if (job.sample == kPlaneSampleCaller) {
        pl = plane_of(job.planes[h]);
        ok = pl_caller_ok(pl);
    } else if (job.sample == kPlaneSampleNormals) {
        const uint32_t i = pl_probe(job.seed, h, 0u, n, [&](uint32_t j) { return plane_bit(job.participants, j) && nm_is_fitted(job.variation[j]); });
        if (i != kPlaneNone) {
            float a[3];
            position(i, a);
            const float k[3] = {job.normals[3u * (size_t)i], job.normals[3u * (size_t)i + 1u], job.normals[3u * (size_t)i + 2u]};
            pl = pl_from_normal(a, k);
            ok = true;
        }
    } else {
        uint32_t slot[3];
        for (uint32_t s = 0; s < 3u; ++s) slot[s] = pl_probe(job.seed, h, s, n, [&](uint32_t j) { return plane_bit(job.participants, j); });
        if (slot[0] != kPlaneNone && slot[1] != kPlaneNone && slot[2] != kPlaneNone && slot[0] != slot[1] && slot[0] != slot[2] && slot[1] != slot[2]) {
            float a[3], b[3], c[3];
            position(slot[0], a);
            position(slot[1], b);
            position(slot[2], c);
            ok = pl_from_triple(a, b, c, &pl);
        }
    }
    if (!ok) pl = pl_invalid();
    job.planes[h] = make_float4(pl.n[0], pl.n[1], pl.n[2], pl.offset);
    job.valid[h] = ok ? 1u : 0u;
}

// FACING: min_cos > 0.  `planes` is job.planes, H job.n_candidates: arguments of their own, so that both live in scalar registers.
template <bool FACING>
__global__ __launch_bounds__(256) void k_plane_score(uint64_t n, const float4* __restrict__ planes, uint32_t H, PlaneJob job) {
    __shared__ uint32_t s_count[kPlaneMaxCandidates];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    H = min(H, kPlaneMaxCandidates);
    for (uint32_t j = t; j < H; j += 256u) s_count[j] = 0u;
    __syncthreads();
    const float tolerance = job.tolerance, min_cos = job.min_cos;
    const uint64_t chunks = extract_groups(n);
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t base = c * kExtractGroup;
        // The lane's four Gaussians: loaded whether they participate or not (a lane beyond n loads Gaussian n - 1), so that the loads
        // are independent of each other; what a Gaussian outside the mask holds is never counted.
        float px[4], py[4], pz[4], kx[4], ky[4], kz[4], var[4];
        unsigned long long part[4];  // with FACING: the participants with a fitted kept normal
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            const uint64_t i = base + k * 256u + t, at = i < n ? i : n - 1u;
            const uint32_t word = job.participants[at >> 5];
            const uint4 e = job.pc[at];
            px[k] = __uint_as_float(e.x);
            py[k] = __uint_as_float(e.y);
            pz[k] = __uint_as_float(e.z);
            kx[k] = ky[k] = kz[k] = 0.0f;
            var[k] = INFINITY;
            if (FACING) {
                kx[k] = job.normals[3u * at];
                ky[k] = job.normals[3u * at + 1u];
                kz[k] = job.normals[3u * at + 2u];
                var[k] = job.variation[at];
            }
            part[k] = __ballot(i < n && ((word >> (uint32_t)(i & 31u)) & 1u) && (!FACING || nm_is_fitted(var[k])));  // (pl_facing's first half)
        }
        // the wave's inliers of one plane among its 256 Gaussians of the chunk (uniform)
        const auto count_of = [&](const Plane& pl) -> uint32_t {
            uint32_t cnt = 0u;
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) {
                unsigned long long in = __ballot(pl_inlier(pl_residual(pl, px[k], py[k], pz[k]), tolerance)) & part[k];
                if (FACING) in &= __ballot(pl_cos_ok(pl, kx[k], ky[k], kz[k], min_cos));  // (pl_facing's second half; the tests meet as masks)
                cnt += (uint32_t)__popcll(in);
            }
            return cnt;
        };
        for (uint32_t hb = 0; hb < H; hb += 64u) {
            const uint32_t m = min(64u, H - hb);
            uint32_t acc = 0u, j = 0u;
            for (; j + 4u <= m; j += 4u) {  // four planes a step: their 64 bytes are one scalar load (the index is uniform)
                Plane pl[4];
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) pl[u] = plane_of(planes[hb + j + u]);
#pragma unroll
                for (uint32_t u = 0; u < 4u; ++u) {
                    const uint32_t cnt = count_of(pl[u]);
                    acc = lane == j + u ? cnt : acc;  // (cnt and j are uniform: one compare, one select)
                }
            }
            for (; j < m; ++j) {
                const uint32_t cnt = count_of(plane_of(planes[hb + j]));
                acc = lane == j ? cnt : acc;
            }
            if (lane < m && acc) atomicAdd(&s_count[hb + lane], acc);
        }
    }
    __syncthreads();
    for (uint32_t j = t; j < H; j += 256u) {
        const uint32_t cnt = s_count[j];
        if (cnt) atomicAdd(&job.counts[j], cnt);
    }
}

// The sums over the inliers of `q` (spec section 28).  pass 0: [0] the count, [1..3] sum p, [4] sum r^2; pass 1, about the centre of pass
// 0's sums rounded to float32: d = p - c in float32, [0..5] the products xx xy xz yy yz zz of the differences taken in double.
__global__ __launch_bounds__(256) void k_plane_moments(uint64_t n, uint32_t pass, float4 q, PlaneJob job) {
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kExtractGroup;
    const Plane pl = plane_of(q);
    float c[3] = {0.0f, 0.0f, 0.0f};
    if (pass) {
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = pl_centre(job.sums[1 + a], job.sums[0]);
    }
    DoubleTerms<kMomentTerms> p;
#pragma unroll
    for (uint32_t k = 0; k < kMomentTerms; ++k) p.v[k] = 0.0;
#pragma unroll 1
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t i = base + k * 256u + t;
        if (i >= n) break;
        if (!plane_bit(job.participants, i)) continue;
        const uint4 e = job.pc[i];
        const float x[3] = {__uint_as_float(e.x), __uint_as_float(e.y), __uint_as_float(e.z)};
        const float r = pl_residual(pl, x[0], x[1], x[2]);
        if (!pl_inlier(r, job.tolerance)) continue;
        if (job.min_cos > 0.0f && !pl_facing(pl, job.normals[3u * i], job.normals[3u * i + 1u], job.normals[3u * i + 2u], job.variation[i], job.min_cos)) continue;
        if (pass == 0u) {
            p.v[0] += 1.0;
#pragma unroll
            for (int a = 0; a < 3; ++a) p.v[1 + a] += (double)x[a];
            p.v[4] += (double)r * (double)r;
            continue;
        }
        const double d[3] = {(double)(x[0] - c[0]), (double)(x[1] - c[1]), (double)(x[2] - c[2])};
        p.v[0] += d[0] * d[0];
        p.v[1] += d[0] * d[1];
        p.v[2] += d[0] * d[2];
        p.v[3] += d[1] * d[1];
        p.v[4] += d[1] * d[2];
        p.v[5] += d[2] * d[2];
    }
    p = combine_terms(p);
    if (t == 0u) {
        double* out = job.partials + (size_t)blockIdx.x * kPlanePartialDoubles;
#pragma unroll
        for (uint32_t k = 0; k < kMomentTerms; ++k) out[k] = p.v[k];
    }
}

// One workgroup: the partials in index order.
__global__ __launch_bounds__(256) void k_plane_moments_finish(uint32_t pass, uint32_t n_partials, PlaneJob job) {
    const uint32_t t = threadIdx.x;
    DoubleTerms<kMomentTerms> p;
#pragma unroll
    for (uint32_t k = 0; k < kMomentTerms; ++k) p.v[k] = 0.0;
    for (uint32_t j = t; j < n_partials; j += 256u) {
        const double* in = job.partials + (size_t)j * kPlanePartialDoubles;
#pragma unroll
        for (uint32_t k = 0; k < kMomentTerms; ++k) p.v[k] += in[k];
    }
    p = combine_terms(p);
    if (t != 0u) return;
    double* out = job.sums + (pass ? 8u : 0u);  // pass 0: [0..4]; pass 1: [8..13]
    const uint32_t terms = pass ? kMomentTerms : 5u;
#pragma unroll
    for (uint32_t k = 0; k < kMomentTerms; ++k)  // (unrolled: the terms stay in registers)
        if (k < terms) out[k] = p.v[k];
}

__global__ __launch_bounds__(256) void k_plane_select(uint64_t n, ModelFilter f, float4 q, PlaneJob job) {
    const uint32_t t = threadIdx.x;
    const Plane pl = plane_of(q);
    SelectCounts counts;
    const uint64_t chunks = extract_groups(n);
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t base = c * kExtractGroup;
#pragma unroll 1
        for (uint32_t k = 0; k < 4u; ++k) {
            if (base + k * 256u >= n) break;  // (uniform: the round holds no Gaussian)
            const uint64_t i = base + k * 256u + t;
            bool hit = prop_keep(f, n, i, t);  // (the selection as it was before the call: this wave alone writes the words it reads)
            if (hit) {
                const uint4 e = job.pc[i];
                const float x = __uint_as_float(e.x), y = __uint_as_float(e.y), z = __uint_as_float(e.z);
                hit = pl_finite3(x, y, z) && pl_in_range(pl_residual(pl, x, y, z), job.lo, job.hi);
                if (hit && job.min_cos > 0.0f)
                    hit = pl_facing(pl, job.normals[3u * i], job.normals[3u * i + 1u], job.normals[3u * i + 2u], job.variation[i], job.min_cos);
            }
            select_write(job.sel, hit, i, n, counts);
        }
    }
    select_store_partial(job.sel, counts);
}

namespace {
uint32_t plane_groups(uint64_t n) { return (uint32_t)std::min<uint64_t>(extract_groups(n), kPropMaxGroups); }
}  // namespace

hipError_t launch_plane_participants(hipStream_t s, uint64_t n, const ModelFilter& f, const PlaneJob& job) {
    GSX_LAUNCH(k_plane_participants, dim3(plane_groups(n)), dim3(256), 0, s, n, f, job);
    return hipGetLastError();
}
hipError_t launch_plane_candidates(hipStream_t s, uint64_t n, const PlaneJob& job) {
    GSX_LAUNCH(k_plane_candidates, dim3((job.n_candidates + 255u) / 256u), dim3(256), 0, s, n, job);
    return hipGetLastError();
}
hipError_t launch_plane_score(hipStream_t s, uint64_t n, const PlaneJob& job) {
    const dim3 grid(plane_groups(n)), block(256);
    if (job.min_cos > 0.0f) GSX_LAUNCH(k_plane_score<true>, grid, block, 0, s, n, job.planes, job.n_candidates, job);
    else GSX_LAUNCH(k_plane_score<false>, grid, block, 0, s, n, job.planes, job.n_candidates, job);
    return hipGetLastError();
}
hipError_t launch_plane_moments(hipStream_t s, uint64_t n, uint32_t pass, const float4& plane, const PlaneJob& job) {
    const uint32_t groups = (uint32_t)extract_groups(n);
    GSX_LAUNCH(k_plane_moments, dim3(groups), dim3(256), 0, s, n, pass, plane, job);
    GSX_LAUNCH(k_plane_moments_finish, dim3(1), dim3(256), 0, s, pass, groups, job);
    return hipGetLastError();
}
hipError_t launch_plane_select(hipStream_t s, uint64_t n, const ModelFilter& f, const float4& plane, const PlaneJob& job) {
    const uint32_t groups = plane_groups(n);
    GSX_LAUNCH(k_plane_select, dim3(groups), dim3(256), 0, s, n, f, plane, job);
    return launch_select_finish(s, job.sel, groups, job.words + kPlaneHit, job.words + kPlaneSelected);
}

}  // namespace gsx
