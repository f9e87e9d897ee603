// neighbors_math.h — the arithmetic of the neighbour counts (spec/RENDER_SPEC.md §18, "Model neighbours"), written once: the
// kernels of kernels_neighbors.hip, the host side of gsx_api_neighbors.cpp and the host restatement of tests/neighbors_driver.cpp
// all include it, so they cannot drift.  It holds the distance test, the grid (cell edge and its reciprocal from the radius), the
// cell of a coordinate (nb_cell: the ONLY copy) and the bucket of a cell.
// Plain float32 / integer arithmetic, <math.h> only; no HIP include (the functions are __host__ __device__ under hipcc).  Built with
// -ffp-contract=off wherever it is included.
//
// Why a pair with d2 <= r2 lies in cells that differ by at most 1 per axis — the walk over 27 cells misses nobody — is proven where
// the walk is written: neighbors_grid.h, nb_walk.  The proof rests on nb_grid and nb_cell as they stand here.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GSX_NB_HD __host__ __device__
#else
#define GSX_NB_HD
#endif

namespace gsx {

constexpr uint32_t kNbMaxCell = 32767u;   // cells 0 .. 2^15 - 1 per axis, counted from the participants' minimum
constexpr uint32_t kNbMaxBits = 24u;      // the bucket table has at most 2^24 entries
constexpr uint32_t kNbMaxCount = 4095u;   // GSX_NEIGHBOR_MAX_COUNT

GSX_NB_HD inline float nb_from_bits(uint32_t u) {
    float f;
    __builtin_memcpy(&f, &u, 4);
    return f;
}
GSX_NB_HD inline bool nb_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }  // false for NaN and +-inf

// d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded to float32
GSX_NB_HD inline float nb_d2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// Is the radius one a call accepts?  finite, above 0, its float32 square neither 0 nor inf
inline bool nb_radius_ok(float radius) {
    const float r2 = radius * radius;
    return nb_finite(radius) && radius > 0.0f && r2 > 0.0f && nb_finite(r2);
}

// The grid of a radius (host: the double square root is taken once a call).
struct NbGrid {
    float r2, h, inv_h;
};
inline NbGrid nb_grid(float radius) {
    NbGrid g;
    g.r2 = radius * radius;
    // (the float32 above r2; above the largest float32: the point from which a square would round to inf)
    const double above = g.r2 < 3.402823466e+38f ? (double)nextafterf(g.r2, INFINITY) : (double)g.r2 * (1.0 + 1.0 / 16777216.0);
    const double rmax = sqrt(above);
    g.h = (float)(rmax * (1.0 + 1.0 / 32.0));
    g.inv_h = 1.0f / g.h;
    return g;
}

// The cell of coordinate x along one axis: x finite, origin finite and <= x.
GSX_NB_HD inline uint32_t nb_cell(float x, float origin, float inv_h) {
    const float u = (x - origin) * inv_h;
    return u >= (float)kNbMaxCell ? kNbMaxCell : (uint32_t)u;  // (u >= 0; +inf clamps)
}

// The cell of a coordinate that need not lie at or above the origin (a query of another model: gsx_model_nearest, spec section 23):
// floor(u) for the same u, clamped to [-2, kNbMaxCell]; x and origin finite.  At or above the origin it is nb_cell's cell.  -1 is
// the cell below the grid's first, whose neighbour 0 holds records; -2 stands for every cell further down, none of whose neighbours
// holds any (neighbors_grid.h: nb_walk's proof, extended below the origin).  A difference that overflows to -inf gives -2.
GSX_NB_HD inline int32_t nb_cell_signed(float x, float origin, float inv_h) {
    const float u = floorf((x - origin) * inv_h);
    if (u >= (float)kNbMaxCell) return (int32_t)kNbMaxCell;
    return u >= -2.0f ? (int32_t)u : -2;
}

// The 32-bit hash of a cell; its low `bits` bits are the bucket.
GSX_NB_HD inline uint32_t nb_hash(uint32_t cx, uint32_t cy, uint32_t cz) {
    uint32_t k = cx * 0x9E3779B1u + cy * 0x85EBCA77u + cz * 0xC2B2AE3Du;
    k ^= k >> 15;
    k *= 0x2C1B3C6Du;
    k ^= k >> 12;
    k *= 0x297A2D39u;
    k ^= k >> 15;
    return k;
}
GSX_NB_HD inline uint32_t nb_bucket(uint32_t cx, uint32_t cy, uint32_t cz, uint32_t bits) { return nb_hash(cx, cy, cz) & ((1u << bits) - 1u); }

// The table the library chooses for a model of n Gaussians: about one bucket per Gaussian (the next power of two), 2^8 at least.
inline uint32_t nb_auto_bits(uint64_t n) {
    uint32_t bits = 8u;
    while (bits < kNbMaxBits && (uint64_t(1) << bits) < n) ++bits;
    return bits;
}

}  // namespace gsx
