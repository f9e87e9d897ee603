// neighbors_grid.h — the device side of the hashed grid that kernels_neighbors.hip builds, written once for the kernels that read it
// (kernels_neighbors / _clusters / _knn / _decimate.hip): the grid's frame, loaded once per kernel, the three-axis cell of a position,
// and the walk over the 27 cells around a cell.  The arithmetic is neighbors_math.h's (nb_cell: the ONLY copy).  The host
// restatements of the walk in tests/*_driver.cpp are the references the GPU tests compare against and do not include this file.
#pragma once
#include "gsx_internal.h"
#include "neighbors_math.h"

namespace gsx {

// What a kernel reads of a grid once: the origin (the participants' minimum), 1 / the cell edge, the table's bits, the participants.
struct NbFrame {
    float ox, oy, oz, inv_h;
    uint32_t bits, total;
};
__device__ inline NbFrame nb_frame(const NeighborJob& job) {
    return NbFrame{__uint_as_float(job.result[kNbOrigin + 0]), __uint_as_float(job.result[kNbOrigin + 1]), __uint_as_float(job.result[kNbOrigin + 2]),
                   job.inv_h, job.bits, job.result[kNbCount]};
}

struct NbCell {
    uint32_t x, y, z;
};
__device__ inline bool operator==(const NbCell& a, const NbCell& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
// the cell of a finite position at or above the origin, given as float bits (a position + colour element, a record)
__device__ inline NbCell nb_cell3(const NbFrame& g, const uint4& e) {
    return NbCell{nb_cell(__uint_as_float(e.x), g.ox, g.inv_h), nb_cell(__uint_as_float(e.y), g.oy, g.inv_h), nb_cell(__uint_as_float(e.z), g.oz, g.inv_h)};
}
__device__ inline uint32_t nb_bucket(const NbFrame& g, const NbCell& c) { return nb_bucket(c.x, c.y, c.z, g.bits); }

// The cell a walk is visiting, as the visitor sees it.  holds(r): is the record's own cell the visited cell?  A cell's bucket holds
// other cells' records too, and two of the 27 cells that share a bucket would otherwise give a record twice: a record counts only
// where holds(r) is true, which is in exactly one of the 27 visits, or in none.
struct NbVisit {
    const NbFrame& g;
    NbCell cell;
    __device__ bool holds(const uint4& r) const { return nb_cell3(g, r) == cell; }
};

// The walk: the 27 cells around `own`, for each the bucket it hashes to, from the bucket's start (the end of the bucket before) to its
// end (checked against the participant count), every record handed to visit(record, NbVisit) -> go on?  The visitor decides the
// order of its own tests and ends the whole walk by returning false.
//
// Why a pair with d2 <= r2 lies in cells that differ by at most 1 per axis (the walk visits 27 cells and must miss nobody):
//   d2 is a rounded sum of non-negative terms, so d2 <= r2 gives fl(dx * dx) <= r2 for every axis, and |dx| <= rmax, the largest
//   float32-representable bound with fl(rmax^2) <= r2: nb_grid takes sqrt(nextafter(r2, inf)) in double, which is above it also where
//   r2 is a denormal.  dx = fl(xj - xi), so the real difference is at most rmax (1 + 2^-24).
//   The cell edge is h = rmax (1 + 2^-5).  u(x) = fl(fl(x - origin) * inv_h) with inv_h = fl(1 / h) is monotone in x (every step is
//   a correctly rounded monotone operation), and so is the cell c(x) = min(floor(u), kNbMaxCell) (x >= origin: u >= 0).  For xi <=
//   xj of a pair: if c(xi) is the clamp, so is c(xj).  Otherwise u(xi) < 2^15, and both u differ from the real t = (x - origin) / h
//   by three roundings, at most 3.0001 * 2^-24 * (2^15 + 1) < 0.0059 each (an underflowing product errs by 2^-150, far less).  The
//   real t differ by at most (1 + 2^-24) / (1 + 2^-5) (1 + 2^-23) < 0.9698 (the last factor: h's own rounding).  So u(xj) - u(xi) <
//   0.9698 + 0.0118 < 1 and floor(u(xj)) <= floor(u(xi)) + 1; the clamp is monotone and only joins cells.  A difference x - origin
//   that overflows is +inf, its cell the clamp.  No NaN arises from finite inputs (inv_h is finite and positive: 1e-23 < h < 2e19).
// Below the origin (a query q of another model, nb_cell_signed; the records' own x stay at or above the origin): u is the same
//   monotone function for x < origin, where it is negative, and the bounds above hold for |u| < 2^15 whatever the sign: a pair (q, xj)
//   within rmax differs by less than 1 in u, so floor(u(xj)) - floor(u(q)) is -1, 0 or 1 also where u(q) < 0 (floor, not truncation:
//   nb_cell_signed takes floorf).  Every record has u >= 0, a cell of 0 or above.  So a query with floor(u(q)) = -1 finds its partners
//   in cell 0 alone, which the walk visits (the cells -2 and -1 wrap above kNbMaxCell and are dropped), and a query with floor(u(q))
//   <= -2 has u(q) < -1 <= u(xj) - 1 for every record: no record is within rmax on this axis.  nb_cell_signed returns -2 for all of
//   them, and for a difference that overflows to -inf: the caller skips the walk.  Above the box a query's cell may be the clamp while a
//   partner's is kNbMaxCell - 1 or the clamp: the clamp only joins cells, the difference stays at most 1.
template <class V>
__device__ inline void nb_walk(const NbFrame& g, const NeighborJob& job, const NbCell& own, V visit) {
    bool go = true;  // (tested where the loops test their ends, as a count against a cap would be: a return from inside costs more)
#pragma unroll 1
    for (uint32_t c = 0; c < 27u && go; ++c) {
        // (a coordinate below 0 wraps above kNbMaxCell: there is no such cell)
        const NbVisit v{g, NbCell{own.x + (c % 3u) - 1u, own.y + ((c / 3u) % 3u) - 1u, own.z + (c / 9u) - 1u}};
        if (v.cell.x > kNbMaxCell || v.cell.y > kNbMaxCell || v.cell.z > kNbMaxCell) continue;
        const uint32_t b = nb_bucket(g, v.cell);
        uint32_t q = b ? job.table[b - 1u] : 0u;
        const uint32_t end = min(job.table[b], g.total);
#pragma unroll 1
        for (; q < end && go; ++q) {
            // ONE 16-byte load, as a vector: read field by field through the visitor's reference, the record's index word becomes a
            // second, dependent load behind the distance test (measured: 12 % on the kNN)
            typedef uint32_t u4v __attribute__((ext_vector_type(4)));
            const u4v raw = *reinterpret_cast<const u4v*>(job.records + q);
            go = visit(make_uint4(raw.x, raw.y, raw.z, raw.w), v);
        }
    }
}

}  // namespace gsx
