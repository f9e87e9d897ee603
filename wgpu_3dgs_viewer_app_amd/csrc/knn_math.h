// knn_math.h — the rules of the nearest-neighbour search (spec/RENDER_SPEC.md §20, "Model nearest neighbours"), written once: the
// kernels of kernels_knn.hip, the host side of gsx_api_knn.cpp, radius_search.h (the order in which the radii and the fallback rule
// are applied: the library's loop, which tests/knn_driver.cpp runs too) and the driver's host version of the work all include it, so
// they cannot drift.  It holds the insertion chain that keeps a lane's K best, the rule that proves a row, the two scores, the
// outlier threshold, the search radii (floor, first estimate, growth) and the rule that sends the unresolved to the exact fallback.
// The distance, the cell and the grid are neighbors_math.h's; nothing of them is restated here.
// Plain float32 / double arithmetic, <math.h> only; no HIP include.  Built with -ffp-contract=off wherever it is included.
//
// Why a round is exact.  neighbors_math.h proves that every pair with d2 <= r2 lies in cells that differ by at most 1 per axis, so a
// lane that walks the 27 cells around its own sees every j with d2(i, j) <= r2, each once (the own-cell test).  Let b be the k-th
// smallest of what it saw and kept (d2 <= r2 only).  If b <= r2, any j it did not see has d2 > r2 >= b, and any j it saw and dropped
// has d2 > r2 >= b too: the k smallest it kept are the k smallest of D(i), as values with multiplicity.  If it kept fewer than k, b is
// +inf and the row is not proven.  A row whose true k-th value is +inf is never proven by a grid (r2 is finite): it ends in the
// exact fallback, which looks at every participant.
#pragma once
#include <math.h>
#include <stdint.h>

#include "neighbors_math.h"

#if defined(__clang__)
#define GSX_KNN_UNROLL _Pragma("unroll")  // the K registers stay registers only where the loops over them are unrolled
#else
#define GSX_KNN_UNROLL
#endif

namespace gsx {

constexpr uint32_t kKnnMaxK = 16u;            // GSX_KNN_MAX_K
constexpr uint32_t kKnnScoreKth = 0u;         // GSX_KNN_SCORE_KTH
constexpr uint32_t kKnnScoreMean = 1u;        // GSX_KNN_SCORE_MEAN
constexpr uint32_t kKnnSelectRange = 0u;      // GSX_KNN_SELECT_RANGE
constexpr uint32_t kKnnSelectOutliers = 1u;   // GSX_KNN_SELECT_OUTLIERS
constexpr uint32_t kKnnMaxRounds = 64u;       // the most grid rounds a caller may ask for
constexpr uint32_t kKnnBruteLanes = 256u;     // the lanes of one workgroup of the exact fallback: as many partial lists are merged
constexpr uint32_t kKnnDirect = 1024u;        // at most this many unresolved entries: the exact fallback answers them at once
constexpr uint64_t kKnnBudget = uint64_t(1) << 37;  // distance tests the exact fallback may be handed while a grid round could still run
constexpr double kKnnCoarse = 0.05;           // a cell edge from this share of the trimmed box's size on is coarse: see knn_coarse
constexpr float kKnnGrowth = 4.0f;            // the radius of the next round over this round's
constexpr float kKnnMinRadius = 1e-22f;       // the radii a search uses lie in [kKnnMinRadius, kKnnMaxRadius]: nb_radius_ok accepts both
constexpr float kKnnMaxRadius = 1.8e19f;
constexpr uint32_t kKnnTrimPermille = 10u;     // the library's first radius comes from the box that leaves 10 permille outside per side
constexpr double kKnnFloorCells = 32000.0;    // the largest extent spans at most this many cell edges (kNbMaxCell = 32767)

// The template a k runs under: the K best are K registers.
inline uint32_t knn_round_k(uint32_t k) { return k <= 4u ? 4u : (k <= 8u ? 8u : 16u); }

// The lane's k best in K registers, k <= K: b[K - k .. K - 1] hold them ascending, +inf where fewer were offered, and b[0 .. K - k - 1]
// are pinned at -inf, which no offer displaces (every d2 is +0 or above).  So the k-th best is always b[K - 1], a constant index, and
// nothing indexes the registers by k.  knn_insert offers one more value (not NaN): a compare-exchange chain over constant indices, so
// b[] stays in registers once the loop is unrolled.  Equal values all count.
template <int K>
GSX_NB_HD inline void knn_clear(float (&b)[K], uint32_t k) {
GSX_KNN_UNROLL
    for (int q = 0; q < K; ++q) b[q] = (uint32_t)q + k < (uint32_t)K ? -INFINITY : INFINITY;
}
template <int K>
GSX_NB_HD inline void knn_insert(float (&b)[K], float v) {
GSX_KNN_UNROLL
    for (int q = 0; q < K; ++q) {
        const float lo = fminf(b[q], v);
        v = fmaxf(b[q], v);
        b[q] = lo;
    }
}
// the k-th best: an offer that is not below it changes nothing
template <int K>
GSX_NB_HD inline float knn_kth(const float (&b)[K]) {
    return b[K - 1];
}
// Is the row of a lane that kept only candidates with d2 <= r2 out of its 27 cells the true row?
GSX_NB_HD inline bool knn_proven(float kth, float r2) { return kth <= r2; }

// The score of a row: correctly rounded float32 sqrt, adds and divide, in ascending order (the first add, to +0, is exact).
template <int K>
GSX_NB_HD inline float knn_score(const float (&b)[K], uint32_t k, uint32_t kind) {
    if (kind == kKnnScoreKth) return sqrtf(b[K - 1]);
    float s = 0.0f;
GSX_KNN_UNROLL
    for (int q = 0; q < K; ++q)
        if ((uint32_t)q + k >= (uint32_t)K) s = s + sqrtf(b[q]);
    return s / (float)k;
}
// The row's k values to out[0 .. k - 1].
template <int K>
GSX_NB_HD inline void knn_store(const float (&b)[K], uint32_t k, float* out) {
GSX_KNN_UNROLL
    for (int q = 0; q < K; ++q)
        if ((uint32_t)q + k >= (uint32_t)K) out[(uint32_t)q + k - (uint32_t)K] = b[q];
}

// The outlier threshold: the double expression, then one rounding to float32.
GSX_NB_HD inline float knn_threshold(double mean, double std, float std_ratio) {
    const double scaled = (double)std_ratio * std;
    return (float)(mean + scaled);
}
// The sample deviation from the sum of squared deviations of m values.
GSX_NB_HD inline double knn_std(double ss, uint64_t m) { return m < 2u ? 0.0 : sqrt(ss / (double)(m - 1u)); }

// A radius a search may use: inside [kKnnMinRadius, kKnnMaxRadius] and not below the floor that keeps the largest extent within
// kKnnFloorCells cells, so that the grid does not clamp the bulk of the model into its last cell.  ext: max - min per axis in double.
inline float knn_radius_floor(const double ext[3]) {
    const double largest = fmax(ext[0], fmax(ext[1], ext[2]));
    const double f = largest / kKnnFloorCells;
    return f >= (double)kKnnMaxRadius ? kKnnMaxRadius : (float)f;
}
inline float knn_clamp_radius(float radius, float floor_) {
    float r = radius > floor_ ? radius : floor_;  // (NaN never arrives: the hint is checked, the estimate is finite or +inf)
    if (r < kKnnMinRadius) r = kKnnMinRadius;
    if (r > kKnnMaxRadius) r = kKnnMaxRadius;
    return r;
}
// The library's own first radius: the ball that holds 2 k of P participants spread evenly over the box's non-degenerate extents
// (4.19 r^3, 3.14 r^2 or 2 r of them); 1 where the box is a point.  The host hands it the trimmed box (spec section 11), which a few
// far outliers do not inflate; the floor above comes from the whole box.
inline float knn_first_radius(const double ext[3], uint64_t P, uint32_t k) {
    double measure = 1.0;
    int dims = 0;
    for (int a = 0; a < 3; ++a)
        if (ext[a] > 0.0) {
            measure *= ext[a];
            ++dims;
        }
    const double per = (double)k * measure / (double)(P ? P : 1u);
    double r = 1.0;
    if (dims == 3) r = cbrt(0.48 * per);
    if (dims == 2) r = sqrt(0.64 * per);
    if (dims == 1) r = per;
    if (!(r < (double)kKnnMaxRadius)) return kKnnMaxRadius;
    return (float)r;
}
// The next round's radius, or 0 where the radius cannot grow any more.
inline float knn_next_radius(float radius) {
    const float next = radius * kKnnGrowth;
    return next <= kKnnMaxRadius ? next : 0.0f;
}

// Is a grid at radius `next` coarse for this model?  From a cell edge of a twentieth of the trimmed box's size (the geometric mean
// of its non-degenerate extents) a cell next to the bulk holds thousands of participants, and one lane walking 27 such cells alone
// is slower than the fallback's 256 lanes walking everybody: what is still unresolved then is far from everything.
inline bool knn_coarse(float next, const double trimmed[3]) {
    double measure = 1.0;
    int dims = 0;
    for (int a = 0; a < 3; ++a)
        if (trimmed[a] > 0.0) {
            measure *= trimmed[a];
            ++dims;
        }
    if (dims == 0) return false;
    const double size = dims == 3 ? cbrt(measure) : (dims == 2 ? sqrt(measure) : measure);
    return (double)next >= kKnnCoarse * size;
}

// After `rounds` grid rounds (0: before the first) U of P participants are unresolved (U > 0) and the radius of the round to come
// is `next` (0: there is none; `coarse`: knn_coarse of it).  Do they go to the exact fallback now?  They must where the radius
// cannot grow.  Otherwise never beyond the budget, whatever max_rounds says: the knob cannot start a kernel of U x P tests of any
// size.  Within the budget: once the caller's rounds are used up, once the entries are few enough that another grid would cost more
// than looking at everyone (which sends a model of up to kKnnDirect participants there at once), or, after at least one round,
// once the next grid would be coarse.
inline bool knn_go_brute(uint64_t U, uint64_t P, uint32_t rounds, uint32_t max_rounds, float next, bool coarse) {
    if (next == 0.0f) return true;
    if (U * P > kKnnBudget) return false;  // (U, P < 2^32)
    return (max_rounds != 0u && rounds >= max_rounds) || U <= kKnnDirect || (rounds >= 1u && coarse);
}

}  // namespace gsx
