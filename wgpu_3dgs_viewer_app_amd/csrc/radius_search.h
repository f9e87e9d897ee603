// radius_search.h — the schedule of a search by grid rounds at growing radii with an exact fallback, written once: the nearest
// neighbours (gsx_api_knn.cpp, spec/RENDER_SPEC.md §20), the nearest search across models (gsx_api_nearest.cpp, §23) and the host
// replays of both (tests/knn_driver.cpp, tests/nearest_driver.cpp) all run this loop, so the ORDER in which the rules of knn_math.h
// and nearest_math.h are applied cannot drift either: when the grid is rebuilt, at which radius, when a round is final, and that the
// radius handed to knn_go_brute is the radius of the round to come.  It holds the schedule and nothing else; the work is the
// caller's, as three callables:
//   grid(r, final)                build the grid of the participants at radius r; `final`: the round at r leaves nothing to a later one
//   round(i, U, final, &left)     round i (0, 1, ...) over the U unresolved entries, on the grid built last; left = how many stay
//                                 unresolved.  A final round need not report: what it did not answer has nothing within max_distance
//   brute(U)                      the exact fallback over the U entries left, against the records of the grid built last
// Each returns a Status that is 0 / false where it went well; the first that is not ends the search and is returned.  Which list a
// round reads and which it writes follows from i alone and is the caller's business.
// The nearest neighbours are the uncapped case, max_distance = 0: nearest_round_radius(r, floor, 0) is r, and no round is final: every
// radius is at most kKnnMaxRadius = 1.8e19, whose float32 square, 3.24e38, is below nearest_cap2(0) = kNearestUnlimited.
// Host only: <math.h> and the two rule headers, no HIP include.  Built with -ffp-contract=off wherever it is included.
#pragma once
#include <math.h>

#include "knn_math.h"
#include "nearest_math.h"

namespace gsx {

struct RadiusSearch {
    double ext[3];       // max - min per axis of the participants' whole box: the radius floor
    double trimmed[3];   // the same of their trimmed box: the first estimate, knn_coarse
    uint32_t P;          // the participants
    float hint;          // the caller's first radius, or 0: knn_first_radius for k
    uint32_t k;
    float max_distance;  // 0: none
    uint32_t max_rounds;
    float first_radius = 0.0f;  // what the search reports
    uint32_t rounds = 0, n_brute = 0;
};

// The whole search over U entries.  The first grid is built whatever U is.
template <class Status, class Grid, class Round, class Brute>
inline Status radius_search(RadiusSearch& s, uint32_t U, Grid&& grid, Round&& round, Brute&& brute) {
    const float floor_ = knn_radius_floor(s.ext), cap2 = nearest_cap2(s.max_distance);
    const auto final_at = [&](float r) { return nearest_final(nb_grid(r).r2, cap2); };
    float radius = nearest_round_radius(knn_clamp_radius(s.hint > 0.0f ? s.hint : knn_first_radius(s.trimmed, s.P, s.k), floor_), floor_, s.max_distance);
    bool final_round = final_at(radius);
    s.first_radius = radius;
    Status st = grid(radius, final_round);
    if (st) return st;
    float next = radius;  // the radius of the round to come, 0 where the radius cannot grow
    while (U && !knn_go_brute(U, s.P, s.rounds, s.max_rounds, next, knn_coarse(next, s.trimmed))) {
        if (s.rounds) {
            radius = next;
            final_round = final_at(radius);
            if ((st = grid(radius, final_round))) return st;
        }
        uint32_t left = 0;
        if ((st = round(s.rounds, U, final_round, &left))) return st;
        s.rounds += 1u;
        U = final_round ? 0u : left;
        next = knn_next_radius(radius);
        if (next != 0.0f) next = nearest_round_radius(next, floor_, s.max_distance);
    }
    s.n_brute = U;
    return U ? brute(U) : Status();
}

}  // namespace gsx
