// clusters_math.h — the union-find of the model clusters (spec/RENDER_SPEC.md §19, "Model clusters"), written once: the kernels of
// kernels_clusters.hip and the host program tests/clusters_driver.cpp both include it, so they cannot drift.  cl_find and cl_union
// are written against three primitives on the array parent[] that the caller supplies as a type P:
//   uint32_t load(uint32_t i)                            parent[i], an atomic read
//   uint32_t cas(uint32_t i, uint32_t expect, uint32_t v) compare-and-swap on parent[i]; returns the value it found
//   void     min(uint32_t i, uint32_t v)                  parent[i] = min(parent[i], v), atomically; the old value is not used
// The kernels map them to relaxed agent-scope atomics on global memory, the driver to relaxed std::atomic<uint32_t> operations.
// No HIP include; integer arithmetic only.
//
// The invariant: parent[i] <= i, and every write lowers the word it writes.  parent[i] = i at the start; cas(a, a, b) is only tried
// with b < a; min only lowers.  From it:
//   * no cycles: a parent chain strictly descends until it meets a word with parent[r] == r, a root;
//   * every loop ends: the words are bounded below by 0 and every failed compare-and-swap means that somebody lowered that word,
//     every step of cl_find moves to a smaller index.  Nobody waits for anybody: a lane that is alone still finishes;
//   * "in the same tree" only grows.  Roots disappear by a successful cas on a root alone (parent[a] == a was the value found): that
//     hooks a's whole tree under b's.  min rewires a non-root to a node that was its ancestor at an earlier time, so one of its own
//     tree then and, since trees only join, of its own tree now: the tree keeps its nodes and its root;
//   * when all unions are done, each tree is one cluster and its root, below all its descendants, is the cluster's smallest index.
// A stale value read from parent[] (an older link) is therefore only a longer way: it names a node of the same tree, at or above
// the index the word holds now; the walk from it still descends to the tree's current root, and the compare-and-swap that hooks a
// root acts on the word itself, not on what was read.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GSX_CL_HD __host__ __device__
#else
#define GSX_CL_HD
#endif

namespace gsx {

constexpr uint32_t kClNone = 0xFFFFFFFFu;  // GSX_CLUSTER_NONE: the label of a Gaussian that does not participate

// The root of i's tree as far as this caller can see; halves the path on the way (parent[cur] becomes its grandparent).
template <class P>
GSX_CL_HD inline uint32_t cl_find(P& p, uint32_t i) {
    uint32_t cur = i;
    for (;;) {
        const uint32_t par = p.load(cur);
        if (par == cur) return cur;
        const uint32_t grand = p.load(par);
        if (grand == par) return par;
        p.min(cur, grand);  // (grand < par < cur)
        cur = grand;
    }
}

// Join the trees of a and b: the larger root goes under the smaller.  A lost compare-and-swap (the root got a parent meanwhile)
// starts again from cl_find.  First the links of a and b themselves: two nodes with one parent are in one tree already, and that is
// what most pairs of a grown cluster look like (path halving has brought both right under the root), so the common case ends
// after two loads of words nobody contends for, without reading the root's word, which every lane of the cluster would read.
// Otherwise the search goes on from the two parents: a node's parent is in the node's tree.
template <class P>
GSX_CL_HD inline void cl_union(P& p, uint32_t a, uint32_t b) {
    {
        const uint32_t pa = p.load(a), pb = p.load(b);
        if (pa == pb) return;
        a = pa;
        b = pb;
    }
    for (;;) {
        a = cl_find(p, a);
        b = cl_find(p, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        if (p.cas(a, a, b) == a) return;  // a was still a root: hooked under b < a
    }
}

}  // namespace gsx
