// clusters_driver.cpp — csrc/clusters_math.h (the lock-free union-find of the model clusters, spec §19) played on the host, for
// tests/test_clusters_cpu.py: a stand-alone program the test builds with the address and undefined-behaviour sanitizers.  The three
// primitives the header is written against are mapped to relaxed std::atomic<uint32_t> operations, and every edge list is united by
// 16 std::threads at once (thread t takes the edges t, t + 16, ...).  stdin, one command a line, numbers in decimal:
//   "edges <n> <a b> ..."     the given edge list on n nodes;              stdout "edges <checks> <label of 0> ... <label of n - 1>"
//   "random <seed> <n> <m>"   m random edges on n nodes (some repeated, some loops)
//   "chain <seed> <edges>"    the path 0 - 1 - ... - edges, its edges in shuffled order
//   "star <n> <hub>"          every node joined to the hub
//                                                                          stdout "<command> <checks> <clusters> <largest>"
// <checks> is 0 when, after the run: parent[i] <= i for every i; no walk along parent[] from any node takes more than n steps (no
// cycle); and the root cl_find reaches from every node is the smallest index of its component as a sequential breadth-first search
// over the same edges finds it.  Otherwise it is the number of nodes that fail.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "clusters_math.h"

using namespace gsx;

namespace {
constexpr uint32_t kThreads = 16;

struct Parent {
    std::atomic<uint32_t>* word;
    uint32_t load(uint32_t i) const { return word[i].load(std::memory_order_relaxed); }
    uint32_t cas(uint32_t i, uint32_t expect, uint32_t v) const {
        word[i].compare_exchange_strong(expect, v, std::memory_order_relaxed, std::memory_order_relaxed);
        return expect;  // (on failure: the value found)
    }
    void min(uint32_t i, uint32_t v) const {
        uint32_t old = word[i].load(std::memory_order_relaxed);
        while (v < old && !word[i].compare_exchange_weak(old, v, std::memory_order_relaxed, std::memory_order_relaxed)) {
        }
    }
};

struct Rng {  // splitmix64
    uint64_t s;
    uint32_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return (uint32_t)((z ^ (z >> 31)) >> 32);
    }
};

typedef std::vector<std::pair<uint32_t, uint32_t>> Edges;

// the smallest index of every node's component, by a sequential breadth-first search
std::vector<uint32_t> reference(uint32_t n, const Edges& e) {
    std::vector<uint32_t> start(n + 1u, 0u), adj(2u * e.size()), label(n, kClNone), queue;
    for (const auto& p : e) {
        start[p.first + 1u] += 1u;
        start[p.second + 1u] += 1u;
    }
    for (uint32_t i = 0; i < n; ++i) start[i + 1u] += start[i];
    std::vector<uint32_t> at(start.begin(), start.end() - 1);
    for (const auto& p : e) {
        adj[at[p.first]++] = p.second;
        adj[at[p.second]++] = p.first;
    }
    for (uint32_t i = 0; i < n; ++i) {  // (ascending: the first node that reaches a component is its smallest)
        if (label[i] != kClNone) continue;
        label[i] = i;
        queue.assign(1, i);
        while (!queue.empty()) {
            const uint32_t x = queue.back();
            queue.pop_back();
            for (uint32_t k = start[x]; k < start[x + 1u]; ++k) {
                if (label[adj[k]] == kClNone) {
                    label[adj[k]] = i;
                    queue.push_back(adj[k]);
                }
            }
        }
    }
    return label;
}

struct Outcome {
    unsigned long long failures, clusters, largest;
    std::vector<uint32_t> label;
};

Outcome play(uint32_t n, const Edges& e) {
    std::unique_ptr<std::atomic<uint32_t>[]> words(new std::atomic<uint32_t>[n]);
    for (uint32_t i = 0; i < n; ++i) words[i].store(i, std::memory_order_relaxed);
    Parent parent{words.get()};
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < kThreads; ++t)
        pool.emplace_back([&, t] {
            Parent mine = parent;
            for (size_t k = t; k < e.size(); k += kThreads) cl_union(mine, e[k].first, e[k].second);
        });
    for (auto& th : pool) th.join();
    const std::vector<uint32_t> want = reference(n, e);
    Outcome out{0, 0, 0, std::vector<uint32_t>(n)};
    std::vector<uint32_t> size(n, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        bool bad = parent.load(i) > i;
        uint32_t x = i, steps = 0;
        while (parent.load(x) != x && steps <= n) {  // (before cl_find halves anything: the forest as the threads left it)
            x = parent.load(x);
            steps += 1u;
        }
        bad = bad || steps > n || x != want[i];
        if (bad) out.failures += 1u;
    }
    for (uint32_t i = 0; i < n; ++i) {
        out.label[i] = cl_find(parent, i);
        if (out.label[i] != want[i] || parent.load(i) > i) out.failures += 1u;
        if (out.label[i] < n) size[out.label[i]] += 1u;
    }
    for (uint32_t i = 0; i < n; ++i) {
        if (out.label[i] == i) out.clusters += 1u;
        if (size[i] > out.largest) out.largest = size[i];
    }
    return out;
}
}  // namespace

int main() {
    std::string line;
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        line = buf;
        while (!line.empty() && line.back() != '\n' && fgets(buf, sizeof buf, stdin)) line += buf;
        const char* s = line.c_str();
        char cmd[32] = {0};
        int used = 0;
        if (sscanf(s, "%31s%n", cmd, &used) != 1) continue;
        s += used;
        std::vector<unsigned long long> w;
        char* end = nullptr;
        for (;;) {
            const unsigned long long x = strtoull(s, &end, 10);
            if (end == s) break;
            w.push_back(x);
            s = end;
        }
        Edges e;
        uint32_t n = 0;
        if (!strcmp(cmd, "edges")) {
            if (w.empty() || w.size() % 2 != 1 || w[0] < 1 || w[0] > (1u << 24)) return 2;
            n = (uint32_t)w[0];
            for (size_t k = 1; k < w.size(); k += 2) {
                if (w[k] >= n || w[k + 1] >= n) return 2;
                e.emplace_back((uint32_t)w[k], (uint32_t)w[k + 1]);
            }
        } else if (!strcmp(cmd, "random")) {
            if (w.size() != 3 || w[1] < 1 || w[1] > (1u << 24) || w[2] > (1u << 24)) return 2;
            Rng g{w[0] * 0x9E3779B97F4A7C15ull + 1u};
            n = (uint32_t)w[1];
            for (unsigned long long k = 0; k < w[2]; ++k) {
                const uint32_t a = g.next() % n, b = g.next() % n;
                e.emplace_back(a, b);
            }
        } else if (!strcmp(cmd, "chain")) {
            if (w.size() != 2 || w[1] < 1 || w[1] > (1u << 24)) return 2;
            Rng g{w[0] * 0x9E3779B97F4A7C15ull + 1u};
            n = (uint32_t)w[1] + 1u;
            for (uint32_t k = 0; k + 1u < n; ++k) e.emplace_back(k, k + 1u);
            for (size_t k = e.size(); k > 1; --k) std::swap(e[k - 1], e[g.next() % k]);
        } else if (!strcmp(cmd, "star")) {
            if (w.size() != 2 || w[0] < 1 || w[0] > (1u << 24) || w[1] >= w[0]) return 2;
            n = (uint32_t)w[0];
            for (uint32_t k = 0; k < n; ++k)
                if (k != w[1]) e.emplace_back(k, (uint32_t)w[1]);
        } else {
            return 3;
        }
        const Outcome out = play(n, e);
        if (!strcmp(cmd, "edges")) {
            printf("edges %llu", out.failures);
            for (uint32_t l : out.label) printf(" %u", l);
            printf("\n");
        } else {
            printf("%s %llu %llu %llu\n", cmd, out.failures, out.clusters, out.largest);
        }
    }
    return 0;
}
