// tools/check_admit.hip — the admission stage alone (csrc/kernels_admit.hip, csrc/window_scan.h, the window pyramid of
// csrc/kernels_spec.hip; all included as source) against a host compaction, at the counts and admitted sets where its
// kernels change path.  Every comparison is exact: integers, no tolerance.  Not part of the product.
//   hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 tools/check_admit.hip \
//         -Iwgpu_3dgs_viewer_app_amd/csrc -Iinclude -o tools/check_admit
//   tools/check_admit small | threshold | superscan | pages | handover | reuse | windows | pyramid
// One line per case (n, path, admitted, result); the first mismatch or HIP error ends the run with a non-zero status and
// nothing is launched behind it; a clean run ends with "<group>: <cases> cases, 0 mismatches".
//
// The buffer contract assumed is the library's own (gsx_frame.cpp, do_preprocess / ensure_msd):
//   * ballots: ceil(n / 64) words + 4; the words of the last 256-Gaussian projection workgroup exist and are zero past n
//     (the four words of padding behind them hold garbage here: nobody may read them for bits);
//   * per-workgroup counts (admitted, visible, offsets): their entries + 4 (k_admit_scan moves them as uint4); the padding
//     holds garbage here;
//   * the bucket sort's workspace: msd_workspace_words(n) words, msd_workspace_init;
//   * a visible record's tile rectangle is not empty and lies inside the grid (the projection culls the others).
#define GSX_LAUNCH_STANDALONE 1  // csrc/gsx_launch.h: launches submit at once, nothing of libgsx is linked
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_sort.hip"
#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_admit.hip"
#include "../wgpu_3dgs_viewer_app_amd/csrc/kernels_spec.hip"

using namespace gsx;
typedef unsigned long long u64h;

static const char* g_group = "";
static size_t g_cases = 0;

[[noreturn]] static void die(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vprintf(fmt, ap);
    va_end(ap);
    printf("\ncheck_admit %s: stopped after %zu cases\n", g_group, g_cases);
    fflush(stdout);
    exit(code);  // nothing is launched after a mismatch or a HIP error
}
#define CK(x)                                                                      \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) die(2, "HIP ERROR %s: %s", #x, hipGetErrorString(e_)); \
    } while (0)

// ---- the table of counts (every group draws from it), and what msd_workspace_words() promises about them: a workspace sized for one
// count serves every launch of a smaller one ----
static const uint32_t kSmallCounts[] = {1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385};
static const uint32_t kThresholdCounts[] = {4194240, 4194241, 4194304, 4194305};   // either side of kCompactSmallWords
static const uint32_t kSuperCounts[] = {10485760, 10485761, 10486017, 10500000};    // either side of k_admit_scan's 40 960-count super-tile
static const uint32_t kPageCounts[] = {73736, 81920, 1000000, 4194304};             // 4 tiles + 8200; 5 full tiles; 62 tiles; 64 tiles of 65 536
static const uint32_t kHandoverCounts[] = {1000000, 4194240, 4194241, 10000000};
static const uint32_t kWindowRecords = 200000;

static void check_workspace_sizes() {
    std::vector<uint32_t> all;
    for (uint32_t c : kSmallCounts) all.push_back(c);
    for (uint32_t c : kThresholdCounts) all.push_back(c);
    for (uint32_t c : kSuperCounts) all.push_back(c);
    for (uint32_t c : kPageCounts) all.push_back(c);
    for (uint32_t c : kHandoverCounts) all.push_back(c);
    all.push_back(kWindowRecords);
    for (uint32_t big : all)
        for (uint32_t small_ : all)
            if (small_ < big && msd_workspace_words(small_) > msd_workspace_words(big))
                die(1, "MISMATCH msd_workspace_words(%u) = %zu > msd_workspace_words(%u) = %zu: a launch of the smaller count overruns a workspace sized for the larger",
                    small_, msd_workspace_words(small_), big, msd_workspace_words(big));
    printf("workspace sizes: msd_workspace_words grows with the count over all %zu counts of the table\n", all.size());
}

// ---- the comparer, and its own test ----
static size_t compare_pairs(const std::vector<uint2>& want, const uint2* got, size_t got_total, size_t* first_bad = nullptr) {
    size_t bad = got_total != want.size() ? 1 : 0, first = ~(size_t)0;
    const size_t m = std::min(want.size(), got_total);
    for (size_t i = 0; i < m; ++i)
        if (want[i].x != got[i].x || want[i].y != got[i].y) {
            if (first == ~(size_t)0) first = i;
            ++bad;
        }
    if (first_bad) *first_bad = first;
    return bad;
}

static void self_test() {
    std::vector<uint2> want;
    for (uint32_t i = 0; i < 1000; ++i) want.push_back(make_uint2(0x3F000000u + 7u * i, 3u * i + 1u));
    if (compare_pairs(want, want.data(), want.size()) != 0) die(1, "MISMATCH self-test: the comparer reports an exact copy");
    std::vector<uint2> c = want;
    std::swap(c[500], c[501]);
    if (compare_pairs(want, c.data(), c.size()) == 0) die(1, "MISMATCH self-test: two neighbouring pairs swapped went unreported");
    c = want;
    c[777].y += 1u;
    if (compare_pairs(want, c.data(), c.size()) == 0) die(1, "MISMATCH self-test: an index off by one went unreported");
    if (compare_pairs(want, want.data(), want.size() - 1) == 0) die(1, "MISMATCH self-test: a total one short went unreported");
    printf("self-test: swapped pairs reported, index off by one reported, total one short reported\n");
}

// ---- keys ----
static uint32_t depth_key(std::mt19937& rng, bool dup) {
    const float f = dup ? 0.2f + 11.8f * (float)(rng() % 997u) / 997.0f : 0.2f + 11.8f * (float)(rng() >> 8) / 16777216.0f;
    uint32_t k;
    memcpy(&k, &f, 4);
    return k;
}
// float bits of depths in [0.2, 12); a quarter culled unless `dense`
static std::vector<uint32_t> make_keys(uint32_t n, bool dup, bool dense, uint32_t seed) {
    std::mt19937 rng(seed);
    std::vector<uint32_t> k(n);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t d = depth_key(rng, dup);
        k[i] = (!dense && (rng() & 3u) == 0u) ? kCulledKey : d;
    }
    return k;
}

// ---- one case on the host: keys, synthetic ballots, what derives from them, and the reference ----
enum Pattern { P_NONE, P_R3, P_R50, P_VISIBLE, P_DENSE, P_FIRST_TILE, P_LAST, P_EXACT };
struct Case {
    uint32_t n = 0;
    std::string name;
    std::vector<uint32_t> key;
    std::vector<u64h> ballots;             // 4 * ceil(n / 256) words (zero past n) + 4 of garbage
    std::vector<uint32_t> c256, v256;      // per 256-Gaussian projection workgroup: admitted, visible (+ 4 of garbage)
    std::vector<uint32_t> c1024, c4096;    // per k_admit_scatter<4> / <16> workgroup
    std::vector<uint2> want;
    uint32_t n_visible = 0;
    bool all_visible = false;              // the admitted set is every visible key: launch_admit without windows must produce it
    uint32_t pages = 0;                    // P_EXACT: pages of kCompactList the tile takes
};
static uint32_t compact_tile(uint32_t n) { return (n + 63u) / 64u < kCompactSmallWords ? 16384u : 65536u; }

static Case make_case(uint32_t n, bool dup, Pattern pat, uint32_t tile, uint32_t P, uint32_t seed) {
    Case c;
    c.n = n;
    c.key = make_keys(n, dup, pat == P_DENSE, seed);
    const uint32_t nb = (n + 255u) / 256u, tg = compact_tile(n);
    c.ballots.assign(4ull * nb + 4, 0ull);
    std::mt19937 rng(seed * 2654435761u + 17u);
    auto admit = [&](uint32_t i) {
        c.ballots[i >> 6] |= 1ull << (i & 63u);
        if (c.key[i] == kCulledKey) c.key[i] = depth_key(rng, dup);  // whatever is admitted is visible
    };
    char nm[64] = "";
    switch (pat) {
        case P_NONE: snprintf(nm, sizeof nm, "none"); break;
        case P_R3:
        case P_R50: {
            const uint32_t pc = pat == P_R3 ? 3u : 50u;
            for (uint32_t i = 0; i < n; ++i)
                if (c.key[i] != kCulledKey && rng() % 100u < pc) admit(i);
            snprintf(nm, sizeof nm, "%u%%", pc);
            break;
        }
        case P_VISIBLE:
        case P_DENSE:
            for (uint32_t i = 0; i < n; ++i)
                if (c.key[i] != kCulledKey) admit(i);
            c.all_visible = true;
            snprintf(nm, sizeof nm, pat == P_DENSE ? "dense" : "visible");
            break;
        case P_FIRST_TILE:
            for (uint32_t i = 0; i < std::min(n, tg); ++i)
                if (c.key[i] != kCulledKey) admit(i);
            snprintf(nm, sizeof nm, "first-tile");
            break;
        case P_LAST: admit(n - 1u); snprintf(nm, sizeof nm, "last-gaussian"); break;
        case P_EXACT: {
            const uint32_t lo = tile * tg, hi = (uint32_t)std::min<uint64_t>(n, (uint64_t)lo + tg), pop = hi - lo;
            uint32_t need = std::min(P, pop);
            c.pages = (need + kCompactList - 1u) / kCompactList;
            snprintf(nm, sizeof nm, "exactly-%u-in-tile-%u(%u-pages)", need, tile, c.pages);
            for (uint32_t i = lo; i < hi && need; ++i)  // selection sampling: exactly `need` of the tile's `pop`
                if (rng() % (hi - i) < need) {
                    admit(i);
                    --need;
                }
            break;
        }
    }
    c.name = nm;
    c.c256.assign(nb + 4, 0x01010101u);
    c.v256.assign(nb + 4, 0x02020202u);
    for (uint32_t b = 0; b < nb; ++b) c.c256[b] = c.v256[b] = 0;
    c.c1024.assign((n + 1023u) / 1024u, 0u);
    c.c4096.assign((n + 4095u) / 4096u, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        if (c.key[i] != kCulledKey) {
            ++c.v256[i >> 8];
            ++c.n_visible;
        }
        if ((c.ballots[i >> 6] >> (i & 63u)) & 1ull) {
            ++c.c256[i >> 8];
            ++c.c1024[i >> 10];
            ++c.c4096[i >> 12];
            c.want.push_back(make_uint2(c.key[i], i));
        }
    }
    for (int k = 0; k < 4; ++k) c.ballots[4ull * nb + k] = ~0ull;  // the padding: garbage
    return c;
}

// ---- device side ----
constexpr uint32_t kSentinel = 0xEEEEEEEEu;
constexpr size_t kPairSlack = 513;  // (the guard slot behind the last pair, and room for a kernel that took the ballots' padding for bits)
struct Ctx {
    hipStream_t s = nullptr;
    uint32_t cap = 0;
    uint32_t *key = nullptr, *c256 = nullptr, *v256 = nullptr, *off256 = nullptr, *cnt = nullptr, *cnt2 = nullptr, *scal = nullptr, *ws = nullptr;
    u64h *bal = nullptr, *bal2 = nullptr;
    uint2 *pairs = nullptr, *h_pairs = nullptr;
    size_t ws_words = 0;
    uint32_t seq = 0;
    uint32_t* d_total() const { return scal; }
    uint32_t* d_nvis() const { return scal + 1; }
    uint32_t* d_zero() const { return scal + 2; }     // d_skip pointing at 0
    uint32_t* d_nonzero() const { return scal + 3; }  // d_skip pointing at a non-zero word
};
static void ctx_free(Ctx& c) {
    for (void* p : {(void*)c.key, (void*)c.c256, (void*)c.v256, (void*)c.off256, (void*)c.cnt, (void*)c.cnt2, (void*)c.scal, (void*)c.ws, (void*)c.bal, (void*)c.bal2,
                    (void*)c.pairs})
        if (p) CK(hipFree(p));
    if (c.h_pairs) CK(hipHostFree(c.h_pairs));
    hipStream_t s = c.s;
    c = Ctx{};
    c.s = s;
}
static void ctx_workspace(Ctx& c, uint32_t n) {  // a fresh workspace for count n
    if (c.ws) CK(hipFree(c.ws));
    c.ws_words = msd_workspace_words(n);
    CK(hipMalloc(&c.ws, 4 * c.ws_words));
    CK(msd_workspace_init(c.s, c.ws, c.ws_words));
    CK(hipStreamSynchronize(c.s));
}
static void ctx_alloc(Ctx& c, uint32_t n) {
    if (!c.s) CK(hipStreamCreate(&c.s));
    ctx_free(c);
    c.cap = n;
    const size_t nb = ((size_t)n + 255) / 256, words = ((size_t)n + 63) / 64;
    CK(hipMalloc(&c.key, 4 * ((size_t)n + 1024)));
    CK(hipMemset(c.key, 0xFF, 4 * ((size_t)n + 1024)));
    CK(hipMalloc(&c.bal, 8 * (4 * nb + 4)));
    CK(hipMalloc(&c.bal2, 8 * (words + 4)));
    CK(hipMalloc(&c.c256, 4 * (nb + 4)));
    CK(hipMalloc(&c.v256, 4 * (nb + 4)));
    CK(hipMalloc(&c.off256, 4 * (nb + 4)));
    CK(hipMalloc(&c.cnt, 4 * (((size_t)n + 1023) / 1024 + 4)));
    CK(hipMalloc(&c.cnt2, 4 * (admit_blocks(n) + 4)));
    CK(hipMalloc(&c.scal, 16));
    const uint32_t sc[4] = {kSentinel, kSentinel, 0u, 7u};
    CK(hipMemcpy(c.scal, sc, 16, hipMemcpyHostToDevice));
    CK(hipMalloc(&c.pairs, 8 * ((size_t)n + kPairSlack)));
    CK(hipHostMalloc(&c.h_pairs, 8 * ((size_t)n + kPairSlack)));
    ctx_workspace(c, n);
}
static void upload(Ctx& c, const Case& k) {
    const size_t nb = ((size_t)k.n + 255) / 256;
    CK(hipMemcpy(c.key, k.key.data(), 4ull * k.n, hipMemcpyHostToDevice));
    CK(hipMemcpy(c.bal, k.ballots.data(), 8 * (4 * nb + 4), hipMemcpyHostToDevice));
    CK(hipMemcpy(c.c256, k.c256.data(), 4 * (nb + 4), hipMemcpyHostToDevice));
    CK(hipMemcpy(c.v256, k.v256.data(), 4 * (nb + 4), hipMemcpyHostToDevice));
}
static void arm(Ctx& c, uint32_t n) {  // results and pairs to the sentinel
    CK(hipMemsetAsync(c.pairs, 0xEE, 8 * ((size_t)n + kPairSlack), c.s));
    CK(hipMemsetAsync(c.scal, 0xEE, 8, c.s));
}
// what a path left behind against the reference.  has_total: the path writes *d_total; nvis >= 0: it writes *d_n_visible;
// skipped: d_skip pointed at 0 — total 0, pairs untouched
static void verify(Ctx& c, const Case& k, const std::vector<uint2>& want, const char* path, bool has_total, long long nvis, bool skipped) {
    CK(hipStreamSynchronize(c.s));
    CK(hipGetLastError());
    uint32_t sc[2];
    CK(hipMemcpy(sc, c.scal, 8, hipMemcpyDeviceToHost));
    ++g_cases;
    if (skipped) {
        const size_t look = std::min<size_t>((size_t)k.n + kPairSlack, 65536);
        CK(hipMemcpy(c.h_pairs, c.pairs, 8 * look, hipMemcpyDeviceToHost));
        size_t touched = 0;
        for (size_t i = 0; i < look; ++i) touched += c.h_pairs[i].x != kSentinel || c.h_pairs[i].y != kSentinel;
        if (sc[0] != 0u || touched) die(1, "MISMATCH n %u %s path %s: d_skip -> 0 must leave total 0 and the pairs untouched: total %u, %zu pairs written", k.n, k.name.c_str(), path, sc[0], touched);
        printf("n %u %s path %s admitted 0 (skipped) ok\n", k.n, k.name.c_str(), path);
        return;
    }
    const size_t total = has_total ? sc[0] : want.size();
    if (total != want.size()) die(1, "MISMATCH n %u %s path %s: total %zu, want %zu", k.n, k.name.c_str(), path, total, want.size());
    CK(hipMemcpy(c.h_pairs, c.pairs, 8 * (total + 1), hipMemcpyDeviceToHost));
    size_t first = 0;
    const size_t bad = compare_pairs(want, c.h_pairs, total, &first);
    if (bad)
        die(1, "MISMATCH n %u %s path %s: %zu of %zu pairs differ, first at %zu: got (%08x, %u) want (%08x, %u)", k.n, k.name.c_str(), path, bad, total, first,
            c.h_pairs[first].x, c.h_pairs[first].y, want[first].x, want[first].y);
    if (c.h_pairs[total].x != kSentinel || c.h_pairs[total].y != kSentinel) die(1, "MISMATCH n %u %s path %s: a pair was written behind the last one (slot %zu)", k.n, k.name.c_str(), path, total);
    if (nvis >= 0 && sc[1] != (uint32_t)nvis) die(1, "MISMATCH n %u %s path %s: n_visible %u, want %lld", k.n, k.name.c_str(), path, sc[1], nvis);
    printf("n %u %s path %s admitted %zu%s ok\n", k.n, k.name.c_str(), path, total, nvis >= 0 ? " n_visible ok" : "");
}

// paths a - d over one case.  full: every combination of path a's switches (small counts); otherwise every value of every switch once
static void run_paths(Ctx& c, const Case& k, bool full) {
    upload(c, k);
    const uint32_t n = k.n;
    char path[96];
    // a. launch_admit_compact
    for (int bv = 0; bv < 2; ++bv)
        for (int hist = 0; hist < 2; ++hist)
            for (int skip = 0; skip < 3; ++skip) {
                if (!full && !((bv == 1 && hist == 1 && skip == 0) || (bv == 0 && hist == 0 && skip == 1) || (bv == 1 && hist == 0 && skip == 2) || (bv == 0 && hist == 1 && skip == 0)))
                    continue;
                arm(c, n);
                const uint32_t* d_skip = skip == 0 ? nullptr : skip == 1 ? c.d_nonzero() : c.d_zero();
                CK(launch_admit_compact(c.s, c.key, n, c.bal, c.d_total(), c.pairs, bv ? c.v256 : nullptr, bv ? c.d_nvis() : nullptr, c.ws, c.seq++, d_skip, hist != 0));
                snprintf(path, sizeof path, "a:compact<%u>%s%s%s", compact_tile(n) == 16384u ? 1u : 4u, bv ? "+visible" : "", hist ? "+histogram" : "",
                         skip == 0 ? "" : skip == 1 ? "+skip->7" : "+skip->0");
                verify(c, k, k.want, path, true, bv && skip != 2 ? (long long)k.n_visible : -1, skip == 2);
            }
    // b. launch_admit_from_project
    for (int sparse = 1; sparse >= 0; --sparse) {
        arm(c, n);
        CK(launch_admit_from_project(c.s, c.key, n, c.bal, c.c256, c.off256, c.d_total(), c.pairs, sparse != 0, c.v256, c.d_nvis()));
        verify(c, k, k.want, sparse ? "b:scan+scatter256" : "b:scan+scatter_dense", true, (long long)k.n_visible, false);
    }
    // c. launch_admit_scatter
    for (uint32_t rounds : {16u, 4u})
        for (int raw = 0; raw < 2; ++raw) {
            const std::vector<uint32_t>& counts = rounds == 16u ? k.c4096 : k.c1024;
            std::vector<uint32_t> up = counts;
            if (!raw) {  // offsets scanned on the host
                uint32_t run = 0;
                for (size_t i = 0; i < up.size(); ++i) {
                    up[i] = run;
                    run += counts[i];
                }
            }
            CK(hipMemcpy(c.cnt, up.data(), 4 * up.size(), hipMemcpyHostToDevice));
            arm(c, n);
            CK(launch_admit_scatter(c.s, c.key, n, c.bal, c.cnt, c.pairs, nullptr, raw ? c.d_total() : nullptr, rounds));
            snprintf(path, sizeof path, "c:scatter<%u>%s", rounds, raw ? "+raw-counts" : "+host-offsets");
            verify(c, k, k.want, path, raw != 0, -1, false);
        }
    // d. launch_admit without windows: k_admit_count makes the ballots from the keys — every visible key
    if (k.all_visible)
        for (int msd = 1; msd >= 0; --msd) {
            Records rec{};
            rec.key = c.key;
            arm(c, n);
            CK(launch_admit(c.s, rec, n, nullptr, 0u, nullptr, 0u, WindowPyramid{}, nullptr, c.bal2, c.cnt2, c.d_total(), c.pairs, msd ? c.ws : nullptr, c.seq++));
            verify(c, k, k.want, msd ? "d:count+compact" : "d:count+scatter<16>", true, -1, false);
        }
    else
        printf("n %u %s path d: not applicable (the admitted set is not every visible key)\n", n, k.name.c_str());
}

static std::vector<uint32_t> tiles_of(uint32_t n) {  // first, a middle and the last k_admit_compact tile
    const uint32_t tg = compact_tile(n), nt = (n + tg - 1u) / tg;
    std::vector<uint32_t> t{0u};
    if (nt > 2u) t.push_back(nt / 2u);
    if (nt > 1u) t.push_back(nt - 1u);
    return t;
}
static void all_patterns(Ctx& c, uint32_t n, bool full, std::initializer_list<uint32_t> sizes) {
    uint32_t seed = n * 31u + 5u;
    for (Pattern p : {P_NONE, P_R3, P_R50, P_VISIBLE, P_DENSE, P_FIRST_TILE, P_LAST}) run_paths(c, make_case(n, false, p, 0, 0, seed++), full);
    for (uint32_t P : sizes)
        for (uint32_t t : tiles_of(n)) run_paths(c, make_case(n, false, P_EXACT, t, P, seed++), full);
}

static void group_small(Ctx& c) {
    for (uint32_t n : kSmallCounts) {
        ctx_alloc(c, n);
        all_patterns(c, n, true, {8191u, 8192u, 8193u, 16384u});
    }
}
static void group_threshold(Ctx& c) {
    for (uint32_t n : kThresholdCounts) {
        ctx_alloc(c, n);
        all_patterns(c, n, false, {8191u, 8192u, 8193u, 16384u});
    }
}
static void group_superscan(Ctx& c) {
    for (uint32_t n : kSuperCounts) {
        ctx_alloc(c, n);
        uint32_t seed = n * 31u + 5u;
        for (Pattern p : {P_R3, P_DENSE, P_FIRST_TILE, P_LAST}) run_paths(c, make_case(n, false, p, 0, 0, seed++), false);
    }
}
static void group_pages(Ctx& c) {
    for (uint32_t n : kPageCounts) {
        ctx_alloc(c, n);
        if (n == 1000000u) all_patterns(c, n, false, {8191u, 8192u, 8193u, 16384u});
        else if (compact_tile(n) == 16384u) all_patterns(c, n, false, {8191u, 8192u, 8193u, 16384u});          // 1, 1, 2, 2 pages
        else all_patterns(c, n, false, {8192u, 8193u, 16384u, 65536u});                                          // 1, 2, 2, 8 pages
    }
}

// ---- the hand-over to the bucket sort: the fine histogram and key range k_admit_compact counted, then hist_done = true ----
static void group_handover(Ctx& c) {
    printf("returning LDS adds lane-ordered on this device: %d\n", (int)radix_lane_ordered_adds());
    struct H { uint32_t n; Pattern p; };
    const H cases[] = {{1000000u, P_NONE}, {1000000u, P_R50}, {4194240u, P_R50}, {4194241u, P_R50}, {10000000u, P_R3}};
    for (const H& h : cases)
        for (int dup = 0; dup < 2; ++dup) {
            if (c.cap != h.n) ctx_alloc(c, h.n);
            ctx_workspace(c, h.n);  // freshly initialised: no key range known
            const uint32_t n = h.n;
            Case k = make_case(n, dup != 0, h.p, 0, 0, n * 7u + (uint32_t)dup);
            k.name += dup ? "/dup-keys" : "/depth-keys";
            upload(c, k);
            uint2 *pa, *pb;
            uint32_t *ko, *vo, *rws;
            const size_t rwords = radix_workspace_words(n);
            CK(hipMalloc(&pa, 8ull * n + 8));
            CK(hipMalloc(&pb, 8ull * n + 8));
            CK(hipMalloc(&ko, 4ull * n + 4));
            CK(hipMalloc(&vo, 4ull * n + 4));
            CK(hipMalloc(&rws, 4 * rwords));
            CK(hipMemset(rws, 0, 4 * rwords));
            std::vector<uint2> sorted = k.want;
            std::stable_sort(sorted.begin(), sorted.end(), [](const uint2& a, const uint2& b) { return a.x < b.x; });
            uint32_t mn = 0xFFFFFFFFu, mx = 0u;
            for (const uint2& p : k.want) {
                mn = std::min(mn, p.x);
                mx = std::max(mx, p.x);
            }
            std::vector<uint32_t> head(kMsdCells + 4), ks(k.want.size()), vs(k.want.size());
            for (int round = 0; round < 2; ++round) {  // round 0: no key range known yet; round 1: the range of the sort before
                const uint32_t seq = c.seq++;
                arm(c, n);
                CK(launch_admit_compact(c.s, c.key, n, c.bal, c.d_total(), c.pairs, c.v256, c.d_nvis(), c.ws, seq, nullptr, true));
                verify(c, k, k.want, round ? "a:compact+histogram (key range known)" : "a:compact+histogram (fresh workspace)", true, (long long)k.n_visible, false);
                CK(hipMemcpy(head.data(), c.ws, 4 * head.size(), hipMemcpyDeviceToHost));
                uint64_t sum = 0;
                for (uint32_t i = 0; i < kMsdFine; ++i) sum += head[i];
                if (sum != k.want.size()) die(1, "MISMATCH n %u %s hand-over: the fine histogram sums to %llu, admitted %zu", n, k.name.c_str(), (unsigned long long)sum, k.want.size());
                if (head[kMsdCells] != mn || head[kMsdCells + 1] != mx)
                    die(1, "MISMATCH n %u %s hand-over: key range {%08x, %08x}, want {%08x, %08x}", n, k.name.c_str(), head[kMsdCells], head[kMsdCells + 1], mn, mx);
                if (k.want.empty()) {
                    printf("n %u %s hand-over: nothing admitted, histogram empty, key range cells untouched ok\n", n, k.name.c_str());
                    break;
                }
                RadixBuffers rb{nullptr, nullptr, c.pairs, ko, vo, pa, pb, rws};
                CK(hipMemsetAsync(ko, 0xEE, 4ull * n, c.s));
                CK(launch_bucket_sort(c.s, rb, n, c.d_total(), false, c.ws, seq, true));
                CK(hipStreamSynchronize(c.s));
                CK(hipGetLastError());
                CK(hipMemcpy(ks.data(), ko, 4 * ks.size(), hipMemcpyDeviceToHost));
                CK(hipMemcpy(vs.data(), vo, 4 * vs.size(), hipMemcpyDeviceToHost));
                size_t bad = 0, first = 0;
                for (size_t i = sorted.size(); i-- > 0;)
                    if (sorted[i].x != ks[i] || sorted[i].y != vs[i]) {
                        ++bad;
                        first = i;
                    }
                ++g_cases;
                if (bad) die(1, "MISMATCH n %u %s hand-over: bucket sort (hist_done) differs from std::stable_sort in %zu of %zu places, first at %zu", n, k.name.c_str(), bad, sorted.size(), first);
                printf("n %u %s path a+launch_bucket_sort(hist_done) round %d admitted %zu: histogram sum ok, key range ok, order == std::stable_sort ok\n", n, k.name.c_str(), round,
                       sorted.size());
            }
            for (void* p : {(void*)pa, (void*)pb, (void*)ko, (void*)vo, (void*)rws}) CK(hipFree(p));
        }
}

// ---- one workspace, launches of different tilings ----
static void group_reuse(Ctx& c) {
    // LEGAL ONLY WITH msd_workspace_words() SIZING FOR THE FINER TILING AT EVERY COUNT: the workspace below is sized for 4 194 305 Gaussians (65 tiles
    // of 65 536), and the first launch — 4 194 240 Gaussians, 256 tiles of 16 384 — writes 256 tiles' status words into it.  Sized by the launch's
    // own tiling the workspace held 66 tiles' words and that launch wrote past its end (check_workspace_sizes() has refused that before this point).
    ctx_alloc(c, 4194305u);
    const Case dense = make_case(4194240u, false, P_DENSE, 0, 0, 101u);
    const Case sparse = make_case(4194305u, false, P_R3, 0, 0, 102u);
    const Case tiny = make_case(16385u, false, P_R50, 0, 0, 103u);
    struct Step { const Case* k; int skip; const char* what; };
    const Step steps[] = {{&dense, 0, "reuse 1/5 a:compact<1> 256 tiles"},
                          {&sparse, 0, "reuse 2/5 a:compact<4> 65 tiles"},
                          {&sparse, 1, "reuse 3/5 a:compact<4> skip->0 (no ticket taken)"},
                          {&tiny, 0, "reuse 4/5 a:compact<1> 2 tiles"},
                          {&dense, 0, "reuse 5/5 a:compact<1> 256 tiles again"}};
    for (const Step& st : steps) {
        upload(c, *st.k);
        arm(c, c.cap);
        CK(launch_admit_compact(c.s, c.key, st.k->n, c.bal, c.d_total(), c.pairs, c.v256, c.d_nvis(), c.ws, c.seq++, st.skip ? c.d_zero() : nullptr, true));
        verify(c, *st.k, st.k->want, st.what, true, st.skip ? -1 : (long long)st.k->n_visible, st.skip != 0);
    }
}

// ---- the window predicate ----
struct Grid {
    uint32_t tx, ty;
    bool rect8;  // rectangles from the four-byte plane (grids of at most 255 x 255 tiles), otherwise from the `a` records
};
static const Grid kGrids[] = {{120, 68, true}, {240, 135, true}, {63, 3, true}, {63, 3, false}, {300, 2, false}};
struct Scene {
    Grid g;
    uint32_t n = kWindowRecords, n_visible = 0;
    std::vector<uint32_t> key, rx, ry;  // rx = x0 | x1 << 16, ry = y0 | y1 << 16 (max exclusive)
    std::vector<uint8_t> gate5;         // a random 5 % of the tiles
    uint32_t hot_x, hot_y;              // the tile of gate5 nearest (tx / 3, ty / 2): a tenth of the rectangles cover it (the one-tile gate)
};
static uint32_t rnd_depth(std::mt19937& rng) { return depth_key(rng, false); }

static Scene make_scene(const Grid& g, uint32_t seed) {
    Scene s;
    s.g = g;
    {
        std::mt19937 grng(seed + 3000u);
        s.gate5.assign((size_t)g.tx * g.ty, 0);
        for (auto& b : s.gate5) b = grng() % 20u == 0u;
        s.hot_x = g.tx / 3u;
        s.hot_y = g.ty / 2u;
        uint32_t best = ~0u;
        for (uint32_t y = 0; y < g.ty; ++y)
            for (uint32_t x = 0; x < g.tx; ++x) {
                const uint32_t dx = x > g.tx / 3u ? x - g.tx / 3u : g.tx / 3u - x, dy = y > g.ty / 2u ? y - g.ty / 2u : g.ty / 2u - y;
                if (s.gate5[(size_t)y * g.tx + x] && dx + dy < best) {
                    best = dx + dy;
                    s.hot_x = x;
                    s.hot_y = y;
                }
            }
        s.gate5[(size_t)s.hot_y * g.tx + s.hot_x] = 1;  // (a grid without one gated tile: none here)
    }
    s.key = make_keys(s.n, false, false, seed);
    s.rx.assign(s.n, 0u);
    s.ry.assign(s.n, 0u);
    std::mt19937 rng(seed ^ 0x9E3779B9u);
    for (uint32_t i = 0; i < s.n; ++i) {
        if (s.key[i] == kCulledKey) continue;  // (a culled record's rectangle: 0, as the projection leaves it)
        ++s.n_visible;
        uint32_t w = 1, h = 1;
        bool right = false, bottom = false;
        const uint32_t cls = rng() % 100u;
        if (cls < 26u) { w = 1; h = 1; }
        else if (cls < 32u) { w = 1 + (rng() & 1u); h = 3 - w; }            // 1x2, 2x1
        else if (cls < 42u) { w = 2; h = 2; }
        else if (cls < 50u) { w = 3; h = 3; }
        else if (cls < 55u) { w = (rng() & 1u) ? 4 : 8; h = 32 / w; }        // 32 tiles: the largest the lane walks alone
        else if (cls < 59u) { w = 33; h = 1; if (rng() & 1u) std::swap(w, h); }  // 33: the smallest the wave scans
        else if (cls < 64u) { w = 6; h = 6; }
        else if (cls < 65u) { w = g.tx; h = g.ty; }                          // the whole grid
        else if (cls < 67u) { w = g.tx; h = 1; }                             // a whole row
        else if (cls < 69u) { w = 1; h = g.ty; }                             // a whole column
        else if (cls < 83u) {                                                // extents of exactly 2^l and 2^l + 1 tiles
            w = (1u << (rng() % 9u)) + (rng() & 1u);
            h = (1u << (rng() % 9u)) + (rng() & 1u);
        } else {                                                             // touching the right / bottom edge
            w = 1 + rng() % 5u;
            h = 1 + rng() % 5u;
            right = (rng() % 3u) != 0u;
            bottom = !right || (rng() & 1u);
        }
        w = std::min(w, g.tx);
        h = std::min(h, g.ty);
        uint32_t x0 = rng() % (g.tx - w + 1u), y0 = rng() % (g.ty - h + 1u);
        if (right) x0 = g.tx - w;
        if (bottom) y0 = g.ty - h;
        if (rng() % 10u == 0u) {  // over the hot tile
            x0 = std::min<uint32_t>(s.hot_x > w - 1u ? s.hot_x - (uint32_t)(rng() % w) : 0u, g.tx - w);
            y0 = std::min<uint32_t>(s.hot_y > h - 1u ? s.hot_y - (uint32_t)(rng() % h) : 0u, g.ty - h);
        }
        s.rx[i] = x0 | (x0 + w) << 16;
        s.ry[i] = y0 | (y0 + h) << 16;
    }
    return s;
}
// style 0: a speculated frame's windows — random [lo, hi), some empty, some from 0, some to kKeyAll; style 1: a repair round's — [lo, kKeyAll) on
// three tiles in ten, nothing on the rest.  In both a block of whole 8 x 8-grid cells has no window at all (zero bits in the cell word).
static std::vector<uint2> make_windows(const Scene& s, int style, uint32_t seed) {
    const Grid& g = s.g;
    const WindowPyramid lay = window_pyramid_layout(g.tx, g.ty, nullptr);
    const uint32_t cy_half = (((g.ty - 1u) >> lay.cell_sy) + 1u) / 2u;
    std::mt19937 rng(seed);
    std::vector<uint2> w((size_t)g.tx * g.ty);
    for (uint32_t y = 0; y < g.ty; ++y)
        for (uint32_t x = 0; x < g.tx; ++x) {
            uint32_t a = rnd_depth(rng), b = rnd_depth(rng);
            if (a > b) std::swap(a, b);
            const uint32_t r = rng() % 100u;
            uint2 v;
            if ((x >> lay.cell_sx) >= 4u && (y >> lay.cell_sy) >= cy_half) v = make_uint2(0u, 0u);
            else if (style == 1) v = r < 30u ? make_uint2(a, kKeyAll) : make_uint2(0u, 0u);
            else if (r < 6u) v = make_uint2(a, a);          // empty
            else if (r < 12u) v = make_uint2(b, a);         // empty: ends before it starts
            else if (r < 32u) v = make_uint2(0u, b);
            else if (r < 36u) v = make_uint2(a, kKeyAll);
            else v = make_uint2(a, b + 1u);
            if (x == s.hot_x && y == s.hot_y) v = make_uint2(0u, kKeyAll);
            w[(size_t)y * g.tx + x] = v;
        }
    return w;
}
static bool host_exact(const Scene& s, const std::vector<uint2>& win, uint32_t i) {
    const uint32_t k = s.key[i], x0 = s.rx[i] & 0xFFFFu, x1 = s.rx[i] >> 16, y0 = s.ry[i] & 0xFFFFu, y1 = s.ry[i] >> 16;
    for (uint32_t y = y0; y < y1; ++y)
        for (uint32_t x = x0; x < x1; ++x) {
            const uint2 w = win[(size_t)y * s.g.tx + x];
            if (k >= w.x && k < w.y) return true;
        }
    return false;
}
static bool host_gated(const Scene& s, const std::vector<uint8_t>& gate, uint32_t i) {
    const uint32_t x0 = s.rx[i] & 0xFFFFu, x1 = s.rx[i] >> 16, y0 = s.ry[i] & 0xFFFFu, y1 = s.ry[i] >> 16;
    for (uint32_t y = y0; y < y1; ++y)
        for (uint32_t x = x0; x < x1; ++x)
            if (gate[(size_t)y * s.g.tx + x]) return true;
    return false;
}
// the host's pyramid: level 0 from the windows, level l the 2 x 2 max (min) of level l - 1
struct HostPyramid {
    WindowPyramid lay;
    std::vector<uint32_t> data, min_ends;
    u64h cells = 0;
};
static HostPyramid host_pyramid(const Scene& s, const std::vector<uint2>& win, bool min_of_starts) {
    HostPyramid h;
    h.lay = window_pyramid_layout(s.g.tx, s.g.ty, nullptr);
    h.lay.min_of_starts = min_of_starts ? 1u : 0u;
    const WindowPyramid& p = h.lay;
    h.data.assign(p.off[p.levels - 1] + p.wx[p.levels - 1] * p.wy[p.levels - 1], 0u);
    h.min_ends = h.data;
    for (uint32_t i = 0; i < p.wx[0] * p.wy[0]; ++i) {
        const uint2 w = win[i];
        h.data[i] = min_of_starts ? (w.y > w.x ? w.x : 0xFFFFFFFFu) : w.y;
        h.min_ends[i] = w.x == 0u ? w.y : 0u;
        if (w.y > w.x) h.cells |= 1ull << ((((i / p.wx[0]) >> p.cell_sy) << 3) | ((i % p.wx[0]) >> p.cell_sx));
    }
    for (uint32_t l = 1; l < p.levels; ++l)
        for (uint32_t y = 0; y < p.wy[l]; ++y)
            for (uint32_t x = 0; x < p.wx[l]; ++x) {
                uint32_t v = min_of_starts ? 0xFFFFFFFFu : 0u, m = 0xFFFFFFFFu;
                for (uint32_t dy = 0; dy < 2; ++dy)
                    for (uint32_t dx = 0; dx < 2; ++dx) {
                        const uint32_t cx = 2 * x + dx, cy = 2 * y + dy;
                        if (cx >= p.wx[l - 1] || cy >= p.wy[l - 1]) continue;
                        const size_t j = p.off[l - 1] + (size_t)cy * p.wx[l - 1] + cx;
                        v = min_of_starts ? std::min(v, h.data[j]) : std::max(v, h.data[j]);
                        m = std::min(m, h.min_ends[j]);
                    }
                h.data[p.off[l] + (size_t)y * p.wx[l] + x] = v;
                h.min_ends[p.off[l] + (size_t)y * p.wx[l] + x] = m;
            }
    return h;
}
// the host's own conservative bound: the level whose cells are at least as wide as the rectangle, every cell of it the rectangle touches
static bool host_bound(const Scene& s, const HostPyramid& h, uint32_t i) {
    const WindowPyramid& p = h.lay;
    const uint32_t k = s.key[i], x0 = s.rx[i] & 0xFFFFu, xb = (s.rx[i] >> 16) - 1u, y0 = s.ry[i] & 0xFFFFu, yb = (s.ry[i] >> 16) - 1u;
    if (p.min_of_starts) {
        bool any = false;
        for (uint32_t cy = y0 >> p.cell_sy; cy <= (yb >> p.cell_sy); ++cy)
            for (uint32_t cx = x0 >> p.cell_sx; cx <= (xb >> p.cell_sx); ++cx) any |= (h.cells >> (cy * 8u + cx)) & 1ull;
        if (!any) return false;
    }
    uint32_t l = 0;
    while ((1u << l) < std::max(xb - x0, yb - y0) + 1u) ++l;
    if (l >= p.levels) return true;
    bool adm = false;
    for (uint32_t cy = y0 >> l; cy <= (yb >> l); ++cy)
        for (uint32_t cx = x0 >> l; cx <= (xb >> l); ++cx) {
            const uint32_t v = h.data[p.off[l] + (size_t)cy * p.wx[l] + cx];
            adm |= p.min_of_starts ? k >= v : k < v;
        }
    return adm;
}

struct WinDev {
    float4* a = nullptr;
    uint32_t *rect8 = nullptr, *gate = nullptr, *pyr = nullptr, *pyr_min = nullptr;
    uint2* win = nullptr;
};
static void upload_scene(Ctx& c, WinDev& d, const Scene& s) {
    CK(hipMemcpy(c.key, s.key.data(), 4ull * s.n, hipMemcpyHostToDevice));
    for (void* p : {(void*)d.a, (void*)d.rect8, (void*)d.gate, (void*)d.pyr, (void*)d.pyr_min, (void*)d.win})
        if (p) CK(hipFree(p));
    d = WinDev{};
    if (s.g.rect8) {
        std::vector<uint32_t> r(s.n);
        for (uint32_t i = 0; i < s.n; ++i) r[i] = (s.rx[i] & 0xFFu) | (s.ry[i] & 0xFFu) << 8 | (s.rx[i] >> 16) << 16 | (s.ry[i] >> 16) << 24;
        CK(hipMalloc(&d.rect8, 4ull * s.n));
        CK(hipMemcpy(d.rect8, r.data(), 4ull * s.n, hipMemcpyHostToDevice));
    } else {
        std::vector<float4> a(s.n);
        for (uint32_t i = 0; i < s.n; ++i) {
            a[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            memcpy(&a[i].z, &s.rx[i], 4);
            memcpy(&a[i].w, &s.ry[i], 4);
        }
        CK(hipMalloc(&d.a, 16ull * s.n));
        CK(hipMemcpy(d.a, a.data(), 16ull * s.n, hipMemcpyHostToDevice));
    }
    const size_t nt = (size_t)s.g.tx * s.g.ty, pw = window_pyramid_words(s.g.tx, s.g.ty);
    CK(hipMalloc(&d.win, 8 * nt));
    CK(hipMalloc(&d.gate, 4 * (size_t)((s.g.tx + 31u) / 32u) * s.g.ty));
    CK(hipMalloc(&d.pyr, 4 * pw));
    CK(hipMalloc(&d.pyr_min, 4 * pw));
}
static Case window_case(const Scene& s, const char* name) {  // a Case shell for verify(): n, name
    Case k;
    k.n = s.n;
    k.name = name;
    return k;
}
static void guard_share(const char* name, size_t part, size_t whole, double lo, double hi, const char* what) {
    const double f = whole ? (double)part / (double)whole : 0.0;
    if (f < lo || f > hi) die(1, "MISMATCH %s: an empty test: %s is %.1f %% of the visible records (wanted %.0f - %.0f %%)", name, what, 100.0 * f, 100.0 * lo, 100.0 * hi);
}

// e. exact windows, with and without a gate
struct WindowCase {
    uint32_t grid;
    int style, gate;
    Case k;                      // name, want
    std::vector<uint32_t> bits;  // the gate bitmap, row_words words per tile row
};
static void group_windows(Ctx& c) {
    // every reference first, and the guards against an empty test: on the host, before any launch
    std::vector<Scene> scenes;
    std::vector<std::vector<uint2>> wins;
    std::vector<WindowCase> cases;
    for (uint32_t gi = 0; gi < sizeof kGrids / sizeof kGrids[0]; ++gi) {
        const Grid& g = kGrids[gi];
        scenes.push_back(make_scene(g, 4001u + 13u * gi));
        const Scene& s = scenes.back();
        const uint32_t row_words = (g.tx + 31u) / 32u;
        for (int style = 0; style < 2; ++style) {
            wins.push_back(make_windows(s, style, 9001u + 7u * gi + (uint32_t)style));
            const std::vector<uint2>& win = wins.back();
            for (int gk = 0; gk < 4; ++gk) {  // no gate; one tile; one row; a random 5 %
                std::vector<uint8_t> gate((size_t)g.tx * g.ty, 0);
                if (gk == 1) gate[(size_t)s.hot_y * g.tx + s.hot_x] = 1;
                if (gk == 2)
                    for (uint32_t x = 0; x < g.tx; ++x) gate[(size_t)s.hot_y * g.tx + x] = 1;
                if (gk == 3) gate = s.gate5;
                WindowCase w;
                w.grid = gi;
                w.style = style;
                w.gate = gk;
                w.bits.assign((size_t)row_words * g.ty, 0u);
                for (uint32_t y = 0; y < g.ty; ++y)
                    for (uint32_t x = 0; x < g.tx; ++x)
                        if (gate[(size_t)y * g.tx + x]) w.bits[(size_t)y * row_words + (x >> 5)] |= 1u << (x & 31u);
                char name[128];
                snprintf(name, sizeof name, "grid %ux%u %s %s windows, %s", g.tx, g.ty, g.rect8 ? "rect8" : "a-plane", style ? "repair" : "speculation",
                         gk == 0 ? "no gate" : gk == 1 ? "gate: one tile" : gk == 2 ? "gate: one row" : "gate: random 5 %");
                w.k = window_case(s, name);
                for (uint32_t i = 0; i < s.n; ++i)
                    if (s.key[i] != kCulledKey && (gk == 0 || host_gated(s, gate, i)) && host_exact(s, win, i)) w.k.want.push_back(make_uint2(s.key[i], i));
                guard_share(name, w.k.want.size(), s.n_visible, 0.05, 0.95, "the exact admitted set");
                printf("reference: %s: %zu of %u visible records admitted\n", name, w.k.want.size(), s.n_visible);
                cases.push_back(std::move(w));
            }
        }
    }
    ctx_alloc(c, kWindowRecords);
    WinDev d;
    uint32_t on_device = ~0u;
    for (const WindowCase& w : cases) {
        const Scene& s = scenes[w.grid];
        if (on_device != w.grid) upload_scene(c, d, s);
        on_device = w.grid;
        const std::vector<uint2>& win = wins[2 * w.grid + w.style];
        CK(hipMemcpy(d.win, win.data(), 8 * win.size(), hipMemcpyHostToDevice));
        CK(hipMemcpy(d.gate, w.bits.data(), 4 * w.bits.size(), hipMemcpyHostToDevice));
        Records rec{};
        rec.key = c.key;
        rec.a = d.a;
        rec.rect8 = d.rect8;
        const bool msd = (w.gate & 1) == 0;
        arm(c, s.n);
        CK(launch_admit(c.s, rec, s.n, d.win, s.g.tx, w.gate ? d.gate : nullptr, (s.g.tx + 31u) / 32u, WindowPyramid{}, nullptr, c.bal2, c.cnt2, c.d_total(), c.pairs,
                        msd ? c.ws : nullptr, c.seq++));
        verify(c, w.k, w.k.want, msd ? "e:exact-windows+compact" : "e:exact-windows+scatter<16>", true, -1, false);
    }
}

// f. the pyramid launch_window_pyramid builds from the same windows: conservative, never refusing what an exact window admits
struct PyramidCase {
    uint32_t grid;
    int style, mos;  // mos 0: the largest end (+ the min-ends pyramid); 1: the smallest start, with the cell word
    std::string name;
    HostPyramid h;
    size_t n_exact, n_bound;
};
static void group_pyramid(Ctx& c) {
    // every reference first, and the guards against an empty test: on the host, before any launch
    std::vector<Scene> scenes;
    std::vector<std::vector<uint2>> wins;
    std::vector<std::vector<uint8_t>> exacts;
    std::vector<PyramidCase> cases;
    for (uint32_t gi = 0; gi < sizeof kGrids / sizeof kGrids[0]; ++gi) {
        const Grid& g = kGrids[gi];
        scenes.push_back(make_scene(g, 4001u + 13u * gi));
        const Scene& s = scenes.back();
        for (int style = 0; style < 2; ++style) {
            wins.push_back(make_windows(s, style, 9001u + 7u * gi + (uint32_t)style));
            const std::vector<uint2>& win = wins.back();
            std::vector<uint8_t> exact(s.n, 0);
            size_t n_exact = 0;
            for (uint32_t i = 0; i < s.n; ++i)
                if (s.key[i] != kCulledKey && host_exact(s, win, i)) {
                    exact[i] = 1;
                    ++n_exact;
                }
            exacts.push_back(std::move(exact));
            for (int mos = 0; mos < 2; ++mos) {
                char name[160];
                snprintf(name, sizeof name, "grid %ux%u %s %s windows, pyramid of %s", g.tx, g.ty, g.rect8 ? "rect8" : "a-plane", style ? "repair" : "speculation",
                         mos ? "smallest starts + cell word" : "largest ends + min-ends");
                PyramidCase p{gi, style, mos, name, host_pyramid(s, win, mos != 0), n_exact, 0};
                for (uint32_t i = 0; i < s.n; ++i) p.n_bound += s.key[i] != kCulledKey && host_bound(s, p.h, i);
                guard_share(name, n_exact, s.n_visible, 0.05, 0.95, "the exact admitted set");
                guard_share(name, s.n_visible - p.n_bound, s.n_visible, 0.05, 1.0, "what the host's conservative bound refuses");
                if (mos && p.h.cells == ~0ull) die(1, "MISMATCH %s: an empty test: the cell word has no zero bit", name);
                printf("reference: %s: %zu of %u visible records admitted by an exact window, %zu by the host's conservative bound\n", name, n_exact, s.n_visible, p.n_bound);
                cases.push_back(std::move(p));
            }
        }
    }
    ctx_alloc(c, kWindowRecords);
    WinDev d;
    uint32_t on_device = ~0u;
    for (const PyramidCase& pc : cases) {
        const Scene& s = scenes[pc.grid];
        const Grid& g = s.g;
        const char* name = pc.name.c_str();
        const HostPyramid& h = pc.h;
        const int mos = pc.mos;
        if (on_device != pc.grid) upload_scene(c, d, s);
        on_device = pc.grid;
        const std::vector<uint2>& win = wins[2 * pc.grid + pc.style];
        const std::vector<uint8_t>& exact = exacts[2 * pc.grid + pc.style];
        CK(hipMemcpy(d.win, win.data(), 8 * win.size(), hipMemcpyHostToDevice));
        Records rec{};
        rec.key = c.key;
        rec.a = d.a;
        rec.rect8 = d.rect8;
        const size_t pw = window_pyramid_words(g.tx, g.ty);
        CK(hipMemsetAsync(d.pyr, 0xEE, 4 * pw, c.s));
        CK(hipMemsetAsync(d.pyr_min, 0xEE, 4 * pw, c.s));
        CK(launch_window_pyramid(c.s, d.win, g.tx, g.ty, d.pyr, mos != 0, nullptr, mos ? nullptr : d.pyr_min));
        CK(hipStreamSynchronize(c.s));
        CK(hipGetLastError());
        std::vector<uint32_t> got(pw), got_min(pw);
        CK(hipMemcpy(got.data(), d.pyr, 4 * pw, hipMemcpyDeviceToHost));
        CK(hipMemcpy(got_min.data(), d.pyr_min, 4 * pw, hipMemcpyDeviceToHost));
        for (uint32_t l = 0; l < h.lay.levels; ++l)
            for (uint32_t j = 0; j < h.lay.wx[l] * h.lay.wy[l]; ++j) {
                const size_t q = h.lay.off[l] + j;
                if (got[q] != h.data[q]) die(1, "MISMATCH %s: pyramid level %u cell %u: %08x, host reduction %08x", name, l, j, got[q], h.data[q]);
                if (!mos && got_min[q] != h.min_ends[q]) die(1, "MISMATCH %s: min-ends level %u cell %u: %08x, host reduction %08x", name, l, j, got_min[q], h.min_ends[q]);
            }
        if (mos) {
            u64h cells;
            memcpy(&cells, &got[h.lay.cells_off], 8);
            if (cells != h.cells) die(1, "MISMATCH %s: cell word %016llx, host %016llx", name, cells, h.cells);
        }
        WindowPyramid p = window_pyramid_layout(g.tx, g.ty, d.pyr);
        p.min_of_starts = mos ? 1u : 0u;
        arm(c, s.n);
        CK(launch_admit(c.s, rec, s.n, nullptr, g.tx, nullptr, 0u, p, nullptr, c.bal2, c.cnt2, c.d_total(), c.pairs, mos ? c.ws : nullptr, c.seq++));
        CK(hipStreamSynchronize(c.s));
        CK(hipGetLastError());
        uint32_t total = 0;
        CK(hipMemcpy(&total, c.d_total(), 4, hipMemcpyDeviceToHost));
        ++g_cases;
        if (total > s.n_visible) die(1, "MISMATCH %s: %u admitted of %u visible", name, total, s.n_visible);
        CK(hipMemcpy(c.h_pairs, c.pairs, 8 * ((size_t)total + 1), hipMemcpyDeviceToHost));
        std::vector<uint8_t> seen(s.n, 0);
        long long last = -1;
        size_t in_bound = 0;
        for (uint32_t q = 0; q < total; ++q) {
            const uint2 pr = c.h_pairs[q];
            if (pr.y >= s.n || (long long)pr.y <= last) die(1, "MISMATCH %s: pair %u holds index %u behind index %lld: not in ascending index order", name, q, pr.y, last);
            last = pr.y;
            if (s.key[pr.y] == kCulledKey) die(1, "MISMATCH %s: record %u is culled and was admitted", name, pr.y);
            if (pr.x != s.key[pr.y]) die(1, "MISMATCH %s: pair %u carries key %08x, record %u has %08x", name, q, pr.x, pr.y, s.key[pr.y]);
            seen[pr.y] = 1;
            in_bound += host_bound(s, h, pr.y);
        }
        if (c.h_pairs[total].x != kSentinel) die(1, "MISMATCH %s: a pair was written behind the last one", name);
        for (uint32_t i = 0; i < s.n; ++i)
            if (exact[i] && !seen[i])
                die(1, "MISMATCH %s: record %u (key %08x, rect x %u..%u y %u..%u) is admitted by an exact window and refused by the pyramid", name, i, s.key[i],
                    s.rx[i] & 0xFFFFu, s.rx[i] >> 16, s.ry[i] & 0xFFFFu, s.ry[i] >> 16);
        printf("n %u %s path f:pyramid-admission admitted %u, every one of the %zu an exact window admits among them, no culled key; levels == host reduction ok; "
               "beyond the exact set: %zu (host bound admits %zu, %zu of the device's inside it)\n",
               s.n, name, total, pc.n_exact, (size_t)total - pc.n_exact, pc.n_bound, in_bound);
    }
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    g_group = argc > 1 ? argv[1] : "";
    struct G { const char* name; void (*run)(Ctx&); };
    const G groups[] = {{"small", group_small},       {"threshold", group_threshold}, {"superscan", group_superscan}, {"pages", group_pages},
                        {"handover", group_handover}, {"reuse", group_reuse},         {"windows", group_windows},     {"pyramid", group_pyramid}};
    const G* g = nullptr;
    for (const G& x : groups)
        if (!strcmp(x.name, g_group)) g = &x;
    if (!g) {
        fprintf(stderr, "usage: check_admit small|threshold|superscan|pages|handover|reuse|windows|pyramid\n");
        return 64;
    }
    // on the host, before any launch
    check_workspace_sizes();
    self_test();
    Ctx c;
    g->run(c);
    CK(hipDeviceSynchronize());
    printf("check_admit %s: %zu cases, 0 mismatches\n", g_group, g_cases);
    return 0;
}
