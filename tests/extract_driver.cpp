// extract_driver.cpp — csrc/extract_math.h (the keep words and destination indices of gsx_model_extract) played on the host, for
// tests/test_extract_cpu.py: a stand-alone program the test builds with the address and undefined-behaviour sanitizers.
// stdin:  "n <N>", "filter <GSX_BOUNDS_* bits>", "invert <0|1>", then the planes that exist, each on one line:
//         "mask <ceil(N/32) hex words>", "sel <hex words>", "edited <hex words>" with "flags <N stored edit flags>".
// stdout: "count <kept>", then "kept <source index of dst 0> <of dst 1> ...": the new model's Gaussians in dst order.
// Or stdin "layout <N of source 0> <N of source 1> ...": stdout "size <workspace bytes>", then per source "source<s> <byte offset
// of its bases> <of its partials> <of its keep words>" (extract_ws_layout; the totals lie at 8 s).
// The three steps are the kernels': a keep word per 32 Gaussians, a popcount partial per kExtractGroup, their exclusive scan, and
// dst index = group base + ranks of the group's preceding words + rank in the word.  Every dst index must be written exactly once.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "extract_math.h"

static std::vector<uint32_t> numbers(const char* s, int base) {
    std::vector<uint32_t> v;
    char* end = nullptr;
    for (;;) {
        const unsigned long x = strtoul(s, &end, base);
        if (end == s) break;
        v.push_back((uint32_t)x);
        s = end;
    }
    return v;
}

// the workspace of the kept-set pass over sources of these sizes: the total size, then every source's three byte offsets
static int layout(const char* sizes) {
    std::vector<uint64_t> n;
    char* end = nullptr;
    for (const char* s = sizes;; s = end) {
        const unsigned long long x = strtoull(s, &end, 10);
        if (end == s) break;
        n.push_back(x);
    }
    std::vector<gsx::ExtractRegion> r(n.size());
    printf("size %zu\n", gsx::extract_ws_layout(n.data(), (uint32_t)n.size(), r.data()));
    for (size_t s = 0; s < n.size(); ++s) printf("source%zu %zu %zu %zu\n", s, r[s].bases, r[s].partials, r[s].keep);
    return 0;
}

int main() {
    uint64_t n = 0;
    uint32_t filter = 0, invert = 0;
    bool have_mask = false, have_sel = false, have_edits = false;
    std::vector<uint32_t> mask, sel, edited, flags;
    std::string line;
    for (int c; (c = getchar()) != EOF;) {
        if (c != '\n') {
            line.push_back((char)c);
            continue;
        }
        const char* s = line.c_str();
        if (!strncmp(s, "n ", 2)) n = strtoull(s + 2, nullptr, 10);
        else if (!strncmp(s, "filter ", 7)) filter = (uint32_t)strtoul(s + 7, nullptr, 10);
        else if (!strncmp(s, "invert ", 7)) invert = (uint32_t)strtoul(s + 7, nullptr, 10);
        else if (!strncmp(s, "mask ", 5)) mask = numbers(s + 5, 16), have_mask = true;
        else if (!strncmp(s, "sel ", 4)) sel = numbers(s + 4, 16), have_sel = true;
        else if (!strncmp(s, "edited ", 7)) edited = numbers(s + 7, 16), have_edits = true;
        else if (!strncmp(s, "flags ", 6)) flags = numbers(s + 6, 10);
        else if (!strncmp(s, "layout ", 7)) return layout(s + 7);
        line.clear();
    }
    const uint64_t n_words = (n + 31) / 32, groups = gsx::extract_groups(n);
    if (n == 0 || (have_mask && mask.size() != n_words) || (have_sel && sel.size() != n_words) ||
        (have_edits && (edited.size() != n_words || flags.size() != n))) {
        fprintf(stderr, "bad input\n");
        return 2;
    }
    // step 1: the keep words and one popcount partial per group
    std::vector<uint32_t> keep(n_words), partials(groups, 0u), bases(groups);
    for (uint64_t w = 0; w < n_words; ++w) {
        gsx::ExtractWords x;
        x.mask = ((filter & 1u) && have_mask) ? mask[w] : 0xFFFFFFFFu;
        x.selection = (filter & 4u) ? (have_sel ? sel[w] : 0u) : 0xFFFFFFFFu;
        x.hidden = 0u;
        if ((filter & 2u) && have_edits)
            for (uint32_t b = 0; b < 32u; ++b) {
                const uint64_t i = w * 32u + b;
                if (i < n && ((edited[w] >> b) & 1u) && gsx::extract_flag_hides(flags[i])) x.hidden |= 1u << b;
            }
        keep[w] = gsx::extract_keep_word(x, invert != 0, n, w);
        partials[w / gsx::kExtractGroupWords] += gsx::extract_popc(keep[w]);
    }
    // step 2: the exclusive scan
    uint64_t total = 0;
    for (uint64_t g = 0; g < groups; ++g) {
        bases[g] = (uint32_t)total;
        total += partials[g];
    }
    // step 3: every kept Gaussian's destination, from the keep words alone
    std::vector<uint64_t> out(total);
    std::vector<uint8_t> written(total, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t w = i >> 5;
        const uint32_t bit = (uint32_t)(i & 31u);
        if (!((keep[w] >> bit) & 1u)) continue;
        uint64_t j = bases[w / gsx::kExtractGroupWords];
        for (uint64_t p = (w / gsx::kExtractGroupWords) * gsx::kExtractGroupWords; p < w; ++p) j += gsx::extract_popc(keep[p]);
        j += gsx::extract_rank(keep[w], bit);
        if (j >= total || written[j]) {
            fprintf(stderr, "destination %llu of source %llu is out of range or taken\n", (unsigned long long)j, (unsigned long long)i);
            return 3;
        }
        written[j] = 1;
        out[j] = i;
    }
    printf("count %llu\nkept", (unsigned long long)total);
    for (uint64_t j = 0; j < total; ++j) {
        if (!written[j]) {
            fprintf(stderr, "destination %llu was never written\n", (unsigned long long)j);
            return 4;
        }
        printf(" %llu", (unsigned long long)out[j]);
    }
    printf("\n");
    return 0;
}
