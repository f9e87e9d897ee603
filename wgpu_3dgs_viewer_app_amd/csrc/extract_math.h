// extract_math.h — the word arithmetic of gsx_model_extract (spec/RENDER_SPEC.md §12, "Model extract"), written once: the kernels
// of kernels_extract.hip and the host restatement of tests/extract_driver.cpp both include it, so the two cannot drift.
// It holds the keep word of 32 Gaussians composed from their mask, selection and hidden words, its inversion, the bits of a
// plane's last word that lie at or above n, and a Gaussian's rank among the kept ones of its word.
// Plain integer arithmetic; no HIP include (the functions are __host__ __device__ under hipcc).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GSX_EX_HD __host__ __device__
#else
#define GSX_EX_HD
#endif

namespace gsx {

// A workgroup of k_extract_keep and of k_extract_scatter owns this many consecutive Gaussians: 32 keep words, one popcount partial.
constexpr uint32_t kExtractGroup = 1024;
constexpr uint32_t kExtractGroupWords = kExtractGroup / 32u;
// k_extract_scan takes this many partials per pass of its one workgroup and carries the running sum from pass to pass.
constexpr uint32_t kExtractScanPass = 256;

constexpr uint32_t kExtractEditEnabled = 1u, kExtractEditHidden = 2u;  // GSX_EDIT_ENABLED, GSX_EDIT_HIDDEN (gsx.h)

GSX_EX_HD inline uint32_t extract_popc(uint32_t w) { return (uint32_t)__builtin_popcount(w); }

// does a stored edit flag hide its Gaussian?  (HIDDEN without ENABLED hides nothing)
GSX_EX_HD inline bool extract_flag_hides(uint32_t flag) { return (flag & kExtractEditEnabled) && (flag & kExtractEditHidden); }

// The bits of word w that belong to Gaussians below n: everything at or above n never counts, whatever a plane's last word holds.
GSX_EX_HD inline uint32_t extract_tail_mask(uint64_t n, uint64_t w) {
    const uint64_t lo = w * 32u;
    if (lo >= n) return 0u;
    if (n - lo >= 32u) return 0xFFFFFFFFu;
    return (1u << (uint32_t)(n - lo)) - 1u;
}

// The words a filter reads for word w of the model, with the absent planes already resolved: no mask (or MASKED not asked for) is
// all ones, SELECTED without a selection is zero, no edit records (or SKIP_HIDDEN not asked for) is a zero hidden word.
struct ExtractWords {
    uint32_t mask, selection, hidden;
};

// The keep word: the conjunction of the filter's flags, complemented over [0, n) when `invert`, tail bits cleared either way.
GSX_EX_HD inline uint32_t extract_keep_word(const ExtractWords& x, bool invert, uint64_t n, uint64_t w) {
    const uint32_t pass = x.mask & x.selection & ~x.hidden;
    return (invert ? ~pass : pass) & extract_tail_mask(n, w);
}

// rank of Gaussian `bit` of a word among the word's kept Gaussians (the bit itself not counted)
GSX_EX_HD inline uint32_t extract_rank(uint32_t keep_word, uint32_t bit) { return extract_popc(keep_word & ((1u << bit) - 1u)); }

// workgroups (= popcount partials) of a model of n Gaussians
GSX_EX_HD inline uint64_t extract_groups(uint64_t n) { return (n + kExtractGroup - 1u) / kExtractGroup; }

}  // namespace gsx
