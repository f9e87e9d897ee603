// extract_math.h — the word arithmetic of gsx_model_extract (spec/RENDER_SPEC.md §12, "Model extract"), written once: the kernels
// of kernels_extract.hip and the host restatement of tests/extract_driver.cpp both include it, so the two cannot drift.
// It holds the keep word of 32 Gaussians composed from their mask, selection and hidden words, its inversion, the bits of a
// plane's last word that lie at or above n, a Gaussian's rank among the kept ones of its word, and the layout of the workspace the
// keep and scan passes of every model operation share (gsx_model_extract, gsx_model_merge, gsx_model_export).
// Plain integer arithmetic; no HIP include (the functions are __host__ __device__ under hipcc).
#pragma once
#include <stddef.h>
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

// a workspace region's size: whole 128-byte lines
inline size_t extract_pad128(size_t b) { return (b + 127u) & ~size_t(127); }

// The workspace of the kept-set pass over n_src sources: the 64-bit totals of all sources first (source s at byte 8 s), then per
// source its bases, partials (extract_groups(n) words each) and keep words (ceil(n / 32)), every region padded to 128 bytes.  With
// one source the total lies at 0 and the bases at 128: total and bases are one contiguous copy.  Returns the workspace's bytes.
struct ExtractRegion {
    size_t bases, partials, keep;  // byte offsets
};
inline size_t extract_ws_layout(const uint64_t* n, uint32_t n_src, ExtractRegion* out) {
    size_t at = extract_pad128(sizeof(uint64_t) * n_src);
    for (uint32_t s = 0; s < n_src; ++s) {
        const size_t group_bytes = extract_pad128(4 * (size_t)extract_groups(n[s]));
        out[s].bases = at;
        out[s].partials = at + group_bytes;
        out[s].keep = at + 2 * group_bytes;
        at = out[s].keep + extract_pad128(4 * (size_t)((n[s] + 31u) / 32u));
    }
    return at;
}

}  // namespace gsx
