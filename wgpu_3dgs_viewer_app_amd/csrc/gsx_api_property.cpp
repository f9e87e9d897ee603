// gsx_api_property.cpp — C ABI of the model properties (spec/RENDER_SPEC.md section 17; kernels_property.hip):
// gsx_model_property_values, gsx_model_histogram and gsx_model_select_range.  The filter is model_filter's, the workspace the model
// operations' (v->extract_ws): [result block, 128 B | 4096 histogram words | the workgroups' partials, 64 KiB | the values of
// gsx_model_property_values].
#include "gsx_state.h"
#include "property_math.h"

using namespace gsx;

namespace {

constexpr size_t kWsHist = 4 * kPropResultWords;         // 128
constexpr size_t kWsPartials = kWsHist + 4 * kPropMaxBins;                            // 16 512
constexpr size_t kWsValues = kWsPartials + 4 * kPropPartialWords * kPropMaxGroups;    // 82 048: a multiple of 128
static_assert(sizeof(gsx_histogram_desc) == 24 && sizeof(gsx_histogram_t) == 48 && sizeof(gsx_select_desc) == 40, "spec section 17's layouts");
static_assert(kWsHist == 128 && kWsValues % 128 == 0, "the workspace regions are whole 128-byte lines");

// what all three calls check about (property, flags); allowed: the flag bits the call knows
gsx_status check_property(const char* fn, uint32_t property, uint32_t flags, uint32_t allowed) {
    if (property >= (uint32_t)GSX_PROP_COUNT) return fail(GSX_ERR_INVALID_ARG, "%s: unknown property %u", fn, property);
    if (flags & ~allowed) return fail(GSX_ERR_INVALID_ARG, "%s: unknown flag bits 0x%x", fn, flags);
    if ((flags & GSX_PROP_WORLD) && !prop_is_position(property))
        return fail(GSX_ERR_INVALID_ARG, "%s: GSX_PROP_WORLD with property %u, which is no position", fn, property);
    return GSX_OK;
}

// bind, find, refuse what gsx_model_extract refuses
gsx_status property_model(gsx_viewer* v, const char* fn, const char* key, Model** out) {
    gsx_status st = viewer_bind(v);  // behind the frames in flight on the lanes
    if (st) return st;
    Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "%s: no model '%s'", fn, key);
    if (has_comm(v)) return fail(GSX_ERR_UNSUPPORTED, "%s: the viewer has a communicator (call it before gsx_viewer_comm_init, or on one GPU)", fn);
    if (model_is_shard(m)) return fail(GSX_ERR_UNSUPPORTED, "%s: model '%s' is a shard of a multi-GPU frame", fn, key);
    *out = m;
    return GSX_OK;
}

PropertyJob property_job(const Model* m, uint32_t property, uint32_t flags, uint32_t* result /* the workspace */) {
    PropertyJob job{};
    job.property = property;
    // an identity transform gives the stored bits (as gsx_model_merge carries an identity source)
    job.world = ((flags & GSX_PROP_WORLD) && !merge_is_identity(m->mt.pos, m->mt.quat, m->mt.scale)) ? 1u : 0u;
    quat_to_rows(m->mt.quat, job.R);
    for (int k = 0; k < 3; ++k) {
        job.s[k] = m->mt.scale[k];
        job.t[k] = m->mt.pos[k];
    }
    job.result = result;
    job.partials = result + kWsPartials / 4;
    return job;
}

}  // namespace

extern "C" {

gsx_status gsx_model_property_values(gsx_viewer* v, const char* key, uint32_t property, uint32_t flags, float* out, uint64_t n) {
    if (!v || !key || !out) return fail(GSX_ERR_INVALID_ARG, "gsx_model_property_values: null argument");
    gsx_status st = check_property("gsx_model_property_values", property, flags, GSX_PROP_WORLD);
    if (st) return st;
    Model* m = nullptr;
    if ((st = property_model(v, "gsx_model_property_values", key, &m))) return st;
    if (n != m->n) return fail(GSX_ERR_INVALID_ARG, "gsx_model_property_values: expected %llu values", (unsigned long long)m->n);
    if (n == 0) return GSX_OK;
    HIPCHK(v->extract_ws.ensure(kWsValues + 4 * (size_t)n));
    char* ws = v->extract_ws.as<char>();
    PropertyJob job = property_job(m, property, flags, reinterpret_cast<uint32_t*>(ws));
    job.values = reinterpret_cast<float*>(ws + kWsValues);
    HIPCHK(launch_property(v->stream, kPropValues, (int)m->cov_kind, n, ModelFilter{}, extract_planes(m, false), job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    HIPCHK(gsx::op::Memcpy(out, job.values, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return GSX_OK;
}

gsx_status gsx_model_histogram(gsx_viewer* v, const char* key, const gsx_histogram_desc* desc, uint64_t* out_bins, gsx_histogram_t* out) {
    if (!v || !key || !desc || !out_bins || !out) return fail(GSX_ERR_INVALID_ARG, "gsx_model_histogram: null argument");
    gsx_status st = check_property("gsx_model_histogram", desc->property, desc->flags, GSX_PROP_WORLD | GSX_HIST_AUTO_RANGE);
    if (st) return st;
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "gsx_model_histogram: unknown filter bits 0x%x", desc->filter);
    if (desc->bins < 1u || desc->bins > kPropMaxBins) return fail(GSX_ERR_INVALID_ARG, "gsx_model_histogram: bins %u is not in 1 .. %u", desc->bins, kPropMaxBins);
    const bool auto_range = (desc->flags & GSX_HIST_AUTO_RANGE) != 0;
    if (!auto_range && !(prop_finite(desc->lo) && prop_finite(desc->hi) && desc->lo <= desc->hi))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_histogram: the range [%g, %g] is not finite and ordered", (double)desc->lo, (double)desc->hi);
    Model* m = nullptr;
    if ((st = property_model(v, "gsx_model_histogram", key, &m))) return st;
    *out = gsx_histogram_t{};
    if (!auto_range) {
        out->lo = desc->lo;
        out->hi = desc->hi;
    }
    for (uint32_t b = 0; b < desc->bins; ++b) out_bins[b] = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    HIPCHK(v->extract_ws.ensure(kWsValues));
    char* ws = v->extract_ws.as<char>();
    uint32_t* result = reinterpret_cast<uint32_t*>(ws);
    PropertyJob job = property_job(m, desc->property, desc->flags, result);
    job.hist = reinterpret_cast<uint32_t*>(ws + kWsHist);
    job.lo = desc->lo;
    job.hi = desc->hi;
    job.bins = desc->bins;
    job.auto_range = auto_range ? 1u : 0u;
    const ModelFilter f = model_filter(m, desc->filter, false);
    const ExtractPlanes src = extract_planes(m, false);
    HIPCHK(launch_property_reset(v->stream, result, job.hist, desc->bins));
    if (auto_range) HIPCHK(launch_property(v->stream, kPropReduce, (int)m->cov_kind, n, f, src, job));
    HIPCHK(launch_property(v->stream, kPropHist, (int)m->cov_kind, n, f, src, job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    std::vector<uint32_t> host(kPropResultWords + desc->bins);  // the result block and the bins: one copy
    HIPCHK(gsx::op::Memcpy(host.data(), ws, 4 * host.size(), hipMemcpyDeviceToHost));
    out->n_nonfinite = host[kPropNonfiniteAt];
    if (host[kPropCount] == 0u) return GSX_OK;  // nothing counted: zeros
    out->count = host[kPropCount];
    out->below = host[kPropBelowAt];
    out->above = host[kPropAboveAt];
    out->min = prop_unkey(host[kPropMinKey]);
    out->max = prop_unkey(host[kPropMaxKey]);
    if (auto_range) {
        out->lo = out->min;
        out->hi = out->max;
    }
    for (uint32_t b = 0; b < desc->bins; ++b) out_bins[b] = host[kPropResultWords + b];  // (32-bit on the device: a model has fewer than 2^32 Gaussians)
    return GSX_OK;
}

gsx_status gsx_model_select_range(gsx_viewer* v, const char* key, const gsx_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected) {
    if (!v || !key || !desc) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_range: null argument");
    gsx_status st = check_property("gsx_model_select_range", desc->property, desc->flags, GSX_PROP_WORLD);  // (AUTO_RANGE is not legal here)
    if (st) return st;
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_range: unknown filter bits 0x%x", desc->filter);
    if ((st = check_selection_op("gsx_model_select_range", desc->selection_op))) return st;
    if (desc->reserved != 0u) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_range: reserved is %u, not 0", desc->reserved);
    if (desc->bins > kPropMaxBins) return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_range: bins %u is above %u", desc->bins, kPropMaxBins);
    if (desc->bins && (desc->bin_lo > desc->bin_hi || desc->bin_hi >= desc->bins))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_range: bins [%u, %u] of %u", desc->bin_lo, desc->bin_hi, desc->bins);
    if (!(prop_finite(desc->lo) && prop_finite(desc->hi) && desc->lo <= desc->hi))
        return fail(GSX_ERR_INVALID_ARG, "gsx_model_select_range: the range [%g, %g] is not finite and ordered", (double)desc->lo, (double)desc->hi);
    Model* m = nullptr;
    if ((st = property_model(v, "gsx_model_select_range", key, &m))) return st;
    if (out_hit) *out_hit = 0;
    if (out_selected) *out_selected = 0;
    const uint64_t n = m->n;
    if (n == 0) return GSX_OK;
    HIPCHK(v->extract_ws.ensure(kWsValues));
    uint32_t* result = v->extract_ws.as<uint32_t>();
    const ModelFilter f = model_filter(m, desc->filter, false);  // (before has_selection changes: none selected = none pass)
    PropertyJob job = property_job(m, desc->property, desc->flags, result);
    if ((st = select_begin(v, m, desc->selection_op, job.partials, &job.sel))) return st;
    job.lo = desc->lo;
    job.hi = desc->hi;
    job.bins = desc->bins;
    job.bin_lo = desc->bin_lo;
    job.bin_hi = desc->bin_hi;
    HIPCHK(launch_property(v->stream, kPropSelect, (int)m->cov_kind, n, f, extract_planes(m, false), job));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    select_end(m);
    uint32_t host[kPropResultWords];
    HIPCHK(gsx::op::Memcpy(host, result, sizeof host, hipMemcpyDeviceToHost));
    if (out_hit) *out_hit = host[kPropHit];
    if (out_selected) *out_selected = host[kPropSelected];
    return GSX_OK;
}

}  // extern "C"
