// gsx_api_bounds.cpp — C ABI of the model bounds (spec/RENDER_SPEC.md section 11; kernels_bounds.hip).
#include "gsx_state.h"

using namespace gsx;

namespace {
// the workspace: [result, padded to 128 B | kBoundsMaxGroups partials | 3 x kBoundsBins histogram words]
constexpr size_t kWsPartials = 128;
constexpr size_t kWsHist = kWsPartials + sizeof(BoundsPartial) * kBoundsMaxGroups;
constexpr size_t kWsBytes = kWsHist + sizeof(uint32_t) * 3u * kBoundsBins;
static_assert(sizeof(gsx_model_bounds_t) == 88 && sizeof(gsx_model_bounds_t) <= kWsPartials, "gsx_model_bounds_t is 88 bytes");
static_assert(sizeof(BoundsPartial) == 64, "BoundsPartial is 64 bytes");
}  // namespace

extern "C" {

void gsx_bounds_desc_default(gsx_bounds_desc* d) {
    if (!d) return;
    *d = gsx_bounds_desc{0u, 0u};
}

gsx_status gsx_model_bounds(gsx_viewer* v, const char* key, const gsx_bounds_desc* desc, gsx_model_bounds_t* out) {
    if (!v || !desc || !out) return fail(GSX_ERR_INVALID_ARG, "gsx_model_bounds: null argument");
    if (desc->filter & ~kModelFilterBits) return fail(GSX_ERR_INVALID_ARG, "gsx_model_bounds: unknown filter bits 0x%x", desc->filter);
    if (desc->trim_permille >= 500u) return fail(GSX_ERR_INVALID_ARG, "gsx_model_bounds: trim_permille %u is not below 500", desc->trim_permille);
    gsx_status st = viewer_bind(v);
    if (st) return st;
    Model* m = find_model(v, key);
    if (!m) return fail(GSX_ERR_NOT_FOUND, "gsx_model_bounds: no model '%s'", key ? key : "(null)");
    HIPCHK(v->bounds_ws.ensure(kWsBytes));
    char* ws = v->bounds_ws.as<char>();
    gsx_model_bounds_t* d_out = reinterpret_cast<gsx_model_bounds_t*>(ws);
    BoundsPartial* partials = reinterpret_cast<BoundsPartial*>(ws + kWsPartials);
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws + kWsHist);
    const ModelFilter f = model_filter(m, desc->filter, false);
    // selected Gaussians of a model without a selection: none — no Gaussian is looked at
    const uint64_t n = f.select_none ? 0 : m->n;
    const bool trim = desc->trim_permille > 0 && n > 0;
    if (n) HIPCHK(launch_bounds_reduce(v->stream, m->pc.as<float4>(), n, f, partials));
    HIPCHK(launch_bounds_finish(v->stream, partials, n ? bounds_reduce_groups(n) : 0u, trim, d_out, hist));
    if (trim) HIPCHK(launch_bounds_trim(v->stream, m->pc.as<float4>(), n, f, desc->trim_permille, d_out, hist));
    HIPCHK(gsx::op::StreamSynchronize(v->stream));
    HIPCHK(gsx::op::Memcpy(out, d_out, sizeof *out, hipMemcpyDeviceToHost));
    return GSX_OK;
}

}  // extern "C"
