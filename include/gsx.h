/*
 * gsx.h — C ABI of libgsx.so, the MI355X-native 3D Gaussian Splatting render path.
 *
 * This header is the drop-in boundary for the one hot path of LioQing/wgpu-3dgs-viewer-app:
 * the per-splat render pipeline that the app drives through the Rust crate
 * `wgpu-3dgs-viewer 0.2.0` (Cargo.toml:25-31).  The reference has no C ABI; each entry point
 * below cites the reference call site (file:line under /root/reference/src) whose crate call it
 * replaces.  A Rust `gs::` facade over these symbols is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C, no C++ / torch types; all matrices column-major (glam `Mat4::to_cols_array()`).
 *  - every function returns gsx_status (0 = OK); gsx_last_error_string() gives a thread-local
 *    message.  Nothing aborts or throws across the ABI (reference: fallible calls return
 *    Result<_, gs::Error>, app.rs:548, scene.rs:234).
 *  - one viewer is used by one thread at a time (reference: "should not be used in multiple
 *    threads", scene.rs:1924-1930).
 *  - all device work is enqueued on the viewer's HIP stream; gsx_sync() is
 *    `device.poll(wgpu::Maintain::Wait)` (scene.rs:614, scene.rs:873).
 */
#ifndef GSX_H
#define GSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSX_ABI_VERSION 3u
#define GSX_TILE 16u /* screen tile edge in pixels (build-internal; the reference has no tiles) */
#define GSX_SH_COEFFS 15u /* SH degree 1..3 coefficients, each an RGB triple (gs::Gaussian::sh) */

typedef int32_t gsx_status;
enum {
    GSX_OK = 0,
    GSX_ERR_INVALID_ARG = 1,
    GSX_ERR_OOM = 2,
    GSX_ERR_HIP = 3,
    GSX_ERR_RCCL = 4,
    GSX_ERR_IO = 5, /* gs::Error::Io, scene.rs:234 */
    GSX_ERR_PLY = 6,
    GSX_ERR_NOT_FOUND = 7,
    GSX_ERR_UNSUPPORTED = 8,
    GSX_ERR_NO_DEVICE = 9
};

typedef struct gsx_viewer gsx_viewer; /* gs::MultiModelViewer<G>, scene.rs:1930 */

/* gs::Gaussian — the CPU-side Gaussian the app streams in (app.rs:1029-1031, scene.rs:2069-2085).
 * Field list follows wgpu-3dgs-viewer 0.2.0 (rot, pos, color, sh, scale). 224 bytes. */
typedef struct gsx_gaussian {
    float rot[4];    /* unit quaternion x,y,z,w (glam Quat) */
    float pos[3];
    uint8_t color[4]; /* r,g,b = clamp(0.5 + SH_C0*f_dc), a = sigmoid(opacity), UNORM8 */
    float sh[GSX_SH_COEFFS][3];
    float scale[3];  /* linear scale (exp already applied) */
} gsx_gaussian;

/* 8-way pod dispatch of the reference (scene.rs:23-81, app.rs:352-383). */
typedef enum gsx_sh_kind { GSX_SH_SINGLE = 0, GSX_SH_HALF = 1, GSX_SH_NORM8 = 2, GSX_SH_NONE = 3 } gsx_sh_kind;
typedef enum gsx_cov3d_kind { GSX_COV3D_SINGLE = 0, GSX_COV3D_HALF = 1 } gsx_cov3d_kind;

/* gs::GaussianDisplayMode (app.rs:1141-1165, transform.rs:106-146). */
typedef enum gsx_display_mode { GSX_DISPLAY_SPLAT = 0, GSX_DISPLAY_ELLIPSE = 1, GSX_DISPLAY_POINT = 2 } gsx_display_mode;

/* Constants of the render spec that the reference tree does not pin (SURVEY.md §8c [BUILD-SPEC]).
 * They are named and switchable so they can be reconciled against the real crate. */
typedef struct gsx_spec_params {
    float max_std_dev;    /* support cutoff: d^T Sigma^-1 d <= max_std_dev^2   (default 3.0) */
    float cull_margin;    /* clip-space frustum margin m: |x|,|y| <= m*w        (default 1.3) */
    float jacobian_clamp; /* view-space x/z,y/z clamp as a multiple of tan(fov/2) (default 1.3) */
    float low_pass;       /* added to the cov2d diagonal, px^2                  (default 0.3) */
    float alpha_max;      /* alpha = min(alpha_max, opacity*weight)             (default 1.0) */
    float alpha_min;      /* contributions with alpha < alpha_min are skipped   (default 0.0) */
    float t_epsilon;      /* front-to-back early termination: stop when T < eps (default 1e-4) */
    float point_radius;   /* GSX_DISPLAY_POINT dot radius in px at size 1       (default 2.0) */
} gsx_spec_params;

/* How gsx_render schedules one model's splats (build-internal; no reference counterpart).
 * progressive = 1: the depth-sorted splats are binned and composited front to back in growing depth slabs
 * [0, N_vis/first_slab_divisor), then `growth` times larger each; tiles whose every pixel has reached
 * T < t_epsilon are flagged and receive no further tile entries.  Pixels are identical to progressive = 0
 * (the per-pixel operation sequence is unchanged); only the work on hidden splats is skipped.
 * speculative = 1 (needs progressive): temporal occlusion speculation.  Every tile remembers the depth at which it
 * saturated in the model's previous frame; only the records in front of (1 + spec_margin) x that depth, maximised over
 * the tile's (2 spec_radius + 1)^2 neighbourhood, enter this frame's depth sort and binning.  The compositor verifies
 * the assumption on the device and a second round hands the tiles that are still open the records they were refused,
 * composited behind — pixels stay identical to speculative = 0 whatever the camera does; a wrong guess only costs
 * time.  After such a frame gsx_model_download_sorted returns the second round's (possibly empty) order, and the model
 * must go through gsx_preprocess + gsx_sort again before it is rendered once more (the app does so every frame;
 * gsx_render refuses otherwise: the frame's admission belongs to windows the frame has replaced).
 * host_verify: the (usually empty) second round is 8 kernel launches (round 6; ~20 before) that fall through at ~4 us of stream time each.
 * 0 (default): gsx_render never waits for the device; the second round is always enqueued.
 * 1: the device verification posts its verdict (how many tiles need the second round) into pinned host memory and
 * gsx_render waits for that one word before it returns; the second round is enqueued only when needed.  The next
 * frame's windows are enqueued before the wait.  The host can no longer run ahead of the device: it pays when the host
 * prepares a frame in a few tens of microseconds and repairs are rare (cfg4, 25 % of the frames repair: 1234 -> 1289 fps
 * from a lean Python loop, cfg3 1452 -> 1507) and costs dearly when they are not (cfg2, 94 %: 1527 -> 1002: the host
 * enqueues the second round while the device idles).
 * 2: ask only while repairs are rare — stop when six of the last eight verdicts needed the second round; the verdicts
 * keep being posted and the host looks at the latest one without waiting: eight repair-free ones in a row and it asks
 * again — AND only while the app waits for its frames anyway (it has called gsx_sync or a blocking readback since the
 * frame before, as the reference does twice per frame): a host that streams frames without waiting gets 0's behaviour
 * (round 6: the second round is 8 launches now; asking while streaming cost 6-10 %, profiles/r06_ab_host_verify.txt).
 * frames_in_flight = L > 1: gsx_render_frame deals consecutive frames round-robin to L lanes, each with its own stream and
 * per-frame buffers (records, sort and tile buffers, framebuffer, speculation windows: a lane speculates from ITS last
 * frame, L poses back); the Gaussian data is shared.  The device then overlaps the latency-bound tail of one frame with
 * the bandwidth-bound projection of the next: more frames per second, each taking longer from first to last kernel.
 * Frames still complete in order per lane and every frame is the same frame bit for bit.  Readback calls
 * (gsx_download_framebuffer, gsx_model_frame_stats, gsx_framebuffer_device_ptr ...) refer to the newest frame; a
 * framebuffer pointer stays valid until the same lane renders again (L frames later).  Calls that touch model data
 * (uploads, masks, selection / edits) are ordered after every frame in flight.  Frames with a selection, stored edits or the
 * highlight overlap like any other (the lanes read the viewer's selection and edit records; the per-frame preparation of those
 * runs only after one of its inputs changed, ordered between the frames in flight).  Depth-tested frames overlap as well (each
 * lane takes its own snapshot of the depth buffer: the depth block below has the ordering).  Frames with a query, a band
 * (gsx_viewer_set_band), an external framebuffer or a sharded model run on the viewer itself, one at a time. */
typedef struct gsx_render_options {
    uint32_t progressive;        /* default 1 */
    uint32_t first_slab_divisor; /* default 16; 1: the first slab is the whole model — one slab */
    uint32_t min_slab;           /* models with N_vis <= min_slab use one slab; default 131072 */
    uint32_t growth;             /* default 2 */
    uint32_t speculative;        /* default 1 */
    float spec_margin;           /* default 0.25 */
    uint32_t spec_radius;        /* default 3 (tiles) */
    uint32_t host_verify;        /* default 0 */
    uint32_t frames_in_flight;   /* default 1; 1 .. 4 — see below */
    uint32_t slab_shading;       /* default 1: a progressive frame WITHOUT windows (the first frame, a probe of the speculation tuner,
                                  * speculative = 0) projects geometry only and gives conic / colour records, depth slab by depth slab, to
                                  * exactly the records some block of tiles still takes — a few per cent of the visible ones on an opaque
                                  * scene; 0: such a frame projects every Gaussian in full (the reference's K1 + K3 vertex work for every
                                  * visible Gaussian).  Same pixels either way. */
} gsx_render_options;
/* progressive, speculative and slab_shading are read by gsx_preprocess: changing one of them sends every model back through
 * gsx_preprocess + gsx_sort.  first_slab_divisor, min_slab and growth are read by gsx_render and may change between gsx_sort and
 * gsx_render: the frame equals the one drawn with the final options throughout, bit for bit. */

typedef struct gsx_viewer_desc {
    uint32_t abi_version; /* GSX_ABI_VERSION */
    int32_t device;       /* HIP device ordinal */
    void* stream;         /* hipStream_t to enqueue on, or NULL to create one */
    uint32_t width, height; /* initial size; reference passes uvec2(1,1), scene.rs:1980 */
} gsx_viewer_desc;

/* ---- error / info ---- */
const char* gsx_last_error_string(void);
uint32_t gsx_abi_version(void);
void gsx_spec_params_default(gsx_spec_params* out);

/* ---- construction: gs::MultiModelViewer::new_with(device, format, depth_stencil, size), scene.rs:1969-1980 ---- */
gsx_status gsx_viewer_create(const gsx_viewer_desc* desc, gsx_viewer** out);
void gsx_viewer_destroy(gsx_viewer* v);
gsx_status gsx_viewer_set_spec_params(gsx_viewer* v, const gsx_spec_params* p);
void gsx_render_options_default(gsx_render_options* out);
gsx_status gsx_viewer_set_render_options(gsx_viewer* v, const gsx_render_options* o);

/* ---- models: MultiModelViewerGaussianBuffers::new_empty + BindGroups::new + models.insert,
 *      scene.rs:2111-2139; viewer.remove_model(&key), scene.rs:2176 ---- */
gsx_status gsx_model_create(gsx_viewer* v, const char* key, uint64_t count, gsx_sh_kind sh, gsx_cov3d_kind cov3d);
gsx_status gsx_model_remove(gsx_viewer* v, const char* key);
gsx_status gsx_model_len(gsx_viewer* v, const char* key, uint64_t* out_count); /* gaussians_buffer.len(), scene.rs:608 */

/* ---- upload: gaussians_buffer.update_range(queue, start, &[gs::Gaussian]), scene.rs:2083-2084.
 *      Converts Gaussian -> pod on the GPU (cov3d from rot/scale) into the resident SoA planes. ---- */
gsx_status gsx_model_upload_range(gsx_viewer* v, const char* key, uint64_t start, const gsx_gaussian* src, uint64_t n);
/* Zero-copy variant: pod-ready planes already in DEVICE memory (pos 3n, color n, sh 45n, cov3d 6n). */
gsx_status gsx_model_upload_pod_device(gsx_viewer* v, const char* key, uint64_t start, uint64_t n,
                                       const float* d_pos, const uint32_t* d_color, const float* d_sh,
                                       const float* d_cov3d);

/* ---- per-frame uniform setters (scene.rs:795-809) ---- */
/* viewer.update_camera(queue, &impl CameraTrait, uvec2 size), scene.rs:795 */
gsx_status gsx_update_camera(gsx_viewer* v, const float view[16], const float proj[16], uint32_t width, uint32_t height);
/* viewer.update_model_transform(queue, key, pos, quat, scale), scene.rs:796-802 */
gsx_status gsx_update_model_transform(gsx_viewer* v, const char* key, const float pos[3], const float quat_xyzw[4],
                                      const float scale[3]);
/* viewer.update_gaussian_transform(queue, size, display_mode, sh_deg, no_sh0), scene.rs:803-809 */
gsx_status gsx_update_gaussian_transform(gsx_viewer* v, float size, gsx_display_mode mode, uint32_t sh_deg,
                                         uint32_t no_sh0);

/* ---- mask (gs::MaskEvaluator result buffer, one bit per Gaussian, scene.rs:1851; app.rs:806-807) ---- */
gsx_status gsx_model_upload_mask(gsx_viewer* v, const char* key, const uint32_t* words, uint64_t n_words);
gsx_status gsx_model_download_mask(gsx_viewer* v, const char* key, uint32_t* words, uint64_t n_words);

/* gs::MaskEvaluator::evaluate(device, queue, &MaskOpTree, mask_buffer, model_transform_buffer, gaussians_buffer),
 * scene.rs:2124-2131, 2201-2209.  The tree (app.rs:1815-1837: Union | Intersection | Difference |
 * SymmetricDifference | Complement | Shape(&pod) | Reset) is passed in postfix order; n_ops == 0 is Reset
 * (every bit set).  A Gaussian is inside a shape when its WORLD position (model transform applied), taken
 * into the shape's frame (pos, rotation, scale), lies in the unit box |x|,|y|,|z| <= 1 or the unit ball.
 * Result: the model's mask buffer, bit = 1 kept / rendered.  One HIP kernel, no readback. */
typedef enum gsx_mask_shape_kind { GSX_MASK_BOX = 0, GSX_MASK_ELLIPSOID = 1 } gsx_mask_shape_kind;
typedef struct gsx_mask_shape { /* gs::MaskOpShapePod (gs::MaskShape {kind, pos, rotation, scale, color}) */
    uint32_t kind;
    float pos[3];
    float quat_xyzw[4];
    float scale[3];
} gsx_mask_shape;
typedef enum gsx_mask_opcode {
    GSX_MASK_OP_SHAPE = 0, /* push shape[arg] */
    GSX_MASK_OP_UNION = 1,
    GSX_MASK_OP_INTERSECTION = 2,
    GSX_MASK_OP_DIFFERENCE = 3, /* a - b, a pushed first */
    GSX_MASK_OP_SYMMETRIC_DIFFERENCE = 4,
    GSX_MASK_OP_COMPLEMENT = 5
} gsx_mask_opcode;
typedef struct gsx_mask_op { uint32_t opcode; uint32_t arg; } gsx_mask_op;
#define GSX_MASK_MAX_OPS 64u
#define GSX_MASK_MAX_SHAPES 32u
gsx_status gsx_mask_evaluate(gsx_viewer* v, const char* key, const gsx_mask_op* ops, uint32_t n_ops,
                             const gsx_mask_shape* shapes, uint32_t n_shapes);

/* ---- frame execution, split exactly like the reference's per-frame protocol (scene.rs:856-873, 2302-2314) ---- */
/* preprocessor.preprocess(encoder, bind_group, N): cull + SH colour + 3D->2D covariance + depth key. scene.rs:856-863 */
gsx_status gsx_preprocess(gsx_viewer* v, const char* key);
/* radix_sorter.sort(encoder, bind_group, indirect_args): depth radix sort of the surviving Gaussians. scene.rs:865-869 */
gsx_status gsx_sort(gsx_viewer* v, const char* key);
/* device.poll(Maintain::Wait), scene.rs:614 / scene.rs:873 */
gsx_status gsx_sync(gsx_viewer* v);
/* for key in model_render_keys (far -> near): renderer.render_with_pass(...), scene.rs:2302-2314.
 * Bins every model's sorted splats into 16x16 tiles and composites them; the result is the
 * premultiplied (r,g,b) + transmittance T framebuffer. */
gsx_status gsx_render(gsx_viewer* v, const char* const* keys_far_to_near, uint32_t n_keys);
/* preprocess + sort for every key, then render: one call per frame. */
gsx_status gsx_render_frame(gsx_viewer* v, const char* const* keys_far_to_near, uint32_t n_keys);

/* ---- depth test against the caller's depth buffer: the `depth_stencil` of gs::MultiModelViewer::new_with,
 *      DepthStencilState { Depth32Float, depth_write_enabled: false, Less } (scene.rs:1969-1980).  The app draws the mask
 *      gizmos and the measurement lines with depth write on first (scene.rs:2145-2160, renderer/measurement.rs:110-115); a
 *      splat behind them is hidden at that pixel (spec §6, "Depth test").  The library draws both itself
 *      (gsx_viewer_set_mask_gizmos, gsx_viewer_set_overlay_lines below), so the app needs no caller buffer for them: this block is
 *      for a host that draws something else of its own into the depth attachment.
 *  - The buffer is float32 [height][width] (row 0 at the top, like the framebuffer) of NDC depth in [0, 1], viewport-sized.
 *    A splat's fragments carry the depth of its centre; with GSX_DEPTH_LESS it is blended at pixel p only if it lies in front
 *    of D(p).  Nothing is written to the buffer.  Every model of a frame is tested against the same buffer.  D >= 1 (a cleared
 *    buffer) hides nothing: the frame is the one without the test, bit for bit; D <= 0 or NaN hides everything.
 *  - The test is made in the depth-key domain and needs a projection whose third and fourth rows depend on view z alone
 *    (P20 = P21 = P30 = P31 = P33 = 0, P32 = -1: perspective_rh, perspective_infinite_rh); gsx_preprocess refuses any other
 *    with GSX_ERR_INVALID_ARG while the test is on, as it refuses a buffer whose size is not the viewport's.
 *  - When the contents are read: on the viewer's stream, by the first gsx_preprocess of a frame (gsx_render_frame's
 *    included) — that snapshot decides which splats enter the depth sort and which pixels they reach; gsx_sort and gsx_render
 *    use it.  The buffer is read again by the next gsx_preprocess after gsx_render / gsx_render_frame, after gsx_update_camera,
 *    or for a model already preprocessed against the current snapshot (a new frame, whether or not the last one was rendered);
 *    every gsx_render_frame reads it.  Writing into a device buffer between gsx_preprocess and gsx_render changes nothing of
 *    that frame.  Calling gsx_viewer_set_depth_test,
 *    gsx_viewer_set_depth_buffer_device or gsx_viewer_upload_depth_buffer between gsx_preprocess and gsx_render makes
 *    gsx_render refuse the frame (GSX_ERR_INVALID_ARG): preprocess + sort the models again.
 *  - gsx_shard_* frames (and gsx_render_more) return GSX_ERR_INVALID_ARG while the test is on.
 *  - With frames_in_flight > 1 a depth-tested frame is dealt to a lane like any other; the lane takes its own snapshot, on its own
 *    stream.  The buffer's contents are read AS IF on the viewer's stream at the gsx_render_frame that uses them:
 *      (a) the lane's snapshot waits for what the viewer's stream held when the frame was dealt — every earlier library call
 *          (gsx_viewer_upload_depth_buffer among them) and, when gsx_viewer_desc.stream is the caller's own, whatever the caller
 *          enqueued there before the call (its writes into a device buffer);
 *      (b) the viewer's stream waits for the snapshot (an event, no host wait) — not for the frame: a later
 *          gsx_viewer_upload_depth_buffer or gsx_viewer_set_depth_buffer_device, and anything the caller enqueues on the viewer's
 *          stream after gsx_render_frame has returned, comes after that frame's read of the old contents.
 *    Frame k therefore sees the buffer as it was set for frame k, however many frames are in flight.  A caller that writes
 *    the buffer from another stream orders those writes against the viewer's stream itself.  GSX_DEPTH_LANES=0 (read when the
 *    viewer is created; A/B) keeps depth-tested frames on the viewer itself. */
typedef enum gsx_depth_compare { GSX_DEPTH_ALWAYS = 0 /* no test (default) */, GSX_DEPTH_LESS = 1 } gsx_depth_compare;
gsx_status gsx_viewer_set_depth_test(gsx_viewer* v, gsx_depth_compare compare);
/* Caller-owned DEVICE memory, 4-byte aligned, read in place: `height` rows of `width` floats, row_pitch_bytes apart (>= 4 * width, a
 * multiple of 4); it must
 * stay valid while frames that read it are in flight.  NULL detaches it (an uploaded buffer, if any, is used again). */
gsx_status gsx_viewer_set_depth_buffer_device(gsx_viewer* v, const float* d_ptr, uint32_t width, uint32_t height,
                                              uint64_t row_pitch_bytes);
/* A copy of host memory (width * height floats, tightly packed) into a viewer-owned buffer, ordered on the viewer's stream; it waits
 * for the stream (≈ 0.2 ms a call at 1920x1080: prefer the device buffer for a depth attachment that changes every frame);
 * replaces any device buffer set before. */
gsx_status gsx_viewer_upload_depth_buffer(gsx_viewer* v, const float* host, uint32_t width, uint32_t height);

/* ---- overlay lines: the app's measurement pass (MeasurementRenderer, src/renderer/measurement.rs:90-120 and :170-174,
 *      src/shader/measurement.wgsl:22-67), which SceneCallback::paint draws before the splats with depth write on.  Drawn by the
 *      library, so a host that shows measurement lines hands no depth attachment over (spec §9, "Overlay lines").
 *  - A line is the reference's HitPair: two world-space ends, an RGBA8 colour and a width; on screen a trapezoid whose half-width at
 *    an end is 0.01 * line_width * height / (2 * distance of that end from the eye), extended past each end by the same length.
 *    Lines are drawn in array order with `Less`, depth write on and straight alpha blending; a line with an end at w <= 0 and a
 *    line whose ends project to one point are not drawn.
 *  - When: where the depth snapshot is taken — by the first gsx_preprocess of a frame (gsx_render_frame's included), on the viewer's
 *    stream, and again under the snapshot's rules (the depth block above).  Also with GSX_DEPTH_ALWAYS.
 *  - The effective depth E(p): the caller's depth buffer D(p) where one is set (it must have the viewport's size), 1 otherwise, then
 *    lowered by every line fragment that passes `Less` against it.  The caller's buffer is never written.  With GSX_DEPTH_LESS the
 *    splats are tested against E — no caller buffer is needed while lines are set — with GSX_DEPTH_ALWAYS the lines lie behind every
 *    splat.  Either way the frame is final = rgb + T * line colour: gsx_download_framebuffer keeps returning the splats' (rgb, T),
 *    gsx_download_rgba8 and gsx_resolve_rgba8_device resolve over the overlay (rgb + T (C + (1 - A) background), alpha 1 - T (1 - A)).
 *  - gsx_viewer_set_overlay_lines between gsx_preprocess and gsx_render makes gsx_render refuse the frame, as the depth calls do.
 *  - While lines are set a frame runs on the viewer itself (frames_in_flight > 1: one at a time, like a frame with a query), and
 *    gsx_shard_* frames, gsx_render_more, gsx_viewer_set_band frames and an external framebuffer return GSX_ERR_INVALID_ARG.
 *  - With no lines set (never, or cleared with n = 0) nothing of this exists: the same launches, the same bits. */
typedef struct gsx_overlay_line { float p0[3]; uint8_t color[4]; float p1[3]; float line_width; } gsx_overlay_line; /* 32 B */
#define GSX_OVERLAY_MAX_LINES 4096u
/* MeasurementRenderer::update_hit_pairs (measurement.rs:133-167); host array, copied; n = 0 clears */
gsx_status gsx_viewer_set_overlay_lines(gsx_viewer* v, const gsx_overlay_line* lines, uint32_t n);

/* ---- mask gizmos: the wireframes of the mask shapes (gs::MaskGizmo; scene.rs:2141-2166 the pass, :2211-2247 its update, :2283-2293
 *      the draws), which SceneCallback::paint draws first of all, with the lines' depth state.  Drawn by the library (spec §10, "Mask
 *      gizmos"); with the lines above, the library then makes all the depth the app's splats are tested against.
 *  - A record is a mask shape in WORLD space — kind, pos, rotation quaternion (x, y, z, w), scale, as gsx_mask_shape — with a straight
 *    RGBA colour in [0, 1] (gs::MaskShape.color) and a width in gsx_overlay_line.line_width units.  The host passes, for each key of
 *    the frame's render keys, that model's visible boxes and then its visible ellipsoids.
 *  - The wireframe is the boundary of the set the mask tests (spec §2c): the 12 edges of the box, or the three circles of the
 *    ellipsoid in the shape's coordinate planes, GSX_GIZMO_CIRCLE_SEGMENTS chords each.  Every segment is clipped against the near
 *    plane (clip z >= 0) — the camera may sit inside a shape — and is then drawn as an overlay line is: the same trapezoid, `Less`,
 *    depth write, straight alpha blending into the same overlay and effective depth E.
 *  - Order: every gizmo segment, in record order then segment order, before the first overlay line.
 *  - Everything else is as for the lines: when they are drawn, E, the resolve, gsx_render's refusal of a frame preprocessed before
 *    the call, frames on the viewer itself while any are set, and the refusal of gsx_shard_* frames, gsx_render_more, band frames and
 *    an external framebuffer.  With none set nothing of this exists.
 *  - GSX_OVERLAY_BATCH_BOXES=0 (read when the viewer is created; A/B) makes the raster walk every batch of 64 records in every tile
 *    instead of culling batches by their pixel boxes; no result changes. */
typedef struct gsx_mask_gizmo { uint32_t kind; float pos[3]; float quat_xyzw[4]; float scale[3]; float color[4]; float line_width; } gsx_mask_gizmo; /* 64 B */
#define GSX_GIZMO_MAX_SHAPES 256u
#define GSX_GIZMO_CIRCLE_SEGMENTS 64u
/* gs::MaskGizmo::update + render_box_with_pass / render_ellipsoid_with_pass (scene.rs:2230-2246, :2283-2293); host array, copied;
 * n = 0 clears.  kind: gsx_mask_shape_kind; an unknown kind or a field that is not finite: GSX_ERR_INVALID_ARG */
gsx_status gsx_viewer_set_mask_gizmos(gsx_viewer* v, const gsx_mask_gizmo* gizmos, uint32_t n);
/* last frame's overlay: premultiplied rgba float [h][w][4] (zeros where nothing), effective depth [h][w]; either nullable; synchronises.
 * A frame without lines or gizmos has no overlay: zeros, and the caller's depth buffer (1 where there is none). */
gsx_status gsx_download_overlay(gsx_viewer* v, float* rgba, float* depth);
/* zero-copy: colour (float4 per pixel, meaningful only in tiles whose flag is 1), per-tile flags (u32 per 16x16 tile, row-major),
 * effective depth (float per pixel) — of the last frame rendered with lines or gizmos set; GSX_ERR_INVALID_ARG when there is none */
gsx_status gsx_overlay_device_ptrs(gsx_viewer* v, void** rgba, void** tile_flags, void** depth);

/* ---- readback (buffer.download(&device,&queue), app.rs:789, app.rs:806) ---- */
/* float32 [height][width][4] = premultiplied r,g,b and transmittance T. Synchronises. */
gsx_status gsx_download_framebuffer(gsx_viewer* v, float* rgbt, uint64_t n_floats);
/* resolve against a background colour into RGBA8 (what the egui target would hold). Synchronises. */
gsx_status gsx_download_rgba8(gsx_viewer* v, const float background_rgb[3], uint8_t* rgba, uint64_t n_bytes);
/* device pointer of the (rgb,T) framebuffer, for zero-copy consumers (RCCL merge, torch). */
gsx_status gsx_framebuffer_device_ptr(gsx_viewer* v, void** out_ptr, uint32_t* out_w, uint32_t* out_h);

/* ---- parity / introspection (no reference counterpart; used by tests and bench) ---- */
typedef struct gsx_frame_stats {
    uint64_t n_gaussians; /* N of the model */
    uint64_t n_visible;   /* N_vis after cull */
    uint64_t n_tile_entries; /* D = list entries binned by the last gsx_render: (Gaussian, tile) pairs for a frame that keeps
                                per-tile lists (progressive = 0, or a single-slab front model: all of them), (Gaussian, block of
                                tiles) pairs for the depth slabs of a progressive frame (fewer: see DESIGN.md, block lists) */
    uint64_t n_sorted;       /* records that entered the depth sort (= n_visible unless the frame was speculated) */
    uint64_t n_repair_tiles; /* speculated frame: tiles that needed the repair round */
    uint64_t n_repair_sorted; /* speculated frame: records that entered the repair round's depth sort */
    uint32_t speculated;     /* 1 if the last gsx_render of this model used last frame's windows */
    uint32_t overflow_slabs; /* depth slabs, over the model's lifetime, whose tile entries exceeded the pair buffers: their tails
                              * were composited pair-free on the device (complete pixels, slower) and the buffers grown */
} gsx_frame_stats;
gsx_status gsx_model_frame_stats(gsx_viewer* v, const char* key, gsx_frame_stats* out);
/* Per-Gaussian projection outputs of the last gsx_preprocess (host arrays of length N; any may be NULL):
 * depth_key (0xFFFFFFFF = culled), rect[4] = tile x0,y0,x1,y1 (exclusive max), mean2d[2],
 * conic_opacity[4], rgb[3]. */
gsx_status gsx_model_download_projection(gsx_viewer* v, const char* key, uint32_t* depth_key, uint32_t* rect,
                                         float* mean2d, float* conic_opacity, float* rgb);
/* Front-to-back order of the last gsx_sort: first n_visible entries are Gaussian indices. */
gsx_status gsx_model_download_sorted(gsx_viewer* v, const char* key, uint32_t* indices, uint64_t capacity,
                                     uint64_t* out_n_visible);
/* Tile lists of the last gsx_render for `key`: tile_offsets has tiles_x*tiles_y+1 entries, list holds D
 * Gaussian indices in front-to-back order per tile. */
gsx_status gsx_model_download_tile_lists(gsx_viewer* v, const char* key, uint32_t* tile_offsets,
                                         uint64_t n_offsets, uint32_t* list, uint64_t capacity);
/* Pod planes as resident in HBM (pos 3n, color n, sh 45n, cov3d 6n), for upload-conversion parity. */
gsx_status gsx_model_download_pod(gsx_viewer* v, const char* key, float* pos, uint32_t* color, float* sh,
                                  float* cov3d);

/* ---- model bounds: the box, the centre and the centroid of a model's Gaussian centres, computed on the device from the resident
 *      positions (spec/RENDER_SPEC.md §11 [BUILD-SPEC]).  `center` is GaussianSplattingModel::center, "the center of the bounding
 *      box" (src/app.rs:1019-1046): what world_center() and the far -> near model order (src/tab/scene.rs:533-558) are computed
 *      from, and what the reference leaves at Vec3::ZERO.
 *      Space and extent: model space (what world_center multiplies by the model transform); Gaussian CENTRES only, not their extent.
 *      Filter: any combination of the flags below; a Gaussian is counted if it passes every one that is set.  The stored buffers are
 *      read as they are: gsx_model_show_unedited does not change what GSX_BOUNDS_SKIP_HIDDEN means.
 *      Non-finite: a Gaussian that passes the filter and has a NaN or infinite coordinate is counted in n_nonfinite and left out of
 *      everything else.
 *      Trimming: k = count * trim_permille / 1000 (integer arithmetic).  Per axis, [trim_min, trim_max] leaves at most k counted
 *      Gaussians below it and at most k above it, and each end is within (max - min) / 2048 of the k-th value from its side; an
 *      axis whose range is zero, not a finite float32, or too small to divide into 2048 float32 bins returns min / max.
 *      With trim_permille = 0, trim_* equal min / max bit for bit.
 *      Empty result: count == 0 gives GSX_OK with every float field 0.0f.
 *      Errors: unknown filter bits or trim_permille >= 500: GSX_ERR_INVALID_ARG; unknown key: GSX_ERR_NOT_FOUND.
 *      Ordering: the call runs on the viewer's stream, behind the frames in flight and every upload enqueued before it, then
 *      synchronises and returns.  The result is the same bits from call to call.  It writes nothing a frame reads.
 *      Sharded viewers: the result covers the resident shard; a caller combines min / max / count across ranks itself.
 *      (The struct is gsx_model_bounds_t, as gsx_shard_layout_t is: C has one name space for a typedef and a function.) ---- */
#define GSX_BOUNDS_MASKED      1u  /* only Gaussians the model's mask keeps (bit set = kept; no mask = all) */
#define GSX_BOUNDS_SKIP_HIDDEN 2u  /* drop Gaussians whose stored edit has ENABLED and HIDDEN */
#define GSX_BOUNDS_SELECTED    4u  /* only selected Gaussians (no selection = none) */
typedef struct gsx_bounds_desc { uint32_t filter; uint32_t trim_permille; } gsx_bounds_desc; /* trim_permille < 500 */
typedef struct gsx_model_bounds_t {
    uint64_t count;       /* Gaussians that passed the filter and have a finite position */
    uint64_t n_nonfinite; /* passed the filter, some coordinate NaN or +-inf: left out of everything else */
    float min[3], max[3]; /* exact */
    float center[3];      /* 0.5f * (min + max), float32: GaussianSplattingModel::center */
    float mean[3];        /* centroid of the counted positions (summed in float64, rounded once) */
    float trim_min[3], trim_max[3];
} gsx_model_bounds_t; /* 88 bytes */
void gsx_bounds_desc_default(gsx_bounds_desc* d); /* filter 0, trim_permille 0 */
gsx_status gsx_model_bounds(gsx_viewer* v, const char* key, const gsx_bounds_desc* desc, gsx_model_bounds_t* out);

/* ---- model extract: part of a model becomes a new model, on the device (spec/RENDER_SPEC.md §12 [BUILD-SPEC]; the reference has no
 *      counterpart).  A stable stream compaction of src's resident planes: what a host does with a mask, a selection or hidden edits
 *      beyond hiding Gaussians every frame ("separate selection into a model", "apply the mask").
 *      Kept set: a Gaussian passes if it passes every GSX_BOUNDS_* flag set in `filter`, with gsx_model_bounds' exact meaning: no
 *      mask = all pass, no selection = none pass, GSX_BOUNDS_SKIP_HIDDEN reads the stored edit flag whatever gsx_model_show_unedited
 *      says.  GSX_EXTRACT_INVERT complements that conjunction over [0, n).  Bits of the last mask or selection word at or above n
 *      never count (a host may leave garbage there).  Non-finite positions are copied like any other.
 *      Order: kept Gaussians keep their relative order: the Gaussian at dst index j is the j-th kept one of src.  The result is the
 *      same bits on every call.
 *      Carried: every resident pod plane as stored bits (positions and colours, the covariance planes, the SH planes of the model's
 *      kind, the shade records): nothing is dequantised or requantised, dst has src's sh and cov3d kinds.  dst gets src's model
 *      transform.  Unless GSX_EXTRACT_DROP_EDITS is set, and if src has edit records, dst gets the kept Gaussians' stored edit records
 *      and edited bits; it gets no edit buffers if src has none.  dst has no mask (everything kept) and no selection, show_unedited is
 *      off, and it starts without speculation windows, like any new model.
 *      src is not written: its planes, mask, selection, edits and next frame are what they were.
 *      Empty result: if nothing is kept the call returns GSX_OK with *out_count == 0 and creates no model.
 *      Errors: a null viewer, key, desc or out, unknown filter or flag bits, a dst_key that exists or equals src_key:
 *      GSX_ERR_INVALID_ARG; unknown src_key: GSX_ERR_NOT_FOUND; a viewer with a communicator initialised, or a sharded src:
 *      GSX_ERR_UNSUPPORTED (index sharding assumes every rank knows the global count); allocation failure: GSX_ERR_OOM, with no dst
 *      left behind.
 *      Ordering: the call runs on the viewer's stream, behind every frame in flight on the lanes and every upload enqueued before it
 *      (as every call that touches model data: "frames in flight" above).  It waits once, for the kept count that sizes dst, then
 *      enqueues the copy.  When it returns, dst can be preprocessed, sorted and rendered, on lanes too. ---- */
#define GSX_EXTRACT_INVERT     1u  /* keep exactly the Gaussians the filter rejects */
#define GSX_EXTRACT_DROP_EDITS 2u  /* the new model starts without edit records */
typedef struct gsx_extract_desc { uint32_t filter; uint32_t flags; } gsx_extract_desc; /* filter: GSX_BOUNDS_* bits */
void gsx_extract_desc_default(gsx_extract_desc* d); /* filter 0, flags 0: a copy of the whole model */
gsx_status gsx_model_extract(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_extract_desc* desc, uint64_t* out_count);

/* ---- model merge: several models become one new model, on the device, their model transforms baked into the Gaussians
 *      (spec/RENDER_SPEC.md §13 [BUILD-SPEC]; the reference has no counterpart: it layers models by centre distance and never merges
 *      them).  The way back from gsx_model_extract: pieces that were split off and moved with gsx_update_model_transform become one
 *      model again, which sorts Gaussian by Gaussian where the pieces interpenetrate and pays one frame pipeline.
 *      Kept set: per source exactly gsx_model_extract's: desc->filter and desc->flags (GSX_EXTRACT_INVERT, GSX_EXTRACT_DROP_EDITS)
 *      apply to every source with that call's meaning (no mask = all pass, no selection = none pass, bits at or above n ignored).
 *      Order: the sources in the order given, inside a source the kept Gaussians in ascending index.  out_counts[s] (nullable) is the
 *      kept count of source s, *out_total their sum.  A key may appear twice: the model is then instantiated twice.  The result is
 *      the same bits on every call.
 *      Identity sources: a source whose model transform is exactly pos 0, scale 1, quat (0,0,0,1) or (0,0,0,-1) contributes its planes
 *      as stored bits, as gsx_model_extract would.
 *      Baked sources: every other source is dequantised exactly, baked and quantised again into the pod kind (§2b), so a Half or
 *      Norm8 source is quantised twice.  Positions p' = R_m (s_m * p) + t_m and covariances S' = M S M^T, M = R_m diag(s_m), in
 *      float32 with the float32 R_m the frame uses; the SH coefficients of bands 1..3 are multiplied by the band's rotation matrix
 *      of R_m (computed on the host in float64 from the normalised quaternion, rounded to float32) — the library evaluates SH in model
 *      space, so a rotation that is baked has to turn the coefficients too; a scale, negative components included, needs nothing.
 *      The colour word (DC and alpha) is carried.  The shade records are written to agree with the planes word for word.
 *      Pod kinds: every source must have the first source's sh and cov3d kinds, and dst takes them (GSX_ERR_INVALID_ARG otherwise).
 *      Sources of mixed kinds are converted first (gsx_model_convert, below), then merged.
 *      Edits: unless GSX_EXTRACT_DROP_EDITS is set, dst gets edit buffers if any source has edit records; kept Gaussians of such a
 *      source carry their stored records and edited bits (edits are colour operations), those of the other sources read as never
 *      edited.  dst has the identity transform, no mask, no selection, show_unedited off and no speculation windows.
 *      The sources are not written: their planes, masks, selections, edits, transforms and next frames are what they were.
 *      Empty result: if nothing is kept anywhere the call returns GSX_OK with *out_total == 0 and creates no model.
 *      Errors: a null viewer, key array, key, desc or out_total, n_src of 0 or above GSX_MERGE_MAX_SOURCES, unknown filter or flag
 *      bits, a dst_key that exists or equals a source, mixed pod kinds, a source transform with a non-finite component or a zero
 *      quaternion: GSX_ERR_INVALID_ARG; an unknown source: GSX_ERR_NOT_FOUND (the message names it); a viewer with a communicator, or
 *      a sharded source: GSX_ERR_UNSUPPORTED; allocation failure: GSX_ERR_OOM, with no dst left behind.
 *      Ordering: as gsx_model_extract, on the viewer's stream behind the lanes' frames.  The keep and scan passes of all sources are
 *      enqueued first; the call waits once, for the n_src counts that size dst, then enqueues the copies.  When it returns, dst can
 *      be preprocessed, sorted and rendered, on lanes too. ---- */
#define GSX_MERGE_MAX_SOURCES 64u
gsx_status gsx_model_merge(gsx_viewer* v, const char* const* src_keys, uint32_t n_src, const char* dst_key,
                           const gsx_extract_desc* desc, uint64_t* out_counts /* n_src entries, nullable */, uint64_t* out_total);

/* ---- model export: a resident model as gsx_gaussian records or as an INRIA PLY file, built on the device (spec/RENDER_SPEC.md §14
 *      [BUILD-SPEC]; the app's export modal and write_ply, src/app.rs:753-817 and 897-947, work on host Gaussians).  The way out for
 *      a model that exists only in device memory (gsx_model_extract, gsx_model_merge), and the way from one pod kind to another: the
 *      records can be uploaded with gsx_model_upload_range into a model of any kind.
 *      Kept set and order: exactly gsx_model_extract's, from `filter` (GSX_BOUNDS_* bits) and GSX_EXTRACT_INVERT: no mask = all pass,
 *      no selection = none pass, bits at or above n ignored; kept Gaussians appear in ascending index order.
 *      Space: model space.  The model transform is NOT applied; a caller who wants it baked calls gsx_model_merge first.
 *      pos: the stored bits, non-finite values included.  sh[15][3]: the exact dequantisation (§2b) of the resident planes, zeros for
 *      an Sh None model.  color: the stored colour word unless edits are baked.  Uploading the records into a model of the same pod
 *      kind therefore reproduces the position, colour and SH planes bit for bit.
 *      rot and scale: from the stored covariance, dequantised exactly, by a cyclic Jacobi eigen-solve in float32 with a fixed number
 *      of sweeps in a fixed pair order (the same bits on every call).  scale_k = sqrtf(max(lambda_k, 0)), scale_0 >= scale_1 >=
 *      scale_2; the eigenvector matrix is made a proper rotation (last column flipped if the determinant is negative); the quaternion
 *      is normalised and has w >= 0 (w == 0: the first non-zero of x, y, z is positive).  The covariance that the upload conversion
 *      makes of (rot, scale) differs from the stored one by at most 4 x what a float64 eigen-solve rounded to float32 gives (§14).
 *      Special cases: an all-zero covariance gives rot (0,0,0,1) and scale 0; a non-finite entry (a Half covariance that overflowed)
 *      gives rot (0,0,0,1) and scale_k = sqrtf(fmaxf(S_kk, 0)), unsorted; a negative eigenvalue (Half rounding) gives scale 0.
 *      Edits: with GSX_EXPORT_BAKE_EDITS on a model that has edit records, a Gaussian whose `edited` bit is set and whose record has
 *      ENABLED gets spec §7 Export's arithmetic, as gsx_ply_write applies it: PLY rows f_dc = (c - 0.5) / C0 from the edited float
 *      colour and opacity = logit(clamp(a, 1e-6, 1 - 1e-6)); records color = floor(255 * clamp(x, 0, 1) + 0.5) per channel.  HIDDEN
 *      Gaussians are dropped only if `filter` has GSX_BOUNDS_SKIP_HIDDEN; gsx_model_show_unedited changes nothing here.  Without the
 *      flag, or on a model without edit records, the stored colour word is exported.
 *      PLY rows: 62 float32 in gsx_ply_write's property order, exactly its conversion of the record: normals 0, f_rest channel-major,
 *      rot as w, x, y, z, scale_k = logf(scale_k) (a zero scale writes -inf).
 *      gsx_model_export: `out` NULL returns only the kept count in *out_count.  Otherwise capacity_bytes must hold count x row bytes;
 *      if it does not, GSX_ERR_INVALID_ARG with *out_count the needed count and nothing written.  A count of 0 is GSX_OK and writes
 *      nothing.
 *      gsx_model_export_ply: the whole file: gsx_ply_write's header for the kept count, byte for byte, then the rows; desc->format is
 *      ignored.  `out` NULL returns the size in *out_size; a capacity below it is GSX_ERR_INVALID_ARG with *out_size set.  The
 *      reference's write_ply(edits, mask) is filter = MASKED | SKIP_HIDDEN, flags = BAKE_EDITS.
 *      Staging: rows are produced into one of two device staging buffers of staging_bytes each (0: the library's default, 32 MiB;
 *      raised to 1024 rows) and copied to `out` chunk by chunk, the kernel of a chunk running while the chunk before it is copied.
 *      The buffers belong to the viewer, are counted by gsx_debug_device_bytes and are freed with it.
 *      Errors: a null viewer, key, desc or count / size pointer, unknown filter bits, flag bits (2u included), format, a non-zero
 *      `reserved`: GSX_ERR_INVALID_ARG; unknown key: GSX_ERR_NOT_FOUND; a viewer with a communicator, or a sharded model:
 *      GSX_ERR_UNSUPPORTED.
 *      Ordering: as gsx_model_extract, on the viewer's stream behind the lanes' frames in flight and earlier uploads.  The call
 *      returns when `out` is complete.  The model is not written: its planes, mask, selection, edits and next frame are what they
 *      were. ---- */
#define GSX_EXPORT_GAUSSIANS    0u /* gsx_gaussian records, 224 B each */
#define GSX_EXPORT_PLY_VERTICES 1u /* INRIA rows, 62 f32 = 248 B each, property order of gsx_ply_write */
#define GSX_EXPORT_BAKE_EDITS   4u /* flag; GSX_EXTRACT_INVERT (1u) is the other legal flag, 2u is not legal here */
typedef struct gsx_export_desc { uint32_t filter; uint32_t flags; uint32_t format; uint32_t reserved; uint64_t staging_bytes; } gsx_export_desc; /* 24 B */
void gsx_export_desc_default(gsx_export_desc* d); /* all zero: whole model, gsx_gaussian records, library-chosen staging */
gsx_status gsx_model_export(gsx_viewer* v, const char* key, const gsx_export_desc* desc, void* out, uint64_t capacity_bytes, uint64_t* out_count);
gsx_status gsx_model_export_ply(gsx_viewer* v, const char* key, const gsx_export_desc* desc, void* out, uint64_t capacity, uint64_t* out_size);

/* ---- PLY import on the device (spec/RENDER_SPEC.md §15 [BUILD-SPEC]): the load path of the app, read_ply_header -> read_ply_gaussians
 *      -> Gaussian::from -> update_range (src/app.rs:1053-1096), without a gsx_gaussian record in between.  Binary vertex rows are
 *      copied into device staging and decoded there straight into the resident planes; the bits a model holds afterwards are those
 *      gsx_model_upload_range leaves for the §15 records of the rows.  Against gsx_ply_read_gaussians (which goes through the host's
 *      float32 expf): pos, rot, sh and the rgb bytes are the same bits for finite inputs, scale is within 1 float32 ulp, alpha within 1.
 *      gsx_model_upload_ply_rows: the streaming form.  `rows` are n binary rows of header->vertex_bytes each (the file's data +
 *      header_bytes + first_row * vertex_bytes), in host memory; they become the Gaussians [start, start + n) of model `key`.  Keys,
 *      ranges, shards and ordering are gsx_model_upload_range's: wherever that call is legal, this one is.  n == 0 is GSX_OK and does
 *      nothing.  The header is the caller's and is checked before a row is read: not ascii, 0 < vertex_bytes <= 1024, every offset -1
 *      or inside the row (offset + 4 <= vertex_bytes), the fourteen properties gsx_ply_read_header requires present; a header that
 *      fails is GSX_ERR_INVALID_ARG, but an ascii one or a stride above 1024 is GSX_ERR_UNSUPPORTED (gsx_ply_read_gaussians reads
 *      those).  Offsets and strides need not be multiples of 4.
 *      gsx_model_import_ply: the whole file.  Runs gsx_ply_read_header, creates model `key` with the header's count and the given pod
 *      kinds, decodes every row; *out_count receives the count.  A count of 0 is GSX_OK with *out_count 0 and no model.
 *      Staging: rows pass through the two device staging buffers the export uses, of staging_bytes each (0: the library's default,
 *      32 MiB; raised to 1024 rows, never more rows than the call has); the kernel of a chunk runs while the next chunk is copied.  The
 *      buffers belong to the viewer, are counted by gsx_debug_device_bytes and are freed with it.
 *      Errors: a null viewer, key, data / header, desc or count pointer, a key that exists, flag bits (none are defined), a non-zero
 *      reserved: GSX_ERR_INVALID_ARG.  Header errors: GSX_ERR_PLY as gsx_ply_read_header returns them.  size below header_bytes +
 *      count x vertex_bytes: GSX_ERR_IO.  ascii, a stride above 1024, a viewer with a communicator: GSX_ERR_UNSUPPORTED.  Allocation
 *      failure: GSX_ERR_OOM.  After an error of gsx_model_import_ply no model `key` exists and the viewer's device bytes are what they
 *      were, the staging buffers apart.
 *      Ordering: as gsx_model_extract, on the viewer's stream behind the lanes' frames in flight and earlier uploads.  Both calls
 *      return when the caller's memory is no longer read and the kernels are complete. ---- */
typedef struct gsx_ply_header gsx_ply_header; /* defined with the PLY I/O block below */
typedef struct gsx_import_desc { uint32_t flags; uint32_t reserved; uint64_t staging_bytes; } gsx_import_desc; /* 16 B */
void gsx_import_desc_default(gsx_import_desc* d); /* all zero */
gsx_status gsx_model_upload_ply_rows(gsx_viewer* v, const char* key, uint64_t start, const void* rows, uint64_t n,
                                     const gsx_ply_header* header, const gsx_import_desc* desc);
gsx_status gsx_model_import_ply(gsx_viewer* v, const char* key, const void* data, uint64_t size, gsx_sh_kind sh,
                                gsx_cov3d_kind cov3d, const gsx_import_desc* desc, uint64_t* out_count);

/* ---- model convert: a resident model into another pod kind, on the device (spec/RENDER_SPEC.md §16 [BUILD-SPEC]).  The app's
 *      Compression Settings (src/app.rs:152-177: SH Single / Half / Norm8 / Remove, covariance Single / Half) take effect when a file
 *      is loaded; these calls apply them to a model that is resident, an extracted or merged one included.
 *      gsx_model_pod_kind: the kinds the model's planes are stored in (those it was created with, or of the last
 *      gsx_model_set_pod_kind).  A null argument: GSX_ERR_INVALID_ARG; an unknown key: GSX_ERR_NOT_FOUND.
 *      gsx_model_convert is gsx_model_extract into a model of the kind (desc->sh, desc->cov3d).  The kept set and its order
 *      (desc->filter: GSX_BOUNDS_* bits; desc->flags: GSX_EXTRACT_INVERT | GSX_EXTRACT_DROP_EDITS), what dst gets and lacks (src's
 *      transform, the kept edit records and edited bits unless dropped; no mask, no selection, no speculation windows), the empty
 *      result (GSX_OK, *out_count == 0, no model), the ordering (on the viewer's stream behind the lanes' frames, one wait for the
 *      count), "src is not written" and every error case are gsx_model_extract's; in addition desc->sh or desc->cov3d out of range is
 *      GSX_ERR_INVALID_ARG.
 *      Planes: position and colour word are carried as stored bits.  Covariance and SH are dequantised exactly (§2b) and quantised
 *      once into the destination kind (f16: round to nearest even, overflow to infinity; snorm8: clamp, floor(v * 127 + 0.5)); the
 *      spare slots at SH floats 45 and above are zero; the shade records agree with the planes word for word, spare words zero.
 *      That is: dst holds the bits gsx_model_upload_pod_device leaves in a fresh model of the destination kind for the four planes
 *      gsx_model_download_pod returns of the kept Gaussians of src.  A source of Sh None stands for 45 zeros; a destination of Sh None
 *      drops the SH and has no shade records.  When the kinds equal src's the call IS gsx_model_extract, bit for bit.  The same bits
 *      on every call.
 *      gsx_model_set_pod_kind: the menu entry applied to a loaded model, which keeps its key.  Its planes become what
 *      gsx_model_convert with filter 0 makes.  It keeps its length, its transform, its mask (with the mask program's hash), its
 *      selection, its edit records and edited bits and show_unedited: those buffers are moved, not copied.  What a frame caches starts
 *      again as for a new model: no speculation windows, the tuner reset, the next frame an unspeculated one, on lanes too.  Handles
 *      retained before the call keep their snapshots.  The same kind returns GSX_OK and does nothing.  Old and new planes exist side
 *      by side during the call; on GSX_ERR_OOM the model is what it was.  Unknown key: GSX_ERR_NOT_FOUND; kind out of range:
 *      GSX_ERR_INVALID_ARG; a viewer with a communicator, or a sharded model: GSX_ERR_UNSUPPORTED.  Ordering as gsx_model_extract;
 *      when it returns the model can be preprocessed, sorted and rendered, on lanes too. ---- */
gsx_status gsx_model_pod_kind(gsx_viewer* v, const char* key, gsx_sh_kind* out_sh, gsx_cov3d_kind* out_cov3d);
typedef struct gsx_convert_desc { uint32_t filter; uint32_t flags; uint32_t sh; uint32_t cov3d; } gsx_convert_desc; /* 16 B */
void gsx_convert_desc_default(gsx_convert_desc* d); /* all zero: the whole model, Sh Single, Cov3d Single */
gsx_status gsx_model_convert(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_convert_desc* desc, uint64_t* out_count);
gsx_status gsx_model_set_pod_kind(gsx_viewer* v, const char* key, gsx_sh_kind sh, gsx_cov3d_kind cov3d);

/* ---- model properties: one float32 per Gaussian, its histogram, and a selection by range, on the device (spec/RENDER_SPEC.md §17
 *      [BUILD-SPEC]).  The reference's Selection tab stops at screen-space tools; "the near-transparent splats", "the huge ones",
 *      "everything above a height", "everything of one colour" are choices by a stored property, made here without a Gaussian
 *      crossing to the host.
 *      Properties (gsx_property): POS_X/Y/Z the stored position bits in model space — with GSX_PROP_WORLD the model transform applied
 *      as gsx_model_merge bakes a position, p' = R_m (s_m * p) + t_m in float32, an identity transform giving the stored bits;
 *      RED/GREEN/BLUE/OPACITY the bytes of the stored colour word / 255.0f; HUE/SATURATION/VALUE the HSV of those three (spec §7's
 *      conversion); SCALE_MAX/MID/MIN scale[0..2] as gsx_model_export solves them from the stored covariance (spec §14), special cases
 *      included.  Stored values are read as they are: edits are not applied, gsx_model_show_unedited changes nothing.
 *      GSX_PROP_WORLD with a property that is no position is GSX_ERR_INVALID_ARG.
 *      gsx_model_property_values: out[i] = the property of Gaussian i, non-finite values as they come; n must be the model's length.
 *      gsx_model_histogram: a Gaussian that passes desc->filter (GSX_BOUNDS_* bits, gsx_model_bounds' meaning) and has a finite value
 *      is counted in `count`; min / max are exact over those (-0 below +0); counted values below lo / above hi go to `below` /
 *      `above`, the others into desc->bins (1 .. 4096) equal bins over [lo, hi], written to out_bins[0 .. bins): their sum is count -
 *      below - above.  NaN and +-inf go to n_nonfinite only.  The bin of a value: edge(0) = lo, edge(bins) = hi, edge(b) = min(hi, lo
 *      + b * width) with width = (hi - lo) / bins; b is the bin with edge(b) <= v <= edge(b + 1) reached from floor((v - lo) * (bins /
 *      (hi - lo))); a range that is zero, not finite, or too small for `bins` float32 bins puts every in-range value into bin 0.
 *      GSX_HIST_AUTO_RANGE: desc->lo / hi are ignored, [min, max] is the range and is returned in out->lo / hi (otherwise they echo
 *      the desc).  count == 0 is GSX_OK with zeros.  lo > hi or a non-finite lo / hi without AUTO_RANGE: GSX_ERR_INVALID_ARG.  The
 *      same bits on every call; nothing a frame reads is written.
 *      gsx_model_select_range: a Gaussian is hit if it passes desc->filter, its value is finite, lo <= value <= hi and, when
 *      desc->bins > 0, its bin under (lo, hi, bins) lies in [bin_lo, bin_hi] — so the hit count is the sum of the bins bin_lo ..
 *      bin_hi of the histogram with the same property, flags, filter, bins, lo and hi, and selecting each bin in turn partitions the
 *      in-range set.  selection_op (gsx_selection_op): Set, the selection becomes the hit set; Add, |=; Remove, &= ~.
 *      GSX_BOUNDS_SELECTED in the filter reads the selection as it was before the call.  A model without a selection gets one (none
 *      = none selected); bits at or above n are written 0.  *out_hit (nullable): the hit count; *out_selected (nullable): the
 *      selected count afterwards.  GSX_HIST_AUTO_RANGE is not legal here.  Ordering and frame consistency are
 *      gsx_model_upload_selection's: on the viewer's stream behind the lanes' frames in flight, the next frame sees the selection.
 *      Errors of all three: a null viewer, key, desc or required out pointer, an unknown property, flag, filter bit or op, bins out
 *      of range, bin_lo > bin_hi, bin_hi >= bins, reserved != 0: GSX_ERR_INVALID_ARG; unknown key: GSX_ERR_NOT_FOUND; a viewer with a
 *      communicator, or a sharded model: GSX_ERR_UNSUPPORTED.  A model of 0 Gaussians: GSX_OK with zeros. ---- */
typedef enum gsx_property {
    GSX_PROP_POS_X = 0, GSX_PROP_POS_Y = 1, GSX_PROP_POS_Z = 2,
    GSX_PROP_RED = 3, GSX_PROP_GREEN = 4, GSX_PROP_BLUE = 5, GSX_PROP_OPACITY = 6,
    GSX_PROP_HUE = 7, GSX_PROP_SATURATION = 8, GSX_PROP_VALUE = 9,
    GSX_PROP_SCALE_MAX = 10, GSX_PROP_SCALE_MID = 11, GSX_PROP_SCALE_MIN = 12,
    GSX_PROP_COUNT = 13
} gsx_property;
#define GSX_PROP_WORLD      1u  /* positions in world space (the model transform applied as gsx_model_merge bakes it) */
#define GSX_HIST_AUTO_RANGE 4u  /* gsx_model_histogram: the range is [min, max] of the counted values */
#define GSX_HIST_MAX_BINS   4096u
typedef struct gsx_histogram_desc { uint32_t property; uint32_t flags; uint32_t filter; uint32_t bins; float lo; float hi; } gsx_histogram_desc; /* 24 B */
typedef struct gsx_histogram_t { uint64_t count; uint64_t below; uint64_t above; uint64_t n_nonfinite; float lo; float hi; float min; float max; } gsx_histogram_t; /* 48 B */
typedef struct gsx_select_desc {
    uint32_t property; uint32_t flags; uint32_t filter; uint32_t selection_op; /* gsx_property, GSX_PROP_WORLD, GSX_BOUNDS_*, gsx_selection_op */
    float lo; float hi;
    uint32_t bins; uint32_t bin_lo; uint32_t bin_hi; uint32_t reserved; /* bins 0: the range alone; reserved: 0 */
} gsx_select_desc; /* 40 B */
gsx_status gsx_model_property_values(gsx_viewer* v, const char* key, uint32_t property, uint32_t flags, float* out, uint64_t n);
gsx_status gsx_model_histogram(gsx_viewer* v, const char* key, const gsx_histogram_desc* desc, uint64_t* out_bins, gsx_histogram_t* out);
gsx_status gsx_model_select_range(gsx_viewer* v, const char* key, const gsx_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected);

/* ---- model neighbours: how many other Gaussians lie within a radius of each one, and a selection by that count, on the device
 *      (spec/RENDER_SPEC.md §18 [BUILD-SPEC]).  Floaters, the isolated splats of a capture, are the Gaussians with few neighbours:
 *      gsx_model_select_neighbors with max_count = k, count_lo = 0, count_hi = k - 1, then gsx_model_extract with
 *      GSX_BOUNDS_SELECTED and GSX_EXTRACT_INVERT.  No Gaussian crosses to the host.
 *      Participants: a Gaussian participates if it passes desc->filter (GSX_BOUNDS_* bits, gsx_model_bounds' meaning) and its three
 *      stored position coordinates are finite; stats.count is their number.  One that passes the filter with a NaN or infinite
 *      coordinate goes to n_nonfinite.  Who does not participate is nobody's neighbour and has count 0.
 *      Distance: model space, the stored position bits as they are — the model transform, the edits and gsx_model_show_unedited change
 *      nothing.  d2(i, j) = (dx*dx + dy*dy) + dz*dz in float32, every operation rounded, dx dy dz the float32 coordinate
 *      differences; r2 = radius * radius in float32.  j is a neighbour of i iff j != i, both participate and d2 <= r2: symmetric;
 *      coincident Gaussians are neighbours of one another; a difference that overflows gives d2 = inf and no neighbour.
 *      Counts: out_counts[i] (nullable; the model's length) = min(neighbours of i, max_count) for a participant, 0 otherwise, 1 <=
 *      max_count <= GSX_NEIGHBOR_MAX_COUNT.  out_hist[c] (nullable; max_count + 1 entries) = the participants with saturated count
 *      c; its sum is stats.count.  The same bits on every call; nothing a frame reads is written.
 *      gsx_model_select_neighbors: a Gaussian is hit iff it participates and count_lo <= its saturated count <= count_hi (count_hi
 *      <= max_count), so *out_hit is the sum of out_hist[count_lo .. count_hi] of gsx_model_neighbors with the same filter, radius
 *      and max_count.  selection_op, a model without a selection, the tail bits, GSX_BOUNDS_SELECTED reading the selection as it was
 *      before the call, *out_hit / *out_selected (nullable), ordering and frame consistency: gsx_model_select_range's.
 *      grid_bits: 0 lets the library choose its hash table, 1 .. 24 forces 2^grid_bits buckets; no value changes a result;
 *      stats.grid_bits returns the value used.
 *      Errors: a null viewer, key, desc or stats pointer, unknown filter bits or op, flags != 0 (none are defined), a radius that is
 *      not finite or not above 0 or whose float32 square is 0 or inf, max_count 0 or above 4095, grid_bits > 24, count_lo > count_hi,
 *      count_hi > max_count, a reserved word != 0: GSX_ERR_INVALID_ARG; unknown key: GSX_ERR_NOT_FOUND; a viewer with a communicator,
 *      or a sharded model: GSX_ERR_UNSUPPORTED; an allocation failure: GSX_ERR_OOM, the model and its selection as they were.  A
 *      model of 0 Gaussians, or 0 participants: GSX_OK with zeros (a select with Set then clears the selection). ---- */
#define GSX_NEIGHBOR_MAX_COUNT 4095u
typedef struct gsx_neighbor_desc { uint32_t filter; uint32_t flags; float radius; uint32_t max_count; uint32_t grid_bits; uint32_t reserved; } gsx_neighbor_desc; /* 24 B */
typedef struct gsx_neighbor_stats_t { uint64_t count; uint64_t n_nonfinite; uint32_t grid_bits; uint32_t reserved; } gsx_neighbor_stats_t; /* 24 B */
typedef struct gsx_neighbor_select_desc {
    uint32_t filter; uint32_t flags; uint32_t selection_op; uint32_t max_count; /* GSX_BOUNDS_*, 0, gsx_selection_op, 1 .. 4095 */
    float radius; uint32_t count_lo; uint32_t count_hi; uint32_t grid_bits; uint32_t reserved[2];
} gsx_neighbor_select_desc; /* 40 B */
void gsx_neighbor_desc_default(gsx_neighbor_desc* d); /* no filter, radius 1, max_count 4095, the library's table */
gsx_status gsx_model_neighbors(gsx_viewer* v, const char* key, const gsx_neighbor_desc* desc, uint32_t* out_counts, uint64_t* out_hist, gsx_neighbor_stats_t* out);
gsx_status gsx_model_select_neighbors(gsx_viewer* v, const char* key, const gsx_neighbor_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected);

/* ---- model clusters: the connected pieces of a model under "within a radius of one another", and a selection by them, on the
 *      device (spec/RENDER_SPEC.md §19 [BUILD-SPEC]).  Keep the object, drop the debris: gsx_model_select_clusters in mode
 *      GSX_CLUSTER_LARGEST, then gsx_model_extract with GSX_BOUNDS_SELECTED; or mode GSX_CLUSTER_BY_SIZE with (1, k - 1), then
 *      extract with GSX_EXTRACT_INVERT.  Select linked: brush a few Gaussians, then mode GSX_CLUSTER_SEEDED with GSX_SELECTION_ADD.
 *      Participants, distance and radius are gsx_model_neighbors' word for word: a Gaussian participates if it passes desc->filter
 *      and its three stored coordinates are finite; d2 in float32, every operation rounded; r2 = radius * radius; i ~ j iff i != j,
 *      both participate and d2 <= r2.  The model transform, the edits and gsx_model_show_unedited change nothing.
 *      A cluster is an equivalence class of the transitive closure of ~ over the participants; a participant without a neighbour is
 *      a cluster of size 1.  out_labels[i] (nullable; the model's length) is the smallest Gaussian index of i's cluster,
 *      GSX_CLUSTER_NONE for a Gaussian that does not participate; out_sizes[i] (nullable) the size of i's cluster, 0 for one that
 *      does not participate.  stats: count participants, n_nonfinite, n_clusters, largest_size, largest_label the label of the
 *      largest cluster (the smallest such label on a tie; GSX_CLUSTER_NONE without participants), grid_bits the table used.  The same
 *      bits on every call; nothing a frame reads is written.
 *      gsx_model_select_clusters, the hit set by mode: GSX_CLUSTER_BY_SIZE participates and size_lo <= the size of its cluster <=
 *      size_hi (1 <= size_lo <= size_hi); GSX_CLUSTER_LARGEST its label is largest_label; GSX_CLUSTER_SEEDED participates and its
 *      cluster holds a seed, a participant whose selection bit was set before the call (a model without a selection has none).  In
 *      the last two modes size_lo and size_hi are 0.  *out_hit is what gsx_model_clusters with the same filter and radius implies.
 *      selection_op, a model without a selection, the tail bits, GSX_BOUNDS_SELECTED reading the selection as it was before the
 *      call, *out_hit / *out_selected (nullable), ordering and frame consistency: gsx_model_select_range's.  grid_bits: as in
 *      gsx_model_neighbors.
 *      Errors: a null viewer, key, desc or stats pointer, unknown filter bits, op or mode, flags != 0 (none are defined), a radius
 *      gsx_model_neighbors refuses, grid_bits > 24, sizes that the mode does not allow, a reserved word != 0: GSX_ERR_INVALID_ARG;
 *      unknown key: GSX_ERR_NOT_FOUND; a viewer with a communicator, or a sharded model: GSX_ERR_UNSUPPORTED; an allocation failure:
 *      GSX_ERR_OOM, the model and its selection as they were.  A model of 0 Gaussians, or 0 participants: GSX_OK with zeros (a
 *      select with Set then clears the selection). ---- */
#define GSX_CLUSTER_NONE 0xFFFFFFFFu
#define GSX_CLUSTER_BY_SIZE 0u
#define GSX_CLUSTER_LARGEST 1u
#define GSX_CLUSTER_SEEDED 2u
typedef struct gsx_cluster_desc { uint32_t filter; uint32_t flags; float radius; uint32_t grid_bits; uint32_t reserved[2]; } gsx_cluster_desc; /* 24 B */
typedef struct gsx_cluster_stats_t {
    uint64_t count; uint64_t n_nonfinite; uint64_t n_clusters; uint64_t largest_size; uint32_t largest_label; uint32_t grid_bits;
} gsx_cluster_stats_t; /* 40 B */
typedef struct gsx_cluster_select_desc {
    uint32_t filter; uint32_t flags; uint32_t selection_op; uint32_t mode; /* GSX_BOUNDS_*, 0, gsx_selection_op, GSX_CLUSTER_* */
    float radius; uint32_t size_lo; uint32_t size_hi; uint32_t grid_bits; uint32_t reserved[2];
} gsx_cluster_select_desc; /* 40 B */
void gsx_cluster_desc_default(gsx_cluster_desc* d); /* no filter, radius 1, the library's table */
gsx_status gsx_model_clusters(gsx_viewer* v, const char* key, const gsx_cluster_desc* desc, uint32_t* out_labels, uint32_t* out_sizes, gsx_cluster_stats_t* out);
gsx_status gsx_model_select_clusters(gsx_viewer* v, const char* key, const gsx_cluster_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected);

/* ---- model nearest neighbours: every Gaussian's k smallest squared distances to the others, a local-scale score from them, the
 *      score's statistics, and a selection by the score, on the device (spec/RENDER_SPEC.md §20 [BUILD-SPEC]).  The radius-free
 *      sibling of the two blocks above: stats.mean of GSX_KNN_SCORE_KTH is the radius to hand to gsx_model_neighbors and
 *      gsx_model_clusters; gsx_model_select_knn in mode GSX_KNN_SELECT_OUTLIERS is the statistical outlier removal of PCL and Open3D
 *      (mean distance to the k nearest above mean + std_ratio * std over the model), then gsx_model_extract with GSX_BOUNDS_SELECTED
 *      and GSX_EXTRACT_INVERT.  No Gaussian crosses to the host.
 *      Participants and distance are gsx_model_neighbors' word for word: a Gaussian participates if it passes desc->filter
 *      (GSX_BOUNDS_* bits) and its three stored coordinates are finite; stats.count is their number, one that passes the filter
 *      with a NaN or infinite coordinate goes to n_nonfinite.  d2(i, j) = (dx*dx + dy*dy) + dz*dz in float32, every operation
 *      rounded; model space, the stored bits as they are: the model transform, the edits and gsx_model_show_unedited change nothing.
 *      A coordinate difference that overflows gives d2 = +inf; no NaN arises from finite inputs.
 *      Rows: for a participant i let D(i) be the multiset { d2(i, j) : j participates, j != i } — self is excluded by index, not by
 *      value: coincident Gaussians are each other's neighbours at distance 0.  nn(i, q), q = 0 .. k - 1, is the q-th smallest
 *      element of D(i), ascending, +inf where D(i) has fewer than q + 1 elements; out_d2[i * k + q] (nullable; n * k floats) holds
 *      it.  A Gaussian that does not participate has a row of +inf.  Values only, no indices: ties cannot make the result
 *      ambiguous.  1 <= k <= GSX_KNN_MAX_K.
 *      Score: out_score[i] (nullable; n floats), computed on the device, +inf for a Gaussian that does not participate.
 *      GSX_KNN_SCORE_KTH: sqrtf(nn(i, k - 1)).  GSX_KNN_SCORE_MEAN: s = sqrtf(nn(i, 0)), then s = s + sqrtf(nn(i, q)) for q = 1 ..
 *      k - 1 in that ascending order, each add rounded to float32; the score is s / (float)k.  sqrtf and the division are correctly
 *      rounded.  A row that holds a +inf has an infinite score.
 *      Statistics, over the m participants with a finite score: n_scored = m; score_min and score_max exact; mean = sum / m in
 *      double; std = sqrt(sum (score - mean)^2 / (m - 1)) in double, two passes, the sample deviation (0 for m < 2); all five 0 for
 *      m = 0.  The sums are combined from per-workgroup partials in a fixed order: the same bits on every call, like everything
 *      else the call returns.
 *      gsx_model_select_knn, the hit set by mode.  GSX_KNN_SELECT_RANGE: participates and lo <= score <= hi (neither bound NaN, lo
 *      <= hi; hi may be +inf, which also takes the Gaussians with fewer than k others; std_ratio 0).  GSX_KNN_SELECT_OUTLIERS:
 *      threshold = (float)(mean + (double)std_ratio * std), the double expression without contraction, rounded to nearest; hit iff
 *      participates, m >= 1 and score > threshold, so an infinite score is an outlier; std_ratio finite; lo and hi 0.  The
 *      threshold is returned in stats.threshold, which is 0 in RANGE mode and from gsx_model_knn.  selection_op, a model without a
 *      selection, the tail bits, GSX_BOUNDS_SELECTED reading the selection as it was before the call, *out_hit / *out_selected
 *      (nullable), ordering and frame consistency: gsx_model_select_range's.
 *      Knobs that change no result: radius_hint is the first search radius (0: the library chooses it); grid_bits as in
 *      gsx_model_neighbors; max_rounds 0 for the library's own rule, or 1 .. 64 grid rounds before the exact fallback (ignored
 *      while the fallback would exceed the library's work budget).  stats.first_radius, rounds, n_brute (the Gaussians the exact
 *      fallback answered) and grid_bits report what ran and may differ with the knobs; no row, score, statistic or selection
 *      word may.
 *      Errors: a null viewer, key, desc or stats pointer of gsx_model_knn, unknown filter bits, score, mode or op, flags != 0 (none
 *      are defined), k outside 1 .. 16, a radius_hint that is negative or NaN, or positive and one gsx_model_neighbors refuses,
 *      grid_bits > 24, max_rounds > 64, bounds the mode does not allow, a reserved word != 0: GSX_ERR_INVALID_ARG; unknown key:
 *      GSX_ERR_NOT_FOUND; a viewer with a communicator, or a sharded model: GSX_ERR_UNSUPPORTED; an allocation failure:
 *      GSX_ERR_OOM, the model and its selection as they were.  A model of 0 Gaussians, or 0 participants: GSX_OK with zeros (a
 *      select with Set then clears the selection). ---- */
#define GSX_KNN_MAX_K 16u
#define GSX_KNN_SCORE_KTH 0u
#define GSX_KNN_SCORE_MEAN 1u
#define GSX_KNN_SELECT_RANGE 0u
#define GSX_KNN_SELECT_OUTLIERS 1u
typedef struct gsx_knn_desc { uint32_t filter; uint32_t flags; uint32_t k; uint32_t score; float radius_hint; uint32_t grid_bits; uint32_t max_rounds; uint32_t reserved; } gsx_knn_desc; /* 32 B */
typedef struct gsx_knn_stats_t {
    uint64_t count; uint64_t n_nonfinite; uint64_t n_scored; uint64_t n_brute; double mean; double std;
    float score_min; float score_max; float first_radius; float threshold; uint32_t rounds; uint32_t grid_bits;
} gsx_knn_stats_t; /* 72 B */
typedef struct gsx_knn_select_desc {
    uint32_t filter; uint32_t flags; uint32_t selection_op; uint32_t mode; /* GSX_BOUNDS_*, 0, gsx_selection_op, GSX_KNN_SELECT_* */
    uint32_t k; uint32_t score; float radius_hint; uint32_t grid_bits;
    uint32_t max_rounds; float lo; float hi; float std_ratio;
} gsx_knn_select_desc; /* 48 B */
void gsx_knn_desc_default(gsx_knn_desc* d); /* no filter, k 3, SCORE_MEAN, everything else 0 */
gsx_status gsx_model_knn(gsx_viewer* v, const char* key, const gsx_knn_desc* desc, float* out_d2 /* nullable, n * k, row i at i * k */,
                         float* out_score /* nullable, n */, gsx_knn_stats_t* out);
gsx_status gsx_model_select_knn(gsx_viewer* v, const char* key, const gsx_knn_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected,
                                gsx_knn_stats_t* out_stats /* nullable */);

/* ---- model nearest, across models: for every Gaussian of a source model the nearest Gaussian of a target model, its index and
 *      squared distance, the one-sided chamfer and Hausdorff distances, a selection by them, and one least-squares registration
 *      step, on the device (spec/RENDER_SPEC.md §23 [BUILD-SPEC]).  What two captures of one scene, or a model and its decimated or
 *      converted copy, need: the overlap before a gsx_model_merge, a selection carried from one model to the other, how far a
 *      decimated model is from its source, one capture registered onto another.  No Gaussian crosses to the host.
 *      Participants: a target (a Gaussian of dst_key) participates if it passes desc->dst_filter (GSX_BOUNDS_* bits) and its three
 *      stored coordinates are finite: gsx_model_neighbors' rule.  A query (a Gaussian of src_key) participates if it passes
 *      desc->src_filter, its stored coordinates are finite and its mapped position q is finite.  stats.count and stats.targets are
 *      their numbers; what passes a filter and fails the finiteness test goes to n_nonfinite and targets_nonfinite.
 *      Mapping: desc->xform is a row-major 3x4 float32 matrix from the source's model space into the targets'; per row
 *      q_r = ((m_r0*x + m_r1*y) + m_r2*z) + m_r3, every operation rounded to float32.  With GSX_NEAREST_MODEL_TRANSFORMS in
 *      desc->flags desc->xform is ignored: the matrix is inv(M_dst) * M_src of the two models' current gsx_update_model_transform
 *      values, M = T R S as in gsx_model_merge, the quaternions normalised, computed in double and rounded to float32 once; a
 *      target scale component of 0 is GSX_ERR_INVALID_ARG.  Either way stats.xform returns the matrix used.
 *      Answer: d2(q, t) = (dx*dx + dy*dy) + dz*dz in float32, gsx_model_neighbors' distance, in the targets' model space.
 *      out_d2[i] (nullable; the source's length) is the smallest d2 over the participating targets that are in reach, out_index[i]
 *      (nullable) the target's index, among equal d2 the smallest index.  In reach: d2 <= fl(max_distance * max_distance), or, with
 *      max_distance 0 (unlimited), d2 finite.  GSX_NEAREST_NONE and +inf for a query that does not participate or has no target in
 *      reach.  src_key may equal dst_key; nothing is excluded by index (with disjoint filters: from the selection to the rest).
 *      Statistics over the found queries: n_found; d_min and d_max = sqrtf of the least and the largest d2 (d_max: the one-sided
 *      Hausdorff distance); mean = sum sqrtf(d2) / n_found (the one-sided chamfer distance) and rms = sqrt(sum d2 / n_found) in
 *      double, the sums combined from per-workgroup partials in index order: the same bits on every call; all 0 for n_found = 0.
 *      Cost: max_distance bounds it.  Without it a query far from every target is asked again at four times the radius until the
 *      grid is coarse and then costs one pass over all targets in the exact fallback (stats.n_brute), as a far point of
 *      gsx_model_knn does; with it the last grid round runs at max_distance and what it leaves is "none".  While the unresolved
 *      times the targets exceed the fallback's budget of 2^37 distance tests the rounds go on instead, on grids whose cells hold
 *      ever more targets: millions of queries beyond the targets' box cost on the order of queries x targets distance tests.
 *      Set max_distance for such a pair of models.
 *      Knobs that change no result: radius_hint, grid_bits and max_rounds as in gsx_knn_desc (the table is over the targets);
 *      stats.first_radius, rounds, n_brute and grid_bits report what ran.
 *      gsx_model_select_nearest writes the SOURCE's selection.  GSX_NEAREST_SELECT_RANGE: the query participates and lo <=
 *      sqrtf(d2) <= hi (lo <= hi, neither NaN; hi = +inf also takes the participants for which nothing was found).
 *      GSX_NEAREST_SELECT_TRANSFER: a target was found and it is selected in dst_key as the call begins (a target model without a
 *      selection: no hits; lo and hi 0).  selection_op, a model without a selection, the tail bits, GSX_BOUNDS_SELECTED reading the
 *      selection as it was before the call (also where src_key equals dst_key), *out_hit / *out_selected (nullable), ordering and
 *      frame consistency: gsx_model_select_range's.  gsx_model_nearest and gsx_model_align_step write nothing a frame reads.
 *      gsx_model_align_step: one step of point-to-point registration; the iteration is the caller's loop.  The search above with
 *      desc->nearest (its max_distance rejects correspondences), then over the found pairs (q, t), in double and in index order:
 *      their number and means, and about the means rounded to float32 the products of the float32 differences: H = sum (q - qm)
 *      (t - tm)^T, sum |q - qm|^2, sum d2.  The host solves for the similarity t ~ s R q + p: the unit quaternion (x, y, z, w;
 *      w >= 0) is the dominant eigenvector of Horn's 4x4 matrix of H; with GSX_ALIGN_SCALE s = sum (t - tm) . R (q - qm) /
 *      sum |q - qm|^2, otherwise 1; p = tm - s R qm.  out->pos, quat, scale: that delta, in double, in the targets' model space; xform_next =
 *      delta o xform, composed in double and rounded once: the next step's desc->nearest.xform; n_pairs; rms_before = sqrt(sum d2 /
 *      n_pairs); nearest: the search's statistics.  Fewer than 3 pairs, no spread among the q, or pairs that determine no single
 *      rotation (all on one line): GSX_OK, out->degenerate = 1, the identity delta and xform_next = the matrix used.
 *      Errors: a null viewer, key, desc or stats / out pointer (out_stats of the select is nullable), unknown filter, flag, mode or
 *      op bits, a max_distance that is not 0 and one gsx_model_neighbors refuses as a radius, a radius_hint that is negative or NaN
 *      or positive and refused, grid_bits > 24, max_rounds > 64, a matrix entry that is not finite, bounds the mode does not allow,
 *      a reserved word != 0: GSX_ERR_INVALID_ARG; an unknown src_key or dst_key: GSX_ERR_NOT_FOUND; a viewer with a communicator,
 *      or a sharded model: GSX_ERR_UNSUPPORTED; an allocation failure: GSX_ERR_OOM, both models as they were.  No queries or no
 *      targets: GSX_OK with zeros and rows of GSX_NEAREST_NONE / +inf (a select with Set then clears the selection). ---- */
#define GSX_NEAREST_NONE 0xFFFFFFFFu
#define GSX_NEAREST_MODEL_TRANSFORMS 1u
#define GSX_NEAREST_SELECT_RANGE 0u
#define GSX_NEAREST_SELECT_TRANSFER 1u
#define GSX_ALIGN_SCALE 1u
typedef struct gsx_nearest_desc {
    uint32_t src_filter; uint32_t dst_filter; uint32_t flags; uint32_t grid_bits; /* GSX_BOUNDS_* twice, GSX_NEAREST_MODEL_TRANSFORMS */
    float max_distance; float radius_hint; uint32_t max_rounds; uint32_t reserved;
    float xform[12];
} gsx_nearest_desc; /* 80 B */
typedef struct gsx_nearest_stats_t {
    uint64_t count; uint64_t n_nonfinite; uint64_t targets; uint64_t targets_nonfinite; uint64_t n_found; uint64_t n_brute;
    double mean; double rms;
    float d_min; float d_max; float first_radius; uint32_t rounds; uint32_t grid_bits; uint32_t reserved;
    float xform[12];
} gsx_nearest_stats_t; /* 136 B */
typedef struct gsx_nearest_select_desc {
    gsx_nearest_desc nearest;
    uint32_t selection_op; uint32_t mode; float lo; float hi; /* gsx_selection_op, GSX_NEAREST_SELECT_* */
} gsx_nearest_select_desc; /* 96 B */
typedef struct gsx_align_desc { gsx_nearest_desc nearest; uint32_t flags; uint32_t reserved; } gsx_align_desc; /* 88 B; flags: GSX_ALIGN_SCALE */
typedef struct gsx_align_step_t {
    double pos[3]; double quat[4]; double scale;
    float xform_next[12];
    uint64_t n_pairs; double rms_before;
    uint32_t degenerate; uint32_t reserved;
    gsx_nearest_stats_t nearest;
} gsx_align_step_t; /* 272 B */
void gsx_nearest_desc_default(gsx_nearest_desc* d); /* no filters, no flags, unlimited, the identity matrix, everything else 0 */
gsx_status gsx_model_nearest(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_nearest_desc* desc,
                             uint32_t* out_index /* nullable, the source's length */, float* out_d2 /* nullable, the source's length */,
                             gsx_nearest_stats_t* out);
gsx_status gsx_model_select_nearest(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_nearest_select_desc* desc, uint64_t* out_hit,
                                    uint64_t* out_selected, gsx_nearest_stats_t* out_stats /* nullable */);
gsx_status gsx_model_align_step(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_align_desc* desc, gsx_align_step_t* out);

/* ---- model transform: move, rotate, scale or mirror the kept Gaussians of a resident model where they lie, on the device
 *      (spec/RENDER_SPEC.md §21 [BUILD-SPEC]).  The edit behind "grab the selection and move it": no copy of the model, the Gaussian
 *      order, every index, the mask, the selection and the edit records stay.  gsx_update_model_transform moves a whole model
 *      without touching its data; this call bakes a transform into part of it.
 *      Kept set: gsx_model_extract's, word for word (desc->filter GSX_BOUNDS_* bits, desc->flags GSX_EXTRACT_INVERT; no mask: all
 *      pass; GSX_BOUNDS_SELECTED without a selection: none passes; bits at or above the count never count, before or after
 *      inversion).  A kept Gaussian is rewritten at its own index; every byte of every other Gaussian stays.  *out_count
 *      (nullable) receives the kept count.
 *      Position: with c = pivot, q = p - c per axis, a = scale * q and R the float32 matrix of the quaternion AS GIVEN (what a
 *      model transform's quaternion becomes in a frame): p'_r = (((R_r0 a0 + R_r1 a1) + R_r2 a2) + pos_r) + c_r, every operation
 *      rounded to float32, no contraction.  With a pivot that is exactly (0, 0, 0) the subtraction and the last addition are not
 *      performed: p' is then what gsx_model_merge bakes for that model transform, bit for bit.  A non-finite coordinate goes
 *      through the same formula.
 *      Covariance and SH: gsx_model_merge's bake (S' = (M S) M^T with M = R diag(scale); per band c' = M_l c with the matrices of
 *      the normalised quaternion), dequantised exactly and quantised again into the model's pod kind; neither depends on the
 *      pivot; the colour word is carried.  Every call that rewrites a quantised plane quantises it again: with Half or Norm8
 *      planes, n calls are not one call with the composed transform.
 *      Planes that are carried as stored bits: the SH planes under quat (0, 0, 0, +-1) (as float32 values); the covariance planes
 *      too when scale is also (1, 1, 1) — a translation writes positions only, which is what makes moving a Half or Norm8 model
 *      lossless; and with pos 0 as well (the identity) nothing is written at all, whatever the pivot, and no frame state is reset.
 *      A quaternion that is the identity only after normalisation, (0, 0, 0, 2), is not the identity: every plane is rewritten.
 *      The shade records of the kept Gaussians agree with the planes afterwards.  Not touched: the model transform, the mask and
 *      selection words (a mask evaluated from shapes is not evaluated again: the bits stay, the positions moved), the edit records,
 *      gsx_model_show_unedited, the pod kind.  Runs on the viewer's stream behind every frame in flight; the next frames are
 *      ordered behind it.  The same bits on every call.  No shear, no general matrix.
 *      Errors: a null viewer, key or desc, unknown filter bits, a flag other than GSX_EXTRACT_INVERT, a non-finite pos, quat,
 *      scale or pivot component, a zero quaternion, reserved != 0: GSX_ERR_INVALID_ARG; unknown key: GSX_ERR_NOT_FOUND; a viewer
 *      with a communicator, or a sharded model: GSX_ERR_UNSUPPORTED; an allocation failure: GSX_ERR_OOM, the model as it was.  A
 *      model of 0 Gaussians or an empty kept set: GSX_OK, count 0, nothing written. ---- */
typedef struct gsx_transform_desc {
    uint32_t filter; uint32_t flags;                 /* GSX_BOUNDS_*, GSX_EXTRACT_INVERT */
    float pos[3]; float quat[4]; float scale[3];     /* as gsx_update_model_transform takes them; quat x, y, z, w */
    float pivot[3]; uint32_t reserved;               /* rotate and scale about this point (model space); 0 */
} gsx_transform_desc; /* 64 B */
void gsx_transform_desc_default(gsx_transform_desc* d); /* no filter, no flags, pos 0, quat (0, 0, 0, 1), scale 1, pivot 0 */
gsx_status gsx_model_apply_transform(gsx_viewer* v, const char* key, const gsx_transform_desc* desc, uint64_t* out_count /* nullable */);

/* ---- model decimate: reduce a resident model's Gaussian count on the device (spec/RENDER_SPEC.md §22 [BUILD-SPEC]).  The
 *      Gaussians that share a cell of a uniform grid of edge desc->cell become ONE moment-matched Gaussian of a new model: 10 M down
 *      to 1 M for a web export, a coarse stand-in for a far model, a merged scene whose overlap holds everything twice.  No Gaussian
 *      crosses to the host.
 *      Participants: a Gaussian participates if it passes desc->filter / desc->flags (GSX_BOUNDS_* bits and GSX_EXTRACT_INVERT,
 *      gsx_model_extract's meaning word for word: no mask = all pass, no selection = none pass, tail bits never count) and its three
 *      stored coordinates are finite; stats.count is their number, stats.n_nonfinite the kept Gaussians with a NaN or infinite
 *      coordinate, which are dropped.
 *      Cells: gsx_model_neighbors' grid with the edge given: origin = the participants' minimum per axis, inv_h = 1 / cell in float32,
 *      a coordinate's cell min(floor((x - origin) * inv_h), 32767) in float32: cells beyond 32767 on an axis are joined.
 *      dst: one Gaussian per occupied cell.  A cell's representative is its member with the smallest index; dst holds the cells in
 *      ascending order of representative.  stats.cells = dst's length, stats.singletons the one-member cells, stats.largest_cell the
 *      largest member count.  out_map[i] (nullable; the model's length) = the dst index Gaussian i went into, 0xFFFFFFFF if it does not
 *      participate.  A one-member cell is copied as stored bits (a cell so small that every cell has one member IS gsx_model_extract of
 *      the participants with GSX_EXTRACT_DROP_EDITS).  A cell of two members and more: mean and covariance of the mixture weighted by
 *      alpha * sqrt(det Sigma) (weight 1 for every member when that sum is not positive and finite), opacity conserving that mass
 *      (at most 1), colour and SH the weighted means; float32, members in ascending index, quantised once into src's pod kind; the
 *      same bits on every call.  dst has src's pod kind and model transform, no mask, no selection and no edit records (members'
 *      edits cannot be averaged: exclude hidden Gaussians with GSX_BOUNDS_SKIP_HIDDEN).  src is not written.
 *      dst_key NULL: count only: stats and out_map are filled, no model is made.  No participants: GSX_OK, cells 0, no model.
 *      grid_bits: gsx_model_neighbors'.  Ordering: gsx_model_extract's; the call waits once, for the cell count.
 *      gsx_model_decimate_edge: an edge for a target count, by 20 count-only bisection steps on log2(edge) between extent / 32767 and
 *      extent * (1 + 2^-5) (one cell), extent the participants' largest axis extent: *out_cell = the smallest probed edge with at most
 *      target_cells cells, *out_cells that count (the count is not strictly monotone in the edge: only this rule is promised).  An
 *      extent of 0: edge 1, one cell.  No participants: edge 0, 0 cells.
 *      Cost at coarse edges: a bucket of more than 2048 records is ordered by ONE workgroup and a cell is reduced by ONE wave, members
 *      in order, so the time grows with the largest cell: 10 M Gaussians into about 1 k cells take 44 to 50 ms, and an edge that puts a
 *      model of millions into one or a few cells runs for seconds inside a single kernel (it is not a hang, and it is not measured).
 *      gsx_model_decimate_edge with a target of a few cells on a large model converges towards such edges and repeats that count up to
 *      20 times: for tiny targets choose the edge from gsx_model_bounds instead.
 *      Errors: a null viewer, src_key / key, desc or out pointer, unknown filter bits, a flag other than GSX_EXTRACT_INVERT, a cell
 *      that is not finite and above 0 or whose float32 reciprocal is 0 or inf, grid_bits > 24, a reserved word != 0, a dst_key that
 *      exists or equals src_key, target_cells 0: GSX_ERR_INVALID_ARG; unknown src: GSX_ERR_NOT_FOUND; a viewer with a communicator,
 *      or a sharded model: GSX_ERR_UNSUPPORTED; an allocation failure: GSX_ERR_OOM, no dst left behind. ---- */
typedef struct gsx_decimate_desc { uint32_t filter; uint32_t flags; float cell; uint32_t grid_bits; uint32_t reserved[2]; } gsx_decimate_desc; /* 24 B */
typedef struct gsx_decimate_stats_t { uint64_t count; uint64_t n_nonfinite; uint64_t cells; uint64_t singletons; uint32_t largest_cell; uint32_t grid_bits; } gsx_decimate_stats_t; /* 40 B */
void gsx_decimate_desc_default(gsx_decimate_desc* d); /* filter 0, flags 0, cell 0 (must be set), grid_bits 0 = the library's */
gsx_status gsx_model_decimate(gsx_viewer* v, const char* src_key, const char* dst_key /* NULL: count only */, const gsx_decimate_desc* desc,
                              uint32_t* out_map /* nullable, n words */, gsx_decimate_stats_t* out);
gsx_status gsx_model_decimate_edge(gsx_viewer* v, const char* key, uint32_t filter, uint32_t flags, uint64_t target_cells,
                                   float* out_cell, uint64_t* out_cells);

/* ---- visibility: which Gaussians the camera sees, and how much (spec/RENDER_SPEC.md section 24; kernels_visibility.hip).
 *      gsx_model_visibility draws the model ALONE — what gsx_render_frame(&key, 1) would draw: the viewer's current camera,
 *      viewport, model transform, Gaussian transform and spec parameters; the mask, the hidden edits, the opacity edits and
 *      show_unedited as in a frame — and keeps, per Gaussian, what the compositor computes and throws away.  Pixel p walks its tile's
 *      front-to-back list with the compositor's per-pixel sequence (support test, alpha by display mode clamped by alpha_max /
 *      alpha_min, w = T * alpha in float32, T *= 1 - alpha, closed at T < t_epsilon; records behind a closed pixel get nothing):
 *        peak   = max over pixels of w;
 *        weight = sum over pixels of round_to_nearest(w * 2^24), a 64-bit integer, reported as double / 2^24;
 *        pixels = the pixels that blended the Gaussian (support hit, pixel open, alpha not removed by alpha_min).
 *      A maximum and integer sums: two calls return the same bytes, whatever ran before and however many frames are in flight.
 *      out_transmittance: the final T of every pixel of this view (height * width floats, row-major).
 *      The planes: 16 bytes a Gaussian, owned by the model, allocated by the first call, counted by gsx_debug_device_bytes, freed
 *      by gsx_model_visibility_reset and gsx_model_remove, and dropped by every call that rewrites the model's pod planes or its
 *      count (the uploads, gsx_model_import_ply, gsx_model_apply_transform unless the identity, gsx_model_convert / set_pod_kind).
 *      A mask, selection or edit change KEEPS them: the planes describe the views that were folded, not the model as it is now.
 *      Without GSX_VIS_ACCUMULATE a call replaces the planes (views = 1); with it peak becomes the maximum, weight and pixels the
 *      sums, views + 1; the viewport may differ from view to view; (views + 1) * width * height >= 2^32 is refused (the pixel
 *      plane would wrap).
 *      gsx_model_select_visibility: selects the Gaussians that pass `filter` (GSX_BOUNDS_* bits) and whose resident measure lies in
 *      [lo, hi] (inclusive; hi = +inf allowed) under `selection_op`; "never seen" is GSX_VIS_PEAK in [0, 0].
 *      State: the call is ordered after every frame in flight, draws into scratch of its own (the viewer's framebuffer, every
 *      lane's and the query hit buffers keep the last frame), and leaves the model unsorted: gsx_preprocess + gsx_sort before the
 *      next gsx_render (which refuses otherwise); gsx_render_frame needs nothing, and draws bit for bit the frame it would have
 *      drawn without the call.
 *      Out of scope (GSX_ERR_INVALID_ARG, by design, not forgotten): the depth test GSX_DEPTH_LESS; overlay lines or mask gizmos
 *      set; a band (gsx_viewer_set_band) or an external framebuffer set; a sharded model.
 *      Other errors: null viewer / key / desc, unknown flag bits, a reserved word != 0, an unknown measure or op, a NaN or reversed
 *      range, a select or a download without planes: GSX_ERR_INVALID_ARG; unknown key: GSX_ERR_NOT_FOUND.  A refused call leaves the
 *      planes untouched. ---- */
#define GSX_VIS_ACCUMULATE 1u   /* fold this view into the model's resident planes instead of replacing them */
typedef enum gsx_visibility_measure { GSX_VIS_PEAK = 0, GSX_VIS_WEIGHT = 1, GSX_VIS_PIXELS = 2 } gsx_visibility_measure;
typedef struct gsx_visibility_desc { uint32_t flags; uint32_t reserved[3]; } gsx_visibility_desc; /* 16 B */
typedef struct gsx_visibility_select_desc {
    uint32_t measure;       /* gsx_visibility_measure */
    uint32_t filter;        /* GSX_BOUNDS_* bits */
    uint32_t selection_op;  /* GSX_SELECTION_SET / _ADD / _REMOVE */
    uint32_t reserved;      /* 0 */
    double lo, hi;          /* inclusive */
} gsx_visibility_select_desc; /* 32 B */
typedef struct gsx_visibility_stats_t {
    uint64_t n_visible;     /* after cull, this view */
    uint64_t n_seen;        /* Gaussians with peak > 0 in the resident planes after this call */
    uint64_t n_pairs;       /* (pixel, Gaussian) pairs blended in this view */
    uint64_t weight_fixed;  /* sum over this view's pairs of the 2^-24 fixed-point weights */
    float peak_max;         /* largest resident peak */
    uint32_t views;         /* views folded into the planes */
} gsx_visibility_stats_t; /* 40 B */
void gsx_visibility_desc_default(gsx_visibility_desc* d);               /* flags 0 */
void gsx_visibility_select_desc_default(gsx_visibility_select_desc* d); /* PEAK in (0, +inf]: lo = the smallest positive float, SET, no filter */
gsx_status gsx_model_visibility(gsx_viewer* v, const char* key, const gsx_visibility_desc* desc, float* out_peak /* n, nullable */,
                                double* out_weight /* n, nullable */, uint32_t* out_pixels /* n, nullable */,
                                float* out_transmittance /* height * width of this view, nullable */, gsx_visibility_stats_t* out /* nullable */);
gsx_status gsx_model_select_visibility(gsx_viewer* v, const char* key, const gsx_visibility_select_desc* desc, uint64_t* out_hit,
                                       uint64_t* out_selected);
gsx_status gsx_model_visibility_reset(gsx_viewer* v, const char* key); /* frees the planes */

/* ---- depth map: the splats' depth per pixel (spec/RENDER_SPEC.md section 25; kernels_depthmap.hip).
 *      gsx_render_depth_map walks the models of `keys_far_to_near` in the order gsx_render_frame composites them — the LAST key
 *      first — with the viewer's current camera, viewport, transforms and spec parameters, the mask and the edits as in a frame.
 *      Pixel p walks each model's complete front-to-back tile list with the compositor's per-pixel sequence (support test, alpha by
 *      display mode clamped by alpha_max / alpha_min, w = T * alpha in float32, T *= 1 - alpha, closed at T < t_epsilon; records
 *      behind a closed pixel add nothing); T is carried from model to model.  d is a Gaussian's view depth: the float whose bits are
 *      its depth key.  Per pixel, height * width values a plane, row-major, row 0 at the top:
 *        transmittance  the final T: the T channel of gsx_render_frame over the same keys, bit for bit;
 *        alpha          A = sum of w (A <- A + w), and
 *        sum            S = sum of w * d (S <- fma(w, d, S)), both float32 in walk order; the expected depth is S / A, left to the
 *                       caller — the library makes no division;
 *        surface        d of the first record after whose blend T < desc.threshold (0.5: the median depth; 1.0: the first record
 *                       that lowers T at all), +inf without such a crossing;
 *        index, layer   that record's Gaussian index and its model's position in `keys_far_to_near`; 0xFFFFFFFF without a crossing;
 *        ndc            only with GSX_DEPTH_MAP_NDC: clamp(P23 / surface - P22, 0, 1) in float32, 1.0 without a crossing — the
 *                       depth test's own relation (gsx_viewer_set_depth_test) read backwards.  The flag needs the projection the
 *                       depth test needs.  A splat lying on the surface itself may pass or fail a later test: parity in that band
 *                       of a few ulps is not pinned, as for the depth test.
 *      The statistics are integers and bit patterns: two calls return the same bytes in every plane and in the statistics,
 *      whatever ran before and however many frames are in flight.  Without a crossing surface_min = +inf and surface_max = 0.
 *      The planes are device memory of the viewer (counted by gsx_debug_device_bytes); gsx_depth_map_device_ptrs returns them.  They
 *      stay valid until the next gsx_render_depth_map, a viewport change or gsx_viewer_destroy; `ndc` is NULL unless the last call
 *      set the flag.  The ndc plane is tightly packed [height][width] float32 and can be handed straight to
 *      gsx_viewer_set_depth_buffer_device(v, ndc, width, height, 4 * width).  Ordering: the call's writes are made on the viewer's
 *      stream and are complete when it returns; a frame dealt afterwards — on the viewer or on a lane — reads behind them.
 *      State: the call is ordered after every frame in flight, draws into scratch of its own (the viewer's framebuffer, every
 *      lane's and the query hit buffers keep the last frame), and leaves every model named unsorted: gsx_preprocess + gsx_sort
 *      before the next gsx_render (which refuses otherwise); gsx_render_frame needs nothing, and draws bit for bit the frame it
 *      would have drawn without the call.
 *      Out of scope (GSX_ERR_INVALID_ARG, by design, not forgotten): the depth test GSX_DEPTH_LESS; overlay lines or mask gizmos
 *      set; a band (gsx_viewer_set_band) or an external framebuffer set; a sharded model or a viewer with a communicator.
 *      Other errors: null viewer / keys / desc, n_keys == 0, a key named twice, unknown flag bits, a reserved word != 0, a threshold
 *      that is not finite or outside [t_epsilon, 1], GSX_DEPTH_MAP_NDC with another projection, device pointers without a depth map
 *      of this viewport: GSX_ERR_INVALID_ARG; unknown key: GSX_ERR_NOT_FOUND.  A refused call leaves the planes as they were.
 *      gsx_depth_map_unproject (host only, float64 inside): the world-space point that the camera (view, proj: column-major, as
 *      gsx_update_camera takes them) sees at pixel position (px, py) — pixel (i, j) has its centre at (i + 0.5, j + 0.5) — at
 *      view depth `view_depth` (a value of the surface plane, or S / A). ---- */
#define GSX_DEPTH_MAP_NDC 1u   /* also write the ndc plane */
typedef struct gsx_depth_map_desc { uint32_t flags; float threshold; uint32_t reserved[2]; } gsx_depth_map_desc; /* 16 B */
typedef struct gsx_depth_map_stats_t { uint64_t n_covered, n_crossed; float surface_min, surface_max; uint32_t models, reserved; } gsx_depth_map_stats_t; /* 32 B */
void gsx_depth_map_desc_default(gsx_depth_map_desc* d); /* flags 0, threshold 0.5 */
gsx_status gsx_render_depth_map(gsx_viewer* v, const char* const* keys_far_to_near, uint32_t n_keys, const gsx_depth_map_desc* desc,
                                float* out_surface, float* out_sum, float* out_alpha, float* out_transmittance,
                                uint32_t* out_index, uint32_t* out_layer, gsx_depth_map_stats_t* out); /* every out_* nullable, height * width */
gsx_status gsx_depth_map_device_ptrs(gsx_viewer* v, void** surface, void** sum, void** alpha, void** transmittance,
                                     void** index, void** layer, void** ndc, uint32_t* width, uint32_t* height); /* every out nullable */
gsx_status gsx_depth_map_unproject(const float view[16], const float proj[16], uint32_t width, uint32_t height,
                                   float px, float py, float view_depth, float out_world[3]);

/* ---- model normals: a plane fitted to every Gaussian and its k nearest, the plane's unit normal, how far the neighbourhood is from
 *      a plane, the neighbours' indices, and a selection by either, on the device (spec/RENDER_SPEC.md §26 [BUILD-SPEC];
 *      kernels_normals.hip).  Selecting the floor: gsx_model_select_normals in mode GSX_NORMALS_SELECT_FACING with dir = up,
 *      GSX_NORMALS_ABS, lo 0.95, hi 1; dropping what floats: mode GSX_NORMALS_SELECT_VARIATION.  No Gaussian crosses to the host.
 *      Participants, distance and space are gsx_model_knn's word for word (the filter, three finite stored coordinates, the float32
 *      d2, model space).  GSX_NORMALS_MIN_K <= k <= GSX_NORMALS_MAX_K.
 *      Neighbour list: N(i) is the k smallest elements of { (d2(i, j), j) : j participates, j != i }, ordered by d2, then by index.
 *      out_index[i * k + q] (nullable; n * k words) is the q-th element's index, GSX_NORMALS_NONE where the set has fewer than
 *      q + 1 elements or the distance is +inf, and in the whole row of a Gaussian that does not participate.  The list's d2 are
 *      gsx_model_knn's row for the same k bit for bit; with the index in the order, ties cannot make the list ambiguous.
 *      Fitted: a participant whose k entries all have a finite d2 and whose k-th d2 is above 0.  Everybody else has the normal
 *      (0, 0, 0) and the variation +inf.
 *      The fit, in double: offsets q_0 = 0 (the Gaussian itself) and q_m = the float32 difference p_j - p_i per axis, m = 1 .. k in
 *      list order; mean = (sum q_m) / (k + 1); scatter C_ab = sum (q_ma - mean_a)(q_mb - mean_b); both sums in ascending m without
 *      contraction; the eigenvalues l0 >= l1 >= l2 and vectors of C by §14's fixed-sweep Jacobi solve in double, the eigenvalues
 *      clamped at 0; ((l0 + l1) + l2) that is 0 or not finite: not fitted.  out_normal[i * 3 ..] (nullable) is the eigenvector of
 *      l2 over its length, rounded to float32; out_variation[i] (nullable) = (float)(l2 / ((l0 + l1) + l2)), in [0, 1/3]: 0 on a
 *      plane, 1/3 where the neighbourhood is isotropic.  The sums follow the list, so no grid can change a bit of the fit.
 *      Sign.  GSX_NORMALS_ORIENT_CANONICAL: the first non-zero component of the float32 normal is positive.
 *      GSX_NORMALS_ORIENT_TOWARD: toward[3] is a finite model-space point; the normal is negated iff sum_a n_a * ((double)toward_a -
 *      (double)p_ia) < 0, the float32 normal in double, in axis order; a sum of exactly 0 falls back to the canonical rule.
 *      Statistics over the fitted: n_fitted, variation_min and variation_max exact, mean = the double sum of the float32 variations
 *      over n_fitted, folded from per-workgroup partials in index order: the same bits on every call; all 0 without any.
 *      gsx_model_select_normals, the hit set by mode.  GSX_NORMALS_SELECT_VARIATION: fitted and lo <= variation <= hi.
 *      GSX_NORMALS_SELECT_FACING: dir[3] finite and not zero, normalised in double and rounded to float32 d; c = (nx dx + ny dy) +
 *      nz dz in float32, every operation rounded; |c| with the flag GSX_NORMALS_ABS; hit iff fitted and lo <= c <= hi.  lo <= hi,
 *      neither NaN.  selection_op, a model without a selection, the tail bits, GSX_BOUNDS_SELECTED reading the selection as it
 *      was before the call, *out_hit / *out_selected (nullable), ordering and frame consistency: gsx_model_select_knn's.
 *      Knobs that change no result: radius_hint, grid_bits, max_rounds, as in gsx_knn_desc.  stats.first_radius, rounds, n_brute
 *      and grid_bits report what ran; no list entry, normal, variation, statistic or selection word depends on them.
 *      Errors: a null viewer, key, desc or stats pointer of gsx_model_normals, unknown filter or flag bits, k outside 3 .. 16, an
 *      unknown orient, mode or op, a toward (orient TOWARD) or a bound that is not finite (a bound may be infinite, not NaN), a dir
 *      (mode FACING) that is zero or not finite, lo > hi, a radius_hint, grid_bits or max_rounds gsx_model_knn refuses, a reserved
 *      word != 0: GSX_ERR_INVALID_ARG; unknown key: GSX_ERR_NOT_FOUND; a viewer with a communicator, or a sharded model:
 *      GSX_ERR_UNSUPPORTED; an allocation failure: GSX_ERR_OOM, the model and its selection as they were.  A model of 0 Gaussians,
 *      or 0 participants: GSX_OK with zeros.  gsx_model_normals writes nothing a frame reads. ---- */
#define GSX_NORMALS_MIN_K 3u
#define GSX_NORMALS_MAX_K 16u
#define GSX_NORMALS_ORIENT_CANONICAL 0u
#define GSX_NORMALS_ORIENT_TOWARD 1u
#define GSX_NORMALS_SELECT_VARIATION 0u
#define GSX_NORMALS_SELECT_FACING 1u
#define GSX_NORMALS_ABS 1u            /* gsx_normals_select_desc.flags: mode FACING tests |c| */
#define GSX_NORMALS_NONE 0xFFFFFFFFu  /* out_index: no such neighbour */
typedef struct gsx_normals_desc {
    uint32_t filter; uint32_t flags; uint32_t k; uint32_t orient; /* GSX_BOUNDS_*, 0, 3 .. 16, GSX_NORMALS_ORIENT_* */
    float radius_hint; uint32_t grid_bits; uint32_t max_rounds; uint32_t reserved;
    float toward[3]; uint32_t reserved2;
} gsx_normals_desc; /* 48 B */
typedef struct gsx_normals_stats_t {
    uint64_t count; uint64_t n_nonfinite; uint64_t n_fitted; uint64_t n_brute; double mean;
    float variation_min; float variation_max; float first_radius; uint32_t rounds; uint32_t grid_bits; uint32_t reserved;
} gsx_normals_stats_t; /* 64 B */
typedef struct gsx_normals_select_desc {
    uint32_t filter; uint32_t flags; uint32_t selection_op; uint32_t mode; /* GSX_BOUNDS_*, GSX_NORMALS_ABS, gsx_selection_op, GSX_NORMALS_SELECT_* */
    uint32_t k; uint32_t orient; float radius_hint; uint32_t grid_bits;
    uint32_t max_rounds; float lo; float hi; uint32_t reserved;
    float dir[3]; float toward[3]; uint32_t reserved2[2];
} gsx_normals_select_desc; /* 80 B */
void gsx_normals_desc_default(gsx_normals_desc* d); /* no filter, flags 0, k 8, ORIENT_CANONICAL, everything else 0 */
gsx_status gsx_model_normals(gsx_viewer* v, const char* key, const gsx_normals_desc* desc, float* out_normal /* nullable, n * 3 */,
                             float* out_variation /* nullable, n */, uint32_t* out_index /* nullable, n * k, row i at i * k */,
                             gsx_normals_stats_t* out);
gsx_status gsx_model_select_normals(gsx_viewer* v, const char* key, const gsx_normals_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected,
                                    gsx_normals_stats_t* out_stats /* nullable */);

/* ---- point-to-plane registration: a model's normals kept on the device, and one Gauss-Newton step that registers a source model
 *      onto a target model's kept planes (spec/RENDER_SPEC.md §27 [BUILD-SPEC]; kernels_nearest.hip, csrc/align_plane_math.h).  Two
 *      captures of one surface are never the same samples: a point-to-point step (gsx_model_align_step) pulls every sample towards
 *      another sample and crawls; the plane step lets a sample slide along the target's surface and says which motions the pairs
 *      determine.  The iteration is the caller's loop, as for gsx_model_align_step.
 *      Kept normals.  gsx_model_normals_keep runs gsx_model_normals' computation (§26: the same desc, the same checks, the same
 *      kernels) and keeps the 16 bytes a Gaussian it produces — the float32 normal and the variation; (0, 0, 0) and +inf where no
 *      plane was fitted — resident with the model, as the visibility planes are.  A second keep replaces the first.
 *      gsx_model_normals_kept reports the plane (present, the k, orient, filter and toward it was made with, the model's count and
 *      n_fitted) and copies it out (out_normal, out_variation: nullable); without a plane it is GSX_OK with present = 0 and the
 *      arrays untouched.  gsx_model_normals_reset frees it.  The plane describes the stored positions it was fitted on: an upload, a
 *      device upload, an import, a transform that moves something and a pod kind change drop it, and it is freed with the model; a
 *      selection, a mask upload, an edit, a rendered frame, gsx_model_normals / _select_normals and the calls of this section do
 *      not.  The filter was evaluated when the plane was made: a later selection or mask does not change which Gaussians are fitted.
 *      Models made by extract, merge, convert and decimate start without one.
 *      gsx_model_align_plane_step.  The search is desc->nearest, exactly gsx_model_align_step's; out->nearest its statistics.  The
 *      pairs used are the found pairs (q, t) whose target has a kept, fitted normal n (a finite variation) and, with max_variation >
 *      0, variation <= max_variation; the other found pairs are counted in n_unfitted.  The sums, in double and in index order,
 *      products of float32 values and of float32 differences taken in double without contraction: pass 0 the count and sum q, the
 *      centre c = fl32(sum q / count); pass 1 per pair d = q - c and g = q - t per axis in float32, a = d x n (each component d_u n_v -
 *      d_v n_u), e = (g_x n_x + g_y n_y) + g_z n_z, J = (a, n): the 21 upper-triangle entries of A = sum J J^T, the 6 of b = sum J e,
 *      sum e^2 and sum d2; folded from per-workgroup partials in index order: the same bits on every call.  No sum depends on the
 *      sign of n: the canonical orientation suffices.
 *      The solve, on the host in double: A's eigenvalues (returned descending) and eigenvectors by cyclic Jacobi; rank = the number
 *      of eigenvalues above 1e-9 x the largest; x = -sum over those of v (v . b) / lambda: the minimum-norm solution, exactly 0
 *      along the undetermined directions (a floor against a floor has rank 3: the lift and two tilts).  With x = (omega, tau): quat
 *      is the rotation by |omega| about omega / |omega| (x, y, z, w; w >= 0; the identity for |omega| = 0), pos = c + tau - R c, and
 *      xform_next = delta o the matrix used, scale 1, rounded once to float32.  Fewer than 3 pairs used, or rank 0: degenerate = 1,
 *      the identity delta and xform_next = the matrix used; not an error.  normal_matrix and rhs are returned: A^-1 is the
 *      registration's uncertainty.  rms_before = sqrt(sum d2 / n_pairs), rms_plane_before = sqrt(sum e^2 / n_pairs).
 *      Errors: gsx_model_normals' for the keep (GSX_ERR_OOM leaves the model and an older plane as they were) and
 *      gsx_model_align_step's for the step, for the same conditions; unknown flag bits, a max_variation that is negative or NaN, a
 *      reserved word != 0, or a dst_key without a kept plane (gsx_model_normals_keep first): GSX_ERR_INVALID_ARG.  No queries or no
 *      targets: GSX_OK, degenerate, zeros. ---- */
typedef struct gsx_normals_kept_t {
    uint32_t present; uint32_t k; uint32_t orient; uint32_t filter; /* 0 / 1; what gsx_model_normals_keep was called with */
    float toward[3]; uint32_t reserved;
    uint64_t count; uint64_t n_fitted; /* the model's Gaussians when the plane was made; those with a plane */
} gsx_normals_kept_t; /* 48 B */
typedef struct gsx_align_plane_desc {
    gsx_nearest_desc nearest;
    uint32_t flags; float max_variation; uint32_t reserved[2]; /* 0; 0: no limit */
} gsx_align_plane_desc; /* 96 B */
typedef struct gsx_align_plane_step_t {
    double pos[3]; double quat[4];   /* the delta: t ~ R(quat) q + pos */
    double normal_matrix[21];        /* the upper triangle of A, row-major */
    double rhs[6];                   /* b */
    double eigenvalues[6];           /* of A, descending */
    double centre[3];                /* c */
    double rms_before; double rms_plane_before;
    uint64_t n_pairs; uint64_t n_unfitted;
    float xform_next[12];
    uint32_t rank; uint32_t degenerate;
    gsx_nearest_stats_t nearest;
} gsx_align_plane_step_t; /* 568 B */
gsx_status gsx_model_normals_keep(gsx_viewer* v, const char* key, const gsx_normals_desc* desc, gsx_normals_stats_t* out);
gsx_status gsx_model_normals_kept(gsx_viewer* v, const char* key, gsx_normals_kept_t* out, float* out_normal /* nullable, n * 3 */,
                                  float* out_variation /* nullable, n */);
gsx_status gsx_model_normals_reset(gsx_viewer* v, const char* key);
gsx_status gsx_model_align_plane_step(gsx_viewer* v, const char* src_key, const char* dst_key, const gsx_align_plane_desc* desc,
                                      gsx_align_plane_step_t* out);

/* ---- the plane of a model: a robust consensus fit of ONE plane to the model's Gaussians, a select by the signed distance to a plane,
 *      and the rigid motion that stands a plane level (spec/RENDER_SPEC.md §28 [BUILD-SPEC]; kernels_plane.hip, csrc/plane_math.h).
 *      Everything is in model space.  The participants are §18's: the GSX_BOUNDS_* filter (the fit: inverted as a whole by the flag
 *      GSX_EXTRACT_INVERT, as gsx_model_extract inverts it) and three finite stored coordinates; the others that pass the filter are
 *      counted in n_nonfinite.
 *      The residual of a participant p against a plane: r = ((nx px + ny py) + nz pz) - offset in float32, every operation rounded.
 *      An inlier has |r| <= tolerance (inclusive) and, with min_cos > 0, a kept fitted normal k (gsx_model_normals_keep first) with
 *      |c| >= min_cos, c = (kx nx + ky ny) + kz nz in float32 (§26's FACING cosine).
 *      gsx_model_fit_plane.  n_candidates planes are made, all participants are tested against each (N x H tests, on the device), the
 *      valid candidate with the most inliers wins (ties: the smaller index), and up to refine_iters rounds fit a least-squares plane
 *      to the current plane's inliers and recount.  Candidates: slot s of candidate h probes the indices mix(seed, h, s, t) mod n,
 *      t = 0 .. 63 (mix: output (h << 16 | s << 8 | t) of the splitmix64 stream seeded with seed) and takes the first participant
 *      (NORMALS: the first participant with a fitted kept normal).  GSX_PLANE_SAMPLE_TRIPLES: three slots a, b, c, which must be
 *      three different indices; u = b - a, v = c - a in float32, u x v and its length in double, the quotient rounded to float32, the
 *      offset (nx ax + ny ay) + nz az in float32.  GSX_PLANE_SAMPLE_NORMALS: one slot, its kept normal, the offset likewise.
 *      GSX_PLANE_SAMPLE_CALLER: `candidates`, used as given: they are NOT normalised, so a residual is a distance only for a unit
 *      normal.  A candidate is invalid if a slot found nothing in 64 probes, two slots coincide, the cross product's length is zero
 *      or not finite, or (CALLER) a component is not finite or the normal is zero: it scores 0, is reported as normal 0, offset 0
 *      and is not counted in n_valid.  out_candidates and out_counts (nullable, n_candidates entries) receive every candidate and
 *      its exact inlier count.  The same seed gives the same bytes.
 *      Refinement.  Pass 0 sums the count, sum p and sum r^2 in double over the plane's inliers; the centre is c = fl32(sum p /
 *      count); pass 1 sums the six products of d = p - c (float32) in double; the normal is the eigenvector of the smallest
 *      eigenvalue (fixed-sweep Jacobi in double), rounded to float32, signed by §26's rule (orient, toward) at the centre; offset =
 *      (float)((nx cx + ny cy) + nz cz).  A recount that gives fewer inliers than the plane before ends the call with the plane
 *      before: n_inliers >= candidate_inliers.  Per-workgroup partials are folded in index order: the same bits on every call.
 *      centroid, eigenvalues (descending), sums (sum p, the six scatter terms xx xy xz yy yz zz, then sum r^2 of the accepted plane
 *      over its own inliers) and rms = sqrt(sum r^2 / n_inliers) describe the last accepted fit and are 0 without one.  No valid
 *      candidate (winner = GSX_PLANE_NONE), or a winner with fewer than 3 inliers: degenerate = 1, GSX_OK, the planes all zero.
 *      gsx_model_select_plane: the hit set is the participants with lo <= r <= hi (signed; a bound may be infinite) and, with
 *      min_cos > 0, the facing rule above; written with selection_op; the tail bits, a model without a selection and
 *      GSX_BOUNDS_SELECTED reading the selection as it was before the call are gsx_model_select_knn's rules.
 *      gsx_plane_level (host only, computed in double and rounded once to float32): quat (x, y, z, w; w >= 0) is the shortest-arc rotation that takes the plane's unit
 *      normal to up / |up|; where they are antiparallel, the half turn about e x n normalised, e the coordinate axis along which
 *      |n| is smallest (the first of equals).  pos = -(offset / |n|) up / |up|: the rotated plane passes through the origin's
 *      height.  The pair is what gsx_update_model_transform or gsx_model_apply_transform takes with scale 1.
 *      Recipes.  Level a capture: fit_plane, gsx_plane_level with the world's up, gsx_update_model_transform.  Remove the floor:
 *      select_plane(lo = -inf, hi = tolerance), then gsx_model_extract with GSX_BOUNDS_SELECTED and GSX_EXTRACT_INVERT.
 *      Peel the next plane: select_plane(-tolerance, tolerance) with GSX_SELECTION_ADD, then fit again with filter
 *      GSX_BOUNDS_SELECTED and flags GSX_EXTRACT_INVERT: the participants are the Gaussians no plane has taken yet (on a model
 *      without a selection: all).
 *      Errors.  GSX_ERR_INVALID_ARG: a null viewer, key, desc or out; unknown filter, flag, sample, orient or op values;
 *      n_candidates outside 1 .. 1024; a tolerance that is negative or not finite; bounds with lo > hi or a NaN; min_cos outside
 *      [0, 1]; refine_iters > 8; CALLER without candidates; a reserved word != 0; a select plane with a non-finite component or a
 *      zero normal; min_cos > 0 or sample NORMALS on a model without kept normals; a toward that is not finite.  GSX_ERR_NOT_FOUND:
 *      an unknown key.  GSX_ERR_UNSUPPORTED: a viewer with a communicator, a sharded model.  GSX_ERR_OOM: the model and its
 *      selection are left as they were.  No Gaussians or no participants: GSX_OK, degenerate, zeros.  Nothing a frame reads is
 *      written, but the selection by the select call. ---- */
typedef struct gsx_plane_t { float normal[3]; float offset; } gsx_plane_t; /* 16 B: the points p with n . p = offset */
#define GSX_PLANE_MAX_CANDIDATES 1024u
#define GSX_PLANE_MAX_REFINE 8u
#define GSX_PLANE_NONE 0xFFFFFFFFu
#define GSX_PLANE_SAMPLE_TRIPLES 0u   /* three sampled participants */
#define GSX_PLANE_SAMPLE_NORMALS 1u   /* one sampled participant and its kept normal (gsx_model_normals_keep first) */
#define GSX_PLANE_SAMPLE_CALLER  2u   /* the planes the caller passes */
typedef struct gsx_plane_fit_desc {
    uint32_t filter; uint32_t flags; uint32_t sample; uint32_t n_candidates; /* GSX_BOUNDS_*; GSX_EXTRACT_INVERT; GSX_PLANE_SAMPLE_*; 1 .. 1024 */
    uint64_t seed;
    float tolerance; float min_cos;       /* finite, >= 0; 0: off, otherwise in (0, 1] */
    uint32_t refine_iters; uint32_t orient; /* 0 .. 8; GSX_NORMALS_ORIENT_* */
    float toward[3]; uint32_t reserved[3];
} gsx_plane_fit_desc; /* 64 B */
typedef struct gsx_plane_fit_t {
    gsx_plane_t plane; gsx_plane_t candidate; /* the result; the winning candidate */
    uint32_t winner; uint32_t n_valid;
    uint64_t count; uint64_t n_nonfinite;     /* participants; filtered Gaussians without a finite position */
    uint64_t candidate_inliers; uint64_t n_inliers;
    float centroid[3]; uint32_t refine_done;
    double eigenvalues[3]; double rms;
    double sums[10];
    uint32_t degenerate; uint32_t reserved;
} gsx_plane_fit_t; /* 208 B */
typedef struct gsx_plane_select_desc {
    gsx_plane_t plane;
    float lo; float hi; float min_cos; uint32_t filter;
    uint32_t selection_op; uint32_t reserved[3];
} gsx_plane_select_desc; /* 48 B */
void gsx_plane_fit_desc_default(gsx_plane_fit_desc* desc);       /* TRIPLES, 256 candidates, seed 0, tolerance 0, 2 refine rounds */
void gsx_plane_select_desc_default(gsx_plane_select_desc* desc); /* the plane z = 0, lo = hi = 0, GSX_SELECTION_SET */
gsx_status gsx_model_fit_plane(gsx_viewer* v, const char* key, const gsx_plane_fit_desc* desc, const gsx_plane_t* candidates /* CALLER only */,
                               gsx_plane_t* out_candidates /* nullable, n_candidates */, uint32_t* out_counts /* nullable, n_candidates */,
                               gsx_plane_fit_t* out);
gsx_status gsx_model_select_plane(gsx_viewer* v, const char* key, const gsx_plane_select_desc* desc, uint64_t* out_hit, uint64_t* out_selected);
gsx_status gsx_plane_level(const gsx_plane_t* plane, const float up[3], float quat_xyzw[4], float pos[3]); /* host only */

/* ---- selection, per-Gaussian edits, queries.  The app builds the pods and calls
 *      the crate (src/tab/scene.rs:740-835, 601-614, 651-657; app.rs:1479-1564); the arithmetic is the build's,
 *      spec/RENDER_SPEC.md §7 [BUILD-SPEC].  None of this costs anything while no selection / edit / query exists. ---- */
#define GSX_EDIT_ENABLED 1u        /* gs::GaussianEditFlag::ENABLED        (app.rs:1546-1552) */
#define GSX_EDIT_HIDDEN 2u         /* gs::GaussianEditFlag::HIDDEN */
#define GSX_EDIT_OVERRIDE_COLOR 4u /* gs::GaussianEditFlag::OVERRIDE_COLOR: color is RGB, otherwise an HSV edit */
/* gs::GaussianEditPod::new(flag, color, contrast, exposure, gamma, alpha) (app.rs:1553-1562); 32 bytes */
typedef struct gsx_gaussian_edit {
    uint32_t flag;
    float color[3]; /* HSV edit: hue shift [0,1], saturation factor, brightness factor; or the override RGB */
    float contrast, exposure, gamma, alpha;
} gsx_gaussian_edit;
void gsx_gaussian_edit_default(gsx_gaussian_edit* e); /* gs::GaussianEditPod::default(): flag 0, (0,1,1), 0, 0, 1, 1 */

typedef enum gsx_query_kind {  /* gs::QueryNonePod / QueryHitPod / the QueryToolset's rect, brush and texture queries */
    GSX_QUERY_NONE = 0, GSX_QUERY_HIT = 1, GSX_QUERY_RECT = 2, GSX_QUERY_BRUSH = 3, GSX_QUERY_TEXTURE = 4
} gsx_query_kind;
typedef enum gsx_selection_op { GSX_SELECTION_SET = 0, GSX_SELECTION_ADD = 1, GSX_SELECTION_REMOVE = 2 } gsx_selection_op;
typedef struct gsx_query {  /* coordinates in viewport pixels, origin top-left */
    uint32_t kind;         /* gsx_query_kind */
    uint32_t selection_op; /* gsx_selection_op (gs::QuerySelectionOp, scene.rs:1605), applied by gsx_postprocess */
    float p0[2];           /* Hit: the point; Rect: one corner; Brush: stroke start */
    float p1[2];           /* Rect: the opposite corner; Brush: stroke end */
    float radius;          /* Brush */
    uint32_t reserved;
} gsx_query;
typedef struct gsx_query_hit { uint32_t index; float depth; float alpha; uint32_t reserved; } gsx_query_hit; /* gs::QueryHitResultPod */
#define GSX_QUERY_MAX_HITS 65536u

/* viewer.update_query(queue, &pod) (scene.rs:785): the query every following gsx_preprocess evaluates. */
gsx_status gsx_update_query(gsx_viewer* v, const gsx_query* q);
/* The query texture the toolset paints its strokes into (viewer.update_query_texture_size + QueryToolset::render,
 * scene.rs:740, 791): width*height bytes from HOST memory, non-zero = selected; must match the viewport. */
gsx_status gsx_update_query_texture(gsx_viewer* v, const uint8_t* texels, uint32_t width, uint32_t height);
/* viewer.update_selection_highlight(queue, rgba) / _with_pod (scene.rs:816-829); alpha 0 = no highlight. */
gsx_status gsx_update_selection_highlight(gsx_viewer* v, const float rgba[4]);
/* viewer.update_selection_edit_with_pod(queue, &pod) (scene.rs:815, 821, 848): while ENABLED, every preprocess writes
 * it into the edit records of the selected Gaussians. */
gsx_status gsx_update_selection_edit(gsx_viewer* v, const gsx_gaussian_edit* e);
/* The "unedited model" bind group (scene.rs:856-863): on != 0 renders the model ignoring (and not touching) edits. */
gsx_status gsx_model_show_unedited(gsx_viewer* v, const char* key, uint32_t on);
/* postprocessor.postprocess(...) (scene.rs:601-611): applies the selection op of a Rect/Brush/Texture query evaluated
 * by the last gsx_preprocess(key) to the model's selection. */
gsx_status gsx_postprocess(gsx_viewer* v, const char* key);
/* Selection bitset, ceil(len/32) words, bit i = Gaussian i selected. */
gsx_status gsx_model_upload_selection(gsx_viewer* v, const char* key, const uint32_t* words, uint64_t n_words);
gsx_status gsx_model_download_selection(gsx_viewer* v, const char* key, uint32_t* words, uint64_t n_words);
/* gaussians_edit_buffer.download() (app.rs:789): len records; Gaussians never edited read as the default pod. */
gsx_status gsx_model_download_edits(gsx_viewer* v, const char* key, gsx_gaussian_edit* out, uint64_t n);
gsx_status gsx_model_upload_edits(gsx_viewer* v, const char* key, const gsx_gaussian_edit* edits, uint64_t n);
/* gs::query::download(count_buffer, results_buffer) (scene.rs:651-657): hits of the last Hit query on `key`, sorted by
 * (depth, index). */
gsx_status gsx_query_download_hits(gsx_viewer* v, const char* key, gsx_query_hit* out, uint64_t capacity, uint64_t* out_n);
/* gs::query::hit_pos_by_closest / hit_pos_by_alpha_range (scene.rs:660-679), host arithmetic: world position on the
 * pixel ray through `coords` at the chosen hit's depth.  view/proj column-major as in gsx_update_camera.
 * GSX_ERR_NOT_FOUND when there is no hit. */
gsx_status gsx_query_hit_pos_by_closest(const gsx_query_hit* hits, uint64_t n, const float view[16], const float proj[16],
                                        uint32_t width, uint32_t height, const float coords[2], uint32_t* out_index,
                                        float out_pos[3]);
gsx_status gsx_query_hit_pos_by_alpha_range(const gsx_query_hit* hits, uint64_t n, const float view[16], const float proj[16],
                                            uint32_t width, uint32_t height, const float coords[2], float range,
                                            uint32_t* out_index, float* out_alpha, float out_pos[3]);

/* ---- the query toolset: gs::QueryToolset, gs::QueryTextureOverlay and gs::QueryCursor (src/tab/scene.rs:740, 766-791, 2003-2014,
 *      2317-2325), in the library.  While the pointer is dragged the app calls query_toolset.update_pos + query_toolset.render(queue,
 *      &mut encoder, &query_texture) every frame and shows the texture over the splats; end() turns the painted texture into ONE texture
 *      query.  One toolset per viewer; the rule it paints by is spec/RENDER_SPEC.md §7, "Toolset".
 *  - State (host only, no device call): use_texture (default 1; 0 = immediate mode: nothing is painted, every frame's query is the live
 *    Rect / Brush segment), brush_radius (default 40), the active tool with its selection op, start, previous and current position.
 *    gsx_toolset_start clears the texture and paints the first shape (Rect: the rectangle start..pos, replaced by every repaint; Brush: a
 *    disc, then one capsule prev -> pos per gsx_toolset_update_pos, of the radius in force at that call, accumulating until the next
 *    start).  gsx_toolset_update_pos without an active tool only records the position, for the cursor.  gsx_toolset_query is
 *    query_toolset.query(), once per frame, and the caller passes what it returns to gsx_update_query: None while a texture stroke is
 *    drawn, the one Texture query after gsx_toolset_end, then None again; in immediate mode the live query, None after gsx_toolset_end.
 *  - gsx_toolset_start and gsx_toolset_update_pos QUEUE their paints (up to 64 brush segments; a full queue is enqueued at once by the
 *    call that filled it — nothing is dropped).  gsx_toolset_render enqueues everything queued as ONE kernel launch over the tiles the
 *    pending shapes touch, on the viewer's stream, and returns: no host copy, no host wait, and — unlike gsx_update_query_texture — no
 *    wait for the frames in flight on the lanes.
 *  - Ordering is stream order on the viewer's stream.  Frames on lanes never read the texture (their query is None: a frame with a query
 *    runs on the viewer itself, see gsx_render_options); the texture-query frame and the RGBA8 resolve run on the viewer's stream, after
 *    every paint enqueued before them — the resolve that draws the stroke also when the frame it resolves was rendered by a lane
 *    (gsx_download_rgba8 then runs it on the viewer's stream, behind that lane's frame).  A paint enqueued while a texture-query frame is
 *    in flight comes after that frame's read.
 *  - Size: the texture follows the viewport.  gsx_toolset_render (or a full queue) allocates and zero-fills it when gsx_update_camera has
 *    changed the size since the texture was made — what was painted is gone, as after viewer.update_query_texture_size (scene.rs:740) —
 *    and from then on a texture query finds a viewport-sized texture.  A texture painted for another viewport and not rendered again is
 *    refused by gsx_preprocess like any wrongly sized one.  gsx_update_query_texture still replaces the contents with the caller's.
 *    (A viewer whose camera was never set has the default 1 x 1 viewport: a render there makes a one-texel texture — harmless, and
 *    replaced by the first render after gsx_update_camera.)
 *  - Drawn by gsx_download_rgba8 and gsx_resolve_rgba8_device, on top of splats over overlay lines over background (gsx_download_framebuffer
 *    keeps returning the splats' (rgb, T)): while a texture stroke is drawn — from gsx_toolset_start to the gsx_toolset_query that hands
 *    out the Texture query — every pixel whose texel is non-zero is blended with texture_rgba (straight alpha: rgb' = rgb (1 - a) + c a,
 *    alpha' = alpha (1 - a) + a, applied to the resolved colour before the 8-bit rounding).  Until the first gsx_toolset_render after
 *    gsx_toolset_start the texture still holds what was there before — the stroke before, a host upload — and a resolve in between draws
 *    nothing of it.  While no texture stroke is drawn, once a position has been reported,
 *    the cursor with cursor_rgba: a ring of radius brush_radius at the position (pixel centres at distance d, |d - brush_radius| <=
 *    cursor_thickness / 2) or, during an immediate-mode Rect stroke, the outline of the rectangle start..pos (pixel centres within
 *    cursor_thickness / 2 of its boundary, Chebyshev, inside or outside).  One or the other, never both.  Both colours default to alpha 0
 *    and neither exists until its alpha is > 0: the same launches, the same bits. */
typedef enum gsx_toolset_tool { GSX_TOOL_RECT = 0, GSX_TOOL_BRUSH = 1 } gsx_toolset_tool;
gsx_status gsx_toolset_set_use_texture(gsx_viewer* v, uint32_t on);
gsx_status gsx_toolset_update_brush_radius(gsx_viewer* v, float radius); /* > 0, finite */
gsx_status gsx_toolset_start(gsx_viewer* v, uint32_t tool, uint32_t selection_op, const float pos[2]);
gsx_status gsx_toolset_update_pos(gsx_viewer* v, const float pos[2]);
gsx_status gsx_toolset_end(gsx_viewer* v);
gsx_status gsx_toolset_query(gsx_viewer* v, gsx_query* out);
/* active: 0 no tool (the other outputs are not written), 1 a stroke is under way; any output may be NULL */
gsx_status gsx_toolset_state(gsx_viewer* v, uint32_t* active, uint32_t* tool, uint32_t* selection_op, float start[2], float pos[2]);
/* query_toolset.render(queue, &mut encoder, &query_texture), scene.rs:791 */
gsx_status gsx_toolset_render(gsx_viewer* v);
/* straight-alpha colours in [0, 1] of the stroke overlay and of the cursor, the cursor's line thickness in pixels (>= 0) */
gsx_status gsx_toolset_set_overlay(gsx_viewer* v, const float texture_rgba[4], const float cursor_rgba[4], float cursor_thickness);
/* the query texture as the device holds it (width x height bytes = its size, the viewport's once rendered). Synchronises. */
gsx_status gsx_download_query_texture(gsx_viewer* v, uint8_t* texels, uint32_t width, uint32_t height);

/* ---- ref-counted buffer handles for readback off the owner's thread.  gs:: buffers are cheaply `Clone`: the export path clones
 *      every model's edit and mask buffer, moves the clones into two spawned threads and downloads there while the UI thread
 *      keeps rendering (app.rs:769-816, scene.rs:635-648).  gsx_model_buffer_retain (owner thread; enqueues a device-side
 *      snapshot on the viewer's stream: the contents as of this call, what a clone + download reads in wgpu's submission
 *      order) returns a handle; gsx_buffer_download runs on ANY thread, concurrently with frames, uploads, gsx_model_remove
 *      and even gsx_viewer_destroy — it touches only the handle.  gsx_buffer_retain adds a reference (a clone),
 *      gsx_buffer_release drops one; the snapshot is freed with the last.  Elements: GSX_BUFFER_EDITS -> gsx_gaussian_edit x
 *      len (never-edited Gaussians read as the default pod); GSX_BUFFER_MASK / _SELECTION -> uint32 x ceil(len / 32). ---- */
typedef struct gsx_buffer gsx_buffer;
typedef enum gsx_buffer_kind { GSX_BUFFER_MASK = 0, GSX_BUFFER_EDITS = 1, GSX_BUFFER_SELECTION = 2 } gsx_buffer_kind;
gsx_status gsx_model_buffer_retain(gsx_viewer* v, const char* key, gsx_buffer_kind kind, gsx_buffer** out);
gsx_status gsx_buffer_retain(gsx_buffer* b);
void gsx_buffer_release(gsx_buffer* b);
gsx_status gsx_buffer_len(gsx_buffer* b, uint64_t* out_elements);
gsx_status gsx_buffer_download(gsx_buffer* b, void* out, uint64_t n_elements);

/* ---- multi-GPU stage split.  No reference counterpart: the reference renders on one wgpu device
 *      (src/main.rs:85-98).  One process per GPU holds an index shard of the Gaussians; the screen is cut into
 *      `world` contiguous bands of tile rows, band g = rank g.  Per frame and rank:
 *        [gsx_shard_set_windows(key, windows)]            optional: lets the projection skip what cannot travel
 *        gsx_preprocess(key)                              project the resident shard
 *        gsx_shard_pack(key, world, windows, ..)          the records some tile's depth-key window [lo, hi) admits,
 *                                                         grouped by destination (first frame: no windows = all)
 *        [RCCL all-to-all of the 48-byte records, done by the caller]
 *        gsx_shard_import(.., windows); gsx_sort(key); gsx_render(&key, 1)   this rank's band, progressive slabs;
 *                                                         a tile bins exactly the records its window admits
 *        gsx_shard_feedback(..) -> per-tile saturation depth keys   one small all-gather: verification AND the
 *                                                                   next frame's windows (caller's policy)
 *        only if a tile with a bounded window is still open: gsx_shard_pack(key, world, windows2, ..) with
 *        windows2 = [hi, inf) for those tiles and [0, 0) elsewhere -> all-to-all -> gsx_shard_import(.., windows2)
 *        -> gsx_sort -> gsx_render_more(&key, 1)          (composited behind what the tiles hold)
 *        [RCCL all-gather of the bands straight into the caller's padded framebuffer]
 *      Pixels equal the single-GPU frame bit for bit whatever was predicted. ---- */
#define GSX_RECORD_BYTES 48u /* mean.xy rect.xy | conic.abc opacity | rgb depth */
typedef struct gsx_shard_layout_t {
    uint32_t rows_per_rank, row_lo, row_hi; /* tallest band of the layout; band of this rank: tile rows [row_lo, row_hi) */
    uint64_t band_bytes;                    /* this rank's band: rows * 16 * width * 16 (equal bands: rows_per_rank rows for every rank) */
    uint64_t band_offset_bytes;             /* of this rank's band inside the framebuffer */
    uint64_t padded_framebuffer_bytes;      /* whole tile rows of every band >= width * height * 16 */
} gsx_shard_layout_t;
gsx_status gsx_shard_layout(gsx_viewer* v, uint32_t world, uint32_t rank, gsx_shard_layout_t* out);
/* Screen-band rendering: this viewer composites only the tile rows [row_lo, row_hi) (clamped to the frame); Gaussians
 * whose tile rectangle misses the band are culled by gsx_preprocess, the other rows of the framebuffer are not touched.
 * With the whole scene resident on every GPU (10 M Gaussians = 8 GB of 288 GB) rank g renders band g of
 * gsx_shard_layout and the bands are all-gathered: no record exchange at all.  Default: every row. */
gsx_status gsx_viewer_set_band(gsx_viewer* v, uint32_t row_lo, uint32_t row_hi);
/* Render into caller-owned DEVICE memory (row-major [height][width] float4; may be padded below). NULL restores
 * the internal framebuffer. */
gsx_status gsx_viewer_set_external_framebuffer(gsx_viewer* v, void* d_ptr, uint64_t bytes);
/* Resolve the pixel rows [y0, y1) of the (rgb, T) framebuffer against a background colour into RGBA8 in caller-owned
 * DEVICE memory ((y1 - y0) * width uint32, R in the low byte) — the app's final blit to its Rgba8Unorm surface, per band:
 * what the screen-band mode all-gathers (4 bytes a pixel instead of 16).  Enqueued on the viewer's stream, no host
 * synchronisation.  Rows below the image (the padding of an external framebuffer) may be included. */
gsx_status gsx_resolve_rgba8_device(gsx_viewer* v, const float background_rgb[3], uint32_t y0, uint32_t y1, void* d_rgba);
/* Tile windows: d_tile_window (device, nullable, copied by the call) = one {uint32 lo, uint32 hi} pair per tile,
 * row-major [height/16 rounded up][width/16 rounded up]; a tile admits a record iff lo <= depth key < hi.
 * NULL = every tile admits everything.
 *
 * counts[world] (host) = records per destination; d_send (device) receives the travelling records grouped by
 * destination, ascending local index inside each group.  A visible record travels to rank g if its tile rectangle
 * holds, inside g's band, a tile that admits it.  Synchronises. */
gsx_status gsx_shard_pack(gsx_viewer* v, const char* key, uint32_t world, const uint32_t* d_tile_window, void* d_send,
                          uint64_t capacity_records, uint64_t* counts);
/* Optional, BEFORE gsx_preprocess: the windows [0, hi) the coming exchange will use (NULL clears).  The projection
 * pass then is geometry only, admits candidates against a max-pyramid of the window ends (a conservative superset of the
 * travellers), and only those get their conic / colour records; gsx_shard_pack(.., d_tile_window = NULL, ..) packs
 * from that candidate list with the exact windows given here — nothing else of the shard is looked at.  A later
 * gsx_shard_pack with explicit windows (the repair exchange) scans the whole shard and shades the travellers the
 * first round did not. */
gsx_status gsx_shard_set_windows(gsx_viewer* v, const char* key, const uint32_t* d_tile_window);
/* d_recv (device): n_records records ordered by (source rank, source index).  They become the model's active
 * record set for gsx_sort / gsx_render(_more); binning is restricted to this rank's band and to the tiles that
 * admit the record (the receiving side of gsx_shard_pack's predicate, so that every tile composites a gap-free
 * depth prefix in each round).  The model's own projection stays available for a second gsx_shard_pack. */
gsx_status gsx_shard_import(gsx_viewer* v, const char* key, const void* d_recv, uint64_t n_records, uint32_t world,
                            uint32_t rank, const uint32_t* d_tile_window);
/* Enqueues the write of *out_words = rows_per_rank * (width/16 rounded up) u32 into DEVICE memory: for every tile of
 * this rank's band, the depth key of the splat that saturated its last pixel this frame, 0 = still open (also for
 * padding rows below the frame).  An all-gather over ranks is the map of the whole (padded) frame. */
gsx_status gsx_shard_feedback_words(gsx_viewer* v, uint32_t world, uint32_t* out_words);
gsx_status gsx_shard_feedback(gsx_viewer* v, const char* key, uint32_t world, uint32_t rank, void* d_out_u32);
/* Second round of the same frame: like gsx_render but continues from the framebuffer / saturated-tile state. */
gsx_status gsx_render_more(gsx_viewer* v, const char* const* keys, uint32_t n_keys);

/* ---- multi-GPU, device-resident protocol.  Windows, verification, the repair round's windows, next frame's limits and every
 *      record count stay on the device; the exchange moves fixed-size SLOTS whose headers carry the counts (buffer of a round
 *      = `world` slots of (1 + T) records of GSX_RECORD_BYTES; record 0 of slot g = {u32 records the sender had for g, u32
 *      records sent = min(that, T)}); the host waits for ONE thing per frame, the verdict of round 0 — two words in pinned
 *      memory that the verification kernel derives from globally gathered data, so that every rank reads the same verdict
 *      and takes the same decision.  Per frame and rank (the STAGE calls below, for a caller that strings the protocol together
 *      itself: wgpu_3dgs_viewer_app_amd/parallel.py runs them with an injectable transport so that the tests can put `world` ranks
 *      on one GPU, or on CPU over gloo.  gsx_shard_render_frame runs the same stages without a host look inside the frame: its
 *      repair rounds are enqueued unasked and decide on the device, except the last model's, which — like a frame whose slots
 *      overflowed — is dealt with when the frame is retired; its verdicts go to a pinned ring that is read then):
 *        gsx_shard_frame_begin(key, world, rank, speculate, NULL)      windows [0, limit) from last frame's limits -> projection
 *        gsx_shard_slot_records(key, world, max_shard, &T)             round-0 slot size (2x what the last verdict reported)
 *        gsx_shard_pack_slots(key, world, 0, d_send, T)
 *        all-to-all of the slots, (1 + T) * 48 bytes per peer          gsx_comm_all_to_all
 *        gsx_shard_import_slots(key, d_recv, world, rank, 0, T)        import + depth sort + render this rank's band
 *        gsx_shard_feedback(key, world, rank, d_band) + all-gather     saturation depth key of every tile + slot statistics
 *        gsx_shard_verify(key, world, d_sat_all, &seq)                 repair windows on the device; posts the verdict
 *        gsx_shard_next_windows(..) ; all-gather of the bands          enqueued before the wait: what follows when all is well
 *        gsx_shard_wait_verdict(key, seq, &verdict)
 *          verdict.overflow: round 0 once more with T = max_shard (always fits), verify + wait again
 *          verdict.need_tiles > 0: gsx_shard_repair_count(d_4words) + all-gather + gsx_shard_post_counts(&seq) + wait -> T1
 *                                  (exact); pack_slots(.., 1, T1) -> all-to-all -> import_slots(.., 1, T1) -> feedback +
 *                                  all-gather -> next_windows + the band all-gather again (they replace the early ones)
 *        gsx_shard_frame_end(key)                                      the limits computed last become the next frame's
 *      Whatever the verdict, the frame that leaves the GPU is complete and equals the single-GPU frame bit for bit. ---- */
typedef struct gsx_shard_verdict {
    uint32_t need_tiles;   /* tiles of the frame with a bounded window that are still open (0 after gsx_shard_post_counts) */
    uint32_t overflow;     /* some rank had more records for a destination than the slot held: round 0 must be redone */
    uint32_t max_records;  /* records the busiest (rank, destination) pair wanted: next frame's slot hint / the repair round's T */
    uint32_t reserved;
} gsx_shard_verdict;
gsx_status gsx_shard_frame_begin(gsx_viewer* v, const char* key, uint32_t world, uint32_t rank, uint32_t speculate,
                                 const uint32_t* d_limit_override /* nullable: device u32 per tile, replaces the limits the last frame left */);
/* shard_records_max: the size of the model's LARGEST shard over all ranks (the caller's partition; ceil(N / world) for equal
 * shards).  Every rank gets the same answer: the policy uses only that and the last verdict's global figure. */
gsx_status gsx_shard_slot_records(gsx_viewer* v, const char* key, uint32_t world, uint32_t shard_records_max, uint32_t* out_records);
gsx_status gsx_shard_pack_slots(gsx_viewer* v, const char* key, uint32_t world, uint32_t round, void* d_send, uint32_t slot_records);
/* round: 0 or 1, | GSX_SHARD_BEHIND for a model of a LAYERED frame that is not the nearest one: its records are composited
 * behind what the nearer models of this frame left in the framebuffer (scene.rs:533-558, 2302-2314: models are painted far ->
 * near and never merged), and its feedback ignores the tiles those models had saturated already. */
#define GSX_SHARD_BEHIND 2u
gsx_status gsx_shard_import_slots(gsx_viewer* v, const char* key, const void* d_recv, uint32_t world, uint32_t rank, uint32_t round,
                                  uint32_t slot_records);
/* d_sat_all: the all-gathered gsx_shard_feedback bands: per rank gsx_shard_feedback_words() words = its band of saturation keys
 * (rows_per_rank tile rows) followed by 4 statistics words {records wanted for its busiest destination, slot overflowed, 0, 0} */
gsx_status gsx_shard_verify(gsx_viewer* v, const char* key, uint32_t world, const void* d_sat_all, uint32_t* out_seq);
gsx_status gsx_shard_wait_verdict(gsx_viewer* v, const char* key, uint32_t seq, gsx_shard_verdict* out);
/* repair round sizing: d_out4 (device, 4 u32) = {records this rank has for its busiest destination under the repair windows, 0,0,0};
 * all-gather those (16 bytes per rank), then gsx_shard_post_counts posts the global maximum as a verdict (max_records) */
gsx_status gsx_shard_repair_count(gsx_viewer* v, const char* key, uint32_t world, void* d_out4);
gsx_status gsx_shard_post_counts(gsx_viewer* v, uint32_t world, const void* d_counts_all, uint32_t* out_seq);
gsx_status gsx_shard_next_windows(gsx_viewer* v, const char* key, uint32_t world, const void* d_sat_all, float margin, uint32_t radius);
gsx_status gsx_shard_frame_end(gsx_viewer* v, const char* key);
/* parity / introspection: the per-tile limits the next frame will use (u32 per tile; 0xFFFFFFFF = unbounded). Synchronises. */
gsx_status gsx_shard_download_limits(gsx_viewer* v, const char* key, uint32_t* limits, uint64_t n_words);

/* ---- the collectives, inside the library over RCCL (xGMI): one communicator per viewer (with frames_in_flight = L sharded
 *      frames: L, the others created by the library on first use — a collective step), enqueued on the viewer's stream.
 *      RCCL is loaded at run time; missing / failing RCCL -> GSX_ERR_RCCL.  Bootstrap like any NCCL program: one rank calls
 *      gsx_comm_unique_id, the 128 bytes reach the other ranks by the host's own means, every rank calls gsx_viewer_comm_init
 *      (collective: returns when all `world` ranks have joined). ---- */
gsx_status gsx_comm_unique_id(uint8_t out_id[128]);
gsx_status gsx_viewer_comm_init(gsx_viewer* v, uint32_t world, uint32_t rank, const uint8_t id[128]);
gsx_status gsx_viewer_comm_destroy(gsx_viewer* v);
/* What the viewer's communicator IS, asked of the transport itself (a scaling record should show that RCCL saw N ranks, not that the
 * caller said N): transport 0 none / 1 RCCL / 2 in-process group / 3 the caller's functions; for RCCL nranks = ncclCommCount, rank =
 * ncclCommUserRank, device = ncclCommCuDevice of the first communicator, version = ncclGetVersion (e.g. 22707), lane_comms = the
 * further communicators frames in flight created; otherwise what the viewer was initialised with. */
typedef struct gsx_comm_info {
    uint32_t transport, nranks, rank, lane_comms;
    int32_t device, version;
} gsx_comm_info;
gsx_status gsx_viewer_comm_info(gsx_viewer* v, gsx_comm_info* out);
/* slot p of d_send goes to rank p, slot p of d_recv comes from rank p (grouped point-to-point: all xGMI links at once) */
gsx_status gsx_comm_all_to_all(gsx_viewer* v, const void* d_send, void* d_recv, uint64_t bytes_per_peer);
/* d_recv = world * bytes_per_rank; in place when d_send == d_recv + rank * bytes_per_rank */
gsx_status gsx_comm_all_gather(gsx_viewer* v, const void* d_send, void* d_recv, uint64_t bytes_per_rank);
/* One whole index-sharded frame of model `key` on this rank (needs a communicator: gsx_viewer_comm_init, _init_group or
 * _init_custom): the sequence above, into a padded framebuffer the library owns; after gsx_sync, gsx_download_framebuffer
 * returns the complete frame on every rank. */
gsx_status gsx_shard_render_frame(gsx_viewer* v, const char* key, uint32_t shard_records_max, uint32_t speculate, float margin, uint32_t radius);
/* The same for several LAYERED models — the reference paints `model_render_keys` far -> near and never merges models
 * (src/tab/scene.rs:533-558, 2302-2314), gsx_render does the same on one GPU.  Every model is index-sharded over the ranks
 * (shard_records_max[i] = largest shard of keys_far_to_near[i]); each keeps its own per-tile limits from frame to frame.  Per
 * model: exchange -> composite into this rank's band behind the nearer models -> verification -> repair exchange; one band
 * all-gather at the end.  The frame goes out model by model: the verdict of model i - 1 is read (a pinned word) before model i is
 * enqueued, and its repair is exchanged exactly sized where one is needed.  With frames_in_flight >= 2 a call alternates between what
 * is left of the frame before and the new one, and returns with half the new frame's models enqueued (any call that looks at a result
 * completes them).  GSX_SHARD_LAYER_PIPELINE=0: all models at once, the inner models' repair exchanges always enqueued with fixed-size
 * slots and decided on the device (measured slower).  Pixels equal gsx_render(keys_far_to_near) on one GPU bit for bit. */
gsx_status gsx_shard_render_frame_keys(gsx_viewer* v, const char* const* keys_far_to_near, uint32_t n_keys,
                                       const uint32_t* shard_records_max, uint32_t speculate, float margin, uint32_t radius);

/* ---- other transports under the same frame loop.  gsx_shard_render_frame only ever calls "all-to-all of equal slots" and
 *      "all-gather of equal pieces"; RCCL is one provider of the two.
 *      (a) in-process group: ONE host process drives several GPUs, one host thread and one viewer per GPU — what a
 *          single-process host such as the egui app (src/main.rs:85-98: one process, one event loop) would do.  The collectives are
 *          device-to-device copies ordered by HIP events (peer-to-peer over xGMI between devices), delivered in RCCL's order
 *          (by source rank); ranks meet at a host rendezvous inside every collective, which gives up after timeout_ms
 *          (0 = 60 s): every rank of the group then gets GSX_ERR_RCCL instead of a hang.  Also how the tests put `world`
 *          ranks on ONE GPU and run the real frame loop.
 *      (b) custom: the caller's own two functions (MPI, a test double ...).  They ENQUEUE on `hip_stream` like
 *          ncclSend / ncclRecv do and return 0 or a gsx_status; slot p of d_send goes to rank p, slot p of d_recv comes from
 *          rank p; the all-gather is in place when d_send == d_recv + rank * bytes_per_rank. ---- */
typedef struct gsx_comm_group gsx_comm_group;
gsx_status gsx_comm_group_create(uint32_t world, uint32_t timeout_ms, gsx_comm_group** out);
void gsx_comm_group_destroy(gsx_comm_group* g); /* after every viewer of the group called gsx_viewer_comm_destroy / _destroy */
gsx_status gsx_viewer_comm_init_group(gsx_viewer* v, gsx_comm_group* g, uint32_t rank);
typedef gsx_status (*gsx_comm_all_to_all_fn)(void* ctx, const void* d_send, void* d_recv, uint64_t bytes_per_peer, void* hip_stream);
typedef gsx_status (*gsx_comm_all_gather_fn)(void* ctx, const void* d_send, void* d_recv, uint64_t bytes_per_rank, void* hip_stream);
gsx_status gsx_viewer_comm_init_custom(gsx_viewer* v, uint32_t world, uint32_t rank, gsx_comm_all_to_all_fn all_to_all,
                                       gsx_comm_all_gather_fn all_gather, void* ctx);
/* A transport that moves pieces of UNEQUAL size (arrays of `world` byte offsets / sizes; a size may be 0): what RCCL's grouped
 * ncclSend / ncclRecv and the in-process group do.  all_to_all_v: send_bytes[p] bytes at d_send + send_offsets[p] go to rank p, what
 * rank p sends lands at d_recv + recv_offsets[p] (recv_bytes[p] bytes: the ranks derive the sizes from gathered data, they agree).
 * gather_v: this rank's send_bytes bytes to every rank (root < 0) or to `root` only; rank p's piece lands at d_recv + recv_offsets[p];
 * d_send may be d_recv + recv_offsets[rank] (in place).  Both ENQUEUE on hip_stream and return 0 or a gsx_status.
 * With such a transport gsx_shard_render_frame balances the bands by the previous frame's per-row work and sizes the exchange slots
 * pair by pair; with the equal-piece functions of gsx_viewer_comm_init_custom the bands stay equal and the slots uniform. */
typedef gsx_status (*gsx_comm_all_to_all_v_fn)(void* ctx, const void* d_send, const uint64_t* send_offsets, const uint64_t* send_bytes,
                                               void* d_recv, const uint64_t* recv_offsets, const uint64_t* recv_bytes, void* hip_stream);
typedef gsx_status (*gsx_comm_gather_v_fn)(void* ctx, const void* d_send, uint64_t send_bytes, void* d_recv, const uint64_t* recv_offsets,
                                           const uint64_t* recv_bytes, int32_t root, void* hip_stream);
gsx_status gsx_viewer_comm_init_custom_v(gsx_viewer* v, uint32_t world, uint32_t rank, gsx_comm_all_to_all_v_fn all_to_all_v,
                                         gsx_comm_gather_v_fn gather_v, void* ctx);
/* Band layout of the sharded frames: rank g owns the tile rows [edges[g], edges[g + 1]) (edges[0] = 0, edges[world] >= tiles_y, non-decreasing;
 * a band may be empty).  gsx_shard_set_band_edges: these edges for every following frame and stage call (NULL: back to the
 * library's own — equal bands, or, in gsx_shard_render_frame over a transport that moves unequal pieces, bands balanced by the previous
 * frame's per-row work; gsx_shard_set_balance(0) keeps those equal too).  Every rank must set the same.  gsx_shard_get_band_edges: the
 * layout the last sharded frame used. */
gsx_status gsx_shard_set_band_edges(gsx_viewer* v, uint32_t world, const uint32_t* edges);
gsx_status gsx_shard_get_band_edges(gsx_viewer* v, uint32_t world, uint32_t* out_edges);
gsx_status gsx_shard_set_balance(gsx_viewer* v, uint32_t enabled);

/* A caller with its own exchange policy (and the tests): per-tile limits the NEXT sharded frame of `key` uses instead of the ones
 * the last frame left (host or device memory, u32 per tile, 0xFFFFFFFF = unbounded; copied by the call), and a fixed round-0 slot size
 * (records; 0 = the library's policy).  Every rank must set the same values. */
gsx_status gsx_shard_set_limits(gsx_viewer* v, const char* key, const uint32_t* limits);
gsx_status gsx_shard_set_slot_records(gsx_viewer* v, const char* key, uint32_t records);
/* What the sharded frames of this viewer did since the last reset (host-side bookkeeping; never synchronises). */
typedef struct gsx_shard_stats {
    uint64_t frames;          /* gsx_shard_render_frame calls completed */
    uint64_t redo_frames;     /* frames whose round 0 was redone with whole-shard slots (a slot overflowed) */
    uint64_t repair_frames;   /* frames that needed the repair exchange */
    uint64_t exchange_rounds; /* all-to-all rounds in total */
    uint64_t wire_bytes;      /* bytes this rank sent to OTHER ranks: slots (fixed size, whatever they hold), feedback and band gathers */
    uint64_t verdict_wait_ns; /* host time spent waiting for verdicts */
    uint32_t last_slot_records, last_repair_slot_records;
    uint32_t last_entries_sum, last_entries_max; /* list entries all ranks / the busiest rank binned in the last frame whose verdict was read
                                                    (balance of the bands: max * world / sum) */
    uint32_t last_work_permille;                 /* work of the busiest rank's tiles x world x 1000 / all ranks': what the bands are balanced
                                                    by (1000 = perfectly even) */
    uint32_t redo_fallbacks;                     /* redone frames whose exactly sized slots overflowed again and that were redone with
                                                    whole-shard slots */
    uint32_t last_repair_records;                /* most records any rank had for one destination in the repair round of the last frame
                                                    whose verdict was read */
    uint32_t reserved0;
} gsx_shard_stats;
gsx_status gsx_shard_get_stats(gsx_viewer* v, gsx_shard_stats* out, uint32_t reset);
/* Where a sharded frame's finished bands go.  root = -1 (default): an all-gather — after gsx_shard_render_frame every rank's
 * framebuffer holds the whole frame ((world - 1) / world of W x H x 16 bytes INTO every rank: 29 MB per rank and frame at
 * 1920x1080 on 8 ranks).  root >= 0: only that rank's does — north_star's "into one framebuffer"; every other rank sends its
 * band there (4 MB each in the same case, arriving on 7 links side by side) and the rest of its own framebuffer is undefined.
 * Every rank must set the same root (ranks that disagree fail the frame).  RCCL and the in-process group gather to the
 * root; a custom transport (gsx_viewer_comm_init_custom) has only its two functions and keeps delivering every band to every rank. */
gsx_status gsx_shard_set_gather_root(gsx_viewer* v, int32_t root);

/* ---- PLY I/O (host side; no GPU needed).  gs::Gaussians::read_ply_header / PlyHeader::count /
 *      read_ply_gaussians + gs::Gaussian::from(PlyGaussianPod) (app.rs:1053-1096) and write_ply (app.rs:897-947).
 *      INRIA 3DGS vertex: x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3 (62 f32, 248 B;
 *      properties are located by NAME, missing f_rest_* read as 0).  binary_little_endian and ascii. ---- */
typedef struct gsx_ply_header {
    uint64_t count;        /* element vertex N  (PlyHeader::count) */
    uint64_t header_bytes; /* offset of the first vertex */
    uint32_t vertex_bytes; /* stride of one binary vertex (0 for ascii) */
    uint32_t is_ascii;
    int32_t offsets[62];   /* byte offset (binary) / column (ascii) of each INRIA property, -1 if absent */
} gsx_ply_header;
/* data/size: the file contents (at least the header). */
gsx_status gsx_ply_read_header(const void* data, uint64_t size, gsx_ply_header* out);
/* Converts vertices [start, start+n) into gs::Gaussian records (rot normalised from w,x,y,z to x,y,z,w;
 * scale = exp; colour = clamp(0.5 + C0*f_dc), alpha = sigmoid(opacity) as UNORM8; f_rest [3][15] -> [15][3]). */
gsx_status gsx_ply_read_gaussians(const void* data, uint64_t size, const gsx_ply_header* header, uint64_t start,
                                  uint64_t n, gsx_gaussian* out);
/* Inverse conversion into a binary_little_endian INRIA PLY.  mask_words (nullable): only Gaussians whose bit
 * is set are written (write_ply's mask iterator).  edits (nullable, n records; write_ply's Option<&[GaussianEditPod]>,
 * app.rs:908-940): ENABLED+HIDDEN Gaussians are dropped, the other ENABLED edits are baked into f_dc / opacity
 * (spec §7 Export).  Call with out == NULL to get the size in *out_size. */
gsx_status gsx_ply_write(const gsx_gaussian* gaussians, uint64_t n, const uint32_t* mask_words,
                         const gsx_gaussian_edit* edits, void* out, uint64_t capacity, uint64_t* out_size);

/* ---- debug: which stable-rank path the radix sort uses.  -1 (default): per device, decided by a start-up probe; 0: wave
 *      ballot matching (documented hardware behaviour only); 1: one returning LDS add per element (relies on same-address
 *      LDS adds of one instruction being served in ascending lane order — what the probe checks).  Process-wide.  Both give
 *      the same order; tests/test_gpu_sort_stress.py and test_gpu_parity.py assert it at full size. ---- */
void gsx_debug_set_radix_rank_mode(int32_t mode);

/* ---- how a frame's kernel launches reach the device.  gsx_preprocess / gsx_sort / gsx_render / gsx_render_frame record their
 *      launches and submit them as cached HIP graphs whose nodes are patched to the frame's arguments (a dependent kernel boundary
 *      costs 1.75 us inside a graph, 3.3 us on a stream; csrc/gsx_launch.h).  The reference records a wgpu CommandEncoder per frame
 *      and submits it once (scene.rs:856-873): same shape.  What a graph saves is HOST time (cfg4: 112 -> 37 us per frame); the
 *      device runs the same kernels at the same pace, and a graph only leaves when its last launch is recorded — so an entry point
 *      that finds its stream idle (a host that waits for every frame) submits launch by launch: the first kernel starts at once.
 *      And the device gains nothing (a real kernel boundary costs the same in a graph as on a stream; a frame that is one graph launch
 *      starts a few microseconds later): 1607 vs 1633 frames/s on cfg4 with one frame in flight.  So the default is
 *      enabled = 0: every launch is submitted at once; 1 (or GSX_GRAPH=1 in the environment): as described — for hosts whose time is what
 *      counts; 2: record even when the stream is idle (tests).  Process-wide.  Either way the same kernels run with the same arguments in the same order:
 *      frames are bit-identical (tests/test_gpu_graph.py). ---- */
void gsx_debug_set_launch_graphs(int32_t enabled);
uint64_t gsx_debug_launch_count(void); /* kernel launches this process has asked for so far (recorded or submitted) */
uint64_t gsx_debug_device_bytes(void); /* device memory the library's buffers hold in this process right now (every viewer, every model) */
/* tests: the framebuffer of lane `lane` (0: the viewer itself, i: its i-th lane) as it is once that lane's stream has drained — WITHOUT
 * completing the frames in flight (every other readback does).  With frames_in_flight = L the frame of call k sits in lane k mod L until
 * call k + L; after call k + 1 it is retired, i.e. complete: this is how a test looks at a frame that was continued across calls. */
gsx_status gsx_debug_download_lane_framebuffer(gsx_viewer* v, uint32_t lane, float* rgbt, uint64_t n_floats);
/* development (viewers created under GSX_TILE_PROFILE=1; tools/tile_profile.py): what every tile of the last frame's first block-compositor
 * launch cost — per tile 4 words: start and duration in 10 ns ticks, chunks of 128 list entries walked | chunks in its list << 16, takers blended */
gsx_status gsx_debug_tile_profile(gsx_viewer* v, uint32_t* out4, uint64_t n_tiles);
typedef struct gsx_launch_stats {
    uint64_t graph_launches;  /* hipGraphLaunch calls */
    uint64_t graph_nodes;     /* kernel launches that left inside a graph */
    uint64_t nodes_patched;   /* graph nodes whose grid / arguments had changed since the graph last ran */
    uint64_t direct_launches; /* kernel launches of recorded segments too short for a graph, submitted one by one */
    uint64_t graphs_built;    /* graphs instantiated (a kernel sequence seen for the first time at its position) */
    uint64_t broken;          /* != 0: a graph call failed on this viewer, it launches directly since (frames stay right) */
    uint64_t idle_direct_scopes; /* entry points that found their stream idle and submitted launch by launch (the device was waiting) */
} gsx_launch_stats;
gsx_status gsx_viewer_launch_stats(gsx_viewer* v, gsx_launch_stats* out, uint32_t reset);

/* ---- timing: HIP events recorded on the viewer's stream around each pass of the last frame ---- */
typedef enum gsx_pass {
    GSX_PASS_PROJECT = 0,
    GSX_PASS_DEPTH_SORT = 1,
    GSX_PASS_BIN = 2,
    GSX_PASS_TILE_SORT = 3,
    GSX_PASS_COMPOSITE = 4,
    GSX_PASS_PROJECT_GEOM = 5, /* the geometry-only projection of a lazily shaded (speculated / sharded) frame: another kernel,
                                  other bytes — timed apart from GSX_PASS_PROJECT so that each average is one kernel's */
    GSX_PASS_SHADE = 6,        /* conic / colour records (SH colour, cov2d) for the Gaussians a lazily shaded frame admitted or a depth slab's
                                  blocks take: the deferred half of K1's arithmetic — k_shade_quads + the frame's colour ops, wherever in
                                  the frame they run (inside the depth sort of a speculated frame, after each slab's binning otherwise).
                                  A speculated frame without colour ops normally has no shading launch at all: rider workgroups of the depth
                                  sort's two launches shade (GSX_SHORT_CHAIN, the default), and that time is the depth sort's.  While THIS
                                  pass is being timed the frame keeps the serial order, so its figure still means "shading alone" — and a
                                  loop timed with every pass bracketed is not the loop the headline rate runs */
    GSX_PASS_COUNT = 7
} gsx_pass;
/* enabled: 0 = off, 1 = every pass, otherwise a mask with bit (p + 1) set for each pass p to bracket with events
 * (an event pair costs a few microseconds of stream gap: time only what is being measured). */
gsx_status gsx_set_pass_timing(gsx_viewer* v, uint32_t enabled);
/* milliseconds of each pass accumulated over all models since the last call (resets accumulators);
 * synchronises. launches[i] = kernel launches of the dominant kernel of pass i. */
gsx_status gsx_get_pass_timing(gsx_viewer* v, float ms[GSX_PASS_COUNT], uint32_t launches[GSX_PASS_COUNT]);

#ifdef __cplusplus
}
#endif
#endif /* GSX_H */
