/*
 * fealess_hip.h -- C ABI of libfealess_hip.so: the MI355X (gfx950) implementation of the
 * rlvc/FEALESS hot path (LINEMOD detection + depth back-projection + ICP refinement).
 *
 * The reference has no FFI of its own: its boundary is the C++ surface of
 * CadReco/obj_reco_temp.h, CadReco/obj_reco_lmicp.h, linemod/linemod.hpp, ICP/ICP.h,
 * ICP/detection.h and ICP/depth_to_3d.h.  Every entry point below names the reference
 * function it replaces (paths relative to the reference root).  The C++ adapter in
 * fealess_amd/cadreco/ re-exposes the reference's own class surface on top of this ABI
 * (see INTEGRATION.md).
 *
 * Conventions: plain pointers and sizes only; no exceptions cross the ABI; every function
 * returns FL_OK (0) or a negative fl_status; fl_last_error() gives the text.  A context is
 * bound to one HIP device; calls on one context must be serialised by the caller (the
 * reference's CObjRecoLmICP is not thread-safe either, obj_reco_lmicp.h:37-51).  Work is queued
 * on the context's stream; functions that return results through host pointers synchronise
 * that stream before returning, functions that write device pointers do not.  The stream is
 * non-blocking (not ordered against the null stream): device buffers handed in (FL_MEM_DEVICE
 * frames, clouds, quantised images) must be complete when the call is made, or have been
 * produced on the stream given to fl_context_set_stream().
 * There is NO CPU fallback: without a HIP device fl_context_create fails.
 */
#ifndef FEALESS_HIP_H
#define FEALESS_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FL_ABI_VERSION 1

typedef enum {
  FL_OK = 0,
  FL_ERR_INVALID = -1,   /* bad argument (the reference returns ERROR_INVALID_PARAM / -1)       */
  FL_ERR_HIP = -2,       /* a HIP runtime call failed                                           */
  FL_ERR_ASSERT = -3,    /* the reference would hit a CV_Assert / cv::Exception here            */
  FL_ERR_OVERFLOW = -4,  /* a fixed-capacity device buffer overflowed (see fl_detector_limits)  */
  FL_ERR_NO_DEVICE = -5,
  FL_ERR_STATE = -6,     /* call order violated (e.g. matching before fl_detector_finalize)     */
  FL_ERR_NO_TEMPLATE = -7 /* fl_extract_template_pyramid: too few candidate features (addTemplate's -1) */
} fl_status;

typedef enum { FL_MEM_HOST = 0, FL_MEM_DEVICE = 1 } fl_mem;

/* ICP accumulation modes.
 *   FL_ICP_PARITY : the 15 centroid/covariance sums and the distance sum are accumulated as
 *                   sequential float32 chains in the reference's order (one lane per scalar),
 *                   so results are bit-identical to the reference's arithmetic (ICP.cpp:8-25,
 *                   731-735, 68-111).  Default.
 *   FL_ICP_FAST   : the same sums as parallel reductions (float32 per-thread partials of ~60
 *                   terms, fp64 tree across the workgroup, rounded once to float32): within 1e-4
 *                   of the EXACT sums' pose, not bit-identical to the reference's float32 chains.
 *                   Against the reference's float32 result the final pose differs by up to 1.1e-4
 *                   (R) / 1.1e-4 (T, relative to the object's distance) on 15 k-point clouds --
 *                   that is the reference's own summation noise (its float32 result is that far
 *                   from the exact sums); tests/test_gpu_icp.py asserts <= 2.5e-4 and "no farther
 *                   than the float32 result is from the exact sums".  Use FL_ICP_PARITY where the
 *                   1e-4 bar against the reference matters.  Timings of both: bench.py `icp_fast`.
 *   FL_ICP_POINT_TO_PLANE : opt-in extension with NO counterpart in the reference (SURVEY.md
 *                   section 8f rank 4): every iteration (the first included) pairs each model point
 *                   with its exact nearest reference point, gates the pair at distance
 *                   <= 3*dist_mean, and minimises sum (n_j . (R m_i + t - r_j))^2 linearised in
 *                   (omega, t): a 6x6 normal-equation system accumulated in fp64, solved by
 *                   Cholesky, omega -> R by Rodrigues.  Reference-cloud normals n_j come from the
 *                   organised scene depth (fl_detection / fl_recognize*) or from the caller
 *                   (fl_icp_point_to_plane).  Loop control, dist_mean / px_ratio and the pose
 *                   composition are those of icpCloudToCloud_Ex.  Validated against ground-truth
 *                   poses of synthetic scenes, not against the reference.                     */
typedef enum { FL_ICP_PARITY = 0, FL_ICP_FAST = 1, FL_ICP_POINT_TO_PLANE = 2 } fl_icp_mode;

typedef struct fl_context fl_context;
typedef struct fl_detector fl_detector;

/* linemod/linemod.hpp:32-43 (Feature), :47-58 (Template), :253-281 (Match) */
typedef struct { int32_t x, y, label; } fl_feature;
typedef struct {
  int32_t width, height, offset_x, offset_y, pyramid_level;
  int32_t feat_begin, feat_count;      /* range in the flat feature array handed over with it */
} fl_template;
typedef struct {
  int32_t x, y;
  float   similarity;
  int32_t class_idx;                   /* index of class_id in std::map (sorted) order */
  int32_t template_id;                 /* class-local id, as in the reference */
} fl_match;

/* CadReco/lotus_common.h:41-50 (TCamIntrinsicParam, without the unused distortion vector) */
typedef struct { int32_t width, height; double fx, fy, cx, cy; } fl_intrinsics;

/* result of icpCloudToCloud_Ex (ICP/ICP.cpp:617-809) */
typedef struct {
  float   R[9], T[3];
  float   dist_mean;                   /* the function's return value (-1 if < 3 points) */
  float   px_ratio;
  int32_t iters;                       /* value of `iter` on exit */
  int32_t n_corr_last;
} fl_icp_result;

/* result of detection() (ICP/detection.cpp:11-254) */
typedef struct {
  float   R_final[9], T_final[3];
  fl_icp_result icp;
  int32_t n_points;
  int32_t status;                      /* FL_OK or FL_ERR_ASSERT (rect outside the image, Q10) */
} fl_detection_result;

/* result of CObjRecoLmICP::Recognition (CadReco/obj_reco_lmicp.cpp:86-204) for one frame */
typedef struct {
  int32_t status;                      /* FL_OK, or the error Recognition would return */
  int32_t found;                       /* 0: vtResult empty; 1: one TObjRecoResult */
  int32_t n_matches;                   /* matches.size() after sort/unique */
  fl_match best;                       /* matches[0] */
  float   pose[16];                    /* TObjRecoResult::tWorld2Cam, row-major 4x4 */
  fl_detection_result det;
} fl_recognition_result;

typedef struct {
  float   matching_threshold;          /* m_matching_threshold, default 75 (obj_reco_lmicp.cpp:52) */
  int32_t icp_it_thr;                  /* default 10 (:53) */
  float   dist_mean_thr;               /* default 0.5 (:54) */
  float   dist_diff_thr;               /* default 0.01 (:55) */
  int32_t icp_mode;                    /* fl_icp_mode */
} fl_recognition_params;

/* ---- context ---------------------------------------------------------------------------- */
int  fl_abi_version(void);
int  fl_context_create(int device, fl_context **out);
void fl_context_destroy(fl_context *ctx);   /* with detectors still alive: deferred until the last fl_detector_destroy */
const char *fl_last_error(const fl_context *ctx);
/* use an existing hipStream_t (e.g. torch's current stream); NULL restores the context's own */
int  fl_context_set_stream(fl_context *ctx, void *hip_stream);
int  fl_context_synchronize(fl_context *ctx);
/* the stream the context queues its work on (a hipStream_t), its device, and a detector's context: what a host layer
 * that adds its own stream-ordered work (libfealess_mg.so: the RCCL collectives of the template-sharded path) needs */
void *fl_context_get_stream(fl_context *ctx);
int  fl_context_get_device(const fl_context *ctx);
fl_context *fl_detector_get_context(fl_detector *det);
/* Development / comparison switches.  They change how the work is scheduled, never a result: "scan_prune" (1; 0 = the scan adds
 * every feature everywhere, as the reference does), "scan_prune_mid" (bit mask of the 8-feature groups after which a modality
 * checks the pruning bound; -1 = built-in), "scan_prune_lanes" (1 = a lane of the scan whose own 16 positions miss the bound stops
 * loading; 0 = a wave stops as a whole or not at all), "scan_prune_step" (feature loads between two checks behind a modality's
 * first eight: 8, 4 or 2; 0 = 4 from 256 frames on, 8 below; bit g of scan_prune_mid enables the checks inside and at the end of
 * group g), "scan_first" (features of a modality's first piece, which is loaded without a check inside: 8, 12, 14 or 16; 0 = by
 * batch size, bank and threshold; its check goes by the bit of scan_prune_mid of the group that holds its last feature), "icp_wide" (-1 = by batch size; 0 / 1 force the 256- / 1024-thread ICP workgroup),
 * "icp_occ" (0 = by batch size; 4 / 5 force the 256-thread kernel built for that many workgroups per CU), "icp_idx16" (-1 = the 256-thread kernel of FL_ICP_PARITY holds pixel and order
 * indices in 16 bits wherever the crop's capacity is at most 65535 points; 0 = never; 1 = wherever the capacity allows, which is what -1
 * does: a larger crop runs the 32-bit build whatever the value), "icp_order" (1 = ICP
 * jobs dealt longest first; 0 = frame order), "icp_wg_per_cu" (0 = as many 256-thread ICP workgroups per CU as fit; 1 .. 3 = at
 * most that many, the rest of the CU left to the kernels of other streams), "pipeline_icp" (3; how fl_recognize_submit queues a batch: 0 = every
 * stage on the context's stream; 1 = the ICP stage on a second stream of the context, beside the next batch's LINEMOD stages; 2 / 3 =
 * the same with that stream at the highest / lowest priority of hipDeviceGetStreamPriorityRange), "frontend_chunk_rows" (0 = a
 * whole-image quantiser launch walks chunks of 120 rows where the batch still fills the device several times over, of 60 otherwise;
 * else that many rows), "scan_run" (0 = a wave of the coarse scan walks 8 work items where the batch still fills the device several
 * times over, and 4, 2 or 1 otherwise; else that many items: 1 is one item per wave), "refine_lds" (0 = a fine level is refined by the
 * kernel that reads a group of candidates' spread bytes from one LDS window where every window of the bank fits it and the batch
 * has a frame per CU, by the one that reads global memory otherwise; 1 = always the latter; 2 = the former wherever the windows
 * fit), "refine_lds_bytes" (0 = the compiled window budget of 65536 bytes; else a smaller one), "verify_fused" (0; 1 = fl_verify_batch renders
 * and scores every pose in the LDS of one workgroup, band by band, in place of the whole-image render and the scoring kernel),
 * "verify_fused_px" (0 = the compiled band budget of 36864 pixels; else a smaller one), and -- sampled by fl_detector_finalize -- "eager_frontend" (1 = finer pyramid
 * levels in full before the scan, the reference's order), "dev_poison" (1 = what the lazy path leaves uncomputed is filled
 * with 0xFF), "ws_pad" (extra bytes of frame-workspace stride).  Their INITIAL values are read once from the environment
 * when the context is created (FL_SCAN_PRUNE, FL_SCAN_PRUNE_MID (hex), FL_SCAN_PRUNE_LANES, FL_SCAN_PRUNE_STEP, FL_SCAN_FIRST, FL_ICP_WIDE, FL_ICP_OCC, FL_ICP_IDX16, FL_ICP_ORDER, FL_ICP_WG_PER_CU,
 * FL_PIPELINE_ICP, FL_FRONTEND_CHUNK_ROWS, FL_SCAN_RUN, FL_REFINE_LDS, FL_REFINE_LDS_BYTES, FL_VERIFY_FUSED, FL_VERIFY_FUSED_PX, FL_EAGER_FRONTEND, FL_DEV_POISON, FL_DEV_WS_PAD); nothing reads the environment after that, so a variable set in a host
 * process later on changes nothing.  Unknown names: FL_ERR_INVALID.
 * Accepted values: scan_prune, scan_prune_lanes, icp_order, eager_frontend, dev_poison {0, 1}; scan_prune_mid -1 .. 0xFF; scan_prune_step {0, 2, 4, 8}; scan_first {0, 8, 12, 14, 16}; icp_wide, icp_idx16 {-1, 0, 1};
 * icp_occ {0, 4, 5}; icp_wg_per_cu 0 .. 3; pipeline_icp 0 .. 3; frontend_chunk_rows 0 and the multiples of 60 up to 61440; scan_run 0 .. 64; refine_lds 0 .. 2; refine_lds_bytes 0 .. 65536; verify_fused {0, 1}; verify_fused_px 0 and 64 .. 36864; ws_pad 0 .. 16 MiB.  fl_context_set_option refuses any other value with
 * FL_ERR_INVALID and leaves the option as it was; an environment value outside its range keeps the built-in default. */
int  fl_context_set_option(fl_context *ctx, const char *name, long value);
int  fl_context_get_option(const fl_context *ctx, const char *name, long *value);

/* ---- detector = cup_linemod::Detector state resident in HBM -------------------------------- */
/* Detector::Detector(modalities, T_pyramid) (linemod.cpp:1348-1354). modalities is 1 or 2:
 * index 0 = ColorGradient, 1 = DepthNormal (getDefaultLINEMOD, linemod.cpp:1829-1835). */
int  fl_detector_create(fl_context *ctx, int modalities, int levels, const int *T_at_level,
                        fl_detector **out);
void fl_detector_destroy(fl_detector *det);
/* Detector::addSyntheticTemplate x n (linemod.cpp:1636-1642) + addPoseInfo (:1617-1622):
 * append a class of n_pyramids template pyramids, each levels*modalities fl_template ordered
 * [l*modalities + m].  poses13 (n_pyramids*13 floats, may be NULL) is the row-major 3x4 pose +
 * distance side table.  Classes are kept in std::map order of class_id. */
int  fl_detector_add_class(fl_detector *det, const char *class_id, int n_pyramids,
                           const fl_template *templates, const fl_feature *features,
                           int n_features, const float *poses13);
/* The per-template depth renders CObjRecoLmICP reads from <dir>/depth/<template_id>.png on
 * every frame (obj_reco_lmicp.cpp:156-157): uploaded once, w*h u16 in 0.1 mm each, for the
 * pyramids [first, first+count) of class class_idx.  src may be host or device memory.
 * class_idx is the class's place in std::map order of the ids added SO FAR: a class added later may sort in front of it.
 * A pyramid that never got a render is a missing depth/<id>.png: refining a match of it reports FL_ERR_STATE in that
 * result's status (found = 0), whether or not other pyramids of its class have renders. */
int  fl_detector_set_model_depths(fl_detector *det, int class_idx, int first, int count,
                                  const uint16_t *depth_01mm, int w, int h, int mem);
/* Freeze the bank for frames of w0 x h0 and at most max_batch frames per call; uploads the
 * flattened feature tables and allocates every per-frame workspace in HBM.  max_candidates is
 * the per-frame capacity of the candidate / match buffers (0 = default 65536). */
int  fl_detector_finalize(fl_detector *det, int w0, int h0, int max_batch, int max_candidates);
/* max_candidates: per-frame capacity of the coarse-candidate / match buffers.  > 0 (or 0 = 65536): an INITIAL size -- a frame
 * that needs more makes the synchronous entry points (fl_match_quantized / _frame / _frame_masked, fl_recognize_batch /
 * _batch_zoom / _topk / _batch_topk / _batch_instances) grow the buffers and run again, because the reference's vectors are unbounded
 * (linemod.cpp:1490-1504, 1575); the queued ones (fl_recognize_submit / fl_match_batch_submit) cannot replay a batch and
 * report FL_ERR_OVERFLOW in that frame's status (the other frames keep their results).  < 0: a hard cap of
 * -max_candidates, FL_ERR_OVERFLOW beyond it. */
/* For the QUEUED entry points (fl_recognize_submit, fl_match_batch_submit), which cannot replay a batch themselves: after
 * a batch in which a frame reported FL_ERR_OVERFLOW (fl_recognition_result.status, or FL_TOPK_OVERFLOW in the records of
 * fl_export_topk_batch), waits for the stream and grows the candidate buffers to what the fullest of the last batch's
 * first n_frames frames needs -- the std::vector growth of linemod.cpp:1490-1504 -- so that the caller can submit the
 * batch again.  *new_cap (may be NULL) = the capacity afterwards.  FL_ERR_OVERFLOW under a hard cap / without memory. */
int  fl_detector_grow_candidates(fl_detector *det, int n_frames, int *new_cap);
/* Detector::match's `class_ids` argument (linemod.hpp:319-327, linemod.cpp:1418-1434): n = 0 matches every
 * class (the default, and what Recognition passes); otherwise only the listed classes that exist.
 * Sticky until changed; may be called before or after fl_detector_finalize. */
int  fl_detector_set_class_filter(fl_detector *det, const char *const *class_ids, int n);
/* class_ids is treated as a SET.  The reference calls matchClass once per listed id, duplicates included
 * (linemod.cpp:1427-1433), and then relies on std::sort + adjacent std::unique (:1437-1439) to drop the repeated matches;
 * whether every repeat ends up adjacent is up to the (unstable) sort, so the duplicate-free list is one of its valid
 * outcomes -- the one returned here.  Unknown ids match nothing (:1429-1431). */
int  fl_detector_num_templates(const fl_detector *det);     /* Detector::numTemplates() :1652 */
int  fl_detector_num_classes(const fl_detector *det);

/* ---- stage entry points (each is the drop-in for one reference function) ------------------- */
/* quantizedOrientations + hysteresisGradient (linemod.cpp:230-385): bgr w*h*3 u8 -> w*h u8 */
int  fl_quantized_orientations(fl_context *ctx, const uint8_t *bgr, int w, int h,
                               float weak_threshold, uint8_t *dst, int mem);
/* quantizedNormals incl. medianBlur (linemod.cpp:595-685): depth w*h u16 (mm) -> w*h u8 */
int  fl_quantized_normals(fl_context *ctx, const uint16_t *depth, int w, int h,
                          int distance_threshold, int difference_threshold, uint8_t *dst, int mem);
/* cv::pyrDown on the colour image (linemod.cpp:443): w*h*3 -> (w/2)*(h/2)*3 */
int  fl_pyrdown_bgr(fl_context *ctx, const uint8_t *src, int w, int h, uint8_t *dst, int mem);
/* Detector::addTemplate (linemod.cpp:1579-1615) for the two default modalities ColorGradient(10, 63, 55) and
 * DepthNormal(2000, 50, 63, 2): quantized pyramids, extractTemplate per level and modality (:461-513, :747-825),
 * selectScatteredFeatures (:135-164), cropTemplates (:52-96).  mask: object mask (w0*h0 u8) or NULL.
 * Out (host): templates[levels * 2] ordered [l * 2 + m] with feat_begin = 63 * (l * 2 + m), features[levels * 2 * 63]
 * (template-relative after the crop), bb = {x, y, width, height} (may be NULL).  Returns FL_ERR_NO_TEMPLATE where
 * the reference returns -1.  The caller appends the pyramid to a class with fl_detector_add_class. */
int  fl_extract_template_pyramid(fl_context *ctx, const uint8_t *bgr, const uint16_t *depth, const uint8_t *mask, int w0,
                                 int h0, int levels, int mem, fl_template *templates, fl_feature *features, int bb[4]);
/* Detector::addTemplate for n_views views of w0 x h0, the same defaults and semantics as fl_extract_template_pyramid
 * (which is this call with n_views = 1).  bgr[v] (w0*h0*3 u8), depth[v] (w0*h0 u16, mm): host or device memory as
 * `mem` says.  mask: NULL (no view has a mask) or n_views pointers, each NULL (that view has none) or w0*h0 u8.
 * Out (host):
 *   templates[(v * levels + l) * 2 + m], feat_begin = 63 * that index (absolute in `features`)
 *   features[63 * ((v * levels + l) * 2 + m) + j]
 *   bb[4 * v .. 4 * v + 3] = {x, y, width, height}
 *   status[v] = FL_OK, or FL_ERR_NO_TEMPLATE where addTemplate returns -1: then the view's templates have
 *               feat_count = 0 and its bb = {0, 0, 0, 0}
 * Returns FL_OK when the batch ran, even if some views failed; FL_ERR_INVALID (nothing written) for n_views < 1, a null
 * array or image, or the sizes and levels fl_extract_template_pyramid refuses.
 * The call works through the batch in chunks of FL_EXTRACT_CHUNK_VIEWS views, each stage launched once per chunk.  A
 * chunk's device scratch (the context's, kept for later calls) is, per view and with px_l = (w0 >> l) * (h0 >> l):
 *   18 px_0 + 3 px_1 + sum_l (19 px_l + 16 next_pow2(px_l)) bytes (each array rounded up to 256 bytes)
 * -- 23.5 MB at 640x480 with two levels, 1.5 GB for a full chunk -- and 4 + 1768 levels bytes of pinned host memory. */
#define FL_EXTRACT_CHUNK_VIEWS 64
int  fl_extract_template_batch(fl_context *ctx, int n_views, const uint8_t *const *bgr, const uint16_t *const *depth,
                               const uint8_t *const *mask, int w0, int h0, int levels, int mem, fl_template *templates,
                               fl_feature *features, int32_t *bb, int32_t *status);
/* ---- training views of a triangle mesh (no counterpart in the reference, which reads views another tool rendered:
 * test/linemod_train.cpp:93-144, 180-255) ------------------------------------------------------------------------------
 * fl_render_views: a batched z-buffer rasteriser.  Inputs (host memory): vertices n_vertices * 3 f32 (object frame, mm);
 * normals n_vertices * 3 f32 or NULL (NULL: the face normal); colors n_vertices * 3 u8 BGR or NULL (NULL: FL_RENDER_GREY);
 * triangles n_triangles * 3 int32, 0-based; poses13 n_views * 13 f32 in the bank's layout (row-major [R|t] object -> camera
 * in mm; the 13th float is ignored, so one pose list feeds the renderer and template_pose); K->width x K->height is the
 * image size.  Pixel (u, v) is sampled along d = ((u - cx) * (1/fx), (v - cy) * (1/fy), 1) in float32, as depthTo3dNoMask
 * back-projects (ICP/depth_to_3d.cpp:103-121).  A triangle covers a pixel when that ray hits it at z > 0 (no clipping);
 * edge-on triangles cover nothing; a pixel exactly on an edge shared by two same-facing triangles belongs to one of them
 * (a top-left style tie rule); the nearest hit wins and equal depths go to the lower triangle index.
 * Outputs (each may be NULL, not all four), views back to back, row-major: bgr h*w*3 u8 = rint(albedo * clamp(|n.l|,
 * ambient, 1)) with albedo and normal interpolated perspective-correctly (the normal then normalised), 0 where nothing is
 * hit; depth h*w u16 = rint(z) in mm, saturated at 65535, 0 where nothing is hit; mask h*w u8 255 / 0; tri h*w int32, the
 * visible triangle or -1.  The arithmetic is float32 in the order written at the top of fealess_amd/csrc/fl_render.hip:
 * results do not depend on the schedule.  params: light direction in the camera frame (the way the light travels) and
 * ambient; NULL = a headlight (0, 0, 1) and FL_RENDER_AMBIENT.  mem: where the outputs are (host: the call synchronises;
 * device: queued on the context's stream).
 * FL_ERR_INVALID, nothing written: n_triangles or n_views < 1, n_vertices < 3, counts above FL_RENDER_MAX_PRIMS, an index
 * outside [0, n_vertices), a size <= 0 or above FL_RENDER_MAX_DIM, a non-finite or non-positive fx / fy (or non-finite
 * cx / cy), ambient outside [0, 1], a zero (or non-finite) light vector, a non-finite vertex / normal / pose, all outputs NULL.
 * Views go through in chunks of FL_RENDER_CHUNK_VIEWS views, fewer when w*h*views would pass FL_RENDER_CHUNK_PIXELS.  A
 * chunk's device scratch (the context's, kept for later calls): 8 bytes of depth key per pixel and view, plus 10 per pixel
 * and view staging for host outputs, plus the mesh -- max(2^25, w*h) * 18 bytes of images at most (604 MB up to 2^25
 * pixels per view, 1.2 GB for one 8192 x 8192 view; 64 views at 640x480: 157 MB of keys, 354 MB with host outputs). */
typedef struct { float light[3]; float ambient; } fl_render_params;
#define FL_RENDER_GREY 180            /* albedo of every channel when colors is NULL */
#define FL_RENDER_AMBIENT 0.2f        /* ambient when params is NULL */
#define FL_RENDER_MAX_DIM 8192
#define FL_RENDER_MAX_PRIMS (1 << 26)
#define FL_RENDER_CHUNK_VIEWS 64
#define FL_RENDER_CHUNK_PIXELS (1 << 25)
int  fl_render_views(fl_context *ctx, const float *vertices, const float *normals, const uint8_t *colors, int n_vertices,
                     const int32_t *triangles, int n_triangles, int n_views, const float *poses13, const fl_intrinsics *K,
                     const fl_render_params *params, int mem, uint8_t *bgr, uint16_t *depth, uint8_t *mask, int32_t *tri);
/* Camera poses on a view sphere, host only (like fl_nms).  Points: the icosahedron with a vertex at each pole, subdivided
 * `subdivisions` times (0..6: 10 * 4^s + 2 points, edge midpoints pushed onto the sphere); upper_hemisphere keeps the
 * points with object-frame z >= 0.  For each point s, distance d (distances_mm, each > 0) and in-plane angle: a camera at
 * d * s looking at the object origin, so t = (0, 0, d) and poses13[12] = d.  Image-up (camera -y) is object +z projected
 * onto the image plane; within 1e-5 of the poles (|s.z| > 1 - 1e-5) it is object +y.  In-plane angles: n_inplane angles
 * about the optical axis evenly spread over [-inplane_deg, +inplane_deg] (0 .. 180; one angle means 0), applied as
 * R = Rz(angle) * R0.  Order: point, then distance, then angle.  *n_views = the count; cap = 0 only queries it (poses13
 * may be NULL), otherwise cap must hold every view.  FL_ERR_INVALID (nothing written) for any other argument. */
int  fl_view_sphere(int subdivisions, int upper_hemisphere, const float *distances_mm, int n_distances, int n_inplane,
                    float inplane_deg, float *poses13, int cap, int *n_views);
/* cv::resize(src, dst, Size(dw, dh), 0, 0, INTER_LINEAR) as PrepareInputData applies it to frames
 * that are not 640 wide (obj_reco_lmicp.cpp:39-45, 229-249: TImage2Mat(..., true)); BGR8 and u16 */
int  fl_resize_linear_bgr8(fl_context *ctx, const uint8_t *src, int sw, int sh, uint8_t *dst, int dw, int dh, int mem);
int  fl_resize_linear_u16(fl_context *ctx, const uint16_t *src, int sw, int sh, uint16_t *dst, int dw, int dh, int mem);
/* ---- depth registration: raw sensor depth re-expressed in the colour camera (the reference leaves it to librealsense:
 * rs2::align(RS2_STREAM_COLOR) on every frameset in front of Recognition, test/linemod_recon.cpp:38-51, test/linemod_acq.cpp:24-42)
 * Every entry point that takes a depth frame assumes it is pixel-aligned with the colour frame and expressed in the colour
 * camera's K.  fl_register_depth_batch makes n_frames such frames from what the depth sensor delivers, on the device.
 * K_depth->width x height is the size of every input frame (wd x hd), K_color->width x height of every output frame
 * (wc x hc).  depth and out are host arrays of n_frames pointers; mem says where the pixels of both live: host -- the call
 * stages them and synchronises; device -- queued on the context's stream, no wait (an output frame must not overlap an input
 * frame).  Depth is u16 millimetres, 0 = no measurement; the output uses the same convention.  depth_to_color: X_colour =
 * R * X_depth + t in mm, R row-major.  Lens distortion is out of scope, as for fl_intrinsics everywhere.
 * Arithmetic: everything is float32, one IEEE operation per operator, in the order written ('/' correctly rounded).
 *   host      fx_d = (float)K_depth->fx and so on for the other intrinsics of both cameras; ifx = 1.0f / fx_d, ify = 1.0f / fy_d
 *   points    a depth pixel (u, v) with d == 0 contributes nothing.  Otherwise z = (float)d and three points are formed, A, B
 *             and C for o = -0.5f, +0.5f, 0 (the same o on both axes):
 *               x = (((float)u + o) - cx_d) * ifx * z,  y = (((float)v + o) - cy_d) * ify * z
 *               X = ((R[0]*x + R[1]*y) + R[2]*z) + t[0];  Y uses row 1 and t[1], Z row 2 and t[2]
 *   reject    the pixel is skipped unless Z_A > 0, Z_B > 0 and Z_C >= 0.5f
 *   value     val = (uint16)fminf(rintf(Z_C), 65535.f): the transformed depth, not the source depth
 *   footprint p = X / Z * fx_c + cx_c and q = Y / Z * fy_c + cy_c, for A and B; the pixel is skipped if any of the four is
 *             not finite.  x0 = ceilf(fminf(pA, pB)), x1 = floorf(fmaxf(pA, pB)); y0, y1 likewise from q.  Each is clamped in
 *             float to [-1, wc] (y: [-1, hc]) before the conversion to int; then x0 = max(x0, 0) and x1 = min(x1, wc - 1,
 *             x0 + FL_REGISTER_MAX_SPLAT - 1), y the same.  An empty range writes nothing.  With equal cameras and identity
 *             extrinsics the footprint is the pixel itself, so the output equals the input.
 *   z-buffer  every output pixel of a footprint takes the minimum of the values that land on it; a pixel nothing lands on
 *             is 0.  The minimum is order-independent: the result does not depend on the schedule.
 *   cracks    with fill_cracks = 1, evaluated on the unfilled image E, never on filled values.  A pixel with E == 0: if its
 *             left and right neighbours both exist and are non-zero it takes their minimum; otherwise, if its upper and lower
 *             neighbours both exist and are non-zero, it takes their minimum; otherwise it stays 0.
 * FL_ERR_INVALID, before any HIP call, nothing written: n_frames < 1; a NULL argument other than params, or a NULL entry of
 * either pointer list; mem outside {0, 1}; a size <= 0 or above FL_RENDER_MAX_DIM; a non-finite or non-positive fx or fy, or a
 * non-finite cx or cy, of either camera (as doubles or as floats); a non-finite entry of R or t; an R that is not a rotation (an
 * element of R^T R - I above 1e-3 in magnitude, or det <= 0); fill_cracks outside {0, 1}.
 * Frames go through in chunks of FL_REGISTER_CHUNK_FRAMES, fewer when the pixels of a chunk's input or output frames would pass
 * FL_RENDER_CHUNK_PIXELS; a chunk is one clear of its z-buffer and two kernel launches.  Device scratch (the context's, kept
 * for later calls, independent of n_frames): 4 bytes per output pixel of a chunk, plus 2 bytes per input and per output pixel
 * of a chunk for host frames -- 79 MB at 640x480, 157 MB with host frames.  Nothing is allocated once the scratch has that size. */
typedef struct { float R[9]; float t[3]; } fl_extrinsics;     /* row-major; X_colour = R * X_depth + t, mm */
typedef struct { int32_t fill_cracks; } fl_register_params;   /* NULL = {1} */
#define FL_REGISTER_MAX_SPLAT 8
#define FL_REGISTER_CHUNK_FRAMES 64
int  fl_register_depth_batch(fl_context *ctx, int n_frames, const uint16_t *const *depth, int mem,
                             const fl_intrinsics *K_depth, const fl_intrinsics *K_color,
                             const fl_extrinsics *depth_to_color, const fl_register_params *params,
                             uint16_t *const *out);
/* The checks fl_register_depth_batch makes of its cameras, extrinsics and parameters, alone and on the host (like fl_nms): FL_OK,
 * or FL_ERR_INVALID for a camera, depth_to_color or params that call refuses.  Each argument may be NULL: it is not checked. */
int  fl_register_check(const fl_intrinsics *K_depth, const fl_intrinsics *K_color, const fl_extrinsics *depth_to_color,
                       const fl_register_params *params);
/* spread + computeResponseMaps + linearize x8 (linemod.cpp:950-1088) for one quantized image:
 * out = 8 * fl_lm_label_stride(w,h,T) bytes, layout [label][T*T grid][(w/T)*(h/T)] + zero pad */
size_t fl_lm_label_stride(int w, int h, int T);
int  fl_build_linear_memories(fl_context *ctx, const uint8_t *quantized, int w, int h, int T,
                              uint8_t *out, int mem);
/* cup_d2pc::depthTo3d, CV_16UC1 depth (ICP/depth_to_3d.cpp:190-221): out w*h*3 f32 (metres) */
int  fl_depth_to_3d(fl_context *ctx, const uint16_t *depth, int w, int h, double fx, double fy,
                    double cx, double cy, float *out, int mem);
/* icpCloudToCloud_Ex (ICP/ICP.cpp:617-809): clouds are n*3 f32 (mm). res is host memory. */
int  fl_icp(fl_context *ctx, const float *ref, int n_ref, const float *model, int n_model,
            int icp_it_thr, float dist_mean_thr, float dist_diff_thr, int icp_mode, int mem,
            fl_icp_result *res);
/* FL_ICP_POINT_TO_PLANE on caller-supplied clouds: ref_normals is n_ref*3 f32 (unit normals of the
 * reference cloud; an all-zero normal excludes that point from the 6x6 system).  fl_icp itself
 * refuses FL_ICP_POINT_TO_PLANE (FL_ERR_INVALID): it has no normals to work with.  No
 * counterpart in the reference. */
int  fl_icp_point_to_plane(fl_context *ctx, const float *ref, const float *ref_normals, int n_ref,
                           const float *model, int n_model, int icp_it_thr, float dist_mean_thr,
                           float dist_diff_thr, int mem, fl_icp_result *res);
/* detection() (ICP/detection.cpp:11-254): two w*h u16 depth images in mm. res is host memory. */
int  fl_detection(fl_context *ctx, const uint16_t *model_depth, const uint16_t *scene_depth,
                  int w, int h, const fl_intrinsics *K, const int rect_model[4],
                  const int rect_ref[4], int icp_it_thr, float dist_mean_thr, float dist_diff_thr,
                  const float r_match[9], const float t_match[3], int icp_mode, int mem,
                  fl_detection_result *res);

/* ---- Detector::match (linemod.cpp:1356-1441) ------------------------------------------------ */
/* From caller-supplied quantized images (what Modality::process + quantize would return):
 * quantized[l*modalities + m] is (w0>>l)*(h0>>l) u8.  out/n_total are host memory; matches come
 * back sorted (similarity desc, template_id asc, then class, y, x asc -- one valid outcome of
 * the reference's unstable std::sort) and de-duplicated as std::unique with Match::operator==. */
int  fl_match_quantized(fl_detector *det, const uint8_t *const *quantized, int mem,
                        float threshold, fl_match *out, int cap, int *n_total);
/* From a BGR8 + depth16 frame with the default modality parameters (linemod.cpp:515-519,827-832) */
int  fl_match_frame(fl_detector *det, const uint8_t *bgr, const uint16_t *depth, int mem,
              float threshold, fl_match *out, int cap, int *n_total);
/* Detector::match's optional `masks` argument (linemod.hpp:319-327, linemod.cpp:1364-1379): masks is
 * NULL (empty vector) or an array of `modalities` pointers to w0*h0 u8 images in `mem`, each of
 * which may be NULL (empty Mat).  A level-l pixel is kept where the l-times NN-halved mask is
 * non-zero (linemod.cpp:445-459, 733-745). */
int  fl_match_frame_masked(fl_detector *det, const uint8_t *bgr, const uint16_t *depth,
                           const uint8_t *const *masks, int mem, float threshold, fl_match *out,
                           int cap, int *n_total);
/* Detector::match for a batch of frames (the reference is called once per camera frame, linemod.cpp:1356-1441;
 * test/linemod_recon.cpp:43-80): front-end and match of n_frames frames are queued on the context's stream, the sorted
 * match lists stay in HBM.  fl_match_batch_collect waits and copies frame `frame`'s list out (same order and
 * de-duplication as fl_match_frame); fl_export_topk reads them on the device. */
int  fl_match_batch_submit(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth,
                           int mem, float threshold);
int  fl_match_batch_collect(fl_detector *det, int frame, fl_match *out, int cap, int *n_total);
/* similarity + addSimilarities (linemod.cpp:1130-1214,1322-1338) for pyramids [first,first+count)
 * at the coarsest level of the frame last passed to fl_match_*: out = count * (W_T*H_T) u16 (host) */
int  fl_similarity_maps(fl_detector *det, int first, int count, uint16_t *out);
/* the quantized images of the frame last passed to fl_match (Detector::match's optional
 * quantized_images output, linemod.cpp:1411-1412): levels*modalities images back to back (host) */
int  fl_last_quantized(fl_detector *det, uint8_t *out);

/* ---- CObjRecoLmICP::Recognition (CadReco/obj_reco_lmicp.cpp:86-204), batched ---------------- */
/* n_frames frames of w0 x h0 (already 640 wide), all stages on the GPU with
 * no host round trip between LINEMOD and ICP.  bgr[i], depth[i] are host or device pointers
 * (all the same kind).  results is host memory.  Frames are independent; results[i] equals what
 * Recognition() returns for frame i. */
int  fl_recognize_batch(fl_detector *det, int n_frames, const uint8_t *const *bgr,
                        const uint16_t *const *depth, int mem, const fl_intrinsics *K,
                        const fl_recognition_params *params, fl_recognition_result *results);
/* PrepareInputData's zoom + Recognition (obj_reco_lmicp.cpp:229-249, 39-45): n_frames frames of src_w x src_h are
 * resized (cv::resize INTER_LINEAR semantics, as fl_resize_linear_*) to the detector's w0 x h0 on the device and
 * recognised from HBM without a host round trip.  K is passed through as the reference passes it. */
int  fl_recognize_batch_zoom(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth,
                             int src_w, int src_h, int mem, const fl_intrinsics *K, const fl_recognition_params *params,
                             fl_recognition_result *results);
/* same, but only queues the work; fl_recognize_collect() waits and copies the results out.  Lets the caller overlap two
 * contexts / batches.
 * Two batches are in flight inside one detector: the LINEMOD stages (staging, front-end, match, refine, sort) are queued on the
 * context's stream and the ICP stage, with the copy of the results, on a second stream the context owns, so the LINEMOD
 * stages of batch i+1 run beside the ICP launch of batch i (option "pipeline_icp").  fl_context_synchronize and
 * fl_recognize_collect wait for both streams, and every other entry point orders itself behind both.  Everything is queued on
 * ONE stream, in order, when the caller gave the context a stream (fl_context_set_stream: synchronising that stream finishes
 * the work), when device frames lie at irregular addresses, or with pipeline_icp = 0.  Results are the same either way.
 * fl_recognize_collect returns the LATEST submitted batch.  fl_recognize_collect_previous returns the batch submitted BEFORE
 * the latest fl_recognize_submit and waits only for that batch, so that
 *     submit(0); for i in 1..: submit(i); collect_previous(i-1); ...; collect(last)
 * keeps two batches in flight and still hands every batch's results over.  It returns FL_ERR_STATE when there is no such
 * batch: fewer than two submits, the batch already collected (by either call), or any other entry point of the detector
 * called since that batch was submitted.  It leaves the stage times as they are. */
int  fl_recognize_submit(fl_detector *det, int n_frames, const uint8_t *const *bgr,
                         const uint16_t *const *depth, int mem, const fl_intrinsics *K,
                         const fl_recognition_params *params);
int  fl_recognize_collect(fl_detector *det, int n_frames, fl_recognition_result *results);
int  fl_recognize_collect_previous(fl_detector *det, int n_frames, fl_recognition_result *results);

/* ---- multi-GPU support: top-k records for the all-gather ------------------------------------ */
/* Multi-hypothesis recognition (the pipeline ICP/NMS.cpp + obj_data.h sketch): the refinement of
 * Recognition() (obj_reco_lmicp.cpp:111-197) for the first k matches of ONE frame, k ICP workgroups in one launch.
 * results[r] (host, r < *n_results = min(k, matches)) has the same content fl_recognize_batch gives for matches[0];
 * a hypothesis whose crop leaves the image has found = 0 and status = FL_ERR_ASSERT. */
int  fl_recognize_topk(fl_detector *det, const uint8_t *bgr, const uint16_t *depth, int mem, const fl_intrinsics *K,
                       const fl_recognition_params *params, int k, fl_recognition_result *results, int *n_results);
/* The same for a batch (n_frames * k ICP workgroups in one launch): results[f * k + r] (host) is hypothesis r of
 * frame f, n_results[f] = min(k, matches of frame f).  Frame pointers as for fl_recognize_batch. */
int  fl_recognize_batch_topk(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth,
                             int mem, const fl_intrinsics *K, const fl_recognition_params *params, int k,
                             fl_recognition_result *results, int *n_results);
/* nonMaximumSuppression (ICP/NMS.cpp:6-40) over refined hypotheses in list order: winners[g] = index of the
 * hypothesis representing group g (translation closer than th_obj_dist to the group's current best). Host only. */
int  fl_nms(const fl_recognition_result *objs, int n, float th_obj_dist, int *winners, int *n_winners);
/* ---- multi-instance recognition: group the match list on the device, refine a few members of each group ----------
 * The sorted match list is not spread over the objects in a frame: every instance contributes a run of near-ties
 * (neighbouring positions, neighbouring views), so the first k matches may all belong to one object.  The entry points
 * below group a frame's list in image space BEFORE the refinement and refine only the first few members of each group.
 *
 * Grouping -- greedy over the list in its sorted order, all in integers: for match i with template pyramid g, the doubled
 * centre of the rectangle Recognition() crops (templates[0], obj_reco_lmicp.cpp:129-132) is
 *   c2 = (2 x + width0(g), 2 y + height0(g)).
 * Match i joins the FIRST group in creation order whose leader has the same class_idx and
 *   (c2x - leader.c2x)^2 + (c2y - leader.c2y)^2 < (2 min_dist_px)^2          (64-bit, strict)
 * -- distances are taken to the leader only -- or else founds a new group while fewer than max_instances exist, or else
 * is dropped (group -1).  Members keep list order inside their group.
 * Refinement -- the first hyp_per_instance members of each group, each exactly as fl_refine_matches refines a match.
 * Pick -- nonMaximumSuppression's choice (ICP/NMS.cpp:6-40, as fl_nms states it) among a group's refined members with
 * found = 1, in list order: o = the first of them, size_th = (int)((float)n_points[o] * 0.85); a later member j replaces
 * o when n_points[j] > size_th && dist_mean[j] < dist_mean[o].  A group without a found member reports its leader
 * (found = 0).  Groups are reported in creation order, which is the order fl_nms reports its winners in. */
typedef struct {
  int32_t max_instances;               /* 1..64: groups per frame                         */
  int32_t min_dist_px;                 /* 1..2^30: group radius, pixels of the w0 x h0 frame */
  int32_t hyp_per_instance;            /* 1..64: members refined per group                */
} fl_instance_params;
typedef struct {
  fl_recognition_result reco;          /* the picked hypothesis; reco.n_matches = the frame's */
  int32_t rank;                        /* its index in the frame's match list */
  int32_t n_members, n_refined, reserved;
} fl_instance_result;
/* The grouping alone, on a caller-supplied list of n >= 0 matches (class-local template ids of THIS detector):
 * group_of[i] = group of match i or -1, group_size[g] for g < ip->max_instances (0 beyond *n_groups), *n_groups.
 * FL_MEM_HOST: host arrays, computed on the host from the classes added so far (no device work, the detector need not be
 * finalized); a match whose class or template is not on the detector: FL_ERR_INVALID, nothing written.
 * FL_MEM_DEVICE: matches, group_of, group_size and n_groups (one int) are device memory; the grouping kernel is queued on
 * the context's stream (finalized detector, no synchronisation); there a match that is not on the detector gets -1. */
int  fl_group_matches(fl_detector *det, const fl_match *matches, int n, int mem, const fl_instance_params *ip,
                      int32_t *group_of, int32_t *group_size, int32_t *n_groups);
/* Recognition() returning every instance in the frame: front-end and Detector::match of the batch, the grouping kernel
 * (one workgroup per frame), ONE ICP launch over n_frames * max_instances * hyp_per_instance jobs (the absent ones exit at
 * once), the pick kernel, one copy to the host -- nothing touches the host in between.  results[f * max_instances + g]
 * for g < n_instances[f] (the rest zeroed); n_dropped[f] = matches of frame f that found no group.  Needs both
 * modalities.  A frame without matches has n_instances = 0.  With {1, any, 1} results[f].reco is what fl_recognize_batch
 * returns.  The ICP workspaces come from the context's scratch, one per job SLOT -- n_frames * max_instances *
 * hyp_per_instance of them, absent jobs included, each about 86 bytes per pixel of the largest template rectangle (2.2 MB at
 * 160 x 160) -- and the call is refused with FL_ERR_INVALID beyond 2^20 slots or 96 GB: at {8, ., 4} and 160 x 160 templates that
 * is about 1300 frames per call; larger batches go through in several calls. */
int  fl_recognize_batch_instances(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth,
                                  int mem, const fl_intrinsics *K, const fl_recognition_params *params,
                                  const fl_instance_params *ip, fl_instance_result *results, int32_t *n_instances,
                                  int32_t *n_dropped);
/* ---- tracking: follow recognised objects from frame to frame against the CAD mesh (no counterpart in the reference,
 * which ships a 2-D KCF box tracker it never wired in: test/linemod_acq.cpp:108-150) ------------------------------------
 * A track is one (object pose, depth frame) pair.  One step of one track: render the mesh at the track's pose, crop both
 * depth images around the render, run detection() (ICP/detection.cpp:11-254) with r_match, t_match = that pose, take the
 * composed pose.  No LINEMOD front-end, no scan, no template bank.  Several tracks may name one frame, many frames may be
 * tracked in one call; time stepping is the caller's loop (feed results[t].pose back in as poses13).
 *
 * fl_tracker_create uploads the mesh (as fl_render_views takes it: vertices n * 3 f32 in mm, triangles 0-based) and
 * allocates every device buffer once -- max_frames frame slots of w * h u16, max_tracks render images, the rasteriser's
 * depth keys for one chunk of views, max_tracks ICP workspaces for crops of up to max_crop_px pixels (about 86 bytes per
 * pixel), the small per-track arrays; fl_track_batch allocates nothing.  FL_ERR_INVALID: null pointers, the mesh limits
 * of fl_render_views, w or h outside 1..FL_RENDER_MAX_DIM, max_frames or max_tracks outside 1..FL_TRACK_MAX_TRACKS,
 * max_crop_px outside [1, min(w * h, FL_TRACK_MAX_CROP_PX)] (the crop sizes the ICP's organised search is exact for without
 * its slow paths), more than 96 GB of ICP workspaces.  A tracker does not keep its context alive: destroy it before the context.
 *
 * fl_track_batch: depth[i], i < n_frames, are w * h u16 in mm, host or device memory as `mem` says; frame_of_track[t] and
 * poses13 (the bank's layout, row-major [R|t] object -> camera in mm, the 13th float ignored) are host memory, as is
 * results.  params == NULL: the defaults below.  K is the SCENE camera (K->width x K->height must be w x h).  Everything
 * is queued on the context's stream and the call waits once, at the end.  Per pass:
 *   render   the mesh at every track's pose, depth only, at w x h with K = 608 / 608 / 320 / 240 whatever the scene's K is:
 *            detection() back-projects the model image with exactly that K (initInternalMat, ICP/common.cpp:358;
 *            ICP/detection.cpp:35-36), so the model cloud is metrically right for any scene camera.
 *   rects    (integers) [x0, x1] x [y0, y1] = the bounding box of the render's non-zero pixels; grown by margin_px on every
 *            side and clamped to the image = rect_model {x, y, w, h}.  rect_ref = rect_model shifted by
 *              dx = (int)rint((fx - 608) * (tx / tz) + (cx - 320)),  dy = (int)rint((fy - 608) * (ty / tz) + (cy - 240))
 *            (fp64, one IEEE operation per operator, (tx, ty, tz) = the pose's translation; 0 when the scene K is the model
 *            K; a shift that is not finite or beyond 2^20 pixels counts as out of view), then clipped to the image, and the
 *            same clip applied to rect_model, so both keep one size and their alignment.  The render's depths inside
 *            rect_model are multiplied by 10 (saturating at 65535): the recognition branch of the ICP reads model images in
 *            0.1 mm through rint(d * 0.1f), which gives back the millimetres for every depth <= 6553 mm.
 *   ICP      one launch over the n_tracks slots, exactly the refinement fl_refine_matches runs.
 *   finish   a track is LOST when detection() found nothing (fewer than 3 paired points: icp.dist_mean < 0) or one of the two
 *            optional gates says so; otherwise pose = detection()'s composition, R = R_icp R_in, T = R_icp (t_in + (c_ref -
 *            c_mod)) + T_icp, which is also the next pass's input.  Passes never touch the host.
 * A track whose render is empty (behind the camera, out of view) or whose rectangles clip to nothing: tracked = 0, status
 * FL_OK, rects and det zero.  A track whose crop has more than max_crop_px pixels: tracked = 0, status FL_ERR_OVERFLOW, the
 * rects reported.  A track that is not tracked in some pass stays so in the later passes and reports the pose it came in
 * with; the other tracks are not affected.  Returns FL_OK when the batch ran, whatever the tracks' fates.
 * FL_ERR_INVALID, nothing written: null pointers, n_frames outside 1..max_frames, n_tracks outside 1..max_tracks, a
 * frame_of_track outside [0, n_frames), a non-finite pose or K, fx or fy <= 0, K's size not w x h, passes outside 1..4,
 * margin_px outside 0..FL_RENDER_MAX_DIM, icp_it_thr < 0, a non-finite threshold, an unknown icp_mode or mem.
 * Limit: both crops have the same pixel size, so a scene camera whose focal length is far from 608 sees the object at
 * another pixel size than the render and the paired compaction of detection() pairs the wrong pixels; the reference's own
 * Recognition() has the same limit (its templates' renders are at 608 too). */
typedef struct fl_tracker fl_tracker;
typedef struct {
  int32_t margin_px;                   /* crop = the render's bounding box grown by this on every side; default 12 */
  int32_t passes;                      /* render + ICP repeated, pass p+1 starting from pass p's pose; 1..4; default 1 */
  int32_t icp_it_thr;                  /* as fl_recognition_params; default 10 */
  float   dist_mean_thr, dist_diff_thr;   /* defaults 0.5, 0.01 */
  int32_t icp_mode;                    /* default FL_ICP_POINT_TO_PLANE */
  float   max_dist_mean;               /* > 0: a result with icp.dist_mean above it is "lost"; <= 0: no test */
  float   min_px_ratio;                /* > 0: a result with icp.px_ratio below it is "lost"; <= 0: no test */
} fl_track_params;
typedef struct {
  int32_t status;                      /* FL_OK; FL_ERR_OVERFLOW: the crop has more pixels than max_crop_px */
  int32_t tracked;                     /* 1: pose is the new pose; 0: lost, pose = the input pose */
  int32_t rect_model[4], rect_ref[4];  /* of the last pass that ran */
  float   pose[16];                    /* row-major 4x4 like fl_recognition_result::pose */
  fl_detection_result det;             /* of the last pass that ran */
} fl_track_result;
#define FL_TRACK_MAX_TRACKS (1 << 16)
#define FL_TRACK_MAX_CROP_PX ((1 << 24) - 4)
#define FL_TRACK_MAX_PASSES 4
int  fl_tracker_create(fl_context *ctx, const float *vertices, int n_vertices, const int32_t *triangles, int n_triangles,
                       int w, int h, int max_frames, int max_tracks, int max_crop_px, fl_tracker **out);
void fl_tracker_destroy(fl_tracker *trk);
int  fl_track_batch(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem,
                    int n_tracks, const int32_t *frame_of_track, const float *poses13,
                    const fl_intrinsics *K, const fl_track_params *params, fl_track_result *results);
/* ---- several meshes on one tracker ---------------------------------------------------------------------------------------
 * fl_tracker_create_meshes is fl_tracker_create for n_meshes meshes (fl_tracker_create IS this call with one mesh): each mesh
 * as fl_tracker_create takes it, a triangle's indices inside its own mesh's vertices.  The meshes share every other buffer of
 * the tracker -- frame slots, render images, depth keys, ICP workspaces -- so device memory grows by the extra meshes and a
 * table of n_meshes ranges only.  FL_ERR_INVALID on top of fl_tracker_create's refusals: meshes NULL, n_meshes outside
 * 1..FL_TRACK_MAX_MESHES, a mesh that breaks fl_tracker_create's mesh rules (the error text says which mesh), more than
 * FL_RENDER_MAX_PRIMS vertices or triangles over all meshes.  All of them precede the device check (FL_ERR_NO_DEVICE).
 * fl_tracker_num_meshes: the number of meshes (FL_ERR_INVALID for NULL).
 * fl_track_batch_meshes, fl_verify_batch_meshes and fl_track_batch_verified_meshes (the latter two are declared below, after
 * the calls they extend) are fl_track_batch, fl_verify_batch and fl_track_batch_verified with one more argument: mesh_of_track
 * / mesh_of_pose, host memory, the mesh of every track or pose, each in [0, n_meshes); NULL: mesh 0 for all of them.  The three
 * calls without the argument are these with NULL, so on a tracker of several meshes they use mesh 0.  An entry out of range:
 * FL_ERR_INVALID, nothing written, before the first HIP call like the other argument checks.
 * CONTRACT: the record of a track or pose whose mesh is m is, byte for byte, the record the call without the argument returns
 * for that pose and frame on a tracker created from mesh m alone (a key's tie rule "equal depths go to the lower triangle
 * index" counts triangles inside mesh m).  Groups (group_first) may mix meshes; the pick compares records as it always does. */
typedef struct {
  const float   *vertices;             /* n_vertices * 3, mm */
  const int32_t *triangles;            /* n_triangles * 3, 0-based into this mesh's vertices */
  int32_t n_vertices, n_triangles;
} fl_mesh;
#define FL_TRACK_MAX_MESHES 256
int  fl_tracker_create_meshes(fl_context *ctx, const fl_mesh *meshes, int n_meshes, int w, int h,
                              int max_frames, int max_tracks, int max_crop_px, fl_tracker **out);
int  fl_tracker_num_meshes(const fl_tracker *trk);
int  fl_track_batch_meshes(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem,
                           int n_tracks, const int32_t *frame_of_track, const int32_t *mesh_of_track, const float *poses13,
                           const fl_intrinsics *K, const fl_track_params *params, fl_track_result *results);
/* ---- verification: is the object where a pose says it is?  (No counterpart in the reference, whose check is visual.) -----
 * The ICP's dist_mean and px_ratio are measured over the point pairs the ICP kept: they say how well the kept points fit,
 * not whether the object is there.  fl_verify_batch renders the tracker's mesh at every pose and lays the render over the
 * pose's depth frame, pixel by pixel.  depth, mem, frame_of_pose, poses13 and K are as fl_track_batch takes them; results
 * (n_poses records) is host memory; params == NULL: the defaults below.  Everything is queued on the context's stream (after
 * a detector's pipelined ICP stage on that context) and the call waits once, at the end; it allocates nothing.  It writes the
 * tracker's frame slots and render images, as fl_track_batch does: the caller serialises the two, as everything on a context.
 *   render   the mesh at every pose, depth only, at w x h with the SCENE camera (float)K->fx, (float)K->fy, (float)K->cx,
 *            (float)K->cy -- not the model camera fl_track_batch renders with: here a render pixel and the frame pixel
 *            under it are one ray, so there is no rectangle shift and no assumption about the image size.
 *   score    (integers) per pixel, r = the render and s = the frame in mm: r == 0 is not counted.  Otherwise the pixel
 *            counts in n_model and, with d = (int)s - (int)r, in exactly one of
 *              n_missing  s == 0              the frame has no depth there
 *              n_inlier   |d| <= tau_mm       supported; |d| is added to sum_abs_inlier
 *              n_front    d < -tau_mm         the scene is nearer: something stands in front of the object, which may be
 *              n_behind   d >  tau_mm         the camera sees through the object, which may not be
 *            so n_model == n_missing + n_inlier + n_front + n_behind.  rect = {x0, y0, x1 - x0 + 1, y1 - y0 + 1} of the
 *            inclusive bounding box [x0, x1] x [y0, y1] of the r != 0 pixels.
 *   finish   inlier_ratio = (float)n_inlier / (float)n_model, behind_ratio = (float)n_behind / (float)n_model, one float32
 *            division each, both 0 when n_model == 0.  accepted = 1 when n_model >= min_model_px and (min_inlier_ratio <= 0
 *            or inlier_ratio >= min_inlier_ratio) and (max_behind_ratio <= 0 or behind_ratio <= max_behind_ratio), else 0.
 *            An empty render (out of view, behind the camera): status FL_OK, accepted 0, rect, counts and ratios zero.
 *   pick     group g is the poses group_first[g] .. group_first[g + 1] - 1 (group_first: n_groups + 1 entries, host memory,
 *            non-decreasing, group_first[0] == 0, group_first[n_groups] == n_poses; a group may be empty and its members may
 *            look at different frames).  best = 1 for at most one pose of a group: among the accepted ones the pose with
 *            the largest n_inlier / n_model, compared exactly -- a beats b when (int64)n_inlier_a * n_model_b >
 *            (int64)n_inlier_b * n_model_a -- and a tie goes to the lower index; a group without an accepted pose has no
 *            best.  group_first == NULL (n_groups is ignored): every pose is its own group, best = accepted.
 * Returns FL_OK when the batch ran, whatever the poses' fates; status is FL_OK in every record then.
 * FL_ERR_INVALID, nothing written: null pointers, n_frames outside 1..max_frames, n_poses outside 1..max_tracks, a
 * frame_of_pose outside [0, n_frames), a non-finite pose or K, fx or fy <= 0 (as doubles or as floats), K's size not w x h,
 * with group_first: n_groups outside 1..max_tracks or a group_first that breaks the rules above, tau_mm outside 0..65535,
 * min_model_px < 1, a non-finite threshold, an unknown mem.  These checks precede the first HIP call. */
typedef struct {
  int32_t tau_mm;                      /* inlier band in mm, 0..65535; default 10 */
  int32_t min_model_px;                /* accepted only if n_model >= this; >= 1; default 1 */
  float   min_inlier_ratio;            /* > 0: accepted only if inlier_ratio >= it; <= 0: no test (default 0) */
  float   max_behind_ratio;            /* > 0: accepted only if behind_ratio <= it; <= 0: no test (default 0) */
} fl_verify_params;
typedef struct {
  int32_t status, accepted, best;
  int32_t rect[4];                     /* x, y, w, h of the render's non-zero pixels; zeros when empty */
  int32_t n_model, n_missing, n_inlier, n_front, n_behind;
  int64_t sum_abs_inlier;              /* sum of |scene - render| in mm over the inliers */
  float   inlier_ratio, behind_ratio;
} fl_verify_result;                    /* 64 bytes */
int  fl_verify_batch(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem,
                     int n_poses, const int32_t *frame_of_pose, const float *poses13,
                     int n_groups, const int32_t *group_first, const fl_intrinsics *K,
                     const fl_verify_params *params, fl_verify_result *results);
/* with a mesh per pose: see "several meshes on one tracker" above for mesh_of_pose and the contract */
int  fl_verify_batch_meshes(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem,
                            int n_poses, const int32_t *frame_of_pose, const int32_t *mesh_of_pose, const float *poses13,
                            int n_groups, const int32_t *group_first, const fl_intrinsics *K,
                            const fl_verify_params *params, fl_verify_result *results);
/* ---- verified tracking: fl_track_batch whose `tracked` is the verification's ---------------------------------------------------
 * Opt-in; fl_track_batch and fl_verify_batch are unchanged.  depth, mem, frame_of_track, poses13, K and params are as
 * fl_track_batch takes them, n_groups and group_first as fl_verify_batch takes them; vparams == NULL: the defaults below.
 * Everything is queued on the context's stream and the call waits once, at the end; it allocates nothing.
 *   passes   all params->passes passes of fl_track_batch, with its lost rule and its gates.  icp_tracked is that call's
 *            `tracked`; track.status, the rects and track.det are that call's.
 *   verify   once, after the last pass, on the device: every track with icp_tracked = 1 has the pose the passes returned
 *            (det.R_final | det.T_final, the twelve floats fl_track_batch would report) verified against its frame exactly as
 *            fl_verify_batch states it -- the render at the SCENE camera (float)K->fx .., not at the model camera the passes
 *            render with, then score and finish -> `verify`.  With keep_input = 1 the pose the track came in with is verified
 *            against the same frame -> `verify_in`.  The render of a pose stays in the LDS of one workgroup whatever the
 *            context option verify_fused says.  Both records carry best = accepted.  A track with icp_tracked = 0 is not
 *            verified: both records zero, tracked = 0, pose = the input pose, kept_input = 0.
 *   decide   per track with icp_tracked = 1, A = verify.accepted and B = keep_input && verify_in.accepted:
 *              neither    tracked = 0, pose = the input pose, kept_input = 0
 *              only A     tracked = 1, pose = the passes' pose
 *              only B     tracked = 1, pose = the input pose as a 4x4, kept_input = 1
 *              both       the input pose is kept (kept_input = 1) only when it verifies strictly better,
 *                         (int64)verify_in.n_inlier * verify.n_model > (int64)verify.n_inlier * verify_in.n_model;
 *                         a tie keeps the passes' pose
 *            A track's CHOSEN record is verify_in where kept_input = 1, else verify.
 *   pick     groups as fl_verify_batch's (several start poses for one object, say the previous pose and a motion model's
 *            prediction): best = 1 for at most one track of a group, among its tracked = 1 tracks the one whose chosen record
 *            has the largest n_inlier / n_model, compared exactly as fl_verify_batch compares, a tie to the lower index; a group
 *            without a tracked member has no best.  group_first == NULL (n_groups is ignored): best = tracked.
 * With the default gates every non-empty render is accepted: the call then reports what fl_track_batch reports, plus figures
 * (a pose whose render at the scene camera is empty is not accepted, and its track comes back with tracked = 0).
 * FL_ERR_INVALID, nothing written, before the first HIP call: everything fl_track_batch refuses; fx, fy not finite and > 0 or
 * cx, cy not finite as floats; fl_verify_batch's rules for n_groups and group_first; fl_verify_params' ranges; keep_input
 * outside {0, 1}. */
typedef struct {
  fl_verify_params verify;             /* tau_mm, min_model_px, min_inlier_ratio, max_behind_ratio: ranges and defaults of fl_verify_batch */
  int32_t keep_input;                  /* 1: the pose a track came in with is verified too and kept where it verifies strictly better; default 0 */
  int32_t reserved;
} fl_track_verify_params;
typedef struct {
  fl_track_result track;               /* status, rects, det: exactly what fl_track_batch reports; tracked and pose: by the rule above */
  fl_verify_result verify;             /* of the pose the passes returned; zeros when icp_tracked == 0 */
  fl_verify_result verify_in;          /* of the input pose; zeros when keep_input == 0 or icp_tracked == 0 */
  int32_t icp_tracked;                 /* what fl_track_batch's `tracked` is for this track */
  int32_t kept_input;                  /* 1: pose is the input pose because it verified better (or alone) */
  int32_t best;                        /* the group pick */
  int32_t reserved;
} fl_verified_track_result;            /* 368 bytes */
int  fl_track_batch_verified(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem,
                             int n_tracks, const int32_t *frame_of_track, const float *poses13,
                             int n_groups, const int32_t *group_first, const fl_intrinsics *K,
                             const fl_track_params *params, const fl_track_verify_params *vparams,
                             fl_verified_track_result *results);
/* with a mesh per track: see "several meshes on one tracker" above for mesh_of_track and the contract; the passes and the
 * verification of a track use the same mesh */
int  fl_track_batch_verified_meshes(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem,
                                    int n_tracks, const int32_t *frame_of_track, const int32_t *mesh_of_track, const float *poses13,
                                    int n_groups, const int32_t *group_first, const fl_intrinsics *K,
                                    const fl_track_params *params, const fl_track_verify_params *vparams,
                                    fl_verified_track_result *results);
/* ---- verified instance pick: fl_recognize_batch_instances whose pick among a group's members is the verification's -----------
 * The call chain of fl_recognize_batch_instances up to and including its ONE ICP launch, then, all on the device and on the
 * same n_frames * max_instances * hyp_per_instance job slots: the verification of every LIVE slot -- its job exists, its
 * result has found = 1 and its class passes class_idx -- exactly as fl_verify_batch states it (render at the scene camera
 * (float)K->fx .., score, finish), with the pose read from the slot's fl_recognition_result::pose (its first 12 floats are the
 * poses13 layout in mm) and the frame read where the detector's batch has it; then the pick, one copy and one wait.  The
 * render of a slot stays in the LDS of one workgroup (see the context option verify_fused).  `mesh` supplies its mesh, its
 * w x h and its context only: none of its frame slots, render images or ICP workspaces is touched, there is no max_tracks
 * limit, and a fl_track_batch or fl_verify_batch before or after is unaffected.  Accumulators and records come out of the
 * context's scratch beside the ICP results.
 * Pick -- a group is VERIFIED when class_idx < 0 or its class is class_idx.  Among a verified group's refined members with
 * found = 1 and accepted = 1, in list order, a beats b when (int64)n_inlier_a * n_model_b > (int64)n_inlier_b * n_model_a; a
 * tie goes to the earlier member (fl_verify_batch's rule).  inst.reco / inst.rank are that member's, verify is its record with
 * best = 1.  A verified group without an accepted member reports fl_recognize_batch_instances' pick with that member's record
 * (accepted = 0, best = 0; zeros when that member was not found).  A group that is not verified reports that pick, verified = 0
 * and a zero record.  nms_rank is always the list index fl_recognize_batch_instances picks.  member_verify (NULL: not wanted):
 * member_verify[(f * max_instances + g) * hyp_per_instance + r] = the finished record of slot r of group g of frame f, best =
 * 1 on a group's picked accepted member only, all zero for a slot that is absent or not live.
 * FL_ERR_INVALID, nothing written: what fl_recognize_batch_instances refuses; mesh or vp NULL; a tracker on another context;
 * the tracker's w x h not the detector's frame size or not K's; the fl_verify_params ranges of fl_verify_batch; fx, fy not
 * finite and > 0 or cx, cy not finite as floats; class_idx outside [-1, classes). */
typedef struct {
  fl_verify_params verify;             /* tau_mm, min_model_px, min_inlier_ratio, max_behind_ratio, as fl_verify_batch */
  int32_t class_idx;                   /* >= 0: only groups of this class are verified against the mesh; -1: every group */
  int32_t reserved;
} fl_instance_verify_params;
typedef struct {
  fl_instance_result inst;             /* as fl_recognize_batch_instances, but inst.reco / inst.rank = the verified pick */
  fl_verify_result verify;             /* of the picked member; zeros when verified == 0 */
  int32_t nms_rank;                    /* the list index nonMaximumSuppression's rule picks (fl_recognize_batch_instances' rank) */
  int32_t verified;                    /* 1: the group's members were verified; 0: its class is not class_idx */
  int32_t reserved[2];
} fl_verified_instance_result;
int  fl_recognize_batch_instances_verified(fl_detector *det, fl_tracker *mesh, int n_frames, const uint8_t *const *bgr,
                                           const uint16_t *const *depth, int mem, const fl_intrinsics *K,
                                           const fl_recognition_params *params, const fl_instance_params *ip,
                                           const fl_instance_verify_params *vp, fl_verified_instance_result *results,
                                           int32_t *n_instances, int32_t *n_dropped, fl_verify_result *member_verify);
/* The same with a mesh per class: `mesh` is a tracker of several meshes (fl_tracker_create_meshes) and mesh_of_class, host
 * memory, has fl_detector_num_classes(det) entries, each a mesh of the tracker or -1.  A slot is LIVE when its job exists, its
 * result has found = 1 and mesh_of_class[its class] >= 0, and is verified against that mesh; a group is VERIFIED when its class
 * maps to a mesh.  Everything else -- the pick, nms_rank, member_verify, a verified group without an accepted member -- is as
 * stated above.  fl_recognize_batch_instances_verified is this call with the map "every class -> mesh 0" (class_idx = -1) or
 * "class_idx -> mesh 0, every other class -> -1".  The map travels with the call's other inputs: no further wait, no allocation
 * beyond the context's scratch and pinned blocks.  FL_ERR_INVALID on top of the refusals above: mesh_of_class NULL, an entry
 * outside [-1, n_meshes), vp->class_idx other than -1 (the map says it). */
int  fl_recognize_batch_instances_verified_meshes(fl_detector *det, fl_tracker *mesh, int n_frames, const uint8_t *const *bgr,
                                                  const uint16_t *const *depth, int mem, const fl_intrinsics *K,
                                                  const fl_recognition_params *params, const fl_instance_params *ip,
                                                  const fl_instance_verify_params *vp, const int32_t *mesh_of_class,
                                                  fl_verified_instance_result *results, int32_t *n_instances, int32_t *n_dropped,
                                                  fl_verify_result *member_verify);
/* ---- scene arbitration: one kept hypothesis per supported surface patch ----------------------------------------------------------
 * Grouping, fl_nms and the picks above decide inside one class or by a distance between translations.  Two classes that fire on
 * one physical object (a bracket whose mesh is part of a housing), or two tracks that drifted onto one object, each verify
 * well.  fl_verify_scene_batch verifies every pose as fl_verify_batch_meshes does and then asks of every two accepted poses of
 * one SCENE how many frame pixels support both; a pose whose support is largely another, stronger pose's is suppressed.  Opt-in:
 * no other entry point changes.  depth, mem, frame_of_pose, mesh_of_pose (NULL: mesh 0), poses13 and K are as
 * fl_verify_batch_meshes takes them; results (n_poses records) is host memory; params == NULL: the defaults below.  Everything
 * is queued on the context's stream and the call waits once, at the end; it allocates nothing beyond the context's scratch
 * and pinned blocks, which persist.  It writes the tracker's frame slots and render images, as fl_verify_batch does.
 *   scenes   scene s is the poses scene_first[s] .. scene_first[s + 1] - 1 (scene_first: n_scenes + 1 entries, host memory,
 *            non-decreasing, scene_first[0] == 0, scene_first[n_scenes] == n_poses).  A scene may be empty, has at most
 *            FL_SCENE_MAX_POSES poses, and all of its poses name one frame.
 *   verify   every pose gets exactly the render (at the SCENE camera), score and finish of fl_verify_batch_meshes with
 *            group_first == NULL -> `verify`, byte for byte that call's record (best = accepted).  The context option
 *            verify_fused is ignored here: the renders are read again afterwards, so they are always written to memory.
 *   support  pixel p supports pose a when r_a(p) != 0 && s(p) != 0 && |s(p) - r_a(p)| <= tau_mm: the pixels n_inlier counts.
 *   shared   shared(a, b) = the number of pixels that support both poses; symmetric; taken as 0 unless both poses are accepted.
 *            Stored compactly: with m_s the size of scene s and pair_first(s) = sum over s' < s of m_s' (m_s' - 1) / 2, the
 *            pair of local indices i < j of scene s is entry pair_first(s) + j (j - 1) / 2 + i.
 *   order    among the accepted poses of a scene, a stands before b when n_inlier_a > n_inlier_b; or these are equal and
 *            (int64)n_inlier_a * n_model_b > (int64)n_inlier_b * n_model_a; or both are equal and a has the lower index.
 *            More explained surface goes first: a large object precedes its own part, whatever their ratios.  What keeps a
 *            large WRONG pose from leading a scene is the gates of `verify` (min_inlier_ratio, max_behind_ratio), not the order.
 *   suppress walk the order with an initially empty kept list.  For pose b: rival = -1, n_shared = 0; for every kept a, in the
 *            order it was kept, n = shared(a, b): if n >= min_shared_px && (float)n / (float)n_inlier_b >= max_shared_ratio
 *            (one float32 division, as the other ratios of this header), b is suppressed: kept = 0, rival = a, n_shared = n,
 *            and the walk over the kept list stops; otherwise if n > n_shared, rival = a and n_shared = n.  A pose no kept pose
 *            suppressed joins the kept list, kept = 1, rival = the kept pose it shares most with (the earliest kept of equals) or
 *            -1.  A suppressed pose never suppresses another.  A pose that is not accepted: kept = 0, order = -1, rival = -1,
 *            n_shared = 0.  rival is a pose index in the call, not in the scene.
 * Returns FL_OK when the batch ran.  FL_ERR_INVALID, nothing written, before the first HIP call: everything
 * fl_verify_batch_meshes refuses (its group rules aside); scene_first NULL, n_scenes outside 1..max_tracks, a scene_first that
 * breaks the rules above, a scene of more than FL_SCENE_MAX_POSES poses or of two frames; max_shared_ratio not finite or outside
 * (0, 1]; min_shared_px < 1.
 * fl_scene_pick is the order and the suppression alone, host only (like fl_nms), on records and a compact shared array the
 * caller has: results[i].verify = records[i], the other fields by the rules above.  It refuses (FL_ERR_INVALID, nothing
 * written) null pointers -- shared may be NULL only when no scene has a pair --, the same scene_first (n_scenes >= 1) and params,
 * and a shared entry of two accepted poses outside 0 .. min(n_inlier_a, n_inlier_b); entries of other pairs are ignored. */
#define FL_SCENE_MAX_POSES 64
typedef struct {
  fl_verify_params verify;             /* per-pose rule and gates: ranges and defaults of fl_verify_batch */
  float   max_shared_ratio;            /* suppressed when shared / n_inlier reaches it; finite, in (0, 1]; default 0.5 */
  int32_t min_shared_px;               /* and shared is at least this; >= 1; default 1 */
} fl_scene_params;
typedef struct {
  fl_verify_result verify;             /* byte for byte fl_verify_batch_meshes' record with group_first == NULL (best = accepted) */
  int32_t kept;                        /* 1: survives the arbitration */
  int32_t order;                       /* 0-based place in its scene's order; -1: not accepted */
  int32_t rival;                       /* pose index in the call, or -1 */
  int32_t n_shared;                    /* shared(rival, this pose); 0 when rival == -1 */
} fl_scene_result;                     /* 80 bytes */
int  fl_verify_scene_batch(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_poses,
                           const int32_t *frame_of_pose, const int32_t *mesh_of_pose, const float *poses13,
                           int n_scenes, const int32_t *scene_first, const fl_intrinsics *K,
                           const fl_scene_params *params, fl_scene_result *results);
int  fl_scene_pick(const fl_verify_result *records, int n_poses, int n_scenes, const int32_t *scene_first,
                   const int32_t *shared, const fl_scene_params *params, fl_scene_result *results);
/* After fl_match_frame / fl_recognize_submit: copy frame `frame`'s first k sorted matches into a
 * device buffer (k * sizeof(fl_match) bytes, padded with template_id = -1) for an RCCL
 * all-gather by the caller; template ids are offset by template_id_base (the shard's first
 * global id).  Queued on the context's stream, no synchronisation. */
int  fl_export_topk(fl_detector *det, int frame, int k, int template_id_base, void *dev_out);
/* the same for every frame of the last batch in one launch: dev_out[frame * k + i].
 * A frame whose candidate buffers overflowed (its list is truncated in an order that depends on atomics) is exported as
 * record 0 = {template_id = FL_TOPK_OVERFLOW, class_idx = -1} and padding: the flag travels with the all-gather, so every
 * rank sees it (fl_select_best_batch turns it into that frame's status; the host merge ignores records with ids < 0). */
#define FL_TOPK_OVERFLOW (-2)
int  fl_export_topk_batch(fl_detector *det, int n_frames, int k, int template_id_base, void *dev_out);
/* merge n_ranks*k gathered records (host) exactly as one Detector::match over the union would
 * order them; returns the number written to out (<= cap). */
int  fl_merge_topk(const fl_match *gathered, int n_records, fl_match *out, int cap);

/* fl_merge_topk per frame of a batch: gathered[(rank * n_frames + frame) * k + i] is what an all-gather of the ranks'
 * fl_export_topk_batch buffers yields; out[frame * cap + j], n_out[frame] (all host memory) */
int  fl_merge_topk_batch(const fl_match *gathered, int n_ranks, int n_frames, int k, fl_match *out, int cap, int *n_out);
/* Template-sharded recognition (BASELINE configs[3]): after the merge, the rank that owns frame f's winning template
 * refines it -- the second half of Recognition() (obj_reco_lmicp.cpp:111-197: crop rectangles from the template, the
 * depth render, detection(), pose) for a match chosen by the caller instead of this detector's own matches[0].
 * frames[j] indexes the batch last queued with fl_match_batch_submit (whose depth frames must still be where they were),
 * matches[j].template_id is class-local on THIS detector; results[j] (host) as fl_recognize_batch fills them. */
int  fl_refine_matches(fl_detector *det, int n_jobs, const int32_t *frames, const fl_match *matches, const fl_intrinsics *K,
                       const fl_recognition_params *params, fl_recognition_result *results);
/* The same hand-over without leaving the device (no host round trip between Detector::match and the ICP):
 * fl_select_best_batch reads the all-gathered records IN DEVICE MEMORY (dev_gathered[(rank * n_frames + frame) * k + i],
 * global template ids) and writes, per frame, matches[0] of one global std::sort + std::unique over all ranks' lists
 * (linemod.cpp:1437-1439, Match::operator< linemod.hpp:262-267; Recognition() uses nothing else, obj_reco_lmicp.cpp:111)
 * to dev_best[frame] (global ids; template_id = -1: no rank matched; FL_TOPK_OVERFLOW: some rank's list overflowed) --
 * every list is sorted, so it is the best of the ranks' first records.  Frames whose winner lies in this rank's slice
 * [tid_first, tid_first + tid_count) become the detector's pending refinement jobs.
 * fl_refine_selected then runs the second half of Recognition() for those jobs (one launch over n_frames workgroups,
 * the ones without a job exit at once) and writes dev_rows[frame][17] = {found, row-major 4x4 pose} as float32, zeros
 * for the frames this rank does not own (a sum or a gather over the ranks gives every frame's pose).  depth_base /
 * depth_stride (bytes) locate the batch's depth frames on the device; NULL / 0 = where fl_match_batch_submit left them.
 * Both are queued on the context's stream without synchronisation. */
int  fl_select_best_batch(fl_detector *det, const void *dev_gathered, int n_ranks, int n_frames, int k, int tid_first,
                          int tid_count, void *dev_best);
int  fl_refine_selected(fl_detector *det, int n_frames, const fl_intrinsics *K, const fl_recognition_params *params,
                        const uint16_t *depth_base, size_t depth_stride, float *dev_rows);

/* diagnostics: per-frame counters of the last match {coarse candidates, matches after sort/unique, overflow flag,
 * level-0 tiles (60 x 60 pixels) whose colour quantisation the lazy fine levels computed; -1 when the batch ran eagerly}
 * (host memory) */
int  fl_frame_counters(fl_detector *det, int frame, int32_t out[4]);

/* per-stage device time (ms) of the last fl_recognize_* call, by stage index; for bench.py.  icp_ms starts at the first ICP
 * launch.  total_ms spans the batch's first to its last event: for a batch whose ICP stage ran on the second stream it
 * includes that stage's wait for the ICP stage of the batch before it. */
typedef struct {
  float frontend_ms, linmem_ms, scan_ms, refine_ms, sort_ms, backproject_ms, icp_ms, total_ms;
  int32_t icp_iters_total, icp_launches;
  double scan_algorithmic_bytes;
  float lazy_frontend_ms;   /* fl_recognize_*: colour quantisation + spread of the finer levels, computed after the scan
                               and only in the tiles the candidates touch (0 when FL_EAGER_FRONTEND=1: then part of
                               frontend_ms / linmem_ms).  refine_ms excludes it. */
  float group_ms;          /* fl_recognize_batch_instances: the grouping and the pick kernel (icp_ms includes them) */
} fl_stage_times;
int  fl_last_stage_times(fl_detector *det, fl_stage_times *out);

#ifdef __cplusplus
}
#endif
#endif /* FEALESS_HIP_H */
