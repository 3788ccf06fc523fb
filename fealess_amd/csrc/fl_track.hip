// fl_track.hip -- 6-DoF model-based tracking (fl_tracker_create / fl_track_batch, include/fealess_hip.h): the batched z-buffer
// rasteriser of fl_render.hip and the ICP workgroup per job of fl_icp.hip, joined on the device.  No counterpart in the
// reference, which links a 2-D KCF box tracker it never calls (test/linemod_acq.cpp:108-150).
//
// A tracker holds one mesh or several (fl_tracker_create_meshes): the meshes lie back to back in one vertex and one triangle
// array, a mesh is a range of triangles (FlMeshRange), and a pose names its mesh through d_mesh_of; frame slots, render images,
// keys and ICP workspaces are shared.  Only the two kernels that read triangles know: k_raster<true> and the k_verify_fused pair.
//
// Here: the tracker, the steps every call on one shares (fl_track_internal.h: checks, staging, render, results),
// fl_track_batch and fl_track_batch_verified.  fl_verify_batch, the other user of those steps, is fl_verify.hip.
//
// One pass of a call, all on the context's stream:
//   fl_tracker_render        the mesh at every track's pose, depth only, K = 608 / 608 / 320 / 240 (the K crop_clouds
//                            back-projects a model image with, fl_icp.hip; ICP/detection.cpp:35-36)
//   k_track_rects            one workgroup per track: bounding box of the render, the rectangle rule, the render x 10 inside
//                            rect_model, and the records the ICP kernel's job-list path reads for slot t: pyr[t], depth_ptrs[t],
//                            jobs[t] (the pose is already at poses[13 t]); frame = -1 for a slot that has nothing to refine
//   fl_launch_detection_tables   k_icp_pipeline over the n_tracks slots, through its job list: class_first = {0}, so slot t's
//                            "template" is g = t
//   k_track_finish           one thread per track: the lost rule, the result record, the pose of the next pass
// fl_track_batch_verified runs the same passes (track_passes), then on the same stream, with no host step in between:
//   k_verify_fused_tracks    (fl_verify.hip, through fl_launch_verify_fused) ONE launch over n_tracks workgroups, 2 n_tracks with
//                            keep_input: the poses k_track_finish left in d_poses, then the poses of d_poses_in, each rendered at
//                            the scene camera in LDS and scored against its frame; a workgroup whose track is lost exits at once
//   k_track_verified_finish  one thread per track: k_verify_finish's record of one or two accumulators, the decision, the whole
//                            fl_verified_track_result (its fl_track_result copied from the passes' record)
//   k_track_verified_pick    one thread per group, only with groups
// The rectangle rule is stated in integers in include/fealess_hip.h and in numpy in tests/track_model.py; the shift is fp64,
// one IEEE operation per operator (the Makefile's -ffp-contract=off: hipcc would contract a * b + c otherwise).
#include "fl_track_internal.h"
#include <stdio.h>
#include <vector>

namespace {

constexpr int TB = 256;                         // k_track_rects: threads per track
constexpr double MODEL_F = 608.0, MODEL_CX = 320.0, MODEL_CY = 240.0;   // initInternalMat (ICP/common.cpp:358)
constexpr double SHIFT_MAX = 1048576.0;         // 2^20: a shift beyond it cannot leave a pixel of an 8192-pixel image in view

struct TrackArgs {
  int n_tracks, w, h, margin, max_crop_px;
  double fx, fy, cx, cy;                        // the scene camera
  uint16_t *render;                             // n_tracks images of w * h, views back to back
  const int32_t *frame_of;
  float *poses;                                 // n_tracks * 13: the pose each pass starts from
  const float *poses_in;                        // n_tracks * 13: the poses the call came in with
  int32_t *lost;                                // per track: 1 once it is not tracked
  FlPyrInfo *pyr;
  const uint16_t **depth_ptrs;
  FlRefineJob *jobs;
  const fl_recognition_result *res;
  fl_track_result *out;
  float max_dist_mean, min_px_ratio;
};

__device__ __forceinline__ void pose_to_4x4(const float *p13, float *m)
{
  for (int k = 0; k < 12; ++k) m[k] = p13[k];
  m[12] = m[13] = m[14] = 0.f;
  m[15] = 1.f;
}

__global__ __launch_bounds__(TB) void k_track_rects(TrackArgs a)
{
  __shared__ int red[4][TB / FL_WAVE];
  __shared__ int rect[5];                       // rect_model after the clip, and whether the slot runs
  const int t = blockIdx.x, tid = threadIdx.x;
  if (a.lost[t]) {                              // not tracked in an earlier pass: the slot exits at once (uniform per workgroup)
    if (tid == 0) a.jobs[t].frame = -1;
    return;
  }
  const int px = a.w * a.h;                     // <= FL_RENDER_MAX_DIM^2, fits an int
  uint16_t *img = a.render + (size_t)t * px;
  int x0 = a.w, x1 = -1, y0 = a.h, y1 = -1;
  if ((px & 7) == 0) {                          // every image starts on a 16-byte boundary: eight pixels per load
    // one workgroup reads a whole image, so the loop is bound by the latency of its loads: four of them in flight per thread
    const uint4 *v4 = (const uint4 *)img;
    const int n8 = px / 8;
    for (int i0 = tid; i0 < n8; i0 += 4 * TB) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * TB;
        v[u] = i < n8 ? v4[i] : make_uint4(0u, 0u, 0u, 0u);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if ((v[u].x | v[u].y | v[u].z | v[u].w) == 0u) continue;
        const int i = i0 + u * TB;
        const unsigned wd[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
        for (int k = 0; k < 4; ++k) {
          if (wd[k] & 0xffffu) bbox_add(8 * i + 2 * k, a.w, x0, x1, y0, y1);
          if (wd[k] >> 16) bbox_add(8 * i + 2 * k + 1, a.w, x0, x1, y0, y1);
        }
      }
    }
  } else {
    for (int i = tid; i < px; i += TB)
      if (img[i]) bbox_add(i, a.w, x0, x1, y0, y1);
  }
  for (int s = 32; s >= 1; s >>= 1) {
    x0 = min(x0, __shfl_xor(x0, s, FL_WAVE)); x1 = max(x1, __shfl_xor(x1, s, FL_WAVE));
    y0 = min(y0, __shfl_xor(y0, s, FL_WAVE)); y1 = max(y1, __shfl_xor(y1, s, FL_WAVE));
  }
  if ((tid & (FL_WAVE - 1)) == 0) {
    const int wv = tid / FL_WAVE;
    red[0][wv] = x0; red[1][wv] = x1; red[2][wv] = y0; red[3][wv] = y1;
  }
  __syncthreads();
  if (tid == 0) {
    for (int wv = 0; wv < TB / FL_WAVE; ++wv) {
      x0 = min(x0, red[0][wv]); x1 = max(x1, red[1][wv]);
      y0 = min(y0, red[2][wv]); y1 = max(y1, red[3][wv]);
    }
    int rm[4] = {0, 0, 0, 0}, rr[4] = {0, 0, 0, 0};
    int status = FL_OK;
    bool run = x1 >= x0;                        // an empty render: out of view
    if (run) {
      const int mx0 = max(x0 - a.margin, 0), my0 = max(y0 - a.margin, 0);
      const int mx1 = min(x1 + a.margin, a.w - 1), my1 = min(y1 + a.margin, a.h - 1);
      const float *p = a.poses + 13 * (size_t)t;
      const double tx = (double)p[3], ty = (double)p[7], tz = (double)p[11];
      const double sx = (a.fx - MODEL_F) * (tx / tz) + (a.cx - MODEL_CX), sy = (a.fy - MODEL_F) * (ty / tz) + (a.cy - MODEL_CY);
      run = fabs(sx) <= SHIFT_MAX && fabs(sy) <= SHIFT_MAX;    // false for NaN too
      if (run) {
        const int dx = (int)rint(sx), dy = (int)rint(sy);
        const int cx0 = max(mx0 + dx, 0), cy0 = max(my0 + dy, 0), cx1 = min(mx1 + dx, a.w - 1), cy1 = min(my1 + dy, a.h - 1);
        run = cx1 >= cx0 && cy1 >= cy0;
        if (run) {
          rr[0] = cx0; rr[1] = cy0; rr[2] = cx1 - cx0 + 1; rr[3] = cy1 - cy0 + 1;
          rm[0] = cx0 - dx; rm[1] = cy0 - dy; rm[2] = rr[2]; rm[3] = rr[3];
          if ((long long)rm[2] * rm[3] > a.max_crop_px) { status = FL_ERR_OVERFLOW; run = false; }
        }
      }
    }
    fl_track_result *o = a.out + t;
    o->status = status;
    for (int k = 0; k < 4; ++k) { o->rect_model[k] = rm[k]; o->rect_ref[k] = rr[k]; rect[k] = rm[k]; }
    rect[4] = run ? 1 : 0;
    FlPyrInfo pi;
    pi.class_idx = 0; pi.template_id = t;
    pi.off_x0 = rm[0]; pi.off_y0 = rm[1]; pi.width0 = rm[2]; pi.height0 = rm[3];
    pi.depth_slot = t; pi.pad = 0;
    a.pyr[t] = pi;
    a.depth_ptrs[t] = img;
    FlRefineJob j;
    j.frame = run ? a.frame_of[t] : -1;
    j.match.x = rr[0]; j.match.y = rr[1]; j.match.similarity = 0.f; j.match.class_idx = 0; j.match.template_id = t;
    a.jobs[t] = j;
  }
  __syncthreads();
  if (!rect[4]) return;
  // millimetres -> 0.1 mm inside rect_model, saturating (what the recognition branch of the ICP kernel reads)
  const int rx = rect[0], ry = rect[1], rw = rect[2], n = rw * rect[3];
  for (int i = tid; i < n; i += TB) {
    const int y = i / rw, x = i - y * rw;
    uint16_t *q = img + (size_t)(ry + y) * a.w + rx + x;
    const unsigned v = 10u * (unsigned)*q;
    *q = (uint16_t)(v > 65535u ? 65535u : v);
  }
}

__global__ __launch_bounds__(64) void k_track_finish(TrackArgs a)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= a.n_tracks || a.lost[t]) return;     // lost earlier: the record of the pass that lost it stands
  fl_track_result *o = a.out + t;
  bool lost = a.jobs[t].frame < 0;              // nothing to refine: out of view or too large a crop (status says which)
  if (!lost) {
    const fl_recognition_result &r = a.res[t];
    o->det = r.det;
    if (r.status != FL_OK) o->status = r.status;
    const fl_icp_result &ic = r.det.icp;
    lost = r.status != FL_OK || !r.found || ic.dist_mean < 0.f || (a.max_dist_mean > 0.f && ic.dist_mean > a.max_dist_mean) ||
           (a.min_px_ratio > 0.f && ic.px_ratio < a.min_px_ratio);
    if (!lost) {
      for (int k = 0; k < 16; ++k) o->pose[k] = r.pose[k];
      float *p = a.poses + 13 * (size_t)t;      // the next pass starts here
      for (int k = 0; k < 12; ++k) p[k] = r.pose[k];
      o->tracked = 1;
      return;
    }
  } else {
    memset(&o->det, 0, sizeof(o->det));
  }
  a.lost[t] = 1;
  o->tracked = 0;
  pose_to_4x4(a.poses_in + 13 * (size_t)t, o->pose);
}

struct TrackVerifiedArgs {
  int n_tracks, n_groups, w, h, min_model_px, keep_input;
  float min_inlier_ratio, max_behind_ratio;
  const fl_track_result *track;                 // the passes' records
  const float *poses_in;
  const FlVerifyAcc *acc;                       // n_tracks of the passes' poses, then n_tracks of the input poses
  const int32_t *group_first;                   // null: best = tracked
  fl_verified_track_result *out;
};

__global__ __launch_bounds__(64) void k_track_verified_finish(TrackVerifiedArgs a)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= a.n_tracks) return;
  fl_verified_track_result *o = a.out + t;
  memset(o, 0, sizeof(*o));
  o->track = a.track[t];
  if (!o->track.tracked) return;                // lost in the passes: its record stands, the pose it came in with included
  o->icp_tracked = 1;
  fl_verify_result v = fl_verify_record(a.acc[t], a.w, a.h, a.min_model_px, a.min_inlier_ratio, a.max_behind_ratio), vi;
  v.best = v.accepted;
  o->verify = v;
  memset(&vi, 0, sizeof(vi));
  if (a.keep_input) {
    vi = fl_verify_record(a.acc[a.n_tracks + t], a.w, a.h, a.min_model_px, a.min_inlier_ratio, a.max_behind_ratio);
    vi.best = vi.accepted;
    o->verify_in = vi;
  }
  const bool A = v.accepted, B = vi.accepted;
  const bool keep = B && (!A || (long long)vi.n_inlier * v.n_model > (long long)v.n_inlier * vi.n_model);
  o->kept_input = keep;
  o->track.tracked = A || B;
  if (keep || !(A || B)) pose_to_4x4(a.poses_in + 13 * (size_t)t, o->track.pose);
  o->best = a.group_first ? 0 : o->track.tracked;
}

__global__ __launch_bounds__(64) void k_track_verified_pick(TrackVerifiedArgs a)
{
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= a.n_groups) return;
  int best = -1;
  long long bi = 0, bm = 1;
  for (int i = a.group_first[g]; i < a.group_first[g + 1]; ++i) {
    const fl_verified_track_result &r = a.out[i];
    if (!r.track.tracked) continue;             // tracked: the chosen record is accepted, n_model >= min_model_px >= 1
    const fl_verify_result &c = r.kept_input ? r.verify_in : r.verify;
    if (best < 0 || (long long)c.n_inlier * bm > bi * (long long)c.n_model) { best = i; bi = c.n_inlier; bm = c.n_model; }
  }
  if (best >= 0) a.out[best].best = 1;
}
}  // namespace

static const fl_track_params k_track_defaults = {12, 1, 10, 0.5f, 0.01f, FL_ICP_POINT_TO_PLANE, 0.f, 0.f};

// the argument checks of fl_tracker_create that concern the sizes (shared with fl_dev_tracker_create_host)
static int tracker_sizes_ok(fl_context *ctx, int w, int h, int max_frames, int max_tracks, int max_crop_px)
{
  if (w < 1 || h < 1 || w > FL_RENDER_MAX_DIM || h > FL_RENDER_MAX_DIM)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_tracker_create: image size %dx%d outside 1..%d", w, h, FL_RENDER_MAX_DIM);
  if (max_frames < 1 || max_tracks < 1 || max_frames > FL_TRACK_MAX_TRACKS || max_tracks > FL_TRACK_MAX_TRACKS)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_tracker_create: max_frames %d / max_tracks %d outside 1..%d", max_frames, max_tracks, FL_TRACK_MAX_TRACKS);
  const long long px = (long long)w * h;
  if (max_crop_px < 1 || max_crop_px > px || max_crop_px > FL_TRACK_MAX_CROP_PX)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_tracker_create: max_crop_px %d outside [1, min(w * h, %d)]", max_crop_px, FL_TRACK_MAX_CROP_PX);
  if (fl_align(fl_icp_ws_bytes(max_crop_px), 256) * (size_t)max_tracks > ((size_t)96 << 30))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_tracker_create: %d ICP workspaces of %d pixels pass 96 GB", max_tracks, max_crop_px);
  return FL_OK;
}

// The argument checks of fl_tracker_create_meshes that concern the meshes (shared with fl_dev_tracker_create_host_meshes): each
// mesh by fl_render_check_mesh's rules, an index inside its own mesh's vertices, then the sums.  name_mesh: the text says which.
static int tracker_meshes_ok(fl_context *ctx, const char *who, bool name_mesh, const fl_mesh *meshes, int n_meshes)
{
  if (!meshes) return fl_set_error(ctx, FL_ERR_INVALID, "%s: null meshes", who);
  if (n_meshes < 1 || n_meshes > FL_TRACK_MAX_MESHES)
    return fl_set_error(ctx, FL_ERR_INVALID, "%s: n_meshes %d outside 1..%d", who, n_meshes, FL_TRACK_MAX_MESHES);
  long long nv = 0, nt = 0;
  for (int m = 0; m < n_meshes; ++m) {
    char w[96];
    if (name_mesh) snprintf(w, sizeof(w), "%s: mesh %d", who, m);
    else snprintf(w, sizeof(w), "%s", who);
    if (int rc = fl_render_check_mesh(ctx, w, meshes[m].vertices, nullptr, meshes[m].n_vertices, meshes[m].triangles, meshes[m].n_triangles)) return rc;
    nv += meshes[m].n_vertices;
    nt += meshes[m].n_triangles;
  }
  if (nv > FL_RENDER_MAX_PRIMS || nt > FL_RENDER_MAX_PRIMS)
    return fl_set_error(ctx, FL_ERR_INVALID, "%s: %lld vertices or %lld triangles over the %d meshes pass %d", who, nv, nt, n_meshes, FL_RENDER_MAX_PRIMS);
  return FL_OK;
}

// a tracker that knows its sizes and owns nothing yet (what fl_tracker_create and fl_dev_tracker_create_host both start from)
static fl_tracker *tracker_new(fl_context *ctx, bool owns_ctx, int w, int h, int max_frames, int max_tracks, int max_crop_px)
{
  fl_tracker *trk = new fl_tracker();
  trk->ctx = ctx;
  trk->owns_ctx = owns_ctx;
  trk->w = w; trk->h = h;
  trk->max_frames = max_frames; trk->max_tracks = max_tracks; trk->max_crop_px = max_crop_px;
  return trk;
}

// The tracker's device memory, every part named once: the meshes' n_vertices vertices and n_triangles triangles and their range
// table, the frame slots, per track a
// render image, an ICP workspace and the small records (two verification accumulators: fl_track_batch_verified scores a track's
// input pose too, and writes its records straight into d_vout), per render chunk the depth keys.  base null: the sizing pass.
static size_t carve_device(fl_tracker *trk, uint8_t *base, size_t n_vertices, size_t n_triangles)
{
  const size_t px = (size_t)trk->w * trk->h, T = (size_t)trk->max_tracks;
  size_t off = 0;
  auto take = [&](auto *&p, size_t bytes) { fl_carve(p, base, off, bytes); };
  take(trk->d_vtx, n_vertices * 3 * 4); take(trk->d_tri, n_triangles * 3 * 4); take(trk->d_ranges, (size_t)trk->n_meshes * sizeof(FlMeshRange));
  take(trk->d_frames, trk->frame_stride * trk->max_frames);
  take(trk->d_render, T * px * 2); take(trk->d_keys, (size_t)trk->chunk * px * 8);
  take(trk->d_icp, trk->ws_one * T);
  take(trk->d_poses, T * 13 * 4); take(trk->d_poses_in, T * 13 * 4);
  take(trk->d_frame_of, T * 4); take(trk->d_mesh_of, T * 4); take(trk->d_lost, T * 4); take(trk->d_class_first, 4);
  take(trk->d_pyr, T * sizeof(FlPyrInfo)); take(trk->d_depth_ptrs, T * sizeof(void *)); take(trk->d_jobs, T * sizeof(FlRefineJob));
  take(trk->d_res, T * sizeof(fl_recognition_result)); take(trk->d_out, T * sizeof(fl_track_result));
  take(trk->d_vacc, 2 * T * sizeof(FlVerifyAcc)); take(trk->d_vres, T * sizeof(fl_verify_result)); take(trk->d_group_first, (T + 1) * 4);
  take(trk->d_vout, T * sizeof(fl_verified_track_result));
  return off;
}

extern "C" void fl_tracker_destroy(fl_tracker *trk)
{
  if (!trk) return;
  if (trk->ctx->device >= 0) {
    (void)hipSetDevice(trk->ctx->device);
    (void)hipStreamSynchronize(trk->ctx->stream);
    for (hipEvent_t e : trk->ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : trk->ev_scene)
      if (e) (void)hipEventDestroy(e);
    if (trk->d_mem) (void)hipFree(trk->d_mem);
    if (trk->h_stage) (void)hipHostFree(trk->h_stage);
  }
  if (trk->owns_ctx) delete trk->ctx;
  delete trk;
}

// fl_tracker_create_meshes, `who` in the texts; name_mesh: a refusal says which mesh (fl_tracker_create's texts stay as they were)
static int tracker_create(fl_context *ctx, const char *who, bool name_mesh, const fl_mesh *meshes, int n_meshes, int w, int h, int max_frames,
                          int max_tracks, int max_crop_px, fl_tracker **out)
{
  if (!ctx || !out) return FL_ERR_INVALID;
  int rc = tracker_meshes_ok(ctx, who, name_mesh, meshes, n_meshes);
  if (rc || (rc = tracker_sizes_ok(ctx, w, h, max_frames, max_tracks, max_crop_px))) return rc;
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "%s: the context has no device", who);
  FL_HIP(ctx, hipSetDevice(ctx->device));
  // the meshes back to back, every triangle's indices moved on by its mesh's first vertex, and the range of each
  std::vector<float> vtx;
  std::vector<int32_t> tri;
  std::vector<FlMeshRange> ranges((size_t)n_meshes);
  int max_n_t = 0;
  for (int m = 0; m < n_meshes; ++m) {
    const int32_t v_first = (int32_t)(vtx.size() / 3);
    ranges[m] = FlMeshRange{(int32_t)(tri.size() / 3), meshes[m].n_triangles};
    max_n_t = std::max(max_n_t, meshes[m].n_triangles);
    vtx.insert(vtx.end(), meshes[m].vertices, meshes[m].vertices + (size_t)meshes[m].n_vertices * 3);
    for (size_t i = 0; i < (size_t)meshes[m].n_triangles * 3; ++i) tri.push_back(meshes[m].triangles[i] + v_first);
  }
  fl_tracker *trk = tracker_new(ctx, false, w, h, max_frames, max_tracks, max_crop_px);
  trk->n_meshes = n_meshes;
  trk->n_t = meshes[0].n_triangles;
  trk->max_n_t = max_n_t;
  trk->chunk = std::min(max_tracks, fl_render_chunk_views(w, h));
  trk->frame_stride = fl_align((size_t)w * h * 2, 256);
  trk->ws_one = fl_align(fl_icp_ws_bytes(max_crop_px), 256);
  auto fail = [&](hipError_t e, const char *what) {
    fl_set_error(ctx, FL_ERR_HIP, "%s: %s -> %s", who, what, hipGetErrorString(e));
    fl_tracker_destroy(trk);
    return FL_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipMalloc((void **)&trk->d_mem, carve_device(trk, nullptr, vtx.size() / 3, tri.size() / 3))) != hipSuccess) { trk->d_mem = nullptr; return fail(e, "hipMalloc"); }
  if ((e = hipHostMalloc((void **)&trk->h_stage, fl_track_stage(trk->stage, nullptr, max_tracks), hipHostMallocDefault)) != hipSuccess) { trk->h_stage = nullptr; return fail(e, "hipHostMalloc"); }
  for (hipEvent_t &v : trk->ev)
    if ((e = hipEventCreate(&v)) != hipSuccess) { v = nullptr; return fail(e, "hipEventCreate"); }
  carve_device(trk, trk->d_mem, vtx.size() / 3, tri.size() / 3);
  fl_track_stage(trk->stage, trk->h_stage, max_tracks);
  // the meshes, once; the one class every slot's "template" belongs to starts at g = 0
  if ((e = hipMemcpyAsync((void *)trk->d_vtx, vtx.data(), vtx.size() * 4, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
      (e = hipMemcpyAsync((void *)trk->d_tri, tri.data(), tri.size() * 4, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
      (e = hipMemcpyAsync((void *)trk->d_ranges, ranges.data(), ranges.size() * sizeof(FlMeshRange), hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
      (e = hipMemsetAsync(trk->d_class_first, 0, 4, ctx->stream)) != hipSuccess || (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
    return fail(e, "mesh upload");
  *out = trk;
  return FL_OK;
}

extern "C" int fl_tracker_create_meshes(fl_context *ctx, const fl_mesh *meshes, int n_meshes, int w, int h, int max_frames, int max_tracks,
                                        int max_crop_px, fl_tracker **out)
{
  return tracker_create(ctx, "fl_tracker_create_meshes", true, meshes, n_meshes, w, h, max_frames, max_tracks, max_crop_px, out);
}

extern "C" int fl_tracker_create(fl_context *ctx, const float *vertices, int n_vertices, const int32_t *triangles, int n_triangles,
                                 int w, int h, int max_frames, int max_tracks, int max_crop_px, fl_tracker **out)
{
  const fl_mesh mesh = {vertices, triangles, n_vertices, n_triangles};
  return tracker_create(ctx, "fl_tracker_create", false, &mesh, 1, w, h, max_frames, max_tracks, max_crop_px, out);
}

extern "C" int fl_tracker_num_meshes(const fl_tracker *trk) { return trk ? trk->n_meshes : FL_ERR_INVALID; }

// Development / test aid, exported but not part of the ABI: a tracker without a device (its own context, device = -1), for the
// argument checks of fl_track_batch and fl_verify_batch, which come before their first HIP call.  fl_tracker_destroy releases both.
extern "C" int fl_dev_tracker_create_host(int w, int h, int max_frames, int max_tracks, int max_crop_px, fl_tracker **out)
{
  if (!out) return FL_ERR_INVALID;
  fl_context *ctx = new fl_context();
  ctx->device = -1;
  if (tracker_sizes_ok(ctx, w, h, max_frames, max_tracks, max_crop_px)) { delete ctx; return FL_ERR_INVALID; }
  *out = tracker_new(ctx, true, w, h, max_frames, max_tracks, max_crop_px);
  return FL_OK;
}

// The same with fl_tracker_create_meshes' mesh checks in front and the number of meshes kept: for the refusals of the *_meshes
// entry points.  A refusal's text dies with the context it was written to; fl_tracker_create_meshes on a context without a
// device gives the same refusals with their text.
extern "C" int fl_dev_tracker_create_host_meshes(const fl_mesh *meshes, int n_meshes, int w, int h, int max_frames, int max_tracks, int max_crop_px,
                                                 fl_tracker **out)
{
  if (!out) return FL_ERR_INVALID;
  fl_context *ctx = new fl_context();
  ctx->device = -1;
  if (tracker_meshes_ok(ctx, "fl_dev_tracker_create_host_meshes", true, meshes, n_meshes) ||
      tracker_sizes_ok(ctx, w, h, max_frames, max_tracks, max_crop_px)) { delete ctx; return FL_ERR_INVALID; }
  fl_tracker *trk = tracker_new(ctx, true, w, h, max_frames, max_tracks, max_crop_px);
  trk->n_meshes = n_meshes;
  trk->n_t = meshes[0].n_triangles;
  *out = trk;
  return FL_OK;
}

// ---- the steps of a call (fl_track_internal.h) ---------------------------------------------------------------------------------
int fl_tracker_check_call(fl_tracker *trk, const char *who, int n_frames, const uint16_t *const *depth, int mem, int n, const int32_t *frame_of,
                          const int32_t *mesh_of, const float *poses13, const fl_intrinsics *K, const void *results)
{
  if (!trk) return FL_ERR_INVALID;
  fl_context *ctx = trk->ctx;
  if (!depth || !frame_of || !poses13 || !K || !results) return fl_set_error(ctx, FL_ERR_INVALID, "%s: null pointer", who);
  if (mem != FL_MEM_HOST && mem != FL_MEM_DEVICE) return fl_set_error(ctx, FL_ERR_INVALID, "%s: bad mem %d", who, mem);
  if (n_frames < 1 || n_frames > trk->max_frames || n < 1 || n > trk->max_tracks)
    return fl_set_error(ctx, FL_ERR_INVALID, "%s: n_frames %d outside 1..%d or %d poses outside 1..%d", who, n_frames, trk->max_frames, n, trk->max_tracks);
  for (int i = 0; i < n_frames; ++i)
    if (!depth[i]) return fl_set_error(ctx, FL_ERR_INVALID, "%s: depth[%d] is null", who, i);
  for (int t = 0; t < n; ++t)
    if (frame_of[t] < 0 || frame_of[t] >= n_frames)
      return fl_set_error(ctx, FL_ERR_INVALID, "%s: frame index %d of pose %d outside [0, %d)", who, frame_of[t], t, n_frames);
  for (int t = 0; mesh_of && t < n; ++t)
    if (mesh_of[t] < 0 || mesh_of[t] >= trk->n_meshes)
      return fl_set_error(ctx, FL_ERR_INVALID, "%s: mesh index %d of pose %d outside [0, %d)", who, mesh_of[t], t, trk->n_meshes);
  for (int t = 0; t < n; ++t)
    if (!fl_finite_all(poses13 + (size_t)13 * t, 12)) return fl_set_error(ctx, FL_ERR_INVALID, "%s: non-finite pose %d", who, t);
  if (K->width != trk->w || K->height != trk->h)
    return fl_set_error(ctx, FL_ERR_INVALID, "%s: intrinsics are %dx%d, tracker created for %dx%d", who, K->width, K->height, trk->w, trk->h);
  if (!(std::isfinite(K->fx) && K->fx > 0 && std::isfinite(K->fy) && K->fy > 0 && std::isfinite(K->cx) && std::isfinite(K->cy)))
    return fl_set_error(ctx, FL_ERR_INVALID, "%s: fx, fy must be finite and > 0, cx, cy finite", who);
  return FL_OK;
}

int fl_tracker_stage(fl_tracker *trk, hipEvent_t ev_start, int n_frames, const uint16_t *const *depth, int mem, int n, const int32_t *frame_of,
                     const int32_t *mesh_of, const float *poses13, float *poses_keep)
{
  fl_context *ctx = trk->ctx;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_context_join(ctx)) return rc;    // a detector's pipelined ICP stage on this context comes first
  const size_t px = (size_t)trk->w * trk->h, T = (size_t)n;
  hipStream_t st = ctx->stream;
  FL_HIP(ctx, hipEventRecord(ev_start, st));
  for (int i = 0; i < n_frames; ++i)
    FL_HIP(ctx, hipMemcpyAsync(trk->d_frames + trk->frame_stride * i, depth[i], px * 2,
                               mem == FL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  memcpy(trk->stage.poses, poses13, T * 13 * 4);
  memcpy(trk->stage.frame_of, frame_of, T * 4);
  FL_HIP(ctx, hipMemcpyAsync(poses_keep ? poses_keep : trk->d_poses, trk->stage.poses, T * 13 * 4, hipMemcpyHostToDevice, st));
  if (poses_keep) FL_HIP(ctx, hipMemcpyAsync(trk->d_poses, poses_keep, T * 13 * 4, hipMemcpyDeviceToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(trk->d_frame_of, trk->stage.frame_of, T * 4, hipMemcpyHostToDevice, st));
  // the meshes only where there is a choice: a tracker of one mesh, or a call that names none, runs the one-mesh kernels on mesh 0
  const bool multi = mesh_of && trk->n_meshes > 1;
  trk->call_ranges = multi ? trk->d_ranges : nullptr;
  trk->call_mesh_of = multi ? trk->d_mesh_of : nullptr;
  if (multi) {
    memcpy(trk->stage.mesh_of, mesh_of, T * 4);
    FL_HIP(ctx, hipMemcpyAsync(trk->d_mesh_of, trk->stage.mesh_of, T * 4, hipMemcpyHostToDevice, st));
  }
  return FL_OK;
}

int fl_tracker_render(fl_tracker *trk, int n, float fx, float fy, float cx, float cy)
{
  const FlRenderMesh mesh = {trk->d_vtx, nullptr, nullptr, trk->d_tri, trk->n_t};
  const float headlight[3] = {0.f, 0.f, 1.f};
  const size_t px = (size_t)trk->w * trk->h;
  for (int v0 = 0; v0 < n; v0 += trk->chunk)
    if (int rc = fl_launch_render_chunk(trk->ctx, mesh, trk->d_poses + (size_t)13 * v0, std::min(trk->chunk, n - v0), trk->w, trk->h, fx, fy, cx, cy,
                                        headlight, FL_RENDER_AMBIENT, trk->d_keys, nullptr, trk->d_render + (size_t)v0 * px, nullptr, nullptr,
                                        trk->call_ranges, trk->call_mesh_of ? trk->call_mesh_of + v0 : nullptr, trk->max_n_t))
      return rc;
  return FL_OK;
}

int fl_tracker_results(fl_tracker *trk, const void *d_records, size_t bytes, void *results)
{
  fl_context *ctx = trk->ctx;
  FL_HIP(ctx, hipMemcpyAsync(trk->stage.results, d_records, bytes, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(results, trk->stage.results, bytes);
  return FL_OK;
}

// device time of the last fl_track_batch by stage, summed over its passes: {copy, render, rects, ICP, finish} in ms
extern "C" int fl_dev_tracker_stage_ms(fl_tracker *trk, float out[5])
{
  if (!trk || !out || trk->last_passes < 1) return FL_ERR_INVALID;
  for (int k = 0; k < 5; ++k) out[k] = 0.f;
  float ms = 0.f;
  if (hipEventElapsedTime(&ms, trk->ev[0], trk->ev[1]) != hipSuccess) return FL_ERR_HIP;
  out[0] = ms;
  for (int p = 0; p < trk->last_passes; ++p)
    for (int k = 0; k < 4; ++k) {
      if (hipEventElapsedTime(&ms, trk->ev[1 + 4 * p + k], trk->ev[2 + 4 * p + k]) != hipSuccess) return FL_ERR_HIP;
      out[1 + k] += ms;
    }
  return FL_OK;
}

// fl_track_params as given or the defaults, refused where out of range
static int track_params(fl_context *ctx, const fl_track_params *params, fl_track_params &P)
{
  P = params ? *params : k_track_defaults;
  if (P.passes < 1 || P.passes > FL_TRACK_MAX_PASSES || P.margin_px < 0 || P.margin_px > FL_RENDER_MAX_DIM || P.icp_it_thr < 0 ||
      !std::isfinite(P.dist_mean_thr) || !std::isfinite(P.dist_diff_thr) || !std::isfinite(P.max_dist_mean) || !std::isfinite(P.min_px_ratio) ||
      (P.icp_mode != FL_ICP_PARITY && P.icp_mode != FL_ICP_FAST && P.icp_mode != FL_ICP_POINT_TO_PLANE))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_params: passes 1..%d, margin_px 0..%d, icp_it_thr >= 0, finite thresholds, a known icp_mode",
                        FL_TRACK_MAX_PASSES, FL_RENDER_MAX_DIM);
  return FL_OK;
}

// Steps 1 to 5 of a tracking call, queued: the inputs, then P.passes passes.  Afterwards d_out holds the records, d_lost who is
// not tracked and d_poses the pose of every track that is.
static int track_passes(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_tracks, const int32_t *frame_of_track,
                        const int32_t *mesh_of_track, const float *poses13, const fl_intrinsics *K, const fl_track_params &P)
{
  fl_context *ctx = trk->ctx;
  int rc;
  // 1. the inputs; the poses stay in d_poses_in too (a lost track reports the pose it came in with)
  if ((rc = fl_tracker_stage(trk, trk->ev[0], n_frames, depth, mem, n_tracks, frame_of_track, mesh_of_track, poses13, trk->d_poses_in))) return rc;
  const size_t T = (size_t)n_tracks;
  hipStream_t st = ctx->stream;
  FL_HIP(ctx, hipMemsetAsync(trk->d_lost, 0, T * 4, st));
  FL_HIP(ctx, hipMemsetAsync(trk->d_out, 0, T * sizeof(fl_track_result), st));
  FL_HIP(ctx, hipEventRecord(trk->ev[1], st));

  TrackArgs a = {n_tracks, trk->w, trk->h, P.margin_px, trk->max_crop_px, K->fx, K->fy, K->cx, K->cy,          // in TrackArgs' order
                 trk->d_render, trk->d_frame_of, trk->d_poses, trk->d_poses_in, trk->d_lost, trk->d_pyr, trk->d_depth_ptrs, trk->d_jobs,
                 trk->d_res, trk->d_out, P.max_dist_mean, P.min_px_ratio};
  const FlDetectionTables tab = {trk->w, trk->h, trk->max_crop_px, nullptr, 0, 0, 0, trk->d_pyr, trk->d_class_first, trk->d_poses,
                                 trk->d_depth_ptrs, nullptr, 0};
  const fl_recognition_params rp = {0.f, P.icp_it_thr, P.dist_mean_thr, P.dist_diff_thr, P.icp_mode};
  for (int pass = 0; pass < P.passes; ++pass) {
    hipEvent_t *ev = trk->ev + 2 + 4 * pass;
    // 2. the render, at the model K whatever the scene's K is
    if ((rc = fl_tracker_render(trk, n_tracks, (float)MODEL_F, (float)MODEL_F, (float)MODEL_CX, (float)MODEL_CY))) return rc;
    FL_HIP(ctx, hipEventRecord(ev[0], st));
    // 3. rectangles, the render in 0.1 mm, the job records
    hipLaunchKernelGGL(k_track_rects, dim3(n_tracks), dim3(TB), 0, st, a);
    FL_HIP(ctx, hipGetLastError());
    FL_HIP(ctx, hipEventRecord(ev[1], st));
    // 4. one ICP launch over the slots (a slot whose job has frame = -1 leaves its zeroed result alone)
    FL_HIP(ctx, hipMemsetAsync(trk->d_res, 0, T * sizeof(fl_recognition_result), st));
    if ((rc = fl_launch_detection_tables(ctx, tab, n_tracks, K, &rp, (const uint16_t *)trk->d_frames, trk->frame_stride, trk->d_icp, trk->ws_one, 1,
                                         trk->d_jobs, trk->d_res, false)))
      return rc;
    FL_HIP(ctx, hipEventRecord(ev[2], st));
    // 5. lost rule, result records, the next pass's poses
    hipLaunchKernelGGL(k_track_finish, dim3((n_tracks + 63) / 64), dim3(64), 0, st, a);
    FL_HIP(ctx, hipGetLastError());
    FL_HIP(ctx, hipEventRecord(ev[3], st));
  }
  return FL_OK;
}

extern "C" int fl_track_batch_meshes(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_tracks,
                                     const int32_t *frame_of_track, const int32_t *mesh_of_track, const float *poses13, const fl_intrinsics *K,
                                     const fl_track_params *params, fl_track_result *results)
{
  int rc = fl_tracker_check_call(trk, "fl_track_batch", n_frames, depth, mem, n_tracks, frame_of_track, mesh_of_track, poses13, K, results);
  if (rc) return rc;
  fl_context *ctx = trk->ctx;
  fl_track_params P;
  if ((rc = track_params(ctx, params, P))) return rc;
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "fl_track_batch: the tracker has no device");
  if ((rc = track_passes(trk, n_frames, depth, mem, n_tracks, frame_of_track, mesh_of_track, poses13, K, P))) return rc;
  // 6. one copy, one wait
  if ((rc = fl_tracker_results(trk, trk->d_out, (size_t)n_tracks * sizeof(fl_track_result), results))) return rc;
  trk->last_passes = P.passes;
  trk->track_verified = false;
  return FL_OK;
}

extern "C" int fl_track_batch(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_tracks,
                              const int32_t *frame_of_track, const float *poses13, const fl_intrinsics *K, const fl_track_params *params,
                              fl_track_result *results)
{
  return fl_track_batch_meshes(trk, n_frames, depth, mem, n_tracks, frame_of_track, nullptr, poses13, K, params, results);
}

// device time of the stages the last fl_track_batch_verified ran after its passes: {fused render and score, finish and pick} in
// ms; the passes themselves are fl_dev_tracker_stage_ms's
extern "C" int fl_dev_tracker_track_verified_ms(fl_tracker *trk, float out[2])
{
  if (!trk || !out || !trk->track_verified) return FL_ERR_INVALID;
  const hipEvent_t *ev = trk->ev + FL_TRACK_EVENTS + FL_VERIFY_EVENTS;
  for (int k = 0; k < 2; ++k)
    if (hipEventElapsedTime(out + k, ev[k], ev[k + 1]) != hipSuccess) return FL_ERR_HIP;
  return FL_OK;
}

static const fl_track_verify_params k_track_verify_defaults = {{10, 1, 0.f, 0.f}, 0, 0};

extern "C" int fl_track_batch_verified_meshes(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_tracks,
                                              const int32_t *frame_of_track, const int32_t *mesh_of_track, const float *poses13, int n_groups,
                                              const int32_t *group_first, const fl_intrinsics *K, const fl_track_params *params,
                                              const fl_track_verify_params *vparams, fl_verified_track_result *results)
{
  int rc = fl_tracker_check_call(trk, "fl_track_batch_verified", n_frames, depth, mem, n_tracks, frame_of_track, mesh_of_track, poses13, K, results);
  if (rc || (rc = fl_verify_check_call(trk, "fl_track_batch_verified", K, n_tracks, n_groups, group_first))) return rc;
  fl_context *ctx = trk->ctx;
  fl_track_params P;
  if ((rc = track_params(ctx, params, P))) return rc;
  const fl_track_verify_params V = vparams ? *vparams : k_track_verify_defaults;
  if (!fl_verify_params_ok(V.verify)) return fl_set_error(ctx, FL_ERR_INVALID, FL_VERIFY_PARAMS_TEXT);
  if (V.keep_input != 0 && V.keep_input != 1) return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_verify_params: keep_input is 0 or 1");
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "fl_track_batch_verified: the tracker has no device");

  if ((rc = track_passes(trk, n_frames, depth, mem, n_tracks, frame_of_track, mesh_of_track, poses13, K, P))) return rc;
  // 6. the groups, and clear accumulators: a lost track's workgroups leave theirs alone
  hipStream_t st = ctx->stream;
  hipEvent_t *ev = trk->ev + FL_TRACK_EVENTS + FL_VERIFY_EVENTS;
  const int n_wg = V.keep_input ? 2 * n_tracks : n_tracks;
  if (group_first) {
    memcpy(trk->stage.group_first, group_first, ((size_t)n_groups + 1) * 4);
    FL_HIP(ctx, hipMemcpyAsync(trk->d_group_first, trk->stage.group_first, ((size_t)n_groups + 1) * 4, hipMemcpyHostToDevice, st));
  }
  FL_HIP(ctx, hipMemsetAsync(trk->d_vacc, 0, (size_t)n_wg * sizeof(FlVerifyAcc), st));
  FL_HIP(ctx, hipEventRecord(ev[0], st));
  // 7. every tracked pose, and with keep_input every tracked track's input pose, rendered at the scene's K in LDS and scored: one
  // launch, always the fused kernel (the render images hold the passes' model-camera renders x 10)
  const FlVerifyFusedJob j = {n_wg, trk->w, trk->h, V.verify.tau_mm, (float)K->fx, (float)K->fy, (float)K->cx, (float)K->cy,
                              {trk->d_vtx, nullptr, nullptr, trk->d_tri, trk->n_t}, trk->d_poses, 13, trk->d_frames, trk->frame_stride, trk->d_frame_of, 1,
                              nullptr, nullptr, trk->call_mesh_of, trk->d_vacc, trk->d_lost, n_tracks, trk->d_poses_in, trk->call_ranges};
  if ((rc = fl_launch_verify_fused(ctx, j))) return rc;
  FL_HIP(ctx, hipEventRecord(ev[1], st));
  // 8. the records and the decision per track, then the best of every group
  const TrackVerifiedArgs a = {n_tracks, group_first ? n_groups : 0, trk->w, trk->h, V.verify.min_model_px, V.keep_input, V.verify.min_inlier_ratio,
                               V.verify.max_behind_ratio, trk->d_out, trk->d_poses_in, (const FlVerifyAcc *)trk->d_vacc,
                               group_first ? trk->d_group_first : nullptr, trk->d_vout};      // in TrackVerifiedArgs' order
  hipLaunchKernelGGL(k_track_verified_finish, dim3((n_tracks + 63) / 64), dim3(64), 0, st, a);
  FL_HIP(ctx, hipGetLastError());
  if (group_first) {
    hipLaunchKernelGGL(k_track_verified_pick, dim3((n_groups + 63) / 64), dim3(64), 0, st, a);
    FL_HIP(ctx, hipGetLastError());
  }
  FL_HIP(ctx, hipEventRecord(ev[2], st));
  // 9. one copy, one wait
  if ((rc = fl_tracker_results(trk, trk->d_vout, (size_t)n_tracks * sizeof(fl_verified_track_result), results))) return rc;
  trk->last_passes = P.passes;
  trk->track_verified = true;
  return FL_OK;
}

extern "C" int fl_track_batch_verified(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_tracks,
                                       const int32_t *frame_of_track, const float *poses13, int n_groups, const int32_t *group_first,
                                       const fl_intrinsics *K, const fl_track_params *params, const fl_track_verify_params *vparams,
                                       fl_verified_track_result *results)
{
  return fl_track_batch_verified_meshes(trk, n_frames, depth, mem, n_tracks, frame_of_track, nullptr, poses13, n_groups, group_first, K, params,
                                        vparams, results);
}
