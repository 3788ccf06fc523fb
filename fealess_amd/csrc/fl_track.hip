// fl_track.hip -- 6-DoF model-based tracking (fl_tracker_create / fl_track_batch, include/fealess_hip.h): the batched z-buffer
// rasteriser of fl_render.hip and the ICP workgroup per job of fl_icp.hip, joined on the device.  No counterpart in the
// reference, which links a 2-D KCF box tracker it never calls (test/linemod_acq.cpp:108-150).
//
// One pass of a call, all on the context's stream:
//   fl_launch_render_chunk   the mesh at every track's pose, depth only, K = 608 / 608 / 320 / 240 (the K crop_clouds
//                            back-projects a model image with, fl_icp.hip; ICP/detection.cpp:35-36)
//   k_track_rects            one workgroup per track: bounding box of the render, the rectangle rule, the render x 10 inside
//                            rect_model, and the records the ICP kernel's job-list path reads for slot t: pyr[t], depth_ptrs[t],
//                            jobs[t] (the pose is already at poses[13 t]); frame = -1 for a slot that has nothing to refine
//   fl_launch_detection_tables   k_icp_pipeline over the n_tracks slots, through its job list: class_first = {0}, so slot t's
//                            "template" is g = t
//   k_track_finish           one thread per track: the lost rule, the result record, the pose of the next pass
// The rectangle rule is stated in integers in include/fealess_hip.h and in numpy in tests/track_model.py; the shift is fp64,
// one IEEE operation per operator (the Makefile's -ffp-contract=off: hipcc would contract a * b + c otherwise).
//
// fl_verify_batch (hypothesis verification on the tracker's mesh, frame slots and render images) is the second half of the file.
#include "fl_internal.h"
#include <math.h>
#include <string.h>
#include <algorithm>

namespace {

constexpr int TB = 256;                         // k_track_rects: threads per track
constexpr int TRACK_EVENTS = 2 + 4 * FL_TRACK_MAX_PASSES;
constexpr int VERIFY_EVENTS = 5;
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

__device__ __forceinline__ void bbox_add(int idx, int w, int &x0, int &x1, int &y0, int &y1)
{
  const int y = idx / w, x = idx - y * w;
  x0 = min(x0, x); x1 = max(x1, x);
  y0 = min(y0, y); y1 = max(y1, y);
}

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

// ---- verification (fl_verify_batch): the render laid over the depth frame ----------------------------------------------------
// k_verify_score   one workgroup per (pose, strip of V_STRIP_PX pixels): the contract's per-pixel rule, reduced in the wave and
//                  in the workgroup, then one integer atomic per counter into the pose's FlVerifyAcc -- exact whatever the order
// k_verify_finish  one thread per pose: rect, ratios, accepted; best = accepted when there are no groups
// k_verify_pick    one thread per group: the best accepted member
// The strip: k_track_rects walks a whole 640 x 480 render with one workgroup and is bound by the latency of its 19 rounds of
// loads.  Here a thread issues its V_LOADS 16-byte render loads at once and never loops, so a workgroup lasts about two memory
// round trips (render, then the scene under the non-zero groups) and a strip is VB * V_LOADS * 8 = 8192 pixels, 16 KB of
// render: 38 workgroups = 152 waves per 640 x 480 pose.  A shorter strip would only add workgroups whose reduction and
// atomics outweigh their one load per thread; a longer one brings the loop and its serial round trips back.  Measured:
// DESIGN.md section 0, row f6.
constexpr int VB = 256;                         // k_verify_score: threads per workgroup
constexpr int V_LOADS = 4;                      // loads in flight per thread
constexpr int V_STRIP_PX = VB * V_LOADS * 8;    // pixels per strip, on both paths

// A pose's accumulators, zeroed before the launch.  box = {w - x0, h - y0, x1 + 1, y1 + 1}: zero means "no pixel" and every
// entry grows, so one atomicMax serves the four sides.
struct FlVerifyAcc {
  int32_t n[5];                                 // model, missing, inlier, front, behind
  int32_t box[4];
  int32_t pad;
  unsigned long long sum;                       // of |d| over the inliers
};

struct VerifyArgs {
  int n_poses, n_groups, w, h, n_strips, tau, min_model_px;
  float min_inlier_ratio, max_behind_ratio;
  const uint16_t *render;                       // n_poses images of w * h, back to back
  const uint8_t *frames;                        // the frame slots
  size_t frame_stride;
  const int32_t *frame_of, *group_first;        // group_first: null when every pose is its own group
  FlVerifyAcc *acc;
  fl_verify_result *out;
};

struct VerifyCount {                            // scalars and sums of conditions, so that it stays in registers
  int model, missing, inlier, front, behind;
  int sum;                                      // a workgroup's share: at most 8192 * 65535 < 2^30
  int x0, x1, y0, y1;
};

__device__ __forceinline__ void verify_px(int r, int s, int idx, int w, int tau, VerifyCount &c)
{
  if (r == 0) return;
  bbox_add(idx, w, c.x0, c.x1, c.y0, c.y1);
  const int d = s - r, ad = d < 0 ? -d : d;     // ints: nothing wraps in 16 bits
  const bool seen = s != 0, in = seen && ad <= tau;
  c.model += 1;
  c.missing += !seen;
  c.inlier += in;
  c.sum += in ? ad : 0;
  c.front += seen && d < -tau;
  c.behind += seen && d > tau;
}

__global__ __launch_bounds__(VB) void k_verify_score(VerifyArgs a)
{
  __shared__ int red[10][VB / FL_WAVE];
  const int t = blockIdx.x / a.n_strips, strip = blockIdx.x - t * a.n_strips, tid = threadIdx.x;
  const int px = a.w * a.h;                     // <= FL_RENDER_MAX_DIM^2, fits an int
  const uint16_t *img = a.render + (size_t)t * px;
  const uint16_t *scn = (const uint16_t *)(a.frames + a.frame_stride * (size_t)a.frame_of[t]);
  VerifyCount c = {0, 0, 0, 0, 0, 0, a.w, -1, a.h, -1};
  if ((px & 7) == 0) {                          // renders and frame slots start on 16-byte boundaries: eight pixels per load
    const uint4 *r4 = (const uint4 *)img, *s4 = (const uint4 *)scn;
    const int n8 = px / 8, i0 = strip * (V_STRIP_PX / 8) + tid;
    uint4 rv[V_LOADS], sv[V_LOADS];
#pragma unroll
    for (int u = 0; u < V_LOADS; ++u) {
      const int i = i0 + u * VB;
      rv[u] = i < n8 ? r4[i] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < V_LOADS; ++u)           // the scene only under a group that has a rendered pixel
      sv[u] = (rv[u].x | rv[u].y | rv[u].z | rv[u].w) != 0u ? s4[i0 + u * VB] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (int u = 0; u < V_LOADS; ++u) {
      if ((rv[u].x | rv[u].y | rv[u].z | rv[u].w) == 0u) continue;
      const int p = 8 * (i0 + u * VB);
      const unsigned rw[4] = {rv[u].x, rv[u].y, rv[u].z, rv[u].w}, sw[4] = {sv[u].x, sv[u].y, sv[u].z, sv[u].w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        verify_px((int)(rw[k] & 0xffffu), (int)(sw[k] & 0xffffu), p + 2 * k, a.w, a.tau, c);
        verify_px((int)(rw[k] >> 16), (int)(sw[k] >> 16), p + 2 * k + 1, a.w, a.tau, c);
      }
    }
  } else {
    const int p0 = strip * V_STRIP_PX + tid;
#pragma unroll 1
    for (int k0 = 0; k0 < V_STRIP_PX / VB; k0 += V_LOADS) {
      int rv[V_LOADS], sv[V_LOADS];
#pragma unroll
      for (int u = 0; u < V_LOADS; ++u) {
        const int p = p0 + (k0 + u) * VB;
        rv[u] = p < px ? (int)img[p] : 0;
      }
#pragma unroll
      for (int u = 0; u < V_LOADS; ++u)
        sv[u] = rv[u] ? (int)scn[p0 + (k0 + u) * VB] : 0;
#pragma unroll
      for (int u = 0; u < V_LOADS; ++u)
        verify_px(rv[u], sv[u], p0 + (k0 + u) * VB, a.w, a.tau, c);
    }
  }
  int v[10] = {c.model, c.missing, c.inlier, c.front, c.behind, c.sum, -c.x0, c.x1, -c.y0, c.y1};   // 0..5 add, 6..9 max
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += __shfl_xor(v[k], s, FL_WAVE);
#pragma unroll
    for (int k = 6; k < 10; ++k) v[k] = max(v[k], __shfl_xor(v[k], s, FL_WAVE));
  }
  if ((tid & (FL_WAVE - 1)) == 0) {
#pragma unroll
    for (int k = 0; k < 10; ++k) red[k][tid / FL_WAVE] = v[k];
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int wv = 1; wv < VB / FL_WAVE; ++wv) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v[k] += red[k][wv];
#pragma unroll
    for (int k = 6; k < 10; ++k) v[k] = max(v[k], red[k][wv]);
  }
  if (v[0] == 0) return;                        // nothing rendered in this strip
  FlVerifyAcc *acc = a.acc + t;
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (v[k]) atomicAdd(&acc->n[k], v[k]);
  if (v[5]) atomicAdd(&acc->sum, (unsigned long long)(unsigned)v[5]);
  atomicMax(&acc->box[0], a.w + v[6]);
  atomicMax(&acc->box[1], a.h + v[8]);
  atomicMax(&acc->box[2], v[7] + 1);
  atomicMax(&acc->box[3], v[9] + 1);
}

__global__ __launch_bounds__(64) void k_verify_finish(VerifyArgs a)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= a.n_poses) return;
  const FlVerifyAcc c = a.acc[t];
  fl_verify_result o;
  memset(&o, 0, sizeof(o));                     // status = FL_OK; an empty render leaves every other field zero too
  if (c.n[0] > 0) {
    const int x0 = a.w - c.box[0], y0 = a.h - c.box[1];
    o.rect[0] = x0; o.rect[1] = y0; o.rect[2] = c.box[2] - x0; o.rect[3] = c.box[3] - y0;
    o.n_model = c.n[0]; o.n_missing = c.n[1]; o.n_inlier = c.n[2]; o.n_front = c.n[3]; o.n_behind = c.n[4];
    o.sum_abs_inlier = (int64_t)c.sum;
    o.inlier_ratio = (float)c.n[2] / (float)c.n[0];
    o.behind_ratio = (float)c.n[4] / (float)c.n[0];
    o.accepted = c.n[0] >= a.min_model_px && (a.min_inlier_ratio <= 0.f || o.inlier_ratio >= a.min_inlier_ratio) &&
                 (a.max_behind_ratio <= 0.f || o.behind_ratio <= a.max_behind_ratio);
  }
  o.best = a.group_first ? 0 : o.accepted;
  a.out[t] = o;
}

__global__ __launch_bounds__(64) void k_verify_pick(VerifyArgs a)
{
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= a.n_groups) return;
  int best = -1;
  long long bi = 0, bm = 1;
  for (int i = a.group_first[g]; i < a.group_first[g + 1]; ++i) {
    const fl_verify_result &r = a.out[i];
    if (!r.accepted) continue;                  // accepted: n_model >= min_model_px >= 1
    if (best < 0 || (long long)r.n_inlier * bm > bi * (long long)r.n_model) { best = i; bi = r.n_inlier; bm = r.n_model; }
  }
  if (best >= 0) a.out[best].best = 1;
}

bool finite_all(const float *p, size_t n)
{
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

}  // namespace

struct fl_tracker {
  fl_context *ctx = nullptr;
  bool owns_ctx = false;                        // fl_dev_tracker_create_host: a context without a device, released with the tracker
  int w = 0, h = 0, max_frames = 0, max_tracks = 0, max_crop_px = 0, n_t = 0;
  int chunk = 0;                                // views per render launch
  uint8_t *d_mem = nullptr;                     // the one device allocation
  const float *d_vtx = nullptr;
  const int32_t *d_tri = nullptr;
  uint8_t *d_frames = nullptr;
  size_t frame_stride = 0;
  uint16_t *d_render = nullptr;
  unsigned long long *d_keys = nullptr;
  uint8_t *d_icp = nullptr;
  size_t ws_one = 0;
  float *d_poses = nullptr, *d_poses_in = nullptr;
  int32_t *d_frame_of = nullptr, *d_lost = nullptr, *d_class_first = nullptr;
  FlPyrInfo *d_pyr = nullptr;
  const uint16_t **d_depth_ptrs = nullptr;
  FlRefineJob *d_jobs = nullptr;
  fl_recognition_result *d_res = nullptr;
  fl_track_result *d_out = nullptr;
  uint8_t *h_stage = nullptr;                   // pinned: poses | frame_of | results | group_first (stage_bytes)
  hipEvent_t ev[TRACK_EVENTS] = {nullptr};      // 0: start, 1: inputs on the device, then per pass render / rects / ICP / finish
  int last_passes = 0;
  // fl_verify_batch
  FlVerifyAcc *d_vacc = nullptr;
  fl_verify_result *d_vres = nullptr;
  int32_t *d_group_first = nullptr;             // max_tracks + 1 entries
  hipEvent_t vev[VERIFY_EVENTS] = {nullptr};    // start, inputs on the device, render, score, finish and pick
  bool verified = false;
};

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

extern "C" void fl_tracker_destroy(fl_tracker *trk)
{
  if (!trk) return;
  if (trk->ctx->device >= 0) {
    (void)hipSetDevice(trk->ctx->device);
    (void)hipStreamSynchronize(trk->ctx->stream);
    for (hipEvent_t e : trk->ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : trk->vev)
      if (e) (void)hipEventDestroy(e);
    if (trk->d_mem) (void)hipFree(trk->d_mem);
    if (trk->h_stage) (void)hipHostFree(trk->h_stage);
  }
  if (trk->owns_ctx) delete trk->ctx;
  delete trk;
}

// pinned: poses | frame_of | results (fl_track_batch's or fl_verify_batch's) | group_first
static size_t stage_results_bytes(int max_tracks)
{
  return fl_align(std::max(sizeof(fl_track_result), sizeof(fl_verify_result)) * (size_t)max_tracks, 256);
}
static size_t stage_bytes(int max_tracks)
{
  return fl_align((size_t)max_tracks * 13 * 4, 256) + fl_align((size_t)max_tracks * 4, 256) + stage_results_bytes(max_tracks) +
         ((size_t)max_tracks + 1) * 4;
}

extern "C" int fl_tracker_create(fl_context *ctx, const float *vertices, int n_vertices, const int32_t *triangles, int n_triangles,
                                 int w, int h, int max_frames, int max_tracks, int max_crop_px, fl_tracker **out)
{
  if (!ctx || !out) return FL_ERR_INVALID;
  int rc = fl_render_check_mesh(ctx, "fl_tracker_create", vertices, nullptr, n_vertices, triangles, n_triangles);
  if (rc || (rc = tracker_sizes_ok(ctx, w, h, max_frames, max_tracks, max_crop_px))) return rc;
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "fl_tracker_create: the context has no device");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  fl_tracker *trk = new fl_tracker();
  trk->ctx = ctx;
  trk->w = w; trk->h = h;
  trk->max_frames = max_frames; trk->max_tracks = max_tracks; trk->max_crop_px = max_crop_px;
  trk->n_t = n_triangles;
  trk->chunk = std::min(max_tracks, fl_render_chunk_views(w, h));
  const size_t px = (size_t)w * h, nv3 = (size_t)n_vertices * 3, nt3 = (size_t)n_triangles * 3, T = (size_t)max_tracks;
  trk->frame_stride = fl_align(px * 2, 256);
  trk->ws_one = fl_align(fl_icp_ws_bytes(max_crop_px), 256);
  size_t off = 0;
  auto take = [&](size_t b) { const size_t o = off; off += fl_align(b, 256); return o; };
  const size_t o_vtx = take(nv3 * 4), o_tri = take(nt3 * 4), o_frames = take(trk->frame_stride * max_frames), o_render = take(T * px * 2),
               o_keys = take((size_t)trk->chunk * px * 8), o_icp = take(trk->ws_one * T), o_poses = take(T * 13 * 4), o_pin = take(T * 13 * 4),
               o_fof = take(T * 4), o_lost = take(T * 4), o_cf = take(4), o_pyr = take(T * sizeof(FlPyrInfo)), o_dp = take(T * sizeof(void *)),
               o_jobs = take(T * sizeof(FlRefineJob)), o_res = take(T * sizeof(fl_recognition_result)), o_out = take(T * sizeof(fl_track_result)),
               o_vacc = take(T * sizeof(FlVerifyAcc)), o_vres = take(T * sizeof(fl_verify_result)), o_gf = take((T + 1) * 4);
  auto fail = [&](hipError_t e, const char *what) {
    fl_set_error(ctx, FL_ERR_HIP, "fl_tracker_create: %s -> %s", what, hipGetErrorString(e));
    fl_tracker_destroy(trk);
    return FL_ERR_HIP;
  };
  hipError_t e;
  if ((e = hipMalloc((void **)&trk->d_mem, off)) != hipSuccess) { trk->d_mem = nullptr; return fail(e, "hipMalloc"); }
  if ((e = hipHostMalloc((void **)&trk->h_stage, stage_bytes(max_tracks), hipHostMallocDefault)) != hipSuccess) { trk->h_stage = nullptr; return fail(e, "hipHostMalloc"); }
  for (hipEvent_t &v : trk->ev)
    if ((e = hipEventCreate(&v)) != hipSuccess) { v = nullptr; return fail(e, "hipEventCreate"); }
  for (hipEvent_t &v : trk->vev)
    if ((e = hipEventCreate(&v)) != hipSuccess) { v = nullptr; return fail(e, "hipEventCreate"); }
  uint8_t *m = trk->d_mem;
  trk->d_vtx = (const float *)(m + o_vtx);
  trk->d_tri = (const int32_t *)(m + o_tri);
  trk->d_frames = m + o_frames;
  trk->d_render = (uint16_t *)(m + o_render);
  trk->d_keys = (unsigned long long *)(m + o_keys);
  trk->d_icp = m + o_icp;
  trk->d_poses = (float *)(m + o_poses);
  trk->d_poses_in = (float *)(m + o_pin);
  trk->d_frame_of = (int32_t *)(m + o_fof);
  trk->d_lost = (int32_t *)(m + o_lost);
  trk->d_class_first = (int32_t *)(m + o_cf);
  trk->d_pyr = (FlPyrInfo *)(m + o_pyr);
  trk->d_depth_ptrs = (const uint16_t **)(m + o_dp);
  trk->d_jobs = (FlRefineJob *)(m + o_jobs);
  trk->d_res = (fl_recognition_result *)(m + o_res);
  trk->d_out = (fl_track_result *)(m + o_out);
  trk->d_vacc = (FlVerifyAcc *)(m + o_vacc);
  trk->d_vres = (fl_verify_result *)(m + o_vres);
  trk->d_group_first = (int32_t *)(m + o_gf);
  // the mesh, once; the one class every slot's "template" belongs to starts at g = 0
  if ((e = hipMemcpyAsync(m + o_vtx, vertices, nv3 * 4, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
      (e = hipMemcpyAsync(m + o_tri, triangles, nt3 * 4, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess ||
      (e = hipMemsetAsync(m + o_cf, 0, 4, ctx->stream)) != hipSuccess || (e = hipStreamSynchronize(ctx->stream)) != hipSuccess)
    return fail(e, "mesh upload");
  *out = trk;
  return FL_OK;
}

// Development / test aid, exported but not part of the ABI: a tracker without a device (its own context, device = -1), for the
// argument checks of fl_track_batch, which come before its first HIP call.  fl_tracker_destroy releases both.
extern "C" int fl_dev_tracker_create_host(int w, int h, int max_frames, int max_tracks, int max_crop_px, fl_tracker **out)
{
  if (!out) return FL_ERR_INVALID;
  fl_context *ctx = new fl_context();
  ctx->device = -1;
  if (tracker_sizes_ok(ctx, w, h, max_frames, max_tracks, max_crop_px)) { delete ctx; return FL_ERR_INVALID; }
  fl_tracker *trk = new fl_tracker();
  trk->ctx = ctx;
  trk->owns_ctx = true;
  trk->w = w; trk->h = h;
  trk->max_frames = max_frames; trk->max_tracks = max_tracks; trk->max_crop_px = max_crop_px;
  *out = trk;
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

extern "C" int fl_track_batch(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_tracks,
                              const int32_t *frame_of_track, const float *poses13, const fl_intrinsics *K, const fl_track_params *params,
                              fl_track_result *results)
{
  if (!trk) return FL_ERR_INVALID;
  fl_context *ctx = trk->ctx;
  if (!depth || !frame_of_track || !poses13 || !K || !results) return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_batch: null pointer");
  if (mem != FL_MEM_HOST && mem != FL_MEM_DEVICE) return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_batch: bad mem %d", mem);
  if (n_frames < 1 || n_frames > trk->max_frames || n_tracks < 1 || n_tracks > trk->max_tracks)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_batch: n_frames %d outside 1..%d or n_tracks %d outside 1..%d", n_frames, trk->max_frames,
                        n_tracks, trk->max_tracks);
  for (int i = 0; i < n_frames; ++i)
    if (!depth[i]) return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_batch: depth[%d] is null", i);
  for (int t = 0; t < n_tracks; ++t)
    if (frame_of_track[t] < 0 || frame_of_track[t] >= n_frames)
      return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_batch: frame_of_track[%d] = %d outside [0, %d)", t, frame_of_track[t], n_frames);
  for (int t = 0; t < n_tracks; ++t)
    if (!finite_all(poses13 + (size_t)13 * t, 12)) return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_batch: non-finite pose of track %d", t);
  if (K->width != trk->w || K->height != trk->h)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_batch: intrinsics are %dx%d, tracker created for %dx%d", K->width, K->height, trk->w, trk->h);
  if (!(std::isfinite(K->fx) && K->fx > 0 && std::isfinite(K->fy) && K->fy > 0 && std::isfinite(K->cx) && std::isfinite(K->cy)))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_batch: fx, fy must be finite and > 0, cx, cy finite");
  const fl_track_params P = params ? *params : k_track_defaults;
  if (P.passes < 1 || P.passes > FL_TRACK_MAX_PASSES || P.margin_px < 0 || P.margin_px > FL_RENDER_MAX_DIM || P.icp_it_thr < 0 ||
      !std::isfinite(P.dist_mean_thr) || !std::isfinite(P.dist_diff_thr) || !std::isfinite(P.max_dist_mean) || !std::isfinite(P.min_px_ratio) ||
      (P.icp_mode != FL_ICP_PARITY && P.icp_mode != FL_ICP_FAST && P.icp_mode != FL_ICP_POINT_TO_PLANE))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_track_params: passes 1..%d, margin_px 0..%d, icp_it_thr >= 0, finite thresholds, a known icp_mode",
                        FL_TRACK_MAX_PASSES, FL_RENDER_MAX_DIM);
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "fl_track_batch: the tracker has no device");

  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_context_join(ctx)) return rc;    // a detector's pipelined ICP stage on this context comes first
  const size_t px = (size_t)trk->w * trk->h, T = (size_t)n_tracks;
  hipStream_t st = ctx->stream;
  FL_HIP(ctx, hipEventRecord(trk->ev[0], st));
  // 1. frames into their slots, poses and frame indices to the device (through the pinned block)
  for (int i = 0; i < n_frames; ++i)
    FL_HIP(ctx, hipMemcpyAsync(trk->d_frames + trk->frame_stride * i, depth[i], px * 2,
                               mem == FL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  float *h_poses = (float *)trk->h_stage;
  int32_t *h_fof = (int32_t *)(trk->h_stage + fl_align((size_t)trk->max_tracks * 13 * 4, 256));
  fl_track_result *h_out = (fl_track_result *)((uint8_t *)h_fof + fl_align((size_t)trk->max_tracks * 4, 256));
  memcpy(h_poses, poses13, T * 13 * 4);
  memcpy(h_fof, frame_of_track, T * 4);
  FL_HIP(ctx, hipMemcpyAsync(trk->d_poses_in, h_poses, T * 13 * 4, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(trk->d_poses, trk->d_poses_in, T * 13 * 4, hipMemcpyDeviceToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(trk->d_frame_of, h_fof, T * 4, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipMemsetAsync(trk->d_lost, 0, T * 4, st));
  FL_HIP(ctx, hipMemsetAsync(trk->d_out, 0, T * sizeof(fl_track_result), st));
  FL_HIP(ctx, hipEventRecord(trk->ev[1], st));

  TrackArgs a;
  a.n_tracks = n_tracks;
  a.w = trk->w; a.h = trk->h;
  a.margin = P.margin_px;
  a.max_crop_px = trk->max_crop_px;
  a.fx = K->fx; a.fy = K->fy; a.cx = K->cx; a.cy = K->cy;
  a.render = trk->d_render;
  a.frame_of = trk->d_frame_of;
  a.poses = trk->d_poses;
  a.poses_in = trk->d_poses_in;
  a.lost = trk->d_lost;
  a.pyr = trk->d_pyr;
  a.depth_ptrs = trk->d_depth_ptrs;
  a.jobs = trk->d_jobs;
  a.res = trk->d_res;
  a.out = trk->d_out;
  a.max_dist_mean = P.max_dist_mean;
  a.min_px_ratio = P.min_px_ratio;
  const FlRenderMesh mesh = {trk->d_vtx, nullptr, nullptr, trk->d_tri, trk->n_t};
  const float headlight[3] = {0.f, 0.f, 1.f};
  const FlDetectionTables tab = {trk->w, trk->h, trk->max_crop_px, nullptr, 0, 0, 0, trk->d_pyr, trk->d_class_first, trk->d_poses,
                                 trk->d_depth_ptrs, nullptr, 0};
  const fl_recognition_params rp = {0.f, P.icp_it_thr, P.dist_mean_thr, P.dist_diff_thr, P.icp_mode};
  int rc;
  for (int pass = 0; pass < P.passes; ++pass) {
    hipEvent_t *ev = trk->ev + 2 + 4 * pass;
    // 2. the render, at the model K whatever the scene's K is
    for (int v0 = 0; v0 < n_tracks; v0 += trk->chunk) {
      const int n = std::min(trk->chunk, n_tracks - v0);
      if ((rc = fl_launch_render_chunk(ctx, mesh, trk->d_poses + (size_t)13 * v0, n, trk->w, trk->h, (float)MODEL_F, (float)MODEL_F, (float)MODEL_CX,
                                       (float)MODEL_CY, headlight, FL_RENDER_AMBIENT, trk->d_keys, nullptr, trk->d_render + (size_t)v0 * px, nullptr,
                                       nullptr)))
        return rc;
    }
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
  // 6. one copy, one wait
  FL_HIP(ctx, hipMemcpyAsync(h_out, trk->d_out, T * sizeof(fl_track_result), hipMemcpyDeviceToHost, st));
  FL_HIP(ctx, hipStreamSynchronize(st));
  memcpy(results, h_out, T * sizeof(fl_track_result));
  trk->last_passes = P.passes;
  return FL_OK;
}

static const fl_verify_params k_verify_defaults = {10, 1, 0.f, 0.f};
static_assert(sizeof(fl_verify_result) == 64, "fl_verify_result is 64 bytes (include/fealess_hip.h)");

// device time of the last fl_verify_batch by stage: {copy, render, score, finish and pick} in ms
extern "C" int fl_dev_tracker_verify_ms(fl_tracker *trk, float out[4])
{
  if (!trk || !out || !trk->verified) return FL_ERR_INVALID;
  for (int k = 0; k < 4; ++k)
    if (hipEventElapsedTime(out + k, trk->vev[k], trk->vev[k + 1]) != hipSuccess) return FL_ERR_HIP;
  return FL_OK;
}

extern "C" int fl_verify_batch(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_poses,
                               const int32_t *frame_of_pose, const float *poses13, int n_groups, const int32_t *group_first,
                               const fl_intrinsics *K, const fl_verify_params *params, fl_verify_result *results)
{
  if (!trk) return FL_ERR_INVALID;
  fl_context *ctx = trk->ctx;
  if (!depth || !frame_of_pose || !poses13 || !K || !results) return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: null pointer");
  if (mem != FL_MEM_HOST && mem != FL_MEM_DEVICE) return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: bad mem %d", mem);
  if (n_frames < 1 || n_frames > trk->max_frames || n_poses < 1 || n_poses > trk->max_tracks)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: n_frames %d outside 1..%d or n_poses %d outside 1..%d", n_frames, trk->max_frames,
                        n_poses, trk->max_tracks);
  for (int i = 0; i < n_frames; ++i)
    if (!depth[i]) return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: depth[%d] is null", i);
  for (int t = 0; t < n_poses; ++t)
    if (frame_of_pose[t] < 0 || frame_of_pose[t] >= n_frames)
      return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: frame_of_pose[%d] = %d outside [0, %d)", t, frame_of_pose[t], n_frames);
  for (int t = 0; t < n_poses; ++t)
    if (!finite_all(poses13 + (size_t)13 * t, 12)) return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: non-finite pose %d", t);
  if (K->width != trk->w || K->height != trk->h)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: intrinsics are %dx%d, tracker created for %dx%d", K->width, K->height, trk->w, trk->h);
  const float fx = (float)K->fx, fy = (float)K->fy, cx = (float)K->cx, cy = (float)K->cy;     // what the rasteriser gets
  if (!(std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy) && std::isfinite(fx) && fx > 0.f &&
        std::isfinite(fy) && fy > 0.f && std::isfinite(cx) && std::isfinite(cy)))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: fx, fy must be finite and > 0, cx, cy finite");
  if (group_first) {
    bool ok = n_groups >= 1 && n_groups <= trk->max_tracks && group_first[0] == 0;
    for (int g = 0; ok && g < n_groups; ++g) ok = group_first[g + 1] >= group_first[g] && group_first[g + 1] <= n_poses;
    if (!ok || group_first[n_groups] != n_poses)
      return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: group_first must have n_groups + 1 (n_groups 1..%d) non-decreasing entries from 0 to n_poses",
                          trk->max_tracks);
  }
  const fl_verify_params P = params ? *params : k_verify_defaults;
  if (P.tau_mm < 0 || P.tau_mm > 65535 || P.min_model_px < 1 || !std::isfinite(P.min_inlier_ratio) || !std::isfinite(P.max_behind_ratio))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_params: tau_mm 0..65535, min_model_px >= 1, finite thresholds");
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "fl_verify_batch: the tracker has no device");

  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_context_join(ctx)) return rc;    // a detector's pipelined ICP stage on this context comes first
  const size_t px = (size_t)trk->w * trk->h, T = (size_t)n_poses;
  hipStream_t st = ctx->stream;
  FL_HIP(ctx, hipEventRecord(trk->vev[0], st));
  // 1. frames into their slots; poses, frame indices and groups to the device (through the pinned block)
  for (int i = 0; i < n_frames; ++i)
    FL_HIP(ctx, hipMemcpyAsync(trk->d_frames + trk->frame_stride * i, depth[i], px * 2,
                               mem == FL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  float *h_poses = (float *)trk->h_stage;
  int32_t *h_fof = (int32_t *)(trk->h_stage + fl_align((size_t)trk->max_tracks * 13 * 4, 256));
  fl_verify_result *h_out = (fl_verify_result *)((uint8_t *)h_fof + fl_align((size_t)trk->max_tracks * 4, 256));
  int32_t *h_gf = (int32_t *)((uint8_t *)h_out + stage_results_bytes(trk->max_tracks));
  memcpy(h_poses, poses13, T * 13 * 4);
  memcpy(h_fof, frame_of_pose, T * 4);
  FL_HIP(ctx, hipMemcpyAsync(trk->d_poses, h_poses, T * 13 * 4, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(trk->d_frame_of, h_fof, T * 4, hipMemcpyHostToDevice, st));
  if (group_first) {
    memcpy(h_gf, group_first, ((size_t)n_groups + 1) * 4);
    FL_HIP(ctx, hipMemcpyAsync(trk->d_group_first, h_gf, ((size_t)n_groups + 1) * 4, hipMemcpyHostToDevice, st));
  }
  FL_HIP(ctx, hipMemsetAsync(trk->d_vacc, 0, T * sizeof(FlVerifyAcc), st));
  FL_HIP(ctx, hipEventRecord(trk->vev[1], st));
  // 2. the render, at the scene's K: a render pixel and the frame pixel under it are one ray
  const FlRenderMesh mesh = {trk->d_vtx, nullptr, nullptr, trk->d_tri, trk->n_t};
  const float headlight[3] = {0.f, 0.f, 1.f};
  for (int v0 = 0; v0 < n_poses; v0 += trk->chunk) {
    const int n = std::min(trk->chunk, n_poses - v0);
    if (int rc = fl_launch_render_chunk(ctx, mesh, trk->d_poses + (size_t)13 * v0, n, trk->w, trk->h, fx, fy, cx, cy, headlight, FL_RENDER_AMBIENT,
                                        trk->d_keys, nullptr, trk->d_render + (size_t)v0 * px, nullptr, nullptr))
      return rc;
  }
  FL_HIP(ctx, hipEventRecord(trk->vev[2], st));
  // 3. the counts
  VerifyArgs a;
  a.n_poses = n_poses;
  a.n_groups = group_first ? n_groups : 0;
  a.w = trk->w; a.h = trk->h;
  a.n_strips = (int)((px + V_STRIP_PX - 1) / V_STRIP_PX);
  a.tau = P.tau_mm;
  a.min_model_px = P.min_model_px;
  a.min_inlier_ratio = P.min_inlier_ratio;
  a.max_behind_ratio = P.max_behind_ratio;
  a.render = trk->d_render;
  a.frames = trk->d_frames;
  a.frame_stride = trk->frame_stride;
  a.frame_of = trk->d_frame_of;
  a.group_first = group_first ? trk->d_group_first : nullptr;
  a.acc = trk->d_vacc;
  a.out = trk->d_vres;
  hipLaunchKernelGGL(k_verify_score, dim3((unsigned)(n_poses * a.n_strips)), dim3(VB), 0, st, a);   // <= 2^16 * 2^13 workgroups
  FL_HIP(ctx, hipGetLastError());
  FL_HIP(ctx, hipEventRecord(trk->vev[3], st));
  // 4. ratios and accepted per pose, then the best of every group
  hipLaunchKernelGGL(k_verify_finish, dim3((n_poses + 63) / 64), dim3(64), 0, st, a);
  FL_HIP(ctx, hipGetLastError());
  if (group_first) {
    hipLaunchKernelGGL(k_verify_pick, dim3((n_groups + 63) / 64), dim3(64), 0, st, a);
    FL_HIP(ctx, hipGetLastError());
  }
  FL_HIP(ctx, hipEventRecord(trk->vev[4], st));
  // 5. one copy, one wait
  FL_HIP(ctx, hipMemcpyAsync(h_out, trk->d_vres, T * sizeof(fl_verify_result), hipMemcpyDeviceToHost, st));
  FL_HIP(ctx, hipStreamSynchronize(st));
  memcpy(results, h_out, T * sizeof(fl_verify_result));
  trk->verified = true;
  return FL_OK;
}
