// fl_verify.hip -- hypothesis verification (fl_verify_batch, include/fealess_hip.h): the mesh rendered at every pose with the
// SCENE camera and laid over the pose's depth frame, on a tracker's mesh, frame slots and render images.  The second user of the
// call steps of fl_track_internal.h (fl_track.hip defines them; fl_track_batch is the first).  No counterpart in the reference.
//
// One call, all on the context's stream, between fl_tracker_stage and fl_tracker_results: fl_tracker_render at the scene's K (a
// render pixel and the frame pixel under it are one ray), then
//   k_verify_score   one workgroup per (pose, strip of V_STRIP_PX pixels): the contract's per-pixel rule, reduced in the wave and
//                    in the workgroup, then one integer atomic per counter into the pose's FlVerifyAcc -- exact whatever the order
//   k_verify_finish  one thread per pose: rect, ratios, accepted; best = accepted when there are no groups
//   k_verify_pick    one thread per group: the best accepted member
// The strip: k_track_rects walks a whole 640 x 480 render with one workgroup and is bound by the latency of its 19 rounds of
// loads.  Here a thread issues its V_LOADS 16-byte render loads at once and never loops, so a workgroup lasts about two memory
// round trips (render, then the scene under the non-zero groups) and a strip is VB * V_LOADS * 8 = 8192 pixels, 16 KB of
// render: 38 workgroups = 152 waves per 640 x 480 pose.  A shorter strip would only add workgroups whose reduction and
// atomics outweigh their one load per thread; a longer one brings the loop and its serial round trips back.  Measured:
// DESIGN.md section 0, row f6.
#include "fl_track_internal.h"

namespace {

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
}  // namespace

static_assert(sizeof(FlVerifyAcc) == FL_VERIFY_ACC_BYTES, "what fl_tracker_create allocates per pose");
static_assert(sizeof(fl_verify_result) == 64, "fl_verify_result is 64 bytes (include/fealess_hip.h)");
static const fl_verify_params k_verify_defaults = {10, 1, 0.f, 0.f};

// device time of the last fl_verify_batch by stage: {copy, render, score, finish and pick} in ms
extern "C" int fl_dev_tracker_verify_ms(fl_tracker *trk, float out[4])
{
  if (!trk || !out || !trk->verified) return FL_ERR_INVALID;
  const hipEvent_t *ev = trk->ev + FL_TRACK_EVENTS;
  for (int k = 0; k < 4; ++k)
    if (hipEventElapsedTime(out + k, ev[k], ev[k + 1]) != hipSuccess) return FL_ERR_HIP;
  return FL_OK;
}

extern "C" int fl_verify_batch(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_poses,
                               const int32_t *frame_of_pose, const float *poses13, int n_groups, const int32_t *group_first,
                               const fl_intrinsics *K, const fl_verify_params *params, fl_verify_result *results)
{
  int rc = fl_tracker_check_call(trk, "fl_verify_batch", n_frames, depth, mem, n_poses, frame_of_pose, poses13, K, results);
  if (rc) return rc;
  fl_context *ctx = trk->ctx;
  // K as floats, which is what the rasteriser gets: 1e-60 is a positive double and a zero float, 1e300 an infinite one
  const float fx = (float)K->fx, fy = (float)K->fy, cx = (float)K->cx, cy = (float)K->cy;
  if (!(std::isfinite(fx) && fx > 0.f && std::isfinite(fy) && fy > 0.f && std::isfinite(cx) && std::isfinite(cy)))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_batch: fx, fy must be finite and > 0, cx, cy finite, as floats too");
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

  // 1. the inputs, and the groups after them
  hipEvent_t *ev = trk->ev + FL_TRACK_EVENTS;
  if ((rc = fl_tracker_stage(trk, ev[0], n_frames, depth, mem, n_poses, frame_of_pose, poses13, nullptr))) return rc;
  const size_t px = (size_t)trk->w * trk->h, T = (size_t)n_poses;
  hipStream_t st = ctx->stream;
  if (group_first) {
    memcpy(trk->stage.group_first, group_first, ((size_t)n_groups + 1) * 4);
    FL_HIP(ctx, hipMemcpyAsync(trk->d_group_first, trk->stage.group_first, ((size_t)n_groups + 1) * 4, hipMemcpyHostToDevice, st));
  }
  FL_HIP(ctx, hipMemsetAsync(trk->d_vacc, 0, T * sizeof(FlVerifyAcc), st));
  FL_HIP(ctx, hipEventRecord(ev[1], st));
  // 2. the render, at the scene's K
  if ((rc = fl_tracker_render(trk, n_poses, fx, fy, cx, cy))) return rc;
  FL_HIP(ctx, hipEventRecord(ev[2], st));
  // 3. the counts
  VerifyArgs a = {n_poses, group_first ? n_groups : 0, trk->w, trk->h, (int)((px + V_STRIP_PX - 1) / V_STRIP_PX), P.tau_mm, P.min_model_px,
                  P.min_inlier_ratio, P.max_behind_ratio, trk->d_render, trk->d_frames, trk->frame_stride, trk->d_frame_of,
                  group_first ? trk->d_group_first : nullptr, (FlVerifyAcc *)trk->d_vacc, trk->d_vres};               // in VerifyArgs' order
  hipLaunchKernelGGL(k_verify_score, dim3((unsigned)(n_poses * a.n_strips)), dim3(VB), 0, st, a);   // <= 2^16 * 2^13 workgroups
  FL_HIP(ctx, hipGetLastError());
  FL_HIP(ctx, hipEventRecord(ev[3], st));
  // 4. ratios and accepted per pose, then the best of every group
  hipLaunchKernelGGL(k_verify_finish, dim3((n_poses + 63) / 64), dim3(64), 0, st, a);
  FL_HIP(ctx, hipGetLastError());
  if (group_first) {
    hipLaunchKernelGGL(k_verify_pick, dim3((n_groups + 63) / 64), dim3(64), 0, st, a);
    FL_HIP(ctx, hipGetLastError());
  }
  FL_HIP(ctx, hipEventRecord(ev[4], st));
  // 5. one copy, one wait
  if ((rc = fl_tracker_results(trk, trk->d_vres, T * sizeof(fl_verify_result), results))) return rc;
  trk->verified = true;
  return FL_OK;
}
