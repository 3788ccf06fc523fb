// fl_scene.hip -- scene arbitration (fl_verify_scene_batch and fl_scene_pick, include/fealess_hip.h): every pose verified as
// fl_verify_batch_meshes verifies it, then of every two accepted poses of one scene the number of frame pixels that support both,
// and an exact greedy suppression on those counts.  The third user of the call steps of fl_track_internal.h.  No counterpart in
// the reference.
//
// One call, all on the context's stream, one wait at the end:
//   fl_verify_queue    (fl_verify.hip) stage, render at the scene camera, k_verify_score, k_verify_finish: the records in d_vres,
//                      the renders in d_render.  Never the fused kernel: the renders are read again below.
//   k_scene_overlap    one workgroup of 256 threads per pair of the compact list.  It finds its scene by a search over pair_first
//                      that every thread makes alike, stores 0 at once unless both records are accepted, both have inliers and
//                      their rects intersect, and otherwise walks the intersection of the two rects row by row: SO_LOADS pixels
//                      of both renders in flight per thread, then the frame under them where both renders have a pixel, counts
//                      in registers, the wave, LDS, one plain store.  No atomics, nothing depends on the schedule.  An
//                      intersection starts at any x, so the loads are single pixels.  The loads of a round are issued together:
//                      with a condition on each load the compiler waits after every one, and the stage took 0.082 ms where it
//                      now takes 0.029.
//   k_scene_pick       one wave per scene, lane = pose: a lane's rank = the number of accepted lanes that stand before it
//                      (scene_before), then lane 0 walks the ranks (scene_walk) over the scene's part of the shared array in LDS,
//                      then every lane writes its record.
// scene_before and scene_walk are host and device code: fl_scene_pick is the same rule on the caller's records.
// pair_first, the shared array and the records live in the context's scratch block, pair_first leaves through its pinned block.
#include "fl_track_internal.h"

namespace {

constexpr int SO = 256;                         // k_scene_overlap: threads per workgroup
constexpr int SO_LOADS = 8;                     // pixels in flight per thread: single u16 loads, so twice k_verify_score's count
constexpr int SP = FL_SCENE_MAX_POSES;          // k_scene_pick: one wave
constexpr int SP_PAIRS = SP * (SP - 1) / 2;
static_assert(SP == FL_WAVE, "k_scene_pick: lane = pose");

// a stands before b in its scene's order (both accepted; a, b: their indices)
__host__ __device__ inline bool scene_before(int ni_a, int nm_a, int a, int ni_b, int nm_b, int b)
{
  if (ni_a != ni_b) return ni_a > ni_b;
  const long long l = (long long)ni_a * nm_b, r = (long long)ni_b * nm_a;
  if (l != r) return l > r;
  return a < b;
}

// The suppression over one scene.  by_rank[r], r < n_acc: the local index of the accepted pose of rank r; n_inlier[i]: of local
// pose i; tri: the scene's part of the compact shared array (local i < j at j (j - 1) / 2 + i); first: the scene's first pose.
// Writes kept, rival and n_shared of the accepted poses, by local index.
template <class Idx>
__host__ __device__ inline void scene_walk(int n_acc, const Idx *by_rank, const int32_t *n_inlier, const int32_t *tri, float max_shared_ratio,
                                           int min_shared_px, int first, int32_t *kept, int32_t *rival, int32_t *n_shared)
{
  for (int r = 0; r < n_acc; ++r) {
    const int b = (int)by_rank[r];
    int rv = -1, ns = 0, keep = 1;
    for (int q = 0; q < r; ++q) {
      const int a = (int)by_rank[q];
      if (!kept[a]) continue;
      const int i = a < b ? a : b, j = a < b ? b : a, n = tri[j * (j - 1) / 2 + i];
      if (n >= min_shared_px && (float)n / (float)n_inlier[b] >= max_shared_ratio) { keep = 0; rv = a; ns = n; break; }
      if (n > ns) { rv = a; ns = n; }
    }
    kept[b] = keep;
    rival[b] = rv < 0 ? -1 : first + rv;
    n_shared[b] = ns;
  }
}

struct SceneArgs {
  int n_scenes, n_pairs, w, h, tau;
  float max_shared_ratio;
  int min_shared_px;
  const uint16_t *render;                       // the call's renders, w * h each, back to back
  const uint8_t *frames;                        // the frame slots
  size_t frame_stride;
  const int32_t *frame_of, *scene_first, *pair_first;   // scene_first, pair_first: n_scenes + 1 entries
  const fl_verify_result *rec;                  // the finished records
  int32_t *shared;                              // n_pairs entries
  fl_scene_result *out;
};

__global__ __launch_bounds__(SO) void k_scene_overlap(SceneArgs a)
{
  __shared__ int red[SO / FL_WAVE];
  const int p = blockIdx.x, tid = threadIdx.x;
  // the scene: the last s with pair_first[s] <= p (a scene without pairs shares its entry with the next one)
  int lo = 0, hi = a.n_scenes;                  // pair_first[lo] <= p < pair_first[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.pair_first[mid] <= p) lo = mid; else hi = mid;
  }
  const int q = p - a.pair_first[lo];           // j (j - 1) / 2 + i, i < j < FL_SCENE_MAX_POSES
  int j = (int)((1.f + sqrtf(1.f + 8.f * (float)q)) * 0.5f);
  while (j * (j - 1) / 2 > q) --j;
  while ((j + 1) * j / 2 <= q) ++j;
  const int i = q - j * (j - 1) / 2, first = a.scene_first[lo], pa = first + i, pb = first + j;
  const fl_verify_result &ra = a.rec[pa], &rb = a.rec[pb];
  const int x0 = max(max(ra.rect[0], rb.rect[0]), 0), x1 = min(min(ra.rect[0] + ra.rect[2], rb.rect[0] + rb.rect[2]), a.w);
  const int y0 = max(max(ra.rect[1], rb.rect[1]), 0), y1 = min(min(ra.rect[1] + ra.rect[3], rb.rect[1] + rb.rect[3]), a.h);
  if (!(ra.accepted && rb.accepted && ra.n_inlier > 0 && rb.n_inlier > 0 && x1 > x0 && y1 > y0)) {   // uniform per workgroup
    if (tid == 0) a.shared[p] = 0;
    return;
  }
  const size_t px = (size_t)a.w * a.h;
  const uint16_t *ia = a.render + px * pa, *ib = a.render + px * pb;
  const uint16_t *scn = (const uint16_t *)(a.frames + a.frame_stride * (size_t)a.frame_of[pa]);   // one frame per scene
  const int iw = x1 - x0, n = iw * (y1 - y0), first_px = y0 * a.w + x0;   // n <= FL_RENDER_MAX_DIM^2
  // pixel k of the intersection, row-major, is (k % iw, k / iw); a thread takes k = tid, tid + SO, ... and keeps (x, y), which a
  // step of SO pixels moves on by sr columns and sq rows
  const int sq = SO / iw, sr = SO - sq * iw;
  int y = tid / iw, x = tid - y * iw, count = 0;
#pragma unroll 1
  for (int k0 = tid; k0 < n; k0 += SO * SO_LOADS) {
    // A load under a condition of its own is a branch with a wait behind it, and the loads of a round would go one after
    // another: a pixel past the end reads the intersection's first pixel instead and counts as empty, and a thread reads the
    // frame under all of its pixels of the round when both renders are non-zero at one of them.
    int idx[SO_LOADS], va[SO_LOADS], vb[SO_LOADS], vs[SO_LOADS];
    bool in[SO_LOADS], both = false;
#pragma unroll
    for (int u = 0; u < SO_LOADS; ++u) {
      in[u] = k0 + u * SO < n;
      idx[u] = in[u] ? (y0 + y) * a.w + x0 + x : first_px;
      x += sr; y += sq;
      if (x >= iw) { x -= iw; ++y; }
    }
#pragma unroll
    for (int u = 0; u < SO_LOADS; ++u) {
      va[u] = (int)ia[idx[u]];
      vb[u] = (int)ib[idx[u]];
    }
#pragma unroll
    for (int u = 0; u < SO_LOADS; ++u) {
      va[u] = in[u] ? va[u] : 0;
      both = both || (va[u] && vb[u]);
      vs[u] = 0;
    }
    if (both) {                                 // the frame only where both renders have a pixel
#pragma unroll
      for (int u = 0; u < SO_LOADS; ++u) vs[u] = (int)scn[idx[u]];
    }
#pragma unroll
    for (int u = 0; u < SO_LOADS; ++u) {
      const int da = vs[u] - va[u], db = vs[u] - vb[u];
      count += va[u] && vb[u] && vs[u] && (da < 0 ? -da : da) <= a.tau && (db < 0 ? -db : db) <= a.tau;
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) count += __shfl_xor(count, s, FL_WAVE);
  if ((tid & (FL_WAVE - 1)) == 0) red[tid / FL_WAVE] = count;
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int wv = 1; wv < SO / FL_WAVE; ++wv) count += red[wv];
  a.shared[p] = count;
}

__global__ __launch_bounds__(SP) void k_scene_pick(SceneArgs a)
{
  __shared__ int32_t tri[SP_PAIRS];
  __shared__ int32_t s_ni[SP], s_nm[SP], s_acc[SP], kept[SP], rival[SP], n_shared[SP];
  __shared__ uint8_t by_rank[SP];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int first = a.scene_first[s], m = a.scene_first[s + 1] - first;   // m <= FL_SCENE_MAX_POSES
  if (m == 0) return;
  fl_verify_result r;
  memset(&r, 0, sizeof(r));
  if (lane < m) r = a.rec[first + lane];
  s_ni[lane] = r.n_inlier; s_nm[lane] = r.n_model; s_acc[lane] = lane < m && r.accepted;
  kept[lane] = 0; rival[lane] = -1; n_shared[lane] = 0;
  const int32_t *src = a.shared + a.pair_first[s];
  for (int k = lane; k < m * (m - 1) / 2; k += SP) tri[k] = src[k];
  __syncthreads();
  int rank = -1;
  if (s_acc[lane]) {
    rank = 0;
    for (int k = 0; k < m; ++k)
      rank += k != lane && s_acc[k] && scene_before(s_ni[k], s_nm[k], k, r.n_inlier, r.n_model, lane);
    by_rank[rank] = (uint8_t)lane;
  }
  __syncthreads();
  if (lane == 0) {
    int n_acc = 0;
    for (int k = 0; k < m; ++k) n_acc += s_acc[k];
    scene_walk(n_acc, by_rank, s_ni, tri, a.max_shared_ratio, a.min_shared_px, first, kept, rival, n_shared);
  }
  __syncthreads();
  if (lane >= m) return;
  fl_scene_result o;
  o.verify = r;
  o.kept = kept[lane]; o.order = rank; o.rival = rival[lane]; o.n_shared = n_shared[lane];
  a.out[first + lane] = o;
}
}  // namespace

static_assert(sizeof(fl_scene_result) == 80, "fl_scene_result is 80 bytes (include/fealess_hip.h)");
static_assert(sizeof(fl_scene_params) == 24, "fl_scene_params is 24 bytes (include/fealess_hip.h)");
static_assert(sizeof(fl_scene_result) <= sizeof(fl_verified_track_result), "the records leave through FlTrackStage::results");
static const fl_scene_params k_scene_defaults = {{10, 1, 0.f, 0.f}, 0.5f, 1};

// what both entry points ask of scene_first and of the two fields fl_scene_params adds; n_pairs: the length of the compact list
static int scene_check(fl_context *ctx, const char *who, int n_poses, int n_scenes, int max_scenes, const int32_t *scene_first, const fl_scene_params &P,
                       long long *n_pairs)
{
  if (!scene_first) return fl_set_error(ctx, FL_ERR_INVALID, "%s: null scene_first", who);
  bool ok = n_scenes >= 1 && n_scenes <= max_scenes && scene_first[0] == 0;
  long long pairs = 0;
  for (int s = 0; ok && s < n_scenes; ++s) {
    const long long m = (long long)scene_first[s + 1] - scene_first[s];
    ok = m >= 0 && m <= FL_SCENE_MAX_POSES && scene_first[s + 1] <= n_poses;
    pairs += m * (m - 1) / 2;
  }
  if (!ok || scene_first[n_scenes] != n_poses)
    return fl_set_error(ctx, FL_ERR_INVALID, "%s: scene_first must have n_scenes + 1 (n_scenes 1..%d) non-decreasing entries from 0 to the number of poses, "
                        "at most %d poses apart", who, max_scenes, FL_SCENE_MAX_POSES);
  if (!(std::isfinite(P.max_shared_ratio) && P.max_shared_ratio > 0.f && P.max_shared_ratio <= 1.f) || P.min_shared_px < 1)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_scene_params: max_shared_ratio finite and in (0, 1], min_shared_px >= 1");
  *n_pairs = pairs;
  return FL_OK;
}

extern "C" int fl_scene_pick(const fl_verify_result *records, int n_poses, int n_scenes, const int32_t *scene_first, const int32_t *shared,
                             const fl_scene_params *params, fl_scene_result *results)
{
  if (!records || !results || n_poses < 0) return FL_ERR_INVALID;
  const fl_scene_params P = params ? *params : k_scene_defaults;
  long long n_pairs = 0;
  if (int rc = scene_check(nullptr, "fl_scene_pick", n_poses, n_scenes, INT32_MAX, scene_first, P, &n_pairs)) return rc;
  if (!fl_verify_params_ok(P.verify) || (n_pairs > 0 && !shared)) return FL_ERR_INVALID;
  const int32_t *tri = shared;
  for (int s = 0; s < n_scenes; ++s) {          // a count two accepted poses cannot share
    const int first = scene_first[s], m = scene_first[s + 1] - first;
    for (int j = 1; j < m; ++j)
      for (int i = 0; i < j; ++i) {
        const fl_verify_result &a = records[first + i], &b = records[first + j];
        if (a.accepted && b.accepted && (tri[j * (j - 1) / 2 + i] < 0 || tri[j * (j - 1) / 2 + i] > std::min(a.n_inlier, b.n_inlier))) return FL_ERR_INVALID;
      }
    tri += m * (m - 1) / 2;
  }
  tri = shared;
  for (int s = 0; s < n_scenes; ++s) {
    const int first = scene_first[s], m = scene_first[s + 1] - first;
    int32_t ni[SP], kept[SP], rival[SP], n_shared[SP], rank[SP], by_rank[SP], n_acc = 0;
    for (int i = 0; i < m; ++i) {
      const fl_verify_result &r = records[first + i];
      ni[i] = r.n_inlier; kept[i] = 0; rival[i] = -1; n_shared[i] = 0; rank[i] = -1;
      if (!r.accepted) continue;
      rank[i] = 0;
      for (int k = 0; k < m; ++k) {
        const fl_verify_result &o = records[first + k];
        rank[i] += k != i && o.accepted && scene_before(o.n_inlier, o.n_model, k, r.n_inlier, r.n_model, i);
      }
      by_rank[rank[i]] = i;
      ++n_acc;
    }
    scene_walk(n_acc, by_rank, ni, tri, P.max_shared_ratio, P.min_shared_px, first, kept, rival, n_shared);
    for (int i = 0; i < m; ++i) {
      fl_scene_result o;
      o.verify = records[first + i];
      o.kept = kept[i]; o.order = rank[i]; o.rival = rival[i]; o.n_shared = n_shared[i];
      results[first + i] = o;
    }
    tri += m * (m - 1) / 2;
  }
  return FL_OK;
}

extern "C" int fl_verify_scene_batch(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_poses, const int32_t *frame_of_pose,
                                     const int32_t *mesh_of_pose, const float *poses13, int n_scenes, const int32_t *scene_first,
                                     const fl_intrinsics *K, const fl_scene_params *params, fl_scene_result *results)
{
  const char *who = "fl_verify_scene_batch";
  int rc = fl_tracker_check_call(trk, who, n_frames, depth, mem, n_poses, frame_of_pose, mesh_of_pose, poses13, K, results);
  if (rc || (rc = fl_verify_check_call(trk, who, K, n_poses, 0, nullptr))) return rc;
  fl_context *ctx = trk->ctx;
  const fl_scene_params P = params ? *params : k_scene_defaults;
  long long n_pairs = 0;
  if ((rc = scene_check(ctx, who, n_poses, n_scenes, trk->max_tracks, scene_first, P, &n_pairs))) return rc;
  for (int s = 0; s < n_scenes; ++s)
    for (int t = scene_first[s] + 1; t < scene_first[s + 1]; ++t)
      if (frame_of_pose[t] != frame_of_pose[scene_first[s]])
        return fl_set_error(ctx, FL_ERR_INVALID, "%s: pose %d of scene %d names frame %d, the scene's first pose frame %d", who, t, s, frame_of_pose[t],
                            frame_of_pose[scene_first[s]]);
  if (!fl_verify_params_ok(P.verify)) return fl_set_error(ctx, FL_ERR_INVALID, FL_VERIFY_PARAMS_TEXT);
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "%s: the tracker has no device", who);

  FL_HIP(ctx, hipSetDevice(ctx->device));
  for (hipEvent_t &e : trk->ev_scene)
    if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; return fl_set_error(ctx, FL_ERR_HIP, "%s: hipEventCreate", who); }
  // scratch: pair_first | shared | records; pinned: pair_first.  Both blocks persist on the context.
  const size_t S = (size_t)n_scenes + 1, o_shared = fl_align(S * 4, 256), o_out = o_shared + fl_align((size_t)n_pairs * 4, 256);
  void *sv = nullptr, *hv = nullptr;
  if ((rc = fl_scratch(ctx, o_out + (size_t)n_poses * sizeof(fl_scene_result), &sv)) || (rc = fl_pinned(ctx, S * 4, &hv))) return rc;
  uint8_t *s = (uint8_t *)sv;
  int32_t *h_pair_first = (int32_t *)hv, *d_pair_first = (int32_t *)s, *d_shared = (int32_t *)(s + o_shared);
  fl_scene_result *d_out = (fl_scene_result *)(s + o_out);
  h_pair_first[0] = 0;
  for (int k = 0; k < n_scenes; ++k) {
    const int m = scene_first[k + 1] - scene_first[k];
    h_pair_first[k + 1] = h_pair_first[k] + m * (m - 1) / 2;     // <= 31.5 * FL_TRACK_MAX_TRACKS
  }
  trk->scene_pairs = -1;
  // 1. to 4. every pose verified, its own group; scene_first travels where group_first travels
  hipEvent_t *ev = trk->ev_scene;
  hipStream_t st = ctx->stream;
  if ((rc = fl_verify_queue(trk, ev, n_frames, depth, mem, n_poses, frame_of_pose, mesh_of_pose, poses13, n_scenes, scene_first, false, false, K, P.verify)))
    return rc;
  FL_HIP(ctx, hipMemcpyAsync(d_pair_first, h_pair_first, S * 4, hipMemcpyHostToDevice, st));
  // 5. the shared counts
  const SceneArgs a = {n_scenes, (int)n_pairs, trk->w, trk->h, P.verify.tau_mm, P.max_shared_ratio, P.min_shared_px, trk->d_render, trk->d_frames,
                       trk->frame_stride, trk->d_frame_of, trk->d_group_first, d_pair_first, trk->d_vres, d_shared, d_out};   // in SceneArgs' order
  if (n_pairs > 0) {
    hipLaunchKernelGGL(k_scene_overlap, dim3((unsigned)n_pairs), dim3(SO), 0, st, a);
    FL_HIP(ctx, hipGetLastError());
  }
  FL_HIP(ctx, hipEventRecord(ev[FL_VERIFY_EVENTS], st));
  // 6. order and suppression per scene
  hipLaunchKernelGGL(k_scene_pick, dim3((unsigned)n_scenes), dim3(SP), 0, st, a);
  FL_HIP(ctx, hipGetLastError());
  FL_HIP(ctx, hipEventRecord(ev[FL_VERIFY_EVENTS + 1], st));
  // 7. one copy, one wait
  if ((rc = fl_tracker_results(trk, d_out, (size_t)n_poses * sizeof(fl_scene_result), results))) return rc;
  trk->scene_shared = d_shared;
  trk->scene_scratch = sv;
  trk->scene_pairs = (int)n_pairs;
  return FL_OK;
}

// Development / test aids, exported but not part of the ABI.
// The compact shared array of the last fl_verify_scene_batch: *n_pairs entries into out (host, room for cap).  FL_ERR_STATE when no
// such call has completed or the context's scratch block has been replaced since; FL_ERR_OVERFLOW when cap is too small.
extern "C" int fl_dev_tracker_scene_shared(fl_tracker *trk, int32_t *out, int cap, int *n_pairs)
{
  if (!trk || !n_pairs || (!out && cap > 0) || cap < 0) return FL_ERR_INVALID;
  fl_context *ctx = trk->ctx;
  if (trk->scene_pairs < 0 || trk->scene_scratch != ctx->scratch) return fl_set_error(ctx, FL_ERR_STATE, "fl_dev_tracker_scene_shared: no shared array to read");
  *n_pairs = trk->scene_pairs;
  if (trk->scene_pairs > cap) return fl_set_error(ctx, FL_ERR_OVERFLOW, "fl_dev_tracker_scene_shared: %d pairs, room for %d", trk->scene_pairs, cap);
  if (trk->scene_pairs == 0) return FL_OK;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  FL_HIP(ctx, hipMemcpyAsync(out, trk->scene_shared, (size_t)trk->scene_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

// device time of the last fl_verify_scene_batch by stage: {copy, render, score, finish, overlap, pick} in ms
extern "C" int fl_dev_tracker_scene_ms(fl_tracker *trk, float out[6])
{
  if (!trk || !out || trk->scene_pairs < 0) return FL_ERR_INVALID;
  for (int k = 0; k < FL_SCENE_EVENTS - 1; ++k)
    if (hipEventElapsedTime(out + k, trk->ev_scene[k], trk->ev_scene[k + 1]) != hipSuccess) return FL_ERR_HIP;
  return FL_OK;
}
