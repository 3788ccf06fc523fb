// fl_track_internal.h -- what the tracker's entry points share (fl_track.hip: fl_track_batch and fl_track_batch_verified,
// fl_verify.hip: fl_verify_batch; fl_scene.hip: fl_verify_scene_batch; not part of the ABI): the tracker, the layout of its pinned block, and the
// steps of a call, which fl_track.hip defines.
#pragma once
#include "fl_internal.h"
#include <math.h>
#include <string.h>
#include <algorithm>

constexpr int FL_TRACK_EVENTS = 2 + 4 * FL_TRACK_MAX_PASSES;   // start, inputs on the device, then per pass render / rects / ICP / finish
constexpr int FL_VERIFY_EVENTS = 5;                            // start, inputs on the device, render, score, finish and pick
constexpr int FL_TRACK_VERIFIED_EVENTS = 3;                    // fl_track_batch_verified after its passes: accumulators clear, fused, finish and pick
constexpr int FL_SCENE_EVENTS = FL_VERIFY_EVENTS + 2;          // fl_verify_scene_batch: fl_verify_batch's, then overlap, then pick

// p = base + off (base null: a sizing pass, p is left alone); off moves on by bytes rounded up to 256
template <class T>
inline void fl_carve(T *&p, uint8_t *base, size_t &off, size_t bytes)
{
  if (base) p = (T *)(base + off);
  off += fl_align(bytes, 256);
}

// The pinned block a call's inputs leave through and its records come back through, and the one statement of its layout:
// max_tracks poses of 13 floats | frame indices | mesh indices | records (of fl_track_batch, fl_verify_batch or
// fl_track_batch_verified, the largest; fl_verify_scene_batch's 80-byte records fit) | max_tracks + 1 group or scene starts
struct FlTrackStage { float *poses; int32_t *frame_of, *mesh_of; uint8_t *results; int32_t *group_first; };
inline size_t fl_track_stage(FlTrackStage &s, uint8_t *base, int max_tracks)   // returns the bytes; base null: nothing else
{
  const size_t T = (size_t)max_tracks;
  size_t off = 0;
  fl_carve(s.poses, base, off, T * 13 * 4);
  fl_carve(s.frame_of, base, off, T * 4);
  fl_carve(s.mesh_of, base, off, T * 4);
  fl_carve(s.results, base, off, T * std::max({sizeof(fl_track_result), sizeof(fl_verify_result), sizeof(fl_verified_track_result)}));
  fl_carve(s.group_first, base, off, (T + 1) * 4);
  return off;
}

struct fl_tracker {
  fl_context *ctx = nullptr;
  bool owns_ctx = false;                        // fl_dev_tracker_create_host: a context without a device, released with the tracker
  int w = 0, h = 0, max_frames = 0, max_tracks = 0, max_crop_px = 0;
  int n_meshes = 1, n_t = 0, max_n_t = 0;       // n_t: of mesh 0, which starts both arrays; max_n_t: of the largest mesh
  int chunk = 0;                                // views per render launch
  uint8_t *d_mem = nullptr;                     // the one device allocation (carve_device, fl_track.hip)
  const float *d_vtx = nullptr;
  const int32_t *d_tri = nullptr;               // every mesh's vertices and triangles back to back, indices rebased
  FlMeshRange *d_ranges = nullptr;              // n_meshes entries
  int32_t *d_mesh_of = nullptr;                 // max_tracks entries: the mesh of every pose of a call that names meshes
  const FlMeshRange *call_ranges = nullptr;     // of the call being queued (fl_tracker_stage): d_ranges and d_mesh_of when it
  const int32_t *call_mesh_of = nullptr;        // named meshes on a tracker that has several, else null: mesh 0 for every pose
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
  uint8_t *d_vacc = nullptr;                    // 2 * max_tracks FlVerifyAcc: a pose's, and with fl_track_batch_verified its input pose's
  fl_verify_result *d_vres = nullptr;
  fl_verified_track_result *d_vout = nullptr;   // max_tracks records of fl_track_batch_verified
  int32_t *d_group_first = nullptr;             // max_tracks + 1 entries
  uint8_t *h_stage = nullptr;                   // the one pinned allocation
  FlTrackStage stage = {};                      // its parts
  hipEvent_t ev[FL_TRACK_EVENTS + FL_VERIFY_EVENTS + FL_TRACK_VERIFIED_EVENTS] = {nullptr};   // fl_track_batch's, fl_verify_batch's, the verified stages'
  int last_passes = 0;                          // of the last fl_track_batch or fl_track_batch_verified; 0: none yet
  bool verified = false;                        // an fl_verify_batch has completed
  bool track_verified = false;                  // the last call that ran passes was an fl_track_batch_verified
  // fl_verify_scene_batch (fl_scene.hip): its events, made by its first call, and where its last call left the compact shared
  // array in the context's scratch block (scene_scratch: the block it was carved from, to tell a block that has moved since)
  hipEvent_t ev_scene[FL_SCENE_EVENTS] = {nullptr};
  const int32_t *scene_shared = nullptr;
  const void *scene_scratch = nullptr;
  int scene_pairs = -1;                         // -1: no fl_verify_scene_batch has completed
};

// The steps of a call, in the order an entry point takes them.
// 1. The checks both entry points make, `who` in the text: null pointers (`results` is only tested for null), mem, n_frames and n
// against the tracker's limits, a null frame, frame_of outside [0, n_frames), mesh_of (null: every pose is mesh 0) outside
// [0, n_meshes), a non-finite pose (floats 0..11), K's size against
// the tracker's, fx, fy finite and > 0 and cx, cy finite AS DOUBLES.  fl_verify_batch then asks the same of them as floats, which
// is what it hands the rasteriser; fl_track_batch renders at the model camera and reads K in fp64: that one difference is meant.
// FL_ERR_INVALID or FL_OK, no HIP call.  The entry point's own checks follow, and the device check (FL_ERR_NO_DEVICE) after all.
int fl_tracker_check_call(fl_tracker *trk, const char *who, int n_frames, const uint16_t *const *depth, int mem, int n, const int32_t *frame_of,
                          const int32_t *mesh_of, const float *poses13, const fl_intrinsics *K, const void *results);
// 1b. What fl_verify_batch and fl_track_batch_verified ask on top of that: K as floats, which is what the rasteriser gets (fx, fy
// finite and > 0, cx, cy finite), and with group_first its rules against n poses.  FL_ERR_INVALID or FL_OK, no HIP call.
int fl_verify_check_call(fl_tracker *trk, const char *who, const fl_intrinsics *K, int n, int n_groups, const int32_t *group_first);
// 2. hipSetDevice, the context's streams joined, ev_start, the frames into their slots, then poses13 and frame_of through the
// pinned block into d_poses and d_frame_of, and on a tracker of several meshes mesh_of (unless null) into d_mesh_of the same way.
// poses_keep (null: none): a second device array the poses pass through on their way to d_poses and stay in.
int fl_tracker_stage(fl_tracker *trk, hipEvent_t ev_start, int n_frames, const uint16_t *const *depth, int mem, int n, const int32_t *frame_of,
                     const int32_t *mesh_of, const float *poses13, float *poses_keep);
// 3. every pose's mesh at the first n poses of d_poses, depth only, into d_render, a chunk of views per launch
int fl_tracker_render(fl_tracker *trk, int n, float fx, float fy, float cx, float cy);
// 4. bytes of records from d_records to the caller through the pinned block: one copy, one wait for the stream
int fl_tracker_results(fl_tracker *trk, const void *d_records, size_t bytes, void *results);
// fl_verify_batch_meshes behind its checks (fl_verify.hip), queued and not waited for: step 2 (ev[0] at its start), `starts`
// (group_first, or fl_verify_scene_batch's scene_first; n_starts + 1 entries, null: none) through the pinned block into
// d_group_first, clear accumulators (ev[1]), the render at the scene camera unless fused (ev[2]), the counts (ev[3]), the
// records, and with pick the best of every group of `starts` (ev[4]); without pick best = accepted.  Afterwards d_vres holds
// the n_poses records and, unless fused, d_render their renders.  ev: five events.
int fl_verify_queue(fl_tracker *trk, hipEvent_t *ev, int n_frames, const uint16_t *const *depth, int mem, int n_poses, const int32_t *frame_of_pose,
                    const int32_t *mesh_of_pose, const float *poses13, int n_starts, const int32_t *starts, bool pick, bool fused,
                    const fl_intrinsics *K, const fl_verify_params &P);

// a pixel index into the bounding box of a w-wide image (k_track_rects, k_verify_score)
__device__ __forceinline__ void bbox_add(int idx, int w, int &x0, int &x1, int &y0, int &y1)
{
  const int y = idx / w, x = idx - y * w;
  x0 = min(x0, x); x1 = max(x1, x);
  y0 = min(y0, y); y1 = max(y1, y);
}

// A pose's verification accumulators, zeroed before the launch.  box = {w - x0, h - y0, x1 + 1, y1 + 1}: zero means "no pixel"
// and every entry grows, so one atomicMax serves the four sides.
struct FlVerifyAcc {
  int32_t n[5];                                 // model, missing, inlier, front, behind
  int32_t box[4];
  int32_t pad;
  unsigned long long sum;                       // of |d| over the inliers
};
static_assert(sizeof(FlVerifyAcc) == FL_VERIFY_ACC_BYTES, "what fl_tracker_create and the detector's scratch allocate per pose");

// The finish of fl_verify_batch on one accumulator: rect, counts, ratios, accepted; best is left 0 (k_verify_finish,
// k_track_verified_finish)
__device__ __forceinline__ fl_verify_result fl_verify_record(const FlVerifyAcc &c, int w, int h, int min_model_px, float min_inlier_ratio,
                                                             float max_behind_ratio)
{
  fl_verify_result o;
  memset(&o, 0, sizeof(o));                     // status = FL_OK; an empty render leaves every other field zero too
  if (c.n[0] > 0) {
    const int x0 = w - c.box[0], y0 = h - c.box[1];
    o.rect[0] = x0; o.rect[1] = y0; o.rect[2] = c.box[2] - x0; o.rect[3] = c.box[3] - y0;
    o.n_model = c.n[0]; o.n_missing = c.n[1]; o.n_inlier = c.n[2]; o.n_front = c.n[3]; o.n_behind = c.n[4];
    o.sum_abs_inlier = (int64_t)c.sum;
    o.inlier_ratio = (float)c.n[2] / (float)c.n[0];
    o.behind_ratio = (float)c.n[4] / (float)c.n[0];
    o.accepted = c.n[0] >= min_model_px && (min_inlier_ratio <= 0.f || o.inlier_ratio >= min_inlier_ratio) &&
                 (max_behind_ratio <= 0.f || o.behind_ratio <= max_behind_ratio);
  }
  return o;
}
