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
// fl_verify_queue is all of that behind the argument checks, queued and not waited for; fl_verify_scene_batch (fl_scene.hip) calls
// it too and goes on with the records and the renders on the device.
// The strip: k_track_rects walks a whole 640 x 480 render with one workgroup and is bound by the latency of its 19 rounds of
// loads.  Here a thread issues its V_LOADS 16-byte render loads at once and never loops, so a workgroup lasts about two memory
// round trips (render, then the scene under the non-zero groups) and a strip is VB * V_LOADS * 8 = 8192 pixels, 16 KB of
// render: 38 workgroups = 152 waves per 640 x 480 pose.  A shorter strip would only add workgroups whose reduction and
// atomics outweigh their one load per thread; a longer one brings the loop and its serial round trips back.  Measured:
// DESIGN.md section 0, row f6.
// With the context's verify_fused option, k_verify_fused (below) takes the place of the render and k_verify_score: it fills the
// same accumulators from a render that stays in LDS.  fl_recognize_batch_instances_verified (fl_pipeline.hip) runs it on the
// refined poses of a batch where they lie, through fl_launch_verify_fused, and finishes them through fl_launch_verify_finish.
// fl_track_batch_verified (fl_track.hip) runs the same body as k_verify_fused_tracks, through the same launcher: the poses its
// passes left on the device and, in the same launch, the poses it came in with, a lost track's workgroups exiting at once.
#include "fl_track_internal.h"
#include "fl_raster.h"

namespace {

constexpr int VB = 256;                         // k_verify_score: threads per workgroup
constexpr int V_LOADS = 4;                      // loads in flight per thread
constexpr int V_STRIP_PX = VB * V_LOADS * 8;    // pixels per strip, on both paths

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

// ---- k_verify_fused: render and score in one workgroup, the render never leaves LDS ---------------------------------------
// A refined pose covers a few per cent of its frame, and verification needs the depth under those pixels only.  One workgroup
// per pose: the WINDOW is the union of k_raster's bounding boxes over the triangles it would not reject; the window is walked in
// BANDS of at most `budget` pixels (whole window rows, or pieces of one row where a row is longer than the budget); a band's
// z-buffer is 32-bit words in LDS, atomicMin on the bits of z (z > 0 orders like its bits, and the u16 conversion is monotone,
// so the nearest z gives the depth image's value whatever triangle it came from); then every thread walks band pixels through
// verify_px, counts in registers across bands.  The result does not depend on the window or the bands beyond the window
// containing every covered pixel: a pixel's word is the minimum over the triangles that cover it, and every triangle whose box
// meets a band is rasterised in it.
// The triangles: every thread sets one up (tri_setup and cover are what k_raster calls, so a pixel's z is the same operations
// on the same operands), VF at a time and neighbours in the mesh in different waves.  A wave then walks its own triangles whose box
// meets the band one after another, the setup broadcast from its lane and the 64 lanes striding box ∩ band as k_raster's do.
// A wave that set up one triangle at a time would wait for a chain of three dependent loads per triangle with nothing else to
// do; and a box of VF_BIG pixels or more is not walked by its wave but queued in LDS and then walked by the whole workgroup:
// a few large triangles would otherwise keep one wave busy long after the other 15 have finished.
constexpr int VF = 1024;                        // threads per workgroup: 16 waves, four per SIMD
constexpr int VF_WAVES = VF / FL_WAVE;
constexpr int VF_BIG = VF;                      // pixels of box ∩ band from which a triangle is the workgroup's
constexpr int VF_QUEUE = 64;                    // such triangles held at a time; one more is walked by its wave after all
constexpr int VF_ENTRY = 17;                    // words of a queued triangle: c[3], n, D, x0, x1, y0, y1
constexpr unsigned Z_EMPTY = 0xFFFFFFFFu;

struct FusedArgs {
  FlVerifyFusedJob j;
  float ifx, ify;
  int budget;                                   // pixels of a band, FL_WAVE .. FL_VERIFY_FUSED_PX: what the launch's dynamic LDS holds
};

// k_raster's rejection and bounding box (fl_render.hip, "bbox" in its contract), margins and clamp included.  false: rejected.
// A COPY of the lines at the top of k_raster, which stays as it is: the two are bound to each other, and a change to one is a
// change to the other (tests/test_gpu_verify_fused.py holds the fused records to the rendered ones bit for bit).
__device__ __forceinline__ bool tri_box(const RenderArgs &a, const TriSetup &s, int &x0, int &x1, int &y0, int &y1)
{
  if (!s.ok || !(s.P[0].z > 0.f || s.P[1].z > 0.f || s.P[2].z > 0.f)) return false;
  x0 = 0; x1 = a.w - 1; y0 = 0; y1 = a.h - 1;
  if (s.P[0].z > 0.f && s.P[1].z > 0.f && s.P[2].z > 0.f) {
    float u0 = INFINITY, u1 = -INFINITY, v0 = INFINITY, v1 = -INFINITY;
    for (int k = 0; k < 3; ++k) {
      const float pu = a.fx * (s.P[k].x / s.P[k].z) + a.cx, pv = a.fy * (s.P[k].y / s.P[k].z) + a.cy;
      u0 = fminf(u0, pu); u1 = fmaxf(u1, pu);
      v0 = fminf(v0, pv); v1 = fmaxf(v1, pv);
    }
    const float wm = (float)(a.w - 1), hm = (float)(a.h - 1);
    x0 = (int)fminf(fmaxf(floorf(u0) - 1.f, 0.f), wm);
    x1 = (int)fminf(fmaxf(ceilf(u1) + 1.f, 0.f), wm);
    y0 = (int)fminf(fmaxf(floorf(v0) - 1.f, 0.f), hm);
    y1 = (int)fminf(fmaxf(ceilf(v1) + 1.f, 0.f), hm);
  }
  return true;
}

__device__ __forceinline__ float lane_f(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ F3 lane_f3(F3 v, int k) { return F3{lane_f(v.x, k), lane_f(v.y, k), lane_f(v.z, k)}; }

// q = p / d and r = p % d for 0 <= p <= VF and 1 <= d < 2^24 without the integer division's 30 instructions: both are exact
// as floats, the reciprocal and the product are each within a few 2^-24 of their true values, so the product is within 2^-10
// of p / d and its integer part within one of the quotient, which the remainder then shows.
__device__ __forceinline__ void divmod24(int p, int d, int &q, int &r)
{
  q = (int)((float)p * __builtin_amdgcn_rcpf((float)d));
  r = p - q * d;
  if (r < 0) { --q; r += d; }
  else if (r >= d) { ++q; r -= d; }
}

// Pixels first, first + stride, ... of the box [x0, x1] x [y0, y1] in row-major order (k_raster's p = lane, lane + 64, ...):
// depth-tested into the band's z-buffer zb, whose word (0, 0) is pixel (bx, by) and whose rows are cw long.  The box lies in
// the band.  A lane keeps (x, y) and moves on by stride % iw columns and stride / iw rows.
__device__ __forceinline__ void raster_box(const RenderArgs &r, const TriSetup &u, int x0, int x1, int y0, int y1, int first, int stride,
                                           unsigned *zb, int bx, int by, int cw)
{
  const int iw = x1 - x0 + 1;                   // <= FL_RENDER_MAX_DIM
  int sq, sr, q, rem;
  divmod24(stride, iw, sq, sr);
  divmod24(first, iw, q, rem);
  int x = x0 + rem, y = y0 + q;
  while (y <= y1) {
    const float dx = ((float)x - r.cx) * r.ifx, dy = ((float)y - r.cy) * r.ify;
    float E[3], z;
    if (cover(u, dx, dy, E, &z)) atomicMin(&zb[(y - by) * cw + (x - bx)], __float_as_uint(z));
    x += sr; y += sq;
    if (x > x1) { x -= iw; ++y; }
  }
}

// One pose by one workgroup: the mesh tri .. n_t (of the job's vertex array) at `pose` against the frame `scn`, the counts into
// accumulator t.  The whole of both kernels below but for which pose, which frame, which mesh and whether at all.
__device__ __forceinline__ void verify_fused_pose(const FusedArgs &a, int t, const float *pose, const uint16_t *scn, const int32_t *tri, int n_t)
{
  extern __shared__ unsigned zbuf[];            // a band's z-buffer, a.budget words
  __shared__ int red[9][VF_WAVES];
  __shared__ unsigned long long red_sum[VF_WAVES];
  __shared__ float queue[VF_QUEUE][VF_ENTRY];   // the triangles the whole workgroup walks
  __shared__ int q_n;
  const FlVerifyFusedJob &j = a.j;
  const int tid = threadIdx.x, lane = tid & (FL_WAVE - 1), wave = tid / FL_WAVE;
  RenderArgs r;
  r.vtx = j.mesh.vtx; r.nrm = nullptr; r.col = nullptr; r.tri = tri; r.pose = j.pose;
  r.n_t = n_t; r.w = j.w; r.h = j.h;
  r.fx = j.fx; r.fy = j.fy; r.cx = j.cx; r.cy = j.cy; r.ifx = a.ifx; r.ify = a.ify;
  r.lx = 0.f; r.ly = 0.f; r.lz = 0.f; r.ambient = 0.f;

  // 1. the window, a triangle per thread
  int wx0, wx1, wy0, wy1;
  {
    int v[4] = {-j.w, -1, -j.h, -1};            // -x0, x1, -y0, y1: four maxima
    for (int i = tid; i < r.n_t; i += VF) {
      const TriSetup s = tri_setup(r, pose, i);
      int x0, x1, y0, y1;
      if (!tri_box(r, s, x0, x1, y0, y1)) continue;
      v[0] = max(v[0], -x0); v[1] = max(v[1], x1); v[2] = max(v[2], -y0); v[3] = max(v[3], y1);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = max(v[k], __shfl_xor(v[k], s, FL_WAVE));
    }
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][wave] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int wv = 0; wv < VF_WAVES; ++wv) {
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = max(v[k], red[k][wv]);
    }
    wx0 = -v[0]; wx1 = v[1]; wy0 = -v[2]; wy1 = v[3];
    __syncthreads();                            // step 3 writes red again, and an empty window has no barrier in between
  }

  // 2. the bands.  An empty window (wx1 < wx0, and then wy1 < wy0 too) has none.
  VerifyCount c = {0, 0, 0, 0, 0, 0, j.w, -1, j.h, -1};
  unsigned long long sum = 0;                   // c.sum is emptied into it after every band: a band gives a thread < 2^30
  const int bw = min(wx1 - wx0 + 1, a.budget), bh = wx1 >= wx0 ? max(1, a.budget / bw) : 1;
  for (int by = wy0; by <= wy1; by += bh) {
    for (int bx = wx0; bx <= wx1; bx += bw) {
      const int cw = min(bw, wx1 - bx + 1), ch = min(bh, wy1 - by + 1), n = cw * ch;   // n <= a.budget
      for (int i = tid; i < n; i += VF) zbuf[i] = Z_EMPTY;
      for (int base = 0; base < r.n_t; base += VF) {          // uniform: every thread reaches the barriers, ballots and broadcasts
        if (tid == 0) q_n = 0;
        __syncthreads();                        // the z-buffer is clear; the queue is empty and nobody reads its length any more
        const int i = base + lane * VF_WAVES + wave;
        TriSetup s = {};
        int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
        bool hit = false;
        if (i < r.n_t) {
          s = tri_setup(r, pose, i);
          hit = tri_box(r, s, x0, x1, y0, y1);
        }
        x0 = max(x0, bx); x1 = min(x1, bx + cw - 1);
        y0 = max(y0, by); y1 = min(y1, by + ch - 1);
        hit = hit && x0 <= x1 && y0 <= y1;
        if (hit && (x1 - x0 + 1) * (y1 - y0 + 1) >= VF_BIG) {
          const int slot = atomicAdd(&q_n, 1);
          if (slot < VF_QUEUE) {
            float *e = queue[slot];
            e[0] = s.c[0].x; e[1] = s.c[0].y; e[2] = s.c[0].z; e[3] = s.c[1].x; e[4] = s.c[1].y; e[5] = s.c[1].z;
            e[6] = s.c[2].x; e[7] = s.c[2].y; e[8] = s.c[2].z; e[9] = s.n.x; e[10] = s.n.y; e[11] = s.n.z; e[12] = s.D;
            e[13] = __int_as_float(x0); e[14] = __int_as_float(x1); e[15] = __int_as_float(y0); e[16] = __int_as_float(y1);
            hit = false;
          }
        }
        for (unsigned long long m = __ballot(hit); m; m &= m - 1) {
          const int k = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
          TriSetup u;                           // what cover reads of lane k's setup
#pragma unroll
          for (int e = 0; e < 3; ++e) u.c[e] = lane_f3(s.c[e], k);
          u.n = lane_f3(s.n, k);
          u.D = lane_f(s.D, k);
          raster_box(r, u, __builtin_amdgcn_readlane(x0, k), __builtin_amdgcn_readlane(x1, k), __builtin_amdgcn_readlane(y0, k),
                     __builtin_amdgcn_readlane(y1, k), lane, FL_WAVE, zbuf, bx, by, cw);
        }
        __syncthreads();                        // the queue is complete
        const int nq = min(q_n, VF_QUEUE);
        for (int k = 0; k < nq; ++k) {
          const float *e = queue[k];
          TriSetup u;
          u.c[0] = F3{e[0], e[1], e[2]}; u.c[1] = F3{e[3], e[4], e[5]}; u.c[2] = F3{e[6], e[7], e[8]};
          u.n = F3{e[9], e[10], e[11]};
          u.D = e[12];
          raster_box(r, u, __float_as_int(e[13]), __float_as_int(e[14]), __float_as_int(e[15]), __float_as_int(e[16]), tid, VF, zbuf, bx, by, cw);
        }
        __syncthreads();                        // the band is rendered as far as these triangles go, and the queue is read
      }
      int sq, sr, py, px;                       // band pixel tid, tid + VF, ... as (px, py), moved on as raster_box moves
      divmod24(VF, cw, sq, sr);
      divmod24(tid, cw, py, px);
      for (int i0 = tid; i0 < n; i0 += 4 * VF) {
        int rv[4], sv[4], idx[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + q * VF;
          const unsigned zw = i < n ? zbuf[i] : Z_EMPTY;
          rv[q] = zw == Z_EMPTY ? 0 : (int)(uint16_t)fminf(rintf(__uint_as_float(zw)), 65535.f);   // k_resolve's depth
          idx[q] = (by + py) * j.w + bx + px;
          px += sr; py += sq;
          if (px >= cw) { px -= cw; ++py; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) sv[q] = rv[q] ? (int)scn[idx[q]] : 0;   // the scene only under a rendered pixel
#pragma unroll
        for (int q = 0; q < 4; ++q) verify_px(rv[q], sv[q], idx[q], j.w, j.tau, c);
      }
      sum += (unsigned)c.sum;
      c.sum = 0;
      __syncthreads();                          // the next band clears what this one read
    }
  }

  // 3. the wave, then the workgroup: one workgroup per pose, so plain stores
  int v[9] = {c.model, c.missing, c.inlier, c.front, c.behind, -c.x0, c.x1, -c.y0, c.y1};   // 0..4 add, 5..8 max
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] += __shfl_xor(v[k], s, FL_WAVE);
#pragma unroll
    for (int k = 5; k < 9; ++k) v[k] = max(v[k], __shfl_xor(v[k], s, FL_WAVE));
    sum += __shfl_xor(sum, s, FL_WAVE);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) red[k][wave] = v[k];
    red_sum[wave] = sum;
  }
  __syncthreads();
  if (tid != 0) return;
#pragma unroll
  for (int wv = 1; wv < VF_WAVES; ++wv) {
#pragma unroll
    for (int k = 0; k < 5; ++k) v[k] += red[k][wv];
#pragma unroll
    for (int k = 5; k < 9; ++k) v[k] = max(v[k], red[k][wv]);
    sum += red_sum[wv];
  }
  FlVerifyAcc o;
#pragma unroll
  for (int k = 0; k < 5; ++k) o.n[k] = v[k];
  o.box[0] = j.w + v[5]; o.box[1] = j.h + v[7]; o.box[2] = v[6] + 1; o.box[3] = v[8] + 1;   // all zero when nothing rendered
  o.pad = 0;
  o.sum = sum;
  ((FlVerifyAcc *)j.acc)[t] = o;
}

// the poses of a recognition batch or of fl_verify_batch
__global__ __launch_bounds__(VF) void k_verify_fused(FusedArgs a)
{
  const FlVerifyFusedJob &j = a.j;
  // Workgroups go to the device's eight XCDs in turn.  The live slots of a recognition batch are the same few slots of every
  // frame, so in slot order some XCDs would get twice the poses of others; walking the frames first deals them out evenly.
  int t = blockIdx.x;
  if (!j.frame_of) {
    const int n_frames = j.n_poses / j.per_frame, slot = t / n_frames;
    t = (t - slot * n_frames) * j.per_frame + slot;
  }
  int m = 0;                                    // the pose's mesh: wave-uniform, as t is
  if (j.job_idx) {
    if (!(j.job_idx[t] >= 0 && j.res[t].found == 1)) return;
    m = j.mesh_of[j.res[t].best.class_idx];     // the map from classes to meshes; found = 1: the class is on the detector
    if (m < 0) return;
  } else if (j.mesh_of) {
    m = j.mesh_of[t];
  }
  const int32_t *tri = j.mesh.tri;
  int n_t = j.mesh.n_t;
  if (j.ranges) {
    const FlMeshRange r = j.ranges[m];
    tri += 3 * (size_t)r.tri_first;
    n_t = r.n_t;
  }
  verify_fused_pose(a, t, j.pose + (size_t)t * j.pose_stride,
                    (const uint16_t *)(j.frames + j.frame_stride * (size_t)(j.frame_of ? j.frame_of[t] : t / j.per_frame)), tri, n_t);
}

// a tracker's tracks (FlVerifyFusedJob::skip): the poses the passes returned, then the poses the call came in with
__global__ __launch_bounds__(VF) void k_verify_fused_tracks(FusedArgs a)
{
  const FlVerifyFusedJob &j = a.j;
  const int t = blockIdx.x, u = t < j.split ? t : t - j.split;
  if (j.skip[u]) return;                        // lost in the passes: no mesh walk (uniform per workgroup)
  const int32_t *tri = j.mesh.tri;
  int n_t = j.mesh.n_t;
  if (j.ranges) {
    const FlMeshRange r = j.ranges[j.mesh_of ? j.mesh_of[u] : 0];
    tri += 3 * (size_t)r.tri_first;
    n_t = r.n_t;
  }
  verify_fused_pose(a, t, (t < j.split ? j.pose : j.pose_in) + (size_t)u * j.pose_stride,
                    (const uint16_t *)(j.frames + j.frame_stride * (size_t)j.frame_of[u]), tri, n_t);
}

__global__ __launch_bounds__(64) void k_verify_finish(VerifyArgs a)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= a.n_poses) return;
  fl_verify_result o = fl_verify_record(a.acc[t], a.w, a.h, a.min_model_px, a.min_inlier_ratio, a.max_behind_ratio);
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

static_assert(sizeof(fl_verify_result) == 64, "fl_verify_result is 64 bytes (include/fealess_hip.h)");
static_assert(sizeof(fl_verified_track_result) == 368, "fl_verified_track_result is 368 bytes (include/fealess_hip.h)");
static const fl_verify_params k_verify_defaults = {10, 1, 0.f, 0.f};

int fl_launch_verify_fused(fl_context *ctx, const FlVerifyFusedJob &j)
{
  // LDS above 64 KB is a kernel's to ask for, once per device, and for the compiled budget whatever this launch uses
  if (!ctx->verify_fused_attr) {
    FL_HIP(ctx, hipFuncSetAttribute((const void *)k_verify_fused, hipFuncAttributeMaxDynamicSharedMemorySize, FL_VERIFY_FUSED_PX * 4));
    FL_HIP(ctx, hipFuncSetAttribute((const void *)k_verify_fused_tracks, hipFuncAttributeMaxDynamicSharedMemorySize, FL_VERIFY_FUSED_PX * 4));
    ctx->verify_fused_attr = true;
  }
  FusedArgs a = {j, 1.0f / j.fx, 1.0f / j.fy, (int)(ctx->opt.verify_fused_px ? ctx->opt.verify_fused_px : FL_VERIFY_FUSED_PX)};   // ifx, ify: as fl_launch_render_chunk
  hipLaunchKernelGGL(j.skip ? k_verify_fused_tracks : k_verify_fused, dim3((unsigned)j.n_poses), dim3(VF), (size_t)a.budget * 4, ctx->stream, a);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

// k_verify_finish over n_poses accumulators, every pose its own group (best = accepted)
int fl_launch_verify_finish(fl_context *ctx, int n_poses, int w, int h, const fl_verify_params &P, const void *acc, fl_verify_result *out)
{
  VerifyArgs a = {};
  a.n_poses = n_poses; a.w = w; a.h = h;
  a.min_model_px = P.min_model_px; a.min_inlier_ratio = P.min_inlier_ratio; a.max_behind_ratio = P.max_behind_ratio;
  a.acc = (FlVerifyAcc *)acc;
  a.out = out;
  hipLaunchKernelGGL(k_verify_finish, dim3((n_poses + 63) / 64), dim3(64), 0, ctx->stream, a);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

int fl_verify_check_call(fl_tracker *trk, const char *who, const fl_intrinsics *K, int n, int n_groups, const int32_t *group_first)
{
  fl_context *ctx = trk->ctx;
  // 1e-60 is a positive double and a zero float, 1e300 an infinite one
  const float fx = (float)K->fx, fy = (float)K->fy, cx = (float)K->cx, cy = (float)K->cy;
  if (!(std::isfinite(fx) && fx > 0.f && std::isfinite(fy) && fy > 0.f && std::isfinite(cx) && std::isfinite(cy)))
    return fl_set_error(ctx, FL_ERR_INVALID, "%s: fx, fy must be finite and > 0, cx, cy finite, as floats too", who);
  if (group_first) {
    bool ok = n_groups >= 1 && n_groups <= trk->max_tracks && group_first[0] == 0;
    for (int g = 0; ok && g < n_groups; ++g) ok = group_first[g + 1] >= group_first[g] && group_first[g + 1] <= n;
    if (!ok || group_first[n_groups] != n)
      return fl_set_error(ctx, FL_ERR_INVALID, "%s: group_first must have n_groups + 1 (n_groups 1..%d) non-decreasing entries from 0 to the number of poses",
                          who, trk->max_tracks);
  }
  return FL_OK;
}

bool fl_verify_params_ok(const fl_verify_params &P)
{
  return P.tau_mm >= 0 && P.tau_mm <= 65535 && P.min_model_px >= 1 && std::isfinite(P.min_inlier_ratio) && std::isfinite(P.max_behind_ratio);
}

// device time of the last fl_verify_batch by stage: {copy, render, score, finish and pick} in ms; with verify_fused the render
// stage is empty and the score stage is k_verify_fused
extern "C" int fl_dev_tracker_verify_ms(fl_tracker *trk, float out[4])
{
  if (!trk || !out || !trk->verified) return FL_ERR_INVALID;
  const hipEvent_t *ev = trk->ev + FL_TRACK_EVENTS;
  for (int k = 0; k < 4; ++k)
    if (hipEventElapsedTime(out + k, ev[k], ev[k + 1]) != hipSuccess) return FL_ERR_HIP;
  return FL_OK;
}

// fl_verify_batch_meshes behind its checks (fl_track_internal.h), queued and not waited for
int fl_verify_queue(fl_tracker *trk, hipEvent_t *ev, int n_frames, const uint16_t *const *depth, int mem, int n_poses, const int32_t *frame_of_pose,
                    const int32_t *mesh_of_pose, const float *poses13, int n_starts, const int32_t *starts, bool pick, bool fused,
                    const fl_intrinsics *K, const fl_verify_params &P)
{
  fl_context *ctx = trk->ctx;
  const float fx = (float)K->fx, fy = (float)K->fy, cx = (float)K->cx, cy = (float)K->cy;
  const int32_t *group_first = pick ? starts : nullptr;
  const int n_groups = n_starts;
  int rc;
  // 1. the inputs, and the groups (or a scene call's scenes) after them
  if ((rc = fl_tracker_stage(trk, ev[0], n_frames, depth, mem, n_poses, frame_of_pose, mesh_of_pose, poses13, nullptr))) return rc;
  const size_t px = (size_t)trk->w * trk->h, T = (size_t)n_poses;
  hipStream_t st = ctx->stream;
  if (starts) {
    memcpy(trk->stage.group_first, starts, ((size_t)n_starts + 1) * 4);
    FL_HIP(ctx, hipMemcpyAsync(trk->d_group_first, trk->stage.group_first, ((size_t)n_starts + 1) * 4, hipMemcpyHostToDevice, st));
  }
  FL_HIP(ctx, hipMemsetAsync(trk->d_vacc, 0, T * sizeof(FlVerifyAcc), st));
  FL_HIP(ctx, hipEventRecord(ev[1], st));
  // 2. the render, at the scene's K
  if (!fused && (rc = fl_tracker_render(trk, n_poses, fx, fy, cx, cy))) return rc;
  FL_HIP(ctx, hipEventRecord(ev[2], st));
  // 3. the counts
  VerifyArgs a = {n_poses, group_first ? n_groups : 0, trk->w, trk->h, (int)((px + V_STRIP_PX - 1) / V_STRIP_PX), P.tau_mm, P.min_model_px,
                  P.min_inlier_ratio, P.max_behind_ratio, trk->d_render, trk->d_frames, trk->frame_stride, trk->d_frame_of,
                  group_first ? trk->d_group_first : nullptr, (FlVerifyAcc *)trk->d_vacc, trk->d_vres};               // in VerifyArgs' order
  if (fused) {                                  // render and counts in one kernel, poses and frames where fl_tracker_stage put them
    const FlVerifyFusedJob j = {n_poses, trk->w, trk->h, P.tau_mm, fx, fy, cx, cy, {trk->d_vtx, nullptr, nullptr, trk->d_tri, trk->n_t},
                                trk->d_poses, 13, trk->d_frames, trk->frame_stride, trk->d_frame_of, 1, nullptr, nullptr, trk->call_mesh_of, trk->d_vacc,
                                nullptr, 0, nullptr, trk->call_ranges};
    if ((rc = fl_launch_verify_fused(ctx, j))) return rc;
  } else {
    hipLaunchKernelGGL(k_verify_score, dim3((unsigned)(n_poses * a.n_strips)), dim3(VB), 0, st, a);   // <= 2^16 * 2^13 workgroups
    FL_HIP(ctx, hipGetLastError());
  }
  FL_HIP(ctx, hipEventRecord(ev[3], st));
  // 4. ratios and accepted per pose, then the best of every group
  hipLaunchKernelGGL(k_verify_finish, dim3((n_poses + 63) / 64), dim3(64), 0, st, a);
  FL_HIP(ctx, hipGetLastError());
  if (group_first) {
    hipLaunchKernelGGL(k_verify_pick, dim3((n_groups + 63) / 64), dim3(64), 0, st, a);
    FL_HIP(ctx, hipGetLastError());
  }
  FL_HIP(ctx, hipEventRecord(ev[4], st));
  return FL_OK;
}

extern "C" int fl_verify_batch_meshes(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_poses,
                                      const int32_t *frame_of_pose, const int32_t *mesh_of_pose, const float *poses13, int n_groups,
                                      const int32_t *group_first, const fl_intrinsics *K, const fl_verify_params *params, fl_verify_result *results)
{
  int rc = fl_tracker_check_call(trk, "fl_verify_batch", n_frames, depth, mem, n_poses, frame_of_pose, mesh_of_pose, poses13, K, results);
  if (rc) return rc;
  if ((rc = fl_verify_check_call(trk, "fl_verify_batch", K, n_poses, n_groups, group_first))) return rc;
  fl_context *ctx = trk->ctx;
  const fl_verify_params P = params ? *params : k_verify_defaults;
  if (!fl_verify_params_ok(P))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_verify_params: tau_mm 0..65535, min_model_px >= 1, finite thresholds");
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "fl_verify_batch: the tracker has no device");
  // 1. to 4. the inputs, the render, the counts, the records and the best of every group
  if ((rc = fl_verify_queue(trk, trk->ev + FL_TRACK_EVENTS, n_frames, depth, mem, n_poses, frame_of_pose, mesh_of_pose, poses13, group_first ? n_groups : 0,
                            group_first, group_first != nullptr, ctx->opt.verify_fused != 0, K, P)))
    return rc;
  // 5. one copy, one wait
  if ((rc = fl_tracker_results(trk, trk->d_vres, (size_t)n_poses * sizeof(fl_verify_result), results))) return rc;
  trk->verified = true;
  return FL_OK;
}

extern "C" int fl_verify_batch(fl_tracker *trk, int n_frames, const uint16_t *const *depth, int mem, int n_poses,
                               const int32_t *frame_of_pose, const float *poses13, int n_groups, const int32_t *group_first,
                               const fl_intrinsics *K, const fl_verify_params *params, fl_verify_result *results)
{
  return fl_verify_batch_meshes(trk, n_frames, depth, mem, n_poses, frame_of_pose, nullptr, poses13, n_groups, group_first, K, params, results);
}
