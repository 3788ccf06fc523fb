// fl_raster.h -- the rasteriser's per-triangle arithmetic, shared by the kernels that rasterise (fl_render.hip: k_raster and
// k_resolve in HBM; fl_verify.hip: k_verify_fused in LDS; not part of the ABI).  The arithmetic contract is the one at the top
// of fl_render.hip: float32, one IEEE operation per operator (-ffp-contract=off), in exactly this order.
#pragma once
#include "fl_internal.h"
#include <math.h>

namespace {

struct RenderArgs {
  const float *vtx;                             // n_v * 3
  const float *nrm;                             // n_v * 3 or NULL
  const uint8_t *col;                           // n_v * 3 or NULL
  const int32_t *tri;                           // n_t * 3
  const float *pose;                            // the chunk's views, 13 floats each
  int n_t, w, h;
  float fx, fy, cx, cy, ifx, ify;
  float lx, ly, lz, ambient;
};

struct F3 { float x, y, z; };

__device__ __forceinline__ F3 cross3(F3 a, F3 b)
{
  return F3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float dot3(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ F3 neg3(F3 a) { return F3{-a.x, -a.y, -a.z}; }

__device__ __forceinline__ F3 xform(const float *p, F3 v, bool with_t)
{
  F3 o;
  o.x = (p[0] * v.x + p[1] * v.y) + p[2] * v.z;
  o.y = (p[4] * v.x + p[5] * v.y) + p[6] * v.z;
  o.z = (p[8] * v.x + p[9] * v.y) + p[10] * v.z;
  if (with_t) { o.x = o.x + p[3]; o.y = o.y + p[7]; o.z = o.z + p[11]; }
  return o;
}

__device__ __forceinline__ F3 load3(const float *a, int i) { return F3{a[3 * i], a[3 * i + 1], a[3 * i + 2]}; }

struct TriSetup {
  F3 P[3], c[3], n;
  float D;
  bool ok;                                      // false: edge-on (D == 0 or NaN)
};

__device__ __forceinline__ TriSetup tri_setup(const RenderArgs &a, const float *pose, int t)
{
  TriSetup s;
  for (int k = 0; k < 3; ++k) s.P[k] = xform(pose, load3(a.vtx, a.tri[3 * t + k]), true);
  s.c[0] = cross3(s.P[1], s.P[2]);
  s.c[1] = cross3(s.P[2], s.P[0]);
  s.c[2] = cross3(s.P[0], s.P[1]);
  const F3 e1{s.P[1].x - s.P[0].x, s.P[1].y - s.P[0].y, s.P[1].z - s.P[0].z};
  const F3 e2{s.P[2].x - s.P[0].x, s.P[2].y - s.P[0].y, s.P[2].z - s.P[0].z};
  s.n = cross3(e1, e2);
  s.D = dot3(s.P[0], s.n);
  s.ok = s.D > 0.f || s.D < 0.f;
  if (s.D < 0.f) {
    for (int k = 0; k < 3; ++k) s.c[k] = neg3(s.c[k]);
    s.n = neg3(s.n);
    s.D = -s.D;
  }
  return s;
}

__device__ __forceinline__ bool edge_in(F3 c, float e)
{
  return e > 0.f || (e == 0.f && (c.x > 0.f || (c.x == 0.f && c.y > 0.f)));
}

// Coverage of pixel ray (dx, dy, 1); z and the edge values on success.
__device__ __forceinline__ bool cover(const TriSetup &s, float dx, float dy, float E[3], float *z)
{
  bool in = true;
  for (int k = 0; k < 3; ++k) {
    E[k] = (s.c[k].x * dx + s.c[k].y * dy) + s.c[k].z;
    in = in && edge_in(s.c[k], E[k]);
  }
  const float S = (s.n.x * dx + s.n.y * dy) + s.n.z;
  if (!in || !(S > 0.f)) return false;
  *z = s.D / S;
  return *z > 0.f && *z < INFINITY;
}

}  // namespace
