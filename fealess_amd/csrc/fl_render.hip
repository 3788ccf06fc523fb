// fl_render.hip -- batched z-buffer rasteriser: RGB-D training views of a triangle mesh, rendered in HBM
// (fl_render_views), and the view sphere that poses them (fl_view_sphere, host only).  No counterpart in the
// reference, which reads views that another tool wrote (test/linemod_train.cpp:93-144, 180-255).
//
// Arithmetic contract.  Everything is float32, one IEEE operation per operator (-ffp-contract=off; '/' and sqrtf are
// correctly rounded on gfx950), in exactly this order, so that a float32 restatement (tests/raster_model.py) matches
// bit for bit.  a x b = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x); dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
//   host    fx, fy, cx, cy = (float) of the doubles; ifx = 1/fx, ify = 1/fy; l = light / sqrtf(dot(light, light))
//   vertex  P_k = ((r_j0*x + r_j1*y) + r_j2*z) + t_j, j = 0..2 ([R|t] = poses13[0..11] row-major; [12] is ignored);
//           a per-vertex normal goes through the same expression without "+ t_j"
//   setup   c0 = P1 x P2, c1 = P2 x P0, c2 = P0 x P1 (edge functions: a shared edge gets bitwise-negated coefficients)
//           n = (P1 - P0) x (P2 - P0), D = dot(P0, n); D == 0 (or NaN): edge-on, covers nothing
//           D < 0: c0, c1, c2, n and D are negated (exact), so that inside means E_k >= 0 and D > 0
//           every vertex at z <= 0 (no vertex z > 0): covers nothing -- no point of it lies in front of the camera
//   bbox    every vertex z > 0: pu = fx*(x/z) + cx, pv = fy*(y/z) + cy; x0 = (int)clamp(floor(min pu) - 1, 0, w-1),
//           x1 = (int)clamp(ceil(max pu) + 1, 0, w-1), rows likewise (clamp = fminf(fmaxf(.))); a vertex with
//           z <= 0: the whole image.  Triangles are not clipped: the ray test decides.
//   pixel   dx = ((float)u - cx)*ifx, dy = ((float)v - cy)*ify (depthTo3dNoMask, ICP/depth_to_3d.cpp:103-121)
//           E_k = (c_k.x*dx + c_k.y*dy) + c_k.z; edge k keeps E_k == 0 when c_k.x > 0 || (c_k.x == 0 && c_k.y > 0)
//           (top-left style: of two same-facing triangles sharing an edge, exactly one owns a pixel on it)
//           S = (n.x*dx + n.y*dy) + n.z; covered iff every edge passes, S > 0 and 0 < z = D/S < +inf
//   depth   key = bits(z) << 32 | triangle, atomicMin: nearest wins, equal z goes to the lower index, whatever the
//           schedule; depth = (u16)fminf(rintf(z), 65535) (a hit nearer than 0.5 mm reads 0, as does background)
//   shade   E = (E0 + E1) + E2, b_k = E_k / E (b = (1, 0, 0) if E is not > 0): perspective-correct, as E_k are the
//           3-D barycentric volumes of the hit; albedo_c = (b0*a0c + b1*a1c) + b2*a2c (a = (float)u8, or FL_RENDER_GREY);
//           N = (b0*N0 + b1*N1) + b2*N2 per component (or the face normal n); L2 = dot(N, N); L2 > 0:
//           s = sqrtf(L2), f = fminf(fmaxf(fabsf(dot(N/s, l)), ambient), 1) (N/s per component); otherwise f = ambient;
//           bgr_c = (u8)fminf(fmaxf(rintf(albedo_c*f), 0), 255)
// Schedule: the key image of a chunk of views is cleared to 0xFF..; k_raster runs one wave per (view, triangle): the
// setup is wave-uniform, the lanes stride over the bounding box; k_resolve then turns each pixel's key into the outputs,
// recomputing the winner's setup for the shading.  The depth test is the vector 64-bit atomic (global_atomic_umin_x2).
#include "fl_raster.h"
#include <algorithm>
#include <map>
#include <vector>

namespace {

constexpr int RB = 256;                         // k_raster: 4 waves per block, one triangle each
constexpr unsigned long long KEY_EMPTY = ~0ull;

// RenderArgs, tri_setup and cover: fl_raster.h, which k_verify_fused (fl_verify.hip) shares

// The rejection and the bounding box below are restated by tri_box (fl_verify.hip), whose window is the union of these boxes:
// the two are bound to each other.
// MULTI (a tracker of several meshes, fl_track.hip): view v walks the triangles of ranges[mesh_of[v]], t counted inside that
// mesh, so that the key's tie rule stays the mesh's own; the grid is sized by the largest mesh and a wave past its view's mesh
// exits.  MULTI = false takes neither argument and is the kernel as it was.
template <bool MULTI>
__global__ __launch_bounds__(RB) void k_raster(RenderArgs a, unsigned long long *keys, const FlMeshRange *ranges, const int32_t *mesh_of)
{
  const int t = blockIdx.x * (RB / FL_WAVE) + (int)(threadIdx.x / FL_WAVE);
  const int lane = threadIdx.x % FL_WAVE;
  if (MULTI) {                                  // uniform per workgroup: blockIdx.y alone decides
    const FlMeshRange r = ranges[mesh_of[blockIdx.y]];
    a.tri += 3 * (size_t)r.tri_first;
    a.n_t = r.n_t;
  }
  if (t >= a.n_t) return;
  const int v = blockIdx.y;
  const float *pose = a.pose + 13 * v;
  const TriSetup s = tri_setup(a, pose, t);
  if (!s.ok || !(s.P[0].z > 0.f || s.P[1].z > 0.f || s.P[2].z > 0.f)) return;
  int x0 = 0, x1 = a.w - 1, y0 = 0, y1 = a.h - 1;
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
  const int bw = x1 - x0 + 1, nb = bw * (y1 - y0 + 1);   // <= FL_RENDER_MAX_DIM^2, fits an int
  unsigned long long *kv = keys + (size_t)v * a.w * a.h;
  for (int p = lane; p < nb; p += FL_WAVE) {
    const int py = p / bw, x = x0 + (p - py * bw), y = y0 + py;
    const float dx = ((float)x - a.cx) * a.ifx, dy = ((float)y - a.cy) * a.ify;
    float E[3], z;
    if (!cover(s, dx, dy, E, &z)) continue;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)t;
    atomicMin(kv + (size_t)y * a.w + x, key);
  }
}

// One thread per pixel of the chunk, pixels of all its views in one flat range.  Output pointers are the chunk's
// (NULL: not wanted).
__global__ __launch_bounds__(256) void k_resolve(RenderArgs a, const unsigned long long *keys, long long n_px, uint8_t *bgr,
                                                 uint16_t *depth, uint8_t *mask, int32_t *tri)
{
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_px) return;
  const int px = a.w * a.h;
  const int v = (int)(g / px), i = (int)(g - (long long)v * px);
  const unsigned long long key = keys[g];
  if (key == KEY_EMPTY) {
    if (bgr) { bgr[3 * g] = 0; bgr[3 * g + 1] = 0; bgr[3 * g + 2] = 0; }
    if (depth) depth[g] = 0;
    if (mask) mask[g] = 0;
    if (tri) tri[g] = -1;
    return;
  }
  const int t = (int)(unsigned)(key & 0xffffffffu);
  const float z = __uint_as_float((unsigned)(key >> 32));
  if (depth) depth[g] = (uint16_t)fminf(rintf(z), 65535.f);
  if (mask) mask[g] = 255;
  if (tri) tri[g] = t;
  if (!bgr) return;
  const float *pose = a.pose + 13 * v;
  const TriSetup s = tri_setup(a, pose, t);
  const int y = i / a.w, x = i - y * a.w;
  const float dx = ((float)x - a.cx) * a.ifx, dy = ((float)y - a.cy) * a.ify;
  float E[3], zz;
  cover(s, dx, dy, E, &zz);                     // the winner covered this pixel: recomputes the same E
  const float Es = (E[0] + E[1]) + E[2];
  float b0 = 1.f, b1 = 0.f, b2 = 0.f;
  if (Es > 0.f) { b0 = E[0] / Es; b1 = E[1] / Es; b2 = E[2] / Es; }
  const int i0 = a.tri[3 * t], i1 = a.tri[3 * t + 1], i2 = a.tri[3 * t + 2];
  F3 N = s.n;
  if (a.nrm) {
    const F3 n0 = xform(pose, load3(a.nrm, i0), false), n1 = xform(pose, load3(a.nrm, i1), false), n2 = xform(pose, load3(a.nrm, i2), false);
    N.x = (b0 * n0.x + b1 * n1.x) + b2 * n2.x;
    N.y = (b0 * n0.y + b1 * n1.y) + b2 * n2.y;
    N.z = (b0 * n0.z + b1 * n1.z) + b2 * n2.z;
  }
  const float L2 = dot3(N, N);
  float f = a.ambient;
  if (L2 > 0.f) {
    const float sl = sqrtf(L2);
    const F3 u{N.x / sl, N.y / sl, N.z / sl};
    f = fminf(fmaxf(fabsf(dot3(u, F3{a.lx, a.ly, a.lz})), a.ambient), 1.f);
  }
  for (int c = 0; c < 3; ++c) {
    float alb;
    if (a.col) alb = (b0 * (float)a.col[3 * i0 + c] + b1 * (float)a.col[3 * i1 + c]) + b2 * (float)a.col[3 * i2 + c];
    else alb = (float)FL_RENDER_GREY;
    bgr[3 * g + c] = (uint8_t)fminf(fmaxf(rintf(alb * f), 0.f), 255.f);
  }
}

}  // namespace

// views per chunk: FL_RENDER_CHUNK_VIEWS, fewer when their pixels would pass FL_RENDER_CHUNK_PIXELS
int fl_render_chunk_views(int w, int h)
{
  const long long px = (long long)w * h;
  return (int)std::max(1LL, std::min((long long)FL_RENDER_CHUNK_VIEWS, (long long)FL_RENDER_CHUNK_PIXELS / px));
}

int fl_render_check_mesh(fl_context *ctx, const char *who, const float *vertices, const float *normals, int n_vertices,
                         const int32_t *triangles, int n_triangles)
{
  if (!vertices || !triangles || n_vertices < 3 || n_triangles < 1 || n_vertices > FL_RENDER_MAX_PRIMS || n_triangles > FL_RENDER_MAX_PRIMS)
    return fl_set_error(ctx, FL_ERR_INVALID, "%s: null input or counts out of range", who);
  const size_t nv3 = (size_t)n_vertices * 3, nt3 = (size_t)n_triangles * 3;
  for (size_t i = 0; i < nt3; ++i)
    if (triangles[i] < 0 || triangles[i] >= n_vertices)
      return fl_set_error(ctx, FL_ERR_INVALID, "%s: triangle %zu has vertex index %d outside [0, %d)", who, i / 3, triangles[i], n_vertices);
  if (!fl_finite_all(vertices, nv3) || (normals && !fl_finite_all(normals, nv3)))
    return fl_set_error(ctx, FL_ERR_INVALID, "%s: non-finite vertex or normal", who);
  return FL_OK;
}

// One chunk of views on device arrays: clear the keys, k_raster, k_resolve (queued on the context's stream).
int fl_launch_render_chunk(fl_context *ctx, const FlRenderMesh &mesh, const float *d_poses13, int n_views, int w, int h, float fx, float fy,
                           float cx, float cy, const float light[3], float ambient, unsigned long long *keys, uint8_t *bgr, uint16_t *depth,
                           uint8_t *mask, int32_t *tri, const FlMeshRange *ranges, const int32_t *mesh_of, int max_n_t)
{
  RenderArgs a;
  a.vtx = mesh.vtx;
  a.nrm = mesh.nrm;
  a.col = mesh.col;
  a.tri = mesh.tri;
  a.pose = d_poses13;
  a.n_t = mesh.n_t;
  a.w = w;
  a.h = h;
  a.fx = fx; a.fy = fy; a.cx = cx; a.cy = cy;
  a.ifx = 1.0f / fx;
  a.ify = 1.0f / fy;
  a.lx = light[0]; a.ly = light[1]; a.lz = light[2];
  a.ambient = ambient;
  const size_t cpx = (size_t)n_views * w * h;
  FL_HIP(ctx, hipMemsetAsync(keys, 0xFF, cpx * 8, ctx->stream));
  if (ranges)
    hipLaunchKernelGGL(k_raster<true>, dim3((max_n_t + RB / FL_WAVE - 1) / (RB / FL_WAVE), n_views), dim3(RB), 0, ctx->stream, a, keys, ranges, mesh_of);
  else
    hipLaunchKernelGGL(k_raster<false>, dim3((mesh.n_t + RB / FL_WAVE - 1) / (RB / FL_WAVE), n_views), dim3(RB), 0, ctx->stream, a, keys,
                       (const FlMeshRange *)nullptr, (const int32_t *)nullptr);
  FL_HIP(ctx, hipGetLastError());
  hipLaunchKernelGGL(k_resolve, dim3((unsigned)((cpx + 255) / 256)), dim3(256), 0, ctx->stream, a, (const unsigned long long *)keys,
                     (long long)cpx, bgr, depth, mask, tri);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

extern "C" int fl_render_views(fl_context *ctx, const float *vertices, const float *normals, const uint8_t *colors, int n_vertices,
                               const int32_t *triangles, int n_triangles, int n_views, const float *poses13, const fl_intrinsics *K,
                               const fl_render_params *params, int mem, uint8_t *bgr, uint16_t *depth, uint8_t *mask, int32_t *tri)
{
  if (!ctx) return FL_ERR_INVALID;
  if (!vertices || !triangles || !poses13 || !K || n_vertices < 3 || n_triangles < 1 || n_views < 1 ||
      n_vertices > FL_RENDER_MAX_PRIMS || n_triangles > FL_RENDER_MAX_PRIMS)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_render_views: null input or counts out of range");
  if (!bgr && !depth && !mask && !tri) return fl_set_error(ctx, FL_ERR_INVALID, "fl_render_views: every output is NULL");
  if (mem != FL_MEM_HOST && mem != FL_MEM_DEVICE) return fl_set_error(ctx, FL_ERR_INVALID, "fl_render_views: bad mem %d", mem);
  const int w = K->width, h = K->height;
  if (w < 1 || h < 1 || w > FL_RENDER_MAX_DIM || h > FL_RENDER_MAX_DIM)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_render_views: image size %dx%d outside 1..%d", w, h, FL_RENDER_MAX_DIM);
  const float fx = (float)K->fx, fy = (float)K->fy, cx = (float)K->cx, cy = (float)K->cy;
  if (!(std::isfinite(fx) && fx > 0.f && std::isfinite(fy) && fy > 0.f && std::isfinite(cx) && std::isfinite(cy)))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_render_views: fx, fy must be finite and > 0, cx, cy finite");
  float light[3] = {0.f, 0.f, 1.f}, ambient = FL_RENDER_AMBIENT;
  if (params) {
    light[0] = params->light[0]; light[1] = params->light[1]; light[2] = params->light[2];
    ambient = params->ambient;
  }
  const float l2 = (light[0] * light[0] + light[1] * light[1]) + light[2] * light[2];
  if (!(ambient >= 0.f && ambient <= 1.f) || !(l2 > 0.f) || !std::isfinite(l2))
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_render_views: ambient outside [0, 1] or a zero / non-finite light vector");
  const size_t nv3 = (size_t)n_vertices * 3, nt3 = (size_t)n_triangles * 3;
  int rc = fl_render_check_mesh(ctx, "fl_render_views", vertices, normals, n_vertices, triangles, n_triangles);
  if (rc) return rc;
  if (!fl_finite_all(poses13, (size_t)n_views * 13)) return fl_set_error(ctx, FL_ERR_INVALID, "fl_render_views: non-finite pose");
  const float ll = sqrtf(l2);

  FL_HIP(ctx, hipSetDevice(ctx->device));
  const size_t px = (size_t)w * h;
  const int cv = fl_render_chunk_views(w, h);
  // scratch: mesh | poses of a chunk | keys of a chunk | (host outputs) staging of a chunk
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off += fl_align(b, 256); return o; };
  const size_t o_vtx = take(nv3 * 4), o_nrm = take(normals ? nv3 * 4 : 0), o_col = take(colors ? nv3 : 0), o_tri = take(nt3 * 4),
               o_pose = take((size_t)cv * 13 * 4), o_keys = take((size_t)cv * px * 8);
  const size_t o_bgr = take(mem == FL_MEM_HOST && bgr ? (size_t)cv * px * 3 : 0), o_dep = take(mem == FL_MEM_HOST && depth ? (size_t)cv * px * 2 : 0),
               o_msk = take(mem == FL_MEM_HOST && mask ? (size_t)cv * px : 0), o_idx = take(mem == FL_MEM_HOST && tri ? (size_t)cv * px * 4 : 0);
  void *sv = nullptr;
  rc = fl_scratch(ctx, off, &sv);
  if (rc) return rc;
  uint8_t *s = (uint8_t *)sv;
  FL_HIP(ctx, hipMemcpyAsync(s + o_vtx, vertices, nv3 * 4, hipMemcpyHostToDevice, ctx->stream));
  if (normals) FL_HIP(ctx, hipMemcpyAsync(s + o_nrm, normals, nv3 * 4, hipMemcpyHostToDevice, ctx->stream));
  if (colors) FL_HIP(ctx, hipMemcpyAsync(s + o_col, colors, nv3, hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(s + o_tri, triangles, nt3 * 4, hipMemcpyHostToDevice, ctx->stream));

  const FlRenderMesh mesh = {(const float *)(s + o_vtx), normals ? (const float *)(s + o_nrm) : nullptr, colors ? s + o_col : nullptr,
                             (const int32_t *)(s + o_tri), n_triangles};
  const float lu[3] = {light[0] / ll, light[1] / ll, light[2] / ll};
  unsigned long long *keys = (unsigned long long *)(s + o_keys);
  const bool host = mem == FL_MEM_HOST;
  for (int v0 = 0; v0 < n_views; v0 += cv) {
    const int n = std::min(cv, n_views - v0);
    const size_t cpx = (size_t)n * px, g0 = (size_t)v0 * px;
    // the pose upload reuses the chunk's slot: stream-ordered behind the previous chunk's kernels
    FL_HIP(ctx, hipMemcpyAsync(s + o_pose, poses13 + (size_t)13 * v0, (size_t)n * 13 * 4, hipMemcpyHostToDevice, ctx->stream));
    uint8_t *ob = bgr ? (host ? s + o_bgr : bgr + 3 * g0) : nullptr;
    uint16_t *od = depth ? (host ? (uint16_t *)(s + o_dep) : depth + g0) : nullptr;
    uint8_t *om = mask ? (host ? s + o_msk : mask + g0) : nullptr;
    int32_t *ot = tri ? (host ? (int32_t *)(s + o_idx) : tri + g0) : nullptr;
    if ((rc = fl_launch_render_chunk(ctx, mesh, (const float *)(s + o_pose), n, w, h, fx, fy, cx, cy, lu, ambient, keys, ob, od, om, ot))) return rc;
    if (host) {
      if (bgr) FL_HIP(ctx, hipMemcpyAsync(bgr + 3 * g0, ob, cpx * 3, hipMemcpyDeviceToHost, ctx->stream));
      if (depth) FL_HIP(ctx, hipMemcpyAsync(depth + g0, od, cpx * 2, hipMemcpyDeviceToHost, ctx->stream));
      if (mask) FL_HIP(ctx, hipMemcpyAsync(mask + g0, om, cpx, hipMemcpyDeviceToHost, ctx->stream));
      if (tri) FL_HIP(ctx, hipMemcpyAsync(tri + g0, ot, cpx * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  if (host) FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

// ---- view sphere (host only) -------------------------------------------------------------------------------------
namespace {
struct D3 { double x, y, z; };
D3 d3_unit(D3 a) { const double l = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z); return D3{a.x / l, a.y / l, a.z / l}; }
D3 d3_cross(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// Icosahedron with vertices at the poles (0, 0, +-1) and two rings of five at z = +-1/sqrt(5), subdivided by edge
// midpoints pushed onto the unit sphere.  Points: the 12 corners, then each level's midpoints in the order they appear.
std::vector<D3> icosphere_points(int subdivisions)
{
  std::vector<D3> p;
  const double zr = 1.0 / std::sqrt(5.0), rr = 2.0 / std::sqrt(5.0), pi = 3.14159265358979323846;
  p.push_back(D3{0, 0, 1});
  for (int k = 0; k < 5; ++k) p.push_back(D3{rr * std::cos(2 * pi * k / 5), rr * std::sin(2 * pi * k / 5), zr});
  for (int k = 0; k < 5; ++k) p.push_back(D3{rr * std::cos(2 * pi * (k + 0.5) / 5), rr * std::sin(2 * pi * (k + 0.5) / 5), -zr});
  p.push_back(D3{0, 0, -1});
  std::vector<int> f;
  for (int k = 0; k < 5; ++k) {
    const int a = 1 + k, b = 1 + (k + 1) % 5, c = 6 + k, d = 6 + (k + 1) % 5;
    const int tri[4][3] = {{0, a, b}, {a, c, b}, {b, c, d}, {11, d, c}};
    for (auto &t : tri) f.insert(f.end(), t, t + 3);
  }
  for (int s = 0; s < subdivisions; ++s) {
    std::vector<int> nf;
    std::map<long long, int> mid;                                // edge (lower, higher index) -> its midpoint
    auto midpoint = [&](int i, int j) {
      const long long key = ((long long)std::min(i, j) << 32) | std::max(i, j);
      auto it = mid.find(key);
      if (it != mid.end()) return it->second;
      p.push_back(d3_unit(D3{(p[i].x + p[j].x) / 2, (p[i].y + p[j].y) / 2, (p[i].z + p[j].z) / 2}));
      mid.emplace(key, (int)p.size() - 1);
      return (int)p.size() - 1;
    };
    for (size_t t = 0; t < f.size(); t += 3) {
      const int a = f[t], b = f[t + 1], c = f[t + 2];
      const int ab = midpoint(a, b), bc = midpoint(b, c), ca = midpoint(c, a);
      const int sub[4][3] = {{a, ab, ca}, {ab, b, bc}, {ca, bc, c}, {ab, bc, ca}};
      for (auto &q : sub) nf.insert(nf.end(), q, q + 3);
    }
    f.swap(nf);
  }
  return p;
}
}  // namespace

extern "C" int fl_view_sphere(int subdivisions, int upper_hemisphere, const float *distances_mm, int n_distances, int n_inplane,
                              float inplane_deg, float *poses13, int cap, int *n_views)
{
  if (subdivisions < 0 || subdivisions > 6 || !distances_mm || n_distances < 1 || n_inplane < 1 || !n_views || cap < 0 ||
      (cap > 0 && !poses13) || !std::isfinite(inplane_deg) || inplane_deg < 0.f || inplane_deg > 180.f)
    return FL_ERR_INVALID;
  for (int i = 0; i < n_distances; ++i)
    if (!std::isfinite(distances_mm[i]) || !(distances_mm[i] > 0.f)) return FL_ERR_INVALID;
  std::vector<D3> pts = icosphere_points(subdivisions);
  if (upper_hemisphere) pts.erase(std::remove_if(pts.begin(), pts.end(), [](const D3 &q) { return q.z < 0.0; }), pts.end());
  const long long total = (long long)pts.size() * n_distances * n_inplane;
  if (total > 0x7fffffffLL) return FL_ERR_INVALID;
  if (cap > 0 && cap < total) return FL_ERR_INVALID;
  if (cap > 0) {
    const double pi = 3.14159265358979323846;
    size_t o = 0;
    for (const D3 &sp : pts) {
      // camera z = -s (towards the object origin); image-up (camera -y) = object +z projected on the image plane, or
      // object +y where +z is within 1e-5 of the optical axis (|s.z| > 1 - 1e-5: the poles)
      const D3 z = D3{-sp.x, -sp.y, -sp.z};
      const D3 up = std::fabs(sp.z) > 1.0 - 1e-5 ? D3{0, 1, 0} : D3{0, 0, 1};
      const double uz = up.x * z.x + up.y * z.y + up.z * z.z;
      const D3 y = d3_unit(D3{-(up.x - uz * z.x), -(up.y - uz * z.y), -(up.z - uz * z.z)});
      const D3 x = d3_cross(y, z);
      for (int di = 0; di < n_distances; ++di) {
        for (int k = 0; k < n_inplane; ++k) {
          const double deg = n_inplane == 1 ? 0.0 : -(double)inplane_deg + 2.0 * inplane_deg * k / (n_inplane - 1);
          const double c = std::cos(deg * pi / 180.0), sn = std::sin(deg * pi / 180.0);
          // R = Rz(angle) * [x; y; z]: a rotation about the optical axis
          const D3 r0{c * x.x - sn * y.x, c * x.y - sn * y.y, c * x.z - sn * y.z};
          const D3 r1{sn * x.x + c * y.x, sn * x.y + c * y.y, sn * x.z + c * y.z};
          const D3 rows[3] = {r0, r1, z};
          float *q = poses13 + 13 * o++;
          for (int r = 0; r < 3; ++r) {
            q[4 * r] = (float)rows[r].x;
            q[4 * r + 1] = (float)rows[r].y;
            q[4 * r + 2] = (float)rows[r].z;
            q[4 * r + 3] = 0.f;
          }
          q[11] = distances_mm[di];
          q[12] = distances_mm[di];
        }
      }
    }
  }
  *n_views = (int)total;
  return FL_OK;
}
