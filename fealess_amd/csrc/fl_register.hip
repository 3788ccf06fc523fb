// fl_register.hip -- depth registration: raw sensor depth frames re-expressed in the colour camera, batched, in HBM
// (fl_register_depth_batch).  The reference leaves this step to librealsense -- rs2::align(RS2_STREAM_COLOR) on every
// frameset in front of Recognition (test/linemod_recon.cpp:38-51, test/linemod_acq.cpp:24-42) -- so there is no reference
// arithmetic to restate; the contract below is this library's own and tests/register_model.py restates it in numpy.
//
// Contract (include/fealess_hip.h says the same).  K_depth->width x height is the size of every input frame (wd x hd),
// K_color->width x height of every output frame (wc x hc); depth is u16 millimetres, 0 = no measurement, in and out.
// X_colour = R * X_depth + t in mm, R row-major.  Lens distortion is out of scope, as for fl_intrinsics everywhere.
// Everything is float32, one IEEE operation per operator (-ffp-contract=off; '/' is correctly rounded on gfx950), in
// exactly this order, so that the float32 restatement matches bit for bit.
//   host      fx_d = (float)K_depth->fx and so on for the other intrinsics of both cameras; ifx = 1.0f / fx_d, ify = 1.0f / fy_d
//   points    a depth pixel (u, v) with d == 0 contributes nothing.  Otherwise z = (float)d and three points are formed,
//             A, B and C for o = -0.5f, +0.5f, 0 (the same o on both axes):
//               x = (((float)u + o) - cx_d) * ifx * z,  y = (((float)v + o) - cy_d) * ify * z
//               X = ((R[0]*x + R[1]*y) + R[2]*z) + t[0];  Y: row 1 and t[1];  Z: row 2 and t[2]
//   reject    the pixel is skipped unless Z_A > 0, Z_B > 0 and Z_C >= 0.5f
//   value     val = (uint16)fminf(rintf(Z_C), 65535.f): the transformed depth, not the source depth
//   footprint p = X / Z * fx_c + cx_c, q = Y / Z * fy_c + cy_c for A and B; skipped if any of the four is not finite
//             x0 = ceilf(fminf(pA, pB)), x1 = floorf(fmaxf(pA, pB)), y0 and y1 likewise from q; each clamped in float to
//             [-1, wc] ([-1, hc] for y) -- fminf(fmaxf(., -1), wc) -- and then converted to int;
//             x0 = max(x0, 0), x1 = min(x1, wc - 1, x0 + FL_REGISTER_MAX_SPLAT - 1), y the same; an empty range writes
//             nothing.  Equal cameras and identity extrinsics: the footprint is the pixel itself, output == input.
//   z-buffer  every output pixel of a footprint takes the minimum of the values that land on it; a pixel nothing lands
//             on is 0.  The minimum does not depend on an order, so the result does not depend on the schedule.
//   cracks    fill_cracks = 1, evaluated on the unfilled image E, never on filled values.  A pixel with E == 0 whose left
//             and right neighbours both exist and are non-zero takes their minimum; otherwise, if its upper and lower
//             neighbours both exist and are non-zero, it takes their minimum; otherwise it stays 0.
// Schedule: a chunk of frames (fl_register_chunk_frames) is one clear of its 32-bit z-buffer to 0xFFFFFFFF, one
// k_register_splat and one k_register_resolve, the frame in blockIdx.y.  The frames' addresses travel in the kernel
// arguments, so nothing but pixels is copied.  k_register_resolve does not write the empty value back in place: a pixel's
// crack fill reads its four neighbours, which other threads own, and a write-back would race with those reads (the result
// would depend on the schedule).  The clear moves the same 4 bytes per pixel a write-back would, and the context's scratch
// is shared with every other entry point, so the z-buffer has to be cleared at the start of a call anyway.
#include "fl_internal.h"
#include <algorithm>

namespace {

constexpr int RG_BLOCK = 256;
constexpr int RG_PX = 8;                        // pixels per thread: one 16-byte load / store of u16
constexpr uint32_t RG_EMPTY = 0xFFFFFFFFu;

struct RegisterArgs {
  int wd, hd, wc, hc;
  float cx_d, cy_d, ifx, ify;                   // depth camera: principal point, 1 / focal lengths
  float fx_c, fy_c, cx_c, cy_c;                 // colour camera
  float R[9], t[3];
  int fill;
  unsigned zstride;                             // z-buffer entries per frame: wc * hc rounded up to RG_PX
};
struct RegisterFrames {                         // the chunk's frames, by value in the kernel arguments
  const uint16_t *in[FL_REGISTER_CHUNK_FRAMES];
  uint16_t *out[FL_REGISTER_CHUNK_FRAMES];
};

// point o of pixel (u, v) at depth z, in the colour camera
__device__ inline void rg_point(const RegisterArgs &a, int u, int v, float o, float z, float &X, float &Y, float &Z)
{
  const float x = (((float)u + o) - a.cx_d) * a.ifx * z;
  const float y = (((float)v + o) - a.cy_d) * a.ify * z;
  X = ((a.R[0] * x + a.R[1] * y) + a.R[2] * z) + a.t[0];
  Y = ((a.R[3] * x + a.R[4] * y) + a.R[5] * z) + a.t[1];
  Z = ((a.R[6] * x + a.R[7] * y) + a.R[8] * z) + a.t[2];
}

// lower and upper end of a footprint along one axis of n pixels: [lo, hi], empty when hi < lo
__device__ inline void rg_range(float a, float b, int n, int &lo, int &hi)
{
  const float fn = (float)n;
  lo = (int)fminf(fmaxf(ceilf(fminf(a, b)), -1.f), fn);
  hi = (int)fminf(fmaxf(floorf(fmaxf(a, b)), -1.f), fn);
  lo = max(lo, 0);
  hi = min(hi, min(n - 1, lo + FL_REGISTER_MAX_SPLAT - 1));
}

__device__ inline void rg_splat(const RegisterArgs &a, uint32_t *zb, int u, int v, unsigned d)
{
  if (d == 0) return;
  const float z = (float)d;
  float XA, YA, ZA, XB, YB, ZB, XC, YC, ZC;
  rg_point(a, u, v, -0.5f, z, XA, YA, ZA);
  rg_point(a, u, v, 0.5f, z, XB, YB, ZB);
  rg_point(a, u, v, 0.f, z, XC, YC, ZC);
  if (!(ZA > 0.f && ZB > 0.f && ZC >= 0.5f)) return;
  const uint32_t val = (uint32_t)(uint16_t)fminf(rintf(ZC), 65535.f);
  const float pA = XA / ZA * a.fx_c + a.cx_c, qA = YA / ZA * a.fy_c + a.cy_c;
  const float pB = XB / ZB * a.fx_c + a.cx_c, qB = YB / ZB * a.fy_c + a.cy_c;
  if (!(isfinite(pA) && isfinite(qA) && isfinite(pB) && isfinite(qB))) return;
  int x0, x1, y0, y1;
  rg_range(pA, pB, a.wc, x0, x1);
  rg_range(qA, qB, a.hc, y0, y1);
  for (int y = y0; y <= y1; ++y)                // 0 <= y < hc and 0 <= x < wc by rg_range
    for (int x = x0; x <= x1; ++x) atomicMin(zb + (size_t)y * a.wc + x, val);
}

// One thread per RG_PX consecutive pixels of a depth frame (rows back to back), the frame in blockIdx.y.
__global__ __launch_bounds__(RG_BLOCK) void k_register_splat(RegisterArgs a, RegisterFrames f, uint32_t *zbuf)
{
  const unsigned npx = (unsigned)a.wd * (unsigned)a.hd;              // <= FL_RENDER_MAX_DIM^2 = 2^26
  const unsigned base = (blockIdx.x * RG_BLOCK + threadIdx.x) * RG_PX;
  if (base >= npx) return;
  const uint16_t *src = f.in[blockIdx.y];
  uint32_t *zb = zbuf + (size_t)blockIdx.y * a.zstride;
  const unsigned n = min((unsigned)RG_PX, npx - base);
  unsigned d[RG_PX];
  if (n == RG_PX && (((uintptr_t)src) & 15) == 0) {                  // base * 2 is a multiple of 16
    const uint4 q = *reinterpret_cast<const uint4 *>(src + base);
    d[0] = q.x & 0xffffu; d[1] = q.x >> 16; d[2] = q.y & 0xffffu; d[3] = q.y >> 16;
    d[4] = q.z & 0xffffu; d[5] = q.z >> 16; d[6] = q.w & 0xffffu; d[7] = q.w >> 16;
  } else {                                                           // the frame's tail, or a frame at an odd address
    for (unsigned j = 0; j < RG_PX; ++j) d[j] = j < n ? src[base + j] : 0u;
  }
  int v = (int)(base / (unsigned)a.wd), u = (int)(base - (unsigned)v * (unsigned)a.wd);
  for (unsigned j = 0; j < n; ++j) {
    rg_splat(a, zb, u, v, d[j]);
    if (++u == a.wd) { u = 0; ++v; }
  }
}

__device__ inline uint32_t rg_e(uint32_t key) { return key == RG_EMPTY ? 0u : key; }   // the unfilled image E

// One thread per RG_PX consecutive pixels of a colour-camera frame, the frame in blockIdx.y.
__global__ __launch_bounds__(RG_BLOCK) void k_register_resolve(RegisterArgs a, RegisterFrames f, const uint32_t *zbuf)
{
  const unsigned npx = (unsigned)a.wc * (unsigned)a.hc;
  const unsigned base = (blockIdx.x * RG_BLOCK + threadIdx.x) * RG_PX;
  if (base >= npx) return;
  const uint32_t *zb = zbuf + (size_t)blockIdx.y * a.zstride;
  uint16_t *dst = f.out[blockIdx.y];
  const unsigned n = min((unsigned)RG_PX, npx - base);
  // the frame's z-buffer is zstride entries, a multiple of RG_PX, at a 32-byte aligned address: these two loads stay inside it
  const uint4 lo = *reinterpret_cast<const uint4 *>(zb + base), hi = *reinterpret_cast<const uint4 *>(zb + base + 4);
  uint32_t e[RG_PX] = {rg_e(lo.x), rg_e(lo.y), rg_e(lo.z), rg_e(lo.w), rg_e(hi.x), rg_e(hi.y), rg_e(hi.z), rg_e(hi.w)};
  uint32_t o[RG_PX];
  int y = (int)(base / (unsigned)a.wc), x = (int)(base - (unsigned)y * (unsigned)a.wc);
  for (unsigned j = 0; j < RG_PX; ++j) {
    o[j] = e[j];
    if (j < n && a.fill && e[j] == 0u) {
      const unsigned p = base + j;
      uint32_t l = 0u, r = 0u;                  // a neighbour that does not exist counts as 0
      if (x > 0) l = j > 0 ? e[j - 1] : rg_e(zb[p - 1]);
      if (x < a.wc - 1) r = j < RG_PX - 1 ? e[j + 1] : rg_e(zb[p + 1]);   // p + 1 < npx: the row goes on
      if (l != 0u && r != 0u) {
        o[j] = min(l, r);
      } else if (y > 0 && y < a.hc - 1) {
        const uint32_t up = rg_e(zb[p - (unsigned)a.wc]), dn = rg_e(zb[p + (unsigned)a.wc]);
        if (up != 0u && dn != 0u) o[j] = min(up, dn);
      }
    }
    if (++x == a.wc) { x = 0; ++y; }
  }
  if (n == RG_PX && (((uintptr_t)dst) & 15) == 0) {
    uint4 q;
    q.x = o[0] | (o[1] << 16); q.y = o[2] | (o[3] << 16); q.z = o[4] | (o[5] << 16); q.w = o[6] | (o[7] << 16);
    *reinterpret_cast<uint4 *>(dst + base) = q;
  } else {
    for (unsigned j = 0; j < n; ++j) dst[base + j] = (uint16_t)o[j];
  }
}

bool intrinsics_ok(const fl_intrinsics *K)
{
  if (K->width < 1 || K->height < 1 || K->width > FL_RENDER_MAX_DIM || K->height > FL_RENDER_MAX_DIM) return false;
  const float fx = (float)K->fx, fy = (float)K->fy, cx = (float)K->cx, cy = (float)K->cy;
  return std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy) && K->fx > 0.0 && K->fy > 0.0 &&
         std::isfinite(fx) && fx > 0.f && std::isfinite(fy) && fy > 0.f && std::isfinite(cx) && std::isfinite(cy);
}

// a rotation: every element of R^T R - I within 1e-3, det > 0 (fp64 on the float entries)
bool rotation_ok(const float *R)
{
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += (double)R[3 * k + i] * (double)R[3 * k + j];
      if (!(std::fabs(s - (i == j ? 1.0 : 0.0)) <= 1e-3)) return false;
    }
  const double det = (double)R[0] * ((double)R[4] * R[8] - (double)R[5] * R[7]) - (double)R[1] * ((double)R[3] * R[8] - (double)R[5] * R[6]) +
                     (double)R[2] * ((double)R[3] * R[7] - (double)R[4] * R[6]);
  return det > 0.0;
}

}  // namespace

// frames per chunk: FL_REGISTER_CHUNK_FRAMES, fewer when the pixels of either camera's frames would pass FL_RENDER_CHUNK_PIXELS
int fl_register_chunk_frames(int wd, int hd, int wc, int hc)
{
  const long long px = std::max((long long)wd * hd, (long long)wc * hc);
  return (int)std::max(1LL, std::min((long long)FL_REGISTER_CHUNK_FRAMES, (long long)FL_RENDER_CHUNK_PIXELS / px));
}

// what fl_register_depth_batch refuses of its cameras, extrinsics and parameters; *what (may be null): the text for fl_set_error
static int register_check(const fl_intrinsics *K_depth, const fl_intrinsics *K_color, const fl_extrinsics *ext, const fl_register_params *params,
                          const char **what)
{
  const char *w = nullptr;
  if ((K_depth && !intrinsics_ok(K_depth)) || (K_color && !intrinsics_ok(K_color))) w = "sizes must be 1..FL_RENDER_MAX_DIM, fx, fy finite and > 0, cx, cy finite";
  else if (ext && (!fl_finite_all(ext->R, 9) || !fl_finite_all(ext->t, 3) || !rotation_ok(ext->R)))
    w = "R must be a rotation (R^T R = I within 1e-3, det > 0), R and t finite";
  else if (params && params->fill_cracks != 0 && params->fill_cracks != 1) w = "fill_cracks must be 0 or 1";
  if (what) *what = w;
  return w ? FL_ERR_INVALID : FL_OK;
}

extern "C" int fl_register_check(const fl_intrinsics *K_depth, const fl_intrinsics *K_color, const fl_extrinsics *depth_to_color,
                                 const fl_register_params *params)
{
  return register_check(K_depth, K_color, depth_to_color, params, nullptr);
}

extern "C" int fl_register_depth_batch(fl_context *ctx, int n_frames, const uint16_t *const *depth, int mem, const fl_intrinsics *K_depth,
                                       const fl_intrinsics *K_color, const fl_extrinsics *depth_to_color, const fl_register_params *params,
                                       uint16_t *const *out)
{
  if (!ctx) return FL_ERR_INVALID;
  if (!depth || !out || !K_depth || !K_color || !depth_to_color || n_frames < 1)
    return fl_set_error(ctx, FL_ERR_INVALID, "fl_register_depth_batch: null argument or n_frames < 1");
  if (mem != FL_MEM_HOST && mem != FL_MEM_DEVICE) return fl_set_error(ctx, FL_ERR_INVALID, "fl_register_depth_batch: bad mem %d", mem);
  for (int i = 0; i < n_frames; ++i)
    if (!depth[i] || !out[i]) return fl_set_error(ctx, FL_ERR_INVALID, "fl_register_depth_batch: frame %d is null", i);
  const char *what = nullptr;
  if (register_check(K_depth, K_color, depth_to_color, params, &what)) return fl_set_error(ctx, FL_ERR_INVALID, "fl_register_depth_batch: %s", what);
  const int fill = params ? params->fill_cracks : 1;
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "fl_register_depth_batch: the context has no device");

  RegisterArgs a;
  a.wd = K_depth->width; a.hd = K_depth->height; a.wc = K_color->width; a.hc = K_color->height;
  a.cx_d = (float)K_depth->cx; a.cy_d = (float)K_depth->cy;
  a.ifx = 1.0f / (float)K_depth->fx; a.ify = 1.0f / (float)K_depth->fy;
  a.fx_c = (float)K_color->fx; a.fy_c = (float)K_color->fy; a.cx_c = (float)K_color->cx; a.cy_c = (float)K_color->cy;
  for (int i = 0; i < 9; ++i) a.R[i] = depth_to_color->R[i];
  for (int i = 0; i < 3; ++i) a.t[i] = depth_to_color->t[i];
  a.fill = fill;
  const size_t px_d = (size_t)a.wd * a.hd, px_c = (size_t)a.wc * a.hc;
  a.zstride = (unsigned)fl_align(px_c, RG_PX);

  FL_HIP(ctx, hipSetDevice(ctx->device));
  const int cf = fl_register_chunk_frames(a.wd, a.hd, a.wc, a.hc);
  const bool host = mem == FL_MEM_HOST;
  // scratch, sized by the chunk and not by n_frames: z-buffer | (host frames) input staging | output staging
  const size_t in_stride = fl_align(px_d * 2, 256), out_stride = fl_align(px_c * 2, 256);
  const size_t o_z = 0, o_in = fl_align((size_t)cf * a.zstride * 4, 256), o_out = o_in + (host ? (size_t)cf * in_stride : 0),
               total = o_out + (host ? (size_t)cf * out_stride : 0);
  void *sv = nullptr;
  if (int rc = fl_scratch(ctx, total, &sv)) return rc;
  uint8_t *s = (uint8_t *)sv;
  uint32_t *zbuf = (uint32_t *)(s + o_z);
  const unsigned gx_d = (unsigned)((px_d + (size_t)RG_BLOCK * RG_PX - 1) / ((size_t)RG_BLOCK * RG_PX));
  const unsigned gx_c = (unsigned)((px_c + (size_t)RG_BLOCK * RG_PX - 1) / ((size_t)RG_BLOCK * RG_PX));
  for (int f0 = 0; f0 < n_frames; f0 += cf) {
    const int n = std::min(cf, n_frames - f0);
    RegisterFrames fr = {};
    for (int i = 0; i < n; ++i) {
      if (host) {
        FL_HIP(ctx, hipMemcpyAsync(s + o_in + (size_t)i * in_stride, depth[f0 + i], px_d * 2, hipMemcpyHostToDevice, ctx->stream));
        fr.in[i] = (const uint16_t *)(s + o_in + (size_t)i * in_stride);
        fr.out[i] = (uint16_t *)(s + o_out + (size_t)i * out_stride);
      } else {
        fr.in[i] = depth[f0 + i];
        fr.out[i] = out[f0 + i];
      }
    }
    FL_HIP(ctx, hipMemsetAsync(zbuf, 0xFF, (size_t)n * a.zstride * 4, ctx->stream));
    hipLaunchKernelGGL(k_register_splat, dim3(gx_d, n), dim3(RG_BLOCK), 0, ctx->stream, a, fr, zbuf);
    FL_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_register_resolve, dim3(gx_c, n), dim3(RG_BLOCK), 0, ctx->stream, a, fr, (const uint32_t *)zbuf);
    FL_HIP(ctx, hipGetLastError());
    if (host)
      for (int i = 0; i < n; ++i)
        FL_HIP(ctx, hipMemcpyAsync(out[f0 + i], s + o_out + (size_t)i * out_stride, px_c * 2, hipMemcpyDeviceToHost, ctx->stream));
  }
  if (host) FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}
