// fl_icp_search.h -- the nearest-neighbour searches of fl_icp.hip: a part of that file, included by it alone (behind its constants and
// uniform_f / cvt_i32_sat), split off so that a search step can be read and changed without icp_run around it.  An organised search
// reads what its OrgSearchCtx names and S (its wave's stage in the chain tiles, S.a1_next, S.stop) and hands what it finds to `found`.
//
// Nearest neighbours: the reference's FLANN kd-tree (exact 1-NN, eps 0) is replaced by a uniform x/y cell grid over the static
// reference cloud built once per frame; a query only visits the cells within sqrt(3*dist_mean) because farther neighbours are
// discarded anyway (PointsCorresponding keeps d^2 <= 3*dist_mean, ICP.cpp:268,708).  Distances use L2_Simple's float expression
// ((dx*dx + dy*dy) + dz*dz); ties go to the lowest index.
//
// Organised search (the recognition / detection() pipeline, where both clouds are back-projected crops).  The grid, its
// CSR headers and their gathers are not needed there: the reference cloud is kept as an IMAGE (crop pixel -> 12-byte point,
// a point at infinity where the pixel was dropped; a point is named by its pixel), and the reference points within distance r of a query
// q can only come from the pixels its ball projects to -- u in [fx (qx -+ r) / (qz +- r)], likewise v -- a window of a
// few pixels.  Queries are taken in 16x4-pixel tile order (a permutation built once per frame), so the 64 queries of a
// wave share a compact union window; the wave stages that window into its share of the (idle) chain tiles in LDS with a
// handful of coalesced loads and every lane enumerates its own window from LDS.  When the union does not fit (the first
// iterations, where sqrt(3 dist_mean) is several pixels) the same enumeration reads the image from L2 instead.
// fl_icp() (caller-supplied clouds, no image structure) keeps the grid search.
#pragma once

// uniform base + 32-bit unsigned byte offset: one VGPR per address (global_load ... v_off, s[base]) instead of a
// sign-extended 64-bit pointer pair -- the search keeps 24 addresses in flight
template <typename T>
__device__ __forceinline__ T ld_u32(const T *__restrict__ base, int idx)
{
  return *(const T *)((const char *)base + (size_t)((unsigned)idx * (unsigned)sizeof(T)));
}

// one 12-byte load (global_load_dwordx3) for a point instead of three dword loads: the phases are bound by the
// number of vector-memory instructions as much as by anything else
struct F3 { float x, y, z; };
__device__ __forceinline__ F3 ld3_u32(const float *__restrict__ base, int i)
{
  F3 v;
  unsigned i3;                                           // 12 i as (2 i + i) << 2: the compiler folds the C form back into a quarter-rate v_mul_lo_u32
  asm("v_lshl_add_u32 %0, %1, 1, %1" : "=v"(i3) : "v"(i));
  __builtin_memcpy(&v, (const char *)base + (size_t)(i3 << 2), 12);
  return v;
}

// bnd[] is only ever an UPPER bound (a wider search radius visits more pixels, the neighbour found is the same), so it is kept
// as the top 16 bits of its float32 pattern, rounded UP: 8 of the ~155 bytes the kernel moves per point and iteration.
// Saturating: a finite value rounds up to at most +inf (0x7F80), and ANY NaN payload is stored as the canonical 0x7FC0 -- "no
// bound" -- instead of carrying into the exponent or the sign (0x7FFFxxxx + 0xFFFF would wrap to 0x8000 = a bound of -0).
// bnd values are non-negative by construction (distances and sums of distances).
typedef uint16_t bnd_t;
// (three instructions: every pattern at or above the canonical NaN -- the negative ones included -- is clamped to it first;
// the NaNs below it round up to a NaN no larger than it; FLT_MAX rounds up to +inf)
__host__ __device__ __forceinline__ uint16_t bnd_pack(unsigned bits)
{
  return (uint16_t)(((bits < 0x7FC00000u ? bits : 0x7FC00000u) + 0xFFFFu) >> 16);
}
__device__ __forceinline__ float bnd_ld(const bnd_t *__restrict__ b, int i) { return __uint_as_float((unsigned)ld_u32(b, i) << 16); }
__device__ __forceinline__ void bnd_st(bnd_t *b, int i, float v) { b[i] = bnd_pack(__float_as_uint(v)); }

// A wave's LDS writes handed to its own lanes (the staged rows of a search step, a block of the deferred chain): no workgroup
// barrier, the data never leaves the wave
__device__ __forceinline__ void wave_lds_handover()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// An UPPER bound of sqrt(x) for the search-radius bookkeeping (bnd[]): the hardware's 1-ulp v_sqrt_f32 inflated past
// its error (and past a flushed denormal) instead of the ~15-instruction correctly rounded sqrtf.  Any over-estimate
// only widens the visited area; the nearest neighbour found is the same.
__device__ __forceinline__ float sqrt_upper(float x) { return __builtin_amdgcn_sqrtf(x) * 1.000001f + 1.1e-19f; }

// A searchable reference point is a float4 (index bits, X, Y, Z): the index comes FIRST so that the 64-bit key
// (index low, d2 high) can be formed in the two registers the load put the index and X into -- X is dead once dx is
// computed -- without a register move per candidate.
__device__ __forceinline__ float4 nn_point(float x, float y, float z, int index) { return make_float4(__int_as_float(index), x, y, z); }
#define NN_OVERRUN 3                // readable points behind the last position of a staged window / of the reference image
#define NN_IDX_NONE 0x7fffffff      // index stored with a dropped pixel of the reference image (real indices are below it)

// ---- uniform x/y grid over the reference cloud --------------------------------------------------
__device__ __forceinline__ int cell_of(float v, float vmin, float inv_c, int G)
{
  float t = floorf((v - vmin) * inv_c);
  int c = t < 0.f ? 0 : (t > (float)(G - 1) ? G - 1 : (int)t);
  return c;
}

template <class SH>
__device__ __forceinline__ void build_grid(SH &S, const float *ref, int n_ref, float4 *sref, int *cell_start, int *cell_cur,
                           int ncell_max)
{
  constexpr int BS = SH::BS, NW = SH::NW;
  // bounding box of the finite points
  float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
  for (int i = threadIdx.x; i < n_ref; i += BS) {
    const F3 p3 = ld3_u32(ref, i);
    const float x = p3.x, y = p3.y, z = p3.z;
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
      xmin = fminf(xmin, x);
      xmax = fmaxf(xmax, x);
      ymin = fminf(ymin, y);
      ymax = fmaxf(ymax, y);
    }
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    xmin = fminf(xmin, __shfl_xor(xmin, s, 64));
    xmax = fmaxf(xmax, __shfl_xor(xmax, s, 64));
    ymin = fminf(ymin, __shfl_xor(ymin, s, 64));
    ymax = fmaxf(ymax, __shfl_xor(ymax, s, 64));
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    const int wv = threadIdx.x >> 6;
    S.fred[0][wv] = xmin;
    S.fred[1][wv] = xmax;
    S.fred[2][wv] = ymin;
    S.fred[3][wv] = ymax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < NW; ++i) {
      xmin = fminf(xmin, S.fred[0][i]);
      xmax = fmaxf(xmax, S.fred[1][i]);
      ymin = fminf(ymin, S.fred[2][i]);
      ymax = fmaxf(ymax, S.fred[3][i]);
    }
    if (!(xmax >= xmin)) { xmin = xmax = 0.f; ymin = ymax = 0.f; }
    const float dx = xmax - xmin, dy = ymax - ymin;
    float c = sqrtf((dx * dy) / (float)(n_ref > 0 ? n_ref : 1));   // about one point per cell on a dense surface
    // scale-free guards: a (nearly) collinear cloud gets cells of extent / sqrt(n); coincident points one cell
    const float ext = fmaxf(dx, dy);
    if (!(c > ext * 1e-4f)) c = ext / sqrtf((float)(n_ref > 0 ? n_ref : 1));
    if (!(c > 0.f) || !isfinite(c)) c = 1.0f;
    int GX, GY;
    for (;;) {
      GX = (int)(dx / c) + 1;
      GY = (int)(dy / c) + 1;
      if ((long long)GX * GY <= ncell_max) break;
      c *= 1.5f;
    }
    S.xmin = xmin;
    S.ymin = ymin;
    S.inv_c = 1.0f / c;
    S.GX = GX;
    S.GY = GY;
  }
  __syncthreads();
  const int ncell = S.GX * S.GY;
  for (int i = threadIdx.x; i < ncell; i += BS) cell_cur[i] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n_ref; i += BS) {
    const F3 p3 = ld3_u32(ref, i);
    const float x = p3.x, y = p3.y, z = p3.z;
    if (isfinite(x) && isfinite(y) && isfinite(z))
      atomicAdd(&cell_cur[cell_of(y, S.ymin, S.inv_c, S.GY) * S.GX + cell_of(x, S.xmin, S.inv_c, S.GX)], 1);
  }
  __syncthreads();
  // exclusive scan of the counts -> cell_start (and cell_cur, the scatter cursors): four consecutive cells per thread,
  // a shuffle scan inside the wave, the wave totals through a double-buffered LDS slot -- one barrier per 4*BS cells
  {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int run = 0, step = 0;
    for (int base = 0; base < ncell; base += 4 * BS, ++step) {
      const int i0 = base + 4 * threadIdx.x;
      int c[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = i0 + u < ncell ? cell_cur[i0 + u] : 0;
      const int mine = (c[0] + c[1]) + (c[2] + c[3]);
      int inc = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d, 64);
        if (lane >= d) inc += t;
      }
      int *slot = S.iscan2[step & 1];
      if (lane == 63) slot[wv] = inc;
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) { const int t = slot[w]; before += w < wv ? t : 0; total += t; }
      int ex = run + before + inc - mine;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i0 + u < ncell) { cell_start[i0 + u] = ex; cell_cur[i0 + u] = ex; }
        ex += c[u];
      }
      run += total;
    }
    if (threadIdx.x == 0) { cell_start[ncell] = run; S.nsorted = run; }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_ref; i += BS) {
    const F3 p3 = ld3_u32(ref, i);
    const float x = p3.x, y = p3.y, z = p3.z;
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
      const int slot = atomicAdd(&cell_cur[cell_of(y, S.ymin, S.inv_c, S.GY) * S.GX + cell_of(x, S.xmin, S.inv_c, S.GX)], 1);
      sref[slot] = nn_point(x, y, z, i);
    }
  }
  __syncthreads();
}

// ---- exact nearest neighbours within a window -------------------------------------------------------
// the grid parameters as wave-uniform scalars (SGPRs): read from LDS they would each cost a VGPR in the search loop
struct NnGrid {
  float xmin, ymin, inv_c;
  int GX, GY, nsorted;
};
template <class SH>
__device__ __forceinline__ NnGrid nn_grid(const SH &S)
{
  NnGrid g;
  g.xmin = uniform_f(S.xmin);
  g.ymin = uniform_f(S.ymin);
  g.inv_c = uniform_f(S.inv_c);
  g.GX = __builtin_amdgcn_readfirstlane(S.GX);
  g.GY = __builtin_amdgcn_readfirstlane(S.GY);
  g.nsorted = __builtin_amdgcn_readfirstlane(S.nsorted);
  return g;
}

// the radius every reference point within distance `lim` of the query lies within, inflated past the float rounding of
// d2, of the coordinate differences and of the bound's own arithmetic (orders of magnitude below the relative margins)
__device__ __forceinline__ float nn_radius(float qx, float qy, float qz, float lim)
{
  return lim * 1.0001f + 2e-6f * (fabsf(qx) + fabsf(qy) + fabsf(qz)) + 1e-30f;
}

// (d2, index) packed as d2's bit pattern (non-negative floats order like unsigned integers) in the high word and the
// reference index in the low word: one 64-bit unsigned minimum implements "smaller distance, ties to the lower
// index" exactly.
#define NN_KEY_NONE 0xFFFFFFFFFFFFFFFFull
__device__ __forceinline__ unsigned long long nn_key(float qx, float qy, float qz, const float4 &p)
{
  const float dx = qx - p.y, dy = qy - p.z, dz = qz - p.w;
  float d = dx * dx;                                     // cvflann::L2_Simple<float>
  d += dy * dy;
  d += dz * dz;
  return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(p.x);
}
#define NN_CONSIDER(P) { const unsigned long long key_ = nn_key(qx, qy, qz, (P)); best = key_ < best ? key_ : best; }
// a key whose index is NN_IDX_NONE (a dropped pixel: d2 = inf) or NN_KEY_NONE itself means "nothing found"
#define NN_UNPACK(best, bi, bd)                                            \
  {                                                                        \
    const unsigned lo_ = (unsigned)((best) & 0xFFFFFFFFull);               \
    const bool found_ = lo_ < (unsigned)NN_IDX_NONE;                       \
    *(bi) = found_ ? (int)lo_ : -1;                                        \
    *(bd) = found_ ? __uint_as_float((unsigned)((best) >> 32)) : NAN;      \
  }

// ---- grid search (fl_icp: caller-supplied clouds) -------------------------------------------------------
// exact 1-NN among the points of the cell rows [cy0, cy1] x [cx0, cx1]; the grid and the sorted cloud are L2-resident
__device__ __forceinline__ void nn_search_grid(const NnGrid &S, const float4 *__restrict__ sref,
                                               const int *__restrict__ cell_start, float qx, float qy, float qz, float r,
                                               int *bi, float *bd)
{
  unsigned long long best = NN_KEY_NONE;
  const int last = S.nsorted - 1;
  if (last < 0) { NN_UNPACK(best, bi, bd) return; }
  int cx0 = 0, cx1 = S.GX - 1, cy0 = 0, cy1 = S.GY - 1;
  if (isfinite(r)) {
    cx0 = cell_of(qx - r, S.xmin, S.inv_c, S.GX);
    cx1 = cell_of(qx + r, S.xmin, S.inv_c, S.GX);
    cy0 = cell_of(qy - r, S.ymin, S.inv_c, S.GY);
    cy1 = cell_of(qy + r, S.ymin, S.inv_c, S.GY);
  }
  // The search is latency-bound and a wave pays for its slowest lane, so round trips are what counts:
  // the headers of 4 grid rows (8 loads) are fetched together, then the candidates of all 4 row segments
  // are enumerated as ONE flat list, ICP_NB per round trip -- a lane needs ceil(total / NB) rounds however the
  // candidates are spread over the rows.  Slots past the end of the list are NOT masked: they read points that
  // follow the last row segment (clamped to the cloud), and looking at extra reference points never changes the
  // answer -- the minimum over a superset that still contains every point within the search radius is the same
  // nearest neighbour, ties to the lowest index included.
  for (int cy = cy0; cy <= cy1; cy += 4) {
    int rb[4], re[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int cyu = min(cy + u, cy1);
      rb[u] = ld_u32(cell_start, cyu * S.GX + cx0);      // cells of a row are contiguous
      re[u] = ld_u32(cell_start, cyu * S.GX + cx1 + 1);
    }
#pragma unroll
    for (int u = 1; u < 4; ++u)
      if (cy + u > cy1) re[u] = rb[u];                  // predicated: keeps rb/re in registers
    // flat index k -> slot k + adj[u] for pre[u] <= k < pre[u + 1]
    const int pre1 = re[0] - rb[0], pre2 = pre1 + (re[1] - rb[1]), pre3 = pre2 + (re[2] - rb[2]);
    const int tot = pre3 + (re[3] - rb[3]);
    const int adj0 = rb[0], adj1 = rb[1] - pre1, adj2 = rb[2] - pre2, adj3 = rb[3] - pre3;
    for (int base = 0; base < tot; base += ICP_NB) {
      float4 p[ICP_NB];
#pragma unroll
      for (int v = 0; v < ICP_NB; ++v) {
        const int k = base + v;
        int adj = k >= pre1 ? adj1 : adj0;
        adj = k >= pre2 ? adj2 : adj;
        adj = k >= pre3 ? adj3 : adj;
        p[v] = ld_u32(sref, min(k + adj, last));
      }
#pragma unroll
      for (int v = 0; v < ICP_NB; ++v) NN_CONSIDER(p[v])
    }
  }
  NN_UNPACK(best, bi, bd)
}

// ---- organised search (recognition / detection: the reference cloud is a back-projected crop) ------------
// The reference cloud of the organised search is an IMAGE of 12-byte points (crop pixel p -> X, Y, Z; +inf where the paired
// compaction dropped the pixel) followed by an image of their indices.  The search identifies a reference point by its PIXEL
// (nn[] holds pixel positions there; ties between equal distances go to the lower pixel, which is the lower index: the
// compaction is row-major), so the staged records need no index from memory -- 12 instead of 16 bytes per staged point, of a
// kernel that is bound by the bytes it moves -- and phase A2 gathers the partner from the image instead of from ref[].
// idximg is read once per frame (tile order) and by the point-to-plane mode (normals are stored by index).
__host__ __device__ __forceinline__ size_t org_idximg_offset(int pixels) { return (size_t)12 * (size_t)(pixels + 4); }
struct OrgGeom {
  int cw, ch;            // crop size: rimg[v * cw + u] holds the point of crop pixel (u, v)
  float offu, offv;      // scene pixel of crop pixel (0, 0) minus the principal point
  float fx, fy;
  int sx0, sy0;          // scene pixel of crop pixel (0, 0)
  float cx, cy, inv_fx, inv_fy;   // as crop_clouds uses them: (float)K.cx, 1.0f / (float)K.fx ...
};
// The reference point of crop pixel (u, v) from its depth factor zsf, by crop_clouds' own expression (depth_to_3d.cpp:119,132 +
// scale_mat_vec3f): bit for bit what the 12-byte image holds.  A dropped pixel (zsf = NaN) gives a NaN point, whose distance
// is NaN: its key orders behind every real one.
// (suf, svf): the SCENE pixel as floats, (float)(g.sx0 + u) and (float)(g.sy0 + v)
__device__ __forceinline__ F3 org_point_f(const OrgGeom &g, float suf, float svf, float zsf)
{
  F3 p;
  p.x = (((suf - g.cx) * g.inv_fx) * zsf) * 1000;
  p.y = (((svf - g.cy) * g.inv_fy) * zsf) * 1000;
  p.z = zsf * 1000;
  return p;
}
__device__ __forceinline__ F3 org_point(const OrgGeom &g, int u, int v, float zsf)
{
  return org_point_f(g, (float)(g.sx0 + u), (float)(g.sy0 + v), zsf);
}
// whole-wave maximum of an int by DPP (row_shr 1, 2, 4, 8, row_bcast 15 / 31), returned as a wave-uniform value
#define FL_DPP_RED(OP, IDENT)                                                                                 \
  v = OP(v, __builtin_amdgcn_update_dpp((int)(IDENT), v, 0x111, 0xF, 0xF, false));                            \
  v = OP(v, __builtin_amdgcn_update_dpp((int)(IDENT), v, 0x112, 0xF, 0xF, false));                            \
  v = OP(v, __builtin_amdgcn_update_dpp((int)(IDENT), v, 0x114, 0xF, 0xF, false));                            \
  v = OP(v, __builtin_amdgcn_update_dpp((int)(IDENT), v, 0x118, 0xF, 0xF, false));                            \
  v = OP(v, __builtin_amdgcn_update_dpp((int)(IDENT), v, 0x142, 0xA, 0xF, false));                            \
  v = OP(v, __builtin_amdgcn_update_dpp((int)(IDENT), v, 0x143, 0xC, 0xF, false));                            \
  return __builtin_amdgcn_readlane(v, 63);
__device__ __forceinline__ int wave_max_i(int v) { FL_DPP_RED(max, (int)0x80000000) }

// N whole-wave maxima at once (a minimum is the maximum of the negated values): the DPP steps of the N reductions are
// interleaved, so the wait states a DPP read needs after the VALU write of its source are filled by the other reductions'
// steps instead of s_nop -- six serial reductions cost 6 x (6 + 6 nops + 2) issue slots, five interleaved ones 5 x 7
template <int N>
__device__ __forceinline__ void wave_max_multi(int (&v)[N])
{
#define FL_DPP_STEP(CTRL, RMASK)                                                                                       \
  _Pragma("unroll") for (int k_ = 0; k_ < N; ++k_)                                                                     \
    v[k_] = max(v[k_], __builtin_amdgcn_update_dpp((int)0x80000000, v[k_], CTRL, RMASK, 0xF, false));
  FL_DPP_STEP(0x111, 0xF)
  FL_DPP_STEP(0x112, 0xF)
  FL_DPP_STEP(0x114, 0xF)
  FL_DPP_STEP(0x118, 0xF)
  FL_DPP_STEP(0x142, 0xA)
  FL_DPP_STEP(0x143, 0xC)
#undef FL_DPP_STEP
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = __builtin_amdgcn_readlane(v[k], 63);
}

// Six whole-wave maxima with gfx950's lane-swap instructions: v_permlane32_swap exchanges the upper half of one register with
// the lower half of another, so ONE maximum of the swapped pair folds the two halves of BOTH values (value A's partials now live
// in lanes 0-31, value B's in 32-63); v_permlane16_swap does the same for 16-lane rows.  Four values folded into the four rows
// of one register and two into the halves of another need 4 + 5 DPP steps in all where six separate reductions need 36:
// 19 vector instructions instead of 36 (+ their wait states) per search step.
__device__ __forceinline__ void wave_max6(int (&v)[6])
{
  auto fold32 = [](int a, int b) {                         // lanes 0-31: max over a's halves, lanes 32-63: over b's
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)a, (unsigned)b, false, false);
    return max((int)r[0], (int)r[1]);
  };
  const int m01 = fold32(v[0], v[1]), m23 = fold32(v[2], v[3]);
  int m45 = fold32(v[4], v[5]);
  const auto q = __builtin_amdgcn_permlane16_swap((unsigned)m01, (unsigned)m23, false, false);
  int n = max((int)q[0], (int)q[1]);                        // rows 0..3: v[0], v[2], v[1], v[3] (16 partials each)
#define FL_DPP_STEP2(CTRL)                                                                                             \
  n = max(n, __builtin_amdgcn_update_dpp((int)0x80000000, n, CTRL, 0xF, 0xF, false));                                  \
  m45 = max(m45, __builtin_amdgcn_update_dpp((int)0x80000000, m45, CTRL, 0xF, 0xF, false));
  FL_DPP_STEP2(0x111)
  FL_DPP_STEP2(0x112)
  FL_DPP_STEP2(0x114)
  FL_DPP_STEP2(0x118)
#undef FL_DPP_STEP2
  m45 = max(m45, __builtin_amdgcn_update_dpp((int)0x80000000, m45, 0x142, 0xA, 0xF, false));   // row_bcast:15 into rows 1, 3
  v[0] = __builtin_amdgcn_readlane(n, 15);
  v[2] = __builtin_amdgcn_readlane(n, 31);
  v[1] = __builtin_amdgcn_readlane(n, 47);
  v[3] = __builtin_amdgcn_readlane(n, 63);
  v[4] = __builtin_amdgcn_readlane(m45, 31);
  v[5] = __builtin_amdgcn_readlane(m45, 63);
}
// The crop pixels whose points can lie within distance r of q: a point (X, Y, Z) of pixel (su, sv) satisfies
// su - cx = X fx / Z up to float rounding (it was generated as X = ((su - cx) / fx) Z), and |X - qx|, |Z - qz| <= r.
// The 0.01-pixel slop is an order of magnitude above that rounding (5e-7 relative on |su - cx| <= 2000 pixels).  An empty window has u_lo > u_hi.
// (the constants folded -- cul / cuh = offu +- slop, cvl / cvh = offv +- slop, wave-uniform -- and the clamping left to the
// saturating float -> int conversion; returns whether the window holds a pixel)
// Branch-free form of org_window2 for the pipelined step: every lane computes the projection (a lane whose radius is not finite
// or reaches Z <= 1 computes garbage and selects the whole crop, a lane that is not queryable selects nothing), so that a step
// has no exec-mask regions in front of its reductions.  Same windows.
__device__ __forceinline__ bool org_window2_flat(const OrgGeom &g, float cul, float cuh, float cvl, float cvh, float qx, float qy, float qz, float r,
                                                 bool queryable, int &u_lo, int &u_hi, int &v_lo, int &v_hi)
{
  const float zlo = qz - r, zhi = qz + r;
  const bool narrow = isfinite(r) && zlo > 1.0f;         // otherwise the whole crop (valid points have 0 < Z <= 900)
  const float ilo = __builtin_amdgcn_rcpf(zlo), ihi = __builtin_amdgcn_rcpf(zhi);
  const float xlo = qx - r, xhi = qx + r, ylo = qy - r, yhi = qy + r;
  const int iul = cvt_i32_sat(ceilf((xlo * (xlo < 0.f ? ilo : ihi)) * g.fx - cul));
  const int iuh = cvt_i32_sat(floorf((xhi * (xhi > 0.f ? ilo : ihi)) * g.fx - cuh));
  const int ivl = cvt_i32_sat(ceilf((ylo * (ylo < 0.f ? ilo : ihi)) * g.fy - cvl));
  const int ivh = cvt_i32_sat(floorf((yhi * (yhi > 0.f ? ilo : ihi)) * g.fy - cvh));
  u_lo = narrow ? max(iul, 0) : 0;
  u_hi = narrow ? min(iuh, g.cw - 1) : g.cw - 1;
  v_lo = narrow ? max(ivl, 0) : 0;
  v_hi = narrow ? min(ivh, g.ch - 1) : g.ch - 1;
  return queryable & (u_lo <= u_hi) & (v_lo <= v_hi);
}
__device__ __forceinline__ bool org_window2(const OrgGeom &g, float cul, float cuh, float cvl, float cvh, float qx, float qy, float qz, float r,
                                            int &u_lo, int &u_hi, int &v_lo, int &v_hi)
{
  u_lo = 0; u_hi = g.cw - 1; v_lo = 0; v_hi = g.ch - 1;
  const float zlo = qz - r, zhi = qz + r;
  if (isfinite(r) && zlo > 1.0f) {                       // otherwise the whole crop (valid points have 0 < Z <= 900)
    const float ilo = __builtin_amdgcn_rcpf(zlo), ihi = __builtin_amdgcn_rcpf(zhi);
    const float xlo = qx - r, xhi = qx + r, ylo = qy - r, yhi = qy + r;
    const int iul = cvt_i32_sat(ceilf((xlo * (xlo < 0.f ? ilo : ihi)) * g.fx - cul));
    const int iuh = cvt_i32_sat(floorf((xhi * (xhi > 0.f ? ilo : ihi)) * g.fx - cuh));
    const int ivl = cvt_i32_sat(ceilf((ylo * (ylo < 0.f ? ilo : ihi)) * g.fy - cvl));
    const int ivh = cvt_i32_sat(floorf((yhi * (yhi > 0.f ? ilo : ihi)) * g.fy - cvh));
    u_lo = max(iul, 0);
    u_hi = min(iuh, g.cw - 1);
    v_lo = max(ivl, 0);
    v_hi = min(ivh, g.ch - 1);
  }
  return u_lo <= u_hi && v_lo <= v_hi;
}

// ---- the organised searches: PointsCorresponding (:193-279) for every model point, exact 1-NN within min(bnd[i], r_lim) ----
// What a search reads (built once per icp_run).  The caller's found(active, i, qx, qy, qz, j, d) owns nn[] / nd[] and the stores
// into bnd[]; j = -1 and d = NaN when no reference point lies within the radius.
// IDX: the type perm[] is stored in (int, or uint16_t in the 16-bit builds of the 256-thread parity kernel: ld_u32 zero-extends it)
template <class IDX>
struct OrgSearchCtx {
  const float *mod;                  // the queries, their radius bounds (read only: found() stores them), their tile order
  const bnd_t *bnd;
  const IDX *perm;
  const float *rimg, *zimg;          // the reference image: 12-byte points / depth factors (org_search_pipe only)
  int n_model;
  OrgGeom og;
  int last_s, last_pt;               // derived: last query; last readable position of the image (its overrun guard included)
  float cwf;                         // (float)og.cw
  bool small_crop;                   // every position of the image is below 2^24: exact in float32 (slot_pos)
};
template <class IDX>
__device__ __forceinline__ OrgSearchCtx<IDX> org_search_ctx(const float *mod, const bnd_t *bnd, const IDX *perm, const float *rimg, const float *zimg,
                                                            int n_model, const OrgGeom &og)
{
  return {mod, bnd, perm, rimg, zimg, n_model, og, n_model - 1, og.cw * og.ch + NN_OVERRUN - 1, (float)og.cw,
          (long long)og.cw * og.ch + NN_OVERRUN < (1 << 24)};
}
// where wave wv stages the rows of its step: its share of the chain tiles, which are idle during a search
template <class SH>
__device__ __forceinline__ float4 *org_stage(SH &S, int wv)
{
  static_assert(sizeof(S.prod) + sizeof(S.dtile) + sizeof(S.stage_pad) >= (size_t)SH::NW * ICP_STAGE_CAP * 16, "the chain tiles (idle during the search) hold every wave's staged rows");
  static_assert(offsetof(SH, stage_pad) == offsetof(SH, dtile) + sizeof(S.dtile) && offsetof(SH, dtile) == offsetof(SH, prod) + sizeof(S.prod),
                "prod, dtile and stage_pad are one contiguous region");
  return (float4 *)&S.prod[0][0][0] + wv * ICP_STAGE_CAP;
}
// the searchable point of image position pos, from the 12-byte image
template <class IDX>
__device__ __forceinline__ float4 org_image_point(const OrgSearchCtx<IDX> &c, int pos)
{
  const F3 pt = ld3_u32(c.rimg, pos);
  return nn_point(pt.x, pt.y, pt.z, pt.x == INFINITY ? NN_IDX_NONE : pos);
}

// The L2 fallback, when the union rectangle does not fit the wave's stage (the first iterations, where sqrt(3 dist_mean) is several
// pixels): every lane's window enumerated in lockstep, maxh rows of maxw positions, ICP_NBQ positions per batch (lanes with a
// smaller window re-read their own last column / row: duplicates do not change a minimum), straight from the 12-byte image
template <class IDX>
__device__ __forceinline__ unsigned long long org_scan(const OrgSearchCtx<IDX> &c, float qx, float qy, float qz, int u_lo, int u_hi, int v_lo, int v_hi,
                                                       int maxw, int maxh)
{
  constexpr int NBQ = ICP_NBQ;
  unsigned long long best = NN_KEY_NONE;
  const int wl = u_hi - u_lo, hl = v_hi - v_lo, RS = c.og.cw;
  const int b0 = v_lo * RS + u_lo;
  // A batch is NBQ CONSECUTIVE positions from a clamped start (one address and immediate offsets instead of a clamp and
  // an address per position).  A window narrower than NBQ reads up to NBQ - 1 = NN_OVERRUN positions past its right edge:
  // the next pixels of the row, the start of the next row, or -- behind the last row -- the points at infinity behind the image.
  // All of them are reference points of this frame or points at infinity: looking at more of those never changes the nearest one.
  static_assert(NBQ - 1 <= NN_OVERRUN, "the overrun guard behind the image is NN_OVERRUN points");
  const int wlc = max(wl - (NBQ - 1), 0);
  for (int dv = 0; dv < maxh; ++dv) {
    const int rb = b0 + min(dv, hl) * RS;
    for (int du = 0; du < maxw; du += NBQ) {
      float4 cur[NBQ];
      const int bb = rb + min(du, wlc);
#pragma unroll
      for (int e = 0; e < NBQ; ++e) cur[e] = org_image_point(c, bb + e);
#pragma unroll
      for (int e = 0; e < NBQ; ++e) NN_CONSIDER(cur[e])
    }
  }
  return best;
}

// The scan of a staged rectangle (W points per row, row0: the lane's own first point).  maxh rows -- a lane with fewer
// re-reads its last one -- of batches of consecutive points: a window narrower than its batch reads on into the next points of
// its row, of the next row, or of the slots behind the rectangle.
static_assert(ICP_NBQ == 4 && NN_OVERRUN == 3, "the staged scans are written for batches of at most 4 (wl - 3, area + 3): "
                                                  "build org_scan's ICP_NBQ variants only with them rewritten to match");
// one batch of NC points per row: no lane window is wider than NC
template <int NC>
__device__ __forceinline__ unsigned long long scan_rows(const float4 *row0, int W, int hl, int maxh, float qx, float qy, float qz)
{
  unsigned long long best = NN_KEY_NONE;
  for (int dv = 0; dv < maxh; ++dv) {
    const float4 *bp = row0 + __mul24(min(dv, hl), W);
    float4 cur[NC];
#pragma unroll
    for (int e = 0; e < NC; ++e) cur[e] = bp[e];
#pragma unroll
    for (int e = 0; e < NC; ++e) NN_CONSIDER(cur[e])
  }
  return best;
}
// nbw batches of four per row, the last clamped to the lane's own window (wl = its width - 1)
__device__ __forceinline__ unsigned long long scan_batches(const float4 *row0, int W, int wl, int hl, int maxh, int nbw, float qx, float qy, float qz)
{
  unsigned long long best = NN_KEY_NONE;
  const int wlc = max(wl - 3, 0);
  for (int dv = 0; dv < maxh; ++dv) {
    const float4 *rowp = row0 + __mul24(min(dv, hl), W);
    for (int du = 0; du < 4 * nbw; du += 4) {
      const float4 *bp = rowp + min(du, wlc);
      float4 cur[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) cur[e] = bp[e];
#pragma unroll
      for (int e = 0; e < 4; ++e) NN_CONSIDER(cur[e])
    }
  }
  return best;
}

// ---- org_search: window, staging, scan of one step after the other (every kernel but the 256-thread parity one) ----
// 64 queries of one (or two adjacent) 16x4-pixel tiles per wave and step.  Steps are claimed from a workgroup counter
// (S.a1_next, reset by the caller) where a wave joins late (SPEC), four steps ahead of the one being scanned; otherwise wave w
// takes steps w, w + NW, ...  poll_stop: give up when S.stop is set (SPEC: the chain wave found the loop over).
// Around the distance scan of a step (which is what the step is for: 4 rows x 46 instructions per batch of four
// positions) round 2 spent as many instructions again; what is left of that:
//  * the union rectangle is staged in whole passes of 64 points, as many as it needs (a compile-time count per case), the
//    point of a slot by a reciprocal multiply: no division, no per-pass predicate, no separate guard points (measured:
//    rows padded to 16 / 32 / 64 points need no address arithmetic at all, but nine steps in ten are 14 - 29 pixels wide
//    and would stage twice the points: 26.8 against 25.4 ms per 2560 frames, profiles/README.md);
//  * the five wave reductions (union rectangle, tallest lane window) are interleaved (wave_max_multi), the batches per
//    row come from two ballots;
//  * the window arithmetic has its constants folded and leaves the clamping to the saturating float -> int conversion.
// It stages from the 12-byte image (the 1024-thread kernel: a frame alone on its CU waits for points rebuilt from the 4-byte
// image -- 2.92 against 2.67 ms per 8 frames -- where four workgroups per CU gain from the bytes: 32.9 against 34.2 ms per 4096).
template <class SH, bool SPEC, class IDX, class F>
__device__ __forceinline__ void org_search(SH &S, const OrgSearchCtx<IDX> &c, const float r_lim, const bool poll_stop, F &&found)
{
  const OrgGeom &og = c.og;
  const int n_model = c.n_model;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  float4 *stage = org_stage(S, wv);
  const float cul = uniform_f(og.offu + 0.01f), cuh = uniform_f(og.offu - 0.01f), cvl = uniform_f(og.offv + 0.01f), cvh = uniform_f(og.offv - 0.01f);
  constexpr int stride = SH::NW * 64;
  int static_next = wv * 64 + 4 * stride;
  auto claim = [&](int count) {                          // `count` queries off the workgroup's list (wave-uniform result)
    int v = 0;
    if (lane == 0) v = atomicAdd(&S.a1_next, count);
    return __builtin_amdgcn_readfirstlane(v);
  };
  auto next_step = [&]() {
    if (SPEC) return claim(64);
    const int v = static_next;
    static_next += stride;
    return v;
  };
  const int sdist = SPEC ? 64 : stride;
  int sb0 = SPEC ? claim(256) : wv * 64, sb1 = sb0 + sdist, sb2 = sb0 + 2 * sdist, sb3 = sb0 + 3 * sdist;
  int i_c = ld_u32(c.perm, min(sb0 + lane, c.last_s));
  int i_n = ld_u32(c.perm, min(sb1 + lane, c.last_s));
  int i_nn = ld_u32(c.perm, min(sb2 + lane, c.last_s));
  F3 q_c = ld3_u32(c.mod, i_c), q_n = ld3_u32(c.mod, i_n);
  float b_c = bnd_ld(c.bnd, i_c), b_n = bnd_ld(c.bnd, i_n);
  // A step's results are handed to found() (which stores them) at the head of the NEXT step, in front of that step's
  // staging loads: vmcnt counts loads and stores in one in-order queue, so stores issued at the end of a step were what the
  // wait at the head of the next one waited for (20 % of the phase); issued here, the wait that follows them is the one
  // for the staging loads, which covers them for free.
  bool pend = false, p_active = false;
  int p_i = 0, p_j = -1;
  float p_qx = 0.f, p_qy = 0.f, p_qz = 0.f, p_d = NAN;
  ST_STAMP_BEGIN;
  while (sb0 < n_model) {
    if (poll_stop && *(volatile int *)&S.stop) break;
    const int sb4 = next_step();
    const int i = i_c;
    const float qx = q_c.x, qy = q_c.y, qz = q_c.z;
    ST_ARRIVED(qx, b_c)                                 // the query and its bound
    ST_STAMP(0)
    if (pend) { found(p_active, p_i, p_qx, p_qy, p_qz, p_j, p_d); pend = false; }
    const bool active = sb0 + lane < n_model;
    const bool queryable = active && r_lim >= 0.f && isfinite(qx) && isfinite(qy) && isfinite(qz);
    // ---- this lane's window, the union rectangle, the tallest window ----
    int u_lo = 1, u_hi = 0, v_lo = 1, v_hi = 0;
    bool some = false;
    if (queryable) some = org_window2(og, cul, cuh, cvl, cvh, qx, qy, qz, nn_radius(qx, qy, qz, fminf(b_c, r_lim)), u_lo, u_hi, v_lo, v_hi);   // NaN bnd -> r_lim
    int red[5] = {some ? -u_lo : -0x3fffffff, some ? u_hi : -1, some ? -v_lo : -0x3fffffff, some ? v_hi : -1, some ? v_hi - v_lo + 1 : 0};
    wave_max_multi(red);
    const int U0 = -red[0], U1 = red[1], V0 = -red[2], V1 = red[3], maxh = red[4];
    const bool any = U1 >= U0;                            // wave-uniform: some lane has a window
    ST_STAMP(1)
    const F3 q_nn = ld3_u32(c.mod, i_nn);
    const float b_nn = bnd_ld(c.bnd, i_nn);
    const int i_nnn = ld_u32(c.perm, min(sb3 + lane, c.last_s));
    int j = -1;
    float d = NAN;
    if (any) {
      if (!some) { u_lo = u_hi = U0; v_lo = v_hi = V0; }     // lanes without a window look at one point of the union: a real
                                                           // reference point beyond their radius, which the gate drops
      const int wl = u_hi - u_lo, hl = v_hi - v_lo;
      // 4-wide batches per row of the widest lane window: 1 or 2 by ballot, beyond that by a reduction (first iterations)
      int nbw = 1;
      if (__ballot(wl > 3) != 0ull) nbw = __ballot(wl > 7) == 0ull ? 2 : (wave_max_i(wl) >> 2) + 1;
      const int W = U1 - U0 + 1, H = V1 - V0 + 1, area = W * H;
      // The union rectangle is staged row by row at its own width: LDS slot k = lane + 64 p holds its point (k / W, k % W).
      // Whole passes of 64 slots are staged, enough for the rectangle and the 3 slots a 4-wide batch may run past its last
      // row; slots past the rectangle hold further points of the image (or the points at infinity behind it), which is
      // all a scan may ever look at: a real reference point of this frame or infinity never changes the nearest one.
      const int npneed = (area + 3 + 63) >> 6, npass = npneed <= 2 ? 2 : (npneed <= 4 ? npneed : 6);
      const bool staged = npneed <= 6;
#ifdef FL_ICP_PHASES
      if (lane == 0) {
        atomicAdd((unsigned long long *)&S.tacc[8], 1ull);
        atomicAdd((unsigned long long *)&S.tacc[9], (unsigned long long)(4 * nbw * maxh));
        atomicAdd((unsigned long long *)&S.tacc[10], staged ? 0ull : 1ull);
        atomicAdd((unsigned long long *)&S.tacc[11], (unsigned long long)(staged ? npass * 64 : 0));
        if (S.iter <= 3) atomicAdd((unsigned long long *)&S.tacc[12], (unsigned long long)(4 * nbw * maxh));
        const int wcl = W <= 13 ? 0 : (W <= 29 ? 1 : (W <= 61 ? 2 : 3)), hcl = H <= 5 ? 0 : (H <= 10 ? 1 : (H <= 20 ? 2 : 3));
        atomicAdd(&S.hist[wcl * 4 + hcl], 1u);
        atomicAdd(&S.hist[16 + min(maxh, 6) - 1], 1u);   // (bins 22..24 and 26..28 carry the chain phases' stamps)
      }
#endif
      unsigned long long best;
      if (staged) {
        // k / W by reciprocal: (k + 0.5) / W stays 0.5 / W away from the integers, three orders of magnitude more than the
        // error of v_rcp_f32 and the product (k < 448)
        const float invW = uniform_f(__builtin_amdgcn_rcpf((float)W));
        const int base = (int)__umul24((unsigned)V0, (unsigned)og.cw) + U0;
        auto stage_passes = [&](auto np_) {
          constexpr int NP = decltype(np_)::value;
          float4 R[NP];
#pragma unroll
          for (int p = 0; p < NP; ++p) {
            const int row = (int)(((float)(lane + 64 * p) + 0.5f) * invW), col = lane + 64 * p - row * W;
            R[p] = org_image_point(c, min((int)__umul24((unsigned)row, (unsigned)og.cw) + col + base, c.last_pt));
          }
#pragma unroll
          for (int p = 0; p < NP; ++p) stage[lane + 64 * p] = R[p];
        };
        if (npass == 3) stage_passes(std::integral_constant<int, 3>());
        else if (npass == 4) stage_passes(std::integral_constant<int, 4>());
        else if (npass == 2) stage_passes(std::integral_constant<int, 2>());
        else stage_passes(std::integral_constant<int, 6>());
        wave_lds_handover();
        ST_STAMP(2)
        const float4 *row0 = stage + (v_lo - V0) * W + (u_lo - U0);
        if (nbw == 1) best = scan_rows<4>(row0, W, hl, maxh, qx, qy, qz);
        else best = scan_batches(row0, W, wl, hl, maxh, nbw, qx, qy, qz);
      } else {
        best = org_scan(c, qx, qy, qz, u_lo, u_hi, v_lo, v_hi, 4 * nbw, maxh);
      }
      if (queryable) NN_UNPACK(best, &j, &d)
      ST_ARRIVED(j, d)
      ST_STAMP(3)
    }
    pend = true; p_active = active; p_i = i; p_qx = qx; p_qy = qy; p_qz = qz; p_j = j; p_d = d;
    i_c = i_n; q_c = q_n; b_c = b_n;
    i_n = i_nn; q_n = q_nn; b_n = b_nn;
    i_nn = i_nnn;
    sb0 = sb1; sb1 = sb2; sb2 = sb3; sb3 = sb4;
    ST_STAMP(4)
  }
  if (pend) found(p_active, p_i, p_qx, p_qy, p_qz, p_j, p_d);
  ST_STAMP_END;
}
// (Measured in round 3 and not kept, profiles/r03_README.md: the next step's rectangle fetched by LDS-DMA while this one is
// scanned; the rectangle staged as 2-byte depths with the points rebuilt in registers.)

// ---- org_search_pipe: the same search with the staging one step ahead (256-thread parity kernel) ------------------------
// With the 4-byte image a step's staged data is a handful of dwords per lane, so the NEXT step can be prepared -- its
// windows, its union rectangle, its staging loads issued -- before this step is scanned: the loads' round trip (a third of a
// step) runs underneath the scan instead of in front of it.  Two prepared-step states trade roles by unrolling the loop
// twice (never by moves: see the chain phases).  A state issues its loads in wave-uniform pairs of passes (the
// first version always issued ICP_PIPE_NP, slots past the rectangle reading the guard behind the image, for fear that a branch
// between issue and use would make the compiler drain the queue: it does not -- the wait in front of the first use is
// counted for the shortest path -- and with the column-major tiles seven steps in ten need only two passes).  Same windows,
// same candidates, same keys: bit-identical to org_search.
#define ICP_PIPE_NP 6
// Slot s = lane + 64 p of a staged W-wide rectangle -> its row and column and the crop position base + row * cw + col, in
// float32: every value is an integer below 2^24 (small_crop), so each product, fma and sum is exact, at full rate, where the
// integer forms cost two quarter-rate multiplies per slot (v_mul_lo_u32, v_mad_u64_u32).
struct SlotPos { float row, col, pos; };
__device__ __forceinline__ SlotPos slot_pos(float slotf, float Wf, float invW, float basef, float cwf)
{
  SlotPos r;
  r.row = __builtin_truncf((slotf + 0.5f) * invW);
  r.col = __builtin_fmaf(-r.row, Wf, slotf);
  r.pos = __builtin_fmaf(r.row, cwf, r.col + basef);
  return r;
}
struct Prep {                                // a prepared step
  int i;                                   // the lane's query (model index) and point
  float qx, qy, qz;
  bool active, queryable;
  int u_lo, u_hi, v_lo, v_hi;              // its window (one pixel of the union if it has none)
  int U0, V0, W, maxh, nbw, npass;         // wave-uniform: union rectangle, tallest window, batches per row, passes
  bool w3;                                 // no lane window is wider than 3 pixels: batches of 3 positions
#ifdef FL_ICP_PHASES
  int wlmax;
#endif
  bool any, staged;
  float z[ICP_PIPE_NP];                    // depth factors of the staged slots lane + 64 p (in flight until finish)
};
template <class SH, class IDX, class F>
__device__ __forceinline__ void org_search_pipe(SH &S, const OrgSearchCtx<IDX> &c, const float r_lim, F &&found)
{
  const OrgGeom &og = c.og;
  const int n_model = c.n_model, last_pt = c.last_pt;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  float4 *stage = org_stage(S, wv);
  const float lanef = (float)lane;
  const float cul = uniform_f(og.offu + 0.01f), cuh = uniform_f(og.offu - 0.01f), cvl = uniform_f(og.offv + 0.01f), cvh = uniform_f(og.offv - 0.01f);
  constexpr int stride = SH::NW * 64;
  // windows, union and staging loads of the step whose queries start at sb
  auto prepare = [&](Prep &P, int sb, int i, const F3 &q, float b) {
    P.i = i; P.qx = q.x; P.qy = q.y; P.qz = q.z;
    P.active = sb + lane < n_model;
    P.queryable = P.active && r_lim >= 0.f && isfinite(q.x) && isfinite(q.y) && isfinite(q.z);
    int u_lo, u_hi, v_lo, v_hi;
    const bool some = org_window2_flat(og, cul, cuh, cvl, cvh, q.x, q.y, q.z, nn_radius(q.x, q.y, q.z, fminf(b, r_lim)), P.queryable,
                                       u_lo, u_hi, v_lo, v_hi);
    // union rectangle, tallest and widest lane window (a lane without a window: one pixel of the union, width 0).  A lane
    // without a window contributes the crop's far corners -- neutral among real windows, and a step in which NO lane has one
    // still gets a pixel of the crop as its "union" without a single wave-uniform select (each costs four scalar instructions)
    int red[6] = {some ? -u_lo : 1 - og.cw, some ? u_hi : 0, some ? -v_lo : 1 - og.ch, some ? v_hi : 0, some ? v_hi - v_lo + 1 : 0,
                  some ? u_hi - u_lo : 0};
    wave_max6(red);
    const int U0 = -red[0], U1 = red[1], V0 = -red[2], V1 = red[3];
    P.maxh = red[4];
    P.any = red[4] > 0;                                        // some lane has a window
    if (!some) { u_lo = u_hi = U0; v_lo = v_hi = V0; }
    P.u_lo = u_lo; P.u_hi = u_hi; P.v_lo = v_lo; P.v_hi = v_hi;
    P.nbw = (red[5] >> 2) + 1;                                 // batches of four positions per row: 1 up to width 3, 2 up to 7, ...
    P.w3 = red[5] <= 2;
#ifdef FL_ICP_PHASES
    P.wlmax = red[5];
#endif
    const int W = max(U1 - U0 + 1, 1), H = max(V1 - V0 + 1, 1), area = W * H;
    const int npneed = (area + 3 + 63) >> 6;
    P.npass = npneed <= 2 ? 2 : npneed;
    P.staged = P.any && npneed <= ICP_PIPE_NP && c.small_crop;
    P.U0 = U0; P.V0 = V0; P.W = W;
    const float Wf = (float)W, invW = uniform_f(__builtin_amdgcn_rcpf(Wf));
    const float basef = (float)((int)__umul24((unsigned)P.V0, (unsigned)og.cw) + P.U0);
    // two passes always, the others in pairs where the rectangle needs them (wave-uniform: with the column-major tiles seven
    // steps in ten need two)
    auto ldz = [&](int p) {
      const SlotPos sp = slot_pos(lanef + (float)(64 * p), Wf, invW, basef, c.cwf);
      P.z[p] = ld_u32(c.zimg, P.staged ? min((int)sp.pos, last_pt) : last_pt);
    };
    ldz(0); ldz(1);
    if (P.staged && P.npass > 2) { ldz(2); ldz(3); }
    if (P.staged && P.npass > 4) { ldz(4); ldz(5); }
  };
  // the step itself: rebuild and stage its rectangle, scan, unpack
  auto finish = [&](const Prep &P, int &j, float &d) {
    j = -1; d = NAN;
    if (!P.any) return;
    const float qx = P.qx, qy = P.qy, qz = P.qz;
    const int u_lo = P.u_lo, u_hi = P.u_hi, v_lo = P.v_lo, v_hi = P.v_hi, W = P.W, U0 = P.U0, V0 = P.V0, maxh = P.maxh, nbw = P.nbw;
    const int wl = u_hi - u_lo, hl = v_hi - v_lo;
#ifdef FL_ICP_PHASES
    {                                                    // dev: steps, scanned / staged positions, what the lanes' own windows hold
      int own = P.queryable ? (wl + 1) * (hl + 1) : 0;
      for (int sft = 32; sft >= 1; sft >>= 1) own += __shfl_xor(own, sft, 64);
      if (lane == 0) {
        atomicAdd((unsigned long long *)&S.tacc[8], 1ull);
        atomicAdd((unsigned long long *)&S.tacc[9], (unsigned long long)((P.w3 ? 3 : 4 * nbw) * maxh));
        atomicAdd((unsigned long long *)&S.tacc[10], P.staged ? 0ull : 1ull);
        atomicAdd((unsigned long long *)&S.tacc[11], (unsigned long long)(P.staged ? P.npass * 64 : 0));
        atomicAdd((unsigned long long *)&S.tacc[12], (unsigned long long)own);     // summed over the 64 lanes
        atomicAdd(&S.hist[16 + min(maxh, 6) - 1], 1u);   // (bins 22..24 and 26..28 carry the chain phases' stamps)
        atomicAdd(&S.hist[5 + min(nbw, 3) - 1], 1u);     // bins 5..7: 1, 2, 3+ batches per row
        atomicAdd(&S.hist[8 + min(P.npass, 4) - 2], 1u); // bins 8..10: 2, 3, 4+ staged passes
        atomicAdd(&S.stime[min(P.wlmax, 4)], 1ull);      // widest lane window of the step: 1, 2, 3, 4, 5+ pixels
      }
    }
#endif
    unsigned long long best;
    if (P.staged) {
      const float Wf = (float)W, invW = uniform_f(__builtin_amdgcn_rcpf(Wf));
      const float basef = (float)((int)__umul24((unsigned)V0, (unsigned)og.cw) + U0);
      const float suf = (float)(og.sx0 + U0), svf = (float)(og.sy0 + V0);   // scene pixel of the rectangle's corner
      // 4 bytes per staged point instead of 12: the pixel's depth factor, its point rebuilt by crop_clouds' expression (a slot
      // clamped to the guard behind the image reads NaN whatever its pixel)
      auto put = [&](int p) {
        const SlotPos sp = slot_pos(lanef + (float)(64 * p), Wf, invW, basef, c.cwf);
        const float zf = P.z[p];
        const F3 pt = org_point_f(og, suf + sp.col, svf + sp.row, zf);
        stage[lane + 64 * p] = nn_point(pt.x, pt.y, pt.z, zf != zf ? NN_IDX_NONE : min((int)sp.pos, last_pt));
      };
      put(0); put(1);
      if (P.npass > 2) put(2);
      if (P.npass > 3) put(3);
      if (P.npass > 4) { put(4); put(5); }
      wave_lds_handover();
      const float4 *row0 = stage + __mul24(v_lo - V0, W) + (u_lo - U0);
      if (P.w3) best = scan_rows<3>(row0, W, hl, maxh, qx, qy, qz);      // (nearly half of the steps: a quarter of their scan saved)
      else if (nbw == 1) best = scan_rows<4>(row0, W, hl, maxh, qx, qy, qz);
      else best = scan_batches(row0, W, wl, hl, maxh, nbw, qx, qy, qz);
    } else {
      best = org_scan(c, qx, qy, qz, u_lo, u_hi, v_lo, v_hi, 4 * nbw, maxh);
    }
    if (P.queryable) NN_UNPACK(best, &j, &d)
  };
  if (!(wv * 64 < n_model)) return;
  int sb0 = wv * 64, sb1 = sb0 + stride, sb2 = sb0 + 2 * stride, sb3 = sb0 + 3 * stride;
  int i_c = ld_u32(c.perm, min(sb0 + lane, c.last_s));
  int i_n = ld_u32(c.perm, min(sb1 + lane, c.last_s));
  int i_nn = ld_u32(c.perm, min(sb2 + lane, c.last_s));
  F3 q_c = ld3_u32(c.mod, i_c), q_n = ld3_u32(c.mod, i_n);
  float b_c = bnd_ld(c.bnd, i_c), b_n = bnd_ld(c.bnd, i_n);
  Prep A, B;
  prepare(A, sb0, i_c, q_c, b_c);
  bool pend = false, p_active = false;
  int p_i = 0, p_j = -1;
  float p_qx = 0.f, p_qy = 0.f, p_qz = 0.f, p_d = NAN;
  // one step: the results of the step before are stored, the queries of the step after next requested, the NEXT step prepared
  // (its loads issued), then THIS step finished
#define ICP_PIPE_STEP(CUR, NXT)                                                                                        \
  {                                                                                                                    \
    if (pend) { found(p_active, p_i, p_qx, p_qy, p_qz, p_j, p_d); pend = false; }                                      \
    const F3 q_nn = ld3_u32(c.mod, i_nn);  const float b_nn = bnd_ld(c.bnd, i_nn); const int i_nnn = ld_u32(c.perm, min(sb3 + lane, c.last_s)); \
    prepare(NXT, sb1, i_n, q_n, b_n);                                                                          \
    int j_; float d_;                                                                                                  \
    finish(CUR, j_, d_);                                                                                               \
    pend = true; p_active = CUR.active; p_i = CUR.i; p_qx = CUR.qx; p_qy = CUR.qy; p_qz = CUR.qz; p_j = j_; p_d = d_;  \
    i_n = i_nn; q_n = q_nn; b_n = b_nn; i_nn = i_nnn; sb0 = sb1; sb1 = sb2; sb2 = sb3; sb3 += stride; \
  }
  for (;;) {
    ICP_PIPE_STEP(A, B)
    if (!(sb0 < n_model)) break;
    ICP_PIPE_STEP(B, A)
    if (!(sb0 < n_model)) break;
  }
#undef ICP_PIPE_STEP
  if (pend) found(p_active, p_i, p_qx, p_qy, p_qz, p_j, p_d);
}
