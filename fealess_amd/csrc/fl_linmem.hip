// fl_linmem.hip -- hand-written gfx950 kernels for the first stage of the online matching half of
// cup_linemod::Detector (reference: linemod/linemod.cpp:882-1577; the later stages: fl_scan.hip, fl_refine.hip, fl_match.hip).
//
//   k_build_lm     spread + computeResponseMaps + linearize x8 fused        (:950-1088)
//   k_spread       the spread image alone, for the finer levels             (:950-965)
//
// Data layout in HBM (per frame, per level, per modality): the 8 linear memories
//   LM[label 0..7][grid (y%T)*T + x%T][(y/T)*W + x/T]   + per-label zero pad
// i.e. exactly the reference's "linearized" Mats laid back to back, so that the reference's
// 1-D scan over template_positions (including its row wrap-around, quirk Q1, and its over-read
// into the next grid row, Q2) is reproduced by plain linear addressing.
// All integer work; the only float expressions are the reference's own score formulas, built
// with -ffp-contract=off so each operator is one IEEE binary32 operation.
#include "fl_internal.h"
#include <algorithm>
#include <type_traits>

// ------------------------------------------------------------------------------------------
// Response of orientation `ori` to a spread byte b (SIMILARITY_LUT of this fork, linemod.cpp:970): 4 if bit ori is set, else 2
// if a neighbouring orientation (+-1 mod 8) is set, else 1 if +-2 is set, else 0 -- evaluated with an 8-bit rotate instead of
// the two 16-entry table look-ups (identical integers).
//
// k_build_lm_generic (any shape): one thread per (grid cell, linear position p); the 8 label bytes it produces go to 8 byte
// streams.  blockIdx.z = frame * n_mod + modality.
__global__ __launch_bounds__(256) void k_build_lm_generic(FlPlanes pl, int n_mod, int w, int h, int T, int W, int WH, uint32_t stride)
{
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int gi = blockIdx.y;
  const int frame = blockIdx.z / n_mod, m = blockIdx.z - frame * n_mod;
  const uint8_t *q = pl.in + (size_t)frame * pl.in_stride + pl.in_off[m];
  uint8_t *out = pl.out + (size_t)frame * pl.out_stride + pl.out_off[m];
  if (p >= WH) return;
  const int gy = gi / T, gx = gi - gy * T;
  const int yt = p / W, xt = p - yt * W;
  const int y = yt * T + gy, x = xt * T + gx;
  // spread (linemod.cpp:950-965): OR over the T x T window anchored at (y, x), clipped
  unsigned b = 0;
  const int rmax = min(T, h - y), cmax = min(T, w - x);
  for (int r = 0; r < rmax; ++r) {
    const uint8_t *row = q + (size_t)(y + r) * w + x;
    for (int c = 0; c < cmax; ++c) b |= row[c];
  }
  const unsigned bb = b | (b << 8);           // rotate helper
#pragma unroll
  for (int ori = 0; ori < 8; ++ori) {
    unsigned rot = (bb >> ori) & 0xFFu;
    unsigned r = (rot & 1u) ? 4u : ((rot & 0x82u) ? 2u : ((rot & 0x44u) ? 1u : 0u));
    out[(size_t)ori * stride + (size_t)gi * WH + p] = (uint8_t)r;
  }
}

// i / d for the small loop indices of the fast kernels: (i + 0.5) * (1/d) in float is at least 0.5/d away from an
// integer while its rounding error is below i/d * 2^-22, so the truncation is exact for i < 2^20 (here i < 2^16).
// 4 VALU instructions instead of the ~35 of an integer division by a run-time divisor.
__device__ __forceinline__ int div_small(int i, float inv_d) { return (int)(((float)i + 0.5f) * inv_d); }

// OR of the T four-byte windows at byte offsets 0 .. T - 1 (T <= 8) of the 12 bytes s0 s1 s2: four pixels of the horizontal
// spread.  One v_alignbyte_b32 extracts a window (full rate).  TT is T where an instance is compiled for it (4, 5, 8) and 0 for
// the run-time form, whose eight taps are all computed and the ones past T dropped by a select.
template <int TT>
__device__ __forceinline__ uint32_t or_windows(uint32_t s0, uint32_t s1, uint32_t s2, int T)
{
  uint32_t acc = s0;
#pragma unroll
  for (int c = 1; c < (TT ? TT : 8); ++c) {
    const uint32_t win = c < 4 ? __builtin_amdgcn_alignbyte(s1, s0, (unsigned)c) : __builtin_amdgcn_alignbyte(s2, s1, (unsigned)(c - 4));
    acc |= (TT || c < T) ? win : 0u;
  }
  return acc;
}

// The fast kernels move rows as 16-byte (V16) or 4-byte pieces; the same code serves both through these.
__device__ __forceinline__ uint32_t v_or(uint32_t a, uint32_t b) { return a | b; }
__device__ __forceinline__ uint4 v_or(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }
__device__ __forceinline__ uint32_t v_keep(uint32_t a, bool p) { return p ? a : 0u; }
__device__ __forceinline__ uint4 v_keep(uint4 a, bool p) { return make_uint4(p ? a.x : 0u, p ? a.y : 0u, p ? a.z : 0u, p ? a.w : 0u); }
// The responses of all 8 labels to four spread bytes packed in a dword, out[label] packed the same way: four 8-byte rows of the
// response table `tab` (one per spread byte, byte l = label l: the SIMILARITY_LUT evaluated for all orientations), transposed
// by byte permutes -- 24 vector instructions where eight refine_resp4 (fl_refine.hip) take 120 (identical integers).
__device__ __forceinline__ void resp_labels(const uint2 *tab, uint32_t s, uint32_t out[8])
{
  const uint2 r0 = tab[s & 0xFFu], r1 = tab[(s >> 8) & 0xFFu], r2 = tab[(s >> 16) & 0xFFu], r3 = tab[s >> 24];
  const uint32_t a0 = __builtin_amdgcn_perm(r1.x, r0.x, 0x05010400u), a1 = __builtin_amdgcn_perm(r1.x, r0.x, 0x07030602u);
  const uint32_t a2 = __builtin_amdgcn_perm(r3.x, r2.x, 0x05010400u), a3 = __builtin_amdgcn_perm(r3.x, r2.x, 0x07030602u);
  const uint32_t b0 = __builtin_amdgcn_perm(r1.y, r0.y, 0x05010400u), b1 = __builtin_amdgcn_perm(r1.y, r0.y, 0x07030602u);
  const uint32_t b2 = __builtin_amdgcn_perm(r3.y, r2.y, 0x05010400u), b3 = __builtin_amdgcn_perm(r3.y, r2.y, 0x07030602u);
  out[0] = __builtin_amdgcn_perm(a2, a0, 0x05040100u); out[1] = __builtin_amdgcn_perm(a2, a0, 0x07060302u);
  out[2] = __builtin_amdgcn_perm(a3, a1, 0x05040100u); out[3] = __builtin_amdgcn_perm(a3, a1, 0x07060302u);
  out[4] = __builtin_amdgcn_perm(b2, b0, 0x05040100u); out[5] = __builtin_amdgcn_perm(b2, b0, 0x07060302u);
  out[6] = __builtin_amdgcn_perm(b3, b1, 0x05040100u); out[7] = __builtin_amdgcn_perm(b3, b1, 0x07060302u);
}
__device__ __forceinline__ void v_resp_labels(const uint2 *tab, uint32_t s, uint32_t out[8]) { resp_labels(tab, s, out); }
__device__ __forceinline__ void v_resp_labels(const uint2 *tab, uint4 s, uint4 out[8])
{
  uint32_t x[8], y[8], z[8], w[8];
  resp_labels(tab, s.x, x); resp_labels(tab, s.y, y); resp_labels(tab, s.z, z); resp_labels(tab, s.w, w);
#pragma unroll
  for (int l = 0; l < 8; ++l) out[l] = make_uint4(x[l], y[l], z[l], w[l]);
}

// k_build_lm, the fast path (w % 4 == 0, (w/T) % 4 == 0, 2 <= T <= 8): one workgroup per (frame, modality, grid row gy, band of
// HB rows yt of the linear memories).  For a fixed gy the T grids (gy, gx = 0 .. T-1) lie back to back in every label's memory,
// so with one band (HB = H, the batched case) a workgroup owns T * W * H contiguous bytes of each of the 8 labels -- 9600 B at
// VGA level 1, 75 whole 128-byte lines that no other workgroup touches.  It needs only the spread rows y = yt * T + gy:
//   1. vertical OR: an item is a (row yt, 16- or 4-byte column piece); its thread issues the T row loads together, ORs them and
//      writes one piece of V[yt][x] to LDS (pitch w + 16, the pad is zero: windows run past x = w - 1).  Every quantised row is
//      read by T workgroups of the frame, which share an XCD (below) and so an L2.
//   2. horizontal OR of V, four pixels per 32-bit operation, reads of four items in flight; the spread bytes are scattered to
//      Lin[gx][yt * W + xt], which is the band's part of a label's memory, gx-major, with the spread byte in place of the response.
//   3. a lane takes 16 (or, where a band's runs are not multiples of 16 B, 4) consecutive bytes of Lin, several items' reads
//      ahead of the first wait, fetches the 8 responses of each byte from a 2 KB LDS table (built over V, which is dead by
//      then), transposes them to labels with byte permutes (resp_labels) and stores 8 pieces of 16 (4) bytes; a wave's store
//      instruction covers 1024 contiguous bytes.  (refine_resp4 on the packed bytes needs no table but 120 instead of 24
//      vector instructions per four bytes, and the kernel is bound by instruction issue: 1.37 against 1.24 ms per launch.)
// Blocks are dealt round-robin over the 8 XCDs: block b serves frame (b & 7) + 8 * ..., as in k_scan, so all pieces of a frame
// (the lines two bands share, and the quantised rows) meet in one L2.  Placement only affects speed.
struct BuildLmArgs {
  FlPlanes pl;
  int n_frames, w, h, T, W, H, HB, nbands, out16;
  uint32_t stride;
};

template <typename VT, int U>
__device__ __forceinline__ void lm_write_labels(const uint8_t *Lin, const uint2 *tab, uint8_t *dst0, int n, int per_gx, int WH,
                                                uint32_t stride, int tid)
{
  constexpr int VB = (int)sizeof(VT);
  const float inv = 1.0f / (float)per_gx;
  for (int base = 0; base < n; base += U * 256) {
    VT s[U];
#pragma unroll
    for (int u = 0; u < U; ++u) s[u] = ((const VT *)Lin)[min(base + tid + 256 * u, n - 1)];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + tid + 256 * u;
      if (i < n) {
        const int gx = div_small(i, inv), rem = i - __mul24(gx, per_gx);
        uint8_t *dst = dst0 + (uint32_t)(gx * WH + rem * VB);
        VT r[8];
        v_resp_labels(tab, s[u], r);
#pragma unroll
        for (int l = 0; l < 8; ++l) *(VT *)(dst + (size_t)l * stride) = r[l];
      }
    }
  }
}

template <int TT, bool V16>
__global__ __launch_bounds__(256) void k_build_lm(BuildLmArgs a)
{
  extern __shared__ __align__(16) uint8_t smem[];
  using VT = typename std::conditional<V16, uint4, uint32_t>::type;
  constexpr int VB = (int)sizeof(VT), TU = TT ? TT : 8;
  const int T = TT ? TT : a.T, tid = threadIdx.x;
  const int pieces = T * a.nbands, q8 = blockIdx.x >> 3;
  const int frame = (blockIdx.x & 7) + 8 * (q8 / pieces);
  if (frame >= a.n_frames) return;                          // workgroup-uniform
  const int piece = q8 % pieces, gy = piece / a.nbands, yt0 = (piece - gy * a.nbands) * a.HB;
  const int hb = min(a.HB, a.H - yt0), nb = hb * a.W, w = a.w, h = a.h, pitch = w + 16;
  uint8_t *V = smem, *Lin = smem + max((a.HB * pitch + 15) & ~15, 2048);
  const uint8_t *q = a.pl.in + (size_t)frame * a.pl.in_stride + a.pl.in_off[blockIdx.y];
  uint8_t *out = a.pl.out + (size_t)frame * a.pl.out_stride + a.pl.out_off[blockIdx.y];
  {
    const int cpad = pitch / VB, cin = w / VB;              // pieces of an LDS row (pad included) and of an image row
    const float inv_cpad = 1.0f / (float)cpad;
    for (int i = tid; i < hb * cpad; i += 256) {
      const int yt = div_small(i, inv_cpad), c = i - __mul24(yt, cpad);
      const int y = (yt0 + yt) * T + gy;
      const uint32_t col = (uint32_t)(min(c, cin - 1) * VB);
      VT v[TU];
#pragma unroll
      for (int r = 0; r < TU; ++r)                          // rows past the image or past T: an address inside the image, dropped below
        v[r] = *(const VT *)(q + ((uint32_t)__mul24(min(y + ((TT || r < T) ? r : 0), h - 1), w) + col));
      VT acc = v_keep(v[0], c < cin);
#pragma unroll
      for (int r = 1; r < TU; ++r) acc = v_or(acc, v_keep(v[r], (TT || r < T) && y + r < h && c < cin));
      *(VT *)(V + (__mul24(yt, pitch) + c * VB)) = acc;
    }
  }
  __syncthreads();
  {
    const int Wd = (a.W >> 2) * T, pd = pitch >> 2, n = hb * Wd;   // W % 4 == 0: a row's W * T spread bytes are whole dwords
    const float inv_Wd = 1.0f / (float)Wd, inv_T = 1.0f / (float)T;
    for (int base = 0; base < n; base += 4 * 256) {
      uint32_t s[4][3];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = min(base + tid + 256 * u, n - 1);
        const int yt = div_small(i, inv_Wd), k = i - __mul24(yt, Wd);
        const uint32_t *src = (const uint32_t *)V + (__mul24(yt, pd) + k);
        s[u][0] = src[0]; s[u][1] = src[1]; s[u][2] = src[2];                     // k + 2 <= w/4 + 1: inside the zero pad
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = base + tid + 256 * u;
        if (i < n) {
          const int yt = div_small(i, inv_Wd), k = i - __mul24(yt, Wd);
          const uint32_t acc = or_windows<TT>(s[u][0], s[u][1], s[u][2], T);
          uint8_t *row = Lin + __mul24(yt, a.W);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int x = 4 * k + j;
            const int xt = TT ? x / (TT ? TT : 1) : div_small(x, inv_T), gx = x - __mul24(xt, T);
            row[__mul24(gx, nb) + xt] = (uint8_t)(acc >> (8 * j));
          }
        }
      }
    }
  }
  __syncthreads();
  uint2 *tab = (uint2 *)smem;                               // over V, which has been read
  {
    const unsigned b = (unsigned)tid, bb = b | (b << 8);
    uint32_t v[2] = {0, 0};
#pragma unroll
    for (int ori = 0; ori < 8; ++ori) {
      const unsigned rot = (bb >> ori) & 0xFFu;
      v[ori >> 2] |= ((rot & 1u) ? 4u : ((rot & 0x82u) ? 2u : ((rot & 0x44u) ? 1u : 0u))) << (8 * (ori & 3));
    }
    tab[tid] = make_uint2(v[0], v[1]);
  }
  __syncthreads();
  uint8_t *dst0 = out + ((size_t)gy * T * a.W * a.H + (size_t)yt0 * a.W);
  if (a.out16) lm_write_labels<uint4, 3>(Lin, tab, dst0, (T * nb) >> 4, nb >> 4, a.W * a.H, a.stride, tid);
  else         lm_write_labels<uint32_t, 4>(Lin, tab, dst0, (T * nb) >> 2, nb >> 2, a.W * a.H, a.stride, tid);
}

// k_spread: the spread image alone (linemod.cpp:950-965) for the finer pyramid levels.  Those levels are only read by the
// refinement (a few 16x16 patches per frame), which evaluates the response LUT on the fly instead of reading 8 linear memories.
// One workgroup per (strip of RS rows, modality, frame):
//   1. the strip's RS + T - 1 quantised rows go to LDS image A; a thread issues all its loads of a batch (clamped to addresses
//      this strip reads anyway, so no branch stands between them) before it writes the first;
//   2. vertical OR of T rows of A into B, the T reads of an item (two items in the 4-byte form) in flight together;
//   3. horizontal OR of B, four pixels per 32-bit operation, and the store.
// V16 (whole images with 16-byte rows): 16-byte loads, LDS accesses and stores.  The 4-byte form also serves the lazy fine
// levels, where the work set is the column window of the marked tiles these rows cross, trimmed by the tiles' row ranges,
// and a strip that touches nothing returns: window edges are multiples of 60 pixels, so no wider access fits them.
struct SpreadArgs {
  FlPlanes pl;
  const uint32_t *tiles;
  size_t tiles_stride;
  int w, h, T, RS;
};

template <int TT, bool V16>
__global__ __launch_bounds__(256) void k_spread(SpreadArgs a)
{
  extern __shared__ __align__(16) uint8_t smem[];
  using VT = typename std::conditional<V16, uint4, uint32_t>::type;
  constexpr int VB = (int)sizeof(VT), TU = TT ? TT : 8;
  const int T = TT ? TT : a.T, w = a.w, h = a.h, RS = a.RS, pitch = w + 16, rows_in = RS + T - 1;
  uint8_t *A = smem, *B = smem + (size_t)rows_in * pitch;
  const uint8_t *q = a.pl.in + (size_t)blockIdx.z * a.pl.in_stride + a.pl.in_off[blockIdx.y];
  uint8_t *out = a.pl.out + (size_t)blockIdx.z * a.pl.out_stride + a.pl.out_off[blockIdx.y];
  const int y0 = blockIdx.x * RS, tid = threadIdx.x;
  const int cpad = pitch / VB, cin = w / VB;
  // column window [lo, lo + n_out) in pieces: everything, or (lazy fine level) the span of the marked tiles
  // that these rows cross -- nothing marked, nothing to do
  int lo = 0, n_out = cin;
  if (!V16 && a.tiles) {
    const uint32_t *tf = a.tiles + (size_t)blockIdx.z * a.tiles_stride;
    const int nstrips = (w + FL_TILE - 1) / FL_TILE;
    const int c0 = y0 / FL_TILE, c1 = min(y0 + RS - 1, h - 1) / FL_TILE;
    int smin = nstrips, smax = -1;
    for (int c = c0; c <= c1; ++c)
      for (int st = 0; st < nstrips; ++st) {
        const int t = c * nstrips + st;
        if (!((tf[t >> 5] >> (t & 31)) & 1u)) continue;
        const uint32_t rw = tf[2 * FL_TILE_WORDS + t];     // rows of this tile that are read: does the strip touch them?
        if ((int)(rw & 0xFFFFu) < y0 || (int)(rw >> 16) > y0 + RS - 1) continue;
        smin = min(smin, st);
        smax = max(smax, st);
      }
    if (smax < 0) return;                                  // workgroup-uniform
    lo = (smin * FL_TILE) >> 2;
    n_out = (min(w, (smax + 1) * FL_TILE) + 3) / 4 - lo;
  }
  const int n_in = V16 ? cpad : min(cpad, lo + n_out + 3) - lo;   // the horizontal OR of dword c reads dwords c .. c + 2
  const float inv_in = 1.0f / (float)n_in, inv_out = 1.0f / (float)n_out;
  const int n_st = rows_in * n_in;
  auto stage = [&](auto ub, int base) {
    constexpr int UB = decltype(ub)::value;
    VT v[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int i = min(base + tid + 256 * u, n_st - 1);
      const int r = div_small(i, inv_in), c = lo + (i - __mul24(r, n_in));
      v[u] = *(const VT *)(q + ((uint32_t)__mul24(min(y0 + r, h - 1), w) + (uint32_t)(min(c, cin - 1) * VB)));
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const int i = base + tid + 256 * u;
      if (i < n_st) {
        const int r = div_small(i, inv_in), c = lo + (i - __mul24(r, n_in));
        *(VT *)(A + (__mul24(r, pitch) + c * VB)) = v_keep(v[u], y0 + r < h && c < cin);
      }
    }
  };
  if (n_st <= 4 * 256) stage(std::integral_constant<int, 4>{}, 0);
  else
    for (int base = 0; base < n_st; base += (V16 ? 8 : 16) * 256) stage(std::integral_constant<int, V16 ? 8 : 16>{}, base);
  __syncthreads();
  {
    constexpr int UV = V16 ? 1 : 2;
    const int n_v = RS * n_in;
    for (int base = 0; base < n_v; base += UV * 256) {
      VT acc[UV];
      int o[UV];
#pragma unroll
      for (int u = 0; u < UV; ++u) {
        const int i = min(base + tid + 256 * u, n_v - 1);
        const int r = div_small(i, inv_in), c = lo + (i - __mul24(r, n_in));
        o[u] = __mul24(r, pitch) + c * VB;
        VT t = *(const VT *)(A + o[u]);
#pragma unroll
        for (int rr = 1; rr < TU; ++rr)
          t = v_or(t, v_keep(*(const VT *)(A + (o[u] + ((TT || rr < T) ? rr : 0) * pitch)), TT || rr < T));
        acc[u] = t;
      }
#pragma unroll
      for (int u = 0; u < UV; ++u)
        if (base + tid + 256 * u < n_v) *(VT *)(B + o[u]) = acc[u];
    }
  }
  __syncthreads();
  {
    constexpr int UH = V16 ? 2 : 4;                         // items whose LDS reads are issued together
    const int n_h = min(RS, h - y0) * n_out;                // rows past the image are not stored
    for (int base = 0; base < n_h; base += UH * 256) {
      VT s[UH];
      uint2 t[UH];
#pragma unroll
      for (int u = 0; u < UH; ++u) {
        const int i = min(base + tid + 256 * u, n_h - 1);
        const int r = div_small(i, inv_out), c = lo + (i - __mul24(r, n_out));
        const uint8_t *src = B + (__mul24(r, pitch) + c * VB);
        s[u] = *(const VT *)src;
        if constexpr (V16) t[u] = *(const uint2 *)(src + 16);                      // the next 8 bytes: inside the row's pad at its end
        else t[u] = make_uint2(((const uint32_t *)src)[1], ((const uint32_t *)src)[2]);
      }
#pragma unroll
      for (int u = 0; u < UH; ++u) {
        const int i = base + tid + 256 * u;
        if (i < n_h) {
          const int r = div_small(i, inv_out), c = lo + (i - __mul24(r, n_out));
          uint8_t *dst = out + ((uint32_t)__mul24(y0 + r, w) + (uint32_t)(c * VB));
          if constexpr (V16) {
            *(uint4 *)dst = make_uint4(or_windows<TT>(s[u].x, s[u].y, s[u].z, T), or_windows<TT>(s[u].y, s[u].z, s[u].w, T),
                                       or_windows<TT>(s[u].z, s[u].w, t[u].x, T), or_windows<TT>(s[u].w, t[u].x, t[u].y, T));
          } else {
            *(uint32_t *)dst = or_windows<TT>(s[u], t[u].x, t[u].y, T);
          }
        }
      }
    }
  }
}

// blockIdx.z = frame * n_mod + modality
__global__ __launch_bounds__(256) void k_spread_generic(FlPlanes pl, int n_mod, int w, int h, int T)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const int frame = blockIdx.z / n_mod, m = blockIdx.z - frame * n_mod;
  const uint8_t *q = pl.in + (size_t)frame * pl.in_stride + pl.in_off[m];
  unsigned b = 0;
  const int rmax = min(T, h - y), cmax = min(T, w - x);
  for (int r = 0; r < rmax; ++r)
    for (int c = 0; c < cmax; ++c) b |= q[(size_t)(y + r) * w + x + c];
  pl.out[(size_t)frame * pl.out_stride + pl.out_off[m] + (size_t)y * w + x] = (uint8_t)b;
}

// The instance of a fast kernel for T (4, 5 and 8 are compiled in; 0 is the run-time form) and the piece size
#define FL_PICK_T(kern, T, v16)                                                                                                  \
  ((v16) ? ((T) == 4 ? kern<4, true> : (T) == 5 ? kern<5, true> : (T) == 8 ? kern<8, true> : kern<0, true>)                      \
         : ((T) == 4 ? kern<4, false> : (T) == 5 ? kern<5, false> : (T) == 8 ? kern<8, false> : kern<0, false>))

// every plane of every frame starts at a multiple of `al` bytes
static bool planes_aligned(const FlPlanes &pl, int n_mod, size_t al)
{
  bool ok = pl.in_stride % al == 0 && pl.out_stride % al == 0;
  for (int m = 0; m < n_mod; ++m) ok = ok && ((uintptr_t)pl.in + pl.in_off[m]) % al == 0 && ((uintptr_t)pl.out + pl.out_off[m]) % al == 0;
  return ok;
}

// One launch for the n_mod modalities of a level (grid.y).  tiles == nullptr: the whole image.  Otherwise (lazy fine level)
// only what the marked tiles need; the generic fallback kernel ignores the marks and spreads everything, which is always
// sufficient.
int fl_launch_spread_tiles(fl_context *ctx, const FlPlanes &pl, int n_mod, int n_frames, int w, int h, int T, const uint32_t *tiles,
                           size_t tiles_stride)
{
  if (w % 4 == 0 && T <= 8 && T >= 2 && planes_aligned(pl, n_mod, 4)) {
    int k = 4;                                   // strips of k x T rows (taller strips cost the lazy fine level more than they save:
                                                 // k = 6 took 5.0 against 3.95 ms per 4096 frames, a strip works for every marked tile it touches)
    for (; k > 1 && (size_t)2 * (k * T + T - 1) * (w + 16) > 60 * 1024; --k) {}
    const size_t lds = (size_t)(2 * k * T + T - 1) * (w + 16);
    if ((size_t)2 * (k * T + T - 1) * (w + 16) <= 64 * 1024) {
      SpreadArgs a{pl, tiles, tiles_stride, w, h, T, k * T};
      const bool v16 = !tiles && w % 16 == 0 && planes_aligned(pl, n_mod, 16);
      dim3 grid((h + a.RS - 1) / a.RS, n_mod, n_frames);
      hipLaunchKernelGGL(FL_PICK_T(k_spread, T, v16), grid, dim3(256), lds, ctx->stream, a);
      FL_HIP(ctx, hipGetLastError());
      return FL_OK;
    }
  }
  dim3 grid((w + 63) / 64, (h + 3) / 4, n_frames * n_mod);
  hipLaunchKernelGGL(k_spread_generic, grid, dim3(256), 0, ctx->stream, pl, n_mod, w, h, T);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

// LDS of a k_build_lm workgroup with bands of HB rows: V (later the 2 KB response table) and Lin
static size_t build_lm_lds(int w, int W, int T, int HB)
{
  return std::max<size_t>(((size_t)HB * (w + 16) + 15) & ~(size_t)15, 2048) + (size_t)T * HB * W;
}

// The band height of k_build_lm (0: the shape takes the generic kernel).  Exposed to the tests through fl_dev_build_lm_band.
//   - whole grid rows (HB = H) where 8 workgroups of that size share a CU's LDS (FL_LM_LDS each; VGA level 1 needs 19 680 B)
//     and the batch fills the GPU: every run a workgroup writes is then T * W * H bytes long;
//   - lower bands where the LDS asks for it, and where n_frames * n_mod * T workgroups would leave CUs idle (FL_LM_BLOCKS),
//     though never runs below FL_LM_RUN bytes;
//   - a band height below H is a multiple of the rows after which a run is again 16-byte aligned, where that is possible.
#define FL_LM_LDS (20 * 1024)
#define FL_LM_BLOCKS 1024
#define FL_LM_RUN 256
static int build_lm_band(int n_frames, int n_mod, int w, int h, int T)
{
  if (T < 2 || T > 8 || w % 4 != 0) return 0;
  const int W = w / T, H = h / T;
  if (W < 4 || W % 4 != 0 || H < 1) return 0;
  int HB = H;
  while (HB > 1 && build_lm_lds(w, W, T, HB) > FL_LM_LDS) --HB;
  if (build_lm_lds(w, W, T, HB) > 64 * 1024) return 0;
  const long blocks = (long)n_frames * n_mod * T;
  if (blocks < FL_LM_BLOCKS) {
    const int bands = (int)((FL_LM_BLOCKS + blocks - 1) / blocks);
    HB = min(HB, max(max(H / bands, (FL_LM_RUN + W - 1) / W), 1));
  }
  int step = 1;
  while ((step * W) % 16 != 0) step *= 2;       // W % 4 == 0: step is 1, 2 or 4
  if (HB < H && HB >= step) HB -= HB % step;
  return HB;
}
extern "C" int fl_dev_build_lm_band(int n_frames, int n_mod, int w, int h, int T) { return build_lm_band(n_frames, n_mod, w, h, T); }

// The 8 linear memories of every modality (grid.y) of a level in one launch.
int fl_launch_build_lm(fl_context *ctx, const FlPlanes &pl, int n_mod, int n_frames, int w, int h, int T)
{
  const int W = w / T, H = h / T, WH = W * H;
  const uint32_t stride = (uint32_t)fl_lm_label_stride(w, h, T);
  const int HB = planes_aligned(pl, n_mod, 4) ? build_lm_band(n_frames, n_mod, w, h, T) : 0;
  if (HB) {
    BuildLmArgs a{pl, n_frames, w, h, T, W, H, HB, (H + HB - 1) / HB, 0, stride};
    a.out16 = WH % 16 == 0 && (a.nbands == 1 || (HB * W) % 16 == 0) && planes_aligned(pl, n_mod, 16);
    const bool v16 = w % 16 == 0 && planes_aligned(pl, n_mod, 16);
    dim3 grid((unsigned)(8 * ((n_frames + 7) / 8) * T * a.nbands), n_mod, 1);
    hipLaunchKernelGGL(FL_PICK_T(k_build_lm, T, v16), grid, dim3(256), build_lm_lds(w, W, T, HB), ctx->stream, a);
    FL_HIP(ctx, hipGetLastError());
    return FL_OK;
  }
  dim3 grid((WH + 255) / 256, T * T, n_frames * n_mod);
  hipLaunchKernelGGL(k_build_lm_generic, grid, dim3(256), 0, ctx->stream, pl, n_mod, w, h, T, W, WH, stride);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

extern "C" int fl_build_linear_memories(fl_context *ctx, const uint8_t *quantized, int w, int h, int T, uint8_t *out,
                                        int mem)
{
  if (!ctx || !quantized || !out || w <= 0 || h <= 0 || T < 1 || T > 16) return FL_ERR_INVALID;
  if (w % T || h % T) return fl_set_error(ctx, FL_ERR_ASSERT, "rows/cols %% T != 0 (CV_Assert linemod.cpp:1062-1063)");
  if ((w * h) % 16) return fl_set_error(ctx, FL_ERR_ASSERT, "rows*cols %% 16 != 0 (CV_Assert linemod.cpp:981)");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nq = (size_t)w * h, nlm = 8 * fl_lm_label_stride(w, h, T);
  const uint8_t *dq = quantized;
  uint8_t *dlm = out;
  if (mem == FL_MEM_HOST) {
    void *s = nullptr;
    int rc = fl_scratch(ctx, fl_align(nq, 256) + nlm, &s);
    if (rc) return rc;
    FL_HIP(ctx, hipMemcpyAsync(s, quantized, nq, hipMemcpyHostToDevice, ctx->stream));
    dq = (const uint8_t *)s;
    dlm = (uint8_t *)s + fl_align(nq, 256);
  }
  FL_HIP(ctx, hipMemsetAsync(dlm, 0, nlm, ctx->stream));       // the zero pads
  const FlPlanes pl{dq, dlm, 0, 0, {0, 0}, {0, 0}};
  int rc = fl_launch_build_lm(ctx, pl, 1, 1, w, h, T);
  if (rc) return rc;
  if (mem == FL_MEM_HOST) {
    FL_HIP(ctx, hipMemcpyAsync(out, dlm, nlm, hipMemcpyDeviceToHost, ctx->stream));
    FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return FL_OK;
}
