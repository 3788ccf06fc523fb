// fl_linemod.hip -- hand-written gfx950 kernels for the online matching half of
// cup_linemod::Detector (reference: linemod/linemod.cpp:882-1577).
//
//   k_build_lm     spread + computeResponseMaps + linearize x8 fused        (:950-1088)
//   k_scan         similarity + addSimilarities + coarse threshold          (:1130-1214, 1322-1338, 1483-1506)
//   k_refine       similarityLocal + 16x16 argmax + filter, one level       (:1226-1300, 1509-1573)
//   k_refine_lds   the same on spread bytes staged in LDS, a group of candidates per window
//   k_sort_unique  std::sort + std::unique of the surviving matches         (:1437-1439)
//
// Data layout in HBM (per frame, per level, per modality): the 8 linear memories
//   LM[label 0..7][grid (y%T)*T + x%T][(y/T)*W + x/T]   + per-label zero pad
// i.e. exactly the reference's "linearized" Mats laid back to back, so that the reference's
// 1-D scan over template_positions (including its row wrap-around, quirk Q1, and its over-read
// into the next grid row, Q2) is reproduced by plain linear addressing.
// All integer work; the only float expressions are the reference's own score formulas, built
// with -ffp-contract=off so each operator is one IEEE binary32 operation.
#include "fl_internal.h"
#include <limits.h>
#include <string.h>
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

// The four responses of label `lab` (0 .. 7) to four spread bytes packed in a dword: every byte is rotated right by lab (the
// reference's LUT is indexed by the rotated byte), then the tests for bit 0 (response 4), bits 0x82 (2) and bits 0x44 (1) run
// on all four bytes at once.
__device__ __forceinline__ uint32_t refine_resp4(uint32_t p, int lab)
{
  const uint32_t M = 0x01010101u;
  const uint32_t lo = (0xFFu >> lab) * M;                                 // the bits of a byte that a right shift by lab keeps
  const uint32_t rot = ((p >> lab) & lo) | ((p << (8 - lab)) & ~lo);
  const uint32_t t1 = rot & M;
  const uint32_t t2 = ((rot >> 1) | (rot >> 7)) & M;
  const uint32_t t3 = ((rot >> 2) | (rot >> 6)) & M;
  const uint32_t n1 = t1 ^ M, n2 = t2 ^ M;
  return (t1 << 2) | (((t2 << 1) | (t3 & n2)) & ((n1 << 1) | n1));
}

// The fast kernels move rows as 16-byte (V16) or 4-byte pieces; the same code serves both through these.
__device__ __forceinline__ uint32_t v_or(uint32_t a, uint32_t b) { return a | b; }
__device__ __forceinline__ uint4 v_or(uint4 a, uint4 b) { return make_uint4(a.x | b.x, a.y | b.y, a.z | b.z, a.w | b.w); }
__device__ __forceinline__ uint32_t v_keep(uint32_t a, bool p) { return p ? a : 0u; }
__device__ __forceinline__ uint4 v_keep(uint4 a, bool p) { return make_uint4(p ? a.x : 0u, p ? a.y : 0u, p ? a.z : 0u, p ? a.w : 0u); }
// The responses of all 8 labels to four spread bytes packed in a dword, out[label] packed the same way: four 8-byte rows of the
// response table `tab` (one per spread byte, byte l = label l: the SIMILARITY_LUT evaluated for all orientations), transposed
// by byte permutes -- 24 vector instructions where eight refine_resp4 take 120 (identical integers).
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

// ------------------------------------------------------------------------------------------
// k_scan: one wavefront per run of (pyramid, 1024-position chunk) work items of a frame.  Lane i owns 16 consecutive
// positions and keeps their u8 partial sums packed in four 32-bit registers per modality:
// with <= 63 features of response <= 4 a byte never carries (63*4 = 252, linemod.cpp:1133-1137),
// so one 32-bit add sums four positions.  Feature offsets are wave-uniform (scalar loads), padded
// to a multiple of 8 with the offset of the zero pad so that 8 independent 16-byte loads are in
// flight per step.  The linear memories (1.2 MB per frame at VGA/T=8) are shared by all
// templates and are served from L2; the feature tables are the only per-template HBM stream.
// Between the modalities and after every 8 features a wave whose positions can no longer reach the coarse threshold stops
// (exact: see `prune` in the kernel); the reference adds every feature of every template everywhere (linemod.cpp:1471-1481).
//
// With pruning most items end after 16 of up to 126 features, and what such an item costs is not its bytes but the chain
// of dependent memory round trips in front of them.  So everything an item needs before its first vector load is one
// 64-byte record (FlScanItem, built at finalize: it depends on the bank and the geometry only) with the first eight
// offsets inline; the class filter's flag is a byte per ITEM, requested with the record; a wave walks `run` items
// (ScanArgs::run, fl_scan_run) and requests the next item's record and flag before it works on the current one; and
// inside an item the next group's eight offsets -- the next modality's first group behind a modality's last -- are
// requested before the current group's vector loads are waited for.  An early-pruned item then costs the two vector
// round trips of its two groups; the record, the flag and the offsets arrive underneath them.
//
// The bound is per lane (a lane's own 16 positions), so a lane that misses it stops loading for itself (ScanArgs::prune_lanes),
// and behind a modality's first eight features the checks come every STEP features (the kernel's second template parameter,
// fl_scan_step): see `alive` in the kernel.  What this buys is load instructions and lanes not issued; the launch is NOT bound by
// the vector cache's line lookups (a quarter fewer of them moved the time by 1 %, profiles/README.md).  What did bind it was the
// scalar cache: lane 63's tail dword, one scalar load per feature at an address all over the linear memories, is now fetched
// only where lane 63 loads.
struct ScanArgs {
  const FlScanItem *items;   // work list: one record per (pyramid, chunk)
  int n_items;
  const uint32_t *offs;      // FL_SCAN_OFF_PAD entries behind the last group
  const uint8_t *enabled;    // per work item, whole dwords: class selected by match()'s class_ids (linemod.cpp:1418-1434)
  uint8_t *ws;               // frame workspace base
  size_t ws_stride;
  size_t lm_off[FL_MAX_MODALITIES];
  size_t off_count, off_cand;
  int M, W, WH, T, cap;
  int bpf, n_frames;         // blocks per frame, frames in this launch
  int run, wave_step, item_step;   // wave w of a frame walks the items w * wave_step + i * item_step, i < run
  float threshold;
  int prune;                 // stop a (template, chunk) between modalities once no position can reach the threshold (exact)
  unsigned prune_mid;        // ... and inside a modality after the 8-feature groups whose bit is set (same bound, same exactness)
  int prune_lanes;           // a lane whose own 16 positions miss the bound stops loading (0: the wave stops as a whole or not at all)
  uint16_t *dbg;             // optional raw u16 maps of pyramids [dbg_first, dbg_first+dbg_count); null: dbg_count = 0
  int dbg_first, dbg_count;
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// the larger even byte and the larger odd byte of a word, as two 16-bit values (v_pk_max_u16)
__device__ __forceinline__ u16x2 pk_bytes_max(uint32_t a)
{
  const uint32_t lo = a & 0x00FF00FFu, hi = (a >> 8) & 0x00FF00FFu;
  return __builtin_elementwise_max(__builtin_bit_cast(u16x2, lo), __builtin_bit_cast(u16x2, hi));
}
__device__ __forceinline__ uint4 ld16(const uint8_t *p)
{
  uint4 v;
  __builtin_memcpy(&v, p, 16);     // global_load_dwordx4, any byte alignment (unaligned access mode)
  return v;
}
// a wave-uniform load of memory no kernel in flight writes: s_load_dword whatever stores the loop holds
#define FL_CONST_AS __attribute__((address_space(4)))
__device__ __forceinline__ uint32_t sload1(const void *p) { return *(const FL_CONST_AS uint32_t *)(uintptr_t)p; }
// What the loop keeps in flight for later -- the next item's record and flag, the next group's offsets -- travels in ONE vector
// register each, a dword per lane, and is taken apart with v_readlane when its turn comes: sixteen and eight scalar registers
// held across an item were more than the scalar file has beside the group in work (the compiler then issued a group's loads
// one at a time).  Vector loads return in order, so the wait for a group's own loads covers the request issued before them.
__device__ __forceinline__ uint32_t rl(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

#ifndef FL_SCAN_PRUNE_MID
#define FL_SCAN_PRUNE_MID 0x7Fu   // 8-feature groups after which a modality checks the bound (every one but the last: the check
                                  // after 16 features is the one that pays -- chunks without colour edges stop there)
#endif
#ifndef FL_SCAN_OFFSETS_AHEAD
#define FL_SCAN_OFFSETS_AHEAD 1   // 0 (comparison builds): every group fetches its own offsets first, a second round trip per group
#endif
// Waves per SIMD.  Without pruning the kernel is bound by the rate of its vector loads and five waves are the optimum (measured
// after the DPP change, ms per 1280 frames x 360 templates: 3: 2.32, 4: 1.95, 5: 1.71, 6: 1.77, 8: 2.17).  With pruning an item is
// two or three round trips and little else, the launch is bound by how many of them are in flight, and six beat five, eight
// beat seven where the first piece is short (profiles/README.md): the same code built twice, the launch picks by ScanArgs::prune.
#ifndef FL_SCAN_WPE
#define FL_SCAN_WPE 5
#endif
#ifndef FL_SCAN_WPE_PRUNED
#define FL_SCAN_WPE_PRUNED 8
#endif
// (The attribute makes the compiler pad a build's register allocation to its waves: a build for fewer than eight waves holds
// fewer although its code fits 64 vector and 80 scalar registers.)
#ifndef FL_SCAN_STEP
#define FL_SCAN_STEP 4            // feature loads between two checks behind a modality's first eight (option scan_prune_step: 8, 4 or 2)
#endif
#ifndef FL_SCAN_TAIL_ALWAYS
#define FL_SCAN_TAIL_ALWAYS 0     // 1 (comparison builds): lane 63's tail dword is loaded for every feature, needed or not
#endif
#ifdef FL_SCAN_STATS
// development aid: per launch {items, feature-load instructions, lane-loads (lanes in EXEC), items that ran to their end}, then
// the items ended by a check after f features of all modalities (f = 0 .. 126); printed by the launcher after a stream
// synchronisation (tools/dev/README.md)
#define FL_SCAN_STATS_N (4 + 2 * FL_MAX_FEATURES + 1 + 1)
__device__ unsigned long long d_scan_stats[FL_SCAN_STATS_N];
#define FL_SCAN_STAT(i, v) do { if (lane == 0) atomicAdd(&d_scan_stats[i], (unsigned long long)(v)); } while (0)
#else
#define FL_SCAN_STAT(i, v) do { } while (0)
#endif
template <int N> struct ScanInt { static constexpr int value = N; };
// STEP: behind a modality's first piece, the feature loads between two checks of the bound (8, 4 or 2)
// FIRST: the features of a modality's first piece, which has one check, behind it (8, 12, 14 or 16; fl_scan_first)
template <int WPE, int STEP, int FIRST>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_scan(ScanArgs a)
{
  static_assert(STEP == 8 || STEP == 4 || STEP == 2, "a group of eight offsets is cut into equal parts");
  static_assert(FIRST == 8 || FIRST == 12 || FIRST == 14 || FIRST == 16, "the first piece ends inside the second group, at an even feature");
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // XCD-aware block mapping: workgroups are dealt round-robin over the 8 XCDs, each with its own
  // 4 MB L2.  All blocks of one frame are given the same residue mod 8, so a frame's linear
  // memories (1.2 MB at VGA level 1) are fetched into ONE L2 and reused by every template there,
  // instead of being streamed into all eight.  Placement only affects speed, never results.
  const int xcd = blockIdx.x & 7, q = blockIdx.x >> 3;
  const int frame = xcd + 8 * (q / a.bpf);
  if (frame >= a.n_frames) return;
  int it = __builtin_amdgcn_readfirstlane(((q % a.bpf) * 4 + wave) * a.wave_step);
  if (it >= a.n_items) return;
  // lanes 0..15: the dwords of item `idx`'s record; the others: the dword that holds its class-filter flag
  const int l7 = lane & 7;
  // What only an item with candidates or a tapped one needs is read from the kernel arguments when it is needed: in scalar
  // registers for the whole loop it would crowd out the offsets and records the loop keeps in flight, and above 80 scalar
  // registers a SIMD holds seven waves, not eight.  (Not what EVERY item needs: a scalar load in front of an item's first
  // vector loads is a round trip of its own -- the switches read per item made the launch 14 % slower.)
  const FL_CONST_AS ScanArgs *ka = (const FL_CONST_AS ScanArgs *)__builtin_amdgcn_kernarg_segment_ptr();
  auto kargs = [&]() {
    const FL_CONST_AS ScanArgs *kr = ka;
    asm volatile("" : "+s"(kr));
    return kr;
  };
  auto request_item = [&](int idx) {
    const uint32_t *p = lane < 16 ? (const uint32_t *)(a.items + idx) + lane : (const uint32_t *)(a.enabled + (idx & ~3));
    return *p;
  };
  // the launch's switches in one scalar register: bits 0..7 the mask of the groups with checks, then F_*
  enum : unsigned { F_PRUNE = 0x100u, F_BY_LANE = 0x200u, F_TAPPED = 0x400u, F_TAPS = 0x800u, F_M2 = 0x1000u };
  const unsigned kflags = (a.prune ? F_PRUNE | (a.prune_mid & 0xFFu) | (a.prune_lanes ? F_BY_LANE : 0u) : 0u) | (a.dbg_count ? F_TAPS : 0u) |
                          (a.M > 1 ? F_M2 : 0u);
  uint32_t rec = request_item(it);
  const uint8_t *lm[FL_MAX_MODALITIES];                  // the frame's linear memories
  for (int m = 0; m < FL_MAX_MODALITIES; ++m) lm[m] = a.ws + (size_t)frame * a.ws_stride + a.lm_off[m];
  const float thr100 = a.threshold / 100.f;
  const unsigned lane_off = (unsigned)lane * 16u;

  // One work item.  `return` = on to the wave's next item; every per-item value starts from zero in here.
  auto scan_item = [&](const uint32_t r) {
    // The record stays in its vector register for the whole item and a field is read from it (v_readlane) where it is used:
    // all of them in scalar registers from the start were nine held for modality 1 and the emission while modality 0 runs.
    auto field = [&](int i) {
      uint32_t rr = r;
      asm volatile("" : "+v"(rr));
      return rl(rr, i);
    };
    const int g = (int)rl(r, 8), chunk = (int)(rl(r, 9) & 0xFFFFu), nf_all = (int)(rl(r, 9) >> 16);
    const int j0 = chunk * 1024 + lane * 16;

    // The lane's 16 totals, two per register: a total is at most 4 x 126 = 504, so position 4 q + b sits in the 16-bit half
    // b >> 1 of tp[2 q + (b & 1)] -- the even and the odd bytes of accumulator word q, each added with one 32-bit add that never
    // carries from one half into the other.  Eight registers instead of sixteen are what lets the kernel live in 64.
    uint32_t tp[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) tp[i] = 0;
    auto tot_at = [&](int i) { return (tp[2 * (i >> 2) + (i & 1)] >> (((i >> 1) & 1) * 16)) & 0xFFFFu; };
    auto tot_max = [&]() {                                 // the lane's largest total (v_pk_max_u16)
      u16x2 m = __builtin_bit_cast(u16x2, tp[0]);
#pragma unroll
      for (int i = 1; i < 8; ++i) m = __builtin_elementwise_max(m, __builtin_bit_cast(u16x2, tp[i]));
      return (uint32_t)max(m.x, m.y);
    };
    // Exact pruning between modalities: a feature adds at most 4 to a position (SIMILARITY_LUT's largest entry), so once the
    // largest total of this wave's 1024 positions plus 4 x (the features of the modalities still to come) cannot exceed the
    // coarse threshold, no position of the chunk can become a candidate (`raw > raw_threshold`, linemod.cpp:1490-1492) and the
    // rest of the template's additions have no observable effect: the item ends.  The colour modality comes first and is
    // sparse (gradients only on edges), so on most (template, chunk) pairs the depth modality -- half of the scan's loads -- is
    // never read.  The same bound is checked inside a modality after the 8-feature groups a.prune_mid names (chunks without
    // colour edges stop after 16 features).  Not when the raw maps are tapped (fl_similarity_maps), and FL_SCAN_PRUNE=0
    // switches it off (a.prune).
    const int prune_threshold = (int)(2 * nf_all + thr100 * (2 * nf_all) + 0.5f);   // = raw_threshold below
    // The item's switches live in ONE scalar register and are tested where they are used: as booleans of their own the
    // compiler keeps each in a register pair from here to the item's end.  A tapped item (only a launch with taps can have
    // one) does not prune.
    unsigned flags_ = kflags;
    const unsigned flags_m2 = kflags & F_M2;
    if (kflags & F_TAPS) {
      const FL_CONST_AS ScanArgs *ki = kargs();
      if ((unsigned)(g - ki->dbg_first) < (unsigned)ki->dbg_count) flags_ = F_TAPPED | flags_m2;
    }
    const unsigned flags = flags_;
    auto flag = [&](unsigned bits) {
      unsigned f = flags;
      asm volatile("" : "+s"(f));
      return (f & bits) != 0u;
    };
    // Per lane: the bound is computed for a lane's own 16 positions, so a lane that misses it can stop for itself.  `alive`
    // holds the lanes that still own a reachable position, wave-uniform in a scalar register pair.  A check removes lanes and
    // never brings one back; the item ends when none is left.  The loads of the groups that follow run under
    // alive | alive << 1 (a lane's bytes 16..19 are its upper neighbour's first dword), so a dead lane's accumulators go
    // stale or, next to a live lane, take in a wrong tail: it has no say in later checks and is kept out of the emission.
    // (Even unguarded it could not emit where its tail is right: its stale totals are below its true totals, which are below
    // the threshold.)  Without a.prune_lanes a check keeps every lane or none, the wave-wide rule.
    uint64_t alive = ~0ull;
    auto still = [&](bool reachable) {                     // one check: false = the item is over
      const uint64_t b = __ballot(reachable) & alive;
      alive = flag(F_BY_LANE) || b == 0ull ? b : ~0ull;
      return alive != 0ull;
    };
    [[maybe_unused]] int f_done = 0;                                     // (FL_SCAN_STATS: features added so far)
    FL_SCAN_STAT(0, 1);
    // the group of eight offsets in flight (lanes 0..7) and where in a.offs it is from: the record brings modality 0's first
    uint32_t ov = r;
    int o_at = (rl(r, 12) & 0xFFFFu) ? (int)rl(r, 11) : -1;
    int nf = 0;
#pragma unroll
    for (int m = 0; m < FL_MAX_MODALITIES; ++m) {
      if (m > 0 && !flag(F_M2)) break;                     // (FL_MAX_MODALITIES is 2)
      const uint32_t rN = m == 0 ? rl(r, 12) : field(12 + 3 * m);
      const int P = (int)(m == 0 ? rl(r, 10) : field(10 + 3 * m)), off_begin = (int)(m == 0 ? rl(r, 11) : field(11 + 3 * m));
      const int n_pad = (int)(rN & 0xFFFFu), h_nf = (int)(rN >> 16);
      uint32_t mx_tot = 0;                                 // the lane's largest total of the modalities done
      if (m > 0 && flag(F_PRUNE)) {
        mx_tot = tot_max();
        if (!still((int)mx_tot + 4 * (nf_all - nf) > prune_threshold)) {                      // wave-uniform
          FL_SCAN_STAT(4 + f_done, 1);
          return;
        }
      }
      nf += h_nf;
      if (chunk * 1024 >= P) continue;                    // wave-uniform; lanes past P load along (masked below): the
                                                         // next lane's first dword is this lane's bytes 16..19
      const uint8_t *lm_u = lm[m] + chunk * 1024;         // lane 0's bytes: wave-uniform
      // descriptor over the frame's linear memories from 4 bytes below this chunk on (scalar offsets stay positive)
      const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(lm_u - 4), 0, 0x7FFFFFFF, 0x00020000);
      uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      // A feature's 16 bytes start at an arbitrary byte.  A byte-aligned 16-byte load costs ~2.4x a 4-byte aligned one
      // on gfx950 (tools/probes/ldwidth.hip) and this loop is bound by exactly those loads, so each feature is fetched as
      // an aligned 16 + 4 bytes and shifted into place with four v_alignbyte (the misalignment is wave-uniform).
      // The extra 4 bytes are the next lane's first dword: one DPP wave shift instead of a second vector load; lane 63's
      // come from a wave-uniform address, i.e. a scalar load.
      const unsigned lm_mis = (unsigned)(size_t)lm_u & 3u;  // same for every lane (lane * 16): keep it a scalar
      // Only the lanes whose 16 positions start below template_positions have anything to add (P = 831 of the 1024 positions
      // of a chunk for a 160-pixel template at VGA level 1: 52 of 64 lanes); one more lane stays on because its first dword is
      // the previous lane's bytes 16..19.  The condition is a contiguous lane range, i.e. one EXEC mask around the whole loop --
      // not a select per load (measured in round 1: that serialised the eight loads in flight) -- and the masked lanes' loads
      // are simply not issued: 19 % less L2 traffic.
      const int lanes_on = min(64, ((P - chunk * 1024 + 15) >> 4) + 1);
      const uint64_t lanes_mask = lanes_on >= 64 ? ~0ull : (1ull << lanes_on) - 1ull;
      // behind this modality's last group the next modality's first is requested (whether or not that one then runs)
      auto next_begin = [&]() { return m + 1 < FL_MAX_MODALITIES ? (int)field(11 + 3 * (m + 1)) : off_begin; };
      // The group after the one in work is requested before that one's vector loads are waited for: a group costs one memory
      // round trip, not two.  Past a bank's last group this reads the table's FL_SCAN_OFF_PAD entries; an offset beyond
      // n_pad is never turned into a load.
      uint32_t nxt = 0;
      auto request = [&](int at) { return a.offs[at + l7]; };
      {
        // One piece: N features from offset S0 of `ov` on -- those behind the group's eighth from `ov2`, the group after it --
        // under one EXEC region: the lanes that are alive and their upper neighbours, of those this modality has positions
        // for.  The first eight loads are issued at once; load 8 + u is issued when load u has been added, into the registers
        // that one leaves, so a long piece keeps eight loads in flight and the load registers stay 32.  No branch stands
        // between the loads of a piece.
        // TAIL: lane 63 loads, and its bytes 16..19 have no upper neighbour to come from.  Lane f of the wave then fetches
        // the dword behind lane 63's sixteen bytes of the feature at offset f -- ONE vector load in front of the piece's
        // feature loads (vector loads return in order), taken apart with v_readlane and a select when the feature is
        // added.  The addresses are all over the linear memories; as one scalar load per feature they were misses of the
        // scalar cache, sixteen per item, and sixteen address pairs and results in scalar registers.  They are needed only
        // where lane 63 loads at all: not for a template whose positions end below the chunk's last lane (52 lanes of a
        // bench template), nor once lane 63 is dead.  Elsewhere the lane the DPP has no source for takes a zero.
        auto piece = [&](auto s0_, auto n_, auto tail_, const uint32_t ov2, const uint32_t tv) {
          constexpr int S0 = decltype(s0_)::value, N = decltype(n_)::value, InFlight = N < 8 ? N : 8;
          constexpr bool TAIL = decltype(tail_)::value != 0;
          uint4 v[InFlight];
          unsigned mis_all = 0;                            // the misalignments, two bits each: one scalar register
          auto issue = [&](const int u) {
            unsigned off = rl(S0 + u < 8 ? ov : ov2, (S0 + u) & 7);
            // (a streamed load waits for the sums of the one whose registers it takes: without this the compiler issues the
            // piece's loads all at once, into twice the registers.  The tie is on the scalar offset, not on the vector register
            // it is read from: a copy of that one made under the piece's EXEC would leave out the dead lanes it is read from.)
            if (u >= InFlight) asm("" : "+s"(off) : "v"(a0), "v"(a1), "v"(a2), "v"(a3));
            const unsigned mis_u = (lm_mis + off) & 3u;
            mis_all |= mis_u << (2 * u);
            // buffer_load ... v_lane_off, s[rsrc], s_feature_off offen: the lane's byte offset is one loop-invariant VGPR and
            // the feature's offset a scalar operand -- no per-lane 64-bit address arithmetic (it was 2 of the 10 VALU
            // instructions per feature)
            const u32x4 ld = __builtin_amdgcn_raw_buffer_load_b128(rsrc, lane_off, off - mis_u + 4u, 0);   // 4-byte aligned
            v[u % InFlight] = make_uint4(ld.x, ld.y, ld.z, ld.w);
          };
          auto take = [&](const int u) {
            const unsigned mis_u = (mis_all >> (2 * u)) & 3u;
            const uint4 x = v[u % InFlight];
            uint32_t e = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x.x, 0x130, 0xF, 0xF, true);        // wave_shl:1
            if (TAIL) {
              const uint32_t t = rl(tv, S0 + u);           // (read for the wave, then selected: no branch)
              e = lane == 63 ? t : e;
            }
            a0 += __builtin_amdgcn_alignbyte(x.y, x.x, mis_u);
            a1 += __builtin_amdgcn_alignbyte(x.z, x.y, mis_u);
            a2 += __builtin_amdgcn_alignbyte(x.w, x.z, mis_u);
            a3 += __builtin_amdgcn_alignbyte(e, x.w, mis_u);
          };
#pragma unroll
          for (int u = 0; u < InFlight; ++u) issue(u);
#pragma unroll
          for (int u = 0; u < N; ++u) {
            take(u);
            if (u + InFlight < N) issue(u + InFlight);
          }
        };
        auto add_features = [&](auto s0_, auto n_, const uint32_t ov2) {
          constexpr int S0 = decltype(s0_)::value, N = decltype(n_)::value;
          const uint64_t need = (alive | alive << 1) & lanes_mask;
          FL_SCAN_STAT(1, N);
          FL_SCAN_STAT(2, N * __builtin_popcountll(need));
          const bool tail_on = FL_SCAN_TAIL_ALWAYS || (need >> 63) != 0ull;   // wave-uniform
          // (by lanes S0 .. S0 + N - 1 whether or not they are alive.  A first piece above eight takes lanes 8 .. 15's addresses
          // from `ov2`, the request just issued, and so waits for it in front of the piece: a round trip only a launch in
          // which lane 63 loads pays; not measured apart, profiles/README.md)
          uint32_t tv = 0;
          if (tail_on && (unsigned)(lane - S0) < (unsigned)N) {
            const uint32_t of = lane < 8 ? ov : ov2;
            tv = __builtin_amdgcn_raw_buffer_load_b32(rsrc, of - ((lm_mis + of) & 3u) + 4u + 1024u, 0, 0);
          }
          if (__builtin_amdgcn_inverse_ballot_w64(need)) {
            if (tail_on) piece(s0_, n_, ScanInt<1>{}, ov2, tv);
            else piece(s0_, n_, ScanInt<0>{}, ov2, tv);
            if (S0 == 0) asm volatile("" :: "v"(nxt));     // (keeps the request above in front of this group's loads)
          }
          f_done += N;
        };
        // the same bound inside the modality, `done` of its (padded) features in: the lane's largest byte so far on top of its
        // largest finished total (an over-estimate of its largest partial total, so nothing reachable is ever dropped)
        auto reachable = [&](int done, [[maybe_unused]] bool first_piece) {
          const u16x2 b0 = pk_bytes_max(a0), b1 = pk_bytes_max(a1), b2 = pk_bytes_max(a2), b3 = pk_bytes_max(a3);
          const u16x2 bm = __builtin_elementwise_max(__builtin_elementwise_max(b0, b1), __builtin_elementwise_max(b2, b3));
          const int part = (int)max(bm.x, bm.y);
          const int left = nf_all - nf + max(0, h_nf - done);
          // (every live lane votes: one past this modality's template_positions adds nothing here, its bound is simply
          // generous -- it may still collect from a modality whose template_positions reach further)
          if (still((int)mx_tot + part + 4 * left > prune_threshold)) return true;                // wave-uniform
          FL_SCAN_STAT(4 + f_done, 1);
          if (first_piece) FL_SCAN_STAT(FL_SCAN_STATS_N - 1, 1);
          return false;
        };
        // A modality's first piece has no check inside: FIRST features where the modality has a second group, its first eight
        // where it has not.  No item of the bench bank ends before its ninth feature, so the check behind eight only costs a
        // round trip; 16 end nearly every item after ONE round trip and are the slowest, because every lane then loads what the
        // checks at 12 and 14 would have spared most of them: 12 measure best (profiles/README.md).  Its check, and those of the
        // rest of that group, go by the bit of the group that holds feature FIRST - 1.  Behind it the pieces end at the multiples of STEP; bit g of
        // `mid` enables the checks inside and at the end of group g.
        int k = 0;
        if (n_pad > 0) {
          if (o_at != off_begin) ov = request(off_begin);  // rare: the modality before this one added nothing in this chunk
          const int nxt_at = 8 < n_pad ? off_begin + 8 : next_begin();
          nxt = request(nxt_at);
          if (FIRST > 8 && n_pad > 8) {
            const int nx2_at = 16 < n_pad ? off_begin + 16 : next_begin();   // the group behind the two this piece reads
            const uint32_t nx2 = request(nx2_at);
            add_features(ScanInt<0>{}, ScanInt<FIRST>{}, nxt);
            asm volatile("" :: "v"(nx2));
            if (flag(2u) && !reachable(FIRST, true)) return;
            ov = nxt;
            if (FIRST == 12 && STEP == 2) {
              add_features(ScanInt<4>{}, ScanInt<2>{}, 0u);
              if (flag(2u) && !reachable(14, false)) return;
            } else if (FIRST == 12) {
              add_features(ScanInt<4>{}, ScanInt<4>{}, 0u);
              if (flag(2u) && !reachable(16, false)) return;
            }
            if (FIRST == 14 || (FIRST == 12 && STEP == 2)) {
              add_features(ScanInt<6>{}, ScanInt<2>{}, 0u);
              if (flag(2u) && !reachable(16, false)) return;
            }
            ov = nx2;
            o_at = FL_SCAN_OFFSETS_AHEAD ? nx2_at : -1;
            k = 16;
          } else {
            add_features(ScanInt<0>{}, ScanInt<8>{}, 0u);
            if (flag(1u) && !reachable(8, true)) return;
            ov = nxt;
            o_at = FL_SCAN_OFFSETS_AHEAD ? nxt_at : -1;
            k = 8;
          }
        }
        for (; k < n_pad; k += 8) {
          const int at = off_begin + k;
          if (o_at != at) ov = request(at);                // (FL_SCAN_OFFSETS_AHEAD = 0)
          const int nxt_at = k + 8 < n_pad ? at + 8 : next_begin();
          nxt = request(nxt_at);
          const bool chk = flag(1u << (k >> 3));           // wave-uniform (k < 64: a bit of the mask)
          if (STEP == 8) {
            add_features(ScanInt<0>{}, ScanInt<8>{}, 0u);
            if (chk && !reachable(k + 8, false)) return;
          } else if (STEP == 4) {
            add_features(ScanInt<0>{}, ScanInt<4>{}, 0u);
            if (chk && !reachable(k + 4, false)) return;
            add_features(ScanInt<4>{}, ScanInt<4>{}, 0u);
            if (chk && !reachable(k + 8, false)) return;
          } else {
            add_features(ScanInt<0>{}, ScanInt<2>{}, 0u);
            if (chk && !reachable(k + 2, false)) return;
            add_features(ScanInt<2>{}, ScanInt<2>{}, 0u);
            if (chk && !reachable(k + 4, false)) return;
            add_features(ScanInt<4>{}, ScanInt<2>{}, 0u);
            if (chk && !reachable(k + 6, false)) return;
            add_features(ScanInt<6>{}, ScanInt<2>{}, 0u);
            if (chk && !reachable(k + 8, false)) return;
          }
          ov = nxt;
          o_at = FL_SCAN_OFFSETS_AHEAD ? nxt_at : -1;
        }
      }
      const uint32_t acc[4] = {a0, a1, a2, a3};
      const int nv = P - j0;                          // the lane's positions below template_positions: cells >= it stay 0 (:1160)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = nv - 4 * q;                     // ... of them in word q
        const uint32_t w = acc[q] & (c >= 4 ? ~0u : c <= 0 ? 0u : (1u << (8 * c)) - 1u);
        tp[2 * q] += w & 0x00FF00FFu;
        tp[2 * q + 1] += (w >> 8) & 0x00FF00FFu;
      }
    }
    // (the pyramid's index is read from the record again where it is needed: the record stays in its vector register)
    const int g_end = (int)field(8);
    if (flag(F_TAPPED)) {
      const FL_CONST_AS ScanArgs *kr = kargs();
      const int WH = kr->WH;
      uint16_t *d = kr->dbg + ((size_t)frame * (unsigned)kr->dbg_count + (g_end - kr->dbg_first)) * WH;
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (j0 + i < WH) d[j0 + i] = (uint16_t)tot_at(i);
    }
    // coarse threshold (linemod.cpp:1483-1506), float expression evaluated as written
    const int raw_threshold = (int)(2 * nf + thr100 * (2 * nf) + 0.5f);
    const uint32_t mx = tot_max();
    FL_SCAN_STAT(3, 1);
    if ((int)mx <= raw_threshold || !__builtin_amdgcn_inverse_ballot_w64(alive)) return;   // dead lanes emit nothing (see `alive`)
    const FL_CONST_AS ScanArgs *kr = kargs();
    const int W = kr->W, WH = kr->WH, T = kr->T, cap = kr->cap;
    uint8_t *ws = kr->ws + (size_t)frame * kr->ws_stride;
    int *count = (int *)(ws + kr->off_count);
    FlCand *cand = (FlCand *)(ws + kr->off_cand);
    const int offset = T / 2 + (T % 2 - 1);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int raw = (int)tot_at(i);
      const int j = j0 + i;
      if (raw > raw_threshold && j < WH) {
        const int rr = j / W, c = j - rr * W;
        const int idx = atomicAdd(count, 1);
        if (idx < cap) {
          FlCand cd;
          cd.x = c * T + offset;
          cd.y = rr * T + offset;
          cd.g = g_end;
          cd.sim = (raw * 100.f) / (4 * nf) + 0.5f;                               // :1502
          cand[idx] = cd;
        }
      }
    }
  };

  const int it_end = min(a.n_items, it + a.run * a.item_step);
  for (;;) {
    const uint32_t cur = rec;
    const bool cur_on = ((rl(cur, 16) >> ((it & 3) * 8)) & 0xFFu) != 0;   // wave-uniform: matchClass is not called for a class left out
    // the next item's record and flag are requested before this item's loads (behind the last item: its own again)
    const int nx = it + a.item_step;
    const bool more = nx < it_end;
    const int nxc = more ? nx : it;
    rec = request_item(nxc);
    if (cur_on) scan_item(cur);
    if (!more) break;
    it = nx;
  }
}

// ------------------------------------------------------------------------------------------
// k_refine: one wavefront per candidate.  The 16x16 patch is held as 64 lanes x 4 packed bytes
// (lane = row*4 + column group); each in-bounds feature costs one 4-byte load per lane.
// Slow path of k_refine: 4 consecutive linear-memory positions that run past a row end (xt >= W) or
// past the memory (yt >= H -> next grid cell; past the last one: 0), mapped back to spread pixels.
// Returns the 4 spread bytes packed.
__device__ __noinline__ uint32_t refine_slow_path(const uint8_t *sp, bool in, int xt0, int yt0, int gx, int gy, int T,
                                                  int W, int H, int w)
{
  uint32_t out = 0;
  const int g0 = gy * T + gx, TT = T * T;
  for (int c = 0; c < 4; ++c) {
    int xx = xt0 + c, yy = yt0, gg = g0;
    const int wx = xx >= W ? xx / W : 0;
    xx -= wx * W;
    yy += wx;
    const int wy = yy >= H ? yy / H : 0;
    yy -= wy * H;
    gg += wy;
    if (in && gg < TT) {
      const int ggy = gg / T, ggx = gg - ggy * T;
      out |= (uint32_t)sp[(size_t)(yy * T + ggy) * w + (size_t)(xx * T + ggx)] << (8 * c);
    }
  }
  return out;
}

struct RefineArgs {
  const FlFineHdr *hdr;
  const FlFineFeat *feat;
  uint8_t *ws;
  size_t ws_stride;
  size_t spread_off[FL_MAX_MODALITIES];
  size_t off_count, off_cand;
  int M, Lm1, level, w, h, T, W, H, cap;
  float threshold;
};

// The reference's refinement arithmetic, once for k_refine, k_refine_lds and k_mark_tiles.
// Where a candidate of the coarser level lands on this one: doubled, clamped so that the template and the 16x16 patch of
// T-steps around it stay inside the image, and the patch's first position.
struct RefinePlace { int x, y, offset_x, offset_y; };

__device__ __forceinline__ RefinePlace refine_place(const RefineArgs &a, const FlFineHdr *hdr, int cx, int cy, int T)
{
  const int border = 8 * T;
  const int max_x = a.w - hdr[0].width - border;                        // :1517-1518 (tp[start])
  const int max_y = a.h - hdr[0].height - border;
  RefinePlace p;
  p.x = min(max(cx * 2 + 1, border), max_x);
  p.y = min(max(cy * 2 + 1, border), max_y);
  p.offset_x = (p.x / T - 8) * T;                                       // C division (trunc), :1240
  p.offset_y = (p.y / T - 8) * T;
  return p;
}

// Lane l's feature of a modality in three ints: x | y << 16, qx | qy << 16, gx | gy << 8 | label << 16; zero past the last
// feature.  One coalesced 12-byte load per lane (<= 63 features <= 64 lanes), after which every feature is read out of a
// lane's registers -- no per-feature memory round trip.
struct RefineFeat { int xy, q, g; };

__device__ __forceinline__ RefineFeat refine_load_feat(const FlFineFeat *ff, int feat_count, int lane)
{
  RefineFeat r = {0, 0, 0};
  if (lane < feat_count) {
    const FlFineFeat f = ff[lane];
    r.xy = (int)(uint16_t)f.x | ((int)(uint16_t)f.y << 16);
    r.q = (int)(uint16_t)f.qx | ((int)(uint16_t)f.qy << 16);
    r.g = (int)f.gx | ((int)f.gy << 8) | ((int)f.label << 16);
  }
  return r;
}

// The end of a candidate: the first strict maximum of the 256 totals in row-major order, the position and similarity written
// back into its slot, and the filter.
__device__ __forceinline__ void refine_finish(const RefineArgs &a, uint32_t tot0, uint32_t tot1, uint32_t tot2, uint32_t tot3,
                                              int numFeatures, const RefinePlace &place, int T, int lane, FlCand cd, FlCand *slot)
{
  // first strict maximum in row-major order (:1547-1562): key = score << 8 | (255 - pos)
  const int pos = (lane >> 2) * 16 + (lane & 3) * 4;
  uint32_t key = (tot0 << 8) | (uint32_t)(255 - pos);
  key = max(key, (tot1 << 8) | (uint32_t)(254 - pos));
  key = max(key, (tot2 << 8) | (uint32_t)(253 - pos));
  key = max(key, (tot3 << 8) | (uint32_t)(252 - pos));
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, s, 64));
  const int best_score = (int)(key >> 8);
  int best_r = -1, best_c = -1;                                         // Q4: all-zero patch
  if (best_score > 0) {
    const int bp = 255 - (int)(key & 0xFFu);
    best_r = bp >> 4;
    best_c = bp & 15;
  }
  if (lane == 0) {
    const int offset = T / 2 + (T % 2 - 1);
    cd.x = (place.x / T - 8 + best_c) * T + offset;                     // :1564-1566
    cd.y = (place.y / T - 8 + best_r) * T + offset;
    cd.sim = (best_score * 100.f) / (4 * numFeatures);
    if (cd.sim < a.threshold) cd.g = -1;                                // MatchPredicate :1447
    *slot = cd;
  }
}

#ifndef FL_REFINE_WPE
#define FL_REFINE_WPE 6           // waves per SIMD; measured (ms per 1280 frames): 4: 0.92, 5 (the compiler's choice): 0.80, 6: 0.76, 8: 1.03
#endif
__attribute__((amdgpu_waves_per_eu(FL_REFINE_WPE, FL_REFINE_WPE)))
__global__ __launch_bounds__(256) void k_refine(RefineArgs a)
{
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int frame = blockIdx.y;
  uint8_t *ws = a.ws + (size_t)frame * a.ws_stride;
  const int n = min(*(const int *)(ws + a.off_count), a.cap);
  FlCand *cand = (FlCand *)(ws + a.off_cand);
  const int row = lane >> 2, col4 = (lane & 3) * 4;
  const int T = a.T, W = a.W, H = a.H;
  const size_t lane_off = (size_t)row * T * a.w + (size_t)col4 * T;
  for (int ci = blockIdx.x * 4 + wave; ci < n; ci += gridDim.x * 4) {
    const FlCand cd = cand[ci];
    const int g = __builtin_amdgcn_readfirstlane(cd.g);
    if (g < 0) continue;
    const FlFineHdr *hdr = a.hdr + ((size_t)g * a.Lm1 + a.level) * a.M;
    const RefinePlace place = refine_place(a, hdr, __builtin_amdgcn_readfirstlane(cd.x), __builtin_amdgcn_readfirstlane(cd.y), T);
    uint32_t tot0 = 0, tot1 = 0, tot2 = 0, tot3 = 0;                    // u16 totals of 4 positions
    int numFeatures = 0;
    const int offx_t = place.offset_x / T, offy_t = place.offset_y / T;
    for (int m = 0; m < a.M; ++m) {
      const FlFineHdr h = hdr[m];
      numFeatures += h.feat_count;
      const uint8_t *sp = ws + a.spread_off[m];
      const RefineFeat feat = refine_load_feat(a.feat + h.feat_begin, h.feat_count, lane);
      uint32_t acc = 0;
      // The reference reads 16 rows x 16 bytes of the feature's linear memory at stride W starting at
      // lm_index (:1260-1297).  Here the same linear index is mapped back to the pixel it was
      // linearised from -- grid cell g, position k = yt*W + xt -> (yt*T + g/T, xt*T + g%T) -- and the
      // response LUT is evaluated on the spread byte.  Running past a row (xt >= W) or past the
      // memory (yt >= H -> next grid cell, past the last one: 0) follows the linear layout exactly.
      // Every feature is broadcast from the lane that holds it; then 8 features x 4 positions = 32
      // independent byte loads per step.  k_refine_lds walks the same way (its else branch): shared as one
      // function template, the walk compiled differently (the LUT as selects) and both kernels measured
      // slower (profiles/README.md), so each kernel keeps its own.
      for (int k = 0; k < h.feat_count; k += 8) {
        uint32_t b[8][4];
        int lab[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = min(k + u, h.feat_count - 1);                    // wave-uniform
          const int xy = __shfl(feat.xy, idx, 64), qq = __shfl(feat.q, idx, 64), gl = __shfl(feat.g, idx, 64);
          const int fx = (int)(int16_t)(xy & 0xFFFF) + place.offset_x, fy = (int)(int16_t)(xy >> 16) + place.offset_y;
          const bool in = (k + u < h.feat_count) && fx >= 0 && fy >= 0 && fx < a.w && fy < a.h;   // :1257
          lab[u] = (gl >> 16) & 0xFF;
          // offsets are multiples of T, so (f + offset) mod T and div T follow from the stored residues
          const int gx = gl & 0xFF, gy = (gl >> 8) & 0xFF;
          const int lm_x = (int)(int16_t)(qq & 0xFFFF) + offx_t, lm_y = (int)(int16_t)(qq >> 16) + offy_t;
          if (in && lm_x + 15 < W && lm_y + 15 < H) {                      // wave-uniform: the usual case
            // the 16x16 patch stays inside its linear memory: position (row, col4 + c) is simply the
            // pixel (fy + row*T, fx + (col4 + c)*T)
            // The lane's four positions are T bytes apart: for the usual T one (or two) 16-byte loads replace four
            // byte loads -- the stage is bound by vector-memory instructions, 8 features x 4 in flight per step.
            const uint8_t *p0 = sp + (size_t)(fy * a.w + fx) + lane_off;
            if (T == 5) {
              const uint4 v = ld16(p0);                                     // bytes 0, 5, 10, 15
              b[u][0] = v.x & 0xFFu; b[u][1] = (v.y >> 8) & 0xFFu; b[u][2] = (v.z >> 16) & 0xFFu; b[u][3] = v.w >> 24;
            } else if (T == 4) {
              const uint4 v = ld16(p0);                                     // bytes 0, 4, 8, 12
              b[u][0] = v.x & 0xFFu; b[u][1] = v.y & 0xFFu; b[u][2] = v.z & 0xFFu; b[u][3] = v.w & 0xFFu;
            } else if (T == 8) {
              const uint4 v0 = ld16(p0), v1 = ld16(p0 + 16);                // bytes 0, 8 | 16, 24
              b[u][0] = v0.x & 0xFFu; b[u][1] = v0.z & 0xFFu; b[u][2] = v1.x & 0xFFu; b[u][3] = v1.z & 0xFFu;
            } else {
#pragma unroll
              for (int c = 0; c < 4; ++c) b[u][c] = p0[c * T];
            }
          } else {
            // rare: the patch leaves its linear memory (or the feature is out of the image); kept out
            // of line so the unrolled step stays small (instruction-cache footprint)
            uint32_t r4 = refine_slow_path(sp, in, lm_x + col4, lm_y + row, gx, gy, T, W, H, a.w);
#pragma unroll
            for (int c = 0; c < 4; ++c) b[u][c] = (r4 >> (8 * c)) & 0xFFu;
          }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          uint32_t packed = 0;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const unsigned bb = b[u][c] | (b[u][c] << 8);
            const unsigned rot = (bb >> lab[u]) & 0xFFu;
            const unsigned r = (rot & 1u) ? 4u : ((rot & 0x82u) ? 2u : ((rot & 0x44u) ? 1u : 0u));
            packed |= r << (8 * c);
          }
          acc += packed;                                                   // 4 packed u8 adds
        }
      }
      tot0 += acc & 0xFFu;
      tot1 += (acc >> 8) & 0xFFu;
      tot2 += (acc >> 16) & 0xFFu;
      tot3 += acc >> 24;
    }
    refine_finish(a, tot0, tot1, tot2, tot3, numFeatures, place, T, lane, cd, cand + ci);
  }
}

// ------------------------------------------------------------------------------------------
// k_refine_lds: k_refine's arithmetic on spread bytes staged in LDS, one 256-thread workgroup per frame.  A frame's
// candidates sit on a few objects and their windows are nearly the same region, which k_refine fetches again for every
// candidate, a cache line per lane.  Here the candidates are taken FL_REFINE_BLOCK at a time, ordered by location (a
// rank sort of (x / T, y / T), column-major, one candidate per thread; erased ones last), and cut into groups: the longest
// run whose united rectangle fits the window budget (fl_refine_plan, at most FL_REFINE_GROUP_MAX).  Per group and
// modality the rectangle is staged with coalesced 16-byte loads, then the four waves take the group's candidates
// round-robin.  Each candidate is refined on its own and written back in place, so neither the order nor the grouping
// can change a result.  What k_refine reads through refine_slow_path is read from global memory here too.
// The resources are those one retired ICP workgroup leaves on a CU: 256 threads, <= 128 VGPRs,
// <= 70 KB of LDS.
static_assert(FL_MAX_MODALITIES == 2, "the first modality's packed sums wait in LDS while the second is staged");
static_assert(FL_REFINE_LDS_BYTES + 4 * 64 * FL_REFINE_GROUP_MAX + 10 * FL_REFINE_BLOCK + 64 <= 70 * 1024, "LDS beside three ICP workgroups");

// 16 bytes at p of which only those before `end` exist
__device__ __noinline__ uint4 refine_stage_tail(const uint8_t *p, const uint8_t *end)
{
  uint32_t v[4] = {0, 0, 0, 0};
  for (int i = 0; i < 16; ++i)
    if (p + i < end) v[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// refine_resp4 (above, beside k_build_lm): the four responses of a lane to one feature, on its four spread bytes packed in a
// dword.  The label is the same for the whole wave.

#ifdef FL_REFINE_STATS
// development aid: per launch {frames with a candidate, groups, bytes staged (all modalities), candidates refined}, printed by the
// launcher after a stream synchronisation (tools/dev/README.md)
__device__ unsigned long long d_refine_stats[4];
#endif

template <int TT>
__attribute__((amdgpu_num_vgpr(128)))
__global__ __launch_bounds__(256) void k_refine_lds(RefineArgs a, const FlFineBox *box, int budget, uint32_t qmask)
{
  __shared__ __attribute__((aligned(16))) uint8_t s_win[FL_REFINE_LDS_BYTES];
  // the block's keys while it is ordered, then the groups' packed sums of modality 0 (group slot, lane)
  __shared__ uint32_t s_keyacc[64 * FL_REFINE_GROUP_MAX > FL_REFINE_BLOCK ? 64 * FL_REFINE_GROUP_MAX : FL_REFINE_BLOCK];
  __shared__ int16_t s_rect[4 * FL_REFINE_BLOCK];          // in processing order
  __shared__ uint16_t s_idx[FL_REFINE_BLOCK];              // processing order -> index in the block
  __shared__ int s_plan[5];                                // the group: length, united rectangle
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  uint8_t *ws = a.ws + (size_t)blockIdx.x * a.ws_stride;
  const int n = min(*(const int *)(ws + a.off_count), a.cap);
  FlCand *cand = (FlCand *)(ws + a.off_cand);
  const int row = lane >> 2, col4 = (lane & 3) * 4;
  const int T = TT ? TT : a.T, W = a.W, H = a.H;
  for (int blk = 0; blk < n; blk += FL_REFINE_BLOCK) {
    const int nb = min(FL_REFINE_BLOCK, n - blk);
    // this thread's candidate: where it is, and the rectangle its in-bounds patches lie in
    uint32_t key = 0xFFFFFFFFu;
    FlRect rc = {0, 0, -1, -1};
    if (tid < nb) {
      const FlCand cd = cand[blk + tid];
      if (cd.g >= 0) {
        const size_t hi = ((size_t)cd.g * a.Lm1 + a.level) * a.M;
        const RefinePlace place = refine_place(a, a.hdr + hi, cd.x, cd.y, T);
        const int offset_x = place.offset_x, offset_y = place.offset_y;
        FlRect b = {0, 0, -1, -1};
        for (int m = 0; m < a.M; ++m) {
          const FlFineBox fb = box[hi + m];
          const FlRect one = {fb.x0, fb.y0, fb.x1, fb.y1};
          b = fl_rect_union(b, one);
        }
        if (b.x1 >= b.x0) {
          rc.x0 = max(0, b.x0 + offset_x);
          rc.y0 = max(0, b.y0 + offset_y);
          rc.x1 = min(a.w - 1, b.x1 + offset_x + 15 * T);
          rc.y1 = min(a.h - 1, b.y1 + offset_y + 15 * T);
          if (rc.x1 < rc.x0 || rc.y1 < rc.y0) rc = FlRect{0, 0, -1, -1};
        }
        key = ((uint32_t)((place.x / T + 0x4000) & 0x7FFF) << 16) | (uint32_t)((place.y / T + 0x4000) & 0x7FFF);
      }
    }
    s_keyacc[tid] = key;
    __syncthreads();
    if (tid < nb) {
      int rank = 0;
      for (int u = 0; u < nb; ++u) {
        const uint32_t k = s_keyacc[u];
        rank += (k < key || (k == key && u < tid)) ? 1 : 0;
      }
      s_idx[rank] = (uint16_t)tid;
      s_rect[4 * rank + 0] = (int16_t)rc.x0;
      s_rect[4 * rank + 1] = (int16_t)rc.y0;
      s_rect[4 * rank + 2] = (int16_t)rc.x1;
      s_rect[4 * rank + 3] = (int16_t)rc.y1;
    }
    const int nvalid = __syncthreads_count(key != 0xFFFFFFFFu);
    for (int gs = 0; gs < nvalid;) {
      if (tid == 0) {
        FlRect u;
        s_plan[0] = fl_refine_plan(s_rect + 4 * gs, nvalid - gs, FL_REFINE_GROUP_MAX, (long)budget, qmask, &u);
        s_plan[1] = u.x0 & ~3;
        s_plan[2] = u.y0;
        s_plan[3] = u.x1;
        s_plan[4] = u.y1;
      }
      __syncthreads();
      const int len = s_plan[0], ux0 = s_plan[1], uy0 = s_plan[2], ux1 = s_plan[3], uy1 = s_plan[4];
      const bool have = ux1 >= ux0;
      const int pitch = have ? fl_refine_pitch(ux1 - ux0 + 1, qmask) : 16;
      const int lane_lds = row * T * pitch + col4 * T;
#ifdef FL_REFINE_STATS
      if (tid == 0) {
        if (blk == 0 && gs == 0) atomicAdd(&d_refine_stats[0], 1ull);
        atomicAdd(&d_refine_stats[1], 1ull);
        atomicAdd(&d_refine_stats[2], have ? (unsigned long long)a.M * pitch * (uy1 - uy0 + 1) : 0ull);
        atomicAdd(&d_refine_stats[3], (unsigned long long)len);
      }
#endif
      for (int m = 0; m < a.M; ++m) {
        const uint8_t *sp = ws + a.spread_off[m];
        if (have) {
          // chunk c = 16 bytes of window row c / cpr; it lands at LDS byte 16 c.  Four loads are in flight per thread before the
          // first store.  Nothing before the image is read (coordinates are not negative); what would lie past its last byte is
          // not read either.
          const int cpr = pitch >> 4, total = (uy1 - uy0 + 1) * cpr;
          const uint8_t *end = sp + (size_t)a.w * a.h;
          for (int c0 = tid; c0 < total; c0 += 4 * 256) {
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int c = c0 + u * 256;
              if (c < total) {
                const int r = c / cpr, j = c - r * cpr;
                const uint8_t *p = sp + (size_t)(uy0 + r) * a.w + (size_t)(ux0 + 16 * j);
                v[u] = p + 16 <= end ? ld16(p) : refine_stage_tail(p, end);
              }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const int c = c0 + u * 256;
              if (c < total) *(uint4 *)(s_win + 16 * (size_t)c) = v[u];
            }
          }
        }
        __syncthreads();
        for (int j = wave; j < len; j += 4) {
          const int ci = blk + s_idx[gs + j];
          const FlCand cd = cand[ci];
          const int g = __builtin_amdgcn_readfirstlane(cd.g);
          const FlFineHdr *hdr = a.hdr + ((size_t)g * a.Lm1 + a.level) * a.M;
          const RefinePlace place = refine_place(a, hdr, __builtin_amdgcn_readfirstlane(cd.x), __builtin_amdgcn_readfirstlane(cd.y), T);
          const int offx_t = place.offset_x / T, offy_t = place.offset_y / T;
          const FlFineHdr h = hdr[m];
          const int feat_count = __builtin_amdgcn_readfirstlane(h.feat_count);
          uint32_t acc = 0;
          // lane l holds feature l; a feature is then read out of that lane into scalar registers (no LDS round trip between the
          // window reads of one feature and the next: a step's 32 byte reads are in flight together), so its address arithmetic
          // and its tests are scalar work
          const RefineFeat feat = refine_load_feat(a.feat + h.feat_begin, feat_count, lane);
          // The usual candidate: every patch stays inside the image and its linear memory, which the modality's box tells
          // without looking at a feature.  Lane l then holds its feature's offset in the window, and a feature costs two lane
          // reads, one address add, four byte reads and refine_resp4.
          const FlFineBox fb = box[((size_t)g * a.Lm1 + a.level) * a.M + m];
          const bool usual = fb.x0 + place.offset_x >= 0 && fb.y0 + place.offset_y >= 0 && fb.x1 + place.offset_x + 16 * T <= a.w &&
                             fb.y1 + place.offset_y + 16 * T <= a.h && feat_count <= 64 && __all(((feat.g >> 16) & 0xFF) < 8);
          if (__builtin_amdgcn_readfirstlane((int)usual)) {
            const int f_off = ((feat.xy >> 16) + place.offset_y - uy0) * pitch + ((int)(int16_t)(feat.xy & 0xFFFF) + place.offset_x - ux0);
            for (int k = 0; k < feat_count; k += 8) {
              uint32_t b[8][4];
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const uint8_t *p0 = s_win + __builtin_amdgcn_readlane(f_off, min(k + u, feat_count - 1)) + lane_lds;
#pragma unroll
                for (int c = 0; c < 4; ++c) b[u][c] = p0[c * T];
              }
#pragma unroll
              for (int u = 0; u < 8; ++u) {
                const int lab = (__builtin_amdgcn_readlane(feat.g, min(k + u, feat_count - 1)) >> 16) & 0xFF;
                const uint32_t r = refine_resp4(b[u][0] | (b[u][1] << 8) | (b[u][2] << 16) | (b[u][3] << 24), lab);
                acc += k + u < feat_count ? r : 0u;                              // 4 packed u8 adds
              }
            }
          } else
          for (int k = 0; k < feat_count; k += 8) {
            uint32_t b[8][4];
            int lab[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const int idx = min(k + u, feat_count - 1);
              const int xy = __builtin_amdgcn_readlane(feat.xy, idx), qq = __builtin_amdgcn_readlane(feat.q, idx), gl = __builtin_amdgcn_readlane(feat.g, idx);
              const int fx = (int)(int16_t)(xy & 0xFFFF) + place.offset_x, fy = (int)(int16_t)(xy >> 16) + place.offset_y;
              const bool in = (k + u < feat_count) && fx >= 0 && fy >= 0 && fx < a.w && fy < a.h;   // :1257
              lab[u] = (gl >> 16) & 0xFF;
              const int gx = gl & 0xFF, gy = (gl >> 8) & 0xFF;
              const int lm_x = (int)(int16_t)(qq & 0xFFFF) + offx_t, lm_y = (int)(int16_t)(qq >> 16) + offy_t;
              if (in && lm_x + 15 < W && lm_y + 15 < H) {                      // wave-uniform: the usual case
                // position (row, col4 + c) is the pixel (fy + row*T, fx + (col4 + c)*T), inside the staged rectangle
                const uint8_t *p0 = s_win + ((fy - uy0) * pitch + (fx - ux0)) + lane_lds;
#pragma unroll
                for (int c = 0; c < 4; ++c) b[u][c] = p0[c * T];
              } else {
                uint32_t r4 = refine_slow_path(sp, in, lm_x + col4, lm_y + row, gx, gy, T, W, H, a.w);
#pragma unroll
                for (int c = 0; c < 4; ++c) b[u][c] = (r4 >> (8 * c)) & 0xFFu;
              }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              uint32_t packed = 0;
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                const unsigned bb = b[u][c] | (b[u][c] << 8);
                const unsigned rot = (bb >> lab[u]) & 0xFFu;
                const unsigned r = (rot & 1u) ? 4u : ((rot & 0x82u) ? 2u : ((rot & 0x44u) ? 1u : 0u));
                packed |= r << (8 * c);
              }
              acc += packed;                                                   // 4 packed u8 adds
            }
          }
          if (m + 1 < a.M) {
            s_keyacc[j * 64 + lane] = acc;                                     // read back by this lane only
            continue;
          }
          const uint32_t acc0 = a.M > 1 ? s_keyacc[j * 64 + lane] : 0u;
          const uint32_t tot0 = (acc0 & 0xFFu) + (acc & 0xFFu), tot1 = ((acc0 >> 8) & 0xFFu) + ((acc >> 8) & 0xFFu);
          const uint32_t tot2 = ((acc0 >> 16) & 0xFFu) + ((acc >> 16) & 0xFFu), tot3 = (acc0 >> 24) + (acc >> 24);
          int numFeatures = 0;
          for (int mm = 0; mm < a.M; ++mm) numFeatures += hdr[mm].feat_count;
          refine_finish(a, tot0, tot1, tot2, tot3, numFeatures, place, T, lane, cd, cand + ci);
        }
        __syncthreads();
      }
      gs += len;
    }
  }
}

// k_mark_tiles (lazy fine levels): which 60x60 tiles of level a.level will k_refine read?  One workgroup per
// frame, one wave per candidate, lane = feature, with k_refine's own arithmetic (placement: refine_place): a feature whose 16x16 patch stays
// inside its linear memory reads the spread bytes (fy + r*T, fx + c*T), r, c < 16; the candidate's features span a
// rectangle, its tiles go into bitmap 0 ("spread bytes read") and the tiles of the rectangle grown by T-1 to the
// right and below into bitmap 1 ("quantised pixels those spreads are made of").  Anything unusual -- a feature
// outside the image, a patch that leaves its linear memory and wraps (Q1/Q2) -- marks the whole frame, which is
// the eager computation.
__global__ __launch_bounds__(256) void k_mark_tiles(RefineArgs a, size_t off_tiles)
{
  __shared__ uint32_t bm[2][FL_TILE_WORDS];
  __shared__ int rlo[2][32 * FL_TILE_WORDS], rhi[2][32 * FL_TILE_WORDS];
  __shared__ int s_all;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int frame = blockIdx.x;
  uint8_t *ws = a.ws + (size_t)frame * a.ws_stride;
  for (int i = threadIdx.x; i < 2 * FL_TILE_WORDS; i += 256) bm[0][i] = 0;
  for (int i = threadIdx.x; i < 2 * 32 * FL_TILE_WORDS; i += 256) { rlo[0][i] = 0xFFFF; rhi[0][i] = 0; }
  if (threadIdx.x == 0) s_all = 0;
  __syncthreads();
  const int n = min(*(const int *)(ws + a.off_count), a.cap);
  const FlCand *cand = (const FlCand *)(ws + a.off_cand);
  const int T = a.T, W = a.W, H = a.H;
  const int nstrips = (a.w + FL_TILE - 1) / FL_TILE, nchunks = (a.h + FL_TILE - 1) / FL_TILE;
  for (int ci = wave; ci < n; ci += 4) {
    const FlCand cd = cand[ci];
    const int g = __builtin_amdgcn_readfirstlane(cd.g);
    if (g < 0) continue;
    const FlFineHdr *hdr = a.hdr + ((size_t)g * a.Lm1 + a.level) * a.M;
    const RefinePlace place = refine_place(a, hdr, __builtin_amdgcn_readfirstlane(cd.x), __builtin_amdgcn_readfirstlane(cd.y), T);
    const int offx_t = place.offset_x / T, offy_t = place.offset_y / T;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    bool odd = false;
    for (int m = 0; m < a.M; ++m) {
      const FlFineHdr h = hdr[m];
      if (lane < h.feat_count) {
        const FlFineFeat f = a.feat[h.feat_begin + lane];
        const int fx = (int)f.x + place.offset_x, fy = (int)f.y + place.offset_y;
        const bool in = fx >= 0 && fy >= 0 && fx < a.w && fy < a.h;
        const int lm_x = (int)f.qx + offx_t, lm_y = (int)f.qy + offy_t;
        if (in && lm_x + 15 < W && lm_y + 15 < H) {
          x0 = min(x0, fx); y0 = min(y0, fy);
          x1 = max(x1, fx + 15 * T); y1 = max(y1, fy + 15 * T);
        } else {
          odd = true;
        }
      }
      if (h.feat_count > 64) odd = true;                    // k_refine keeps one feature per lane
    }
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) {
      x0 = min(x0, __shfl_xor(x0, sft, 64)); y0 = min(y0, __shfl_xor(y0, sft, 64));
      x1 = max(x1, __shfl_xor(x1, sft, 64)); y1 = max(y1, __shfl_xor(y1, sft, 64));
    }
    if (__any(odd) || x1 >= a.w || y1 >= a.h) { if (lane == 0) s_all = 1; continue; }
    if (x1 < 0) continue;                                  // no feature at all
#pragma unroll
    for (int kind = 0; kind < 2; ++kind) {
      const int grow = kind ? T - 1 : 0;
      const int yb = min(a.h - 1, y1 + grow);
      const int s0 = x0 / FL_TILE, s1 = min(a.w - 1, x1 + grow) / FL_TILE, c0 = y0 / FL_TILE, c1 = yb / FL_TILE;
      const int ns = s1 - s0 + 1, nt = ns * (c1 - c0 + 1);
      for (int t = lane; t < nt; t += 64) {
        const int c = t / ns, tile = (c0 + c) * nstrips + s0 + (t - c * ns);
        atomicOr(&bm[kind][tile >> 5], 1u << (tile & 31));
        atomicMin(&rlo[kind][tile], max(y0, (c0 + c) * FL_TILE));
        atomicMax(&rhi[kind][tile], min(yb, (c0 + c) * FL_TILE + FL_TILE - 1));
      }
    }
  }
  __syncthreads();
  uint32_t *out = (uint32_t *)(ws + off_tiles) + (size_t)a.level * FL_TILE_BLOCK_WORDS;
  const int ntiles = nstrips * nchunks;
  const bool all = s_all != 0;
  for (int i = threadIdx.x; i < 2 * FL_TILE_WORDS; i += 256) {
    const int wd = i % FL_TILE_WORDS;
    uint32_t v = bm[0][i];
    if (all) v = wd * 32 + 32 <= ntiles ? 0xFFFFFFFFu : (wd * 32 < ntiles ? (1u << (ntiles - wd * 32)) - 1u : 0u);
    out[i] = v;
  }
  for (int i = threadIdx.x; i < 2 * 32 * FL_TILE_WORDS; i += 256) {
    uint32_t v = ((uint32_t)rlo[0][i] << 16) | (uint32_t)rhi[0][i];
    if (all) v = (uint32_t)(a.h - 1);                       // rows 0 .. h-1: the consumers clip to their own tile
    out[2 * FL_TILE_WORDS + i] = v;
  }
}

// ------------------------------------------------------------------------------------------
// k_sort_unique: one 1024-thread workgroup per frame.  128-bit keys, sorted descending:
//   hi = similarity bits << 32 | (0x7FFFFFFF - template_id)     (Match::operator<, linemod.hpp:262)
//   lo = (0xFFFF - class) << 32 | (0xFFFF - (y+32768)) << 16 | (0xFFFF - (x+32768))
// lo only fixes the order std::sort leaves unspecified (Q5).  Bitonic network in LDS when the
// padded count fits, otherwise in the frame's key scratch in HBM (same code, block-level sync).
struct Key128 { unsigned long long hi, lo; };
__device__ __forceinline__ bool key_gt(const Key128 &a, const Key128 &b) { return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo); }

struct SortArgs {
  const FlPyrInfo *pyr;
  uint8_t *ws;
  size_t ws_stride;
  size_t off_count, off_cand, off_keys, off_match;
  int cap;
};

#define FL_SORT_LDS_KEYS 2048

template <bool IN_LDS>
__device__ void bitonic_desc(Key128 *k, int n2)
{
  for (int size = 2; size <= n2; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (n2 >> 1); t += blockDim.x) {
        const int i = 2 * t - (t & (stride - 1));
        const int j = i + stride;
        const bool desc = ((i & size) == 0);
        Key128 a = k[i], b = k[j];
        if (key_gt(b, a) == desc) { k[i] = b; k[j] = a; }
      }
    }
  __syncthreads();
}

__global__ __launch_bounds__(1024) void k_sort_unique(SortArgs a)
{
  __shared__ Key128 lds_keys[FL_SORT_LDS_KEYS];
  __shared__ int s_n, s_scan[1024], s_base;
  const int frame = blockIdx.x;
  uint8_t *ws = a.ws + (size_t)frame * a.ws_stride;
  int *counters = (int *)(ws + a.off_count);      // [0] candidates, [1] matches out, [2] overflow flag
  const int n_raw = *counters;
  const int n = min(n_raw, a.cap);
  const FlCand *cand = (const FlCand *)(ws + a.off_cand);
  Key128 *gkeys = (Key128 *)(ws + a.off_keys);
  fl_match *out = (fl_match *)(ws + a.off_match);
  if (threadIdx.x == 0) { s_n = 0; s_base = 0; }
  __syncthreads();
  // gather live candidates (order irrelevant before the sort)
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const FlCand c = cand[i];
    if (c.g >= 0) {
      const FlPyrInfo pi = a.pyr[c.g];
      Key128 k;
      k.hi = ((unsigned long long)__float_as_uint(c.sim) << 32) | (unsigned)(0x7FFFFFFF - pi.template_id);
      k.lo = ((unsigned long long)(0xFFFF - pi.class_idx) << 32) | ((unsigned long long)(0xFFFF - (c.y + 32768)) << 16) |
             (unsigned long long)(0xFFFF - (c.x + 32768));
      const int slot = atomicAdd(&s_n, 1);
      gkeys[slot] = k;
    }
  }
  __syncthreads();
  const int nl = s_n;
  int n2 = 1;
  while (n2 < nl) n2 <<= 1;
  const Key128 zero = {0ull, 0ull};
  Key128 *keys;
  if (n2 <= FL_SORT_LDS_KEYS) {
    for (int i = threadIdx.x; i < n2; i += blockDim.x) lds_keys[i] = i < nl ? gkeys[i] : zero;
    keys = lds_keys;
    bitonic_desc<true>(keys, n2);
  } else {
    for (int i = nl + threadIdx.x; i < n2; i += blockDim.x) gkeys[i] = zero;
    keys = gkeys;
    bitonic_desc<false>(keys, n2);
  }
  // std::unique with Match::operator== (x, y, similarity, class; template_id ignored) + compaction
  for (int base = 0; base < nl; base += blockDim.x) {
    const int i = base + threadIdx.x;
    int flag = 0;
    Key128 k = zero;
    if (i < nl) {
      k = keys[i];
      if (i == 0) flag = 1;
      else {
        const Key128 p = keys[i - 1];
        flag = !((k.hi >> 32) == (p.hi >> 32) && k.lo == p.lo);
      }
    }
    s_scan[threadIdx.x] = flag;
    __syncthreads();
    for (int d = 1; d < (int)blockDim.x; d <<= 1) {      // Hillis-Steele inclusive scan
      int v = threadIdx.x >= d ? s_scan[threadIdx.x - d] : 0;
      __syncthreads();
      s_scan[threadIdx.x] += v;
      __syncthreads();
    }
    const int pos = s_base + s_scan[threadIdx.x] - flag;
    if (flag) {
      fl_match m;
      m.similarity = __uint_as_float((unsigned)(k.hi >> 32));
      m.template_id = 0x7FFFFFFF - (int)(k.hi & 0xFFFFFFFFu);
      m.class_idx = 0xFFFF - (int)(k.lo >> 32);
      m.y = (0xFFFF - (int)((k.lo >> 16) & 0xFFFF)) - 32768;
      m.x = (0xFFFF - (int)(k.lo & 0xFFFF)) - 32768;
      out[pos] = m;
    }
    __syncthreads();
    if (threadIdx.x == blockDim.x - 1) s_base += s_scan[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counters[1] = s_base;
    counters[2] = n_raw > a.cap ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------
// Work items a wave of k_scan walks: FL_SCAN_RUN_AUTO where the launch then still has FL_SCAN_FILL times the waves the device
// holds at once, else half of that, and so on down to 1 (so the small-batch launches are what they were: one frame of 2000
// templates is 2000 items for 1024 SIMDs).  Option scan_run != 0 forces a length.
#ifndef FL_SCAN_RUN_AUTO
#define FL_SCAN_RUN_AUTO 8
#endif
#ifndef FL_SCAN_STRIDED
#define FL_SCAN_STRIDED 1
#endif
#define FL_SCAN_FILL 4
#define FL_SCAN_FILL_WAVES 6      // (the pruned scan's waves per SIMD when the run lengths were measured: the small batches keep them)
static int fl_scan_run(const fl_context *ctx, int items, int n_frames)
{
  if (ctx->opt.scan_run) return (int)ctx->opt.scan_run;
  const long need = (long)FL_SCAN_FILL * ctx->cus * 4 * (ctx->opt.scan_prune ? FL_SCAN_FILL_WAVES : FL_SCAN_WPE);
  int run = FL_SCAN_RUN_AUTO;
  while (run > 1 && (long)n_frames * ((items + run - 1) / run) < need) run /= 2;
  return run;
}

// Feature loads between two of k_scan's checks behind a modality's first eight (the STEP the kernel is built for).  A finer step
// trades a dependent round trip for load instructions not issued, which pays where the launch keeps every CU's vector memory
// path busy: from FL_SCAN_STEP_FRAMES frames on (measured at 256 and 4096); below, where an item costs its round trips and
// nothing else, groups of eight (the scan of 1 and of 64 frames: 0.017 against 0.020 ms, 0.111 against 0.113 ms,
// profiles/README.md).  Option scan_prune_step != 0 forces a step.
#ifndef FL_SCAN_STEP_FRAMES
#define FL_SCAN_STEP_FRAMES 256
#endif
static int fl_scan_step(const fl_context *ctx, int n_frames)
{
  if (ctx->opt.scan_prune_step) return (int)ctx->opt.scan_prune_step;
  return n_frames >= FL_SCAN_STEP_FRAMES ? FL_SCAN_STEP : 8;
}

// Features of a modality's first piece (the FIRST the kernel is built for).  A longer piece pays where the check behind eight
// features ends no item: where a position may lose more than seven features' worth of points (4 nf - raw_threshold > 28, from
// the bank's typical feature count and the call's threshold), so that only a lane that has scored next to nothing goes there.
// Measured both ways (profiles/README.md): the 62-feature bench bank at 75 % may lose 31 points and gains 5 % with 12; the
// 30-feature coarsest level of the three-level bank may lose 15, most of its items end behind eight features, and 12 cost it
// 20 % of the scan.  The boundary at 28 lies between these two measured points and has not been measured itself.
// FL_SCAN_FIRST from FL_SCAN_STEP_FRAMES frames on, eight below.  Option scan_first != 0 forces a length.
#ifndef FL_SCAN_FIRST
#define FL_SCAN_FIRST 12
#endif
static int fl_scan_first(const fl_detector *det, int n_frames, float threshold)
{
  const fl_context *ctx = det->ctx;
  if (ctx->opt.scan_first) return (int)ctx->opt.scan_first;
  const int nf = det->scan_nf_typical;
  const int raw_threshold = (int)(2 * nf + threshold / 100.f * (2 * nf) + 0.5f);
  return n_frames >= FL_SCAN_STEP_FRAMES && 4 * nf - raw_threshold > 28 ? FL_SCAN_FIRST : 8;
}

// Which refinement kernel a fine level gets.  k_refine_lds needs every candidate's window to fit the budget (decided from
// the bank at finalize: refine_window_max) and, being one workgroup per frame, a batch that fills the device: below
// FL_REFINE_LDS_FRAMES_PER_CU frames per CU k_refine's 4 .. 256 workgroups per frame are faster (profiles/README.md).
// Option refine_lds: 1 = never, 2 = wherever the windows fit; refine_lds_bytes: a smaller budget.
#ifndef FL_REFINE_LDS_FRAMES_PER_CU
#define FL_REFINE_LDS_FRAMES_PER_CU 1
#endif
static bool fl_refine_use_lds(const fl_detector *det, int level, int n_frames, long *budget)
{
  const fl_context *ctx = det->ctx;
  *budget = ctx->opt.refine_lds_bytes ? ctx->opt.refine_lds_bytes : (long)FL_REFINE_LDS_BYTES;
  if (ctx->opt.refine_lds == 1 || det->refine_window_max[level] > *budget) return false;
  return ctx->opt.refine_lds == 2 || n_frames >= FL_REFINE_LDS_FRAMES_PER_CU * ctx->cus;
}

extern "C" int fl_dev_refine_pitch(int width, int T) { return fl_refine_pitch(width, fl_refine_qmask(T)); }
extern "C" int fl_dev_refine_plan(const int32_t *rects, int n, int max_len, long budget, int T, int32_t *uni)
{
  FlRect u;
  const int len = fl_refine_plan(rects, n, max_len, budget, fl_refine_qmask(T), &u);
  if (uni) { uni[0] = u.x0; uni[1] = u.y0; uni[2] = u.x1; uni[3] = u.y1; }
  return len;
}
extern "C" int fl_dev_refine_kernel(const fl_detector *det, int level)
{
  return det && level >= 0 && level < det->L - 1 ? det->refine_ran[level] : -1;
}
extern "C" long fl_dev_refine_window_max(const fl_detector *det, int level)
{
  return det && level >= 0 && level < det->L - 1 ? det->refine_window_max[level] : -1;
}

static int launch_scan_refine_sort(fl_detector *det, int n_frames, float threshold, uint16_t *dbg, int dbg_first,
                                   int dbg_count)
{
  fl_context *ctx = det->ctx;
  const int L = det->L, M = det->M;
  {
    const FlLevelGeom &g = det->geom[L - 1];
    ScanArgs a;
    a.offs = det->d_scan_off;
    a.enabled = det->d_item_enabled;
    a.ws = det->d_ws;
    a.ws_stride = det->ws_stride;
    for (int m = 0; m < FL_MAX_MODALITIES; ++m) a.lm_off[m] = g.lm_off[m < M ? m : 0];
    a.off_count = det->off_count;
    a.off_cand = det->off_cand;
    a.M = M;
    a.W = g.W;
    a.WH = g.WH;
    a.T = g.T;
    a.cap = det->cap;
    a.threshold = threshold;
    a.prune = ctx->opt.scan_prune != 0;                   // development switches (fl_context_set_option)
    a.prune_mid = ctx->opt.scan_prune_mid >= 0 ? (unsigned)ctx->opt.scan_prune_mid : FL_SCAN_PRUNE_MID;
    a.prune_lanes = ctx->opt.scan_prune_lanes != 0;
    a.dbg = dbg;
    a.dbg_first = dbg_first;
    a.dbg_count = dbg ? dbg_count : 0;
    a.items = det->d_scan_items;
    a.n_items = det->n_scan_items;
    const int items = det->n_scan_items;
    if (items > 0) {
      a.run = fl_scan_run(ctx, items, n_frames);
      const int waves = (items + a.run - 1) / a.run;      // per frame
      a.bpf = (waves + 3) / 4;
#if FL_SCAN_STRIDED
      a.wave_step = 1;                                    // wave w: items w, w + 4 bpf, ...: the trained views, which lead the bank
      a.item_step = a.bpf * 4;                            // and never prune, are spread over the frame's waves
#else
      a.wave_step = a.run;
      a.item_step = 1;
#endif
      a.n_frames = n_frames;
      dim3 grid((unsigned)(a.bpf * ((n_frames + 7) / 8) * 8));
#define FL_SCAN_LAUNCH(WPE, STEP, FIRST) hipLaunchKernelGGL((k_scan<WPE, STEP, FIRST>), grid, dim3(256), 0, ctx->stream, a)
#define FL_SCAN_LAUNCH_STEP(STEP) \
      switch (first) { \
      case 12: FL_SCAN_LAUNCH(FL_SCAN_WPE_PRUNED, STEP, 12); break; \
      case 14: FL_SCAN_LAUNCH(FL_SCAN_WPE_PRUNED, STEP, 14); break; \
      case 16: FL_SCAN_LAUNCH(FL_SCAN_WPE_PRUNED, STEP, 16); break; \
      default: FL_SCAN_LAUNCH(FL_SCAN_WPE_PRUNED, STEP, 8); break; \
      }
      const int first = fl_scan_first(det, n_frames, threshold);
      if (!a.prune) FL_SCAN_LAUNCH(FL_SCAN_WPE, 8, 8);
      else switch (fl_scan_step(ctx, n_frames)) {
      case 2: FL_SCAN_LAUNCH_STEP(2); break;
      case 4: FL_SCAN_LAUNCH_STEP(4); break;
      default: FL_SCAN_LAUNCH_STEP(8); break;
      }
#undef FL_SCAN_LAUNCH_STEP
#undef FL_SCAN_LAUNCH
      FL_HIP(ctx, hipGetLastError());
#ifdef FL_SCAN_STATS
      {
        unsigned long long st[FL_SCAN_STATS_N], zero[FL_SCAN_STATS_N] = {0};
        FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        FL_HIP(ctx, hipMemcpyFromSymbol(st, HIP_SYMBOL(d_scan_stats), sizeof(st)));
        FL_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(d_scan_stats), zero, sizeof(zero)));
        fprintf(stderr, "k_scan: %d frames, %llu items, %.2f feature loads and %.1f lane-loads per item, %llu items to their end; ended "
                "by a first piece's check %llu; after f features:", n_frames, st[0], st[0] ? (double)st[1] / st[0] : 0.0,
                st[0] ? (double)st[2] / st[0] : 0.0, st[3], st[FL_SCAN_STATS_N - 1]);
        for (int f = 0; f + 5 < FL_SCAN_STATS_N; ++f)
          if (st[4 + f]) fprintf(stderr, " %d: %llu", f, st[4 + f]);
        fprintf(stderr, "\n");
      }
#endif
    }
  }
  if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[3], ctx->stream));
  for (int l = L - 2; l >= 0; --l) {
    const FlLevelGeom &g = det->geom[l];
    RefineArgs a;
    const bool lazy_level = det->lazy;
    a.hdr = det->d_fine_hdr;
    a.feat = det->d_fine_feat;
    a.ws = det->d_ws;
    a.ws_stride = det->ws_stride;
    for (int m = 0; m < FL_MAX_MODALITIES; ++m) a.spread_off[m] = g.spread_off[m < M ? m : 0];
    a.off_count = det->off_count;
    a.off_cand = det->off_cand;
    a.M = M;
    a.Lm1 = L - 1;
    a.level = l;
    a.w = g.w;
    a.h = g.h;
    a.T = g.T;
    a.W = g.W;
    a.H = g.H;
    a.cap = det->cap;
    a.threshold = threshold;
    if (lazy_level) {
      // the level's colour quantisation and spread images, only where these candidates will look
      if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[8 + 2 * l], ctx->stream));
      hipLaunchKernelGGL(k_mark_tiles, dim3(n_frames), dim3(256), 0, ctx->stream, a, det->off_tiles);
      FL_HIP(ctx, hipGetLastError());
      int rc = fl_launch_lazy_level(det, n_frames, l);
      if (rc) return rc;
      if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[9 + 2 * l], ctx->stream));
    }
    long budget;
    if (fl_refine_use_lds(det, l, n_frames, &budget)) {
      const uint32_t qmask = fl_refine_qmask(g.T);
      const dim3 grid(n_frames), block(256);
      switch (g.T) {
      case 4: hipLaunchKernelGGL(k_refine_lds<4>, grid, block, 0, ctx->stream, a, det->d_fine_box, (int)budget, qmask); break;
      case 5: hipLaunchKernelGGL(k_refine_lds<5>, grid, block, 0, ctx->stream, a, det->d_fine_box, (int)budget, qmask); break;
      case 8: hipLaunchKernelGGL(k_refine_lds<8>, grid, block, 0, ctx->stream, a, det->d_fine_box, (int)budget, qmask); break;
      default: hipLaunchKernelGGL(k_refine_lds<0>, grid, block, 0, ctx->stream, a, det->d_fine_box, (int)budget, qmask); break;
      }
      det->refine_ran[l] = 2;
#ifdef FL_REFINE_STATS
      {
        unsigned long long st[4], zero[4] = {0, 0, 0, 0};
        FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
        FL_HIP(ctx, hipMemcpyFromSymbol(st, HIP_SYMBOL(d_refine_stats), sizeof(st)));
        FL_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(d_refine_stats), zero, sizeof(zero)));
        fprintf(stderr, "k_refine_lds level %d: %d frames, %llu with candidates, %.2f groups per such frame, %.0f bytes staged per group, "
                "%.2f candidates per group\n", l, n_frames, st[0], st[0] ? (double)st[1] / st[0] : 0.0, st[1] ? (double)st[2] / st[1] : 0.0,
                st[1] ? (double)st[3] / st[1] : 0.0);
      }
#endif
    } else {
      // few workgroups per frame: candidates are typically tens per frame and idle workgroups are not
      // free (every wave still fetches the frame's counter); heavy frames just loop longer
      dim3 grid(n_frames >= 64 ? 4 : (n_frames >= 8 ? 32 : 256), n_frames);
      hipLaunchKernelGGL(k_refine, grid, dim3(256), 0, ctx->stream, a);
      det->refine_ran[l] = 1;
    }
    FL_HIP(ctx, hipGetLastError());
  }
  if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[4], ctx->stream));
  {
    SortArgs a;
    a.pyr = det->d_pyr;
    a.ws = det->d_ws;
    a.ws_stride = det->ws_stride;
    a.off_count = det->off_count;
    a.off_cand = det->off_cand;
    a.off_keys = det->off_keys;
    a.off_match = det->off_match;
    a.cap = det->cap;
    hipLaunchKernelGGL(k_sort_unique, dim3(n_frames), dim3(1024), 0, ctx->stream, a);
    FL_HIP(ctx, hipGetLastError());
  }
  if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[5], ctx->stream));
  return FL_OK;
}

// spread/response/linearize for all levels and modalities of n_frames frames, then the match core
int fl_launch_match_core(fl_detector *det, int n_frames, float threshold)
{
  fl_context *ctx = det->ctx;
  // the ICP stage that last read this set of counters and match lists (two batches ago, on the ICP stream) comes first
  if (det->set_busy[det->set]) {
    det->set_busy[det->set] = false;
    FL_HIP(ctx, hipStreamWaitEvent(ctx->stream, det->ev_set_read[det->set], 0));
  }
  // zero the per-frame counters
  FL_HIP(ctx, hipMemset2DAsync(det->d_ws + det->off_count, det->ws_stride, 0, 16, n_frames, ctx->stream));
  for (int l = 0; l < det->L; ++l) {
    const FlLevelGeom &g = det->geom[l];
    if (det->lazy && l < det->L - 1) continue;             // spread of a fine level: after the scan, marked tiles only
    const bool coarsest = l == det->L - 1;
    const FlPlanes pl = fl_level_planes(det, g, coarsest ? g.lm_off : g.spread_off);
    int rc = coarsest ? fl_launch_build_lm(ctx, pl, det->M, n_frames, g.w, g.h, g.T)
                      : fl_launch_spread_tiles(ctx, pl, det->M, n_frames, g.w, g.h, g.T, nullptr, 0);
    if (rc) return rc;
  }
  if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[2], ctx->stream));
  return launch_scan_refine_sort(det, n_frames, threshold, nullptr, 0, 0);
}

static int read_matches(fl_detector *det, int frame, fl_match *out, int cap, int *n_total)
{
  fl_context *ctx = det->ctx;
  int counters[4];
  uint8_t *ws = det->d_ws + (size_t)frame * det->ws_stride;
  FL_HIP(ctx, hipMemcpyAsync(counters, ws + det->off_count, sizeof(counters), hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (counters[2]) return fl_set_error(ctx, FL_ERR_OVERFLOW, "more than %d candidates in one frame", det->cap);
  if (n_total) *n_total = counters[1];
  int n = counters[1] < cap ? counters[1] : cap;
  if (n > 0 && out) {
    FL_HIP(ctx, hipMemcpyAsync(out, ws + det->off_match, sizeof(fl_match) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return FL_OK;
}

int fl_overflow_needed(fl_detector *det, int n_frames, int *needed)
{
  fl_context *ctx = det->ctx;
  std::vector<int> c((size_t)4 * n_frames);
  FL_HIP(ctx, hipMemcpy2DAsync(c.data(), 16, det->d_ws + det->off_count, det->ws_stride, 16, n_frames, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *needed = 0;
  for (int f = 0; f < n_frames; ++f)
    if (c[4 * f + 2] && c[4 * f] > *needed) *needed = c[4 * f];
  return FL_OK;
}

// The queued entry points cannot replay a batch themselves; their caller can: after a batch in which a frame reported
// FL_ERR_OVERFLOW (fl_recognition_result.status, or FL_TOPK_OVERFLOW in the exported records), this waits for the stream,
// grows the candidate buffers to what the fullest of the last batch's first n_frames frames needs, and the caller submits
// the batch again.  *new_cap = the capacity afterwards (unchanged when no frame had overflowed).
extern "C" int fl_detector_grow_candidates(fl_detector *det, int n_frames, int *new_cap)
{
  if (!det || n_frames <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || n_frames > det->max_batch) return fl_set_error(ctx, FL_ERR_INVALID, "n_frames");
  if (det->batch.n == 0) {                               // nothing matched yet: no counters to read, just report the capacity
    if (new_cap) *new_cap = det->cap;
    return FL_OK;
  }
  // only the last batch's frames have counters that mean anything: a flag left by an earlier, larger batch must not trigger a
  // stream sync, a free and a re-layout of every frame workspace
  if (n_frames > det->batch.n)
    return fl_set_error(ctx, FL_ERR_STATE, "n_frames %d > the %d frames of the last batch", n_frames, det->batch.n);
  FL_HIP(ctx, hipSetDevice(ctx->device));
  int needed = 0;
  int rc = fl_pipeline_join(det);
  if (rc == FL_OK) rc = fl_overflow_needed(det, n_frames, &needed);
  if (rc == FL_OK && needed > 0) rc = fl_grow_candidates(det, needed);
  if (new_cap) *new_cap = det->cap;
  return rc;
}

extern "C" int fl_match_quantized(fl_detector *det, const uint8_t *const *quantized, int mem, float threshold,
                                  fl_match *out, int cap, int *n_total)
{
  if (!det || !quantized || cap < 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (int rc = fl_check_frames(det, 1)) return rc;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  for (int attempt = 0;; ++attempt) {
    if (int rc = fl_pipeline_join(det)) return rc;
    fl_batch_forget(det);
    for (int l = 0; l < det->L; ++l)
      for (int m = 0; m < det->M; ++m) {
        const FlLevelGeom &g = det->geom[l];
        FL_HIP(ctx, hipMemcpyAsync(det->d_ws + g.quant_off[m], quantized[l * det->M + m], (size_t)g.w * g.h,
                                   mem == FL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
      }
    det->have_times = false;
    det->lazy = false;                     // every level's quantised image was just supplied
    int rc = fl_launch_match_core(det, 1, threshold);
    if (rc) return rc;
    fl_batch_record(det, 1, nullptr, 0, false);    // no depth frame belongs to this batch
    rc = read_matches(det, 0, out, cap, n_total);
    if (!fl_grow_after_overflow(det, 1, attempt, &rc)) return rc;
  }
}

// QuantizedPyramid::quantize with a mask (`angle.copyTo(dst, mask)` linemod.cpp:455-459, `normal.copyTo(dst, mask)`
// :741-745): level l keeps a pixel only where the l-times NN-halved mask (:445-450, :733-738) is non-zero.  The chain of
// cv::resize(INTER_NEAREST) source coordinates is composed here so the mask pyramid is never materialised.
__global__ __launch_bounds__(256) void k_apply_mask(uint8_t *__restrict__ quant, const uint8_t *__restrict__ mask, int w0,
                                                    int h0, int level)
{
  const int w = w0 >> level, h = h0 >> level;
  int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const size_t o = (size_t)y * w + x;
  for (int k = level; k >= 1; --k) {
    const int sw = w0 >> (k - 1), sh = h0 >> (k - 1), dw = sw / 2, dh = sh / 2;
    x = min((int)floor(x * (1.0 / ((double)dw / sw))), sw - 1);
    y = min((int)floor(y * (1.0 / ((double)dh / sh))), sh - 1);
  }
  if (!mask[(size_t)y * w0 + x]) quant[o] = 0;
}

// a single frame into workspace 0, where the single-frame entry points (fl_match_frame*, fl_recognize_topk) run it
int fl_upload_frame0(fl_detector *det, const uint8_t *bgr, const uint16_t *depth, int mem)
{
  fl_context *ctx = det->ctx;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  const hipMemcpyKind kind = mem == FL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const size_t px = (size_t)det->w0 * det->h0;
  FL_HIP(ctx, hipMemcpyAsync(det->d_ws + det->off_bgr, bgr, px * 3, kind, ctx->stream));
  if (det->M == 2) FL_HIP(ctx, hipMemcpyAsync(det->d_ws + det->off_depth, depth, px * 2, kind, ctx->stream));
  return FL_OK;
}

static int match_frame_masked_once(fl_detector *det, const uint8_t *bgr, const uint16_t *depth,
                                   const uint8_t *const *masks, int mem, float threshold, fl_match *out, int cap,
                                   int *n_total)
{
  if (!det || !bgr || cap < 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  int rc = fl_check_frames(det, 1);
  if (rc) return rc;
  if (det->M == 2 && !depth) return fl_set_error(ctx, FL_ERR_INVALID, "sources.size() != modalities.size() (linemod.cpp:1364)");
  if ((rc = fl_pipeline_join(det))) return rc;
  fl_batch_forget(det);
  if ((rc = fl_upload_frame0(det, bgr, depth, mem))) return rc;
  det->have_times = false;
  const size_t px = (size_t)det->w0 * det->h0;
  // whole quantised pyramids (masks apply to them, fl_last_quantized returns them): no lazy levels here
  rc = fl_launch_frontend(det, 1, det->d_ws + det->off_bgr, det->ws_stride, (const uint16_t *)(det->d_ws + det->off_depth),
                          det->ws_stride, false);
  if (rc) return rc;
  uint8_t *d_mask = nullptr;
  if (masks) {
    if (mem != FL_MEM_DEVICE) FL_HIP(ctx, hipMalloc(&d_mask, px * det->M));
    for (int m = 0; m < det->M && rc == FL_OK; ++m) {
      if (!masks[m]) continue;
      const uint8_t *dm = masks[m];
      if (mem != FL_MEM_DEVICE) {
        dm = d_mask + px * m;
        if (hipMemcpyAsync((void *)dm, masks[m], px, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = FL_ERR_HIP;
      }
      for (int l = 0; l < det->L && rc == FL_OK; ++l) {
        const FlLevelGeom &g = det->geom[l];
        hipLaunchKernelGGL(k_apply_mask, dim3((g.w + 63) / 64, (g.h + 3) / 4), dim3(256), 0, ctx->stream,
                           det->d_ws + g.quant_off[m], dm, det->w0, det->h0, l);
        if (hipGetLastError() != hipSuccess) rc = FL_ERR_HIP;
      }
    }
  }
  if (rc == FL_OK) rc = fl_launch_match_core(det, 1, threshold);
  if (rc == FL_OK) {
    fl_batch_record(det, 1, nullptr, 0, false);    // single-frame Detector::match: fl_refine_matches belongs to batch submits
    rc = read_matches(det, 0, out, cap, n_total);
  } else if (rc == FL_ERR_HIP) {
    fl_set_error(ctx, rc, "mask upload / k_apply_mask launch failed");
  }
  if (d_mask) {
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_mask);
  }
  return rc;
}

extern "C" int fl_match_frame_masked(fl_detector *det, const uint8_t *bgr, const uint16_t *depth,
                                     const uint8_t *const *masks, int mem, float threshold, fl_match *out, int cap,
                                     int *n_total)
{
  for (int attempt = 0;; ++attempt) {
    int rc = match_frame_masked_once(det, bgr, depth, masks, mem, threshold, out, cap, n_total);
    if (!fl_grow_after_overflow(det, 1, attempt, &rc)) return rc;
  }
}

extern "C" int fl_match_frame(fl_detector *det, const uint8_t *bgr, const uint16_t *depth, int mem, float threshold,
                        fl_match *out, int cap, int *n_total)
{
  return fl_match_frame_masked(det, bgr, depth, nullptr, mem, threshold, out, cap, n_total);
}

// the sorted, de-duplicated matches of frame `frame` of the batch last queued with fl_match_batch_submit (or any other
// fl_match_* / fl_recognize_* call: the lists stay in HBM until the next batch)
extern "C" int fl_match_batch_collect(fl_detector *det, int frame, fl_match *out, int cap, int *n_total)
{
  if (!det || cap < 0 || (cap > 0 && !out)) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || frame < 0 || frame >= det->batch.n) return fl_set_error(ctx, FL_ERR_STATE, "no such frame in the last batch");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_pipeline_join(det)) return rc;
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  fl_update_stage_times(det, det->batch.n, nullptr);
  return read_matches(det, frame, out, cap, n_total);
}

extern "C" int fl_similarity_maps(fl_detector *det, int first, int count, uint16_t *out)
{
  if (!det || !out || first < 0 || count <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || det->batch.n < 1) return fl_set_error(ctx, FL_ERR_STATE, "no frame matched yet");
  if (first + count > det->n_pyr) return fl_set_error(ctx, FL_ERR_INVALID, "pyramid range");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  const FlLevelGeom &g = det->geom[det->L - 1];
  size_t bytes = (size_t)count * g.WH * sizeof(uint16_t);
  void *d = nullptr;
  int rc = fl_pipeline_join(det);          // frame 0's counters are rewritten below
  if (rc == FL_OK) rc = fl_scratch(ctx, bytes, &d);
  if (rc) return rc;
  FL_HIP(ctx, hipMemsetAsync(d, 0, bytes, ctx->stream));
  // re-run the scan on frame 0's resident linear memories with the debug tap on; threshold 200%
  // keeps the candidate buffer untouched in practice (counters are reset by the launcher)
  det->have_times = false;
  // frame 0's counters are saved and restored around the debug scan: its match list (fl_export_topk, fl_frame_counters,
  // fl_match_batch_collect) stays what the last match left (no candidate survives 200 %, so the list itself is untouched)
  uint8_t *saved = det->d_ws + det->off_count + 64;
  FL_HIP(ctx, hipMemcpyAsync(saved, det->d_ws + det->off_count, 16, hipMemcpyDeviceToDevice, ctx->stream));
  FL_HIP(ctx, hipMemsetAsync(det->d_ws + det->off_count, 0, 16, ctx->stream));
  const bool was_lazy = det->lazy;       // no candidate survives 200 %: nothing of the finer levels is needed, and the
  det->lazy = false;                     // batch's colour frames (lazy_bgr) may be gone by now
  rc = launch_scan_refine_sort(det, 1, 200.0f, (uint16_t *)d, first, count);
  det->lazy = was_lazy;
  if (rc) return rc;
  FL_HIP(ctx, hipMemcpyAsync(det->d_ws + det->off_count, saved, 16, hipMemcpyDeviceToDevice, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

extern "C" int fl_frame_counters(fl_detector *det, int frame, int32_t out[4])
{
  if (!det || !out) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || frame < 0 || frame >= det->max_batch) return fl_set_error(ctx, FL_ERR_INVALID, "frame");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_pipeline_join(det)) return rc;
  FL_HIP(ctx, hipMemcpyAsync(out, det->d_ws + (size_t)frame * det->ws_stride + det->off_count, 16, hipMemcpyDeviceToHost, ctx->stream));
  uint32_t bm[2 * FL_TILE_WORDS];
  const bool lazy = det->lazy && det->L > 1 && frame < det->batch.n;
  if (lazy)        // level 0's two tile bitmaps: [0] tiles whose spread bytes are read, [1] tiles whose pixels are quantised
    FL_HIP(ctx, hipMemcpyAsync(bm, det->d_ws + (size_t)frame * det->ws_stride + det->off_tiles, sizeof(bm), hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  out[3] = -1;
  if (lazy) {
    int n = 0;
    for (int k = 0; k < FL_TILE_WORDS; ++k) n += __builtin_popcount(bm[FL_TILE_WORDS + k]);
    out[3] = n;
  }
  return FL_OK;
}

extern "C" int fl_last_quantized(fl_detector *det, uint8_t *out)
{
  if (!det || !out) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || det->batch.n < 1) return fl_set_error(ctx, FL_ERR_STATE, "no frame matched yet");
  if (det->lazy)
    return fl_set_error(ctx, FL_ERR_STATE, "the last batch (fl_recognize_*) quantised its finer levels only around the candidates; "
                                           "use fl_match_frame, or FL_EAGER_FRONTEND=1, for whole quantised pyramids");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  for (int l = 0; l < det->L; ++l)
    for (int m = 0; m < det->M; ++m) {
      const FlLevelGeom &g = det->geom[l];
      FL_HIP(ctx, hipMemcpyAsync(out, det->d_ws + g.quant_off[m], (size_t)g.w * g.h, hipMemcpyDeviceToHost, ctx->stream));
      out += (size_t)g.w * g.h;
    }
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

// Development read-back (not in include/fealess_hip.h; tests/test_gpu_batch_frontend.py): what frame `frame` of the last batch
// holds in its workspace, as it is -- lazy batches included, where the finer levels' colour quantisation and spreads exist only
// in the marked tiles.  kind 0: quantised image of (level, modality), w*h bytes; 1: pyrDown BGR of a level >= 1, w*h*3 bytes
// (level 0 may have been read in place, so it is not offered); 2: spread image of a fine level, w*h bytes; 3: the coarsest
// level's 8 linear memories, 8 * fl_lm_label_stride bytes in the layout of fl_build_linear_memories.  Nothing after the match
// (ICP, fl_export_topk*, fl_similarity_maps) writes these regions: the ICP stages use off_icp only.  The next call that runs a
// front-end (any fl_match_* / fl_recognize_*) overwrites them, fl_recognize_topk and fl_match_frame* in workspace 0.
// *bytes is set whenever the request is valid, also when cap is too small (FL_ERR_INVALID).
extern "C" int fl_dev_frame_image(fl_detector *det, int frame, int kind, int level, int modality, uint8_t *out, size_t cap,
                                  size_t *bytes)
{
  if (!det || !bytes) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || det->batch.n < 1) return fl_set_error(ctx, FL_ERR_STATE, "no batch matched yet");
  if (frame < 0 || frame >= det->batch.n) return fl_set_error(ctx, FL_ERR_INVALID, "frame %d is not in the last batch", frame);
  if (level < 0 || level >= det->L || modality < 0 || modality >= det->M)
    return fl_set_error(ctx, FL_ERR_INVALID, "level %d / modality %d out of range", level, modality);
  const FlLevelGeom &g = det->geom[level];
  const bool coarsest = level == det->L - 1;
  size_t off = 0, n = 0;
  switch (kind) {
  case 0: off = g.quant_off[modality]; n = (size_t)g.w * g.h; break;
  case 1:
    if (level == 0) return fl_set_error(ctx, FL_ERR_INVALID, "level 0's colour image is the input frame");
    off = g.bgr_off; n = (size_t)g.w * g.h * 3; break;
  case 2:
    if (coarsest) return fl_set_error(ctx, FL_ERR_INVALID, "the coarsest level has linear memories, not a spread image");
    off = g.spread_off[modality]; n = (size_t)g.w * g.h; break;
  case 3:
    if (!coarsest) return fl_set_error(ctx, FL_ERR_INVALID, "only the coarsest level has linear memories");
    off = g.lm_off[modality]; n = (size_t)8 * g.stride; break;
  default: return fl_set_error(ctx, FL_ERR_INVALID, "kind %d", kind);
  }
  *bytes = n;
  if (!out || cap < n) return fl_set_error(ctx, FL_ERR_INVALID, "%zu bytes needed, %zu given", n, cap);
  FL_HIP(ctx, hipSetDevice(ctx->device));
  FL_HIP(ctx, hipMemcpyAsync(out, det->d_ws + (size_t)frame * det->ws_stride + off, n, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
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

// ------------------------------------------------------------------------------------------
// multi-GPU helpers: fixed-size top-k export for the RCCL all-gather, and the host merge
__global__ void k_export_topk(const uint8_t *ws, size_t off_count, size_t off_match, int k, int tid_base, fl_match *out)
{
  const int n = ((const int *)(ws + off_count))[1];
  const fl_match *m = (const fl_match *)(ws + off_match);
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    fl_match r;
    if (i < n) { r = m[i]; r.template_id += tid_base; }
    else { r.x = r.y = 0; r.similarity = 0.f; r.class_idx = -1; r.template_id = -1; }
    out[i] = r;
  }
}

extern "C" int fl_export_topk(fl_detector *det, int frame, int k, int template_id_base, void *dev_out)
{
  if (!det || !dev_out || k <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || frame < 0 || frame >= det->max_batch) return fl_set_error(ctx, FL_ERR_INVALID, "frame");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_pipeline_join(det)) return rc;
  hipLaunchKernelGGL(k_export_topk, dim3(1), dim3(256), 0, ctx->stream, det->d_ws + (size_t)frame * det->ws_stride,
                     det->off_count, det->off_match, k, template_id_base, (fl_match *)dev_out);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

__global__ void k_export_topk_batch(const uint8_t *ws, size_t ws_stride, size_t off_count, size_t off_match, int k, int tid_base,
                                    fl_match *out)
{
  const uint8_t *w = ws + (size_t)blockIdx.x * ws_stride;
  const int *counters = (const int *)(w + off_count);
  const bool over = counters[2] != 0;                      // the candidate buffers overflowed: the list is not the frame's list
  const int n = over ? 0 : counters[1];
  const fl_match *m = (const fl_match *)(w + off_match);
  fl_match *o = out + (size_t)blockIdx.x * k;
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    fl_match r;
    if (i < n) { r = m[i]; r.template_id += tid_base; }
    else { r.x = r.y = 0; r.similarity = 0.f; r.class_idx = -1; r.template_id = (over && i == 0) ? FL_TOPK_OVERFLOW : -1; }
    o[i] = r;
  }
}

// the first k matches of each of the last batch's n_frames frames: dev_out[frame * k + i]; one launch
extern "C" int fl_export_topk_batch(fl_detector *det, int n_frames, int k, int template_id_base, void *dev_out)
{
  if (!det || !dev_out || k <= 0 || n_frames <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || n_frames > det->max_batch) return fl_set_error(ctx, FL_ERR_INVALID, "n_frames");
  if (n_frames > det->batch.n) return fl_set_error(ctx, FL_ERR_STATE, "%d frames asked for, the last batch had %d", n_frames, det->batch.n);
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_pipeline_join(det)) return rc;
  hipLaunchKernelGGL(k_export_topk_batch, dim3(n_frames), dim3(64), 0, ctx->stream, det->d_ws, det->ws_stride, det->off_count,
                     det->off_match, k, template_id_base, (fl_match *)dev_out);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

// Match::operator< (linemod.hpp:262-267: similarity descending, then template id ascending) extended to a total order
// by (class, y, x) -- the comparator of fl_merge_topk
__device__ __forceinline__ bool match_before(const fl_match &a, const fl_match &b)
{
  if (a.similarity != b.similarity) return a.similarity > b.similarity;
  if (a.template_id != b.template_id) return a.template_id < b.template_id;
  if (a.class_idx != b.class_idx) return a.class_idx < b.class_idx;
  if (a.y != b.y) return a.y < b.y;
  return a.x < b.x;
}

// one thread per frame: the best of the ranks' first records = matches[0] of the global sort; its refinement job if the
// winner's template lies in this rank's slice
__global__ __launch_bounds__(64) void k_select_best(const fl_match *__restrict__ gathered, int n_ranks, int n_frames, int k,
                                                    int tid_first, int tid_count, fl_match *__restrict__ best, FlRefineJob *__restrict__ jobs)
{
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n_frames) return;
  fl_match b;
  b.x = b.y = 0; b.similarity = 0.f; b.class_idx = -1; b.template_id = -1;
  bool over = false;
  for (int r = 0; r < n_ranks; ++r) {
    const fl_match m = gathered[((size_t)r * n_frames + f) * k];
    if (m.template_id == FL_TOPK_OVERFLOW) over = true;
    else if (m.template_id >= 0 && (b.template_id < 0 || match_before(m, b))) b = m;
  }
  if (over) { b.x = b.y = 0; b.similarity = 0.f; b.class_idx = -1; b.template_id = FL_TOPK_OVERFLOW; }
  best[f] = b;
  FlRefineJob j;
  j.frame = -1;
  j.match = b;
  if (b.template_id >= tid_first && b.template_id < tid_first + tid_count) {
    j.frame = f;
    j.match.template_id = b.template_id - tid_first;      // class-local on this rank's detector
  }
  jobs[f] = j;
}

extern "C" int fl_select_best_batch(fl_detector *det, const void *dev_gathered, int n_ranks, int n_frames, int k, int tid_first,
                                    int tid_count, void *dev_best)
{
  if (!det || !dev_gathered || !dev_best || n_ranks <= 0 || n_frames <= 0 || k <= 0 || tid_first < 0 || tid_count < 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (int rc = fl_check_frames(det, n_frames)) return rc;
  if (det->classes.size() != 1 || tid_count != det->classes[0].n_pyramids)
    return fl_set_error(ctx, FL_ERR_INVALID, "template-sharded refinement: one class per detector, tid_count = its %d pyramids",
                        det->classes.empty() ? 0 : det->classes[0].n_pyramids);
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_pipeline_join(det)) return rc;
  if (!det->d_jobs) FL_HIP(ctx, hipMalloc((void **)&det->d_jobs, sizeof(FlRefineJob) * (size_t)det->max_batch));
  hipLaunchKernelGGL(k_select_best, dim3((n_frames + 63) / 64), dim3(64), 0, ctx->stream, (const fl_match *)dev_gathered, n_ranks,
                     n_frames, k, tid_first, tid_count, (fl_match *)dev_best, det->d_jobs);
  FL_HIP(ctx, hipGetLastError());
  det->selected_frames = n_frames;
  return FL_OK;
}

// ------------------------------------------------------------------------------------------
// Multi-instance grouping (include/fealess_hip.h, "multi-instance recognition"): the greedy walk over a frame's sorted
// match list, one workgroup per frame.  The sequential rule "match i joins the first group whose leader is near, else
// founds one" is run as rounds: in round r the lowest-index match without a group becomes leader r and every match
// without a group within its radius joins it.  Both give the same groups: a match reaches round r only if it is outside
// the radius of leaders 0 .. r-1, leader r is the first match the walk could not place, and a match joins the earliest
// leader it is near in either order.
// A match's state (GRP_FREE, -1 = dropped, or its group) is one byte in LDS for lists of up to FL_GROUP_LDS_MAX matches
// and lives in the group_of output itself beyond that; thread t owns the matches i = t (mod GRP_BS) in every pass.
#define GRP_BS 256
#define GRP_FREE (-2)
struct GrpKey { long long cx, cy; int cls; };      // doubled box centre; cls < 0: class / template not on the detector
struct GrpShared {
  int wmin[2][GRP_BS / FL_WAVE];
  int size[FL_GROUP_MAX];
  int dropped;
};

__device__ __forceinline__ GrpKey grp_key(const FlGroupArgs &a, const fl_match &m)
{
  GrpKey k;
  k.cx = k.cy = 0;
  k.cls = -1;
  if (m.class_idx < 0 || m.class_idx >= a.n_classes || m.template_id < 0) return k;
  const int first = a.class_first[m.class_idx];
  const int end = m.class_idx + 1 < a.n_classes ? a.class_first[m.class_idx + 1] : a.n_pyr;
  if (m.template_id >= end - first) return k;
  const FlPyrInfo pi = a.pyr[first + m.template_id];
  k.cls = m.class_idx;
  k.cx = 2ll * m.x + pi.width0;
  k.cy = 2ll * m.y + pi.height0;
  return k;
}
// |d| < r first: then the squares (r <= 2^31) cannot leave 64 bits whatever the coordinates are
__device__ __forceinline__ bool grp_near(const FlGroupArgs &a, const GrpKey &k, const GrpKey &l)
{
  const long long dx = k.cx - l.cx, dy = k.cy - l.cy;
  if (k.cls != l.cls || dx <= -a.r || dx >= a.r || dy <= -a.r || dy >= a.r) return false;
  return dx * dx + dy * dy < a.r2;
}
// workgroup-wide minimum (one barrier; `parity` alternates between consecutive calls)
__device__ __forceinline__ int grp_wg_min(GrpShared &S, int v, int parity)
{
  for (int o = FL_WAVE / 2; o; o >>= 1) v = min(v, __shfl_xor(v, o));
  if ((threadIdx.x & (FL_WAVE - 1)) == 0) S.wmin[parity][threadIdx.x / FL_WAVE] = v;
  __syncthreads();
  int r = S.wmin[parity][0];
  for (int w = 1; w < GRP_BS / FL_WAVE; ++w) r = min(r, S.wmin[parity][w]);
  return r;
}

template <bool LDS>
__device__ void grp_frame(const FlGroupArgs &a, GrpShared &S, int8_t *st8, const fl_match *__restrict__ m, int n, int f)
{
  const int tid = threadIdx.x, lane = tid & (FL_WAVE - 1);
  int32_t *gof = a.group_of + (size_t)f * a.group_of_stride;
  auto get = [&](int i) -> int { return LDS ? (int)st8[i] : gof[i]; };
  auto set = [&](int i, int v) { if (LDS) st8[i] = (int8_t)v; else gof[i] = v; };
  // every match starts without a group; the first leader is the first match that is on the detector
  int mymin = INT_MAX;
  for (int i = tid; i < n; i += GRP_BS) {
    const bool ok = grp_key(a, m[i]).cls >= 0;
    set(i, ok ? GRP_FREE : -1);
    if (ok && mymin == INT_MAX) mymin = i;
  }
  int parity = 0;
  int leader = grp_wg_min(S, mymin, parity);
  int G = 0;
  while (leader != INT_MAX && G < a.G) {
    const GrpKey lk = grp_key(a, m[leader]);
    int joined = 0;
    mymin = INT_MAX;
    for (int i = leader / GRP_BS * GRP_BS + tid; i < n; i += GRP_BS) {
      if (i < leader || get(i) != GRP_FREE) continue;
      if (grp_near(a, grp_key(a, m[i]), lk)) { set(i, G); ++joined; }     // the leader itself too: distance 0
      else if (mymin == INT_MAX) mymin = i;
    }
    if (joined) atomicAdd(&S.size[G], joined);
    parity ^= 1;
    leader = grp_wg_min(S, mymin, parity);     // the next leader: the first match still without a group
    ++G;
  }
  // what is left found no group
  int dropped = 0;
  for (int i = tid; i < n; i += GRP_BS) {
    const int g = get(i);
    if (g < 0) ++dropped;
    if (LDS) { if (a.write_group_of) gof[i] = g < 0 ? -1 : g; }
    else if (g == GRP_FREE) gof[i] = -1;
  }
  for (int o = FL_WAVE / 2; o; o >>= 1) dropped += __shfl_xor(dropped, o);
  if (lane == 0 && dropped) atomicAdd(&S.dropped, dropped);
  __syncthreads();
  if (tid < a.G) a.group_size[(size_t)f * a.G + tid] = S.size[tid];
  if (tid == 0) {
    int32_t *info = a.info + 4 * (size_t)f;
    info[0] = G; info[1] = S.dropped; info[2] = 0; info[3] = n;
  }
  if (!a.jobs || tid >= FL_WAVE) return;
  // The first h members of every group, in list order, by one wave: lane g counts the members of group g seen so far, a
  // ballot per group present in a chunk of 64 matches gives each member its place (an atomic counter would scramble it).
  const int want = min(S.size[lane], a.h);
  int total = want;
  for (int o = FL_WAVE / 2; o; o >>= 1) total += __shfl_xor(total, o);
  int mycnt = 0, filled = 0;
  for (int base = 0; base < n && filled < total; base += FL_WAVE) {
    const int i = base + lane;
    const int g = i < n ? get(i) : -1;
    unsigned long long rem = __ballot(g >= 0);
    while (rem) {
      const int g0 = __shfl(g, __ffsll((long long)rem) - 1);
      const unsigned long long mask = __ballot(g == g0);
      const int c0 = __shfl(mycnt, g0), c1 = c0 + __popcll(mask);
      const int r = c0 + __popcll(mask & ((1ull << lane) - 1ull));
      if (g == g0 && r < a.h) {
        const size_t slot = ((size_t)f * a.G + g0) * a.h + r;
        FlRefineJob j;
        j.frame = f;
        j.match = m[i];
        a.jobs[slot] = j;
        a.job_idx[slot] = i;
      }
      filled += min(c1, a.h) - min(c0, a.h);
      if (lane == g0) mycnt = c1;
      rem &= ~mask;
    }
  }
}

__global__ __launch_bounds__(GRP_BS) void k_group_matches(FlGroupArgs a)
{
  __shared__ GrpShared S;
  __shared__ int8_t st8[FL_GROUP_LDS_MAX];
  const int f = blockIdx.x, tid = threadIdx.x;
  const fl_match *m = a.matches;
  int n = a.n;
  bool over = false;
  if (a.frame_ws) {
    const uint8_t *w = a.frame_ws + (size_t)f * a.frame_stride;
    const int *counters = (const int *)(w + a.off_count);
    over = counters[2] != 0;             // the candidate buffers overflowed: the list is truncated, never group it
    n = min(counters[1], a.n);
    m = (const fl_match *)(w + a.off_match);
  }
  if (tid < FL_GROUP_MAX) S.size[tid] = 0;
  if (tid == 0) S.dropped = 0;
  if (a.jobs)
    for (int s = tid; s < a.G * a.h; s += GRP_BS) {
      const size_t slot = (size_t)f * a.G * a.h + s;
      a.jobs[slot].frame = -1;
      a.job_idx[slot] = -1;
    }
  if (over) {                            // uniform
    if (tid < a.G) a.group_size[(size_t)f * a.G + tid] = 0;
    if (tid == 0) { int32_t *info = a.info + 4 * (size_t)f; info[0] = 0; info[1] = 0; info[2] = FL_ERR_OVERFLOW; info[3] = n; }
    return;
  }
  if (n <= FL_GROUP_LDS_MAX) grp_frame<true>(a, S, st8, m, n, f);
  else grp_frame<false>(a, S, st8, m, n, f);
}

int fl_launch_group_matches(fl_detector *det, int n_frames, const FlGroupArgs &a)
{
  fl_context *ctx = det->ctx;
  hipLaunchKernelGGL(k_group_matches, dim3(n_frames), dim3(GRP_BS), 0, ctx->stream, a);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

bool fl_instance_params_ok(const fl_instance_params *ip)
{
  return ip && ip->max_instances >= 1 && ip->max_instances <= FL_GROUP_MAX && ip->min_dist_px >= 1 && ip->min_dist_px <= (1 << 30) &&
         ip->hyp_per_instance >= 1 && ip->hyp_per_instance <= FL_GROUP_HYP_MAX;
}

// what both paths of the grouping take from the detector and the parameters; the lists and outputs are the caller's
FlGroupArgs fl_group_args(const fl_detector *det, const fl_instance_params *ip)
{
  FlGroupArgs a;
  memset(&a, 0, sizeof(a));
  a.pyr = det->d_pyr;
  a.class_first = det->d_class_first;
  a.n_classes = (int)det->classes.size();
  a.n_pyr = det->n_pyr;
  a.G = ip->max_instances;
  a.h = ip->hyp_per_instance;
  a.r = 2ll * ip->min_dist_px;
  a.r2 = a.r * a.r;
  return a;
}

extern "C" int fl_group_matches(fl_detector *det, const fl_match *matches, int n, int mem, const fl_instance_params *ip,
                                int32_t *group_of, int32_t *group_size, int32_t *n_groups)
{
  if (!det || n < 0 || (n > 0 && (!matches || !group_of)) || !group_size || !n_groups || (mem != FL_MEM_HOST && mem != FL_MEM_DEVICE))
    return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!fl_instance_params_ok(ip)) return fl_set_error(ctx, FL_ERR_INVALID, FL_INSTANCE_PARAMS_TEXT);
  if (mem == FL_MEM_DEVICE) {
    int rc = fl_check_frames(det, 1);
    if (rc) return rc;
    FL_HIP(ctx, hipSetDevice(ctx->device));
    void *sv = nullptr;
    if ((rc = fl_scratch(ctx, 256, &sv))) return rc;
    FlGroupArgs a = fl_group_args(det, ip);
    a.matches = matches;
    a.n = n;
    a.group_of = group_of;
    a.group_size = group_size;
    a.info = (int32_t *)sv;
    a.write_group_of = 1;
    if ((rc = fl_launch_group_matches(det, 1, a))) return rc;
    FL_HIP(ctx, hipMemcpyAsync(n_groups, sv, sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
    return FL_OK;
  }
  // the walk as the header states it
  const long long r = 2ll * ip->min_dist_px, r2 = r * r;
  std::vector<long long> cx((size_t)n), cy((size_t)n);
  for (int i = 0; i < n; ++i) {
    const fl_match &m = matches[i];
    if (m.class_idx < 0 || m.class_idx >= (int)det->classes.size() || m.template_id < 0 || m.template_id >= det->classes[m.class_idx].n_pyramids)
      return fl_set_error(ctx, FL_ERR_INVALID, "match %d: template %d of class %d is not on this detector", i, m.template_id, m.class_idx);
    const fl_template &t0 = det->classes[m.class_idx].templates[(size_t)m.template_id * det->L * det->M];
    cx[i] = 2ll * m.x + t0.width;
    cy[i] = 2ll * m.y + t0.height;
  }
  int leaders[FL_GROUP_MAX], G = 0;
  for (int g = 0; g < ip->max_instances; ++g) group_size[g] = 0;
  for (int i = 0; i < n; ++i) {
    int g = 0;
    for (; g < G; ++g) {
      const int l = leaders[g];
      const long long dx = cx[i] - cx[l], dy = cy[i] - cy[l];
      if (matches[i].class_idx == matches[l].class_idx && dx > -r && dx < r && dy > -r && dy < r && dx * dx + dy * dy < r2) break;
    }
    if (g == G) {
      if (G == ip->max_instances) { group_of[i] = -1; continue; }
      leaders[G++] = i;
    }
    group_of[i] = g;
    ++group_size[g];
  }
  *n_groups = G;
  return FL_OK;
}

// see fl_internal.h
extern "C" int fl_dev_detector_create_host(int modalities, int levels, const int *T_at_level, fl_detector **out)
{
  if (!out) return FL_ERR_INVALID;
  fl_context *ctx = new fl_context();
  ctx->device = -1;                      // no device: fl_detector_destroy / the context's release make no HIP call
  ctx->destroy_pending = true;           // the detector's destruction releases the context
  const int rc = fl_detector_create(ctx, modalities, levels, T_at_level, out);
  if (rc) delete ctx;
  return rc;
}

extern "C" int fl_dev_group_jobs(fl_detector *det, const fl_match *matches, int n, const fl_instance_params *ip, int32_t *group_of,
                                 int32_t *group_size, int32_t *info, void *jobs, int32_t *job_idx)
{
  if (!det || n < 0 || !matches || !group_of || !group_size || !info || !jobs || !job_idx || !fl_instance_params_ok(ip)) return FL_ERR_INVALID;
  if (int rc = fl_check_frames(det, 1)) return rc;
  FL_HIP(det->ctx, hipSetDevice(det->ctx->device));
  FlGroupArgs a = fl_group_args(det, ip);
  a.matches = matches;
  a.n = n;
  a.group_of = group_of;
  a.group_size = group_size;
  a.info = info;
  a.jobs = (FlRefineJob *)jobs;
  a.job_idx = job_idx;
  a.write_group_of = 1;
  return fl_launch_group_matches(det, 1, a);
}

#include <algorithm>
extern "C" int fl_merge_topk(const fl_match *gathered, int n_records, fl_match *out, int cap)
{
  if (!gathered || !out || n_records < 0 || cap < 0) return FL_ERR_INVALID;
  std::vector<fl_match> v;
  for (int i = 0; i < n_records; ++i)
    if (gathered[i].template_id >= 0) v.push_back(gathered[i]);
  std::sort(v.begin(), v.end(), [](const fl_match &a, const fl_match &b) {
    if (a.similarity != b.similarity) return a.similarity > b.similarity;
    if (a.template_id != b.template_id) return a.template_id < b.template_id;
    if (a.class_idx != b.class_idx) return a.class_idx < b.class_idx;
    if (a.y != b.y) return a.y < b.y;
    return a.x < b.x;
  });
  auto eq = [](const fl_match &a, const fl_match &b) {
    return a.x == b.x && a.y == b.y && a.similarity == b.similarity && a.class_idx == b.class_idx;
  };
  v.erase(std::unique(v.begin(), v.end(), eq), v.end());
  int n = (int)std::min<size_t>(v.size(), (size_t)cap);
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return n;
}

// fl_merge_topk for a whole batch: gathered = what an all-gather of fl_export_topk_batch buffers gives, i.e.
// gathered[(rank * n_frames + frame) * k + i]; out[frame * cap + j], n_out[frame]
extern "C" int fl_merge_topk_batch(const fl_match *gathered, int n_ranks, int n_frames, int k, fl_match *out, int cap, int *n_out)
{
  if (!gathered || !out || !n_out || n_ranks <= 0 || n_frames <= 0 || k <= 0 || cap <= 0) return FL_ERR_INVALID;
  std::vector<fl_match> one((size_t)n_ranks * k);
  for (int f = 0; f < n_frames; ++f) {
    for (int r = 0; r < n_ranks; ++r)
      memcpy(&one[(size_t)r * k], gathered + ((size_t)r * n_frames + f) * k, sizeof(fl_match) * (size_t)k);
    const int n = fl_merge_topk(one.data(), n_ranks * k, out + (size_t)f * cap, cap);
    if (n < 0) return n;
    n_out[f] = n;
  }
  return FL_OK;
}
