// fl_refine.hip -- the refinement of the coarse scan's candidates down the pyramid, one level per launch, in the online
// matching half of cup_linemod::Detector (reference: linemod/linemod.cpp:882-1577).
//
//   k_refine       similarityLocal + 16x16 argmax + filter, one level       (:1226-1300, 1509-1573)
//   k_refine_lds   the same on spread bytes staged in LDS, a group of candidates per window
//   k_mark_tiles   lazy fine levels: the tiles of a level that k_refine will read
#include "fl_internal.h"
#include <limits.h>

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

__device__ __forceinline__ uint4 ld16(const uint8_t *p)
{
  uint4 v;
  __builtin_memcpy(&v, p, 16);     // global_load_dwordx4, any byte alignment (unaligned access mode)
  return v;
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

// refine_resp4 (above): the four responses of a lane to one feature, on its four spread bytes packed in a
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

// The candidates of n_frames frames refined from the level below the coarsest down to level 0, one launch per level; with
// lazy fine levels a level's tiles are marked and its quantisation and spreads made first.
int fl_launch_refine(fl_detector *det, int n_frames, float threshold)
{
  fl_context *ctx = det->ctx;
  const int L = det->L, M = det->M;
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
  return FL_OK;
}
