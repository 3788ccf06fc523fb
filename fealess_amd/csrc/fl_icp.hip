// fl_icp.hip -- gfx950 kernels for the ICP half of the FEALESS hot path.
//
// Replaces (reference paths): cup_d2pc::depthTo3d (ICP/depth_to_3d.cpp:99-137,190-269),
// scale_mat_vec3f / matToVec / is_vec3f_valid (ICP/common.cpp:261-266,382-425), detection()
// (ICP/detection.cpp:11-254), icpCloudToCloud_Ex + getMean/transformPoints/getL2distClouds/
// PointsCorresponding (ICP/ICP.cpp:8-111,193-279,617-809) and the tail of
// CObjRecoLmICP::Recognition (CadReco/obj_reco_lmicp.cpp:111-199).
//
// Execution model: ONE workgroup owns one frame's whole refinement -- crop back-projection,
// paired-valid compaction, centroid pre-alignment, every ICP iteration and the final pose -- in
// a single launch; a batch is a grid of such workgroups.  No host round trip and no inter-
// workgroup synchronisation exists anywhere in the path: phases inside a frame are separated by
// workgroup barriers only.  Parallelism comes from frames (hundreds to thousands resident in
// 288 GB HBM), which is what lets the reference's strictly sequential float32 sums be kept:
//   * FL_ICP_PARITY: each of the 15 centroid/covariance scalars (and the distance sum) is a
//     float32 chain accumulated in the reference's order by its own lane; dropped pairs add an
//     exact +0.0f so the chain is branch-free.  Bit-identical to the reference's arithmetic.
//   * FL_ICP_FAST: per-thread partials + fixed-shape fp64 tree, rounded once to float32.
//   * FL_ICP_POINT_TO_PLANE (no reference counterpart): NN pairs from the first
//     iteration on, 27 fp64 sums of the linearised point-to-plane system, 6x6 Cholesky + Rodrigues.
// The workgroup is 256 threads at full batches (built for 4 and for 5 workgroups per CU: icp_small_wpe picks) and 1024 threads
// when the batch would leave CUs idle anyway (up to two frames per CU; a camera-rate caller: 1-8 frames): the search and the
// chain producers get 4x the lanes, the next iteration's search runs underneath the dist_mean chain ("Search ahead of the
// distance chain" in icp_run), and a frame's latency drops to about what its two sequential chains cost.
//
// Where things are.  This file: workspace and LDS layout, the float32 chains (chain_tile, chain_deferred), l2dist_phase, the pose solvers,
// first_pass (the 256-thread parity kernel's fused pre-translation, copyPoints, initial distances and iteration-1 sums), icp_run (the algorithm: A1 search, A2 sums, solve, distances), crop_clouds / build_tile_order, the kernels, the host entries and, in one
// block at the end, the dev / test entries.  fl_icp_search.h (included here only): what the searches are made of -- loads, bnd[], the grid
// and its search, the reference image, wave reductions, windows -- and the organised searches org_search / org_search_pipe themselves.
// Built with -ffp-contract=off: one IEEE binary32/64 operation per operator.
#include "fl_internal.h"
#include <float.h>
#include <math.h>
#include <string.h>
#include <type_traits>
#include <mutex>
#include <map>
#include <utility>

#define ICP_BS_SMALL 256
#define ICP_BS_WIDE 1024
#define ICP_DT 512                 // terms per block of the deferred dist_mean chain (two float4 per lane of the chain wave)
#ifdef FL_ICP_PHASES
#define TSTAMP(k) do { if (threadIdx.x == 0) { long long now_ = clock64(); S.tacc[k] += now_ - S.tlast; S.tlast = now_; } } while (0)
// set-up passes of k_icp_pipeline (S.tset[k]: 0 crop, 1 tile counts, 2 tile placing, 3 getMean, 4 pre-translation, 5 copyPoints,
// 6 initial distances (fused: the whole first pass), 7 iteration 1's sums, 9 everything between them); summed over the launch's
// workgroups in g_icp_setup and printed by the launcher
#define SSTAMP(k) do { if (threadIdx.x == 0) { long long now_ = clock64(); S.tset[k] += now_ - S.tslast; S.tslast = now_; } } while (0)
// chain phases: what the chain wave spends adding and at the tile barrier (S.hist[k], [k + 1]), and what the first producer
// wave spends at the tile barriers (S.hist[k]; one barrier in `every` is timed); units of 16 cycles
#define CH_STAMP_BEGIN long long c_add = 0, c_bar = 0, c_last = clock64()
#define CH_STAMP(v) { const long long now_ = clock64(); v += now_ - c_last; c_last = now_; }
#define CH_STAMP_END(k) { if (threadIdx.x == 0) { S.hist[k] += (unsigned)(c_add >> 4); S.hist[(k) + 1] += (unsigned)(c_bar >> 4); } }
#define PR_STAMP_BARRIER(k, every) { const long long b0_ = clock64(); tile_barrier(); if (threadIdx.x == 64) S.hist[k] += (unsigned)(((clock64() - b0_) * (every)) >> 4); }
// search step: cycles of a wave's step segments, summed into S.stime[k] when the search ends; ST_ARRIVED: the two values are in
// their registers (the stamp that follows includes the wait for them)
#define ST_STAMP_BEGIN long long st_acc[6] = {0, 0, 0, 0, 0, 0}, st_last = clock64()
#define ST_STAMP(k) { const long long now_ = clock64(); st_acc[k] += now_ - st_last; st_last = now_; }
#define ST_ARRIVED(a, b) asm volatile("" :: "v"(a), "v"(b));
#define ST_STAMP_END { if ((threadIdx.x & 63) == 0) for (int k = 0; k < 5; ++k) atomicAdd(&S.stime[k], (unsigned long long)st_acc[k]); }
#else
#define TSTAMP(k) do { } while (0)
#define SSTAMP(k) do { } while (0)
#define CH_STAMP_BEGIN
#define CH_STAMP(v) { }
#define CH_STAMP_END(k) { }
#define PR_STAMP_BARRIER(k, every) tile_barrier()
#define ST_STAMP_BEGIN
#define ST_STAMP(k) { }
#define ST_ARRIVED(a, b)
#define ST_STAMP_END
#endif
// the barrier between the tiles of a chain phase: this wave's LDS writes complete, then a raw s_barrier (why: phase A2 in icp_run)
__device__ __forceinline__ void tile_barrier()
{
  __builtin_amdgcn_s_waitcnt(0xC07F);                      // s_waitcnt lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
}
#define ICP_PARITY_WPE 4          // waves per SIMD the default 256-thread recognition kernel is compiled for (4 -> 128 VGPRs, 5 -> 96; a
                                  // second instance for 5 is always built, see k_icp_pipeline).  ICP us per frame, one box: mid-round
                                  // 5 @ 1280 frames 11.65, 4 @ 2048 10.4 (the 96-VGPR build spilled in the search loop); after the scan
                                  // batches lost 10 instructions and a few registers: 5 @ 2560 9.76, 4 @ 2048 10.15
#define ICP_FAST_WPE 4
#define ICP_PLANE_WPE 4
// waves per SIMD kernel k_icp_pipeline<MODE, 256> is compiled for
#define ICP_MODE_WPE(MODE) ((MODE) == FL_ICP_PARITY ? ICP_PARITY_WPE : ((MODE) == FL_ICP_POINT_TO_PLANE ? ICP_PLANE_WPE : ICP_FAST_WPE))
#define ICP_NBQ 4                 // organised search: candidate positions fetched per batch (4 VGPRs each)
#define ICP_NBUF_SMALL 4          // 16-row register batches of a chain in the 256-thread kernel.  Round 3: 2 / 3 / 4 measured the same; since
                                  // the dist_mean chain runs over blocks of four tiles (ICP_BMACRO) 2 / 3 / 4 / 6 give 29.5 / 29.2 / 29.1 /
                                  // 38.1 ms per 4096 frames (6: the batches spill)
#define ICP_TILE_W 16             // organised search: the queries of a step come from ICP_TILE_W x (64 / ICP_TILE_W)-pixel tiles.  Wider tiles =
                                  // longer contiguous runs in the tile-ordered gathers / scatters (mod, bnd, nn: 192 instead of 96 bytes per row piece)
                                  // against a larger staged rectangle; measured at 4096 frames, ICP ms per launch: 4 x 16 35.4, 8 x 8 33.9 / 33.8,
                                  // 16 x 4 33.6 / 33.6, 32 x 2 35.8
#define ICP_BMACRO 4              // dist_mean phase, 256-thread parity kernel: tiles per barrier (l2dist_phase)
#define ICP_STAGE_CAP 384         // points a wave stages per search step: six passes of 64
#define ICP_NB 10                 // candidates fetched per round trip of the NN search (measured: 8..20)
// Variants measured and not adopted (profiles/README.md): exact block sums of the dist_mean chain in the 256-thread kernel
// (it keeps the term-by-term chain: with four workgroups per CU nobody waits for it), chain waves elected onto distinct
// SIMDs, a 16-bit depth image, two tiles of loads in flight per producer, fp64 partials in FL_ICP_FAST, row-major search tiles,
// the search running ahead of the chain in the 256-thread kernel, and extra LDS per workgroup.

// HBM layout of one frame's ICP workspace (n = capacity in points):
//   ref   n x 3 f32   reference cloud, index order (pairing + iteration 1)
//   mod   n x 3 f32   model cloud, transformed in place every iteration
//   sref  (n+4) x 16 bytes.  grid search: reference cloud sorted by grid cell as float4 (index bits, X, Y, Z);
//                     organised search: the reference IMAGE, crop pixel p -> X, Y, Z (3 x f32; +inf where the pixel was
//                     dropped by the paired compaction), then the image of the points' indices (i32, NN_IDX_NONE where dropped)
//   zimg   (n+4) x f32  organised search: crop pixel p -> rescaleDepth's z factor of the scene pixel (depth * (1 / 1000.0)), NaN where
//                     the paired compaction dropped the pixel: the point is (((sx - cx) / fx... crop_clouds' expression) of it
//   nn     n x i32    nearest reference point j of model point i (kept pair: j, dropped: -1): its index (grid search) or its
//                     crop pixel (organised search)
//   bnd    n x 16 bit upper bound on the distance from model point i to its nearest reference point: the top half of the
//                     float32 pattern, rounded up (bnd_ld / bnd_st)
//   nd     n x f32    organised search, parity mode: squared distance to nn[i] (the search runs ahead of the threshold it is
//                     compared with, see "Search ahead of the distance chain")
//   dterm  n x f32    parity mode: the terms of getL2distClouds' dist_mean chain, index order (0 for a dropped pair)
//   perm   n x i32    organised search: model indices in 16x4-pixel tile order, column by column inside a tile (build_tile_order)
//   cell_start / cell_cur   CSR offsets of the x/y cell grid (grid search)
//   nrm   n x 3 f32   unit normals of the reference cloud, index order (FL_ICP_POINT_TO_PLANE only; 0 = unknown)
// The 16-bit builds of the 256-thread parity kernel (k_icp_pipeline<.., uint16_t>: n <= 65535, so every crop pixel and point index
// fits 16 bits and 0xFFFF names none) use the same slots at the same offsets:
//   nn     n x u16    crop pixel of the partner, 0xFFFF = none (read back as -1)
//   perm   n x u16    model indices in tile order
//   dterm  n x u16    pix: crop pixel of point i  } written by crop_clouds; l2dist_phase rebuilds ref[i] from them (org_point)
//   nd     n x f32    zref: its depth factor      } every iteration instead of loading its 12 bytes; that kernel neither defers
//                                                    the dist_mean chain nor searches ahead of it, so the two slots are free
struct IcpWsLayout {
  size_t ref, mod, sref, zimg, nn, bnd, nd, dterm, perm, cell_start, cell_cur, nrm, total;
  int ncell_max;
};
static __host__ __device__ inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
static __host__ __device__ inline IcpWsLayout icp_layout(int n)
{
  IcpWsLayout L;
  size_t o = 0, nn = (size_t)(n > 0 ? n : 1);
  L.ncell_max = n + 4096;
  L.ref = o; o = al256(o + 12 * nn);
  L.mod = o; o = al256(o + 12 * nn);
  L.sref = o; o = al256(o + 16 * (nn + 4));          // + NN_OVERRUN points at infinity behind the reference image
  L.zimg = o; o = al256(o + 4 * (nn + 4));           // organised search: crop pixel -> depth factor (float), + the overrun guard
  L.nn = o; o = al256(o + 4 * nn);
  L.bnd = o; o = al256(o + 4 * nn);
  L.nd = o; o = al256(o + 4 * nn);
  L.dterm = o; o = al256(o + 4 * nn + 4 * ICP_DT);     // read in whole blocks of ICP_DT terms
  L.perm = o; o = al256(o + 4 * nn);
  L.cell_start = o; o = al256(o + 4 * ((size_t)L.ncell_max + 1));
  L.cell_cur = o; o = al256(o + 4 * (size_t)L.ncell_max);
  L.nrm = o; o = al256(o + 12 * nn);
  L.total = o;
  return L;
}
size_t fl_icp_ws_bytes(int n_pts_max) { return icp_layout(n_pts_max).total; }

struct IcpJob {          // what one workgroup needs besides its workspace
  int kind;              // 0: recognition (read the frame's best match), 1: detection, 2: clouds given
  int n_ref, n_model;    // kind 2
  int rect_model[4], rect_ref[4];      // kind 1
  float r_match[9], t_match[3];        // kind 1
  const uint16_t *model_depth;         // kind 1 (mm)
  const uint16_t *scene_depth;         // kind 1 (mm)
};

struct IcpArgs {
  uint8_t *ws;           // frame 0's ICP workspace
  size_t ws_stride;
  int n_max;
  // scene
  int w, h;
  float fx, fy, cx, cy;  // (float)dFx ... as Mat_<float> K would hold them (common.cpp:374-379)
  int it_thr;
  float dmt, ddt;
  int mode;
  IcpJob job;            // kinds 1, 2
  // kind 0: recognition batch
  const uint8_t *frame_ws;   // detector frame workspaces
  size_t frame_stride;       // their stride (= ws_stride in the per-frame pipeline)
  int ranks;                 // hypotheses per frame: workgroup b refines match (b % ranks) of frame (b / ranks)
  size_t off_count, off_match;
  const uint16_t *scene_base;   // frame i's depth = scene_base + i*scene_stride (bytes)
  size_t scene_stride;
  const FlPyrInfo *pyr;
  const int *class_first;
  const float *poses;
  const uint16_t *const *depth_ptrs;
  fl_recognition_result *results;
  const FlRefineJob *jobs;     // kind 0 with caller-chosen matches (fl_refine_matches): job b refines jobs[b].match on frame jobs[b].frame
  const int *order;            // kind 0 batches: workgroup b runs job order[b] (longest first, see k_icp_order); null: job b
};

// LDS state of one frame workgroup of BS_ threads.  Parity mode: virtual wave 0 chains, the other BS/64 - 1 waves
// produce one tile row per thread.
template <int BS_>
struct IcpSharedT {
  static constexpr int BS = BS_;
  static constexpr int NW = BS_ / 64;
  // Parity mode: wave 0 runs the chains, producer waves write one tile row per thread.  A 16-wave workgroup keeps the
  // waves that share wave 0's SIMD (waves 4, 8, 12: the SPI deals a workgroup's waves round-robin over the 4 SIMDs) out
  // of the producer role, so the chain wave has its SIMD's issue slots to itself.
  static constexpr int NPROD = NW >= 8 ? NW - NW / 4 : NW - 1;
  static constexpr int CHAIN_NBUF = BS_ >= 1024 ? 4 : ICP_NBUF_SMALL;
  static constexpr int TQ = NPROD * 64;   // rows per LDS tile
  // Which wave chains in the 256-thread workgroup: always wave 0, but read from LDS as a runtime value (set to 0 at kernel
  // entry) for the register allocation's sake, not for flexibility -- a literal 0 here raises the scratch of
  // k_icp_pipeline<0, 256, 4> from 240 to 368 bytes per lane and of <0, 256, 5> from 352 to 496.
  int cw;
  // tile row of this thread, or -1 (chain wave / idle wave)
  __device__ __forceinline__ int producer_slot() const
  {
    const int t = (int)threadIdx.x, w = t >> 6;
    if (NW >= 8) return (w & 3) == 0 ? -1 : t - 64 * (1 + (w >> 2));
    const int v = (w - __builtin_amdgcn_readfirstlane(cw) - 1) & (NW - 1);     // producers are virtual waves 0 .. NW - 2
    return v == NW - 1 ? -1 : v * 64 + (t & 63);
  }
  // lane of this thread in the chain wave, or -1
  __device__ __forceinline__ int chain_lane() const
  {
    const int t = (int)threadIdx.x;
    if (NW >= 8) return t < 64 ? t : -1;
    return (t >> 6) == __builtin_amdgcn_readfirstlane(cw) ? (t & 63) : -1;
  }
  static constexpr int TS = TQ + 4;       // tile column stride (floats): 16-byte aligned columns for ds_read_b128; the +4
                                          // keeps the 16 chain lanes of a b128 read on distinct bank groups
  float R[9], T[3], Ropt[9], Topt[3];
  float dist_mean, dist_diff, px, thr;
  int iter, n_corr, go, ok;
  int cnt, inl;                          // deferred dist_mean chain: valid pairs / inliers of the terms in dterm[]
  int stop;                              // the chain wave found the loop over: the search running ahead is abandoned
  int a1_next;                           // organised search: next unclaimed query (64 per step)
  float xmin, ymin, inv_c;
  int GX, GY, nsorted;
  float sums[16];
  double dsum[NW][32];                  // [wave][scalar]
  int iscan[NW + 1];
  int iscan2[2][NW];                    // crop_clouds / CSR scan: per-wave counts, double-buffered
  float fred[4][NW];
  int n, rect_m[4], rect_r[4], status, g;
  // double-buffered LDS tiles feeding the sequential float32 chains (FL_ICP_PARITY):
  // prod[b][k][r] = scalar k (9 products, 3 model coords, 3 reference coords) of row r of tile b
  alignas(16) float prod[2][15][TS];
  static constexpr bool BSUM = NW >= 8;  // exact block sums of the dist_mean chain in this kernel
  alignas(16) float dtile[2][TQ];
  // the organised search stages ICP_STAGE_CAP points per wave in the tile region above: a workgroup with few waves has small
  // tiles (TQ rows), so the region is padded up to what its waves stage
  static constexpr int STAGE_FLOATS = NW * 384 * 4, TILE_FLOATS = 2 * 15 * TS + 2 * TQ;
  alignas(16) float stage_pad[STAGE_FLOATS > TILE_FLOATS ? STAGE_FLOATS - TILE_FLOATS : 4];
  alignas(16) float dchain[2][ICP_DT];   // the deferred dist_mean chain's staging (chain wave only)
  float first_sums[16];                  // 256-thread parity kernel: iteration 1's 15 sums, left by first_pass until the loop head has decided
#ifdef FL_ICP_PHASES
  long long tacc[16], tlast, tkernel;   // tkernel: clock at kernel entry (k_icp_pipeline)
  long long wall0;                      // wall_clock64() (constant 100 MHz) at kernel entry
  unsigned long long stime[8];         // FL_ICP_PHASES: cycles of the search step's segments, summed over the workgroup's waves
  unsigned hist[40];                    // organised search: [0,16) union (W class x H class), [16,26) largest lane window height, [26,30) width class
  long long tset[10], tslast;           // SSTAMP
#endif
};

__device__ __forceinline__ bool vvalid(float z) { return z <= 900.0f; }      // common.cpp:261-266
__device__ __forceinline__ float uniform_f(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }
// float -> int as the hardware converts: saturating, NaN -> 0 (a C cast of an out-of-range value is undefined)
__device__ __forceinline__ int cvt_i32_sat(float f)
{
  int r;
  asm("v_cvt_i32_f32 %0, %1" : "=v"(r) : "v"(f));
  return r;
}

#include "fl_icp_search.h"

// ---- block-level helpers (every thread of the workgroup must call) ---------------------------
template <class SH>
__device__ __forceinline__ int block_sum_int(SH &S, int v)
{
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) S.iscan[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int i = 0; i < SH::NW; ++i) t += S.iscan[i];
  return t;
}

__device__ __forceinline__ double shfl_xor_d(double v, int s)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __shfl_xor(lo, s, 64);
  hi = __shfl_xor(hi, s, 64);
  return __hiloint2double(hi, lo);
}

// fixed-shape fp64 reduction of NS scalars per thread; the result (double) is left in S.dsum[0][k], the caller rounds
template <int NS, class SH>
__device__ __forceinline__ void block_sum_double(SH &S, double *v)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    double x = v[k];
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) x += shfl_xor_d(x, s);
    v[k] = x;
  }
  __syncthreads();
  if (lane == 0)
    for (int k = 0; k < NS; ++k) S.dsum[wave][k] = v[k];
  __syncthreads();
  if (threadIdx.x < NS) {
    double t = 0;
    for (int i = 0; i < SH::NW; ++i) t += S.dsum[i][threadIdx.x];
    S.dsum[0][threadIdx.x] = t;
  }
  __syncthreads();
}

// ---- 3x3 helpers with cv::Matx float semantics (s = 0; s += a*b ...) --------------------------
__device__ __forceinline__ void mat_vec(const float *R, const float *v, float *o)
{
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float s = 0;
    s += R[i * 3 + 0] * v[0];
    s += R[i * 3 + 1] * v[1];
    s += R[i * 3 + 2] * v[2];
    o[i] = s;
  }
}
__device__ __forceinline__ void mat_mat(const float *A, const float *B, float *O)
{
  float t[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      float s = 0;
      for (int k = 0; k < 3; ++k) s += A[i * 3 + k] * B[k * 3 + j];
      t[i * 3 + j] = s;
    }
  for (int i = 0; i < 9; ++i) O[i] = t[i];
}

// cv::SVD::compute on 3x3 CV_32F: OpenCV JacobiSVDImpl_<float> restated (same text as
// oracle/icp_oracle.c orc_svd3, which documents the one deviation: hypot -> sqrt(p*p+b*b)).
__device__ __noinline__ void svd3(const float *A, float *U, float *Vt)
{
  float At[9];
  double W[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) At[i * 3 + j] = A[j * 3 + i];
  const float eps = FLT_EPSILON * 2;
  const double minval = FLT_MIN;
  for (int i = 0; i < 3; ++i) {
    double sd = 0;
    for (int k = 0; k < 3; ++k) { float t = At[i * 3 + k]; sd += (double)t * t; }
    W[i] = sd;
    for (int k = 0; k < 3; ++k) Vt[i * 3 + k] = 0;
    Vt[i * 3 + i] = 1;
  }
  for (int iter = 0; iter < 30; ++iter) {
    bool changed = false;
    for (int i = 0; i < 2; ++i)
      for (int j = i + 1; j < 3; ++j) {
        float *Ai = At + i * 3, *Aj = At + j * 3;
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < 3; ++k) p += (double)Ai[k] * Aj[k];
        if (fabs(p) <= eps * sqrt((double)a * b)) continue;
        p *= 2;
        double beta = a - b, gamma = sqrt(p * p + beta * beta);
        float c, s;
        if (beta < 0) {
          double delta = (gamma - beta) * 0.5;
          s = (float)sqrt(delta / gamma);
          c = (float)(p / (gamma * s * 2));
        } else {
          c = (float)sqrt((gamma + beta) / (gamma * 2));
          s = (float)(p / (gamma * c * 2));
        }
        a = b = 0;
        for (int k = 0; k < 3; ++k) {
          float t0 = c * Ai[k] + s * Aj[k];
          float t1 = -s * Ai[k] + c * Aj[k];
          Ai[k] = t0;
          Aj[k] = t1;
          a += (double)t0 * t0;
          b += (double)t1 * t1;
        }
        W[i] = a;
        W[j] = b;
        changed = true;
        float *Vi = Vt + i * 3, *Vj = Vt + j * 3;
        for (int k = 0; k < 3; ++k) {
          float t0 = c * Vi[k] + s * Vj[k];
          float t1 = -s * Vi[k] + c * Vj[k];
          Vi[k] = t0;
          Vj[k] = t1;
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < 3; ++i) {
    double sd = 0;
    for (int k = 0; k < 3; ++k) { float t = At[i * 3 + k]; sd += (double)t * t; }
    W[i] = sqrt(sd);
  }
  for (int i = 0; i < 2; ++i) {
    int j = i;
    for (int k = i + 1; k < 3; ++k)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      double t = W[i]; W[i] = W[j]; W[j] = t;
      for (int k = 0; k < 3; ++k) { float f = At[i * 3 + k]; At[i * 3 + k] = At[j * 3 + k]; At[j * 3 + k] = f; }
      for (int k = 0; k < 3; ++k) { float f = Vt[i * 3 + k]; Vt[i * 3 + k] = Vt[j * 3 + k]; Vt[j * 3 + k] = f; }
    }
  }
  for (int i = 0; i < 3; ++i) {
    double sd = W[i];
    float s = (float)(sd > minval ? 1 / sd : 0.);
    for (int k = 0; k < 3; ++k) At[i * 3 + k] *= s;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) U[i * 3 + j] = At[j * 3 + i];
}

__device__ __forceinline__ bool finite_all(const float *v, int n)
{
  for (int i = 0; i < n; ++i)
    if (!isfinite(v[i])) return false;
  return true;
}

// ---- sequential float32 chains (FL_ICP_PARITY) ------------------------------------------------
// one chain step over an LDS tile: acc += col[0], col[1], ... col[rows-1], strictly in order.
// The adds are one dependent chain; what made a tile slow was the LDS read latency in front of every 16 of
// them.  The column (16-byte aligned) is read 16 rows at a time with four ds_read_b128, two batches in flight:
// batch B is issued before batch A is added and vice versa, so the reads overlap the chain.
__device__ __forceinline__ void chain_load16(const float *col, float4 (&v)[4])
{
#pragma unroll
  for (int u = 0; u < 4; ++u) v[u] = *(const float4 *)(col + 4 * u);
}
__device__ __forceinline__ float chain_add16(const float4 (&v)[4], float acc)
{
#pragma unroll
  for (int u = 0; u < 4; ++u) { acc += v[u].x; acc += v[u].y; acc += v[u].z; acc += v[u].w; }
  return acc;
}
// NBUF 16-row batches of the chain's column are kept in registers: NBUF - 1 of them are in flight while one is added (an
// LDS read takes longer than the 16 dependent adds of a batch).  Measured: 4 in the 1024-thread kernel (128 VGPRs:
// 9.5 -> 8.7 M cycles per frame at batch 1), 2 in the 256-thread one (96 VGPRs: 4 spills, 18 -> 21 ms per 1280 frames).
template <int NBUF>
__device__ __forceinline__ float chain_tile(const float *col, int rows, float acc)
{
  const int nb = rows >> 4;                              // full batches
  int b = 0;
  if (nb >= NBUF) {
    float4 buf[NBUF][4];
#pragma unroll
    for (int u = 0; u < NBUF; ++u) chain_load16(col + 16 * u, buf[u]);
    for (; b + 2 * NBUF <= nb; b += NBUF) {              // steady state: every batch added is replaced by the one NBUF ahead
#pragma unroll
      for (int u = 0; u < NBUF; ++u) {
        acc = chain_add16(buf[u], acc);
        chain_load16(col + 16 * (b + NBUF + u), buf[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < NBUF; ++u) acc = chain_add16(buf[u], acc);
    b += NBUF;
  }
  for (; b < nb; ++b) {                                  // fewer than NBUF batches are left (last tile only)
    float4 one[4];
    chain_load16(col + 16 * b, one);
    acc = chain_add16(one, acc);
  }
  for (int r = nb << 4; r < rows; ++r) acc += col[r];
  return acc;
}

// ---- exact block sums of a float32 chain with non-negative terms (getL2distClouds' dist_mean, ICP.cpp:68-111) ----------
// acc <- fl(fl(fl(acc + x0) + x1) + ...) is a chain of dependent adds (8.25 cycles each, one useful lane).  But while the
// running sum stays inside ONE binade [2^e, 2^(e+1)), every float it can take is a multiple of u = 2^(e-23), and
// fl(s + x) = s + rne(x / u) u for a multiple s of u -- unless x / u lies exactly half way between two integers (then the
// parity of s decides).  So for a block of terms x_k >= 0 (the sum only grows): if no x_k / u is a tie and
// acc / u + sum_k rne(x_k / u) < 2^24, the chain's result after the block is exactly that integer times u, whatever the
// order -- a wave-wide integer reduction instead of 64 x N dependent adds.  Ties (about 1 term in 2^(e - e_x)) and binade
// crossings (log2 of the sum over a whole cloud) make the block fall back to the term-by-term chain.  Bit-identical by
// construction; x * 2^(23-e) is exact (a power of two; an underflow rounds to a value below 1/2, which still rounds to 0).
struct BlkScale {
  float scale, ulp;      // 2^(23-e), 2^(e-23)
  int ai;                // acc / ulp, in [2^23, 2^24)
  bool ok;               // acc is a positive normal float whose scale and ulp are normal too
};
__device__ __forceinline__ BlkScale blk_scale(float acc)
{
  BlkScale b;
  const unsigned eb = __float_as_uint(acc) >> 23;          // sign + exponent: a negative, zero, denormal, inf or NaN acc fails the test
  b.ok = eb >= 24u && eb <= 254u;
  const unsigned e2 = b.ok ? eb : 127u;
  b.scale = __uint_as_float((277u - e2) << 23);
  b.ulp = __uint_as_float((e2 - 23u) << 23);
  b.ai = cvt_i32_sat(acc * b.scale);
  return b;
}
#define BLK_LANE_MAX 2097152.0f                             // 2^21: 768 terms below it sum to less than 2^31
__device__ __forceinline__ void blk_term(const BlkScale &b, float x, int &isum, bool &bad)
{
  const float y = x * b.scale, q = __builtin_rintf(y), f = y - q;
  bad = bad || !(x >= 0.0f) || !(y < BLK_LANE_MAX) || __builtin_fabsf(f) == 0.5f;
  isum += cvt_i32_sat(q);
}
// wave-wide: true and the new sum in acc if the block could be added exactly
__device__ __forceinline__ bool blk_finish(const BlkScale &b, int isum, bool bad, float &acc)
{
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) isum += __shfl_xor(isum, s, 64);
  const int ni = b.ai + isum;
  if (!b.ok || __ballot(bad) != 0ull || ni >= (1 << 24) || isum < 0) return false;
  acc = (float)ni * b.ulp;
  return true;
}
// all 64 lanes of the chain wave: acc + col[0 .. rows), as the term-by-term chain would leave it; every lane returns the sum
template <int NBUF>
__device__ __forceinline__ float chain_block_nonneg(const float *col, int rows, float acc)
{
  const int lane = threadIdx.x & 63;
  const BlkScale b = blk_scale(acc);
  int isum = 0;
  bool bad = false;
  for (int r = lane; r < rows; r += 64) blk_term(b, col[r], isum, bad);
  if (blk_finish(b, isum, bad, acc)) return acc;
  float r = acc;
  if (lane == 0) r = chain_tile<NBUF>(col, rows, acc);
  return uniform_f(r);
}

// The deferred dist_mean chain (executed by ONE wave, all 64 lanes enter): dterm[0 .. n) added strictly in order by lane 0.
// The wave streams the terms from HBM ICP_DT at a time (two coalesced float4 per lane, the next block in flight while
// this one is added) through its own LDS buffer `buf` (2 x ICP_DT floats); the array is padded to whole blocks.
template <int NBUF>
__device__ __forceinline__ float chain_deferred(const float *__restrict__ dterm, float (*buf)[ICP_DT], int n)
{
  const int lane = threadIdx.x & 63;
  const int nblk = (n + ICP_DT - 1) / ICP_DT;
  float acc = 0.0f;
  float4 r0, r1;
  if (nblk > 0) {
    r0 = *(const float4 *)(dterm + 4 * lane);
    r1 = *(const float4 *)(dterm + 256 + 4 * lane);
  }
  for (int b = 0; b < nblk; ++b) {
    const int cnt = min(ICP_DT, n - b * ICP_DT);
    const float4 c0 = r0, c1 = r1;
    if (b + 1 < nblk) {
      r0 = *(const float4 *)(dterm + (size_t)(b + 1) * ICP_DT + 4 * lane);
      r1 = *(const float4 *)(dterm + (size_t)(b + 1) * ICP_DT + 256 + 4 * lane);
    }
    {
      // the block straight from the registers it arrived in, as one exact integer sum (chain_block_nonneg); the words behind
      // term n - 1 of the last block are padding
      const BlkScale bs = blk_scale(acc);
      int isum = 0;
      bool bad = false;
      const float v[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
      for (int k = 0; k < 8; ++k) blk_term(bs, (k < 4 ? 4 * lane + k : 256 + 4 * lane + k - 4) < cnt ? v[k] : 0.0f, isum, bad);
      if (blk_finish(bs, isum, bad, acc)) continue;
    }
    float *dst = buf[b & 1];
    *(float4 *)(dst + 4 * lane) = c0;
    *(float4 *)(dst + 256 + 4 * lane) = c1;
    wave_lds_handover();
    if (lane == 0) acc = chain_tile<NBUF>(dst, cnt, acc);
    acc = uniform_f(acc);
  }
  return acc;                                            // every lane holds the sum
}

// ---- getL2distClouds (ICP.cpp:68-111) over the index-paired clouds, optionally fused with the
// in-place transformPoints that precedes it (ICP.cpp:28-45, 756).  FL_ICP_PARITY: the producer waves write
// the per-point terms into double-buffered LDS tiles while lane 0 of wave 0 adds the previous tile
// in index order (the reference's `dist_mean += dist` chain); one barrier per tile.
// Also maintains bnd[i], an upper bound on the distance from model point i to SOME reference point: the index pair
// before the first iteration (Ropt == nullptr), afterwards the bound grows by how far point i moved (the search
// replaces it by the distance it found).
// DEFER (parity mode, organised search): the terms go to dterm[] in HBM instead of LDS tiles and are NOT added here;
// every thread produces, the valid / inlier counts are left in S.cnt / S.inl, and the chain wave adds the terms later
// (chain_deferred) while the other waves already search for the next iteration.
// REFPIX (the 16-bit builds, every call but the initial one): reference point i is not read from ref[] (12 bytes) but rebuilt from
// its crop pixel pix[i] and depth factor zref[i] (6 bytes) by org_point, crop_clouds' own expression: bit for bit what ref[i] holds.
template <int MODE, bool DEFER, bool REFPIX, class SH>
__device__ __forceinline__ float l2dist_phase(SH &S, float *mod, const float *ref, bnd_t *bnd, float *dterm, int n, float thr,
                                             const float *Ropt, const float *Topt, const uint16_t *pix, const float *zref, const OrgGeom &og)
{
  constexpr bool parity = MODE == FL_ICP_PARITY && !DEFER;   // chains in this phase
  constexpr int TQ = parity ? SH::TQ : SH::BS;           // rows per tile
  const int slot = parity ? S.producer_slot() : (int)threadIdx.x;
  const int clane = parity ? S.chain_lane() : -1;        // lane of this thread in the chain wave, or -1
  int counter = 0, inl = 0;
  double dsum[1] = {0.0};
  float acc = 0.0f;
  const int ntiles = (n + TQ - 1) / TQ;
  // 256-thread parity kernel: the chain wave and the producers meet at a barrier every KB tiles, not every tile.  The chain is
  // one lane adding one float per row; at a barrier per 192 rows it spent 2 - 3 of its ~11 cycles per row there and in the LDS
  // round trip that opens each tile (phase stamps: 11.3 -> 9.5 cycles per row inside blocks of 4, 8.6 inside blocks of 8 -- but
  // the chain starts a block after the producers and ends a block after them, which is why 4 beats 8 and 15; blocks graded
  // 1, 1, 2, 2, 4, 4, 8 ... from both ends cost more in bookkeeping than they saved).  The terms of a block go to one of two
  // buffers of KB tiles in the (idle) tiles of phase A2.
  constexpr int KB = parity && !SH::BSUM ? ICP_BMACRO : 1;
  static_assert(KB == 1 || sizeof(S.prod) >= (size_t)2 * KB * TQ * sizeof(float), "two blocks of KB tiles of terms fit the A2 tiles");
  // Block 0 is tile 0 alone (the chain starts after one tile, not after KB), block m >= 1 the tiles (m - 1) KB + 1 .. m KB.
  auto dbuf = [&](int t) -> float * {                    // where the terms of tile t go
    if (KB == 1) return S.dtile[t & 1];
    const int m = (t + KB - 1) / KB, first = m == 0 ? 0 : (m - 1) * KB + 1;
    return (float *)&S.prod[0][0][0] + ((m & 1) * KB + (t - first)) * TQ;
  };
  // The phase is one memory round trip + one barrier per tile, so the next tile's (coalesced) loads are issued before this
  // tile is processed.  Two register sets trade roles by unrolling the tile loop twice -- never by moving registers, and
  // nothing computes with a loaded value in the iteration that issued its load: either makes the compiler drain the whole
  // memory queue (s_waitcnt vmcnt(0)) once per tile (see the A2 phase in icp_run).  With chains in this phase (parity) the
  // tile barrier is a raw s_barrier behind an lgkmcnt wait: the LDS tile must be complete, the global stores of this
  // phase (mod, bnd) need not be before the phase ends.
  struct Row { F3 a, b; float bnd; int p; };              // REFPIX: b.x = the depth factor, p = the crop pixel, until row_process
  const float inv_cw = REFPIX ? uniform_f(1.0f / (float)max(og.cw, 1)) : 0.0f;
  auto row_load = [&](Row &w, int t) {
    const int i = min(t * TQ + slot, n - 1);              // clamped: unused past the end
    w.a = ld3_u32(mod, i);
    if (REFPIX) { w.p = ld_u32(pix, i); w.b.x = ld_u32(zref, i); }
    else w.b = ld3_u32(ref, i);
    w.bnd = Ropt ? bnd_ld(bnd, i) : 0.0f;
  };
  auto row_process = [&](const Row &w, int t) {
    const int i = t * TQ + slot;
    float term = 0.0f;
    float a[3] = {w.a.x, w.a.y, w.a.z};
    F3 rp = w.b;
    if (REFPIX) {
      // the pixel's crop row by a float reciprocal and one correction step (phase A2's row_write): exact, the pixel is below 2^16
      int vv = (int)(((float)w.p + 0.5f) * inv_cw), uu = w.p - __mul24(vv, og.cw);
      if (uu < 0) { --vv; uu += og.cw; } else if (uu >= og.cw) { ++vv; uu -= og.cw; }
      rp = org_point(og, uu, vv, w.b.x);
    }
    const float b0 = rp.x, b1 = rp.y, b2 = rp.z;
    if (i < n) {
      if (Ropt) {
        float move = 0.0f;
        if (vvalid(a[2])) {                               // transformPoints in place (:28-45, :756)
          float o[3];
          mat_vec(Ropt, a, o);
          o[0] += Topt[0];
          o[1] += Topt[1];
          o[2] += Topt[2];
          const float mx = o[0] - a[0], my = o[1] - a[1], mz = o[2] - a[2];
          move = sqrt_upper(mx * mx + my * my + mz * mz);
          a[0] = o[0];
          a[1] = o[1];
          a[2] = o[2];
          mod[3 * i] = a[0];
          mod[3 * i + 1] = a[1];
          mod[3 * i + 2] = a[2];
        }
        bnd_st(bnd, i, w.bnd + move);                     // triangle inequality: still reaches the old partner
      } else {
        // first bound: the index pair (n_ref >= n_model); NaN/inf simply disable the bound
        const float ex = a[0] - b0, ey = a[1] - b1, ez = a[2] - b2;
        bnd_st(bnd, i, sqrt_upper(ex * ex + ey * ey + ez * ez));
      }
      if (vvalid(b2) && vvalid(a[2])) {
        const float dx = a[0] - b0, dy = a[1] - b1, dz = a[2] - b2;
        // cv::norm(Vec3f): squares accumulated in double, sqrt in double, stored to float (:88)
        const float dist = (float)sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
        if (dist <= thr) { term = dist; ++inl; dsum[0] += (double)dist; }
        ++counter;
      }
    }
    if (parity) dbuf(t)[slot] = term;                     // non-inliers add an exact +0.0f
    if (DEFER && i < n) dterm[i] = term;
  };
  // tile t (block t of KB tiles) is complete in LDS: the chain wave adds it (every lane of the wave enters)
  auto chain_step = [&](int t) {
    const int first = KB == 1 || t == 0 ? t : (t - 1) * KB + 1, last = KB == 1 || t == 0 ? t : t * KB;   // the block's tiles
    const float *col = dbuf(first);
    const int rows = min((last + 1) * TQ, n) - first * TQ;
    if (SH::BSUM) acc = chain_block_nonneg<SH::CHAIN_NBUF>(col, rows, acc);
    else if (clane == 0) acc = chain_tile<SH::CHAIN_NBUF>(col, rows, acc);
  };
  // blocks of tiles; barriers inside the phase: behind every COMPLETE block (tile 0, tile KB, tile 2 KB, ...)
  const int nblocks = KB == 1 ? ntiles : (ntiles > 0 ? (ntiles - 1 + KB - 1) / KB + 1 : 0);
  const int nbar = KB == 1 ? ntiles : (ntiles > 0 ? (ntiles - 1) / KB + 1 : 0);
  auto block_barrier = [&](int t) {                       // behind tile t: the barrier that closes a block
    if (parity && (KB == 1 || t % KB == 0)) tile_barrier();
  };
  const bool chain_wave = parity && __builtin_amdgcn_readfirstlane(clane) >= 0;
  if (chain_wave) {
    // the chain wave's own loop (see the A2 phase): one barrier per tile like the producers' below
    CH_STAMP_BEGIN;
    for (int t = 0; t < nbar; ++t) {
      if (t > 0) chain_step(t - 1);
      CH_STAMP(c_add);
      tile_barrier();
      CH_STAMP(c_bar);
    }
    CH_STAMP_END(26);
  } else if (slot >= 0) {
    // one tile of loads in flight per thread: two register sets trade roles by unrolling (see above)
    Row A, B;
    if (ntiles > 0) row_load(A, 0);
    for (int t = 0; t < ntiles; t += 2) {
      row_load(B, t + 1);
      row_process(A, t);
      block_barrier(t);
      if (t + 1 < ntiles) {
        row_load(A, t + 2);
        row_process(B, t + 1);
        block_barrier(t + 1);
      }
    }
  } else if (parity) {
    for (int t = 0; t < nbar; ++t) tile_barrier();         // a wave that neither chains nor produces (1024-thread workgroup)
  }
  __syncthreads();                                         // the phase's stores (mod, bnd, dterm) are visible to the workgroup
  if (parity && chain_wave)                                // the blocks the loop above has not added: the last one, or the last two
    for (int t = max(nbar - 1, 0); t < nblocks; ++t) chain_step(t);
  counter = block_sum_int(S, counter);
  inl = block_sum_int(S, inl);
  if (DEFER) {
    // An upper bound of the dist_mean the chain will produce, from a parallel fp64 sum P of the same terms: the float32
    // chain c of n non-negative terms satisfies c <= (1 + n u) E, u = 2^-24, E the exact sum (and P = E to 1e-12), and
    // the division adds one rounding.
    block_sum_double<1>(S, dsum);
    if (threadIdx.x == 0) { S.cnt = counter; S.inl = inl; }
    const double P = S.dsum[0][0];
    __syncthreads();
    if (counter <= 0) return INFINITY;                   // dist_mean = FLT_MAX
    return (float)(P / (double)inl * (1.0 + 1.3e-7 * (double)n + 1.0e-6)) * 1.000001f;      // 0 inliers: NaN, as dist_mean will be
  }
  float dm;
  if (parity) {
    if (clane == 0) S.sums[0] = acc;
    __syncthreads();
    dm = S.sums[0];
    if (counter > 0) dm /= (float)inl;                   // 0/0 -> NaN ends the loop (Q9)
  } else {
    block_sum_double<1>(S, dsum);
    dm = counter > 0 ? (float)(S.dsum[0][0] / (double)inl) : 0.f;
  }
  if (threadIdx.x == 0) {
    if (counter > 0) {
      S.dist_mean = dm;
      S.px = (float)inl / (float)counter;
    } else {
      S.dist_mean = FLT_MAX;
      S.px = 0.0f;
    }
  }
  __syncthreads();
  return 0.0f;
}

// ---- the pose solvers of an iteration and the pose accumulation (one thread, from the sums in S.sums / S.dsum[0]) ----
// R_optimal, T_optimal from the 9 products and the two centroids' sums (ICP.cpp:737-748); S.ok = checkRange
template <int MODE, class SH>
__device__ __forceinline__ void solve_rigid(SH &S, int ncm, int ncr)
{
  float C[9], mc[3], rc[3];
  if (MODE == FL_ICP_PARITY) {
    for (int k = 0; k < 9; ++k) C[k] = S.sums[k];
    for (int k = 0; k < 3; ++k) { mc[k] = S.sums[9 + k] / (float)ncm; rc[k] = S.sums[12 + k] / (float)ncr; }   // getMean :19-24
  } else {
    for (int k = 0; k < 9; ++k) C[k] = (float)S.dsum[0][k];
    for (int k = 0; k < 3; ++k) { mc[k] = (float)(S.dsum[0][9 + k] / ncm); rc[k] = (float)(S.dsum[0][12 + k] / ncr); }
  }
  float u[9], vt[9];
  svd3(C, u, vt);                                    // :742
  for (int i = 0; i < 3; ++i)                        // R_optimal = Mat(vt.t() * u.t()) :744 (gemm: double acc)
    for (int j = 0; j < 3; ++j) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += (double)vt[k * 3 + i] * (double)u[j * 3 + k];
      S.Ropt[i * 3 + j] = (float)s;
    }
  float Rm[3];
  mat_vec(S.Ropt, mc, Rm);
  for (int k = 0; k < 3; ++k) S.Topt[k] = rc[k] - Rm[k];                      // :747
  S.ok = finite_all(S.Ropt, 9) && finite_all(S.Topt, 3);                      // checkRange :748
}
// FL_ICP_POINT_TO_PLANE: the 6x6 normal equations (21 + 6 sums) by Cholesky, the rotation by Rodrigues; S.ok = solvable and finite
template <class SH>
__device__ __forceinline__ void solve_point_to_plane(SH &S)
{
  double A[6][6], x[6], tr = 0.0;
  int q = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = S.dsum[0][q++];
  for (int a = 0; a < 6; ++a) { x[a] = -S.dsum[0][21 + a]; tr += A[a][a]; }
  bool ok = tr > 0.0 && tr < 1.0e300;
  for (int a = 0; a < 6; ++a) A[a][a] += 1.0e-12 * tr;          // keeps a barely constrained direction finite
  for (int c = 0; c < 6 && ok; ++c) {                            // Cholesky A = L L^T (lower triangle in place)
    double d = A[c][c];
    for (int k = 0; k < c; ++k) d -= A[c][k] * A[c][k];
    if (!(d > 1.0e-13 * tr)) { ok = false; break; }              // a direction the pairs do not constrain
    d = sqrt(d);
    A[c][c] = d;
    for (int r = c + 1; r < 6; ++r) {
      double v = A[r][c];
      for (int k = 0; k < c; ++k) v -= A[r][k] * A[c][k];
      A[r][c] = v / d;
    }
  }
  if (ok) {
    for (int r = 0; r < 6; ++r) {                                // L y = b
      double v = x[r];
      for (int k = 0; k < r; ++k) v -= A[r][k] * x[k];
      x[r] = v / A[r][r];
    }
    for (int r = 5; r >= 0; --r) {                               // L^T x = y
      double v = x[r];
      for (int k = r + 1; k < 6; ++k) v -= A[k][r] * x[k];
      x[r] = v / A[r][r];
    }
    // Rodrigues: R = I + (sin t / t) K + ((1 - cos t) / t^2) K^2, K = [omega]x
    const double wx = x[0], wy = x[1], wz = x[2], t2 = wx * wx + wy * wy + wz * wz, t = sqrt(t2);
    const double sa = t > 1.0e-9 ? sin(t) / t : 1.0 - t2 / 6.0, sb = t > 1.0e-9 ? (1.0 - cos(t)) / t2 : 0.5 - t2 / 24.0;
    const double Kx[9] = {0, -wz, wy, wz, 0, -wx, -wy, wx, 0};
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double k2 = 0;
        for (int k = 0; k < 3; ++k) k2 += Kx[i * 3 + k] * Kx[k * 3 + j];
        S.Ropt[i * 3 + j] = (float)((i == j ? 1.0 : 0.0) + sa * Kx[i * 3 + j] + sb * k2);
      }
    for (int k = 0; k < 3; ++k) S.Topt[k] = (float)x[3 + k];
  }
  S.ok = ok && finite_all(S.Ropt, 9) && finite_all(S.Topt, 3);
}
// T = Ropt T + Topt, R = Ropt R (:793-797)
template <class SH>
__device__ __forceinline__ void pose_accumulate(SH &S)
{
  float RT[3];
  mat_vec(S.Ropt, S.T, RT);
  for (int k = 0; k < 3; ++k) S.T[k] = RT[k] + S.Topt[k];
  mat_mat(S.Ropt, S.R, S.R);
}
// the result of a run that cannot start (:633-638)
__device__ __forceinline__ void icp_result_none(fl_icp_result *res)
{
  for (int i = 0; i < 9; ++i) res->R[i] = 0.f;
  for (int i = 0; i < 3; ++i) res->T[i] = 0.f;
  res->dist_mean = -1.0f; res->px_ratio = 0.f;
  res->iters = 0; res->n_corr_last = 0;
}

// ---- the first pass of the 256-thread parity pipeline kernel ------------------------------------------------------------------
// Four passes of the reference read the same rows in the same index order before the first searched iteration, and their 16
// float32 chains are independent of each other: transformPoints(pts_mod, I, t_match_tmp) (detection.cpp:206), copyPoints
// (ICP.cpp:666-667), the initial getL2distClouds (:670) and iteration 1's getMean x2 + covariance loop over the index pairs
// (:700-704, :731-735).  Here they are ONE producer / chain pass shaped like l2dist_phase's: each model point is loaded raw,
// pre-translated by `pre_t` with the very expression of the transform (mat_vec(I, v) + t), zeroed if its new z is not valid,
// and stored once; the row's first bnd[], its 15 products (S.prod) and its distance term (S.dtile) follow from the registers.
// Lanes 0 - 14 of the chain wave add their column of S.prod, lane 15 adds S.dtile: sixteen chains, one barrier per tile.
// Leaves S.dist_mean / S.px as the initial l2dist_phase does and iteration 1's sums in S.first_sums (the loop head decides
// whether the iteration runs; if not, they are dropped).  n >= 3; in the pipeline n_ref == n_model == n.
template <class SH>
__device__ __forceinline__ void first_pass(SH &S, float *mod, const float *ref, bnd_t *bnd, int n, const float *pre_t)
{
  constexpr int TQ = SH::TQ;
  const int slot = S.producer_slot(), clane = S.chain_lane();
  const int ntiles = (n + TQ - 1) / TQ;
  const float thr = FLT_MAX;
  int counter = 0, inl = 0;
  float acc = 0.0f;
  struct Row { F3 m, r; };
  auto row_load = [&](Row &w, int t) {                   // issue only (see l2dist_phase)
    const int i = min(t * TQ + slot, n - 1);              // clamped: unused past the end
    w.m = ld3_u32(mod, i);
    w.r = ld3_u32(ref, i);
  };
  auto row_process = [&](const Row &w, int t) {
    const int i = t * TQ + slot;
    float m[3] = {0.f, 0.f, 0.f}, r[3] = {0.f, 0.f, 0.f}, term = 0.0f;
    if (i < n) {
      float a[3] = {w.m.x, w.m.y, w.m.z};
      if (vvalid(a[2])) {                                 // transformPoints(pts_mod, I, t_match_tmp) detection.cpp:206
        const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        float o[3];
        mat_vec(I, a, o);
        a[0] = o[0] + pre_t[0];
        a[1] = o[1] + pre_t[1];
        a[2] = o[2] + pre_t[2];
      }
      if (!vvalid(a[2])) { a[0] = 0.f; a[1] = 0.f; a[2] = 0.f; }    // copyPoints :666-667: invalid points become Vec3f() = 0
      mod[3 * i] = a[0];
      mod[3 * i + 1] = a[1];
      mod[3 * i + 2] = a[2];
      const float b0 = w.r.x, b1 = w.r.y, b2 = w.r.z;
      // first bound: the index pair; NaN/inf simply disable the bound
      const float ex = a[0] - b0, ey = a[1] - b1, ez = a[2] - b2;
      bnd_st(bnd, i, sqrt_upper(ex * ex + ey * ey + ez * ez));
      if (vvalid(b2) && vvalid(a[2])) {                   // getL2distClouds :68-111, dist_thr = FLT_MAX
        const float dx = a[0] - b0, dy = a[1] - b1, dz = a[2] - b2;
        // cv::norm(Vec3f): squares accumulated in double, sqrt in double, stored to float (:88)
        const float dist = (float)sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
        if (dist <= thr) { term = dist; ++inl; }
        ++counter;
      }
      // iteration 1 pairs by index, invalid -> 0 (:700-704)
      if (vvalid(a[2])) { m[0] = a[0]; m[1] = a[1]; m[2] = a[2]; }
      if (vvalid(b2)) { r[0] = b0; r[1] = b1; r[2] = b2; }
    }
    float (*tile)[SH::TS] = S.prod[t & 1];
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = 0; q < 3; ++q) tile[p * 3 + q][slot] = m[p] * r[q];     // (*it_s) * (*it_ref).t()
#pragma unroll
    for (int q = 0; q < 3; ++q) { tile[9 + q][slot] = m[q]; tile[12 + q][slot] = r[q]; }
    S.dtile[t & 1][slot] = term;                          // non-inliers add an exact +0.0f
  };
  // the chain lane's column of tile t: one of the 15 of S.prod, or the distance terms
  auto chain_step = [&](int t) {
    const float *col = clane < 15 ? S.prod[t & 1][clane] : S.dtile[t & 1];
    acc = chain_tile<SH::CHAIN_NBUF>(col, min(TQ, n - t * TQ), acc);
  };
  const bool chain_wave = __builtin_amdgcn_readfirstlane(clane) >= 0;
  if (chain_wave) {
    for (int t = 0; t < ntiles; ++t) {
      if (t > 0 && clane < 16) chain_step(t - 1);
      tile_barrier();
    }
  } else if (slot >= 0) {
    // one tile of loads in flight per thread: two register sets trade roles by unrolling (see l2dist_phase)
    Row A, B;
    row_load(A, 0);
    for (int t = 0; t < ntiles; t += 2) {
      row_load(B, t + 1);
      row_process(A, t);
      tile_barrier();
      if (t + 1 < ntiles) {
        row_load(A, t + 2);
        row_process(B, t + 1);
        tile_barrier();
      }
    }
  }
  __syncthreads();                                         // the pass's stores (mod, bnd) are visible to the workgroup
  if (chain_wave && clane < 16) chain_step(ntiles - 1);
  counter = block_sum_int(S, counter);
  inl = block_sum_int(S, inl);
  if (clane >= 0 && clane < 15) S.first_sums[clane] = acc;
  if (clane == 15) S.sums[0] = acc;
  __syncthreads();
  float dm = S.sums[0];
  if (counter > 0) dm /= (float)inl;                       // 0/0 -> NaN ends the loop (Q9)
  if (threadIdx.x == 0) {
    if (counter > 0) {
      S.dist_mean = dm;
      S.px = (float)inl / (float)counter;
    } else {
      S.dist_mean = FLT_MAX;
      S.px = 0.0f;
    }
  }
  __syncthreads();
}

// ---- icpCloudToCloud_Ex (ICP.cpp:617-809) --------------------------------------------------------
// ORG: the reference cloud is also available as the image `og` describes (sref = image of points + image of indices, perm = tile order), see
// "Organised search" at the top; otherwise the grid is built here and searched.
// IDX: the type nn[] and perm[] are stored in: int, or uint16_t in the 16-bit builds of the 256-thread parity kernel ("none" is
// IDX(-1), read back as -1: nn_get), which also rebuild phase B's reference point from pix[] / zref[] (l2dist_phase<REFPIX>).
template <class IDX>
__device__ __forceinline__ int nn_get(IDX v) { return sizeof(IDX) == 2 && (int)v == 0xFFFF ? -1 : (int)v; }
// FIRST (the 256-thread parity pipeline kernel; n_ref == n_model): the caller has NOT applied its pre-translation `pre_t` to mod[];
// first_pass applies it together with copyPoints, the initial distances and iteration 1's sums.  Everyone else passes null.
template <int MODE, bool ORG, class IDX, bool FIRST = false, class SH>
__device__ __forceinline__ void icp_run(SH &S, uint8_t *wsb, const IcpWsLayout &L, int n_ref, int n_model,
                        int it_thr, float dmt, float ddt, fl_icp_result *res, const OrgGeom &og, const float *pre_t = nullptr)
{
  constexpr int BS = SH::BS, NW = SH::NW;
  float *ref = (float *)(wsb + L.ref), *mod = (float *)(wsb + L.mod);
  float4 *sref = (float4 *)(wsb + L.sref);
  // where the partner of nn[i] = j is read from: the organised search names it by its crop pixel (the image of points),
  // the grid search by its index (ref[]); idximg maps a pixel to its index (point-to-plane: normals are stored by index)
  const float *jsrc = ORG ? (const float *)sref : ref;
  const int *idximg = ORG ? (const int *)((const uint8_t *)sref + org_idximg_offset(og.cw * og.ch)) : nullptr;
  constexpr bool IDX16 = sizeof(IDX) == 2;
  static_assert(!IDX16 || (MODE == FL_ICP_PARITY && ORG && SH::NW < 8), "16-bit indices: the 256-thread parity kernel of the organised search only");
  IDX *nn = (IDX *)(wsb + L.nn);
  bnd_t *bnd = (bnd_t *)(wsb + L.bnd);
  float *nd = (float *)(wsb + L.nd), *dterm = (float *)(wsb + L.dterm);
  const IDX *perm = (const IDX *)(wsb + L.perm);
  // 16-bit builds: the crop pixel and depth factor of point i, in the regions this kernel leaves unused (crop_clouds)
  const uint16_t *pix = (const uint16_t *)(wsb + L.dterm);
  const float *zref = (const float *)(wsb + L.nd);
  const float *nrm = (const float *)(wsb + L.nrm);
  int *cell_start = (int *)(wsb + L.cell_start), *cell_cur = (int *)(wsb + L.cell_cur);
  constexpr bool plane = MODE == FL_ICP_POINT_TO_PLANE;
  constexpr int NSUM = plane ? 27 : 15;

  if (threadIdx.x == 0) {
    for (int i = 0; i < 9; ++i) S.R[i] = 0.f;           // cv::Matx33f R; cv::Vec3f T; zero-initialised
    for (int i = 0; i < 3; ++i) S.T[i] = 0.f;
    S.iter = 0;
    S.n_corr = 0;
    S.px = 0.f;
#ifdef FL_ICP_PHASES
    for (int i = 0; i < 16; ++i) S.tacc[i] = 0;
    for (int i = 0; i < 40; ++i) S.hist[i] = 0;
    for (int i = 0; i < 8; ++i) S.stime[i] = 0;
    S.tlast = clock64();
    S.tacc[6] = S.tlast - S.tkernel;
#endif
  }
  __syncthreads();
  if (n_model < 3 || n_ref < 3 || n_ref < n_model) {    // :633-638 (n_ref < n_model: reference reads OOB)
    if (threadIdx.x == 0) icp_result_none(res);
    __syncthreads();
    return;
  }
  if (!ORG) build_grid(S, ref, n_ref, sref, cell_start, cell_cur, L.ncell_max);
  TSTAMP(0);
  SSTAMP(9);
  // copyPoints(pts_model, pts_model_tmp) (:666-667): invalid points become Vec3f() = 0
  if (!FIRST)
    for (int i = threadIdx.x; i < n_model; i += BS)
      if (!vvalid(mod[3 * i + 2])) { mod[3 * i] = 0.f; mod[3 * i + 1] = 0.f; mod[3 * i + 2] = 0.f; }
  if (threadIdx.x == 0) {
    S.R[0] = S.R[4] = S.R[8] = 1.f;                      // R = eye, T = 0 (:644-645)
    S.dist_diff = FLT_MAX;
  }
  __syncthreads();
  SSTAMP(5);
  // Search ahead of the distance chain (parity mode, organised search).  getL2distClouds' dist_mean is one float32 chain over
  // all points: alone it costs a quarter of an iteration during which every wave but one waits.  So the terms are written
  // to dterm[] (l2dist_phase<DEFER>), and while the chain wave adds them the other waves already run PointsCorresponding for
  // the NEXT iteration -- against a threshold that is not known yet.  It needs none: the search radius of a point is
  // min(bnd[i], r_lim) with r_lim >= sqrt(3 dist_mean) whatever the chain will find (l2dist_phase returns an upper bound
  // of its result, a fraction of a percent above a parallel sum of the same terms), the exact neighbour and its distance
  // are stored (nn[], nd[]), and `d <= 3 dist_mean` (:268) is applied where the pairs are consumed.  A wider radius only
  // visits more pixels; the neighbour found is the same.  If the chain ends the loop, the search is abandoned (S.stop).
  // Only the 1024-thread workgroup (batches that leave CUs idle) does this: with four 256-thread workgroups per CU the
  // other workgroups already fill the chain's shadow, and the extra traffic (dterm, nd) costs 7 % there (profiles/README.md).
  constexpr bool SPEC = BS >= ICP_BS_WIDE && MODE == FL_ICP_PARITY && ORG;
  static_assert(!(IDX16 && SPEC), "pix[] / zref[] live where the deferred chain keeps dterm[] / nd[]");
  static_assert(!FIRST || (MODE == FL_ICP_PARITY && ORG && !SPEC), "first_pass: the 256-thread parity pipeline kernel only");
  float mean_ub = 0.0f;
  if constexpr (FIRST) first_pass(S, mod, ref, bnd, n_model, pre_t);      // :670 with what precedes and follows it
  else mean_ub = l2dist_phase<MODE, SPEC, false>(S, mod, ref, bnd, dterm, n_model, FLT_MAX, nullptr, nullptr, pix, zref, og);   // :670
  SSTAMP(6);
  int pending = SPEC ? 1 : 0;                            // 1: the initial distances await their chain, 2: an iteration's
  bool have_nn = false;                                  // nn[] / nd[] hold the neighbours of the current model cloud
  float old_mean = 0.0f;                                 // dist_mean before the pending distances (pending == 2)

  // what the organised searches read (fl_icp_search.h); the pairs they find go to the `found` callables below
  const auto ctx = org_search_ctx(mod, bnd, perm, (const float *)sref, (const float *)(wsb + L.zimg), n_model, og);
  // the deferred dist_mean chain of the pending distances (chain wave), then -- every wave -- the search for the next iteration
  auto chain_and_search = [&](const int pend, const bool want, const float r_lim, const float old_mean_) {
    if (pend && threadIdx.x < 64) {
      const float acc = chain_deferred<SH::CHAIN_NBUF>(dterm, S.dchain, n_model);
      if (threadIdx.x == 0) {
        const int counter = S.cnt, inl = S.inl;
        float dm = acc;
        if (counter > 0) dm /= (float)inl;               // 0/0 -> NaN ends the loop (Q9)
        const float new_mean = counter > 0 ? dm : FLT_MAX;
        S.px = counter > 0 ? (float)inl / (float)counter : 0.0f;
        if (pend == 2) {
          S.dist_diff = old_mean_ - new_mean;
          pose_accumulate(S);
        }
        S.dist_mean = new_mean;
        const bool go = (new_mean > dmt) && (S.dist_diff > ddt) && (S.iter < it_thr);       // :684, as the loop head will find it
        *(volatile int *)&S.stop = go ? 0 : 1;
      }
    }
    if (want)
      org_search<SH, SPEC>(S, ctx, r_lim, true, [&](bool active, int i, float, float, float, int j, float d) {
        if (active) {
          nn[i] = (IDX)j;
          nd[i] = d;
          if (j >= 0) bnd_st(bnd, i, sqrt_upper(d));             // else: the old partner is still within the old bound
        }
      });
  };

  for (;;) {
    if (SPEC) {
      const int it_done = __builtin_amdgcn_readfirstlane(S.iter);
      const bool want = !have_nn && it_done >= 1 && it_done < it_thr;   // the next iteration, if there is one, searches
      if (pending || want) {
        const float r_lim = pending ? sqrtf(3.0f * mean_ub) * 1.00001f : sqrtf(3 * S.dist_mean);
        if (threadIdx.x == 0) { S.a1_next = 0; S.stop = 0; }
        __syncthreads();
        chain_and_search(pending, want, uniform_f(r_lim), old_mean);
        __syncthreads();                                 // dist_mean, nn[], nd[], bnd[] complete
        TSTAMP(2);
        if (want) have_nn = true;
        pending = 0;
      }
    }
    if (threadIdx.x == 0) S.go = (S.dist_mean > dmt) && (S.dist_diff > ddt) && (S.iter < it_thr);   // :684
    __syncthreads();
    if (!S.go) break;
    // point-to-plane gates pairs at distance 3*dist_mean; the reference compares the SQUARED distance
    // with 3*dist_mean (Q9), which parity/fast keep
    if (threadIdx.x == 0) { ++S.iter; S.thr = plane ? (3 * S.dist_mean) * (3 * S.dist_mean) : 3 * S.dist_mean; S.a1_next = 0; }
    __syncthreads();
    const int iter = __builtin_amdgcn_readfirstlane(S.iter);
    const float thr = uniform_f(S.thr);
    const int rows = iter == 1 ? n_ref : n_model;
    constexpr bool parity = MODE == FL_ICP_PARITY;
    int kept = 0;
    const bool index_pairs = iter == 1 && !plane;       // :700-704
    // fast and point-to-plane: per-thread partials.  The thread's ~60 terms are summed in float32 (27 registers
    // instead of 54) and only the cross-thread tree runs in fp64; the point-to-plane 6x6 system is re-linearised every
    // iteration, so a 1e-6 relative error in a sum is immaterial.
    float ds[NSUM];
#pragma unroll
    for (int k = 0; k < NSUM; ++k) ds[k] = 0.0;
    // a kept pair (model point m, reference point r with index j) enters the sums of the modes that do not chain
    auto pair_sums = [&](float m0, float m1, float m2, float r0, float r1, float r2, int j) {
      if (plane) {
        // linearised point-to-plane: residual e = n.(m - r), Jacobian row J = [m x n, n] wrt (omega, t);
        // ds = upper triangle of sum J J^T (21) followed by sum J e (6)
        const F3 nv = ld3_u32(nrm, ORG ? ld_u32(idximg, j) : j);
        const float n0 = nv.x, n1 = nv.y, n2 = nv.z;
        const float J[6] = {m1 * n2 - m2 * n1, m2 * n0 - m0 * n2, m0 * n1 - m1 * n0, n0, n1, n2};
        const float e = n0 * (m0 - r0) + n1 * (m1 - r1) + n2 * (m2 - r2);
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
          for (int b = a; b < 6; ++b) ds[q++] += J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) ds[21 + a] += J[a] * e;
      } else if (!parity) {
        const float m[3] = {m0, m1, m2}, r[3] = {r0, r1, r2};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) ds[a * 3 + b] += (double)m[a] * (double)r[b];
#pragma unroll
        for (int q = 0; q < 3; ++q) { ds[9 + q] += (double)m[q]; ds[12 + q] += (double)r[q]; }
      }
    };
    if (!index_pairs && !SPEC) {
      // Phase A1 -- PointsCorresponding (:193-279): all waves search.  bnd[i] (distance to the partner found
      // last time plus the motion since; initially the index pair) bounds the search radius, so a converging
      // cloud visits only a handful of candidates per point; the result is still the exact 1-NN.
      const float r_thr = uniform_f(sqrtf(thr));
      auto on_found = [&](bool active, int i, float qx, float qy, float qz, int j, float d) {
        const bool keep = d <= thr;                       // dists[i][0] <= dist_thr (:268)
        if (active) {
          nn[i] = (IDX)(keep ? j : -1);
          if (j >= 0) bnd_st(bnd, i, sqrt_upper(d));      // else: the old partner is still within the old bound
        }
        if (keep) {
          ++kept;
          if (!parity) { const F3 rv = ld3_u32(jsrc, j); pair_sums(qx, qy, qz, rv.x, rv.y, rv.z, j); }
        }
      };
      if (ORG) {
        if (MODE == FL_ICP_PARITY && NW < 8) org_search_pipe(S, ctx, r_thr, on_found);   // the 256-thread parity kernel
        else org_search<SH, SPEC>(S, ctx, r_thr, false, on_found);
      } else {
        const NnGrid G = nn_grid(S);
        int i = threadIdx.x;
        float qx = 0.f, qy = 0.f, qz = 0.f, qb = 0.f;
        if (i < n_model) { const F3 q3 = ld3_u32(mod, i); qx = q3.x; qy = q3.y; qz = q3.z; qb = bnd_ld(bnd, i); }
        for (; i < n_model; i += BS) {
          const int in = min(i + BS, n_model - 1);           // clamped: unused past the end
          const F3 nq3 = ld3_u32(mod, in);
          const float nqx = nq3.x, nqy = nq3.y, nqz = nq3.z, nqb = bnd_ld(bnd, in);
          int j = -1;
          float d = NAN;
          if (thr >= 0.f && isfinite(qx) && isfinite(qy) && isfinite(qz))
            nn_search_grid(G, sref, cell_start, qx, qy, qz, nn_radius(qx, qy, qz, fminf(qb, r_thr)), &j, &d);
          on_found(true, i, qx, qy, qz, j, d);
          qx = nqx; qy = nqy; qz = nqz; qb = nqb;
        }
      }
      __syncthreads();                                   // nn[] complete
      TSTAMP(2);
    }
    // Phase A2 (iteration 1: the only phase): rows in index order.  Parity mode: the producer waves write
    // the 15 scalars of each row into double-buffered LDS tiles, wave 0 adds the previous tile
    // in row order -- getMean (:8-25) and the covariance loop (:731-735) as 15 float32 chains.
    constexpr int TQ = parity ? SH::TQ : BS;
    const int slot = parity ? S.producer_slot() : (int)threadIdx.x;
    const int clane = parity ? S.chain_lane() : -1;      // lane of this thread in the chain wave, or -1
    const bool summed = FIRST && iter == 1;              // first_pass has left this iteration's sums in S.first_sums
    const int ntiles = ((parity || index_pairs) && !summed) ? (rows + TQ - 1) / TQ : 0;
    float acc = 0.0f;                                    // chain accumulator of lane k < 15 of wave 0
    SSTAMP(9);
    if (parity && iter > 1) {
      // Register pipeline of the producers: a tile row costs its nn / mod loads (coalesced) and then the dependent gather
      // ref[j]; with thousands of frames in flight both come from HBM (thousands of cycles under load) while the chain
      // needs a tile every TQ * 8 cycles.  Three tiles are in flight per thread -- loaded (t + 2), gathered (t + 1), written
      // (t) -- in three register sets that trade roles by UNROLLING the tile loop three times, never by moving registers:
      // a rotation by moves reads the registers of loads that were issued in the same iteration, and the compiler answers it
      // with s_waitcnt vmcnt(0) -- every tile then waits for a full memory round trip and the prefetch is void (that was
      // the state of round 2: "1 / 2 / 3 / 4 tiles ahead measure the same").  For the same reason nothing computes with a
      // loaded value in the iteration that issued its load (the kept-pair test is applied where the row is gathered), and
      // the tile barrier is a raw s_barrier behind an lgkmcnt wait: the LDS tile must be complete, the loads in flight and
      // this phase's own global stores need not be (__syncthreads would drain them: it is a fence).
      struct Row {                                         // one tile row of this thread on its way to LDS
        int j;                                             // nearest reference index (valid from the gather on)
        float d;                                           // SPEC: its squared distance
        bool in;                                           // the row exists (below `rows`)
        F3 m, r;                                           // model point, reference point (ZIMG: r.x = its depth factor until row_write)
      };
      constexpr bool ZIMG = ORG && NW < 8;
      const float *zimg = (const float *)(wsb + L.zimg);
      const float inv_cw = uniform_f(1.0f / (float)max(og.cw, 1));
      auto row_load = [&](Row &w, int t) {                 // issue only: nothing here reads what it loads
        const int i = t * TQ + slot;
        w.in = i < rows;
        const int ic = min(i, rows - 1);                   // clamped: unused past the end
        w.j = ld_u32(nn, ic);
        w.d = SPEC ? ld_u32(nd, ic) : 0.0f;
        w.m = ld3_u32(mod, ic);
      };
      auto row_gather = [&](Row &w) {                      // SPEC: nn[] holds the neighbour whatever its distance; the pair is kept
        if (!(w.in && (!SPEC || w.d <= thr)) || (IDX16 && w.j == 0xFFFF)) w.j = -1;   // if d <= dist_thr (:268; NaN = none found);
                                                           // 16-bit builds: "none" was stored as 0xFFFF
        if (ZIMG) w.r.x = ld_u32(zimg, max(w.j, 0));      // 4 bytes: the partner pixel's depth factor (rebuilt in row_write)
        else w.r = ld3_u32(jsrc, max(w.j, 0));
      };
      auto row_write = [&](const Row &w, int t) {
        const bool have = w.j >= 0;                        // dropped pairs contribute an exact +0.0f: (+0) * (+0)
        if (SPEC && have) ++kept;
        float (*tile)[SH::TS] = S.prod[t & 1];
        F3 rp = w.r;
        if (ZIMG) {                                        // the partner's point from its pixel and depth factor (org_point)
          // its crop row by a float reciprocal and one correction step instead of an integer division (three quarter-rate
          // multiplies): exact for every pixel index (the estimate is off by at most one below 2^24 pixels; beyond: divide)
          const int jj = max(w.j, 0);
          int vv, uu;
          if (ctx.small_crop) {
            vv = (int)(((float)jj + 0.5f) * inv_cw);
            uu = jj - __mul24(vv, og.cw);
            if (uu < 0) { --vv; uu += og.cw; } else if (uu >= og.cw) { ++vv; uu -= og.cw; }
          } else {
            vv = jj / og.cw;
            uu = jj - vv * og.cw;
          }
          rp = org_point(og, uu, vv, w.r.x);
        }
        const float mm[3] = {have ? w.m.x : 0.0f, have ? w.m.y : 0.0f, have ? w.m.z : 0.0f};
        const float rr[3] = {have ? rp.x : 0.0f, have ? rp.y : 0.0f, have ? rp.z : 0.0f};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) tile[a * 3 + b][slot] = mm[a] * rr[b];   // (*it_s) * (*it_ref).t()
#pragma unroll
        for (int q = 0; q < 3; ++q) { tile[9 + q][slot] = mm[q]; tile[12 + q][slot] = rr[q]; }
      };
      const bool chain_wave = __builtin_amdgcn_readfirstlane(clane) >= 0;
      if (chain_wave) {
        // the chain wave's own loop: one barrier per tile like the producers' below
        CH_STAMP_BEGIN;
        for (int t = 0; t < ntiles; ++t) {
          if (t > 0 && clane < 15)
            acc = chain_tile<SH::CHAIN_NBUF>(S.prod[(t - 1) & 1][clane], min(TQ, rows - (t - 1) * TQ), acc);
          CH_STAMP(c_add);
          tile_barrier();
          CH_STAMP(c_bar);
        }
        CH_STAMP_END(22);
      } else if (slot >= 0) {
        Row X, Y, Z;
        row_load(X, 0);
        row_load(Y, 1);
        row_gather(X);
        for (int t = 0; t < ntiles; t += 3) {
          row_load(Z, t + 2); row_gather(Y); row_write(X, t);
          PR_STAMP_BARRIER(24, 3);
          if (t + 1 < ntiles) {
            row_load(X, t + 3); row_gather(Z); row_write(Y, t + 1);
            tile_barrier();
          }
          if (t + 2 < ntiles) {
            row_load(Y, t + 4); row_gather(X); row_write(Z, t + 2);
            tile_barrier();
          }
        }
      } else {
        for (int t = 0; t < ntiles; ++t) tile_barrier();   // a wave that neither chains nor produces (1024-thread workgroup)
      }
      __syncthreads();                                     // (the loads still in flight belong to rows past the end)
    } else
    for (int t = 0; t < (FIRST ? 0 : ntiles); ++t) {
      if (slot >= 0) {
        const int i = t * TQ + slot;
        float m[3] = {0.f, 0.f, 0.f}, r[3] = {0.f, 0.f, 0.f};
        bool have_m = false, have_pair = false;
        if (i < rows) {
          if (iter == 1) {                               // :700-704: index pairs, invalid -> 0
            if (i < n_model) {
              have_m = true;
              have_pair = true;
              if (vvalid(mod[3 * i + 2])) { m[0] = mod[3 * i]; m[1] = mod[3 * i + 1]; m[2] = mod[3 * i + 2]; }
            }
            if (vvalid(ref[3 * i + 2])) { r[0] = ref[3 * i]; r[1] = ref[3 * i + 1]; r[2] = ref[3 * i + 2]; }
          } else {
            const int j = nn_get(nn[i]);
            if (j >= 0) {
              have_m = have_pair = true;
              m[0] = mod[3 * i]; m[1] = mod[3 * i + 1]; m[2] = mod[3 * i + 2];
              r[0] = jsrc[3 * j]; r[1] = jsrc[3 * j + 1]; r[2] = jsrc[3 * j + 2];
            }
          }
        }
        if (parity) {
          // dropped pairs contribute an exact +0.0f, so the chains are branch-free
          float (*tile)[SH::TS] = S.prod[t & 1];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) tile[a * 3 + b][slot] = have_pair ? m[a] * r[b] : 0.0f;   // (*it_s) * (*it_ref).t()
#pragma unroll
          for (int q = 0; q < 3; ++q) { tile[9 + q][slot] = have_m ? m[q] : 0.0f; tile[12 + q][slot] = r[q]; }
        } else {
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) ds[a * 3 + b] += (double)m[a] * (double)r[b] * (have_pair ? 1.0 : 0.0);
#pragma unroll
          for (int q = 0; q < 3; ++q) { ds[9 + q] += have_m ? (double)m[q] : 0.0; ds[12 + q] += (double)r[q]; }
        }
      } else if (t > 0 && clane >= 0 && clane < 15) {
        acc = chain_tile<SH::CHAIN_NBUF>(S.prod[(t - 1) & 1][clane], min(TQ, rows - (t - 1) * TQ), acc);
      }
      if (parity) __syncthreads();
    }
    if (parity && ntiles > 0 && clane >= 0 && clane < 15)
      acc = chain_tile<SH::CHAIN_NBUF>(S.prod[(ntiles - 1) & 1][clane], min(TQ, rows - (ntiles - 1) * TQ), acc);
    if (summed && clane >= 0 && clane < 15) acc = S.first_sums[clane];
    kept = block_sum_int(S, kept);
    TSTAMP(3);
    if (iter == 1) SSTAMP(7);
    const int ncm = index_pairs ? n_model : kept, ncr = index_pairs ? n_ref : kept;
    if (threadIdx.x == 0) S.n_corr = ncm;
    if (ncr < 3 || ncm < 3) {                            // :711-715
      __syncthreads();
      if (threadIdx.x == 0) S.iter = it_thr;
      __syncthreads();
      continue;
    }
    if (MODE == FL_ICP_PARITY) {
      if (clane >= 0 && clane < 15) S.sums[clane] = acc;
      __syncthreads();
    } else {
      double dd[NSUM];
#pragma unroll
      for (int k = 0; k < NSUM; ++k) dd[k] = (double)ds[k];
      block_sum_double<NSUM>(S, dd);
    }
    if (threadIdx.x == 0) {
      if (plane) solve_point_to_plane(S);
      else solve_rigid<MODE>(S, ncm, ncr);
    }
    __syncthreads();
    TSTAMP(4);
    if (!S.ok) continue;                                 // :749
    float Ro[9], To[3];
    for (int k = 0; k < 9; ++k) Ro[k] = S.Ropt[k];
    for (int k = 0; k < 3; ++k) To[k] = S.Topt[k];
    old_mean = S.dist_mean;
    __syncthreads();
    mean_ub = l2dist_phase<MODE, SPEC, IDX16>(S, mod, ref, bnd, dterm, n_model, 3 * old_mean, Ro, To, pix, zref, og);   // :756, :778-780
    TSTAMP(5);
    if (SPEC) {                                          // the chain, dist_diff and the pose update follow at the loop head
      pending = 2;
      have_nn = false;
      continue;
    }
    if (threadIdx.x == 0) {
      S.dist_diff = old_mean - S.dist_mean;
      pose_accumulate(S);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    for (int i = 0; i < 9; ++i) res->R[i] = S.R[i];
    for (int i = 0; i < 3; ++i) res->T[i] = S.T[i];
    res->dist_mean = S.dist_mean;
    res->px_ratio = S.px;
    res->iters = S.iter;
    res->n_corr_last = S.n_corr;
#ifdef FL_ICP_PHASES
    // dev build only: phase cycles (grid, -, A1, A2, svd, B, before icp_run, whole kernel) of this workgroup instead of R
    for (int i = 0; i < 6; ++i) res->R[i] = (float)S.tacc[i];
    res->R[6] = (float)S.tacc[6];
    res->R[7] = (float)(clock64() - S.tkernel);
    res->R[8] = (float)S.tacc[8];                       // organised search: steps, candidates, fallbacks
    res->T[0] = (float)S.tacc[9];
    res->T[1] = (float)S.tacc[10];
    res->T[2] = (float)S.tacc[11];
    res->dist_mean = (float)S.tacc[12];
#endif
  }
  __syncthreads();
}

// ---- detection() front half: crop back-projection + paired-valid compaction ----------------------
// Unit surface normal at scene pixel (x, y) for FL_ICP_POINT_TO_PLANE (no reference counterpart): least-squares
// depth gradient (zu, zv) over the (2r+1)^2 window -- on a complete window the fit decouples into
// zu = sum du*z / sum du^2 -- then n = Pu x Pv of the back-projected surface P(u,v) = ((u-cx)/fx*z, (v-cy)/fy*z, z).
// A window that leaves the image, holds a missing return or crosses a depth step (> 2 % + 2 mm of the centre
// depth) gives n = 0: the point still takes part in the NN search but not in the 6x6 system.
#define ICP_NRM_R 3
__device__ __forceinline__ void scene_normal(const uint16_t *__restrict__ scene, int w, int h, int x, int y, float fx, float fy,
                                             float cx, float cy, float *n)
{
  n[0] = n[1] = n[2] = 0.f;
  if (x < ICP_NRM_R || y < ICP_NRM_R || x + ICP_NRM_R >= w || y + ICP_NRM_R >= h) return;
  const float zc = (float)scene[(size_t)y * w + x], gate = 0.02f * zc + 2.0f;
  float su = 0.f, sv = 0.f;
  bool ok = zc > 0.f;
  for (int dv = -ICP_NRM_R; dv <= ICP_NRM_R; ++dv)
    for (int du = -ICP_NRM_R; du <= ICP_NRM_R; ++du) {
      const float z = (float)scene[(size_t)(y + dv) * w + x + du];
      ok = ok && z > 0.f && fabsf(z - zc) <= gate;
      su += (float)du * z;
      sv += (float)dv * z;
    }
  if (!ok) return;
  const float s2 = (float)((2 * ICP_NRM_R + 1) * ICP_NRM_R * (ICP_NRM_R + 1) * (2 * ICP_NRM_R + 1) / 3);   // sum du^2 over the window
  const float zu = su / s2, zv = sv / s2, X = (x - cx) / fx, Y = (y - cy) / fy;
  const float pu[3] = {zc / fx + X * zu, Y * zu, zu}, pv[3] = {X * zv, zc / fy + Y * zv, zv};
  const float c[3] = {pu[1] * pv[2] - pu[2] * pv[1], pu[2] * pv[0] - pu[0] * pv[2], pu[0] * pv[1] - pu[1] * pv[0]};
  const float len = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  if (!(len > 0.f)) return;
  n[0] = c[0] / len; n[1] = c[1] / len; n[2] = c[2] / len;
}

template <class SH>
__device__ __forceinline__ int crop_clouds(SH &S, const IcpArgs &a, const uint16_t *scene, const uint16_t *model, bool model_01mm,
                           const int *rm, const int *rr, float *ref, float *mod, float *nrm, float *rimg, int *idximg, float *zimg,
                           uint16_t *pix, float *zref)
{
  constexpr int BS = SH::BS, NW = SH::NW;
  const int cw = rm[2], ch = rm[3], np = cw * ch;
  const float inv_fx = 1.0f / a.fx, inv_fy = 1.0f / a.fy;                        // depth_to_3d.cpp:103-104
  const float minv_fx = 1.0f / 608.f, minv_fy = 1.0f / 608.f;                   // initInternalMat common.cpp:358
  const float zs = (float)(1 / 1000.0);
  // Row-major compaction of the paired-valid pixels.  Per BS pixels: rank inside the wave by ballot + mbcnt, the
  // wave counts through a double-buffered LDS slot -- ONE barrier per step; every thread keeps the running total itself.
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_cw = 1.0f / (float)cw;                   // p / cw below: exact for p < 2^20, cw <= 2^10 (see div_small)
  int kept_before = 0, step = 0;
  __syncthreads();
  for (int base = 0; base < np; base += BS, ++step) {
    const int p = base + threadIdx.x;
    float A[3] = {0, 0, 0}, B[3] = {0, 0, 0};
    float zsf_keep = NAN;                                   // the scene pixel's depth factor (what org_point rebuilds A from)
    int keep = 0;
    if (p < np) {
      const int y = np < (1 << 20) && cw <= 1024 ? (int)(((float)p + 0.5f) * inv_cw) : p / cw, x = p - y * cw;
      const int sx = rr[0] + x, sy = rr[1] + y, mx = rm[0] + x, my = rm[1] + y;
      const unsigned ds = scene[(size_t)sy * a.w + sx];
      unsigned dm = model[(size_t)my * a.w + mx];
      if (model_01mm) {                                  // convertTo(CV_16UC1, 0.1) obj_reco_lmicp.cpp:188
        int v = __float2int_rn((float)dm * 0.1f);
        dm = (unsigned)(v < 0 ? 0 : (v > 65535 ? 65535 : v));
      }
      const float zsf = ds == 0 ? NAN : (float)ds * zs;                           // rescaleDepth :257-259
      zsf_keep = zsf;
      const float zmf = dm == 0 ? NAN : (float)dm * zs;
      A[0] = ((((float)sx - a.cx) * inv_fx) * zsf) * 1000;                        // :119,:132; scale_mat_vec3f
      A[1] = ((((float)sy - a.cy) * inv_fy) * zsf) * 1000;
      A[2] = zsf * 1000;
      B[0] = ((((float)mx - 320.f) * minv_fx) * zmf) * 1000;
      B[1] = ((((float)my - 240.f) * minv_fy) * zmf) * 1000;
      B[2] = zmf * 1000;
      keep = vvalid(A[2]) && vvalid(B[2]);                                        // matToVec common.cpp:382-405
    }
    const unsigned long long bal = __ballot(keep);
    const int in_wave = __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
    int *slot = S.iscan2[step & 1];
    if (lane == 0) slot[wv] = __popcll(bal);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) { const int c = slot[i]; before += i < wv ? c : 0; total += c; }
    // the reference cloud as an image (organised search): the point or a point at infinity, and its index
    if (p < np) {
      const F3 pt = {keep ? A[0] : INFINITY, keep ? A[1] : INFINITY, keep ? A[2] : INFINITY};
      __builtin_memcpy(rimg + 3 * p, &pt, 12);
      idximg[p] = keep ? kept_before + before + in_wave : NN_IDX_NONE;
      if (zimg) zimg[p] = keep ? zsf_keep : NAN;
    }
    if (keep) {
      const int k = kept_before + before + in_wave;
      ref[3 * k] = A[0]; ref[3 * k + 1] = A[1]; ref[3 * k + 2] = A[2];
      mod[3 * k] = B[0]; mod[3 * k + 1] = B[1]; mod[3 * k + 2] = B[2];
      if (pix) { pix[k] = (uint16_t)p; zref[k] = zsf_keep; }      // 16-bit builds: what l2dist_phase rebuilds ref[k] from
      if (nrm) {
        float nv[3];
        scene_normal(scene, a.w, a.h, rr[0] + p % cw, rr[1] + p / cw, a.fx, a.fy, a.cx, a.cy, nv);
        nrm[3 * k] = nv[0]; nrm[3 * k + 1] = nv[1]; nrm[3 * k + 2] = nv[2];
      }
    }
    kept_before += total;
  }
  if (threadIdx.x < 3 * NN_OVERRUN) rimg[3 * np + threadIdx.x] = INFINITY;     // overrun guard: points at infinity behind the image (org_scan)
  if (zimg && threadIdx.x < NN_OVERRUN + 1) zimg[np + threadIdx.x] = NAN;
  __syncthreads();                                         // the clouds are complete for every thread
  return kept_before;
}

// The model indices in tile order (ICP_TILE_W x 64 / ICP_TILE_W pixels: 16 x 4) (tile rows alternately left-to-right and right-to-left, so consecutive tiles
// are neighbours; inside a tile column by column): the 64 queries a wave takes per step then project into a
// compact window of the reference image.
// Index k of crop pixel p is idximg[p] (the paired compaction keeps the same pixels of both clouds).
template <class SH, class IDX>
__device__ __forceinline__ void build_tile_order(SH &S, const int *idximg, int cw, int ch, int n, IDX *perm)
{
  constexpr int BS = SH::BS, NW = SH::NW;
  int *cnt = (int *)&S.prod[0][0][0];
  constexpr int CAP = (int)(sizeof(S.prod) / 4);
  constexpr int TW = ICP_TILE_W, TH = 64 / ICP_TILE_W;
  static_assert(TW * TH == 64 && (TW & (TW - 1)) == 0, "a tile is one wavefront of pixels");
  const int ntx = (cw + TW - 1) / TW, nty = (ch + TH - 1) / TH, ntile = ntx * nty;
  if (ntile > CAP) {                                       // more tiles than the scratch holds (crops beyond 1.5 Mpixel): index order
    if constexpr (sizeof(IDX) == 2) {
      // (a 32-bit byte offset the compiler cannot turn into a 64-bit pointer walk: that one widened a register pair the kernel
      // spills during set-up to four registers in the 16-bit builds)
      for (unsigned i = threadIdx.x; i < (unsigned)n; i += BS) {
        unsigned o = 2 * i;
        asm volatile("" : "+v"(o));
        *(IDX *)((char *)perm + (size_t)o) = (IDX)i;
      }
    } else {
      for (int i = threadIdx.x; i < n; i += BS) perm[i] = i;
    }
    __syncthreads();
    return;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float inv_ntx = 1.0f / (float)ntx;
  auto tile_index = [&](int t, bool &has) {
    const int ty = (int)(((float)t + 0.5f) * inv_ntx);
    int tx = t - ty * ntx;
    if (ty & 1) tx = ntx - 1 - tx;
    // column by column inside a tile, in the direction the tile row is walked: 64 consecutive entries of perm[] -- a search
    // step -- then always cover ONE contiguous run of columns of the tile row (row by row, a step that starts in the middle of
    // a tile takes its lower rows, the next tile and the upper rows of the one after: up to three tiles wide)
    const int c = lane / TH, x = tx * TW + ((ty & 1) ? TW - 1 - c : c), y = ty * TH + (lane & (TH - 1));
    int k = NN_IDX_NONE;
    if (x < cw && y < ch) k = idximg[y * cw + x];
    has = (unsigned)k < (unsigned)NN_IDX_NONE;
    return k;
  };
  for (int t = wv; t < ntile; t += NW) {
    bool has;
    tile_index(t, has);
    const unsigned long long bal = __ballot(has);
    if (lane == 0) cnt[t] = __popcll(bal);
  }
  __syncthreads();
  SSTAMP(1);
  // exclusive scan of cnt[0 .. ntile) in place: a contiguous chunk per thread, the thread totals scanned by shuffles and
  // one LDS round
  {
    const int per = (ntile + BS - 1) / BS, lo = min((int)threadIdx.x * per, ntile), hi = min(lo + per, ntile);
    int mine = 0;
    for (int t = lo; t < hi; ++t) mine += cnt[t];
    int inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(inc, d, 64);
      if (lane >= d) inc += v;
    }
    if (lane == 63) S.iscan[wv] = inc;
    __syncthreads();
    int before = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) before += w < wv ? S.iscan[w] : 0;
    int ex = before + inc - mine;
    for (int t = lo; t < hi; ++t) { const int c = cnt[t]; cnt[t] = ex; ex += c; }
  }
  __syncthreads();
  for (int t = wv; t < ntile; t += NW) {
    bool has;
    const int k = tile_index(t, has);
    const unsigned long long bal = __ballot(has);
    if (has) perm[cnt[t] + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u))] = (IDX)k;
  }
  __syncthreads();
  SSTAMP(2);
}

#ifdef FL_ICP_PHASES
__device__ unsigned long long g_icp_setup[12];       // SSTAMP slots 0..9, whole-kernel cycles, workgroups: sums over a launch
#endif
// waves per SIMD a kernel instance is compiled for: the 256-thread one shares a CU with up to ICP_MODE_WPE - 1 others,
// a 1024-thread workgroup is 4 waves per SIMD by itself
#define ICP_WPE(MODE, BS) ((BS) == ICP_BS_SMALL ? ICP_MODE_WPE(MODE) : (BS) / 256)

// icpCloudToCloud_Ex on clouds the host staged in the workspace (fl_icp)
template <int MODE, int BS>
__global__ __launch_bounds__(BS) void k_icp_clouds(IcpArgs a)
{
  extern __shared__ __align__(16) uint8_t icp_smem[];
  using SH = IcpSharedT<BS>;
  SH &S = *(SH *)icp_smem;
  const IcpWsLayout L = icp_layout(a.n_max);
  uint8_t *wsb = a.ws + (size_t)blockIdx.x * a.ws_stride;
  const OrgGeom none = {};
  if (threadIdx.x == 0) S.cw = 0;                         // the chain wave (IcpSharedT::cw)
  __syncthreads();
  icp_run<MODE, false, int>(S, wsb, L, a.job.n_ref, a.job.n_model, a.it_thr, a.dmt, a.ddt, &a.results[blockIdx.x].det.icp, none);
}

// WPE: waves per SIMD this instance is compiled for.  The 256-thread parity kernel exists twice, for 4 (128 VGPRs) and for 5
// (96 VGPRs, a few more spills) workgroups per CU: 5 per CU finish a full round of 5 x #CUs frames 4 % faster per frame,
// 4 per CU win when the batch is not a multiple of that (icp_small_wpe).
// IDX: int, or uint16_t for the two 256-thread parity instances the launcher picks when the workspace capacity a.n_max is at most
// 65535 points (icp_idx16): every crop pixel and point index then fits 16 bits, 0xFFFF is free for "none".
template <int MODE, int BS, int WPE = ICP_WPE(MODE, BS), class IDX = int>
__global__ __launch_bounds__(BS) __attribute__((amdgpu_waves_per_eu(WPE, WPE > 4 ? WPE : 4)))
void k_icp_pipeline(IcpArgs a)
{
  extern __shared__ __align__(16) uint8_t icp_smem[];
  using SH = IcpSharedT<BS>;
  SH &S = *(SH *)icp_smem;
#ifdef FL_ICP_PHASES
  if (threadIdx.x == 0) {
    S.tkernel = clock64(); S.wall0 = wall_clock64();
    for (int i = 0; i < 10; ++i) S.tset[i] = 0;
    S.tslast = S.tkernel;
  }
#endif
  constexpr bool FIRST = MODE == FL_ICP_PARITY && BS == ICP_BS_SMALL;   // the 256-thread parity instances fuse their first pass (first_pass)
  const int job = a.order ? a.order[blockIdx.x] : (int)blockIdx.x, rank = a.job.kind == 0 && !a.jobs ? job % a.ranks : 0;
  const int frame = a.job.kind == 0 ? (a.jobs ? a.jobs[job].frame : job / a.ranks) : job;
  const IcpWsLayout L = icp_layout(a.n_max);
  uint8_t *wsb = a.ws + (size_t)job * a.ws_stride;
  float *ref = (float *)(wsb + L.ref), *mod = (float *)(wsb + L.mod);

  fl_recognition_result *res = &a.results[job];
  if (a.job.kind == 0 && a.jobs && frame < 0) return;    // fl_refine_selected: this frame's winner belongs to another rank (uniform per workgroup)
  const uint16_t *scene, *model;
  float r_match[9], t_match[3];
  bool model_01mm;
  if (a.job.kind == 1) {
    if (threadIdx.x == 0) {
      for (int k = 0; k < 4; ++k) { S.rect_m[k] = a.job.rect_model[k]; S.rect_r[k] = a.job.rect_ref[k]; }
      S.status = FL_OK;
      res->status = FL_OK;
      res->found = 1;
    }
    scene = a.job.scene_depth;
    model = a.job.model_depth;
    for (int k = 0; k < 9; ++k) r_match[k] = a.job.r_match[k];
    for (int k = 0; k < 3; ++k) t_match[k] = a.job.t_match[k];
    model_01mm = false;
    __syncthreads();
  } else {
    // CObjRecoLmICP::Recognition after Detector::match (obj_reco_lmicp.cpp:106-152)
    const uint8_t *fws = a.frame_ws + (size_t)frame * a.frame_stride;
    const int *counters = (const int *)(fws + a.off_count);
    const fl_match *matches = (const fl_match *)(fws + a.off_match);
    if (threadIdx.x == 0) {
      S.status = FL_OK;
      S.g = -1;
      res->n_matches = a.jobs ? 1 : counters[1];
      res->found = 0;
      res->status = FL_OK;
      if (!a.jobs && counters[2]) S.status = res->status = FL_ERR_OVERFLOW;
      else if (a.jobs || counters[1] > rank) {
        const fl_match best = a.jobs ? a.jobs[job].match : matches[rank];   // matches[0] :111 (rank > 0: multi-hypothesis extension)
        res->best = best;
        const int g = a.class_first[best.class_idx] + best.template_id;
        const FlPyrInfo pi = a.pyr[g];
        S.g = g;
        S.rect_m[0] = pi.off_x0; S.rect_m[1] = pi.off_y0; S.rect_m[2] = pi.width0; S.rect_m[3] = pi.height0;   // :129
        S.rect_r[0] = best.x; S.rect_r[1] = best.y; S.rect_r[2] = pi.width0; S.rect_r[3] = pi.height0;         // :130-132
        if (!a.depth_ptrs[g]) S.status = res->status = FL_ERR_STATE;      // no depth/<id>.png uploaded
      }
    }
    __syncthreads();
    if (S.g < 0 || S.status != FL_OK) return;            // vtResult stays empty (:106-109)
    const int g = S.g;
    scene = (const uint16_t *)((const uint8_t *)a.scene_base + (size_t)frame * a.scene_stride);
    model = a.depth_ptrs[g];
    const float *p = a.poses + 13 * (size_t)g;           // :141-152
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) r_match[i * 3 + j] = p[i * 4 + j];
      t_match[i] = p[i * 4 + 3];
    }
    model_01mm = true;
  }
  // Q10: a rect leaving the image is a cv::Mat ROI assertion in the reference (detection.cpp:43-44)
  {
    const int *rm = S.rect_m, *rr = S.rect_r;
    const bool bad = rm[0] < 0 || rm[1] < 0 || rm[2] < 0 || rm[3] < 0 || rm[0] + rm[2] > a.w || rm[1] + rm[3] > a.h ||
                     rr[0] < 0 || rr[1] < 0 || rr[2] < 0 || rr[3] < 0 || rr[0] + rr[2] > a.w || rr[1] + rr[3] > a.h ||
                     rm[2] != rr[2] || rm[3] != rr[3] || (long long)rm[2] * rm[3] > a.n_max;
    if (bad) {
      if (threadIdx.x == 0) { res->status = FL_ERR_ASSERT; res->det.status = FL_ERR_ASSERT; res->found = 0; }
      return;
    }
  }
  if (threadIdx.x == 0) S.cw = 0;                         // the chain wave (IcpSharedT::cw)
  __syncthreads();
  float *rimg = (float *)(wsb + L.sref);                  // image of 12-byte points, then the image of their indices (16 bytes per pixel in all)
  SSTAMP(9);
  const int np = crop_clouds(S, a, scene, model, model_01mm, S.rect_m, S.rect_r, ref, mod,
                             MODE == FL_ICP_POINT_TO_PLANE ? (float *)(wsb + L.nrm) : nullptr, rimg,
                             (int *)((uint8_t *)rimg + org_idximg_offset(S.rect_m[2] * S.rect_m[3])),
                             MODE == FL_ICP_PARITY && BS < ICP_BS_WIDE ? (float *)(wsb + L.zimg) : nullptr,
                             sizeof(IDX) == 2 ? (uint16_t *)(wsb + L.dterm) : nullptr, (float *)(wsb + L.nd));
  SSTAMP(0);
  // wave-uniform values read from LDS are VGPRs unless told otherwise: the search loop keeps them in SGPRs
  const OrgGeom og = {__builtin_amdgcn_readfirstlane(S.rect_r[2]), __builtin_amdgcn_readfirstlane(S.rect_r[3]),
                      uniform_f((float)S.rect_r[0] - a.cx), uniform_f((float)S.rect_r[1] - a.cy), a.fx, a.fy,
                      __builtin_amdgcn_readfirstlane(S.rect_r[0]), __builtin_amdgcn_readfirstlane(S.rect_r[1]), a.cx, a.cy,
                      uniform_f(1.0f / a.fx), uniform_f(1.0f / a.fy)};
  build_tile_order(S, (const int *)((const uint8_t *)rimg + org_idximg_offset(og.cw * og.ch)), og.cw, og.ch, np, (IDX *)(wsb + L.perm));
  // getMean x2 (detection.cpp:165-166), t_match_tmp = r - m (:177), t_init (:199)
  float mc[3] = {0, 0, 0}, rc[3] = {0, 0, 0};
  if (MODE == FL_ICP_PARITY) {
    // getMean x2 as six float32 chains in index order, fed like phase A2: the producer waves load TQ rows per tile
    // (coalesced 12-byte loads) into the LDS tiles, lanes 0..5 of wave 0 add the previous tile
    {
      constexpr int TQ = SH::TQ;
      const int slot = S.producer_slot(), clane = S.chain_lane(), ntiles = (np + TQ - 1) / TQ;
      float acc = 0.0f;
      for (int t = 0; t < ntiles; ++t) {
        if (slot >= 0) {
          const int i = t * TQ + slot;
          F3 m3 = {0.f, 0.f, 0.f}, r3 = {0.f, 0.f, 0.f};
          if (i < np) { m3 = ld3_u32(mod, i); r3 = ld3_u32(ref, i); }
          float (*tile)[SH::TS] = S.prod[t & 1];
          tile[0][slot] = m3.x; tile[1][slot] = m3.y; tile[2][slot] = m3.z;
          tile[3][slot] = r3.x; tile[4][slot] = r3.y; tile[5][slot] = r3.z;
        } else if (t > 0 && clane >= 0 && clane < 6) {
          acc = chain_tile<SH::CHAIN_NBUF>(S.prod[(t - 1) & 1][clane], min(TQ, np - (t - 1) * TQ), acc);
        }
        __syncthreads();
      }
      if (ntiles > 0 && clane >= 0 && clane < 6)
        acc = chain_tile<SH::CHAIN_NBUF>(S.prod[(ntiles - 1) & 1][clane], min(TQ, np - (ntiles - 1) * TQ), acc);
      if (clane >= 0 && clane < 6) S.sums[clane] = acc;
    }
    __syncthreads();
    for (int k = 0; k < 3; ++k) { mc[k] = S.sums[k]; rc[k] = S.sums[3 + k]; }
    if (np > 0)
      for (int k = 0; k < 3; ++k) { mc[k] /= (float)np; rc[k] /= (float)np; }
  } else {
    double ds[6] = {0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < np; i += BS)
      for (int k = 0; k < 3; ++k) { ds[k] += mod[3 * i + k]; ds[3 + k] += ref[3 * i + k]; }
    block_sum_double<6>(S, ds);
    if (np > 0)
      for (int k = 0; k < 3; ++k) { mc[k] = (float)(S.dsum[0][k] / np); rc[k] = (float)(S.dsum[0][3 + k] / np); }
  }
  float t_tmp[3], t_init[3];
  for (int k = 0; k < 3; ++k) { t_tmp[k] = rc[k] - mc[k]; t_init[k] = t_tmp[k] + t_match[k]; }
  __syncthreads();
  SSTAMP(3);
  if (!FIRST)                                            // (FIRST: icp_run's first pass applies t_tmp)
    for (int i = threadIdx.x; i < np; i += BS) {         // transformPoints(pts_mod, I, t_match_tmp) :206
      if (!vvalid(mod[3 * i + 2])) continue;
      const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
      float v[3] = {mod[3 * i], mod[3 * i + 1], mod[3 * i + 2]}, o[3];
      mat_vec(I, v, o);
      mod[3 * i] = o[0] + t_tmp[0];
      mod[3 * i + 1] = o[1] + t_tmp[1];
      mod[3 * i + 2] = o[2] + t_tmp[2];
    }
  __syncthreads();
  SSTAMP(4);
  icp_run<MODE, true, IDX, FIRST>(S, wsb, L, np, np, a.it_thr, a.dmt, a.ddt, &res->det.icp, og, FIRST ? t_tmp : nullptr);      // :228
  if (threadIdx.x == 0) {
    const fl_icp_result &ic = res->det.icp;
    float Rt[3];
    mat_vec(ic.R, t_init, Rt);                           // T_final = R*t_init + T, R_final = R*r_match :232-234
    for (int k = 0; k < 3; ++k) res->det.T_final[k] = Rt[k] + ic.T[k];
    mat_mat(ic.R, r_match, res->det.R_final);
    res->det.n_points = np;
    res->det.status = FL_OK;
    for (int i = 0; i < 3; ++i) {                        // Convert() obj_reco_lmicp.cpp:20-30
      for (int j = 0; j < 3; ++j) res->pose[i * 4 + j] = res->det.R_final[i * 3 + j];
      res->pose[i * 4 + 3] = res->det.T_final[i];
    }
    res->pose[12] = res->pose[13] = res->pose[14] = 0.f;
    res->pose[15] = 1.f;
    res->found = 1;
#ifdef FL_ICP_PHASES
    // dev build only: histograms of the organised search instead of the pose
    for (int i = 0; i < 16; ++i) res->pose[i] = (float)S.hist[i];
    for (int i = 0; i < 9; ++i) res->det.R_final[i] = (float)S.hist[16 + i];
    for (int i = 0; i < 3; ++i) res->det.T_final[i] = (float)S.hist[26 + i];
    for (int i = 0; i < 5; ++i) res->pose[11 + i] = (float)S.stime[i];   // the last five union classes (wider than 29 pixels) make room
    // start / end of this workgroup on the 100 MHz wall clock (two 24-bit halves each: a float holds 24 bits), and its CU
    {
      const long long w1 = wall_clock64();
      res->pose[0] = (float)((S.wall0 >> 24) & 0xffffff); res->pose[1] = (float)(S.wall0 & 0xffffff);
      res->pose[2] = (float)((w1 >> 24) & 0xffffff); res->pose[3] = (float)(w1 & 0xffffff);
      unsigned hwid;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
      res->pose[4] = (float)(hwid & 0xffffff);
    }
    for (int i = 0; i < 10; ++i) atomicAdd(&g_icp_setup[i], (unsigned long long)S.tset[i]);
    atomicAdd(&g_icp_setup[10], (unsigned long long)(clock64() - S.tkernel));
    atomicAdd(&g_icp_setup[11], 1ull);
#endif
  }
}

// ------------------------------------------------------------------------------------------
// cup_d2pc::depthTo3d full frame (the stage entry point; the pipeline only back-projects crops)
__global__ __launch_bounds__(256) void k_depth_to_3d(const uint16_t *__restrict__ depth, int w, int h, float fx, float fy,
                                                     float cx, float cy, float *__restrict__ out)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const float inv_fx = 1.0f / fx, inv_fy = 1.0f / fy;
  const unsigned d = depth[(size_t)y * w + x];
  const float z = d == 0 ? NAN : (float)d * (float)(1 / 1000.0);
  float *p = out + ((size_t)y * w + x) * 3;
  p[0] = (((float)x - cx) * inv_fx) * z;
  p[1] = (((float)y - cy) * inv_fy) * z;
  p[2] = z;
}

extern "C" int fl_depth_to_3d(fl_context *ctx, const uint16_t *depth, int w, int h, double fx, double fy, double cx,
                              double cy, float *out, int mem)
{
  if (!ctx || !depth || !out || w <= 0 || h <= 0) return FL_ERR_INVALID;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  const size_t nin = (size_t)w * h * 2, nout = (size_t)w * h * 12;
  const uint16_t *din = depth;
  float *dout = out;
  if (mem == FL_MEM_HOST) {
    void *s = nullptr;
    int rc = fl_scratch(ctx, fl_align(nin, 256) + nout, &s);
    if (rc) return rc;
    FL_HIP(ctx, hipMemcpyAsync(s, depth, nin, hipMemcpyHostToDevice, ctx->stream));
    din = (const uint16_t *)s;
    dout = (float *)((uint8_t *)s + fl_align(nin, 256));
  }
  dim3 grid((w + 63) / 64, (h + 3) / 4);
  hipLaunchKernelGGL(k_depth_to_3d, grid, dim3(256), 0, ctx->stream, din, w, h, (float)fx, (float)fy, (float)cx, (float)cy,
                     dout);
  FL_HIP(ctx, hipGetLastError());
  if (mem == FL_MEM_HOST) {
    FL_HIP(ctx, hipMemcpyAsync(out, dout, nout, hipMemcpyDeviceToHost, ctx->stream));
    FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return FL_OK;
}

// ---- longest job first ------------------------------------------------------------------------------------------------
// A batch of a few thousand frames is two or three rounds of workgroups on the chip's slots, and a frame's refinement takes
// time in proportion to its cloud (13 k - 17 k points on the bench scenes: lifetimes of 6.4 - 10.9 ms in one launch).  The
// hardware deals workgroups to slots as they free up, in blockIdx order, so with jobs in frame order the last ones to start
// are average jobs behind the slowest first-round ones, and a launch of 2048 frames took 20.0 ms for 2 x 8.5 ms of mean
// work per slot (85 % of the slots' time used; profiles/README.md).  Dealt longest first, the long jobs run in the first
// round and the short ones fill in behind them.  k_icp_count estimates a job's size as the number of pixels of its crop
// that are valid in both depth images (what crop_clouds will keep); k_icp_order sorts the jobs by it, descending.
__global__ __launch_bounds__(256) void k_icp_count(IcpArgs a, int *__restrict__ size)
{
  __shared__ int part[4];
  const int job = blockIdx.x;
  const uint8_t *fws = a.frame_ws + (size_t)job * a.frame_stride;
  const int *counters = (const int *)(fws + a.off_count);
  const fl_match *matches = (const fl_match *)(fws + a.off_match);
  int n = 0;
  if (!counters[2] && counters[1] > 0) {
    const fl_match best = matches[0];
    const int g = a.class_first[best.class_idx] + best.template_id;
    const FlPyrInfo pi = a.pyr[g];
    const uint16_t *model = a.depth_ptrs[g];
    const uint16_t *scene = (const uint16_t *)((const uint8_t *)a.scene_base + (size_t)job * a.scene_stride);
    const int cw = pi.width0, ch = pi.height0;
    const bool ok = model && pi.off_x0 >= 0 && pi.off_y0 >= 0 && best.x >= 0 && best.y >= 0 && cw > 0 && ch > 0 && pi.off_x0 + cw <= a.w &&
                    pi.off_y0 + ch <= a.h && best.x + cw <= a.w && best.y + ch <= a.h;
    if (ok)
      for (int y = threadIdx.x >> 6; y < ch; y += 4)
        for (int x = threadIdx.x & 63; x < cw; x += 64) {
          const unsigned ds = scene[(size_t)(best.y + y) * a.w + best.x + x], dm = model[(size_t)(pi.off_y0 + y) * a.w + pi.off_x0 + x];
          n += (ds != 0 && ds <= 900 && dm != 0 && dm <= 9004) ? 1 : 0;      // z <= 900 mm in both (the render is in 0.1 mm): an estimate
        }
  }
#pragma unroll
  for (int sft = 32; sft >= 1; sft >>= 1) n += __shfl_xor(n, sft, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) size[job] = part[0] + part[1] + part[2] + part[3];
}

// order[0 .. n) = the jobs by size, descending (ties by job index): one workgroup, bitonic sort of 64-bit keys in LDS
#define ICP_ORDER_MAX 8192
__global__ __launch_bounds__(1024) void k_icp_order(const int *__restrict__ size, int n, int *__restrict__ order)
{
  extern __shared__ unsigned long long okeys[];
  int m = 1;
  while (m < n) m <<= 1;
  for (int i = threadIdx.x; i < m; i += 1024)
    okeys[i] = i < n ? ((unsigned long long)(unsigned)(0x7fffffff - size[i]) << 32) | (unsigned)i : ~0ull;
  __syncthreads();
  for (int k = 2; k <= m; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < m; i += 1024) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long x = okeys[i], y = okeys[l];
          if (((i & k) == 0) == (x > y)) { okeys[i] = y; okeys[l] = x; }
        }
      }
      __syncthreads();
    }
  for (int i = threadIdx.x; i < n; i += 1024) order[i] = (int)(unsigned)(okeys[i] & 0xffffffffull);
}

#define ICP_WPE_MAX 5
static_assert(sizeof(IcpSharedT<ICP_BS_SMALL>) + 16 <= 160 * 1024 / ICP_WPE_MAX, "IcpSharedT<256> must leave room for 5 workgroups per CU");
static_assert(sizeof(IcpSharedT<ICP_BS_WIDE>) + 16 <= 160 * 1024, "IcpSharedT<1024> must fit the CU's LDS");
template <int BS, typename K>
static int icp_launch_one(fl_context *ctx, K kern, int n_jobs, const IcpArgs &a)
{
  size_t lds = (sizeof(IcpSharedT<BS>) + 15) & ~(size_t)15;
  // option icp_wg_per_cu = 1 .. 3: no more than that many 256-thread workgroups per CU (the launch asks for so much LDS that
  // one more does not fit) -- leaves registers and LDS to the kernels of ANOTHER stream (a second pipeline's LINEMOD stages)
  const long cap = ctx->opt.icp_wg_per_cu;
  if (BS == ICP_BS_SMALL && cap >= 1 && cap <= 3) {
    const size_t want = ((size_t)(160 * 1024) / (size_t)cap - 256) & ~(size_t)15;
    if (want > lds) lds = want;
  }
  // The attribute is set per kernel and device, not per launch: at the first launch, and again whenever a launch needs more
  // than it was set to (icp_wg_per_cu changed after that kernel's first launch: cap 1 asks for about 160 KB).
  {
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> attr_set;
    std::lock_guard<std::mutex> lock(mu);
    size_t &cur = attr_set[{(const void *)kern, ctx->device}];
    if (cur < lds) {
      size_t attr = lds > (size_t)(82 * 1024) ? lds : (size_t)(82 * 1024);
      if (attr > (size_t)(160 * 1024)) attr = (size_t)(160 * 1024);
      FL_HIP(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attr));
      cur = attr;
    }
  }
  hipLaunchKernelGGL(kern, dim3(n_jobs), dim3(BS), lds, ctx->stream, a);
  FL_HIP(ctx, hipGetLastError());
#ifdef FL_ICP_PHASES
  {
    // dev build only (it waits for the stream: not for timing): the set-up passes' cycles per workgroup of this launch
    unsigned long long h[12], zero[12] = {};
    FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    FL_HIP(ctx, hipMemcpyFromSymbol(h, HIP_SYMBOL(g_icp_setup), sizeof(h)));
    FL_HIP(ctx, hipMemcpyToSymbol(HIP_SYMBOL(g_icp_setup), zero, sizeof(zero)));
    if (h[11]) {
      const double w = (double)h[11];
      fprintf(stderr, "icp set-up cycles per workgroup (%llu workgroups, life %.0f): crop %.0f, tile counts %.0f, tile placing %.0f, getMean %.0f, "
              "pre-translation %.0f, copyPoints %.0f, initial distances / first pass %.0f, iteration 1 sums %.0f, between %.0f\n", h[11], h[10] / w,
              h[0] / w, h[1] / w, h[2] / w, h[3] / w, h[4] / w, h[5] / w, h[6] / w, h[7] / w, h[9] / w);
    }
  }
#endif
  return FL_OK;
}
// Workgroup width by batch size: with no more jobs than CUs every job runs alone on its CU whatever its width, so it
// gets the 1024-thread kernel; two rounds of it still beat two 256-thread workgroups per CU (measured, ICP ms per launch,
// 1024- vs 256-thread: 256 jobs 3.6 / 6.8, 384: 6.4 / 7.2, 512: 6.8 / 7.7, 768: 10.0 / 8.9, 1024: 13.2 / 11.1).
// option icp_wide = 0 / 1 forces one or the other (fl_context_set_option)
static bool icp_wide(fl_context *ctx, int n_jobs)
{
  if (ctx->opt.icp_wide == 0) return false;
  if (ctx->opt.icp_wide == 1) return true;
  return n_jobs <= 2 * ctx->cus;
}
// Workgroups per CU of the 256-thread parity kernel: whichever of 4 and 5 needs fewer rounds by the measured cost of a full
// round (5 per CU: about 1.25 x the time of 4 per CU for 1.25 x the frames -- the 96-VGPR build spills more; round 3, jobs
// dealt longest first, ICP ms per launch at 4 / 5 per CU: 2560 frames 24.9 / 24.0, 3840: 33.4 / 33.2, 4096: 35.0 / 36.5,
// 5120: 46.7 / 47.7, 6144: 56.0 / 58.5).  Option icp_occ = 4 / 5 forces one (fl_context_set_option).
static int icp_small_wpe(fl_context *ctx, int n_jobs)
{
  if (ctx->opt.icp_occ == 4 || ctx->opt.icp_occ == 5) return (int)ctx->opt.icp_occ;
  const int cus = ctx->cus;
  const int r4 = (n_jobs + 4 * cus - 1) / (4 * cus), r5 = (n_jobs + 5 * cus - 1) / (5 * cus);
  return 1.25 * r5 < 1.0 * r4 ? 5 : 4;
}
// 16-bit pixel and order indices in the 256-thread parity kernel: chosen per launch by the workspace capacity (no crop of the
// launch has more pixels: the kernel refuses one that does), so that 0xFFFF names no pixel.  Option icp_idx16 = 0 keeps the
// 32-bit build; 1 asks for what the default does, and beyond 65535 points still gets the 32-bit build.
static bool icp_idx16(fl_context *ctx, const IcpArgs &a)
{
  return ctx->opt.icp_idx16 != 0 && a.n_max <= 65535;
}
template <int MODE>
static int icp_launch_mode(fl_context *ctx, int n_jobs, const IcpArgs &a)
{
  const bool wide = icp_wide(ctx, n_jobs);
  if constexpr (MODE == FL_ICP_PARITY) {              // the 5-per-CU and the 16-bit builds exist for the parity kernel only
    if (a.job.kind != 2 && !wide) {
      const bool five = icp_small_wpe(ctx, n_jobs) == 5;
      if (icp_idx16(ctx, a))
        return five ? icp_launch_one<ICP_BS_SMALL>(ctx, k_icp_pipeline<MODE, ICP_BS_SMALL, 5, uint16_t>, n_jobs, a)
                    : icp_launch_one<ICP_BS_SMALL>(ctx, k_icp_pipeline<MODE, ICP_BS_SMALL, ICP_PARITY_WPE, uint16_t>, n_jobs, a);
      if (five) return icp_launch_one<ICP_BS_SMALL>(ctx, k_icp_pipeline<MODE, ICP_BS_SMALL, 5>, n_jobs, a);
    }
  }
  if (a.job.kind == 2)
    return wide ? icp_launch_one<ICP_BS_WIDE>(ctx, k_icp_clouds<MODE, ICP_BS_WIDE>, n_jobs, a)
                : icp_launch_one<ICP_BS_SMALL>(ctx, k_icp_clouds<MODE, ICP_BS_SMALL>, n_jobs, a);
  return wide ? icp_launch_one<ICP_BS_WIDE>(ctx, k_icp_pipeline<MODE, ICP_BS_WIDE>, n_jobs, a)
              : icp_launch_one<ICP_BS_SMALL>(ctx, k_icp_pipeline<MODE, ICP_BS_SMALL>, n_jobs, a);
}
static int icp_launch(fl_context *ctx, int n_jobs, const IcpArgs &a)
{
  switch (a.mode) {
    case FL_ICP_PARITY: return icp_launch_mode<FL_ICP_PARITY>(ctx, n_jobs, a);
    case FL_ICP_FAST: return icp_launch_mode<FL_ICP_FAST>(ctx, n_jobs, a);
    case FL_ICP_POINT_TO_PLANE: return icp_launch_mode<FL_ICP_POINT_TO_PLANE>(ctx, n_jobs, a);
    default: return fl_set_error(ctx, FL_ERR_INVALID, "unknown fl_icp_mode");
  }
}

// the fields every ICP launch sets; all others zero
static IcpArgs icp_args(uint8_t *ws, int n_max, int it_thr, float dmt, float ddt, int mode)
{
  IcpArgs a;
  memset(&a, 0, sizeof(a));
  a.ws = ws;
  a.n_max = n_max;
  a.it_thr = it_thr;
  a.dmt = dmt;
  a.ddt = ddt;
  a.mode = mode;
  return a;
}
// the scene's frame size and intrinsics (kinds 0, 1)
static void icp_set_camera(IcpArgs &a, int w, int h, const fl_intrinsics *K)
{
  a.w = w; a.h = h;
  a.fx = (float)K->fx; a.fy = (float)K->fy; a.cx = (float)K->cx; a.cy = (float)K->cy;
}

// one job (kinds 1, 2) with its result slot at a.results: launch it and read the result back
static int icp_run_one(fl_context *ctx, const IcpArgs &a, fl_recognition_result *out)
{
  int rc = icp_launch(ctx, 1, a);
  if (rc) return rc;
  fl_recognition_result *h = nullptr;
  if ((rc = fl_pinned(ctx, sizeof(*h), (void **)&h))) return rc;
  FL_HIP(ctx, hipMemcpyAsync(h, a.results, sizeof(*h), hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *out = *h;
  return FL_OK;
}

static int icp_clouds(fl_context *ctx, const float *ref, const float *ref_normals, int n_ref, const float *model, int n_model,
                      int icp_it_thr, float dist_mean_thr, float dist_diff_thr, int icp_mode, int mem, fl_icp_result *res)
{
  if (!ctx || !res || n_ref < 0 || n_model < 0 || (n_ref && !ref) || (n_model && !model)) return FL_ERR_INVALID;
  if (icp_mode == FL_ICP_POINT_TO_PLANE && n_ref && !ref_normals)
    return fl_set_error(ctx, FL_ERR_INVALID, "FL_ICP_POINT_TO_PLANE needs reference normals: use fl_icp_point_to_plane or fl_detection");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  const int n_max = n_ref > n_model ? n_ref : n_model;
  const IcpWsLayout L = icp_layout(n_max);
  void *s = nullptr;
  int rc = fl_scratch(ctx, L.total + 4096, &s);
  if (rc) return rc;
  uint8_t *wsb = (uint8_t *)s;
  const hipMemcpyKind kind = mem == FL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (n_ref) FL_HIP(ctx, hipMemcpyAsync(wsb + L.ref, ref, 12 * (size_t)n_ref, kind, ctx->stream));
  if (n_model) FL_HIP(ctx, hipMemcpyAsync(wsb + L.mod, model, 12 * (size_t)n_model, kind, ctx->stream));
  if (n_ref && ref_normals) FL_HIP(ctx, hipMemcpyAsync(wsb + L.nrm, ref_normals, 12 * (size_t)n_ref, kind, ctx->stream));
  IcpArgs a = icp_args(wsb, n_max, icp_it_thr, dist_mean_thr, dist_diff_thr, icp_mode);
  a.job.kind = 2;
  a.job.n_ref = n_ref;
  a.job.n_model = n_model;
  a.results = (fl_recognition_result *)(wsb + L.total);
  fl_recognition_result r;
  if ((rc = icp_run_one(ctx, a, &r))) return rc;
  *res = r.det.icp;
  return FL_OK;
}

extern "C" int fl_icp(fl_context *ctx, const float *ref, int n_ref, const float *model, int n_model, int icp_it_thr,
                      float dist_mean_thr, float dist_diff_thr, int icp_mode, int mem, fl_icp_result *res)
{
  return icp_clouds(ctx, ref, nullptr, n_ref, model, n_model, icp_it_thr, dist_mean_thr, dist_diff_thr, icp_mode, mem, res);
}

extern "C" int fl_icp_point_to_plane(fl_context *ctx, const float *ref, const float *ref_normals, int n_ref, const float *model,
                                     int n_model, int icp_it_thr, float dist_mean_thr, float dist_diff_thr, int mem,
                                     fl_icp_result *res)
{
  return icp_clouds(ctx, ref, ref_normals, n_ref, model, n_model, icp_it_thr, dist_mean_thr, dist_diff_thr,
                    FL_ICP_POINT_TO_PLANE, mem, res);
}

extern "C" int fl_detection(fl_context *ctx, const uint16_t *model_depth, const uint16_t *scene_depth, int w, int h,
                            const fl_intrinsics *K, const int rect_model[4], const int rect_ref[4], int icp_it_thr,
                            float dist_mean_thr, float dist_diff_thr, const float r_match[9], const float t_match[3],
                            int icp_mode, int mem, fl_detection_result *res)
{
  if (!ctx || !model_depth || !scene_depth || !K || !rect_model || !rect_ref || !r_match || !t_match || !res || w <= 0 ||
      h <= 0)
    return FL_ERR_INVALID;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  long long area = (long long)rect_model[2] * rect_model[3];
  if (area < 0 || area > (long long)w * h) area = 0;     // the kernel reports FL_ERR_ASSERT for bad rects
  const int n_max = (int)(area > 0 ? area : 1);
  const IcpWsLayout L = icp_layout(n_max);
  const size_t img = fl_align((size_t)w * h * 2, 256);
  void *s = nullptr;
  int rc = fl_scratch(ctx, L.total + 4096 + 2 * img, &s);
  if (rc) return rc;
  uint8_t *wsb = (uint8_t *)s;
  fl_recognition_result *dres = (fl_recognition_result *)(wsb + L.total);
  const uint16_t *dm = model_depth, *dsn = scene_depth;
  if (mem == FL_MEM_HOST) {
    uint8_t *b = wsb + L.total + 4096;
    FL_HIP(ctx, hipMemcpyAsync(b, model_depth, (size_t)w * h * 2, hipMemcpyHostToDevice, ctx->stream));
    FL_HIP(ctx, hipMemcpyAsync(b + img, scene_depth, (size_t)w * h * 2, hipMemcpyHostToDevice, ctx->stream));
    dm = (const uint16_t *)b;
    dsn = (const uint16_t *)(b + img);
  }
  FL_HIP(ctx, hipMemsetAsync(dres, 0, sizeof(*dres), ctx->stream));
  IcpArgs a = icp_args(wsb, n_max, icp_it_thr, dist_mean_thr, dist_diff_thr, icp_mode);
  icp_set_camera(a, w, h, K);
  a.job.kind = 1;
  for (int k = 0; k < 4; ++k) { a.job.rect_model[k] = rect_model[k]; a.job.rect_ref[k] = rect_ref[k]; }
  for (int k = 0; k < 9; ++k) a.job.r_match[k] = r_match[k];
  for (int k = 0; k < 3; ++k) a.job.t_match[k] = t_match[k];
  a.job.model_depth = dm;
  a.job.scene_depth = dsn;
  a.results = dres;
  fl_recognition_result r;
  if ((rc = icp_run_one(ctx, a, &r))) return rc;
  *res = r.det;
  if (r.status == FL_ERR_ASSERT) {
    res->status = FL_ERR_ASSERT;
    return fl_set_error(ctx, FL_ERR_ASSERT, "crop rectangle leaves the image (cv::Mat ROI assert, detection.cpp:43-44)");
  }
  return FL_OK;
}

// once per detector (fl_detector_finalize): the job-order buffer and k_icp_order's LDS size, so that no launch path allocates
// (an implicit device synchronisation) or sets function attributes
int fl_icp_prepare(fl_detector *det)
{
  fl_context *ctx = det->ctx;
  if (det->max_batch > 4 * ctx->cus && !det->d_icp_order)      // (used for batches of up to ICP_ORDER_MAX frames)
    FL_HIP(ctx, hipMalloc((void **)&det->d_icp_order, sizeof(int) * 2 * (size_t)det->max_batch));
  FL_HIP(ctx, hipFuncSetAttribute((const void *)k_icp_order, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(unsigned long long) * ICP_ORDER_MAX)));
  return FL_OK;
}

// Recognition refinement on the detector's frames (depth of frame i at depth + i * depth_stride bytes): n_jobs workgroups,
// job b with the ICP workspace ws + b * ws_stride and result slot b.  Job b refines match (b % ranks) of frame (b / ranks) -- the
// first `ranks` matches of each frame (multi-hypothesis) -- or, with d_jobs, the caller-chosen match d_jobs[b] (template-sharded
// recognition: the rank that owns the winning template refines it).  longest_first: a batch with more jobs than the chip has
// slots is dealt longest first (see k_icp_order; option icp_order = 0 keeps the frame order).
int fl_launch_detection(fl_detector *det, int n_jobs, const fl_intrinsics *K, const fl_recognition_params *p, const uint16_t *depth,
                        size_t depth_stride, uint8_t *ws, size_t ws_stride, int ranks, const FlRefineJob *d_jobs,
                        fl_recognition_result *d_results, bool longest_first)
{
  const FlDetectionTables t = {det->w0, det->h0, det->n_pts_max, det->d_ws, det->ws_stride, det->off_count, det->off_match, det->d_pyr,
                               det->d_class_first, det->d_poses, det->d_depth_ptrs, det->d_icp_order, det->max_batch};
  return fl_launch_detection_tables(det->ctx, t, n_jobs, K, p, depth, depth_stride, ws, ws_stride, ranks, d_jobs, d_results, longest_first);
}

// The same launch on tables the caller names (a detector's, above, or a tracker's: fl_track.hip).
int fl_launch_detection_tables(fl_context *ctx, const FlDetectionTables &t, int n_jobs, const fl_intrinsics *K, const fl_recognition_params *p,
                               const uint16_t *depth, size_t depth_stride, uint8_t *ws, size_t ws_stride, int ranks, const FlRefineJob *d_jobs,
                               fl_recognition_result *d_results, bool longest_first)
{
  IcpArgs a = icp_args(ws, t.n_pts_max, p->icp_it_thr, p->dist_mean_thr, p->dist_diff_thr, p->icp_mode);
  a.ws_stride = ws_stride;
  icp_set_camera(a, t.w, t.h, K);
  a.job.kind = 0;
  a.frame_ws = t.frame_ws;
  a.frame_stride = t.frame_stride;
  a.ranks = ranks;
  a.scene_base = depth;
  a.scene_stride = depth_stride;
  a.off_count = t.off_count;
  a.off_match = t.off_match;
  a.pyr = t.pyr;
  a.class_first = t.class_first;
  a.poses = t.poses;
  a.depth_ptrs = t.depth_ptrs;
  a.results = d_results;
  a.jobs = d_jobs;
  if (longest_first && n_jobs > 4 * ctx->cus && n_jobs <= ICP_ORDER_MAX && t.icp_order && ctx->opt.icp_order != 0) {
    int *d_size = t.icp_order + t.order_cap;
    hipLaunchKernelGGL(k_icp_count, dim3(n_jobs), dim3(256), 0, ctx->stream, a, d_size);
    int m = 1;
    while (m < n_jobs) m <<= 1;
    hipLaunchKernelGGL(k_icp_order, dim3(1), dim3(1024), sizeof(unsigned long long) * (size_t)m, ctx->stream, (const int *)d_size, n_jobs,
                       t.icp_order);
    FL_HIP(ctx, hipGetLastError());
    a.order = t.icp_order;
  }
  return icp_launch(ctx, n_jobs, a);
}

// ---- dev / test entries ----
extern "C" unsigned fl_dev_bnd_pack(unsigned bits) { return bnd_pack(bits); }      // for tests/test_abi_cpu.py (host arithmetic, no GPU)
// dev / tests: both reductions on one wavefront of inputs (tests/test_gpu_icp.py checks them against each other and numpy)
__global__ void k_dev_wave_max6(const int *in, int *out)
{
  int a[6], b[6];
  for (int k = 0; k < 6; ++k) a[k] = b[k] = in[k * 64 + threadIdx.x];
  wave_max6(a);
  wave_max_multi(b);
  if (threadIdx.x == 0)
    for (int k = 0; k < 6; ++k) { out[k] = a[k]; out[6 + k] = b[k]; }
}

// host entry for the test: 6 x 64 ints in, 6 (wave_max6) + 6 (wave_max_multi) out; plain HIP calls on the null stream
extern "C" int fl_dev_wave_max6(const int *in_host, int *out_host)
{
  int *d_in = nullptr, *d_out = nullptr;
  if (hipMalloc(&d_in, 6 * 64 * sizeof(int)) != hipSuccess || hipMalloc(&d_out, 12 * sizeof(int)) != hipSuccess) { (void)hipFree(d_in); return FL_ERR_HIP; }
  bool ok = hipMemcpy(d_in, in_host, 6 * 64 * sizeof(int), hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_dev_wave_max6, dim3(1), dim3(64), 0, 0, d_in, d_out);
    ok = hipGetLastError() == hipSuccess && hipMemcpy(out_host, d_out, 12 * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess;
  }
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  return ok ? FL_OK : FL_ERR_HIP;
}

// dev / tests: scene_normal at n pixels (xy[2 k], xy[2 k + 1]) of a w x h depth image (tests/test_gpu_icp.py checks it against
// the fp64 restatement in tests/p2plane_model.py)
__global__ void k_dev_scene_normals(const uint16_t *depth, int w, int h, float fx, float fy, float cx, float cy, const int *xy, int n,
                                    float *out)
{
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  float nv[3];
  scene_normal(depth, w, h, xy[2 * k], xy[2 * k + 1], fx, fy, cx, cy, nv);
  out[3 * k] = nv[0]; out[3 * k + 1] = nv[1]; out[3 * k + 2] = nv[2];
}

// host entry for the test: pixels outside the image are refused (scene_normal's window test assumes 0 <= x < w, 0 <= y < h);
// plain HIP calls on the null stream.  The image is followed by one spare row of zeros, so that a window rule that is off by
// one reads a zero inside the allocation and the test reports a wrong normal.
extern "C" int fl_dev_scene_normals(const uint16_t *depth_host, int w, int h, float fx, float fy, float cx, float cy, const int *xy_host,
                                    int n, float *out_host)
{
  if (w <= 0 || h <= 0 || n <= 0 || (long long)w * (h + 1) > (1ll << 28)) return FL_ERR_INVALID;
  for (int k = 0; k < n; ++k)
    if (xy_host[2 * k] < 0 || xy_host[2 * k] >= w || xy_host[2 * k + 1] < 0 || xy_host[2 * k + 1] >= h) return FL_ERR_INVALID;
  const size_t img = sizeof(uint16_t) * (size_t)w * h, pad = sizeof(uint16_t) * (size_t)w;
  uint16_t *d_depth = nullptr;
  int *d_xy = nullptr;
  float *d_out = nullptr;
  bool ok = hipMalloc(&d_depth, img + pad) == hipSuccess && hipMalloc(&d_xy, 2 * sizeof(int) * (size_t)n) == hipSuccess &&
            hipMalloc(&d_out, 3 * sizeof(float) * (size_t)n) == hipSuccess;
  ok = ok && hipMemcpy(d_depth, depth_host, img, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemset((uint8_t *)d_depth + img, 0, pad) == hipSuccess &&
       hipMemcpy(d_xy, xy_host, 2 * sizeof(int) * (size_t)n, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_dev_scene_normals, dim3((n + 255) / 256), dim3(256), 0, 0, d_depth, w, h, fx, fy, cx, cy, d_xy, n, d_out);
    ok = hipGetLastError() == hipSuccess && hipMemcpy(out_host, d_out, 3 * sizeof(float) * (size_t)n, hipMemcpyDeviceToHost) == hipSuccess;
  }
  (void)hipFree(d_depth);
  (void)hipFree(d_xy);
  (void)hipFree(d_out);
  return ok ? FL_OK : FL_ERR_HIP;
}
