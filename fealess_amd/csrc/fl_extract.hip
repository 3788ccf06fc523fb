// fl_extract.hip -- template extraction on the GPU:
//   Detector::addTemplate (linemod/linemod.cpp:1579-1615) for the two default modalities,
//   ColorGradientPyramid::extractTemplate (:461-513), DepthNormalPyramid::extractTemplate (:747-825),
//   QuantizedPyramid::selectScatteredFeatures (:135-164), cropTemplates (:52-96), pyrDown (:434-453, :721-739).
//
// Offline path, batched over training views: fl_extract_template_batch runs every stage once per chunk of up to
// FL_EXTRACT_CHUNK_VIEWS views, with a grid dimension over the views or over the chunk's (view, level, modality) jobs;
// fl_extract_template_pyramid is its n_views = 1 case.  What matters is that the selected features equal the
// reference's bit for bit (oracle/extract_oracle.c):
//   k_local_mask         border mask (mask - erode3x3(mask)) / 5x5-eroded mask, for the views that have a mask
//   k_color_candidates   strong-gradient test, 64-bit sort keys appended to the job's key segment
//   k_depth_candidates   exact chessboard distance to the nearest pixel of another label
//                        (= cv::distanceTransform(DIST_C, 3) of the per-label images), per-label counts
//   k_depth_keys         score / label_count -> sort keys
//   k_pad_keys, k_bitonic_step/_local  bitonic sort of each job's keys as its own segment of next_pow2(candidates) keys
//                        (2048-key blocks in LDS, the wider steps in global memory): (score desc, raster order asc) is
//                        exactly what std::stable_sort with Candidate::operator< yields, whatever order the atomics
//                        appended the candidates in
//   k_select_scattered   the greedy selection, one 1024-thread workgroup per job and all jobs in one launch; sequential
//                        in its result but not in its work: every candidate keeps its squared distance to the nearest
//                        chosen feature, the walk to the next passing candidate is a workgroup-wide min
// A chunk makes two host round trips whatever its size: the candidate counts (they size the sort) and the results.
// Two test entries outside the ABI (fl_internal.h) run parts of this on a caller's data through the same launch functions:
// fl_dev_extract_select (the sort and the selection on candidate lists) and fl_dev_extract_quantized (the candidate kernels,
// the sort and the selection of one level on quantized images).
#include "fl_internal.h"
#include <limits.h>
#include <string.h>
#include <algorithm>
#include <vector>

namespace {

struct ExtractCounters {
  int n_cand;            // number of candidates
  int label_counts[8];   // depth modality
  int area;              // countNonZero(local_mask)
  int n_out;             // features written (= num_features on success); -1: too few candidates
};

// One (view, level, modality) of a chunk, written on the host once the candidate counts are known.
struct ExtractJob {
  unsigned long long *keys;    // the job's key segment (n_pow2 keys once padded)
  const uint8_t *labels;       // quantised image of the job's level and modality (the features' labels)
  uint32_t *xy;                // selection scratch, n_cand entries each
  int *mind2;
  ExtractCounters *cnt;
  fl_feature *out;             // 64 entries
  int w, num_features, depth_mode, total_px;
  int n_pow2;                  // sort segment length; 0: the view cannot yield a template, nothing to sort or select
  int pad;
};

__device__ __forceinline__ int ex_label(int q)           // getLabel (linemod.cpp:15-30); -1 where the reference throws
{
  return (q != 0 && (q & (q - 1)) == 0 && q < 256) ? (31 - __clz(q)) : -1;
}

// A candidate's sort key: descending score, then raster order (positive floats order like their bit patterns).  The one
// expression behind k_color_candidates, k_depth_keys and fl_dev_extract_select.
__host__ __device__ __forceinline__ unsigned long long ex_pack_key(float score, int raster)
{
  return ((unsigned long long)(~__builtin_bit_cast(unsigned, score)) << 32) | (unsigned)raster;
}

__device__ __forceinline__ int ex_min_rect(const uint8_t *m, int w, int h, int x, int y, int r)   // cv::erode, BORDER_REPLICATE
{
  int v = 255;
  for (int dy = -r; dy <= r; ++dy) {
    const int yy = min(max(y + dy, 0), h - 1);
    for (int dx = -r; dx <= r; ++dx) v = min(v, (int)m[(size_t)yy * w + min(max(x + dx, 0), w - 1)]);
  }
  return v;
}

// The per-view kernels below find view z = blockIdx.z at base + z * vs (vs: bytes per view) and its counters at
// cnt + z * cnt_stride.  has_mask[z] = 0: the view has no mask (the reference's empty cv::Mat).

// local_mask of the two extractTemplate()s: iterations = 1 -> border of the mask (mask - erode(mask), :467-468),
// iterations = 2 -> the mask eroded by a 5x5 rectangle (:752-755)
__global__ __launch_bounds__(256) void k_local_mask(const uint8_t *__restrict__ mask_, uint8_t *__restrict__ local_, size_t vs,
                                                    const int *__restrict__ has_mask, int w, int h, int iterations, int border)
{
  const int z = blockIdx.z;
  if (!has_mask[z]) return;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const uint8_t *mask = mask_ + (size_t)z * vs;
  const size_t i = (size_t)y * w + x;
  const int e = ex_min_rect(mask, w, h, x, y, iterations);
  const int m = mask[i];
  local_[(size_t)z * vs + i] = (uint8_t)(border ? (m > e ? m - e : 0) : e);
}

// quantized / mag: the views' images at a pitch of w * h elements
__global__ __launch_bounds__(256) void k_color_candidates(const uint8_t *__restrict__ quantized, const float *__restrict__ mag,
                                                          const uint8_t *__restrict__ local, size_t vs, const int *__restrict__ has_mask,
                                                          int w, int h, float thr_sq, uint8_t *__restrict__ keys_,
                                                          ExtractCounters *cnt_, int cnt_stride)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const int z = blockIdx.z;
  const size_t i = (size_t)y * w + x, vo = (size_t)z * vs, io = (size_t)z * w * h + i;
  if (has_mask[z] && !local[vo + i]) return;               // the precomputed local_mask
  const int q = quantized[io];
  const float score = mag[io];
  if (q > 0 && score > thr_sq) {
    const int pos = atomicAdd(&cnt_[(size_t)z * cnt_stride].n_cand, 1);
    ((unsigned long long *)(keys_ + vo))[pos] = ex_pack_key(score, (int)i);
  }
}

// exact L-infinity distance from (x, y) to the nearest pixel whose per-label image is zero, i.e. a pixel outside
// the eroded mask or whose normal does not carry `bit`; 8192 when there is none (OpenCV's capped INIT_DIST0)
__device__ float ex_chessboard(const uint8_t *normal, const uint8_t *mask, int w, int h, int x, int y, int bit)
{
  const int rmax = max(max(x, w - 1 - x), max(y, h - 1 - y));
  for (int r = 1; r <= rmax; ++r) {
    bool zero = false;
    for (int k = -r; k <= r && !zero; ++k) {
      // the four sides of the ring at radius r
      const int xs[4] = {x + k, x + k, x - r, x + r}, ys[4] = {y - r, y + r, y + k, y + k};
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) {
        const int xx = xs[s4], yy = ys[s4];
        if (xx < 0 || yy < 0 || xx >= w || yy >= h) continue;          // outside the image: not a source
        const size_t j = (size_t)yy * w + xx;
        if ((mask && !mask[j]) || !(normal[j] & bit)) zero = true;
      }
    }
    if (zero) return (float)r;
  }
  return 8192.0f;
}

__global__ __launch_bounds__(256) void k_depth_candidates(const uint8_t *__restrict__ normal_, const uint8_t *__restrict__ local_,
                                                          size_t vs, const int *__restrict__ has_mask, int w, int h,
                                                          int extract_threshold, uint8_t *__restrict__ raster_,
                                                          uint8_t *__restrict__ score_, ExtractCounters *cnt_, int cnt_stride)
{
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= w || y >= h) return;
  const int z = blockIdx.z;
  const size_t i = (size_t)y * w + x, vo = (size_t)z * vs;
  const uint8_t *normal = normal_ + vo;
  const uint8_t *mask = has_mask[z] ? local_ + vo : nullptr;   // the precomputed local_mask (5x5-eroded)
  ExtractCounters *cnt = cnt_ + (size_t)z * cnt_stride;
  const bool in_mask = !mask || mask[i] != 0;
  if (mask && in_mask) atomicAdd(&cnt->area, 1);
  if (!in_mask) return;
  const int q = normal[i];
  if (q == 0 || q == 255) return;                          // background and shadow (:782)
  const int label = ex_label(q);
  if (label < 0) return;
  const float d = ex_chessboard(normal, mask, w, h, x, y, 1 << label);
  if (d >= (float)extract_threshold) {
    const int pos = atomicAdd(&cnt->n_cand, 1);
    ((int *)(raster_ + vo))[pos] = (int)i;
    ((float *)(score_ + vo))[pos] = d;
    atomicAdd(&cnt->label_counts[label], 1);
  }
}

// grid-stride over the view's candidates: their count is only known on the device here
__global__ __launch_bounds__(256) void k_depth_keys(const uint8_t *__restrict__ normal_, const uint8_t *__restrict__ raster_,
                                                    const uint8_t *__restrict__ score_, size_t vs, const ExtractCounters *cnt_,
                                                    int cnt_stride, uint8_t *__restrict__ keys_)
{
  const int z = blockIdx.z;
  const size_t vo = (size_t)z * vs;
  const ExtractCounters *cnt = cnt_ + (size_t)z * cnt_stride;
  const uint8_t *normal = normal_ + vo;
  const int *raster = (const int *)(raster_ + vo);
  const float *score = (const float *)(score_ + vo);
  unsigned long long *keys = (unsigned long long *)(keys_ + vo);
  const int n = cnt->n_cand;
  for (int k = blockIdx.x * 256 + threadIdx.x; k < n; k += gridDim.x * 256) {
    const int i = raster[k];
    const float s = score[k] / (float)cnt->label_counts[ex_label(normal[i])];   // :806-810
    keys[k] = ex_pack_key(s, i);
  }
}

// The sort kernels take blockIdx.y = job; a job's segment is keys[0 .. n_pow2).
__global__ __launch_bounds__(256) void k_pad_keys(const ExtractJob *__restrict__ jobs)
{
  const ExtractJob &jb = jobs[blockIdx.y];
  const int n = jb.cnt->n_cand, np2 = jb.n_pow2;
  for (int k = n + blockIdx.x * 256 + threadIdx.x; k < np2; k += gridDim.x * 256) jb.keys[k] = ~0ull;
}

__global__ __launch_bounds__(256) void k_bitonic_step(const ExtractJob *__restrict__ jobs, int kk, int j)
{
  const ExtractJob &jb = jobs[blockIdx.y];
  const int np2 = jb.n_pow2;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (kk > np2 || i >= np2) return;                        // a shorter segment has no stage kk
  unsigned long long *keys = jb.keys;
  const int l = i ^ j;
  if (l > i) {
    const unsigned long long a = keys[i], b = keys[l];
    const bool up = (i & kk) == 0;
    if ((a > b) == up) { keys[i] = b; keys[l] = a; }
  }
}

// The bitonic network's steps with partner distance j < SORT_CHUNK stay inside a SORT_CHUNK-key block: one workgroup
// runs them back to back in LDS instead of one launch per step.  first_kk == 2: every stage up to min(n_pow2, SORT_CHUNK)
// (a full sort of each block, direction by the index in the segment); otherwise the tail (j = SORT_CHUNK/2 .. 1) of
// stage kk = first_kk = last_kk, in the segments that have that stage.
#define SORT_CHUNK 2048
__global__ __launch_bounds__(SORT_CHUNK / 2) void k_bitonic_local(const ExtractJob *__restrict__ jobs, int first_kk, int last_kk)
{
  __shared__ unsigned long long sk[SORT_CHUNK];
  const ExtractJob &jb = jobs[blockIdx.y];
  const int n_pow2 = jb.n_pow2;
  if (n_pow2 == 0 || (first_kk > 2 && last_kk > n_pow2)) return;
  const int chunk = min(n_pow2, SORT_CHUNK), base = blockIdx.x * chunk, t = threadIdx.x;
  if (base >= n_pow2) return;                              // block-uniform
  if (first_kk == 2) last_kk = chunk;
  unsigned long long *keys = jb.keys;
  for (int e = t; e < chunk; e += SORT_CHUNK / 2) sk[e] = keys[base + e];
  __syncthreads();
  for (int kk = first_kk; kk <= last_kk; kk <<= 1) {
    for (int j = min(kk >> 1, chunk >> 1); j > 0; j >>= 1) {
      if (t < (chunk >> 1)) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long a = sk[i], b = sk[l];
        const bool up = ((base + i) & kk) == 0;
        if ((a > b) == up) { sk[i] = b; sk[l] = a; }
      }
      __syncthreads();
    }
  }
  for (int e = t; e < chunk; e += SORT_CHUNK / 2) keys[base + e] = sk[e];
}

// selectScatteredFeatures (:135-164), one workgroup per job.  The reference re-tests every candidate against every
// chosen feature on every pass (~candidates x features x passes distance tests, with the distance dropping by one per
// pass).  Here each candidate carries mind2 = its squared distance to the nearest chosen feature so far, so `keep` is
// one compare, an accepted feature is folded into mind2 with one test per candidate, and the sequential walk "next
// candidate at or after i that passes" is a workgroup-wide min.  Same features in the same order.  Thread t owns
// candidates t, t + 1024, ...: xy / mind2 (global scratch) are only ever touched by their owner, so no fences are needed.
#define SEL_BS 1024
__global__ __launch_bounds__(SEL_BS) void k_select_scattered(const ExtractJob *__restrict__ jobs)
{
  __shared__ int s_min[SEL_BS / 64];
  const ExtractJob &jb = jobs[blockIdx.x];
  const int tid = threadIdx.x;
  ExtractCounters *cnt = jb.cnt;
  const unsigned long long *keys = jb.keys;
  const int w = jb.w, num_features = jb.num_features, depth_mode = jb.depth_mode;
  uint32_t *xy = jb.xy;
  int *mind2 = jb.mind2;
  const int n = cnt->n_cand;
  // "We require a certain number of features"; n_pow2 == 0: a job of the same view has too few
  if (jb.n_pow2 == 0 || n < num_features || num_features > 1024) { if (tid == 0) cnt->n_out = -1; return; }
  float distance;
  if (depth_mode) {
    // countNonZero(local_mask) with a mask (depth_mode 2), the pixel count without (:815-817)
    const float area = cnt->area > 0 || depth_mode == 2 ? (float)cnt->area : (float)jb.total_px;
    distance = sqrtf(area) / sqrtf((float)num_features) + 1.5f;
  } else {
    distance = (float)(n / num_features + 1);                                    // :503-505
  }
  float distance_sq = distance * distance;
  for (int c = tid; c < n; c += SEL_BS) {
    const unsigned raster = (unsigned)(keys[c] & 0xFFFFFFFFull);
    xy[c] = (raster % (unsigned)w) | ((raster / (unsigned)w) << 16);
    mind2[c] = INT_MAX;                                    // no feature chosen yet: every test passes
  }
  int nf = 0, i = 0, fx = 0, fy = 0;
  bool fold = false;
  while (nf < num_features) {
    int mine = INT_MAX;                                    // my first candidate >= i that is far enough from all features
    for (int c = tid; c < n; c += SEL_BS) {
      int m = mind2[c];
      if (fold) {
        const uint32_t u = xy[c];
        const int dx = (int)(u & 0xFFFFu) - fx, dy = (int)(u >> 16) - fy;
        m = min(m, dx * dx + dy * dy);
        mind2[c] = m;
      }
      if (c >= i && (float)m >= distance_sq) mine = min(mine, c);
    }
    fold = false;
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) mine = min(mine, __shfl_xor(mine, sft, 64));
    __syncthreads();                                       // s_min of the previous round has been read by everyone
    if ((tid & 63) == 0) s_min[tid >> 6] = mine;
    __syncthreads();
    int p = INT_MAX;
#pragma unroll
    for (int k = 0; k < SEL_BS / 64; ++k) p = min(p, s_min[k]);
    if (p == INT_MAX) {                                    // nobody up to the end of the list: relax and start over
      i = 0;
      distance -= 1.0f;
      distance_sq = distance * distance;
      continue;
    }
    const int raster = (int)(keys[p] & 0xFFFFFFFFull);
    fx = raster % w;
    fy = raster / w;
    if (tid == 0) {
      jb.out[nf].x = fx;
      jb.out[nf].y = fy;
      jb.out[nf].label = ex_label(jb.labels[raster]);
    }
    fold = true;
    ++nf;
    i = p + 1;
    if (i == n) {                                          // start over with a relaxed distance
      i = 0;
      distance -= 1.0f;
      distance_sq = distance * distance;
    }
  }
  if (tid == 0) cnt->n_out = nf;
}

int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// A view's slab (offsets from the view's base, every array 256-byte aligned; px_l = (w0 >> l) * (h0 >> l)):
//   colour A (3 px_0) | colour B (3 px_1) | depth (2 px_0) | local mask (px_0) | depth candidates' raster, score
//   (4 px_0 each) | per level: mask, normals (px_l each) and per modality the key segment (8 next_pow2(px_l)) and the
//   selection's xy, mind2 (4 px_l each).  The colour labels (px_l per level) and the magnitude (4 px_0) of the chunk's
//   views sit in arrays of their own (k_color_quantize writes them at the pitch of one image).  include/fealess_hip.h
//   states the total per view.
struct ViewLayout {
  size_t bgr0, bgr1, depth, local, raster, score;
  size_t mask[FL_MAX_LEVELS], normal[FL_MAX_LEVELS];
  size_t keys[FL_MAX_LEVELS][2], xy[FL_MAX_LEVELS][2], mind2[FL_MAX_LEVELS][2];
  size_t bytes;
};

ViewLayout view_layout(int w0, int h0, int levels)
{
  ViewLayout v;
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off += fl_align(b, 256); return o; };
  const size_t px = (size_t)w0 * h0, px1 = (size_t)(w0 >> 1) * (h0 >> 1);
  v.bgr0 = take(px * 3);
  v.bgr1 = take(px1 * 3);
  v.depth = take(px * 2);
  v.local = take(px);
  v.raster = take(px * 4);
  v.score = take(px * 4);
  for (int l = 0; l < levels; ++l) {
    const size_t pl = (size_t)(w0 >> l) * (h0 >> l);
    v.mask[l] = take(pl);
    v.normal[l] = take(pl);
    for (int m = 0; m < 2; ++m) {
      v.keys[l][m] = take((size_t)next_pow2((int)pl) * 8);
      v.xy[l][m] = take(pl * 4);
      v.mind2[l][m] = take(pl * 4);
    }
  }
  v.bytes = off;
  return v;
}

}  // namespace

// cropTemplates (:52-96), host side
static void crop_templates(fl_template *t, int n, fl_feature *f, int bb[4])
{
  int min_x = INT_MAX, min_y = INT_MAX, max_x = INT_MIN, max_y = INT_MIN;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < t[i].feat_count; ++j) {
      const int x = f[t[i].feat_begin + j].x << t[i].pyramid_level, y = f[t[i].feat_begin + j].y << t[i].pyramid_level;
      min_x = x < min_x ? x : min_x;
      min_y = y < min_y ? y : min_y;
      max_x = x > max_x ? x : max_x;
      max_y = y > max_y ? y : max_y;
    }
  if (min_x % 2 == 1) --min_x;
  if (min_y % 2 == 1) --min_y;
  for (int i = 0; i < n; ++i) {
    t[i].width = (max_x - min_x) >> t[i].pyramid_level;
    t[i].height = (max_y - min_y) >> t[i].pyramid_level;
    t[i].offset_x = min_x >> t[i].pyramid_level;
    t[i].offset_y = min_y >> t[i].pyramid_level;
    for (int j = 0; j < t[i].feat_count; ++j) {
      f[t[i].feat_begin + j].x -= t[i].offset_x;
      f[t[i].feat_begin + j].y -= t[i].offset_y;
    }
  }
  bb[0] = min_x; bb[1] = min_y; bb[2] = max_x - min_x; bb[3] = max_y - min_y;
}

// The launches behind the job list: every job's keys[0 .. n_cand) padded to n_pow2 keys and sorted as its own segment,
// then the selection.  max_np2: the largest n_pow2 of the nj jobs (0: nothing to sort).
static int launch_sort_select(fl_context *ctx, const ExtractJob *d_jobs, int nj, int max_np2)
{
  const dim3 blk(256);
  if (max_np2 > 0) {
    hipLaunchKernelGGL(k_pad_keys, dim3(std::min((max_np2 + 255) / 256, 64), nj), blk, 0, ctx->stream, d_jobs);
    hipLaunchKernelGGL(k_bitonic_local, dim3(max_np2 / std::min(max_np2, SORT_CHUNK), nj), dim3(SORT_CHUNK / 2), 0, ctx->stream,
                       d_jobs, 2, SORT_CHUNK);
    for (int kk = 2 * SORT_CHUNK; kk <= max_np2; kk <<= 1) {
      for (int j = kk >> 1; j >= SORT_CHUNK; j >>= 1)
        hipLaunchKernelGGL(k_bitonic_step, dim3(max_np2 / 256, nj), blk, 0, ctx->stream, d_jobs, kk, j);
      hipLaunchKernelGGL(k_bitonic_local, dim3(max_np2 / SORT_CHUNK, nj), dim3(SORT_CHUNK / 2), 0, ctx->stream, d_jobs,
                         kk, kk);
    }
    FL_HIP(ctx, hipGetLastError());
  }
  hipLaunchKernelGGL(k_select_scattered, dim3(nj), dim3(SEL_BS), 0, ctx->stream, d_jobs);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

// One pyramid level of one modality for n views, queued on the context's stream: what extract_chunk runs per level and what
// fl_dev_extract_quantized runs on a caller's quantized images.  View z's mask, local mask, normals, raster / score lists and
// key segment sit at a pitch of vs bytes, its colour labels and magnitude at a pitch of w * h elements, its counters at
// cnt + z * cnt_stride.  d_flags[z] = 0: the view has no mask; any_mask = false: none has, k_local_mask is not launched.
static int launch_color_level(fl_context *ctx, const uint8_t *quantized, const float *mag, const uint8_t *mask, uint8_t *local, uint8_t *keys,
                              size_t vs, const int *d_flags, bool any_mask, int n, int w, int h, float strong_threshold,
                              ExtractCounters *cnt, int cnt_stride)
{
  const dim3 grid((w + 63) / 64, (h + 3) / 4, n), blk(256);
  if (any_mask) hipLaunchKernelGGL(k_local_mask, grid, blk, 0, ctx->stream, mask, local, vs, d_flags, w, h, 1, 1);
  hipLaunchKernelGGL(k_color_candidates, grid, blk, 0, ctx->stream, quantized, mag, local, vs, d_flags, w, h,
                     strong_threshold * strong_threshold, keys, cnt, cnt_stride);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

static int launch_depth_level(fl_context *ctx, const uint8_t *normal, const uint8_t *mask, uint8_t *local, uint8_t *raster, uint8_t *score,
                              uint8_t *keys, size_t vs, const int *d_flags, bool any_mask, int n, int w, int h, int extract_threshold,
                              ExtractCounters *cnt, int cnt_stride)
{
  const dim3 grid((w + 63) / 64, (h + 3) / 4, n), blk(256);
  if (any_mask) hipLaunchKernelGGL(k_local_mask, grid, blk, 0, ctx->stream, mask, local, vs, d_flags, w, h, 2, 0);
  hipLaunchKernelGGL(k_depth_candidates, grid, blk, 0, ctx->stream, normal, local, vs, d_flags, w, h, extract_threshold, raster, score, cnt,
                     cnt_stride);
  const int kb = (int)std::min<size_t>(((size_t)w * h + 255) / 256, 64);
  hipLaunchKernelGGL(k_depth_keys, dim3(kb, 1, n), blk, 0, ctx->stream, normal, raster, score, vs, cnt, cnt_stride, keys);
  FL_HIP(ctx, hipGetLastError());
  return FL_OK;
}

// The record of one job, once its candidate count is known.  sortable = false: the job's view cannot yield a template
// (this job or another of the view has fewer candidates than features), nothing is sorted or selected.
static ExtractJob make_job(unsigned long long *keys, const uint8_t *labels, uint32_t *xy, int *mind2, ExtractCounters *cnt, fl_feature *out,
                           int w, int total_px, int num_features, int depth_mode, int n_cand, bool sortable)
{
  ExtractJob jb;
  jb.keys = keys;
  jb.labels = labels;
  jb.xy = xy;
  jb.mind2 = mind2;
  jb.cnt = cnt;
  jb.out = out;
  jb.w = w;
  jb.num_features = num_features;
  jb.depth_mode = depth_mode;
  jb.total_px = total_px;
  jb.n_pow2 = sortable ? next_pow2(n_cand) : 0;
  jb.pad = 0;
  return jb;
}

// Views [v0, v0 + n) of a batch, n <= FL_EXTRACT_CHUNK_VIEWS: outputs at the batch's indices (feat_begin absolute).
static int extract_chunk(fl_context *ctx, int v0, int n, const uint8_t *const *bgr, const uint16_t *const *depth, const uint8_t *const *mask,
                         int w0, int h0, int levels, int mem, fl_template *templates, fl_feature *features, int32_t *bb, int32_t *status)
{
  const int M = 2, J = levels * M;                         // jobs per view, index l * 2 + m
  const ViewLayout lo = view_layout(w0, h0, levels);
  const size_t vs = lo.bytes;
  // device: view slabs | colour labels per level (n px_l) | magnitude (n 4 px_0) | then, also in pinned host memory at
  // the same relative offsets: has_mask[n] | counters[n J] | features[n J 64] | jobs[n J]
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off += fl_align(b, 256); return o; };
  const size_t px = (size_t)w0 * h0;
  const size_t o_views = take(vs * n);
  size_t o_quant[FL_MAX_LEVELS];
  for (int l = 0; l < levels; ++l) o_quant[l] = take((size_t)n * (w0 >> l) * (h0 >> l));
  const size_t o_mag = take(px * 4 * n), o_flags = take(sizeof(int) * n), o_cnt = take(sizeof(ExtractCounters) * n * J),
               o_feats = take(sizeof(fl_feature) * 64 * n * J), o_jobs = take(sizeof(ExtractJob) * n * J);
  void *sv = nullptr, *pv = nullptr;
  int rc = fl_scratch(ctx, off, &sv);
  if (rc) return rc;
  if ((rc = fl_pinned(ctx, off - o_flags, &pv))) return rc;
  uint8_t *s = (uint8_t *)sv, *vw = s + o_views;
  auto pin = [&](size_t o) { return (uint8_t *)pv + (o - o_flags); };
  int *d_flags = (int *)(s + o_flags), *h_flags = (int *)pin(o_flags);
  ExtractCounters *d_cnt = (ExtractCounters *)(s + o_cnt), *h_cnt = (ExtractCounters *)pin(o_cnt);
  fl_feature *d_feats = (fl_feature *)(s + o_feats), *h_feats = (fl_feature *)pin(o_feats);
  ExtractJob *d_jobs = (ExtractJob *)(s + o_jobs), *h_jobs = (ExtractJob *)pin(o_jobs);

  const hipMemcpyKind kind = mem == FL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  bool any_mask = false;
  for (int v = 0; v < n; ++v) {
    uint8_t *b = vw + (size_t)v * vs;
    const uint8_t *mk = mask ? mask[v0 + v] : nullptr;
    FL_HIP(ctx, hipMemcpyAsync(b + lo.bgr0, bgr[v0 + v], px * 3, kind, ctx->stream));
    FL_HIP(ctx, hipMemcpyAsync(b + lo.depth, depth[v0 + v], px * 2, kind, ctx->stream));
    if (mk) FL_HIP(ctx, hipMemcpyAsync(b + lo.mask[0], mk, px, kind, ctx->stream));
    h_flags[v] = mk != nullptr;
    any_mask = any_mask || mk;
  }
  FL_HIP(ctx, hipMemcpyAsync(d_flags, h_flags, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(ExtractCounters) * n * J, ctx->stream));

  // modality 0: ColorGradient(10, 63, 55) (:515-519); pyrDown :434-453.  The NN-halved mask pyramid made here is also
  // modality 1's: it halves the same level-0 mask the same way (:721-739).
  {
    int w = w0, h = h0;
    for (int l = 0; l < levels; ++l) {
      const size_t img = (l & 1) ? lo.bgr1 : lo.bgr0;      // level l's colour image: A for even levels, B for odd ones
      if (l > 0) {
        if ((rc = fl_launch_pyrdown_bgr(ctx, vw + ((l & 1) ? lo.bgr0 : lo.bgr1), vs, vw + img, vs, n, w, h))) return rc;
        if (any_mask && (rc = fl_launch_resize_nn_half(ctx, vw + lo.mask[l - 1], vs, vw + lo.mask[l], vs, n, w, h))) return rc;
        w /= 2;
        h /= 2;
      }
      if ((rc = fl_launch_quantized_orientations_mag(ctx, vw + img, vs, s + o_quant[l], (size_t)w * h, n, w, h, 10.0f, (float *)(s + o_mag))))
        return rc;
      if ((rc = launch_color_level(ctx, s + o_quant[l], (const float *)(s + o_mag), vw + lo.mask[l], vw + lo.local, vw + lo.keys[l][0], vs, d_flags,
                                   any_mask, n, w, h, 55.0f, d_cnt + l * M + 0, J)))
        return rc;
    }
  }
  // modality 1: DepthNormal(2000, 50, 63, 2) (:827-832)
  {
    int w = w0, h = h0;
    if ((rc = fl_launch_quantized_normals(ctx, (const uint16_t *)(vw + lo.depth), vs, vw + lo.normal[0], vs, nullptr, 0, n, w, h, 2000, 50)))
      return rc;
    for (int l = 0; l < levels; ++l) {
      if (l > 0) {
        if ((rc = fl_launch_resize_nn_half(ctx, vw + lo.normal[l - 1], vs, vw + lo.normal[l], vs, n, w, h))) return rc;
        w /= 2;
        h /= 2;
      }
      // raster / score are reused by the next level, whose candidates queue behind this level's keys
      if ((rc = launch_depth_level(ctx, vw + lo.normal[l], vw + lo.mask[l], vw + lo.local, vw + lo.raster, vw + lo.score, vw + lo.keys[l][1], vs,
                                   d_flags, any_mask, n, w, h, 2 >> l, d_cnt + l * M + 1, J)))
        return rc;
    }
  }

  // host round trip 1: every job's candidate count sizes its sort segment
  FL_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(ExtractCounters) * n * J, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int max_np2 = 0;
  for (int v = 0; v < n; ++v) {
    bool view_ok = true;                                   // a view that cannot yield a template sorts nothing
    for (int k = 0; k < J; ++k) view_ok = view_ok && h_cnt[v * J + k].n_cand >= (63 >> (k / M));
    uint8_t *b = vw + (size_t)v * vs;
    for (int k = 0; k < J; ++k) {
      const int l = k / M, m = k % M;
      const int total_px = (w0 >> l) * (h0 >> l);
      ExtractJob &jb = h_jobs[v * J + k];
      jb = make_job((unsigned long long *)(b + lo.keys[l][m]), m == 0 ? s + o_quant[l] + (size_t)v * total_px : b + lo.normal[l],
                    (uint32_t *)(b + lo.xy[l][m]), (int *)(b + lo.mind2[l][m]), d_cnt + v * J + k, d_feats + (size_t)64 * (v * J + k), w0 >> l,
                    total_px, 63 >> l, m == 0 ? 0 : (h_flags[v] ? 2 : 1), h_cnt[v * J + k].n_cand, view_ok);
      max_np2 = std::max(max_np2, jb.n_pow2);
    }
  }
  const int nj = n * J;
  FL_HIP(ctx, hipMemcpyAsync(d_jobs, h_jobs, sizeof(ExtractJob) * nj, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = launch_sort_select(ctx, d_jobs, nj, max_np2))) return rc;

  // host round trip 2: the counters (n_out) and the selected features
  FL_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(ExtractCounters) * nj, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(h_feats, d_feats, sizeof(fl_feature) * 64 * nj, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int v = 0; v < n; ++v) {
    const int gv = v0 + v;
    bool ok = true;
    for (int k = 0; k < J; ++k) ok = ok && h_cnt[v * J + k].n_out == (63 >> (k / M));
    fl_template *t = templates + (size_t)gv * J;
    for (int k = 0; k < J; ++k) {
      t[k].width = t[k].height = -1;
      t[k].offset_x = t[k].offset_y = 0;
      t[k].pyramid_level = k / M;
      t[k].feat_begin = 63 * (gv * J + k);
      t[k].feat_count = ok ? 63 >> (k / M) : 0;
      for (int j = 0; j < t[k].feat_count; ++j) features[t[k].feat_begin + j] = h_feats[(size_t)64 * (v * J + k) + j];
    }
    int box[4] = {0, 0, 0, 0};
    if (ok) crop_templates(t, J, features, box);
    for (int c = 0; c < 4; ++c) bb[4 * gv + c] = box[c];
    status[gv] = ok ? FL_OK : FL_ERR_NO_TEMPLATE;
  }
  return FL_OK;
}

extern "C" int fl_extract_template_batch(fl_context *ctx, int n_views, const uint8_t *const *bgr, const uint16_t *const *depth,
                                         const uint8_t *const *mask, int w0, int h0, int levels, int mem, fl_template *templates,
                                         fl_feature *features, int32_t *bb, int32_t *status)
{
  if (!ctx || n_views < 1 || !bgr || !depth || !templates || !features || !bb || !status || w0 < 16 || h0 < 16 || levels < 1 ||
      levels > FL_MAX_LEVELS)
    return FL_ERR_INVALID;
  if ((w0 >> (levels - 1)) < 8 || (h0 >> (levels - 1)) < 8) return fl_set_error(ctx, FL_ERR_INVALID, "image too small for %d levels", levels);
  for (int v = 0; v < n_views; ++v)
    if (!bgr[v] || !depth[v]) return fl_set_error(ctx, FL_ERR_INVALID, "view %d: null image", v);
  FL_HIP(ctx, hipSetDevice(ctx->device));
  for (int v0 = 0; v0 < n_views; v0 += FL_EXTRACT_CHUNK_VIEWS) {
    const int rc = extract_chunk(ctx, v0, std::min(FL_EXTRACT_CHUNK_VIEWS, n_views - v0), bgr, depth, mask, w0, h0, levels, mem, templates,
                                 features, bb, status);
    if (rc) return rc;
  }
  return FL_OK;
}

extern "C" int fl_extract_template_pyramid(fl_context *ctx, const uint8_t *bgr, const uint16_t *depth, const uint8_t *mask, int w0,
                                           int h0, int levels, int mem, fl_template *templates, fl_feature *features, int bb[4])
{
  if (!bgr || !depth) return FL_ERR_INVALID;
  int32_t box[4], st = FL_OK;
  const int rc = fl_extract_template_batch(ctx, 1, &bgr, &depth, mask ? &mask : nullptr, w0, h0, levels, mem, templates, features, box, &st);
  if (rc) return rc;
  if (st != FL_OK) return fl_set_error(ctx, FL_ERR_NO_TEMPLATE, "too few candidate features at some pyramid level (addTemplate returns -1)");
  if (bb) { bb[0] = box[0]; bb[1] = box[1]; bb[2] = box[2]; bb[3] = box[3]; }
  return FL_OK;
}

// see fl_internal.h
extern "C" int fl_dev_extract_select(fl_context *ctx, int n_jobs, const fl_dev_select_job *jobs)
{
  if (!ctx || n_jobs < 1 || n_jobs > 4096 || !jobs) return FL_ERR_INVALID;
  for (int k = 0; k < n_jobs; ++k) {
    const fl_dev_select_job &j = jobs[k];
    if (!j.labels || !j.n_out || !j.features || !j.sorted_keys || j.n_cand < 0 || j.n_cand > (1 << 24) || (j.n_cand > 0 && (!j.raster || !j.score)))
      return FL_ERR_INVALID;
    if (j.num_features < 1 || j.num_features > FL_MAX_FEATURES || j.depth_mode < 0 || j.depth_mode > 2 || j.area < 0) return FL_ERR_INVALID;
    // the selection packs a candidate's x and y into 16 bits each
    if (j.w < 1 || j.w > 65536 || j.total_px < j.w || j.total_px % j.w || j.total_px / j.w > 65536) return FL_ERR_INVALID;
    // A depth job's start distance is fractional and never reaches 0: fewer than num_features distinct pixels would
    // never finish, in the reference as here.  A colour job's distance reaches 0, where a repeated pixel passes.
    std::vector<bool> seen(j.depth_mode ? (size_t)j.total_px : 0);
    for (int c = 0; c < j.n_cand; ++c) {
      if (j.raster[c] < 0 || j.raster[c] >= j.total_px || !(j.score[c] > 0.0f)) return FL_ERR_INVALID;   // keys order positive scores only
      if (j.depth_mode) {
        if (seen[j.raster[c]]) return FL_ERR_INVALID;
        seen[j.raster[c]] = true;
      }
    }
  }
  // device, mirrored in pinned host memory: per job keys (next_pow2(n_cand)) | labels, then counters | features | jobs;
  // device only: per job xy | mind2
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off += fl_align(b, 256); return o; };
  std::vector<size_t> o_keys(n_jobs), o_labels(n_jobs), o_xy(n_jobs), o_mind2(n_jobs);
  for (int k = 0; k < n_jobs; ++k) {
    o_keys[k] = take((size_t)next_pow2(std::max(jobs[k].n_cand, 1)) * 8);
    o_labels[k] = take((size_t)jobs[k].total_px);
  }
  const size_t o_cnt = take(sizeof(ExtractCounters) * n_jobs), o_feats = take(sizeof(fl_feature) * 64 * n_jobs),
               o_jobs = take(sizeof(ExtractJob) * n_jobs), mirrored = off;
  for (int k = 0; k < n_jobs; ++k) {
    o_xy[k] = take((size_t)jobs[k].n_cand * 4);
    o_mind2[k] = take((size_t)jobs[k].n_cand * 4);
  }
  void *sv = nullptr, *pv = nullptr;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  int rc = fl_scratch(ctx, off, &sv);
  if (rc) return rc;
  if ((rc = fl_pinned(ctx, mirrored, &pv))) return rc;
  uint8_t *s = (uint8_t *)sv, *p = (uint8_t *)pv;
  ExtractCounters *h_cnt = (ExtractCounters *)(p + o_cnt);
  fl_feature *h_feats = (fl_feature *)(p + o_feats);
  ExtractJob *h_jobs = (ExtractJob *)(p + o_jobs);
  int max_np2 = 0;
  for (int k = 0; k < n_jobs; ++k) {
    const fl_dev_select_job &j = jobs[k];
    unsigned long long *keys = (unsigned long long *)(p + o_keys[k]);
    for (int c = 0; c < j.n_cand; ++c) keys[c] = ex_pack_key(j.score[c], j.raster[c]);
    memcpy(p + o_labels[k], j.labels, (size_t)j.total_px);
    memset(&h_cnt[k], 0, sizeof(ExtractCounters));
    h_cnt[k].n_cand = j.n_cand;
    h_cnt[k].area = j.area;
    memcpy(h_feats + (size_t)64 * k, j.features, sizeof(fl_feature) * 64);   // what the kernel does not write comes back as it went in
    ExtractJob &jb = h_jobs[k];
    jb = make_job((unsigned long long *)(s + o_keys[k]), s + o_labels[k], (uint32_t *)(s + o_xy[k]), (int *)(s + o_mind2[k]),
                  (ExtractCounters *)(s + o_cnt) + k, (fl_feature *)(s + o_feats) + (size_t)64 * k, j.w, j.total_px, j.num_features, j.depth_mode,
                  j.n_cand, j.n_cand >= j.num_features);
    max_np2 = std::max(max_np2, jb.n_pow2);
  }
  FL_HIP(ctx, hipMemcpyAsync(s, p, mirrored, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = launch_sort_select(ctx, (const ExtractJob *)(s + o_jobs), n_jobs, max_np2))) return rc;
  FL_HIP(ctx, hipMemcpyAsync(p, s, o_jobs, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n_jobs; ++k) {
    const fl_dev_select_job &j = jobs[k];
    *j.n_out = h_cnt[k].n_out;
    memcpy(j.features, h_feats + (size_t)64 * k, sizeof(fl_feature) * 64);
    if (h_jobs[k].n_pow2 > 0) memcpy(j.sorted_keys, p + o_keys[k], (size_t)j.n_cand * 8);
  }
  return FL_OK;
}

// see fl_internal.h
extern "C" int fl_dev_extract_quantized(fl_context *ctx, int n_views, const fl_dev_extract_view *views, int w, int h, int modality,
                                        float strong_threshold, int extract_threshold, int num_features)
{
  if (!ctx || !views || n_views < 1 || n_views > FL_EXTRACT_CHUNK_VIEWS || modality < 0 || modality > 1) return FL_ERR_INVALID;
  if (num_features < 1 || num_features > FL_MAX_FEATURES) return FL_ERR_INVALID;
  // the selection packs a candidate's x and y into 16 bits each; rasters are ints and every list holds w * h entries
  if (w < 1 || h < 1 || w > 65536 || h > 65536 || (size_t)w * h > ((size_t)1 << 24)) return FL_ERR_INVALID;
  bool any_mask = false;
  for (int v = 0; v < n_views; ++v) {
    const fl_dev_extract_view &vw = views[v];
    if (!vw.quantized || (modality == 0 && !vw.magnitude) || (vw.mask && !vw.local_mask) || !vw.counters || !vw.cand_raster || !vw.cand_score ||
        !vw.sorted_keys || !vw.features)
      return FL_ERR_INVALID;
    any_mask = any_mask || vw.mask;
  }
  const int n = n_views;
  const size_t px = (size_t)w * h;
  // a view's slab: mask | local mask | normals | depth candidates' raster, score | key segment | the selection's xy, mind2
  size_t off = 0;
  auto take = [&](size_t b) { size_t o = off; off += fl_align(b, 256); return o; };
  const size_t v_mask = take(px), v_local = take(px), v_normal = take(px), v_raster = take(px * 4), v_score = take(px * 4),
               v_keys = take((size_t)next_pow2((int)px) * 8), v_xy = take(px * 4), v_mind2 = take(px * 4), vs = off;
  // device: view slabs | colour labels (n px) | magnitude (n 4 px) | then, also in pinned host memory at the same relative
  // offsets: has_mask[n] | counters[n] | features[n 64] | jobs[n]
  off = 0;
  const size_t o_views = take(vs * n), o_quant = take(px * n), o_mag = take(px * 4 * n), o_flags = take(sizeof(int) * n),
               o_cnt = take(sizeof(ExtractCounters) * n), o_feats = take(sizeof(fl_feature) * 64 * n), o_jobs = take(sizeof(ExtractJob) * n);
  void *sv = nullptr, *pv = nullptr;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  int rc = fl_scratch(ctx, off, &sv);
  if (rc) return rc;
  if ((rc = fl_pinned(ctx, off - o_flags, &pv))) return rc;
  uint8_t *s = (uint8_t *)sv, *slab = s + o_views;
  auto pin = [&](size_t o) { return (uint8_t *)pv + (o - o_flags); };
  int *d_flags = (int *)(s + o_flags), *h_flags = (int *)pin(o_flags);
  ExtractCounters *d_cnt = (ExtractCounters *)(s + o_cnt), *h_cnt = (ExtractCounters *)pin(o_cnt);
  fl_feature *d_feats = (fl_feature *)(s + o_feats), *h_feats = (fl_feature *)pin(o_feats);
  ExtractJob *d_jobs = (ExtractJob *)(s + o_jobs), *h_jobs = (ExtractJob *)pin(o_jobs);

  for (int v = 0; v < n; ++v) {
    const fl_dev_extract_view &vw = views[v];
    uint8_t *b = slab + (size_t)v * vs;
    if (modality == 0) {
      FL_HIP(ctx, hipMemcpyAsync(s + o_quant + v * px, vw.quantized, px, hipMemcpyHostToDevice, ctx->stream));
      FL_HIP(ctx, hipMemcpyAsync(s + o_mag + v * px * 4, vw.magnitude, px * 4, hipMemcpyHostToDevice, ctx->stream));
    } else {
      FL_HIP(ctx, hipMemcpyAsync(b + v_normal, vw.quantized, px, hipMemcpyHostToDevice, ctx->stream));
    }
    if (vw.mask) {
      FL_HIP(ctx, hipMemcpyAsync(b + v_mask, vw.mask, px, hipMemcpyHostToDevice, ctx->stream));
      // what k_local_mask does not write comes back as it went in; a view without a mask keeps whatever the slab holds
      FL_HIP(ctx, hipMemcpyAsync(b + v_local, vw.local_mask, px, hipMemcpyHostToDevice, ctx->stream));
    }
    h_flags[v] = vw.mask != nullptr;
    memcpy(h_feats + (size_t)64 * v, vw.features, sizeof(fl_feature) * 64);
  }
  FL_HIP(ctx, hipMemcpyAsync(d_flags, h_flags, sizeof(int) * n, hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(d_feats, h_feats, sizeof(fl_feature) * 64 * n, hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(ExtractCounters) * n, ctx->stream));
  if (modality == 0)
    rc = launch_color_level(ctx, s + o_quant, (const float *)(s + o_mag), slab + v_mask, slab + v_local, slab + v_keys, vs, d_flags, any_mask, n,
                            w, h, strong_threshold, d_cnt, 1);
  else
    rc = launch_depth_level(ctx, slab + v_normal, slab + v_mask, slab + v_local, slab + v_raster, slab + v_score, slab + v_keys, vs, d_flags,
                            any_mask, n, w, h, extract_threshold, d_cnt, 1);
  if (rc) return rc;

  // host round trip 1: the candidate counts; the lists as they stand before the sort leave ahead of it in stream order
  FL_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(ExtractCounters) * n, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::vector<size_t> first(n + 1, 0);
  for (int v = 0; v < n; ++v) {
    if (h_cnt[v].n_cand < 0 || (size_t)h_cnt[v].n_cand > px) return fl_set_error(ctx, FL_ERR_INVALID, "view %d: %d candidates of %zu pixels", v, h_cnt[v].n_cand, px);
    first[v + 1] = first[v] + (modality == 0 ? h_cnt[v].n_cand : 0);
  }
  std::vector<unsigned long long> unsorted(first[n]);      // colour: the candidates exist as keys only
  int max_np2 = 0;
  for (int v = 0; v < n; ++v) {
    const fl_dev_extract_view &vw = views[v];
    uint8_t *b = slab + (size_t)v * vs;
    const int nc = h_cnt[v].n_cand;
    h_jobs[v] = make_job((unsigned long long *)(b + v_keys), modality == 0 ? s + o_quant + v * px : b + v_normal, (uint32_t *)(b + v_xy),
                         (int *)(b + v_mind2), d_cnt + v, d_feats + (size_t)64 * v, w, (int)px, num_features,
                         modality == 0 ? 0 : (h_flags[v] ? 2 : 1), nc, nc >= num_features);
    max_np2 = std::max(max_np2, h_jobs[v].n_pow2);
    if (nc == 0) continue;
    if (modality == 0) {
      FL_HIP(ctx, hipMemcpyAsync(unsorted.data() + first[v], b + v_keys, (size_t)nc * 8, hipMemcpyDeviceToHost, ctx->stream));
    } else {
      FL_HIP(ctx, hipMemcpyAsync(vw.cand_raster, b + v_raster, (size_t)nc * 4, hipMemcpyDeviceToHost, ctx->stream));
      FL_HIP(ctx, hipMemcpyAsync(vw.cand_score, b + v_score, (size_t)nc * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
  }
  FL_HIP(ctx, hipMemcpyAsync(d_jobs, h_jobs, sizeof(ExtractJob) * n, hipMemcpyHostToDevice, ctx->stream));
  if ((rc = launch_sort_select(ctx, d_jobs, n, max_np2))) {
    (void)hipStreamSynchronize(ctx->stream);                  // copies into `unsorted` and the caller's lists may be in flight
    return rc;
  }

  // host round trip 2: the counters (n_out), the features, the local masks and the sorted segments
  FL_HIP(ctx, hipMemcpyAsync(h_cnt, d_cnt, sizeof(ExtractCounters) * n, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(h_feats, d_feats, sizeof(fl_feature) * 64 * n, hipMemcpyDeviceToHost, ctx->stream));
  for (int v = 0; v < n; ++v) {
    const fl_dev_extract_view &vw = views[v];
    uint8_t *b = slab + (size_t)v * vs;
    if (vw.mask) FL_HIP(ctx, hipMemcpyAsync(vw.local_mask, b + v_local, px, hipMemcpyDeviceToHost, ctx->stream));
    if (h_jobs[v].n_pow2 > 0)
      FL_HIP(ctx, hipMemcpyAsync(vw.sorted_keys, b + v_keys, (size_t)h_cnt[v].n_cand * 8, hipMemcpyDeviceToHost, ctx->stream));
  }
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int v = 0; v < n; ++v) {
    const fl_dev_extract_view &vw = views[v];
    static_assert(sizeof(ExtractCounters) == 11 * sizeof(int32_t), "fl_dev_extract_view.counters");
    memcpy(vw.counters, &h_cnt[v], sizeof(ExtractCounters));
    memcpy(vw.features, h_feats + (size_t)64 * v, sizeof(fl_feature) * 64);
    for (size_t c = first[v]; c < first[v + 1]; ++c) {
      vw.cand_raster[c - first[v]] = (int32_t)(unsorted[c] & 0xFFFFFFFFull);
      vw.cand_score[c - first[v]] = __builtin_bit_cast(float, ~(unsigned)(unsorted[c] >> 32));
    }
  }
  return FL_OK;
}
