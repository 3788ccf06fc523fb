// fl_match.hip -- the match stage of the online matching half of cup_linemod::Detector (reference: linemod/linemod.cpp:882-1577):
// the sort of the surviving matches, the launch sequence over the stages of fl_linmem.hip, fl_scan.hip and fl_refine.hip, and
// the fl_match_* entry points.
//
//   k_sort_unique  std::sort + std::unique of the surviving matches         (:1437-1439)
#include "fl_internal.h"

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

// the surviving candidates of n_frames frames into their sorted, de-duplicated match lists
int fl_launch_sort(fl_detector *det, int n_frames)
{
  fl_context *ctx = det->ctx;
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
  if (int rc = fl_launch_scan(det, n_frames, threshold, nullptr, 0, 0)) return rc;
  if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[3], ctx->stream));
  if (int rc = fl_launch_refine(det, n_frames, threshold)) return rc;
  if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[4], ctx->stream));
  if (int rc = fl_launch_sort(det, n_frames)) return rc;
  if (det->have_times) FL_HIP(ctx, hipEventRecord(det->ev[5], ctx->stream));
  return FL_OK;
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
  rc = fl_launch_scan(det, 1, 200.0f, (uint16_t *)d, first, count);
  if (rc == FL_OK) rc = fl_launch_refine(det, 1, 200.0f);
  if (rc == FL_OK) rc = fl_launch_sort(det, 1);
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
