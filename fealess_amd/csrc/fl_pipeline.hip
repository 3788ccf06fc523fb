// fl_pipeline.hip -- CObjRecoLmICP::Recognition (CadReco/obj_reco_lmicp.cpp:86-204) for a batch
// of frames: quantise -> linear memories -> scan -> refine -> sort/unique -> (device-side
// hand-over of matches[0]) -> crop back-projection -> ICP -> 4x4 pose, queued with no host
// synchronisation in between.  Every kernel is launched over the whole batch (grid.z / grid.y /
// one workgroup per frame), so the launch count per batch is constant (about a dozen) whatever
// the number of frames.
//
// fl_recognize_submit queues a batch as two stages on two streams (option pipeline_icp, see
// fl_internal.h): staging, front-end, match, refine and sort on the context's stream, then --
// after an event recorded behind the sort -- the ICP stage and the copy of the results on the
// context's ICP stream.  The ICP stage reads only the frame's counters and sorted match list, the
// caller's depth frames and the bank, and the frame workspaces hold the counters and the list
// twice, so the LINEMOD stages of batch i+1 run beside the ICP launch of batch i and fill the
// tails of its occupancy-bound launch.  Batch i+2's match stage waits for ICP(i) before it zeroes
// the set ICP(i) read.  One stream carries everything, in the order above, when pipeline_icp is 0,
// when the caller set a stream of their own (synchronising that stream must finish the work), or
// when device frames had to be gathered into the frame workspaces (ICP reads the depth there).
// Every other entry point first makes the context's stream wait for the ICP stream
// (fl_pipeline_join / fl_context_join).
#include "fl_track_internal.h"
#include <cmath>
#include <vector>
#include <string.h>

static bool uniform_stride(const void *const *ptrs, int n, size_t min_bytes, size_t *stride)
{
  if (n == 1) { *stride = 0; return true; }
  const uint8_t *p0 = (const uint8_t *)ptrs[0], *p1 = (const uint8_t *)ptrs[1];
  if (p1 < p0 + min_bytes) return false;
  const size_t s = (size_t)(p1 - p0);
  for (int i = 2; i < n; ++i)
    if ((const uint8_t *)ptrs[i] != p0 + s * (size_t)i) return false;
  *stride = s;
  return true;
}

// argument checks, frame staging, front-end and Detector::match of a batch, which it records (refinable when depth frames were
// given); the depth frames' device location comes back (K == nullptr: Detector::match only, no intrinsics to check)
// pipelined != nullptr (fl_recognize_submit): the caller may run the ICP stage on the ICP stream; *pipelined says whether it is to
static int stage_and_match(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth, int mem,
                           const fl_intrinsics *K, float threshold, const uint16_t **depth_base_out,
                           size_t *depth_stride_out, int *host_buf_out, bool *pipelined = nullptr)
{
  int host_buf = -1;     // the input buffer the batch was uploaded to (host frames), released by input_done()
  if (!det || !bgr || n_frames <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  int rc = fl_check_frames(det, n_frames);
  if (rc) return rc;
  if (det->M == 2 && !depth) return fl_set_error(ctx, FL_ERR_INVALID, "depth frames required (2 modalities)");
  // PrepareInputData (obj_reco_lmicp.cpp:216-259): image size must equal the intrinsics' size
  if (K && (rc = fl_check_intrinsics(det, K))) return rc;
  for (int i = 0; i < n_frames; ++i)
    if (!bgr[i] || (det->M == 2 && !depth[i])) return fl_set_error(ctx, FL_ERR_INVALID, "frame %d: null pData (CheckTImage)", i);
  FL_HIP(ctx, hipSetDevice(ctx->device));

  const size_t bgr_bytes = (size_t)det->w0 * det->h0 * 3, depth_bytes = (size_t)det->w0 * det->h0 * 2;
  const uint8_t *bgr_base = det->d_ws + det->off_bgr;
  const uint16_t *depth_base = (const uint16_t *)(det->d_ws + det->off_depth);
  size_t bgr_stride = det->ws_stride, depth_stride = det->ws_stride;
  size_t s1 = 0, s2 = 0;
  const bool in_place = mem == FL_MEM_DEVICE && uniform_stride((const void *const *)bgr, n_frames, bgr_bytes, &s1) &&
                        (det->M < 2 || (uniform_stride((const void *const *)depth, n_frames, depth_bytes, &s2) && s2 % 2 == 0));
  // two stages on two streams, or today's one-stream order (see the header comment)
  const bool two_streams = pipelined && ctx->opt.pipeline_icp != 0 && ctx->stream == ctx->own_stream && (in_place || mem == FL_MEM_HOST);
  if (pipelined) *pipelined = two_streams;
  if (two_streams) {                       // this batch's match stage fills the set the ICP stage in flight does not read
    det->set ^= 1;
    det->off_count = det->off_count_set[det->set];
    det->off_match = det->off_match_set[det->set];
  } else if ((rc = pipelined ? fl_context_join(ctx) : fl_pipeline_join(det))) {
    return rc;
  }
  fl_batch_forget(det);
  det->icp_ev = 5;
  if (in_place) {
    // frames already in HBM at a regular pitch: read them in place
    bgr_base = bgr[0];
    bgr_stride = s1;
    if (det->M == 2) { depth_base = depth[0]; depth_stride = s2; }
  } else if (mem == FL_MEM_HOST) {
    // host frames: upload on the copy stream into the input buffer that is not being read (see fl_internal.h)
    const int b = det->in_flip;
    det->in_flip ^= 1;
    const size_t depth_off = fl_align(bgr_bytes, 256), frame_in = depth_off + fl_align(depth_bytes, 256);
    if (!det->copy_stream) FL_HIP(ctx, hipStreamCreateWithFlags(&det->copy_stream, hipStreamNonBlocking));
    if (!det->d_in[b]) {
      FL_HIP(ctx, hipMalloc((void **)&det->d_in[b], frame_in * (size_t)det->max_batch));
      FL_HIP(ctx, hipEventCreateWithFlags(&det->ev_up[b], hipEventDisableTiming));
      FL_HIP(ctx, hipEventCreateWithFlags(&det->ev_read[b], hipEventDisableTiming));
    }
    if (det->read_pending[b]) FL_HIP(ctx, hipStreamWaitEvent(det->copy_stream, det->ev_read[b], 0));
    size_t hs1 = 0, hs2 = 0;
    if (n_frames > 1 && uniform_stride((const void *const *)bgr, n_frames, bgr_bytes, &hs1) &&
        (det->M < 2 || uniform_stride((const void *const *)depth, n_frames, depth_bytes, &hs2))) {
      // frames at a regular pitch (one host array): one strided copy per modality instead of one per frame
      FL_HIP(ctx, hipMemcpy2DAsync(det->d_in[b], frame_in, bgr[0], hs1, bgr_bytes, n_frames, hipMemcpyHostToDevice, det->copy_stream));
      if (det->M == 2)
        FL_HIP(ctx, hipMemcpy2DAsync(det->d_in[b] + depth_off, frame_in, depth[0], hs2, depth_bytes, n_frames, hipMemcpyHostToDevice,
                                     det->copy_stream));
    } else {
      for (int i = 0; i < n_frames; ++i) {
        uint8_t *dst = det->d_in[b] + (size_t)i * frame_in;
        FL_HIP(ctx, hipMemcpyAsync(dst, bgr[i], bgr_bytes, hipMemcpyHostToDevice, det->copy_stream));
        if (det->M == 2) FL_HIP(ctx, hipMemcpyAsync(dst + depth_off, depth[i], depth_bytes, hipMemcpyHostToDevice, det->copy_stream));
      }
    }
    FL_HIP(ctx, hipEventRecord(det->ev_up[b], det->copy_stream));
    FL_HIP(ctx, hipStreamWaitEvent(ctx->stream, det->ev_up[b], 0));
    bgr_base = det->d_in[b];
    bgr_stride = frame_in;
    depth_base = (const uint16_t *)(det->d_in[b] + depth_off);
    depth_stride = frame_in;
    host_buf = b;
  } else {
    for (int i = 0; i < n_frames; ++i) {     // device frames at irregular addresses: gather them into the frame workspaces
      uint8_t *ws = det->d_ws + (size_t)i * det->ws_stride;
      FL_HIP(ctx, hipMemcpyAsync(ws + det->off_bgr, bgr[i], bgr_bytes, hipMemcpyDeviceToDevice, ctx->stream));
      if (det->M == 2) FL_HIP(ctx, hipMemcpyAsync(ws + det->off_depth, depth[i], depth_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
  }
  det->have_times = true;
  FL_HIP(ctx, hipEventRecord(det->ev[0], ctx->stream));
  if ((rc = fl_launch_frontend(det, n_frames, bgr_base, bgr_stride, depth_base, depth_stride, true))) return rc;
  if ((rc = fl_launch_match_core(det, n_frames, threshold))) return rc;
  fl_batch_record(det, n_frames, depth ? depth_base : nullptr, depth_stride, K == nullptr);
  *depth_base_out = depth_base;
  *depth_stride_out = depth_stride;
  *host_buf_out = host_buf;
  return FL_OK;
}

// per-stage device times of the batch that was just synchronised (HIP events recorded on the launch stream)
void fl_update_stage_times(fl_detector *det, int n_frames, const fl_recognition_result *results)
{
  if (!det->have_times) return;
  fl_stage_times &t = det->times;
  memset(&t, 0, sizeof(t));
  float ms = 0;
  auto el = [&](int a, int b) { ms = 0; (void)hipEventElapsedTime(&ms, det->ev[a], det->ev[b]); return ms; };
  t.frontend_ms = el(0, 1);
  t.linmem_ms = el(1, 2);
  t.scan_ms = el(2, 3);
  t.refine_ms = el(3, 4);
  if (det->lazy) {
    for (int l = 0; l + 1 < det->L; ++l) t.lazy_frontend_ms += el(8 + 2 * l, 9 + 2 * l);
    t.refine_ms -= t.lazy_frontend_ms;
  }
  t.sort_ms = el(4, 5);
  // from the event before the ICP launches to the one after them; total_ms spans the batch's first and last event, which for
  // a pipelined batch includes its ICP stage's wait for the ICP stage of the batch before
  t.icp_ms = det->batch.match_only ? 0.f : el(det->icp_ev, 6);
  t.total_ms = el(0, 6);
  t.backproject_ms = 0;                 // fused into the per-frame ICP workgroup
  t.icp_launches = det->batch.match_only ? 0 : 1;
  if (results)
    for (int i = 0; i < n_frames; ++i) t.icp_iters_total += results[i].found ? results[i].det.icp.iters : 0;
  t.scan_algorithmic_bytes = det->scan_bytes_per_frame * n_frames;
  det->have_times = false;
}

// after the last kernel that reads the batch's frames has been queued: the copy stream may reuse the buffer after it
static int input_done(fl_detector *det, int host_buf)
{
  if (host_buf < 0) return FL_OK;
  fl_context *ctx = det->ctx;
  FL_HIP(ctx, hipEventRecord(det->ev_read[host_buf], ctx->stream));
  det->read_pending[host_buf] = true;
  return FL_OK;
}

// ctx->stream names the ICP stream for the lifetime of this object: the launchers take their stream from that field
struct FlStreamScope {
  fl_context *ctx;
  hipStream_t saved;
  FlStreamScope(fl_context *c, hipStream_t s) : ctx(c), saved(c->stream) { c->stream = s; }
  ~FlStreamScope() { ctx->stream = saved; }
};

extern "C" int fl_recognize_submit(fl_detector *det, int n_frames, const uint8_t *const *bgr,
                                   const uint16_t *const *depth, int mem, const fl_intrinsics *K,
                                   const fl_recognition_params *params)
{
  const uint16_t *depth_base = nullptr;
  size_t depth_stride = 0;
  int host_buf = -1;
  bool pipelined = false;
  if (!K || !params) return FL_ERR_INVALID;
  // the batch before this one stays collectable (fl_recognize_collect_previous) if it was a fl_recognize_submit nobody collected
  const int prev_n = det && det->latest_open ? det->batch.n : 0;
  if (det) { det->prev_n = 0; det->latest_open = false; }
  int rc = stage_and_match(det, n_frames, bgr, depth, mem, K, params->matching_threshold, &depth_base, &depth_stride, &host_buf, &pipelined);
  if (rc) return rc;
  fl_context *ctx = det->ctx;
  const int hb = det->h_flip ^ 1;          // the half of h_results the batch before this one did not use
  fl_recognition_result *h_res = det->h_results + (size_t)hb * det->max_batch;
  {
    hipStream_t icp = ctx->stream;
    if (pipelined) {
      if ((rc = fl_icp_stream(ctx, &icp))) return rc;
      FL_HIP(ctx, hipStreamWaitEvent(icp, det->ev[5], 0));      // recorded behind the sort
    }
    FlStreamScope scope(ctx, icp);
    FL_HIP(ctx, hipMemsetAsync(det->d_results, 0, sizeof(fl_recognition_result) * (size_t)n_frames, ctx->stream));
    FL_HIP(ctx, hipEventRecord(det->ev[7], ctx->stream));      // icp_ms starts here: behind the wait for the ICP stage before
    det->icp_ev = 7;
    rc = fl_launch_detection(det, n_frames, K, params, depth_base, depth_stride, det->d_ws + det->off_icp, det->ws_stride, 1, nullptr,
                             det->d_results, true);
    if (rc) return rc;
    if ((rc = input_done(det, host_buf))) return rc;
    FL_HIP(ctx, hipEventRecord(det->ev[6], ctx->stream));
    FL_HIP(ctx, hipMemcpyAsync(h_res, det->d_results, sizeof(fl_recognition_result) * (size_t)n_frames, hipMemcpyDeviceToHost, ctx->stream));
    FL_HIP(ctx, hipEventRecord(det->ev_done[hb], ctx->stream));
    if (pipelined) {
      FL_HIP(ctx, hipEventRecord(det->ev_set_read[det->set], ctx->stream));
      det->set_busy[det->set] = true;
      FL_HIP(ctx, hipEventRecord(ctx->ev_icp_tail, ctx->stream));
      ctx->icp_pending = true;
    }
  }
  det->h_flip = hb;
  det->prev_n = prev_n;
  det->latest_open = true;
  return FL_OK;
}

// Detector::match (linemod.cpp:1356-1441) for a batch of frames: the reference is called once per camera frame; here
// front-end and match of n_frames frames are queued together and the sorted match lists stay in HBM until
// fl_match_batch_collect / fl_export_topk reads them.
extern "C" int fl_match_batch_submit(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth,
                                     int mem, float threshold)
{
  const uint16_t *depth_base = nullptr;
  size_t depth_stride = 0;
  int host_buf = -1;
  int rc = stage_and_match(det, n_frames, bgr, depth, mem, nullptr, threshold, &depth_base, &depth_stride, &host_buf);
  if (rc) return rc;
  if ((rc = input_done(det, host_buf))) return rc;
  FL_HIP(det->ctx, hipEventRecord(det->ev[6], det->ctx->stream));
  return FL_OK;
}

extern "C" int fl_recognize_collect(fl_detector *det, int n_frames, fl_recognition_result *results)
{
  if (!det || !results || n_frames <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || n_frames > det->batch.n) return fl_set_error(ctx, FL_ERR_STATE, "nothing submitted");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_context_sync_all(ctx)) return rc;        // the latest batch: both streams
  memcpy(results, det->h_results + (size_t)det->h_flip * det->max_batch, sizeof(fl_recognition_result) * (size_t)n_frames);
  fl_update_stage_times(det, n_frames, results);
  det->latest_open = false;
  return FL_OK;
}

// The results of the batch submitted BEFORE the latest fl_recognize_submit, while the latest is still in flight: waits for
// that batch's completion event only and leaves the stage times alone.
extern "C" int fl_recognize_collect_previous(fl_detector *det, int n_frames, fl_recognition_result *results)
{
  if (!det || !results || n_frames <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || det->prev_n < 1)
    return fl_set_error(ctx, FL_ERR_STATE, "no uncollected batch before the latest fl_recognize_submit (or another call ran in between)");
  if (n_frames > det->prev_n) return fl_set_error(ctx, FL_ERR_STATE, "%d frames asked for, the batch before the latest had %d", n_frames, det->prev_n);
  FL_HIP(ctx, hipSetDevice(ctx->device));
  const int hb = det->h_flip ^ 1;
  FL_HIP(ctx, hipEventSynchronize(det->ev_done[hb]));
  memcpy(results, det->h_results + (size_t)hb * det->max_batch, sizeof(fl_recognition_result) * (size_t)n_frames);
  det->prev_n = 0;
  return FL_OK;
}

extern "C" int fl_recognize_batch(fl_detector *det, int n_frames, const uint8_t *const *bgr,
                                  const uint16_t *const *depth, int mem, const fl_intrinsics *K,
                                  const fl_recognition_params *params, fl_recognition_result *results)
{
  // a frame with more coarse candidates than the buffers hold reports FL_ERR_OVERFLOW in its status: grow the buffers to
  // what it needs and run the batch again, so that no valid input of the reference turns into an error here
  for (int attempt = 0;; ++attempt) {
    int rc = fl_recognize_submit(det, n_frames, bgr, depth, mem, K, params);
    if (rc) return rc;
    if ((rc = fl_recognize_collect(det, n_frames, results))) return rc;
    for (int i = 0; i < n_frames; ++i)
      if (results[i].status == FL_ERR_OVERFLOW) rc = FL_ERR_OVERFLOW;
    if (!fl_grow_after_overflow(det, n_frames, attempt, &rc)) return FL_OK;   // a failed growth too: the per-frame statuses say why
  }
}

// PrepareInputData's zoom (obj_reco_lmicp.cpp:229-249: TImage2Mat(..., true) = cv::resize INTER_LINEAR of both images to
// width 640) followed by Recognition, for a batch, with the zoomed frames staying in HBM: the sw x sh sources (host or
// device) are resized on the device into a detector-owned buffer and recognised from there.
extern "C" int fl_recognize_batch_zoom(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth,
                                       int src_w, int src_h, int mem, const fl_intrinsics *K, const fl_recognition_params *params,
                                       fl_recognition_result *results)
{
  if (!det || !bgr || !depth || !K || !params || !results || n_frames <= 0 || src_w <= 0 || src_h <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (int rc = fl_check_frames(det, n_frames)) return rc;
  for (int i = 0; i < n_frames; ++i)
    if (!bgr[i] || !depth[i]) return fl_set_error(ctx, FL_ERR_INVALID, "frame %d: null pData (CheckTImage)", i);
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_pipeline_join(det)) return rc;
  fl_batch_forget(det);                  // d_zoom may hold the last batch's depth frames
  const int w = det->w0, h = det->h0;
  const size_t zb = fl_align((size_t)w * h * 3, 256), zf = zb + fl_align((size_t)w * h * 2, 256);
  if (!det->d_zoom) FL_HIP(ctx, hipMalloc((void **)&det->d_zoom, zf * (size_t)det->max_batch));
  const size_t sb = fl_align((size_t)src_w * src_h * 3, 256), sf = sb + fl_align((size_t)src_w * src_h * 2, 256);
  if (mem == FL_MEM_HOST && det->zoom_src_bytes < sf * (size_t)n_frames) {
    FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (det->d_zoom_src) (void)hipFree(det->d_zoom_src);
    det->d_zoom_src = nullptr;
    det->zoom_src_bytes = 0;
    FL_HIP(ctx, hipMalloc((void **)&det->d_zoom_src, sf * (size_t)n_frames));
    det->zoom_src_bytes = sf * (size_t)n_frames;
  }
  std::vector<const uint8_t *> zbp(n_frames);
  std::vector<const uint16_t *> zdp(n_frames);
  for (int i = 0; i < n_frames; ++i) {
    const uint8_t *sbgr = bgr[i];
    const uint16_t *sdep = depth[i];
    if (mem == FL_MEM_HOST) {
      uint8_t *d = det->d_zoom_src + sf * (size_t)i;
      FL_HIP(ctx, hipMemcpyAsync(d, bgr[i], (size_t)src_w * src_h * 3, hipMemcpyHostToDevice, ctx->stream));
      FL_HIP(ctx, hipMemcpyAsync(d + sb, depth[i], (size_t)src_w * src_h * 2, hipMemcpyHostToDevice, ctx->stream));
      sbgr = d;
      sdep = (const uint16_t *)(d + sb);
    }
    uint8_t *z = det->d_zoom + zf * (size_t)i;
    int rc = fl_launch_resize_linear_bgr8(ctx, sbgr, src_w, src_h, z, w, h);
    if (rc == FL_OK) rc = fl_launch_resize_linear_u16(ctx, sdep, src_w, src_h, (uint16_t *)(z + zb), w, h);
    if (rc) return rc;
    zbp[i] = z;
    zdp[i] = (const uint16_t *)(z + zb);
  }
  return fl_recognize_batch(det, n_frames, zbp.data(), zdp.data(), FL_MEM_DEVICE, K, params, results);
}

// The refinement half of Recognition() (obj_reco_lmicp.cpp:111-197) for matches the CALLER chose, on frames of the batch
// last queued with fl_match_batch_submit: template-sharded recognition merges the ranks' top-k lists and then asks the rank
// that owns the winning template to refine it.  matches[j].template_id is class-local on this detector.
extern "C" int fl_refine_matches(fl_detector *det, int n_jobs, const int32_t *frames, const fl_match *matches, const fl_intrinsics *K,
                                 const fl_recognition_params *params, fl_recognition_result *results)
{
  if (!det || !frames || !matches || !K || !params || !results || n_jobs <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  // the batch record has depth frames only while they are where it says (see FlBatch)
  if (!det->finalized || det->batch.n < 1 || !det->batch.depth) return fl_set_error(ctx, FL_ERR_STATE, "fl_match_batch_submit first");
  int rc = fl_check_frames(det, n_jobs);
  if (rc || (rc = fl_check_intrinsics(det, K))) return rc;
  std::vector<FlRefineJob> jobs((size_t)n_jobs);
  for (int j = 0; j < n_jobs; ++j) {
    if (frames[j] < 0 || frames[j] >= det->batch.n) return fl_set_error(ctx, FL_ERR_INVALID, "job %d: frame %d is not in the last batch", j, frames[j]);
    const fl_match &m = matches[j];
    if (m.class_idx < 0 || m.class_idx >= (int)det->classes.size() || m.template_id < 0 ||
        m.template_id >= det->classes[m.class_idx].n_pyramids)
      return fl_set_error(ctx, FL_ERR_INVALID, "job %d: template %d of class %d is not on this detector", j, m.template_id, m.class_idx);
    jobs[j].frame = frames[j];
    jobs[j].match = m;
  }
  FL_HIP(ctx, hipSetDevice(ctx->device));
  void *sv = nullptr;
  if ((rc = fl_pipeline_join(det)) || (rc = fl_scratch(ctx, sizeof(FlRefineJob) * (size_t)n_jobs, &sv))) return rc;
  FL_HIP(ctx, hipMemcpyAsync(sv, jobs.data(), sizeof(FlRefineJob) * (size_t)n_jobs, hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipMemsetAsync(det->d_results, 0, sizeof(fl_recognition_result) * (size_t)n_jobs, ctx->stream));
  det->have_times = false;
  if ((rc = fl_launch_detection(det, n_jobs, K, params, det->batch.depth, det->batch.depth_stride, det->d_ws + det->off_icp, det->ws_stride, 1,
                                (const FlRefineJob *)sv, det->d_results, false)))
    return rc;
  FL_HIP(ctx, hipMemcpyAsync(det->h_results, det->d_results, sizeof(fl_recognition_result) * (size_t)n_jobs, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));          // also covers the pageable `jobs` upload
  memcpy(results, det->h_results, sizeof(fl_recognition_result) * (size_t)n_jobs);
  return FL_OK;
}

// {found, 4x4 pose} rows of a batch of results, for the ranks' exchange (template-sharded recognition)
__global__ __launch_bounds__(64) void k_pack_pose_rows(const fl_recognition_result *__restrict__ res, int n, float *__restrict__ rows)
{
  const int f = blockIdx.x;
  if (f >= n) return;
  const int t = threadIdx.x;
  if (t == 0) rows[(size_t)f * 17] = res[f].found ? 1.0f : 0.0f;
  else if (t <= 16) rows[(size_t)f * 17 + t] = res[f].found ? res[f].pose[t - 1] : 0.0f;
}

// The device-side twin of fl_refine_matches: the jobs fl_select_best_batch left in det->d_jobs (frame = -1: not ours, the
// workgroup exits), results packed as rows for the exchange; nothing here touches the host.
extern "C" int fl_refine_selected(fl_detector *det, int n_frames, const fl_intrinsics *K, const fl_recognition_params *params,
                                  const uint16_t *depth_base, size_t depth_stride, float *dev_rows)
{
  if (!det || !K || !params || !dev_rows || n_frames <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (!det->finalized || !det->d_jobs || det->selected_frames != n_frames)
    return fl_set_error(ctx, FL_ERR_STATE, "fl_select_best_batch for these %d frames first", n_frames);
  if (int rc = fl_check_intrinsics(det, K)) return rc;
  if (!depth_base) {
    if (!det->batch.depth || n_frames > det->batch.n)
      return fl_set_error(ctx, FL_ERR_STATE, "no depth frames given and fl_match_batch_submit did not leave any");
    depth_base = det->batch.depth;
    depth_stride = det->batch.depth_stride;
  }
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_pipeline_join(det)) return rc;
  FL_HIP(ctx, hipMemsetAsync(det->d_results, 0, sizeof(fl_recognition_result) * (size_t)n_frames, ctx->stream));
  det->have_times = false;
  int rc = fl_launch_detection(det, n_frames, K, params, depth_base, depth_stride, det->d_ws + det->off_icp, det->ws_stride, 1, det->d_jobs,
                               det->d_results, false);
  if (rc) return rc;
  hipLaunchKernelGGL(k_pack_pose_rows, dim3(n_frames), dim3(64), 0, ctx->stream, det->d_results, n_frames, dev_rows);
  FL_HIP(ctx, hipGetLastError());
  det->selected_frames = 0;
  return FL_OK;
}

// Multi-hypothesis recognition of one frame + nonMaximumSuppression (ICP/NMS.cpp, obj_data.h)
static int recognize_topk_once(fl_detector *det, const uint8_t *bgr, const uint16_t *depth, int mem, const fl_intrinsics *K,
                               const fl_recognition_params *params, int k, fl_recognition_result *results, int *n_results)
{
  if (!det || !bgr || !depth || !K || !params || !results || !n_results || k < 1 || k > 1024) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  int rc = fl_check_frames(det, 1);
  if (rc) return rc;
  if (det->M != 2) return fl_set_error(ctx, FL_ERR_INVALID, "needs the colour + depth modalities");
  if ((rc = fl_check_intrinsics(det, K))) return rc;
  if ((rc = fl_pipeline_join(det))) return rc;
  fl_batch_forget(det);
  if ((rc = fl_upload_frame0(det, bgr, depth, mem))) return rc;
  det->have_times = false;
  const uint16_t *d_depth = (const uint16_t *)(det->d_ws + det->off_depth);
  if ((rc = fl_launch_frontend(det, 1, det->d_ws + det->off_bgr, det->ws_stride, d_depth, det->ws_stride, true))) return rc;
  if ((rc = fl_launch_match_core(det, 1, params->matching_threshold))) return rc;
  fl_batch_record(det, 1, nullptr, 0, false);   // the frame lives in workspace 0 only until the next call: not a batch to refine later
  const size_t icp_bytes = fl_align(fl_icp_ws_bytes(det->n_pts_max), 256) * (size_t)k, res_bytes = sizeof(fl_recognition_result) * (size_t)k;
  void *sv = nullptr;
  if ((rc = fl_scratch(ctx, icp_bytes + fl_align(res_bytes, 256), &sv))) return rc;
  fl_recognition_result *d_res = (fl_recognition_result *)((uint8_t *)sv + icp_bytes);
  FL_HIP(ctx, hipMemsetAsync(d_res, 0, res_bytes, ctx->stream));
  if ((rc = fl_launch_detection(det, k, K, params, d_depth, 0, (uint8_t *)sv, fl_icp_ws_bytes(det->n_pts_max), k, nullptr, d_res, false)))
    return rc;
  FL_HIP(ctx, hipMemcpyAsync(results, d_res, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (results[0].status == FL_ERR_OVERFLOW) return fl_set_error(ctx, FL_ERR_OVERFLOW, "more than %d candidates in the frame", det->cap);
  const int n = results[0].n_matches < k ? results[0].n_matches : k;
  *n_results = n < 0 ? 0 : n;
  return FL_OK;
}

extern "C" int fl_recognize_topk(fl_detector *det, const uint8_t *bgr, const uint16_t *depth, int mem, const fl_intrinsics *K,
                                 const fl_recognition_params *params, int k, fl_recognition_result *results, int *n_results)
{
  for (int attempt = 0;; ++attempt) {
    int rc = recognize_topk_once(det, bgr, depth, mem, K, params, k, results, n_results);
    if (!fl_grow_after_overflow(det, 1, attempt, &rc)) return rc;
  }
}

// The same for a whole batch: n_frames * k ICP workgroups in one launch.  results[f * k + r] is hypothesis r of frame f,
// n_results[f] = min(k, matches of frame f).
static int recognize_batch_topk_once(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth,
                                     int mem, const fl_intrinsics *K, const fl_recognition_params *params, int k,
                                     fl_recognition_result *results, int *n_results)
{
  if (!results || !n_results || k < 1 || k > 1024) return FL_ERR_INVALID;
  if (det && det->M != 2) return fl_set_error(det->ctx, FL_ERR_INVALID, "needs the colour + depth modalities");
  const uint16_t *depth_base = nullptr;
  size_t depth_stride = 0;
  int host_buf = -1;
  if (!K || !params) return FL_ERR_INVALID;
  int rc = stage_and_match(det, n_frames, bgr, depth, mem, K, params->matching_threshold, &depth_base, &depth_stride, &host_buf);
  if (rc) return rc;
  fl_context *ctx = det->ctx;
  det->have_times = false;
  const size_t jobs = (size_t)n_frames * k, ws_one = fl_align(fl_icp_ws_bytes(det->n_pts_max), 256);
  const size_t icp_bytes = ws_one * jobs, res_bytes = sizeof(fl_recognition_result) * jobs;
  if (jobs > (1u << 20) || icp_bytes > ((size_t)96 << 30))
    return fl_set_error(ctx, FL_ERR_INVALID, "%d frames x %d hypotheses need %zu MB of ICP workspaces", n_frames, k, icp_bytes >> 20);
  void *sv = nullptr;
  if ((rc = fl_scratch(ctx, icp_bytes + fl_align(res_bytes, 256), &sv))) return rc;
  fl_recognition_result *d_res = (fl_recognition_result *)((uint8_t *)sv + icp_bytes);
  FL_HIP(ctx, hipMemsetAsync(d_res, 0, res_bytes, ctx->stream));
  if ((rc = fl_launch_detection(det, n_frames * k, K, params, depth_base, depth_stride, (uint8_t *)sv, fl_icp_ws_bytes(det->n_pts_max), k,
                                nullptr, d_res, false)))
    return rc;
  if ((rc = input_done(det, host_buf))) return rc;
  FL_HIP(ctx, hipMemcpyAsync(results, d_res, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int f = 0; f < n_frames; ++f) {
    const fl_recognition_result &r0 = results[(size_t)f * k];
    if (r0.status == FL_ERR_OVERFLOW) return fl_set_error(ctx, FL_ERR_OVERFLOW, "frame %d: more than %d candidates", f, det->cap);
    const int n = r0.n_matches < k ? r0.n_matches : k;
    n_results[f] = n < 0 ? 0 : n;
  }
  return FL_OK;
}

extern "C" int fl_recognize_batch_topk(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth,
                                       int mem, const fl_intrinsics *K, const fl_recognition_params *params, int k,
                                       fl_recognition_result *results, int *n_results)
{
  for (int attempt = 0;; ++attempt) {
    int rc = recognize_batch_topk_once(det, n_frames, bgr, depth, mem, K, params, k, results, n_results);
    if (!fl_grow_after_overflow(det, n_frames, attempt, &rc)) return rc;
  }
}

// ---- multi-instance recognition (include/fealess_hip.h): match -> group -> one ICP launch -> pick, all on the device ----
// What the pick kernel leaves for the one copy to the host: results[n_frames * G], then n_instances, n_dropped and status
// (FL_ERR_OVERFLOW: the frame's candidate buffers overflowed and nothing was grouped), n_frames ints each.
static size_t instances_out_bytes(int n_frames, int G) { return sizeof(fl_instance_result) * (size_t)n_frames * G + sizeof(int32_t) * 3 * (size_t)n_frames; }

// One thread per (frame, group): nonMaximumSuppression's choice among the group's refined members (see the header).
__global__ __launch_bounds__(64) void k_pick_instances(const fl_recognition_result *__restrict__ res, const int32_t *__restrict__ job_idx,
                                                       const int32_t *__restrict__ group_size, const int32_t *__restrict__ info, int n_frames,
                                                       int G, int h, fl_instance_result *__restrict__ out)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_frames * G) return;
  const int f = t / G, g = t - f * G;
  const int32_t *fi = info + 4 * (size_t)f;
  if (g == 0) {
    int32_t *tail = (int32_t *)(out + (size_t)n_frames * G);
    tail[f] = fi[0];
    tail[n_frames + f] = fi[1];
    tail[2 * n_frames + f] = fi[2];
  }
  if (g >= fi[0]) return;                                  // the slot stays zeroed
  const size_t first = (size_t)t * h;
  int o = -1, size_th = 0, n_refined = 0;
  for (int r = 0; r < h && job_idx[first + r] >= 0; ++r) {
    ++n_refined;
    const fl_recognition_result &c = res[first + r];
    if (!c.found) continue;
    if (o < 0) { o = r; size_th = (int)((double)(float)c.det.n_points * 0.85); }     // NMS.cpp:13, the double product fl_nms takes
    else if (c.det.n_points > size_th && c.det.icp.dist_mean < res[first + o].det.icp.dist_mean) o = r;
  }
  if (o < 0) o = 0;                                        // no member was found: the leader, found = 0
  fl_instance_result v;
  v.reco = res[first + o];
  v.reco.n_matches = fi[3];
  v.rank = job_idx[first + o];
  v.n_members = group_size[t];
  v.n_refined = n_refined;
  v.reserved = 0;
  out[t] = v;
}

// The verified pick (fl_recognize_batch_instances_verified, see the header), one thread per (frame, group).  vres: the finished
// record of every job slot, best = accepted as k_verify_finish leaves it; a verified group's `best` fields are rewritten here.
// The group's class is its leader's, which every member shares (the grouping rule); mesh_of_class maps it to the mesh the
// group is verified against, negative: not verified.
__global__ __launch_bounds__(64) void k_pick_verified(const fl_recognition_result *__restrict__ res, const FlRefineJob *__restrict__ jobs,
                                                      const int32_t *__restrict__ job_idx, const int32_t *__restrict__ group_size,
                                                      const int32_t *__restrict__ info, int n_frames, int G, int h,
                                                      const int32_t *__restrict__ mesh_of_class, fl_verify_result *vres, fl_verified_instance_result *__restrict__ out)
{
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_frames * G) return;
  const int f = t / G, g = t - f * G;
  const int32_t *fi = info + 4 * (size_t)f;
  if (g == 0) {
    int32_t *tail = (int32_t *)(out + (size_t)n_frames * G);
    tail[f] = fi[0];
    tail[n_frames + f] = fi[1];
    tail[2 * n_frames + f] = fi[2];
  }
  if (g >= fi[0]) return;                                  // the slot stays zeroed
  const size_t first = (size_t)t * h;
  int o = -1, size_th = 0, n_refined = 0;                  // k_pick_instances' pick
  for (int r = 0; r < h && job_idx[first + r] >= 0; ++r) {
    ++n_refined;
    const fl_recognition_result &c = res[first + r];
    if (!c.found) continue;
    if (o < 0) { o = r; size_th = (int)((double)(float)c.det.n_points * 0.85); }
    else if (c.det.n_points > size_th && c.det.icp.dist_mean < res[first + o].det.icp.dist_mean) o = r;
  }
  if (o < 0) o = 0;
  const int verified = mesh_of_class[jobs[first].match.class_idx] >= 0;
  int pick = o, best = -1;
  if (verified) {
    long long bi = 0, bm = 1;
    for (int r = 0; r < n_refined; ++r) {
      const fl_verify_result &v = vres[first + r];
      if (!res[first + r].found || !v.accepted) continue;  // accepted: n_model >= min_model_px >= 1
      if (best < 0 || (long long)v.n_inlier * bm > bi * (long long)v.n_model) { best = r; bi = v.n_inlier; bm = v.n_model; }
    }
    for (int r = 0; r < n_refined; ++r) vres[first + r].best = r == best;
    if (best >= 0) pick = best;
  }
  fl_verified_instance_result v;
  v.inst.reco = res[first + pick];
  v.inst.reco.n_matches = fi[3];
  v.inst.rank = job_idx[first + pick];
  v.inst.n_members = group_size[t];
  v.inst.n_refined = n_refined;
  v.inst.reserved = 0;
  if (verified) v.verify = vres[first + pick];
  else memset(&v.verify, 0, sizeof(v.verify));
  v.nms_rank = job_idx[first + o];
  v.verified = verified;
  v.reserved[0] = 0; v.reserved[1] = 0;
  out[t] = v;
}

// What fl_recognize_batch_instances_verified adds to the call below (null: fl_recognize_batch_instances as it always was).
struct InstVerify {
  fl_tracker *mesh;
  const fl_instance_verify_params *vp;
  fl_verified_instance_result *results;
  fl_verify_result *member_verify;                         // may be null
  bool by_map;                                             // fl_recognize_batch_instances_verified_meshes: mesh_of_class, not vp->class_idx
  const int32_t *mesh_of_class;                            // host, one entry per class of the detector
};

static int recognize_batch_instances_once(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth, int mem,
                                          const fl_intrinsics *K, const fl_recognition_params *params, const fl_instance_params *ip,
                                          fl_instance_result *results, int32_t *n_instances, int32_t *n_dropped, const InstVerify *v = nullptr)
{
  if (!det || !bgr || n_frames <= 0 || !K || !params || !ip || !(v ? (void *)v->results : (void *)results) || !n_instances || !n_dropped)
    return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (det->M != 2) return fl_set_error(ctx, FL_ERR_INVALID, "needs the colour + depth modalities");
  if (!fl_instance_params_ok(ip)) return fl_set_error(ctx, FL_ERR_INVALID, FL_INSTANCE_PARAMS_TEXT);
  float kf[4] = {0.f, 0.f, 0.f, 0.f};                       // the scene camera as floats, which is what the rasteriser gets
  if (v) {                                                 // refusals that need no device, and so no finalized detector either
    const char *who = "fl_recognize_batch_instances_verified";
    if (!v->mesh || !v->vp) return fl_set_error(ctx, FL_ERR_INVALID, "%s: null tracker or fl_instance_verify_params", who);
    if (!fl_verify_params_ok(v->vp->verify)) return fl_set_error(ctx, FL_ERR_INVALID, FL_VERIFY_PARAMS_TEXT);
    kf[0] = (float)K->fx; kf[1] = (float)K->fy; kf[2] = (float)K->cx; kf[3] = (float)K->cy;
    if (!(std::isfinite(kf[0]) && kf[0] > 0.f && std::isfinite(kf[1]) && kf[1] > 0.f && std::isfinite(kf[2]) && std::isfinite(kf[3])))
      return fl_set_error(ctx, FL_ERR_INVALID, "%s: fx, fy must be finite and > 0, cx, cy finite, as floats too", who);
    if (v->by_map) {
      if (!v->mesh_of_class) return fl_set_error(ctx, FL_ERR_INVALID, "%s_meshes: null mesh_of_class", who);
      if (v->vp->class_idx != -1)
        return fl_set_error(ctx, FL_ERR_INVALID, "%s_meshes: class_idx %d must be -1, the map says which classes are verified", who, v->vp->class_idx);
      for (int c = 0; c < (int)det->classes.size(); ++c)
        if (v->mesh_of_class[c] < -1 || v->mesh_of_class[c] >= v->mesh->n_meshes)
          return fl_set_error(ctx, FL_ERR_INVALID, "%s_meshes: mesh_of_class[%d] = %d outside [-1, %d)", who, c, v->mesh_of_class[c], v->mesh->n_meshes);
    } else if (v->vp->class_idx < -1 || v->vp->class_idx >= (int)det->classes.size()) {
      return fl_set_error(ctx, FL_ERR_INVALID, "%s: class_idx %d outside [-1, %d)", who, v->vp->class_idx, (int)det->classes.size());
    }
    if (v->mesh->ctx != ctx) return fl_set_error(ctx, FL_ERR_INVALID, "%s: the tracker is on another context", who);
    if (v->mesh->w != det->w0 || v->mesh->h != det->h0 || v->mesh->w != K->width || v->mesh->h != K->height)
      return fl_set_error(ctx, FL_ERR_INVALID, "%s: the tracker's %d x %d is not the detector's %d x %d or not K's %d x %d", who, v->mesh->w,
                          v->mesh->h, det->w0, det->h0, K->width, K->height);
  }
  int rc = fl_check_frames(det, n_frames);
  if (rc) return rc;
  // Everything that can refuse or fail without the batch comes BEFORE the batch is queued: a return between stage_and_match
  // and input_done would leave the input buffer's read event unrecorded.
  const int G = ip->max_instances, h = ip->hyp_per_instance;
  const size_t jobs = (size_t)n_frames * G * h, ws_one = fl_align(fl_icp_ws_bytes(det->n_pts_max), 256);
  // the verified variant's output block: its results, the same three ints per frame, then (8-aligned) every slot's record
  const size_t vout_bytes = fl_align(sizeof(fl_verified_instance_result) * (size_t)n_frames * G + sizeof(int32_t) * 3 * (size_t)n_frames, 8);
  const size_t icp_bytes = ws_one * jobs, out_bytes = v ? vout_bytes + sizeof(fl_verify_result) * jobs : instances_out_bytes(n_frames, G);
  const size_t copy_bytes = v && !v->member_verify ? vout_bytes : out_bytes;
  if (jobs > (1u << 20) || icp_bytes > ((size_t)96 << 30))
    return fl_set_error(ctx, FL_ERR_INVALID, "%d frames x %d instances x %d hypotheses need %zu MB of ICP workspaces", n_frames, G, h, icp_bytes >> 20);
  // one scratch block: ICP workspaces, their results, the job list and its list indices, sizes, counters, output -- and the
  // group ids only where the kernel needs them as working storage (lists longer than FL_GROUP_LDS_MAX)
  const bool need_gof = det->cap > FL_GROUP_LDS_MAX;
  size_t off = icp_bytes;
  auto take = [&](size_t bytes) { const size_t o = off; off = fl_align(off + bytes, 256); return o; };
  const size_t o_res = take(sizeof(fl_recognition_result) * jobs), o_jobs = take(sizeof(FlRefineJob) * jobs), o_idx = take(sizeof(int32_t) * jobs);
  const size_t o_gof = take(need_gof ? sizeof(int32_t) * (size_t)det->cap * n_frames : 0), o_size = take(sizeof(int32_t) * (size_t)n_frames * G);
  const size_t o_info = take(sizeof(int32_t) * 4 * (size_t)n_frames), o_out = take(out_bytes);
  const size_t o_acc = take(v ? FL_VERIFY_ACC_BYTES * jobs : 0);
  // the verified variant's map from classes to meshes: behind the records in the pinned block, and from there into the scratch
  const size_t map_bytes = v ? sizeof(int32_t) * det->classes.size() : 0, h_map = fl_align(copy_bytes, 256), o_map = take(map_bytes);
  void *sv = nullptr, *hv = nullptr;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if ((rc = fl_scratch(ctx, off, &sv)) || (rc = fl_pinned(ctx, v ? h_map + map_bytes : copy_bytes, &hv))) return rc;
  uint8_t *s = (uint8_t *)sv;
  if (v) {                                                 // without a map: class_idx -> mesh 0, every other class -> none; -1: every class -> mesh 0
    int32_t *hm = (int32_t *)((uint8_t *)hv + h_map);
    for (int c = 0; c < (int)det->classes.size(); ++c)
      hm[c] = v->by_map ? v->mesh_of_class[c] : (v->vp->class_idx < 0 || v->vp->class_idx == c ? 0 : -1);
    FL_HIP(ctx, hipMemcpyAsync(s + o_map, hm, map_bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  const uint16_t *depth_base = nullptr;
  size_t depth_stride = 0;
  int host_buf = -1;
  if ((rc = stage_and_match(det, n_frames, bgr, depth, mem, K, params->matching_threshold, &depth_base, &depth_stride, &host_buf))) return rc;
  fl_recognition_result *d_res = (fl_recognition_result *)(s + o_res);
  FL_HIP(ctx, hipMemsetAsync(d_res, 0, sizeof(fl_recognition_result) * jobs, ctx->stream));
  FL_HIP(ctx, hipMemsetAsync(s + o_out, 0, out_bytes, ctx->stream));
  if (v) FL_HIP(ctx, hipMemsetAsync(s + o_acc, 0, FL_VERIFY_ACC_BYTES * jobs, ctx->stream));   // a slot that is not live keeps zeros
  FL_HIP(ctx, hipEventRecord(det->ev[16], ctx->stream));
  FlGroupArgs a = fl_group_args(det, ip);
  a.n = det->cap;
  a.frame_ws = det->d_ws;
  a.frame_stride = det->ws_stride;
  a.off_count = det->off_count;
  a.off_match = det->off_match;
  a.group_of = need_gof ? (int32_t *)(s + o_gof) : nullptr;
  a.group_of_stride = need_gof ? (size_t)det->cap : 0;
  a.group_size = (int32_t *)(s + o_size);
  a.info = (int32_t *)(s + o_info);
  a.jobs = (FlRefineJob *)(s + o_jobs);
  a.job_idx = (int32_t *)(s + o_idx);
  if ((rc = fl_launch_group_matches(det, n_frames, a))) return rc;
  FL_HIP(ctx, hipEventRecord(det->ev[17], ctx->stream));
  if ((rc = fl_launch_detection(det, (int)jobs, K, params, depth_base, depth_stride, s, ws_one, 1, a.jobs, d_res, false))) return rc;
  if (!v && (rc = input_done(det, host_buf))) return rc;   // the verification reads the frames too
  FL_HIP(ctx, hipEventRecord(det->ev[18], ctx->stream));
  if (v) {
    // every live slot rendered and scored where its pose and its frame lie, the records, then the pick
    fl_verify_result *d_vres = (fl_verify_result *)(s + o_out + vout_bytes);
    const fl_tracker *m = v->mesh;
    const FlVerifyFusedJob j = {(int)jobs, m->w, m->h, v->vp->verify.tau_mm, kf[0], kf[1], kf[2], kf[3], {m->d_vtx, nullptr, nullptr, m->d_tri, m->n_t},
                                d_res->pose, (int)(sizeof(fl_recognition_result) / sizeof(float)), (const uint8_t *)depth_base, depth_stride, nullptr,
                                G * h, a.job_idx, d_res, (const int32_t *)(s + o_map), s + o_acc, nullptr, 0, nullptr,
                                m->n_meshes > 1 ? m->d_ranges : nullptr};
    if ((rc = fl_launch_verify_fused(ctx, j))) { (void)input_done(det, host_buf); return rc; }   // the frames' last reader, queued or not
    if ((rc = input_done(det, host_buf))) return rc;
    FL_HIP(ctx, hipEventRecord(det->ev[19], ctx->stream));
    if ((rc = fl_launch_verify_finish(ctx, (int)jobs, m->w, m->h, v->vp->verify, s + o_acc, d_vres))) return rc;
    hipLaunchKernelGGL(k_pick_verified, dim3((n_frames * G + 63) / 64), dim3(64), 0, ctx->stream, d_res, a.jobs, a.job_idx, a.group_size, a.info, n_frames,
                       G, h, (const int32_t *)(s + o_map), d_vres, (fl_verified_instance_result *)(s + o_out));
  } else {
    hipLaunchKernelGGL(k_pick_instances, dim3((n_frames * G + 63) / 64), dim3(64), 0, ctx->stream, d_res, a.job_idx, a.group_size, a.info, n_frames, G, h,
                       (fl_instance_result *)(s + o_out));
  }
  FL_HIP(ctx, hipGetLastError());
  FL_HIP(ctx, hipEventRecord(det->ev[6], ctx->stream));
  FL_HIP(ctx, hipMemcpyAsync(hv, s + o_out, copy_bytes, hipMemcpyDeviceToHost, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  det->verify_timed = v != nullptr;
  const size_t res_size = v ? sizeof(fl_verified_instance_result) : sizeof(fl_instance_result);
  const int32_t *tail = (const int32_t *)((const uint8_t *)hv + res_size * (size_t)n_frames * G);
  for (int f = 0; f < n_frames; ++f)
    if (tail[2 * n_frames + f] == FL_ERR_OVERFLOW) return fl_set_error(ctx, FL_ERR_OVERFLOW, "frame %d: more than %d candidates", f, det->cap);
  if (v) {
    memcpy(v->results, hv, res_size * (size_t)n_frames * G);
    if (v->member_verify) memcpy(v->member_verify, (const uint8_t *)hv + vout_bytes, sizeof(fl_verify_result) * jobs);
  } else {
    memcpy(results, hv, res_size * (size_t)n_frames * G);
  }
  memcpy(n_instances, tail, sizeof(int32_t) * (size_t)n_frames);
  memcpy(n_dropped, tail + n_frames, sizeof(int32_t) * (size_t)n_frames);
  // stage times: the ICP stage of this call is grouping + ICP + pick; group_ms is the two new kernels' part of it
  fl_update_stage_times(det, n_frames, nullptr);
  float ms = 0;
  if (hipEventElapsedTime(&ms, det->ev[16], det->ev[17]) == hipSuccess) det->times.group_ms = ms;
  if (hipEventElapsedTime(&ms, det->ev[18], det->ev[6]) == hipSuccess) det->times.group_ms += ms;
  for (int f = 0; f < n_frames; ++f)
    for (int g = 0; g < n_instances[f]; ++g) {
      const fl_recognition_result &r = v ? v->results[(size_t)f * G + g].inst.reco : results[(size_t)f * G + g].reco;
      det->times.icp_iters_total += r.found ? r.det.icp.iters : 0;        // of the picked hypotheses
    }
  return FL_OK;
}

extern "C" int fl_recognize_batch_instances(fl_detector *det, int n_frames, const uint8_t *const *bgr, const uint16_t *const *depth,
                                            int mem, const fl_intrinsics *K, const fl_recognition_params *params,
                                            const fl_instance_params *ip, fl_instance_result *results, int32_t *n_instances,
                                            int32_t *n_dropped)
{
  for (int attempt = 0;; ++attempt) {
    int rc = recognize_batch_instances_once(det, n_frames, bgr, depth, mem, K, params, ip, results, n_instances, n_dropped);
    if (!fl_grow_after_overflow(det, n_frames, attempt, &rc)) return rc;
  }
}

extern "C" int fl_recognize_batch_instances_verified(fl_detector *det, fl_tracker *mesh, int n_frames, const uint8_t *const *bgr,
                                                     const uint16_t *const *depth, int mem, const fl_intrinsics *K,
                                                     const fl_recognition_params *params, const fl_instance_params *ip,
                                                     const fl_instance_verify_params *vp, fl_verified_instance_result *results,
                                                     int32_t *n_instances, int32_t *n_dropped, fl_verify_result *member_verify)
{
  const InstVerify v = {mesh, vp, results, member_verify, false, nullptr};
  for (int attempt = 0;; ++attempt) {
    int rc = recognize_batch_instances_once(det, n_frames, bgr, depth, mem, K, params, ip, nullptr, n_instances, n_dropped, &v);
    if (!fl_grow_after_overflow(det, n_frames, attempt, &rc)) return rc;
  }
}

extern "C" int fl_recognize_batch_instances_verified_meshes(fl_detector *det, fl_tracker *mesh, int n_frames, const uint8_t *const *bgr,
                                                            const uint16_t *const *depth, int mem, const fl_intrinsics *K,
                                                            const fl_recognition_params *params, const fl_instance_params *ip,
                                                            const fl_instance_verify_params *vp, const int32_t *mesh_of_class,
                                                            fl_verified_instance_result *results, int32_t *n_instances, int32_t *n_dropped,
                                                            fl_verify_result *member_verify)
{
  const InstVerify v = {mesh, vp, results, member_verify, true, mesh_of_class};
  for (int attempt = 0;; ++attempt) {
    int rc = recognize_batch_instances_once(det, n_frames, bgr, depth, mem, K, params, ip, nullptr, n_instances, n_dropped, &v);
    if (!fl_grow_after_overflow(det, n_frames, attempt, &rc)) return rc;
  }
}

// device time of the verification stage of the last fl_recognize_batch_instances_verified: {fused verify, finish + pick} in ms
extern "C" int fl_dev_instances_verify_ms(fl_detector *det, float out[2])
{
  if (!det || !out || !det->verify_timed) return FL_ERR_INVALID;
  if (hipEventElapsedTime(out, det->ev[18], det->ev[19]) != hipSuccess || hipEventElapsedTime(out + 1, det->ev[19], det->ev[6]) != hipSuccess)
    return FL_ERR_HIP;
  return FL_OK;
}

// k_pick_verified on caller-supplied records: n_groups groups of h slots each, laid out as one frame of n_groups groups.  Host
// arrays: res and jobs and job_idx and vres have n_groups * h entries (vres is read and written back: the `best` fields),
// group_size n_groups; out n_groups records.  Every group counts as present.
extern "C" int fl_dev_pick_verified(fl_context *ctx, int n_groups, int h, int class_idx, const fl_recognition_result *res, const FlRefineJob *jobs,
                                    const int32_t *job_idx, const int32_t *group_size, fl_verify_result *vres, fl_verified_instance_result *out)
{
  if (!ctx || n_groups < 1 || n_groups > (1 << 20) || h < 1 || h > FL_GROUP_HYP_MAX || !res || !jobs || !job_idx || !group_size || !vres || !out)
    return FL_ERR_INVALID;
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_NO_DEVICE, "fl_dev_pick_verified: no device");
  const size_t n = (size_t)n_groups * h;
  // the kernel's map from classes to meshes, as the entry point builds it from class_idx, over the classes the leaders name
  int n_cls = 1;
  for (int g = 0; g < n_groups; ++g) {
    const int c = jobs[(size_t)g * h].match.class_idx;
    if (c < 0 || c >= (1 << 20)) return fl_set_error(ctx, FL_ERR_INVALID, "fl_dev_pick_verified: group %d has class %d", g, c);
    n_cls = std::max(n_cls, c + 1);
  }
  std::vector<int32_t> map((size_t)n_cls);
  for (int c = 0; c < n_cls; ++c) map[c] = class_idx < 0 || class_idx == c ? 0 : -1;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = fl_align(off + bytes, 256); return o; };
  const size_t o_res = take(sizeof(*res) * n), o_jobs = take(sizeof(*jobs) * n), o_idx = take(4 * n), o_size = take(4 * (size_t)n_groups), o_info = take(16);
  const size_t o_vres = take(sizeof(*vres) * n), o_out = take(sizeof(*out) * (size_t)n_groups + 12), o_map = take(4 * (size_t)n_cls);
  void *sv = nullptr;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  int rc = fl_context_join(ctx);
  if (rc || (rc = fl_scratch(ctx, off, &sv))) return rc;
  uint8_t *s = (uint8_t *)sv;
  const int32_t info[4] = {n_groups, 0, 0, 0};
  hipStream_t st = ctx->stream;
  FL_HIP(ctx, hipMemcpyAsync(s + o_res, res, sizeof(*res) * n, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(s + o_jobs, jobs, sizeof(*jobs) * n, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(s + o_idx, job_idx, 4 * n, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(s + o_size, group_size, 4 * (size_t)n_groups, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(s + o_info, info, 16, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(s + o_vres, vres, sizeof(*vres) * n, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipMemcpyAsync(s + o_map, map.data(), 4 * (size_t)n_cls, hipMemcpyHostToDevice, st));
  FL_HIP(ctx, hipStreamSynchronize(st));                   // info is on the stack, and the caller's arrays are pageable
  hipLaunchKernelGGL(k_pick_verified, dim3((n_groups + 63) / 64), dim3(64), 0, st, (const fl_recognition_result *)(s + o_res),
                     (const FlRefineJob *)(s + o_jobs), (const int32_t *)(s + o_idx), (const int32_t *)(s + o_size), (const int32_t *)(s + o_info), 1,
                     n_groups, h, (const int32_t *)(s + o_map), (fl_verify_result *)(s + o_vres), (fl_verified_instance_result *)(s + o_out));
  FL_HIP(ctx, hipGetLastError());
  FL_HIP(ctx, hipMemcpyAsync(vres, s + o_vres, sizeof(*vres) * n, hipMemcpyDeviceToHost, st));
  FL_HIP(ctx, hipMemcpyAsync(out, s + o_out, sizeof(*out) * (size_t)n_groups, hipMemcpyDeviceToHost, st));
  FL_HIP(ctx, hipStreamSynchronize(st));
  return FL_OK;
}

// nonMaximumSuppression (ICP/NMS.cpp:6-40) over refined hypotheses, in list order.  winners[g] = index of the
// hypothesis that represents group g; returns the number of groups in *n_winners.  Host-only arithmetic.
extern "C" int fl_nms(const fl_recognition_result *objs, int n, float th_obj_dist, int *winners, int *n_winners)
{
  if ((n > 0 && !objs) || !winners || !n_winners || n < 0) return FL_ERR_INVALID;
  std::vector<char> done((size_t)(n > 0 ? n : 1), 0);
  int n_out = 0;
  for (int i = 0; i < n; ++i) {
    if (done[i]) continue;
    int o = i;
    const int size_th = static_cast<int>((float)objs[i].det.n_points * 0.85);
    for (int j = i + 1; j < n; ++j) {
      if (done[j]) continue;
      double s = 0;
      for (int c = 0; c < 3; ++c) { const double d = (double)objs[o].det.T_final[c] - (double)objs[j].det.T_final[c]; s += d * d; }
      if (std::sqrt(s) < th_obj_dist) {
        done[j] = 1;
        if (objs[j].det.n_points > size_th && objs[j].det.icp.dist_mean < objs[o].det.icp.dist_mean) o = j;
      }
    }
    winners[n_out++] = o;
  }
  *n_winners = n_out;
  return FL_OK;
}

extern "C" int fl_last_stage_times(fl_detector *det, fl_stage_times *out)
{
  if (!det || !out) return FL_ERR_INVALID;
  *out = det->times;
  return FL_OK;
}
