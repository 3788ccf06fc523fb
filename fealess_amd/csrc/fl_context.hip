// fl_context.hip -- context, detector construction and HBM layout of libfealess_hip.so.
//
// Replaces (reference paths): cup_linemod::Detector construction / addSyntheticTemplate /
// addPoseInfo (linemod/linemod.cpp:1348-1354, 1617-1642) and the per-frame disk read of the
// template depth render (CadReco/obj_reco_lmicp.cpp:156-157, uploaded once here instead).
#include "fl_internal.h"
#include <stdlib.h>
#include <stdarg.h>
#include <string.h>
#include <algorithm>

int fl_set_error(fl_context *ctx, int code, const char *fmt, ...)
{
  if (ctx) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof(ctx->err), fmt, ap);
    va_end(ap);
  }
  return code;
}

// (the single-shot entry points all come through here or fl_pinned before they queue work: ctx->stream first waits for
// whatever a pipelined fl_recognize_submit left on the ICP stream)
int fl_scratch(fl_context *ctx, size_t bytes, void **out)
{
  if (int rc = fl_context_join(ctx)) return rc;
  if (bytes > ctx->scratch_bytes) {
    if (ctx->scratch) {
      FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
      FL_HIP(ctx, hipFree(ctx->scratch));
      ctx->scratch = nullptr;
      ctx->scratch_bytes = 0;
    }
    size_t nb = fl_align(bytes + bytes / 4, 1 << 20);
    FL_HIP(ctx, hipMalloc(&ctx->scratch, nb));
    ctx->scratch_bytes = nb;
  }
  *out = ctx->scratch;
  return FL_OK;
}

int fl_pinned(fl_context *ctx, size_t bytes, void **out)
{
  if (int rc = fl_context_join(ctx)) return rc;
  if (bytes > ctx->pinned_bytes) {
    if (ctx->pinned) {
      FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
      FL_HIP(ctx, hipHostFree(ctx->pinned));
      ctx->pinned = nullptr;
      ctx->pinned_bytes = 0;
    }
    size_t nb = fl_align(bytes, 1 << 16);
    FL_HIP(ctx, hipHostMalloc(&ctx->pinned, nb, hipHostMallocDefault));
    ctx->pinned_bytes = nb;
  }
  *out = ctx->pinned;
  return FL_OK;
}

int fl_context_join(fl_context *ctx)
{
  if (!ctx->icp_pending) return FL_OK;
  ctx->icp_pending = false;
  FL_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_icp_tail, 0));
  return FL_OK;
}

int fl_context_sync_all(fl_context *ctx)
{
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (ctx->icp_stream) FL_HIP(ctx, hipStreamSynchronize(ctx->icp_stream));
  ctx->icp_pending = false;
  return FL_OK;
}

// pipeline_icp 1: the ICP stream at the default priority; 2 / 3: at the highest / lowest the device offers.  A stream keeps
// the priority it was created with, so a changed option value replaces the stream once its work has finished.
int fl_icp_stream(fl_context *ctx, hipStream_t *out)
{
  const long mode = ctx->opt.pipeline_icp;
  if (ctx->icp_stream && ctx->icp_stream_mode != mode) {
    FL_HIP(ctx, hipStreamSynchronize(ctx->icp_stream));
    FL_HIP(ctx, hipStreamDestroy(ctx->icp_stream));
    ctx->icp_stream = nullptr;
  }
  if (!ctx->icp_stream) {
    int least = 0, greatest = 0;
    FL_HIP(ctx, hipDeviceGetStreamPriorityRange(&least, &greatest));
    FL_HIP(ctx, hipStreamCreateWithPriority(&ctx->icp_stream, hipStreamNonBlocking, mode == 2 ? greatest : (mode == 3 ? least : 0)));
    ctx->icp_stream_mode = mode;
  }
  if (!ctx->ev_icp_tail) FL_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_icp_tail, hipEventDisableTiming));
  *out = ctx->icp_stream;
  return FL_OK;
}

extern "C" int fl_abi_version(void) { return FL_ABI_VERSION; }

// name, environment variable, field, environment value in hex, accepted values lo .. hi (icp_occ: 0, 4 or 5;
// frontend_chunk_rows: multiples of 60; scan_run: 0 = automatic; scan_prune_step: 0 = automatic, 2, 4 or 8;
// scan_first: 0 = automatic, 8, 12, 14 or 16)
struct FlOptionName { const char *name, *env; long fl_context::Options::*field; bool hex; long lo, hi; };
static const FlOptionName fl_option_names[] = {
  {"scan_prune", "FL_SCAN_PRUNE", &fl_context::Options::scan_prune, false, 0, 1},
  {"scan_prune_mid", "FL_SCAN_PRUNE_MID", &fl_context::Options::scan_prune_mid, true, -1, 0xFF},
  {"scan_prune_lanes", "FL_SCAN_PRUNE_LANES", &fl_context::Options::scan_prune_lanes, false, 0, 1},
  {"scan_prune_step", "FL_SCAN_PRUNE_STEP", &fl_context::Options::scan_prune_step, false, 0, 8},
  {"scan_first", "FL_SCAN_FIRST", &fl_context::Options::scan_first, false, 0, 16},
  {"icp_wide", "FL_ICP_WIDE", &fl_context::Options::icp_wide, false, -1, 1},
  {"icp_occ", "FL_ICP_OCC", &fl_context::Options::icp_occ, false, 0, 5},
  {"icp_idx16", "FL_ICP_IDX16", &fl_context::Options::icp_idx16, false, -1, 1},
  {"icp_order", "FL_ICP_ORDER", &fl_context::Options::icp_order, false, 0, 1},
  {"icp_wg_per_cu", "FL_ICP_WG_PER_CU", &fl_context::Options::icp_wg_per_cu, false, 0, 3},
  {"eager_frontend", "FL_EAGER_FRONTEND", &fl_context::Options::eager_frontend, false, 0, 1},
  {"dev_poison", "FL_DEV_POISON", &fl_context::Options::dev_poison, false, 0, 1},
  {"ws_pad", "FL_DEV_WS_PAD", &fl_context::Options::ws_pad, false, 0, 16l << 20},
  {"pipeline_icp", "FL_PIPELINE_ICP", &fl_context::Options::pipeline_icp, false, 0, 3},
  {"frontend_chunk_rows", "FL_FRONTEND_CHUNK_ROWS", &fl_context::Options::frontend_chunk_rows, false, 0, 60 * 1024},
  {"scan_run", "FL_SCAN_RUN", &fl_context::Options::scan_run, false, 0, 64},
  {"refine_lds", "FL_REFINE_LDS", &fl_context::Options::refine_lds, false, 0, 2},
  {"refine_lds_bytes", "FL_REFINE_LDS_BYTES", &fl_context::Options::refine_lds_bytes, false, 0, FL_REFINE_LDS_BYTES},
  {"verify_fused", "FL_VERIFY_FUSED", &fl_context::Options::verify_fused, false, 0, 1},
  {"verify_fused_px", "FL_VERIFY_FUSED_PX", &fl_context::Options::verify_fused_px, false, 0, FL_VERIFY_FUSED_PX},
};

// A value outside an option's range is refused rather than taken for "default": a forced kernel variant with a mistyped
// value would otherwise run the default one without anyone noticing.
static bool fl_option_valid(const FlOptionName &o, long v)
{
  if (v < o.lo || v > o.hi) return false;
  if (o.field == &fl_context::Options::frontend_chunk_rows) return v % 60 == 0;
  if (o.field == &fl_context::Options::verify_fused_px) return v == 0 || v >= FL_WAVE;
  if (o.field == &fl_context::Options::scan_prune_step) return v == 0 || v == 2 || v == 4 || v == 8;
  if (o.field == &fl_context::Options::scan_first) return v == 0 || v == 8 || v == 12 || v == 14 || v == 16;
  return o.field != &fl_context::Options::icp_occ || v == 0 || v >= 4;
}

extern "C" int fl_context_create(int device, fl_context **out)
{
  if (!out) return FL_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FL_ERR_NO_DEVICE;   // no CPU fallback
  if (device < 0 || device >= n) return FL_ERR_INVALID;
  fl_context *ctx = new fl_context();
  ctx->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return FL_ERR_HIP;
  }
  ctx->stream = ctx->own_stream;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) ctx->cus = prop.multiProcessorCount;
  }
  // the development switches' initial values: the environment is read here and nowhere else
  // (a value outside the option's range keeps the built-in default)
  for (const FlOptionName &o : fl_option_names)
    if (const char *e = getenv(o.env)) {
      const long v = o.hex ? (long)strtoul(e, nullptr, 16) : atol(e);
      if (fl_option_valid(o, v)) ctx->opt.*(o.field) = v;
    }
  *out = ctx;
  return FL_OK;
}

extern "C" void *fl_context_get_stream(fl_context *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
extern "C" int fl_context_get_device(const fl_context *ctx) { return ctx ? ctx->device : -1; }
extern "C" fl_context *fl_detector_get_context(fl_detector *det) { return det ? det->ctx : nullptr; }

extern "C" int fl_context_set_option(fl_context *ctx, const char *name, long value)
{
  if (!ctx || !name) return FL_ERR_INVALID;
  for (const FlOptionName &o : fl_option_names)
    if (!strcmp(name, o.name)) {
      if (!fl_option_valid(o, value)) return fl_set_error(ctx, FL_ERR_INVALID, "option '%s': %ld is out of range", name, value);
      ctx->opt.*(o.field) = value;
      return FL_OK;
    }
  return fl_set_error(ctx, FL_ERR_INVALID, "unknown option '%s'", name);
}

extern "C" int fl_context_get_option(const fl_context *ctx, const char *name, long *value)
{
  if (!ctx || !name || !value) return FL_ERR_INVALID;
  for (const FlOptionName &o : fl_option_names)
    if (!strcmp(name, o.name)) { *value = ctx->opt.*(o.field); return FL_OK; }
  return FL_ERR_INVALID;
}

// A context outlives the detectors created on it whatever order the caller destroys them in: fl_context_destroy on a
// context that still has detectors only marks it; the last fl_detector_destroy releases it.
static void context_release(fl_context *ctx)
{
  if (ctx->device < 0) { delete ctx; return; }           // a host-only detector's context (fl_dev_detector_create_host): no device state
  (void)hipSetDevice(ctx->device);
  (void)fl_context_sync_all(ctx);
  if (ctx->icp_stream) (void)hipStreamDestroy(ctx->icp_stream);
  if (ctx->ev_icp_tail) (void)hipEventDestroy(ctx->ev_icp_tail);
  if (ctx->scratch) (void)hipFree(ctx->scratch);
  if (ctx->pinned) (void)hipHostFree(ctx->pinned);
  if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

extern "C" void fl_context_destroy(fl_context *ctx)
{
  if (!ctx) return;
  if (ctx->detectors > 0) { ctx->destroy_pending = true; return; }
  context_release(ctx);
}

extern "C" const char *fl_last_error(const fl_context *ctx) { return ctx ? ctx->err : "null context"; }

extern "C" int fl_context_set_stream(fl_context *ctx, void *hip_stream)
{
  if (!ctx) return FL_ERR_INVALID;
  if (int rc = fl_context_sync_all(ctx)) return rc;
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  return FL_OK;
}

extern "C" int fl_context_synchronize(fl_context *ctx)
{
  if (!ctx) return FL_ERR_INVALID;
  FL_HIP(ctx, hipSetDevice(ctx->device));
  return fl_context_sync_all(ctx);
}

// ---------------------------------------------------------------------------------------------
extern "C" size_t fl_lm_label_stride(int w, int h, int T)
{
  // [T*T grids][W*H] + zero pad covering every over-read the reference can make inside one
  // continuous linear-memory Mat (Q2 of SURVEY.md section 8; oracle/linemod_oracle.c has the
  // same formula)
  size_t W = (size_t)(w / T), H = (size_t)(h / T);
  size_t pad = W * H + 16 * W + 64;
  size_t s = (size_t)T * T * W * H + pad;
  return (s + 63) & ~(size_t)63;
}

extern "C" int fl_detector_create(fl_context *ctx, int modalities, int levels, const int *T_at_level,
                                  fl_detector **out)
{
  if (!ctx || !out || !T_at_level) return FL_ERR_INVALID;
  if (modalities < 1 || modalities > FL_MAX_MODALITIES || levels < 1 || levels > FL_MAX_LEVELS)
    return fl_set_error(ctx, FL_ERR_INVALID, "modalities must be 1..%d and levels 1..%d", FL_MAX_MODALITIES,
                        FL_MAX_LEVELS);
  for (int l = 0; l < levels; ++l)
    if (T_at_level[l] < 1 || T_at_level[l] > 16) return fl_set_error(ctx, FL_ERR_INVALID, "T out of range");
  fl_detector *det = new fl_detector();
  det->ctx = ctx;
  ++ctx->detectors;
  det->M = modalities;
  det->L = levels;
  for (int l = 0; l < levels; ++l) det->T[l] = T_at_level[l];
  memset(&det->times, 0, sizeof(det->times));
  *out = det;
  return FL_OK;
}

static void free_device_tables(fl_detector *det)
{
  (void)hipFree(det->d_scan_items);
  (void)hipFree(det->d_scan_off);
  (void)hipFree(det->d_fine_hdr);
  (void)hipFree(det->d_fine_box);
  (void)hipFree(det->d_fine_feat);
  (void)hipFree(det->d_pyr);
  (void)hipFree(det->d_poses);
  (void)hipFree(det->d_class_first);
  (void)hipFree(det->d_item_enabled);
  (void)hipFree((void *)det->d_depth_ptrs);
  (void)hipFree(det->d_ws);
  (void)hipFree(det->d_results);
  if (det->h_results) (void)hipHostFree(det->h_results);
  det->d_scan_items = nullptr;
  det->n_scan_items = 0;
  det->scan_item_g.clear();
  det->d_scan_off = nullptr;
  det->d_fine_hdr = nullptr;
  det->d_fine_box = nullptr;
  det->d_fine_feat = nullptr;
  det->d_pyr = nullptr;
  det->d_poses = nullptr;
  det->d_class_first = nullptr;
  det->d_item_enabled = nullptr;
  det->d_depth_ptrs = nullptr;
  det->d_ws = nullptr;
  det->d_results = nullptr;
  det->h_results = nullptr;
  for (auto &e : det->ev)
    if (e) { (void)hipEventDestroy(e); e = nullptr; }
  for (int b = 0; b < 2; ++b) {
    if (det->ev_done[b]) { (void)hipEventDestroy(det->ev_done[b]); det->ev_done[b] = nullptr; }
    if (det->ev_set_read[b]) { (void)hipEventDestroy(det->ev_set_read[b]); det->ev_set_read[b] = nullptr; }
    det->set_busy[b] = false;
  }
  det->prev_n = 0;
  det->latest_open = false;
  if (det->d_jobs) { (void)hipFree(det->d_jobs); det->d_jobs = nullptr; }
  if (det->d_icp_order) { (void)hipFree(det->d_icp_order); det->d_icp_order = nullptr; }
  det->selected_frames = 0;
  if (det->d_zoom) { (void)hipFree(det->d_zoom); det->d_zoom = nullptr; }
  if (det->d_zoom_src) { (void)hipFree(det->d_zoom_src); det->d_zoom_src = nullptr; det->zoom_src_bytes = 0; }
  for (int b = 0; b < 2; ++b) {
    if (det->d_in[b]) { (void)hipFree(det->d_in[b]); det->d_in[b] = nullptr; }
    if (det->ev_up[b]) { (void)hipEventDestroy(det->ev_up[b]); det->ev_up[b] = nullptr; }
    if (det->ev_read[b]) { (void)hipEventDestroy(det->ev_read[b]); det->ev_read[b] = nullptr; }
    det->read_pending[b] = false;
  }
  if (det->copy_stream) { (void)hipStreamSynchronize(det->copy_stream); (void)hipStreamDestroy(det->copy_stream); det->copy_stream = nullptr; }
}

extern "C" void fl_detector_destroy(fl_detector *det)
{
  if (!det) return;
  fl_context *ctx = det->ctx;
  if (ctx->device >= 0) {                                // a host-only detector never had device state
    (void)hipSetDevice(ctx->device);
    (void)fl_context_sync_all(ctx);
    free_device_tables(det);
    for (auto &c : det->classes)
      if (c.d_depths) (void)hipFree(c.d_depths);
  }
  delete det;
  if (--ctx->detectors == 0 && ctx->destroy_pending) context_release(ctx);
}

extern "C" int fl_detector_add_class(fl_detector *det, const char *class_id, int n_pyramids,
                                     const fl_template *templates, const fl_feature *features,
                                     int n_features, const float *poses13)
{
  if (!det || !class_id || n_pyramids < 0 || (n_pyramids && !templates)) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (det->finalized) return fl_set_error(ctx, FL_ERR_STATE, "detector already finalized");
  for (auto &c : det->classes)
    if (c.id == class_id) return fl_set_error(ctx, FL_ERR_ASSERT, "class '%s' already present (linemod.cpp:1727)", class_id);
  size_t nt = (size_t)n_pyramids * det->L * det->M;
  for (size_t i = 0; i < nt; ++i) {
    const fl_template &t = templates[i];
    if (t.feat_count < 0 || t.feat_begin < 0 || (long)t.feat_begin + t.feat_count > n_features)
      return fl_set_error(ctx, FL_ERR_INVALID, "template %zu: feature range outside the feature array", i);
    if (t.feat_count > FL_MAX_FEATURES)
      return fl_set_error(ctx, FL_ERR_ASSERT, "template %zu has %d features > 63 (CV_Assert linemod.cpp:1137)", i,
                          t.feat_count);
    for (int k = 0; k < t.feat_count; ++k) {
      const fl_feature &f = features[t.feat_begin + k];
      if (f.label < 0 || f.label > 7) return fl_set_error(ctx, FL_ERR_INVALID, "feature label outside 0..7");
      if (f.x < -32768 || f.x > 32767 || f.y < -32768 || f.y > 32767)
        return fl_set_error(ctx, FL_ERR_INVALID, "feature coordinate outside int16");
    }
  }
  FlClass c;
  c.id = class_id;
  c.n_pyramids = n_pyramids;
  c.templates.assign(templates, templates + nt);
  c.features.assign(features, features + n_features);
  if (poses13) c.poses.assign(poses13, poses13 + (size_t)n_pyramids * 13);
  auto it = std::lower_bound(det->classes.begin(), det->classes.end(), c,
                             [](const FlClass &a, const FlClass &b) { return a.id < b.id; });
  det->classes.insert(it, std::move(c));
  return FL_OK;
}

extern "C" int fl_detector_set_model_depths(fl_detector *det, int class_idx, int first, int count,
                                            const uint16_t *depth_01mm, int w, int h, int mem)
{
  if (!det || !depth_01mm || w <= 0 || h <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_STATE, "a host-only detector holds no depth renders");
  if (class_idx < 0 || class_idx >= (int)det->classes.size()) return fl_set_error(ctx, FL_ERR_INVALID, "class_idx");
  FlClass &c = det->classes[class_idx];
  if (first < 0 || count < 0 || first + count > c.n_pyramids) return fl_set_error(ctx, FL_ERR_INVALID, "pyramid range");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_pipeline_join(det)) return rc;     // an ICP stage in flight reads the renders
  size_t per = (size_t)w * h * sizeof(uint16_t);
  // the finalized tables hold a pointer per pyramid that has a render: renders that arrive later join them below, and
  // have to be frame-sized like the ones fl_detector_finalize checked
  if (det->finalized && (w != det->w0 || h != det->h0))
    return fl_set_error(ctx, FL_ERR_INVALID, "model depth renders must be %dx%d like the frames", det->w0, det->h0);
  if (!c.d_depths) {
    FL_HIP(ctx, hipMalloc((void **)&c.d_depths, per * (size_t)c.n_pyramids));
    FL_HIP(ctx, hipMemsetAsync(c.d_depths, 0, per * (size_t)c.n_pyramids, ctx->stream));
    c.has_depth.assign((size_t)c.n_pyramids, 0);
    c.dw = w;
    c.dh = h;
  } else if (c.dw != w || c.dh != h)
    return fl_set_error(ctx, FL_ERR_INVALID, "model depth size changed");
  FL_HIP(ctx, hipMemcpyAsync((uint8_t *)c.d_depths + per * (size_t)first, depth_01mm, per * (size_t)count,
                             mem == FL_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  std::vector<const uint16_t *> ptrs;
  for (int p = first; p < first + count; ++p) {
    c.has_depth[(size_t)p] = 1;
    ptrs.push_back(c.d_depths + (size_t)p * w * h);
  }
  if (det->finalized && det->d_depth_ptrs && count > 0) {
    FL_HIP(ctx, hipMemcpyAsync(det->d_depth_ptrs + c.first_g + first, ptrs.data(), sizeof(ptrs[0]) * (size_t)count, hipMemcpyHostToDevice,
                               ctx->stream));
  }
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

extern "C" int fl_detector_num_templates(const fl_detector *det)
{
  if (!det) return FL_ERR_INVALID;
  int n = 0;
  for (auto &c : det->classes) n += c.n_pyramids;
  return n;
}
extern "C" int fl_detector_num_classes(const fl_detector *det) { return det ? (int)det->classes.size() : FL_ERR_INVALID; }

template <typename T>
static int upload(fl_context *ctx, const std::vector<T> &v, T **out)
{
  size_t bytes = std::max<size_t>(v.size(), 1) * sizeof(T);
  FL_HIP(ctx, hipMalloc((void **)out, bytes));
  if (!v.empty()) FL_HIP(ctx, hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return FL_OK;
}

// k_scan's work list: one item per (pyramid, chunk of 1024 coarse positions) -- only the chunks some modality's
// template_positions reach (a 160-pixel template at VGA level 1 has P = 831 of 1200 cells: its second chunk is empty).
// scan_off gains FL_SCAN_OFF_PAD zero offsets: the kernel requests the next group of eight while it adds the current one,
// behind a bank's last group too.
void fl_build_scan_items(const std::vector<FlScanHdr> &hdr, int n_pyr, int M, int WH, uint32_t zero_off, std::vector<uint32_t> &scan_off,
                         std::vector<FlScanItem> &items)
{
  const int nchunks = (WH + 1023) / 1024;
  scan_off.insert(scan_off.end(), FL_SCAN_OFF_PAD, zero_off);
  items.clear();
  for (int g = 0; g < n_pyr; ++g) {
    int pmax = 0, nf_all = 0;
    for (int m = 0; m < M; ++m) {
      pmax = std::max(pmax, (int)hdr[(size_t)g * M + m].P);
      nf_all += hdr[(size_t)g * M + m].nf;
    }
    for (int c = 0; c < nchunks && (c == 0 || c * 1024 < pmax); ++c) {    // chunk 0 always: the debug tap zero-fills through it
      FlScanItem it;
      it.g = g;
      it.chunk_nf = (uint32_t)c | ((uint32_t)nf_all << 16);
      for (int m = 0; m < FL_MAX_MODALITIES; ++m) {
        const FlScanHdr h = m < M ? hdr[(size_t)g * M + m] : FlScanHdr{0, 0, 0, 0};
        it.mod[m].P = h.P;
        it.mod[m].off_begin = h.off_begin;
        it.mod[m].npad_nf = (uint32_t)h.n_pad | ((uint32_t)h.nf << 16);
      }
      const FlScanHdr h0 = hdr[(size_t)g * M];
      for (int u = 0; u < 8; ++u) it.off0[u] = h0.n_pad > 0 ? scan_off[(size_t)h0.off_begin + u] : zero_off;
      items.push_back(it);
    }
  }
}

// fl_build_scan_items on caller-supplied headers (hdr: n_pyr * M entries of {P, off_begin, n_pad, nf}) and offsets, for
// tests/test_scan_items_cpu.py: items_out receives up to cap_items records of 16 words, offs_out the padded offset table
// (n_offs + FL_SCAN_OFF_PAD entries).  Returns the number of items, or FL_ERR_INVALID.  Host arithmetic, no GPU.
extern "C" int fl_dev_scan_items(const int32_t *hdr, int n_pyr, int M, int WH, uint32_t zero_off, const uint32_t *offs, int n_offs,
                                 uint32_t *items_out, int cap_items, uint32_t *offs_out)
{
  if (!hdr || !offs || !items_out || !offs_out || n_pyr < 0 || M < 1 || M > FL_MAX_MODALITIES || WH < 1 || n_offs < 0) return FL_ERR_INVALID;
  std::vector<FlScanHdr> h((size_t)n_pyr * M);
  for (size_t i = 0; i < h.size(); ++i) {
    h[i] = FlScanHdr{hdr[4 * i], hdr[4 * i + 1], hdr[4 * i + 2], hdr[4 * i + 3]};
    if (h[i].n_pad < 0 || h[i].n_pad % 8 || h[i].off_begin < 0 || (long)h[i].off_begin + h[i].n_pad > n_offs) return FL_ERR_INVALID;
  }
  std::vector<uint32_t> so(offs, offs + n_offs);
  std::vector<FlScanItem> items;
  fl_build_scan_items(h, n_pyr, M, WH, zero_off, so, items);
  for (size_t i = 0; i < items.size() && (int)i < cap_items; ++i) memcpy(items_out + 16 * i, &items[i], sizeof(FlScanItem));
  memcpy(offs_out, so.data(), so.size() * sizeof(uint32_t));
  return (int)items.size();
}

// Detector::match's class_ids (linemod.cpp:1418-1434): empty = every class; otherwise only the listed classes
// that exist are matched (unknown ids are ignored, repeats change nothing after sort + unique).
int fl_apply_class_filter(fl_detector *det)
{
  fl_context *ctx = det->ctx;
  std::vector<uint8_t> en;
  for (size_t ci = 0; ci < det->classes.size(); ++ci) {
    bool on = det->class_filter.empty();
    for (size_t k = 0; k < det->class_filter.size(); ++k) on = on || det->class_filter[k] == det->classes[ci].id;
    en.insert(en.end(), (size_t)det->classes[ci].n_pyramids, on ? 1 : 0);
  }
  // k_scan reads the flag of a work item, not of a pyramid, as a byte of an aligned dword on the scalar side: it is
  // requested together with the item's record instead of behind it
  if (det->scan_item_g.empty()) return FL_OK;            // before fl_detector_finalize: it applies the filter
  std::vector<uint8_t> item_en(fl_align(det->scan_item_g.size(), 4), 0);
  for (size_t i = 0; i < det->scan_item_g.size(); ++i) item_en[i] = en[(size_t)det->scan_item_g[i]];
  if (!det->d_item_enabled) FL_HIP(ctx, hipMalloc((void **)&det->d_item_enabled, item_en.size()));
  FL_HIP(ctx, hipMemcpyAsync(det->d_item_enabled, item_en.data(), item_en.size(), hipMemcpyHostToDevice, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

extern "C" int fl_detector_set_class_filter(fl_detector *det, const char *const *class_ids, int n)
{
  if (!det || n < 0 || (n > 0 && !class_ids)) return FL_ERR_INVALID;
  det->class_filter.clear();
  for (int i = 0; i < n; ++i) det->class_filter.push_back(class_ids[i] ? class_ids[i] : "");
  if (!det->finalized) return FL_OK;                     // applied by fl_detector_finalize
  FL_HIP(det->ctx, hipSetDevice(det->ctx->device));
  return fl_apply_class_filter(det);
}

// The per-frame workspace (one allocation, frame stride ws_stride) for candidate capacity `cap`; allocates d_ws.
static int layout_workspace(fl_detector *det, int cap)
{
  fl_context *ctx = det->ctx;
  const int L = det->L, M = det->M, w0 = det->w0, h0 = det->h0;
  // per-frame workspace layout
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off = fl_align(off + bytes, 256); return o; };
  det->off_bgr = take((size_t)w0 * h0 * 3);
  det->off_depth = take((size_t)w0 * h0 * 2);
  for (int l = 0; l < L; ++l) {
    FlLevelGeom &g = det->geom[l];
    g.bgr_off = l == 0 ? det->off_bgr : take((size_t)g.w * g.h * 3);
    for (int m = 0; m < M; ++m) g.quant_off[m] = take((size_t)g.w * g.h);
    // only the coarsest level is scanned by every template and gets linear memories; the finer
    // levels are touched by a handful of 16x16 patches per frame and keep just the spread image
    for (int m = 0; m < M; ++m) {
      g.lm_off[m] = l == L - 1 ? take((size_t)8 * g.stride + 64) : 0;
      g.spread_off[m] = l == L - 1 ? 0 : take((size_t)g.w * g.h + 64);
    }
  }
  det->off_tmp = take((size_t)w0 * h0);
  det->off_count = take(256);
  det->off_tiles = take((size_t)(L > 1 ? L - 1 : 1) * FL_TILE_BLOCK_WORDS * sizeof(uint32_t));
  det->lazy_capable = L > 1;
  for (int l = 0; l + 1 < L; ++l) {
    const FlLevelGeom &g = det->geom[l];
    if (((g.w + FL_TILE - 1) / FL_TILE) * ((g.h + FL_TILE - 1) / FL_TILE) > FL_TILE_WORDS * 32) det->lazy_capable = false;
  }
  det->off_cand = take((size_t)cap * sizeof(FlCand));
  det->off_keys = take((size_t)cap * 16);
  det->off_match = take((size_t)cap * sizeof(fl_match));
  det->n_pts_max = det->max_tw * det->max_th;
  det->off_icp = take(fl_icp_ws_bytes(det->n_pts_max));
  // the second set of what the ICP stage reads (see fl_internal.h); off_count / off_match keep naming the current set
  det->off_count_set[0] = det->off_count;
  det->off_match_set[0] = det->off_match;
  det->off_count_set[1] = take(256);
  det->off_match_set[1] = take((size_t)cap * sizeof(fl_match));
  det->off_count = det->off_count_set[det->set];
  det->off_match = det->off_match_set[det->set];
  det->ws_stride = fl_align(off, 4096);
  det->cap = cap;
  if (ctx->opt.ws_pad > 0) det->ws_stride += fl_align((size_t)ctx->opt.ws_pad, 4096);   // dev aid: stride sensitivity
  if (hipMalloc((void **)&det->d_ws, det->ws_stride * (size_t)det->max_batch) != hipSuccess) {
    det->d_ws = nullptr;
    (void)hipGetLastError();
    return fl_set_error(ctx, FL_ERR_HIP, "frame workspaces: %zu MB for %d frames with %d candidates each", (det->ws_stride * (size_t)det->max_batch) >> 20,
                        det->max_batch, cap);
  }
  // on the context's stream (it is non-blocking: a null-stream hipMemset is not ordered against it and would still be
  // zeroing the workspace while the replay after fl_grow_candidates fills it), and finished before anything else starts
  FL_HIP(ctx, hipMemsetAsync(det->d_ws, 0, det->ws_stride * (size_t)det->max_batch, ctx->stream));
  FL_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return FL_OK;
}

// The reference's candidate / match vectors grow without limit (linemod.cpp:1490-1504, 1575); here they are fixed-size
// slices of the frame workspace, so a frame that overflows them makes the caller-facing entry points grow the slices
// (workspace re-laid out for the next power of two >= `needed`) and run the batch again.  Nothing but scratch lives
// in the workspace between calls.
int fl_grow_candidates(fl_detector *det, int needed)
{
  fl_context *ctx = det->ctx;
  if (det->cap_hard) return fl_set_error(ctx, FL_ERR_OVERFLOW, "more than %d candidates in one frame (hard cap asked for at fl_detector_finalize)", det->cap);
  long long want = det->cap;
  while (want < needed || want <= det->cap) want <<= 1;
  if (want > (1ll << 28)) return fl_set_error(ctx, FL_ERR_OVERFLOW, "%d candidates in one frame", needed);
  if (int rc = fl_context_sync_all(ctx)) return rc;         // both streams: ICP reads the match lists and writes its workspaces
  (void)fl_pipeline_join(det);
  const int old_cap = det->cap;
  fl_batch_forget(det);                                  // the frame workspaces are about to be freed
  (void)hipFree(det->d_ws);
  det->d_ws = nullptr;
  int rc = layout_workspace(det, (int)want);
  if (rc) {                                              // not enough memory: back to the old size, report the overflow
    if (layout_workspace(det, old_cap)) det->finalized = false;
    return fl_set_error(ctx, FL_ERR_OVERFLOW, "%d candidates in one frame and no memory for %d frames of that capacity", needed, det->max_batch);
  }
  return FL_OK;
}

// The synchronous entry points' retry policy, after attempt `attempt` returned *rc: on FL_ERR_OVERFLOW grow the candidate
// buffers to what the fullest of the last batch's n_frames frames needs and return true (run the call again), up to 6 times.
// A valid Detector::match input never becomes an error unless the caller asked for a hard cap: then, or without the memory,
// *rc becomes fl_grow_candidates' error.
bool fl_grow_after_overflow(fl_detector *det, int n_frames, int attempt, int *rc)
{
  if (!det || *rc != FL_ERR_OVERFLOW || attempt >= 6) return false;
  int needed = 0;
  if (fl_overflow_needed(det, n_frames, &needed) != FL_OK || needed <= 0) return false;
  const int g = fl_grow_candidates(det, needed);
  if (g != FL_OK) { *rc = g; return false; }
  return true;
}

extern "C" int fl_detector_finalize(fl_detector *det, int w0, int h0, int max_batch, int max_candidates)
{
  if (!det || w0 <= 0 || h0 <= 0 || max_batch <= 0) return FL_ERR_INVALID;
  fl_context *ctx = det->ctx;
  if (ctx->device < 0) return fl_set_error(ctx, FL_ERR_STATE, "a host-only detector cannot be finalized");
  FL_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = fl_context_sync_all(ctx)) return rc;
  free_device_tables(det);
  det->finalized = false;
  fl_batch_forget(det);
  const int L = det->L, M = det->M;
  // max_candidates > 0: initial per-frame capacity of the candidate / match buffers, grown on demand (the reference's
  // vectors are unbounded, linemod.cpp:1490-1504); < 0: a hard cap of -max_candidates (FL_ERR_OVERFLOW beyond it);
  // 0: 65536, grown on demand
  int cap = max_candidates > 0 ? max_candidates : (max_candidates < 0 ? -max_candidates : 65536);
  det->cap_hard = max_candidates < 0;
  int cap2 = 1;
  while (cap2 < cap) cap2 <<= 1;
  cap = cap2;                                        // power of two (bitonic sort)

  // geometry per level; reference asserts (linemod.cpp:981, 1062-1063)
  for (int l = 0; l < L; ++l) {
    FlLevelGeom &g = det->geom[l];
    g.w = w0 >> l;
    g.h = h0 >> l;
    g.T = det->T[l];
    if (g.w <= 0 || g.h <= 0) return fl_set_error(ctx, FL_ERR_INVALID, "level %d is empty", l);
    if (g.w % g.T || g.h % g.T)
      return fl_set_error(ctx, FL_ERR_ASSERT, "level %d: %dx%d not divisible by T=%d (CV_Assert linemod.cpp:1062)", l, g.w,
                          g.h, g.T);
    if ((g.w * g.h) % 16) return fl_set_error(ctx, FL_ERR_ASSERT, "level %d: rows*cols %% 16 != 0 (linemod.cpp:981)", l);
    g.W = g.w / g.T;
    g.H = g.h / g.T;
    g.WH = g.W * g.H;
    size_t s = fl_lm_label_stride(g.w, g.h, g.T);
    if (8 * s > 0xFFFFFFFFull) return fl_set_error(ctx, FL_ERR_INVALID, "linear memory too large");
    g.stride = (uint32_t)s;
    g.zero_off = (uint32_t)(7 * s + (size_t)g.T * g.T * g.WH);   // pad of label 7
  }

  // flatten the bank
  std::vector<FlScanHdr> scan_hdr;
  std::vector<uint32_t> scan_off;
  std::vector<FlFineHdr> fine_hdr;
  std::vector<FlFineFeat> fine_feat;
  std::vector<FlFineBox> fine_box;
  for (int l = 0; l < FL_MAX_LEVELS; ++l) det->refine_window_max[l] = 0;
  std::vector<FlPyrInfo> pyr;
  std::vector<float> poses;
  std::vector<const uint16_t *> depth_ptrs;
  std::vector<int> class_first;
  int g_idx = 0;
  double scan_bytes = 0.0;
  det->max_tw = det->max_th = 1;
  det->depth_w = det->depth_h = 0;
  for (size_t ci = 0; ci < det->classes.size(); ++ci) {
    FlClass &c = det->classes[ci];
    c.first_g = g_idx;
    class_first.push_back(g_idx);
    if (c.d_depths) {
      if (c.dw != w0 || c.dh != h0)
        return fl_set_error(ctx, FL_ERR_INVALID, "model depth renders must be %dx%d like the frames", w0, h0);
      det->depth_w = c.dw;
      det->depth_h = c.dh;
    }
    for (int p = 0; p < c.n_pyramids; ++p, ++g_idx) {
      const fl_template *tp = &c.templates[(size_t)p * L * M];
      FlPyrInfo pi;
      pi.class_idx = (int)ci;
      pi.template_id = p;
      pi.off_x0 = tp[0].offset_x;
      pi.off_y0 = tp[0].offset_y;
      pi.width0 = tp[0].width;
      pi.height0 = tp[0].height;
      const bool has_depth = c.d_depths && c.has_depth[(size_t)p];
      pi.depth_slot = has_depth ? p : -1;
      pi.pad = 0;
      pyr.push_back(pi);
      det->max_tw = std::max(det->max_tw, std::min(tp[0].width, w0));
      det->max_th = std::max(det->max_th, std::min(tp[0].height, h0));
      for (int k = 0; k < 13; ++k) poses.push_back(c.poses.empty() ? 0.f : c.poses[(size_t)p * 13 + k]);
      depth_ptrs.push_back(has_depth ? c.d_depths + (size_t)p * c.dw * c.dh : nullptr);
      // coarsest level: scan tables (similarity(), linemod.cpp:1130-1214)
      {
        const FlLevelGeom &g = det->geom[L - 1];
        for (int m = 0; m < M; ++m) {
          const fl_template &t = tp[(L - 1) * M + m];
          FlScanHdr h;
          int wf = (t.width - 1) / g.T + 1, hf = (t.height - 1) / g.T + 1;
          int span_x = g.W - wf, span_y = g.H - hf;
          h.P = span_y * g.W + span_x + 1;
          if (h.P > g.WH) h.P = g.WH;              // dst has only W*H cells (width/height <= 0 input)
          h.off_begin = (int)scan_off.size();
          h.nf = t.feat_count;
          int n = 0;
          for (int k = 0; k < t.feat_count; ++k) {
            const fl_feature &f = c.features[t.feat_begin + k];
            if (f.x < 0 || f.x >= g.w || f.y < 0 || f.y >= g.h) continue;        // :1179
            uint32_t off = (uint32_t)f.label * g.stride + (uint32_t)((f.y % g.T) * g.T + (f.x % g.T)) * g.WH +
                           (uint32_t)((f.y / g.T) * g.W + f.x / g.T);             // accessLinearMemory :1094
            scan_off.push_back(off);
            ++n;
          }
          while (n % 8) { scan_off.push_back(g.zero_off); ++n; }
          h.n_pad = n;
          scan_hdr.push_back(h);
          // B_tmpl = sum_m nf_m*P + M*P + 2*P (bytes the reference touches)
          const double Pd = h.P > 0 ? (double)h.P : 0.0;
          scan_bytes += (double)t.feat_count * Pd + Pd + (m == 0 ? 2.0 * Pd : 0.0);
        }
      }
      // finer levels: refinement tables (similarityLocal(), linemod.cpp:1226-1300)
      for (int l = 0; l < L - 1; ++l) {
        FlRect all = {0, 0, -1, -1};                       // the boxes of this pyramid's modalities at this level, united
        for (int m = 0; m < M; ++m) {
          const fl_template &t = tp[l * M + m];
          FlRect box = {0, 0, -1, -1};
          FlFineHdr h;
          h.feat_begin = (int)fine_feat.size();
          h.feat_count = t.feat_count;
          h.width = t.width;
          h.height = t.height;
          for (int k = 0; k < t.feat_count; ++k) {
            const fl_feature &f = c.features[t.feat_begin + k];
            FlFineFeat ff;
            ff.x = (int16_t)f.x;
            ff.y = (int16_t)f.y;
            {
              const int Tl = det->geom[l].T;
              const int rx = ((f.x % Tl) + Tl) % Tl, ry = ((f.y % Tl) + Tl) % Tl;
              ff.gx = (uint8_t)rx;
              ff.gy = (uint8_t)ry;
              ff.qx = (int16_t)((f.x - rx) / Tl);
              ff.qy = (int16_t)((f.y - ry) / Tl);
              ff.label = (uint8_t)f.label;
              ff.pad = 0;
            }
            fine_feat.push_back(ff);
            const FlRect one = {ff.x, ff.y, ff.x, ff.y};
            box = fl_rect_union(box, one);
          }
          fine_hdr.push_back(h);
          fine_box.push_back(FlFineBox{(int16_t)box.x0, (int16_t)box.y0, (int16_t)box.x1, (int16_t)box.y1});
          all = fl_rect_union(all, box);
        }
        if (all.x1 >= all.x0) {
          // the largest window a candidate of this pyramid can ask for: its box grown by a patch's span, no wider or taller
          // than the image, starting up to 3 bytes early (the window starts at a multiple of 4)
          const FlLevelGeom &gl = det->geom[l];
          const int ww = std::min(all.x1 - all.x0 + 15 * gl.T + 1 + 3, (gl.w + 3) & ~3);
          const int hh = std::min(all.y1 - all.y0 + 15 * gl.T + 1, gl.h);
          const long bytes = (long)fl_refine_pitch(ww, fl_refine_qmask(gl.T)) * hh;
          det->refine_window_max[l] = std::max(det->refine_window_max[l], bytes);
        }
      }
    }
  }
  det->n_pyr = g_idx;
  det->scan_bytes_per_frame = scan_bytes;

  int rc;
  {
    std::vector<FlScanItem> items;
    fl_build_scan_items(scan_hdr, g_idx, M, det->geom[L - 1].WH, det->geom[L - 1].zero_off, scan_off, items);
    det->n_scan_items = (int)items.size();
    det->scan_item_g.clear();
    for (const FlScanItem &it : items) det->scan_item_g.push_back(it.g);
    std::vector<int> nfs;
    for (const FlScanItem &it : items) nfs.push_back((int)(it.chunk_nf >> 16));
    if (!nfs.empty()) std::nth_element(nfs.begin(), nfs.begin() + nfs.size() / 2, nfs.end());
    det->scan_nf_typical = nfs.empty() ? 0 : nfs[nfs.size() / 2];
    if ((rc = upload(ctx, items, &det->d_scan_items))) return rc;
  }
  if ((rc = upload(ctx, scan_off, &det->d_scan_off))) return rc;
  if ((rc = upload(ctx, fine_hdr, &det->d_fine_hdr))) return rc;
  if ((rc = upload(ctx, fine_feat, &det->d_fine_feat))) return rc;
  if ((rc = upload(ctx, fine_box, &det->d_fine_box))) return rc;
  if ((rc = upload(ctx, pyr, &det->d_pyr))) return rc;
  if ((rc = upload(ctx, poses, &det->d_poses))) return rc;
  if ((rc = upload(ctx, class_first, &det->d_class_first))) return rc;
  if ((rc = fl_apply_class_filter(det))) return rc;
  {
    const uint16_t **tmp = nullptr;
    if ((rc = upload(ctx, depth_ptrs, (const uint16_t ***)&tmp))) return rc;
    det->d_depth_ptrs = tmp;
  }

  det->w0 = w0;
  det->h0 = h0;
  det->max_batch = max_batch;
  det->eager_env = ctx->opt.eager_frontend != 0;          // development switches (fl_context_set_option), sampled here
  det->poison_env = ctx->opt.dev_poison != 0;
  if ((rc = layout_workspace(det, cap))) return rc;
  if ((rc = fl_icp_prepare(det))) return rc;
  FL_HIP(ctx, hipMalloc((void **)&det->d_results, sizeof(fl_recognition_result) * (size_t)max_batch));
  FL_HIP(ctx, hipHostMalloc((void **)&det->h_results, sizeof(fl_recognition_result) * 2 * (size_t)max_batch,
                            hipHostMallocDefault));
  for (auto &e : det->ev) FL_HIP(ctx, hipEventCreate(&e));
  for (int b = 0; b < 2; ++b) {
    FL_HIP(ctx, hipEventCreateWithFlags(&det->ev_done[b], hipEventDisableTiming));
    FL_HIP(ctx, hipEventCreateWithFlags(&det->ev_set_read[b], hipEventDisableTiming));
  }
  det->finalized = true;
  return FL_OK;
}
