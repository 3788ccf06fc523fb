// fl_internal.h -- shared host-side state of libfealess_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/fealess_hip.h"

#define FL_WAVE 64

struct fl_context {
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  // Pipelined recognition (fl_recognize_submit, option pipeline_icp): the ICP stage of a batch runs on this second
  // non-blocking stream while the next batch's LINEMOD stages run on `stream`.  Created on first use with the priority the
  // option asks for.  ev_icp_tail is recorded after the last work queued on it; icp_pending: `stream` has not waited for it yet.
  hipStream_t icp_stream = nullptr;
  long icp_stream_mode = 0;     // the pipeline_icp value icp_stream was created for
  hipEvent_t ev_icp_tail = nullptr;
  bool icp_pending = false;
  char err[512] = {0};
  // scratch for the single-shot stage entry points (grown on demand)
  void *scratch = nullptr;
  size_t scratch_bytes = 0;
  void *pinned = nullptr;       // small pinned host buffer for result read-back
  size_t pinned_bytes = 0;
  int cus = 256;                // multiProcessorCount of the device (launch heuristics), read once
  // Development / comparison switches (fl_context_set_option).  Speed only: results are identical whatever they hold.
  // Initial values come from the environment ONCE, when the context is created; no launch path reads the environment.
  struct Options {
    long scan_prune = 1;        // FL_SCAN_PRUNE: k_scan's exact pruning
    long scan_prune_mid = -1;   // FL_SCAN_PRUNE_MID: bit mask of the 8-feature groups after which a modality checks the bound (-1: built-in)
    long scan_prune_lanes = 1;  // FL_SCAN_PRUNE_LANES: 1 = a lane whose own 16 positions miss the bound stops loading, 0 = a wave stops as a
                                // whole or not at all
    long scan_prune_step = 0;   // FL_SCAN_PRUNE_STEP: feature loads between two checks behind a modality's first eight: 8, 4 or 2;
                                // 0 = 4 from 256 frames on, else 8 (fl_scan_step)
    long scan_first = 0;        // FL_SCAN_FIRST: features of a modality's first piece, streamed and with one check behind it: 8, 12, 14
                                // or 16; 0 = by batch size, bank and threshold (fl_scan_first)
    long icp_wide = -1;         // FL_ICP_WIDE: -1 by batch size, 0 / 1 force the 256- / 1024-thread ICP kernel
    long icp_occ = 0;           // FL_ICP_OCC: 0 by batch size, 4 / 5 force the 256-thread parity kernel built for 4 / 5 workgroups per CU
    long icp_idx16 = -1;        // FL_ICP_IDX16: -1 / 1 the 256-thread parity kernel keeps nn[] / perm[] as 16-bit values and rebuilds the
                                // distance phase's reference point from a 16-bit pixel where the workspace capacity is at most 65535
                                // points (the 32-bit build beyond), 0 = always the 32-bit build
    long icp_order = 1;         // FL_ICP_ORDER: ICP jobs dealt longest first
    long icp_wg_per_cu = 0;     // FL_ICP_WG_PER_CU: 0 = as many 256-thread ICP workgroups per CU as fit (4); 1 .. 3 = at most that many, the
                                // rest of the CU left to kernels of other streams (two pipelines on one GPU)
    long eager_frontend = 0;    // FL_EAGER_FRONTEND: finer pyramid levels in full before the scan (read by fl_detector_finalize)
    long dev_poison = 0;        // FL_DEV_POISON: fill what the lazy path leaves uncomputed with 0xFF (read by fl_detector_finalize)
    long ws_pad = 0;            // FL_DEV_WS_PAD: extra bytes of frame workspace stride (read by fl_detector_finalize)
    long pipeline_icp = 3;      // FL_PIPELINE_ICP: 0 = fl_recognize_submit queues everything on one stream; 1 = a batch's ICP stage on a
                                // second stream beside the next batch's LINEMOD stages; 2 / 3 = the same with that stream at the
                                // highest / lowest priority the device offers (3 measured best: the short LINEMOD kernels get the
                                // slots the long ICP launch frees, profiles/README.md)
    long frontend_chunk_rows = 0;   // FL_FRONTEND_CHUNK_ROWS: output rows a wave of the whole-image quantiser launches walks; 0 = 120 where
                                // the launch still fills the device several times over, else 60; a multiple of 60 is used as given
    long scan_run = 0;          // FL_SCAN_RUN: work items a wave of k_scan walks; 0 = FL_SCAN_RUN_AUTO where the launch still fills the
                                // device several times over, else a shorter run (fl_scan_run); 1 .. 64 is used as given
    long refine_lds = 0;        // FL_REFINE_LDS: 0 = k_refine_lds where the level's windows fit and the batch fills the device
                                // (fl_refine_use_lds), 1 = always k_refine, 2 = k_refine_lds wherever the windows fit
    long refine_lds_bytes = 0;  // FL_REFINE_LDS_BYTES: 0 = the compiled window budget, otherwise a smaller one (tests: group boundaries)
    long verify_fused = 0;      // FL_VERIFY_FUSED: 1 = fl_verify_batch renders and scores a pose in one workgroup's LDS (k_verify_fused)
                                // in place of the whole-image render and k_verify_score
    long verify_fused_px = 0;   // FL_VERIFY_FUSED_PX: 0 = the compiled band budget FL_VERIFY_FUSED_PX, otherwise a smaller one, from
                                // one wave's 64 pixels up (tests: band boundaries)
  } opt;
  bool verify_fused_attr = false;   // k_verify_fused's dynamic-LDS limit is set on this context's device (fl_launch_verify_fused)
  int detectors = 0;            // live fl_detector objects on this context
  bool destroy_pending = false; // fl_context_destroy was called while detectors were alive: the last one releases the context
};

int fl_set_error(fl_context *ctx, int code, const char *fmt, ...);
int fl_scratch(fl_context *ctx, size_t bytes, void **out);
int fl_pinned(fl_context *ctx, size_t bytes, void **out);
int fl_context_join(fl_context *ctx);        // ctx->stream waits for everything queued on the ICP stream (no host wait)
int fl_context_sync_all(fl_context *ctx);    // the host waits for both streams
int fl_icp_stream(fl_context *ctx, hipStream_t *out);   // the ICP stream for the current pipeline_icp value, created on first use

#define FL_HIP(ctx, call)                                                                  \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fl_set_error((ctx), FL_ERR_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #call, \
                          hipGetErrorString(e_));                                          \
  } while (0)

static inline size_t fl_align(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline bool fl_finite_all(const float *p, size_t n)   // host arrays: meshes, poses
{
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

// ---- device-side table entries ------------------------------------------------------------
// Offset of a feature's linear memory relative to the (level, modality) LM base of a frame.
#define FL_MAX_LEVELS 4
#define FL_MAX_MODALITIES 2
#define FL_MAX_FEATURES 63

struct FlScanHdr {       // one per (pyramid g, modality m) at the coarsest level
  int32_t P;             // template_positions (linemod.cpp:1155); <= 0: nothing to add
  int32_t off_begin;     // first entry in scan_offsets
  int32_t n_pad;         // entries, padded to a multiple of 8 with the zero offset
  int32_t nf;            // templ.features.size() (counts skipped features too)
};
// k_scan's work item: everything a wave needs of a (pyramid, 1024-position chunk) before its first vector load, in 64
// bytes: one dword per lane of a single load, the first group's offsets in the lanes a later group's offsets arrive in.  Built by fl_build_scan_items from the FlScanHdr entries: it depends on the bank and the
// geometry only.
struct FlScanItem {
  uint32_t off0[8];      // the first 8-offset group of modality 0 (the zero offset where it has none)
  int32_t g;             // pyramid
  uint32_t chunk_nf;     // chunk | (features of all modalities << 16)
  struct {
    int32_t P;           // FlScanHdr::P
    int32_t off_begin;   // FlScanHdr::off_begin
    uint32_t npad_nf;    // FlScanHdr::n_pad | (FlScanHdr::nf << 16)
  } mod[FL_MAX_MODALITIES];
};
static_assert(sizeof(FlScanItem) == 64 && FL_MAX_MODALITIES == 2, "a dword per lane of a 16-lane load");
#define FL_SCAN_OFF_PAD 8   // entries behind the last group of the offset table: k_scan requests a group ahead of the one it adds
// The work list of a bank: one item per (pyramid, chunk some modality's template_positions reach; chunk 0 always), pyramid
// major.  Appends FL_SCAN_OFF_PAD zero offsets to scan_off.  Host code only (tests/test_scan_items_cpu.py: fl_dev_scan_items).
void fl_build_scan_items(const std::vector<FlScanHdr> &hdr, int n_pyr, int M, int WH, uint32_t zero_off, std::vector<uint32_t> &scan_off,
                         std::vector<FlScanItem> &items);
struct FlFineFeat {      // one per feature at the finer levels (12 bytes)
  int16_t x, y;          // template-relative position
  int16_t qx, qy;        // floor(x / T), floor(y / T)
  uint8_t gx, gy;        // x mod T, y mod T (non-negative): the grid cell, invariant under offsets that are multiples of T
  uint8_t label, pad;    // quantized orientation 0..7
};
struct FlFineHdr {       // one per (pyramid g, level l < L-1, modality m)
  int32_t feat_begin, feat_count;
  int32_t width, height; // of this template (tp[start].width/height are taken from m == 0)
};
struct FlFineBox {       // beside FlFineHdr, same index: bounding box of the features' (x, y); x1 < x0: no features
  int16_t x0, y0, x1, y1;
};
struct FlPyrInfo {       // one per pyramid g
  int32_t class_idx, template_id;
  int32_t off_x0, off_y0, width0, height0;   // template[0]: rect_model_raw (obj_reco_lmicp.cpp:129)
  int32_t depth_slot;                        // index into the model-depth bank or -1
  int32_t pad;
};
struct FlCand {          // a candidate / match in flight
  int32_t x, y;
  int32_t g;             // global pyramid index; -1 once filtered out
  float sim;
};

struct FlRefineJob {     // fl_refine_matches: refine `match` (class-local template id) on frame `frame` of the last batch
  int32_t frame;
  fl_match match;
};

// ---- k_refine_lds: a group of candidates reads its spread bytes from one LDS window --------------------------------
// A candidate's in-bounds patches lie in a rectangle known before any feature is read: the features' box moved by the
// candidate's offsets, grown by the 15 * T a patch spans, clipped to the image.  Rectangles are inclusive; x1 < x0: empty.
#define FL_REFINE_LDS_BYTES 65536  // window budget of a workgroup; with the sort and planning state below it stays under the
                                   // 70 KB that one retired ICP workgroup leaves on a CU
#define FL_REFINE_GROUP_MAX 8      // candidates per group: two per wave, whose first modality's sums wait in LDS
#define FL_REFINE_BLOCK 256        // candidates ordered by location at a time: one per thread
struct FlRect { int x0, y0, x1, y1; };
// Pitch rule.  The window starts at x0 rounded down to a multiple of 4 and a row takes `pitch` bytes: a multiple of 16, so the
// 16-byte staging stores stay inside their row, whose quarter q = pitch / 4 has its bit (q mod 32) set in qmask: the residues
// at which the 8 rows x 4 column groups that one LDS cycle serves fall on the fewest common banks for this T (fl_refine_qmask).
__host__ __device__ inline int fl_refine_pitch(int width, uint32_t qmask)
{
  int q = (width + 3) >> 2;
  while (!((qmask >> (q & 31)) & 1u)) ++q;
  return q * 4;
}
// lane (row, cg) of a 32-lane group reads byte row * T * pitch + cg * 4 * T + const: bank (T * (row * q + cg)) mod 32
__host__ __device__ inline uint32_t fl_refine_qmask(int T)
{
  uint32_t mask = 0;
  int best = 33;
  for (int q = 0; q < 32; q += 4) {
    int n[32] = {0}, worst = 0;
    for (int row = 0; row < 8; ++row)
      for (int cg = 0; cg < 4; ++cg) {
        const int b = (T * (row * q + cg)) & 31;
        if (++n[b] > worst) worst = n[b];
      }
    if (worst < best) { best = worst; mask = 0; }
    if (worst == best) mask |= 1u << q;
  }
  return mask;
}
__host__ __device__ inline FlRect fl_rect_union(FlRect a, FlRect b)
{
  if (a.x1 < a.x0) return b;
  if (b.x1 < b.x0) return a;
  FlRect r;
  r.x0 = a.x0 < b.x0 ? a.x0 : b.x0;
  r.y0 = a.y0 < b.y0 ? a.y0 : b.y0;
  r.x1 = a.x1 > b.x1 ? a.x1 : b.x1;
  r.y1 = a.y1 > b.y1 ? a.y1 : b.y1;
  return r;
}
__host__ __device__ inline long fl_refine_window_bytes(FlRect r, uint32_t qmask)
{
  if (r.x1 < r.x0) return 0;
  return (long)fl_refine_pitch(r.x1 - (r.x0 & ~3) + 1, qmask) * (r.y1 - r.y0 + 1);
}
// The planner: the longest prefix of rects[0 .. n) (4 coordinates each, processing order), at most max_len long, whose union
// window fits `budget` bytes.  At least 1: finalize keeps a level whose largest single window does not fit on k_refine.
// *uni: the union of the prefix returned.
template <typename C>
__host__ __device__ inline int fl_refine_plan(const C *rects, int n, int max_len, long budget, uint32_t qmask, FlRect *uni)
{
  FlRect u = {rects[0], rects[1], rects[2], rects[3]};
  int len = 1;
  while (len < n && len < max_len) {
    const C *c = rects + 4 * len;
    const FlRect r = {c[0], c[1], c[2], c[3]};
    const FlRect v = fl_rect_union(u, r);
    if (fl_refine_window_bytes(v, qmask) > budget) break;
    u = v;
    ++len;
  }
  *uni = u;
  return len;
}
extern "C" int fl_dev_refine_pitch(int width, int T);
extern "C" int fl_dev_refine_plan(const int32_t *rects, int n, int max_len, long budget, int T, int32_t *uni);
extern "C" int fl_dev_refine_kernel(const fl_detector *det, int level);   // refine_ran[level]; -1: no such fine level
extern "C" long fl_dev_refine_window_max(const fl_detector *det, int level);   // refine_window_max[level]; -1: no such fine level

#define FL_TILE 60                 // tile edge in pixels (= CQ_COLS = CQ_CH of k_color_quantize)
#define FL_TILE_WORDS 16           // bitmap words per frame, level and kind: up to 512 tiles (1280x960: 352)
// One block of uint32 per frame and fine level: bm[2][FL_TILE_WORDS] (kind 0: tiles whose spread bytes are read,
// kind 1: tiles whose quantised pixels those spreads are made of), then rows[2][32 * FL_TILE_WORDS]: for a marked
// tile (first needed image row << 16) | last needed image row.
#define FL_TILE_BLOCK_WORDS (66 * FL_TILE_WORDS)
#define FL_NUM_EVENTS 24

struct FlLevelGeom {
  int32_t w, h, T, W, H, WH;
  uint32_t stride;       // bytes per label block
  uint32_t zero_off;     // offset (within a modality's LM) of >= WH+16W+64 zero bytes
  size_t quant_off[FL_MAX_MODALITIES];   // offsets inside a frame workspace
  size_t lm_off[FL_MAX_MODALITIES];      // coarsest level only: the 8 linear memories
  size_t spread_off[FL_MAX_MODALITIES];  // finer levels: the spread image (w*h bytes)
  size_t bgr_off;                        // colour image of this level
};

struct FlClass {
  std::string id;
  int n_pyramids = 0;
  std::vector<fl_template> templates;
  std::vector<fl_feature> features;
  std::vector<float> poses;              // n_pyramids*13 or empty
  int first_g = 0;                       // set at finalize
  uint16_t *d_depths = nullptr;          // n_pyramids * dw*dh u16 (0.1 mm) or null
  std::vector<uint8_t> has_depth;        // per pyramid: a render was uploaded (empty while d_depths is null).  The others are
                                         // a missing depth/<id>.png: FL_ERR_STATE when refined, not an all-zero render
  int dw = 0, dh = 0;
};

// The batch whose front-end images, match lists and counters the frame workspaces hold, and where its depth frames are.
// A call forgets it once its arguments pass their checks, before it overwrites frame workspaces or input buffers, and
// records its own batch as soon as that batch's front-end and match are queued (a frame that overflows its candidate
// buffers does not undo that).  A call that fails in between leaves no batch.
struct FlBatch {
  int n = 0;                             // frames (0: none)
  const uint16_t *depth = nullptr;       // the frames' depth on the device; null: the batch cannot be refined (fl_refine_*)
  size_t depth_stride = 0;
  bool match_only = false;               // fl_match_batch_submit: no ICP stage to time
};

struct fl_detector {
  fl_context *ctx = nullptr;
  int M = 0, L = 0;
  int T[FL_MAX_LEVELS] = {0};
  std::vector<FlClass> classes;          // kept sorted by id
  bool finalized = false;
  int w0 = 0, h0 = 0, max_batch = 0, cap = 0;
  bool cap_hard = false;                 // cap is a hard limit (FL_ERR_OVERFLOW) instead of an initial size that grows
  int n_pyr = 0;
  FlLevelGeom geom[FL_MAX_LEVELS];

  // device tables
  FlScanItem *d_scan_items = nullptr;    // (pyramid g, 1024-position chunk) pairs that have positions to scan: k_scan's work list
  int n_scan_items = 0;
  int scan_nf_typical = 0;    // the median over the work items of a pyramid's features at the coarsest level (fl_scan_first)
  std::vector<int32_t> scan_item_g;      // the items' pyramids on the host (fl_apply_class_filter)
  uint32_t *d_scan_off = nullptr;        // every (pyramid, modality)'s offsets, padded to groups of 8, + FL_SCAN_OFF_PAD
  FlFineHdr *d_fine_hdr = nullptr;       // n_pyr * (L-1) * M, index (g*(L-1)+l)*M+m
  FlFineBox *d_fine_box = nullptr;       // same index as d_fine_hdr
  long refine_window_max[FL_MAX_LEVELS] = {0};   // per fine level: LDS bytes of the largest single-candidate window over the bank (fl_refine_window_bytes)
  int refine_ran[FL_MAX_LEVELS] = {0};   // per fine level, last match stage: 0 none, 1 k_refine, 2 k_refine_lds (fl_dev_refine_kernel)
  FlFineFeat *d_fine_feat = nullptr;
  FlPyrInfo *d_pyr = nullptr;            // n_pyr
  int *d_class_first = nullptr;          // first global pyramid index of each class
  uint8_t *d_item_enabled = nullptr;     // per work item, padded to whole dwords: 0 = its pyramid's class is excluded by the class filter of match()
  std::vector<std::string> class_filter; // empty = all classes (Detector::match's class_ids)
  float *d_poses = nullptr;              // n_pyr * 13 (zeros when absent)
  const uint16_t **d_depth_ptrs = nullptr; // n_pyr pointers to model depth (0.1mm) or null
  int depth_w = 0, depth_h = 0;
  int max_tw = 0, max_th = 0;            // largest template[0] width/height: bounds the ICP clouds

  // per-frame workspace: one allocation, frame stride `ws_stride`
  uint8_t *d_ws = nullptr;
  size_t ws_stride = 0;
  size_t off_bgr = 0, off_depth = 0, off_cand = 0, off_count = 0, off_keys = 0, off_match = 0;
  size_t off_icp = 0, off_tmp = 0;
  // What the ICP stage reads of a frame workspace -- the counters and the sorted match list -- exists twice, so that the
  // match stage of batch i+1 can fill one set while ICP(i) still reads the other (pipelined fl_recognize_submit).
  // off_count / off_match always name the set of the batch last queued: every reader of "the last batch" uses them as before.
  // ev_set_read[s] is recorded on the ICP stream after the ICP stage that reads set s; set_busy[s]: ctx->stream has not waited
  // for it yet, which it does before the match stage next zeroes the set's counters.
  size_t off_count_set[2] = {0, 0}, off_match_set[2] = {0, 0};
  int set = 0;
  hipEvent_t ev_set_read[2] = {nullptr, nullptr};
  bool set_busy[2] = {false, false};
  // Lazy fine levels (fl_recognize_*): the finer levels are only ever read by k_refine, around the candidates the
  // coarse scan produced.  Their colour quantisation and spread images are therefore computed after the scan and
  // only in the 60x60-pixel tiles the candidates' 16x16 patches can touch (k_mark_tiles).  Two bitmaps per frame
  // and fine level: tiles whose spread bytes are read, tiles whose quantised pixels those spreads read.
  size_t off_tiles = 0;                  // [L-1][FL_TILE_BLOCK_WORDS] uint32 per frame
  bool lazy_capable = false;             // tile grid fits the bitmaps
  bool lazy = false;                     // this batch runs lazily (set by fl_launch_frontend)
  bool eager_env = false, poison_env = false;   // FL_EAGER_FRONTEND / FL_DEV_POISON (dev knobs, read at finalize)
  const uint8_t *lazy_bgr = nullptr;     // level-0 colour frames of the batch in flight
  // Host frames (fl_recognize_submit with FL_MEM_HOST): uploaded on a copy stream into one of two input buffers, so
  // the upload of batch i+1 overlaps the compute of batch i (the compute stream waits on the upload's event, the
  // copy stream on the event of the compute that last read the buffer it is about to overwrite).
  hipStream_t copy_stream = nullptr;
  uint8_t *d_in[2] = {nullptr, nullptr}; // max_batch * (bgr + depth) bytes each, allocated on first use
  hipEvent_t ev_up[2] = {nullptr, nullptr}, ev_read[2] = {nullptr, nullptr};
  bool read_pending[2] = {false, false};
  int in_flip = 0;
  size_t lazy_bgr_stride = 0;
  uint8_t *d_zoom = nullptr;             // fl_recognize_batch_zoom: the batch's zoomed frames (max_batch * w0*h0*5 bytes), on first use
  uint8_t *d_zoom_src = nullptr;         // and the un-zoomed host frames uploaded for it
  size_t zoom_src_bytes = 0;
  int n_pts_max = 0;
  FlBatch batch;                         // what the last call left in the workspaces: fl_batch_forget / fl_batch_record only

  int *d_icp_order = nullptr;            // ICP launch: job order (longest first) + the jobs' size estimates, 2 * max_batch ints, on first use
  // template-sharded recognition on the device: the jobs fl_select_best_batch chose (frame = -1: not this rank's)
  FlRefineJob *d_jobs = nullptr;         // max_batch, allocated on first use
  int selected_frames = 0;               // frames of the last fl_select_best_batch (0: none pending)

  // results
  fl_recognition_result *d_results = nullptr;   // max_batch
  fl_recognition_result *h_results = nullptr;   // pinned, 2 * max_batch: fl_recognize_submit alternates between the halves
  // fl_recognize_submit / _collect / _collect_previous: half h_flip holds the latest submitted batch, the other half the one
  // before it while prev_n > 0 (its frame count; 0: none, collected, or another entry point ran since).  ev_done[b] is
  // recorded after the copy into half b.  latest_open: the latest call was a fl_recognize_submit not collected yet.
  int h_flip = 0, prev_n = 0;
  bool latest_open = false;
  hipEvent_t ev_done[2] = {nullptr, nullptr};
  int icp_ev = 5;                        // the event that starts icp_ms: 5, or 7 where fl_recognize_submit recorded it before its ICP launch
  // timing
  hipEvent_t ev[FL_NUM_EVENTS] = {nullptr};   // 0..6 stage boundaries, 7 start of the ICP launches (fl_recognize_submit), 8 + 2l / 9 + 2l around the lazy work of fine level l
  fl_stage_times times;
  bool have_times = false;
  bool verify_timed = false;             // the last instances call was the verified one: ev[18], ev[19], ev[6] bound its verification (fl_dev_instances_verify_ms)
  double scan_bytes_per_frame = 0;       // SURVEY 8(d) B_tmpl summed over the bank
};

static inline void fl_batch_forget(fl_detector *det) { det->batch = FlBatch(); }
// Before an entry point other than fl_recognize_submit forgets the batch or queues work on ctx->stream: that stream waits
// for the ICP stage a pipelined fl_recognize_submit may still have in flight on the ICP stream (it writes d_results and the
// frames' ICP workspaces and reads the match lists), and the batch before the latest is no longer there to collect.
static inline int fl_pipeline_join(fl_detector *det)
{
  det->prev_n = 0;
  det->latest_open = false;
  det->set_busy[0] = det->set_busy[1] = false;
  return fl_context_join(det->ctx);
}
static inline void fl_batch_record(fl_detector *det, int n, const uint16_t *depth, size_t depth_stride, bool match_only)
{
  det->batch = FlBatch{n, depth, depth_stride, match_only};
}

// argument checks shared by entry points that return the same codes for them.  The `finalized` check is also what keeps a
// host-only detector (fl_dev_detector_create_host, context device = -1) away from every HIP call: it can never be finalized,
// and every entry point that takes a detector tests `finalized` -- here or on its own -- before its first device call.
static inline int fl_check_frames(fl_detector *det, int n_frames)     // finalized (FL_ERR_STATE), n_frames <= max_batch (FL_ERR_INVALID)
{
  if (!det->finalized) return fl_set_error(det->ctx, FL_ERR_STATE, "fl_detector_finalize first");
  if (n_frames > det->max_batch) return fl_set_error(det->ctx, FL_ERR_INVALID, "n_frames %d > max_batch %d", n_frames, det->max_batch);
  return FL_OK;
}
static inline int fl_check_intrinsics(fl_detector *det, const fl_intrinsics *K)   // the finalized image size (FL_ERR_INVALID)
{
  if (K->width == det->w0 && K->height == det->h0) return FL_OK;
  return fl_set_error(det->ctx, FL_ERR_INVALID, "intrinsics are %dx%d, detector finalized for %dx%d", K->width, K->height, det->w0, det->h0);
}

int fl_apply_class_filter(fl_detector *det);
int fl_grow_candidates(fl_detector *det, int needed);      // re-lays the frame workspaces out for >= needed candidates per frame
bool fl_grow_after_overflow(fl_detector *det, int n_frames, int attempt, int *rc);   // the synchronous entry points' retry policy
int fl_upload_frame0(fl_detector *det, const uint8_t *bgr, const uint16_t *depth, int mem);   // a single frame into workspace 0
int fl_overflow_needed(fl_detector *det, int n_frames, int *needed);   // after a sync: largest candidate count of an overflowed frame, 0 if none
void fl_update_stage_times(fl_detector *det, int n_frames, const fl_recognition_result *results);

// ---- stage launchers (defined in the per-domain .hip files) ---------------------------------
// linemod
// The input and output planes of one stage at one level, all modalities: plane m of frame f is at base + f * stride + off[m].
struct FlPlanes {
  const uint8_t *in;
  uint8_t *out;
  size_t in_stride, out_stride;
  size_t in_off[FL_MAX_MODALITIES], out_off[FL_MAX_MODALITIES];
};
// quantised images of level g in, linear memories (g.lm_off) or spread images (g.spread_off) out, in the frame workspaces
inline FlPlanes fl_level_planes(const fl_detector *det, const FlLevelGeom &g, const size_t *out_off)
{
  FlPlanes pl{det->d_ws, det->d_ws, det->ws_stride, det->ws_stride, {}, {}};
  for (int m = 0; m < FL_MAX_MODALITIES; ++m) {
    pl.in_off[m] = g.quant_off[m < det->M ? m : 0];
    pl.out_off[m] = out_off[m < det->M ? m : 0];
  }
  return pl;
}
// one launch each for the n_mod modalities of a level; tiles: see fl_launch_spread_tiles in fl_linmem.hip
int fl_launch_build_lm(fl_context *ctx, const FlPlanes &pl, int n_mod, int n_frames, int w, int h, int T);
int fl_launch_spread_tiles(fl_context *ctx, const FlPlanes &pl, int n_mod, int n_frames, int w, int h, int T, const uint32_t *tiles,
                           size_t tiles_stride);
int fl_launch_match_core(fl_detector *det, int n_frames, float threshold);   // fl_match.hip: the two above, then the three below
// fl_scan.hip; dbg (fl_similarity_maps): the raw u16 maps of pyramids [dbg_first, dbg_first + dbg_count), else null
int fl_launch_scan(fl_detector *det, int n_frames, float threshold, uint16_t *dbg, int dbg_first, int dbg_count);
int fl_launch_refine(fl_detector *det, int n_frames, float threshold);        // fl_refine.hip: every fine level, lazy levels included
int fl_launch_sort(fl_detector *det, int n_frames);                           // fl_match.hip
int fl_launch_lazy_level(fl_detector *det, int n_frames, int level);   // frontend: colour quantisation + spreads of the marked tiles
// Multi-instance grouping (fl_group_matches, fl_recognize_batch_instances): one workgroup per frame groups that frame's
// match list.  The list is `matches[0 .. n)` (frame_ws == nullptr, one frame) or the sorted list the match stage left in
// each frame workspace.  Per frame f: group_of + f * group_of_stride (one int per match, also the kernel's working storage
// for lists longer than FL_GROUP_LDS_MAX), group_size[f * G .. + G), info[f * 4 .. + 4) = {groups, matches without a group,
// FL_ERR_OVERFLOW if the frame's candidate buffers overflowed (then nothing is grouped) else 0, matches}.  With jobs != nullptr:
// jobs[(f * G + g) * h + r] = member r of group g (frame = -1 where absent) and job_idx[same] = its index in the list (-1).
#define FL_GROUP_MAX 64            // groups per frame: one lane of a wave each
#define FL_GROUP_HYP_MAX 64        // members refined per group
#define FL_GROUP_LDS_MAX 16384     // matches whose group ids the kernel keeps in LDS (one byte each)
struct FlGroupArgs {
  const fl_match *matches;
  int n;
  const uint8_t *frame_ws;
  size_t frame_stride, off_count, off_match;
  const FlPyrInfo *pyr;
  const int *class_first;
  int n_classes, n_pyr;
  int G, h;
  long long r2, r;                 // (2 * min_dist_px)^2 and 2 * min_dist_px
  int32_t *group_of;
  size_t group_of_stride;
  int32_t *group_size, *info;
  FlRefineJob *jobs;
  int32_t *job_idx;
  int write_group_of;              // 0: group_of is written only where it is the working storage (n > FL_GROUP_LDS_MAX; else it may be null)
};
int fl_launch_group_matches(fl_detector *det, int n_frames, const FlGroupArgs &a);
bool fl_instance_params_ok(const fl_instance_params *ip);   // the ranges include/fealess_hip.h states (the one check of both entry points)
#define FL_INSTANCE_PARAMS_TEXT "fl_instance_params: max_instances 1..64, min_dist_px 1..2^30, hyp_per_instance 1..64"
FlGroupArgs fl_group_args(const fl_detector *det, const fl_instance_params *ip);   // the detector's tables and the parameters; the rest zero
// Development / test aids, exported but not part of the ABI (no header declares them).
// A detector that holds its bank on the host only, on a context without a device (device = -1: no HIP call is ever made for
// it): for the entry points that never touch the device (fl_group_matches with FL_MEM_HOST).  It cannot be finalized
// (FL_ERR_STATE); fl_detector_destroy releases it and its context.
extern "C" int fl_dev_detector_create_host(int modalities, int levels, const int *T_at_level, fl_detector **out);
// k_group_matches on one caller-supplied device list WITH the job list: jobs[g * h + r] (FlRefineJob, frame 0 or -1) and
// job_idx[g * h + r], info[4]; every pointer is device memory, queued on the context's stream.
extern "C" int fl_dev_group_jobs(fl_detector *det, const fl_match *matches, int n, const fl_instance_params *ip, int32_t *group_of,
                                 int32_t *group_size, int32_t *info, void *jobs, int32_t *job_idx);
// The sort and the selection of template extraction (fl_extract.hip) on caller-supplied candidate lists, all jobs in one
// call through the launch sequence fl_extract_template_batch uses.  Everything is host memory.  Per job: the candidates as
// (raster, score > 0) pairs in the order given (the keys are packed in that order), the w x (total_px / w) image the
// features' labels are read from, num_features 1..63, depth_mode 0 (colour distance) / 1 (depth, total_px) / 2 (depth, area).
// A job with n_cand >= num_features is sorted and selected, any other is handed to the kernels as a job that cannot yield a
// template.  Out: n_out (num_features, or -1); features[64], uploaded as given and read back, so that what the kernel
// does not write returns unchanged; sorted_keys[n_cand], the job's sorted key segment, written only for a job that was sorted.
// FL_ERR_INVALID with nothing launched or written: null pointers, n_jobs < 1, num_features outside 1..63, n_cand < 0,
// a raster outside [0, total_px), a score that is not positive, a repeated raster in a depth job (its
// fractional distance never reaches 0, so too few distinct pixels would never finish), w or total_px / w beyond 65536.
struct fl_dev_select_job {
  int32_t w, total_px, num_features, depth_mode, area, n_cand;
  const int32_t *raster;
  const float *score;
  const uint8_t *labels;
  int32_t *n_out;
  fl_feature *features;
  unsigned long long *sorted_keys;
};
extern "C" int fl_dev_extract_select(fl_context *ctx, int n_jobs, const fl_dev_select_job *jobs);
// The stage between quantisation and the sort on caller-supplied QUANTIZED images: n_views (1..FL_EXTRACT_CHUNK_VIEWS) views
// of one modality (0 colour, 1 depth) and one w x h go through the launches extract_chunk runs for one pyramid level of that
// modality -- k_local_mask when any view has a mask, k_color_candidates or k_depth_candidates + k_depth_keys with the view in
// blockIdx.z and the per-view has_mask flags, the count round trip, the job records, the sort and the selection -- by the
// same functions (launch_color_level / launch_depth_level / make_job / launch_sort_select).  strong_threshold (colour; the
// library's 55), extract_threshold (depth; 2 >> level) and num_features (1..63; 63 >> level) are extract_chunk's constants
// as parameters.  Everything is host memory.  Per view, in: quantized (w * h labels), magnitude (colour: w * h floats; depth:
// ignored), mask (w * h, or null).  Out:
//   local_mask   w * h, where the view has a mask (else untouched, may be null): the border mask (colour) / the 5x5-eroded
//                mask (depth); uploaded as given and read back
//   counters     11 ints: n_cand, label_counts[8], area (counted under a depth view's mask only), n_out (num_features, or -1)
//   cand_raster, cand_score   w * h entries each, the first n_cand written: the candidates as they stood before the sort, in
//                the order the atomics gave them, with the score the candidate kernel produced (colour: the magnitude; depth:
//                the undivided distance)
//   sorted_keys  w * h entries, the first n_cand written and only for a view that was sorted (n_cand >= num_features)
//   features     64 entries, uploaded as given and read back
// What a kernel does not write returns unchanged.  FL_ERR_INVALID with nothing launched or written: null pointers, n_views
// outside 1..FL_EXTRACT_CHUNK_VIEWS, a modality other than 0 / 1, num_features outside 1..63, w or h below 1 or beyond 65536
// (the selection packs x and y into 16 bits each), more than 2^24 pixels.
struct fl_dev_extract_view {
  const uint8_t *quantized;
  const float *magnitude;
  const uint8_t *mask;
  uint8_t *local_mask;
  int32_t *counters;
  int32_t *cand_raster;
  float *cand_score;
  unsigned long long *sorted_keys;
  fl_feature *features;
};
extern "C" int fl_dev_extract_quantized(fl_context *ctx, int n_views, const fl_dev_extract_view *views, int w, int h, int modality,
                                        float strong_threshold, int extract_threshold, int num_features);
// fl_launch_quantized_orientations_mag (k_color_quantize<true, *>) on n_frames packed host frames: fl_frontend.hip
extern "C" int fl_dev_quantized_orientations_mag(fl_context *ctx, const uint8_t *bgr, int n_frames, int w, int h, float weak_threshold,
                                                 uint8_t *quantized, float *magnitude);
// frontend
int fl_launch_quantized_orientations(fl_context *ctx, const uint8_t *bgr, size_t in_stride,
                                     uint8_t *dst, size_t out_stride, int n_frames, int w, int h,
                                     float weak_threshold);
// dst1 (null: none): the half-size NN image of the normals, written by the same kernel (even w and h only)
int fl_launch_quantized_normals(fl_context *ctx, const uint16_t *depth, size_t in_stride,
                                uint8_t *dst, size_t out_stride, uint8_t *dst1, size_t out1_stride,
                                int n_frames, int w, int h, int distance_threshold,
                                int difference_threshold);
int fl_launch_pyrdown_bgr(fl_context *ctx, const uint8_t *src, size_t in_stride, uint8_t *dst,
                          size_t out_stride, int n_frames, int w, int h);
int fl_launch_resize_nn_half(fl_context *ctx, const uint8_t *src, size_t in_stride, uint8_t *dst,
                             size_t out_stride, int n_frames, int w, int h);
int fl_launch_quantized_orientations_mag(fl_context *ctx, const uint8_t *bgr, size_t in_stride, uint8_t *dst, size_t out_stride,
                                         int n_frames, int w, int h, float weak_threshold, float *mag_out);
int fl_launch_frontend(fl_detector *det, int n_frames, const uint8_t *bgr, size_t bgr_stride,
                       const uint16_t *depth, size_t depth_stride, bool allow_lazy);
int fl_launch_resize_linear_bgr8(fl_context *ctx, const uint8_t *src, int sw, int sh, uint8_t *dst, int dw, int dh);
int fl_launch_resize_linear_u16(fl_context *ctx, const uint16_t *src, int sw, int sh, uint16_t *dst, int dw, int dh);
// icp
size_t fl_icp_ws_bytes(int n_pts_max);
int fl_icp_prepare(fl_detector *det);      // fl_detector_finalize: job-order buffer, function attributes
int fl_launch_detection(fl_detector *det, int n_jobs, const fl_intrinsics *K, const fl_recognition_params *p, const uint16_t *depth,
                        size_t depth_stride, uint8_t *ws, size_t ws_stride, int ranks, const FlRefineJob *d_jobs,
                        fl_recognition_result *d_results, bool longest_first);
// The device arrays the recognition branch of the ICP kernel reads, whoever owns them: a detector's (fl_launch_detection
// fills this from the detector) or a tracker's (fl_track.hip, which always goes through the job list: frame_ws stays null).
struct FlDetectionTables {
  int w, h, n_pts_max;                   // frame size; capacity in points of one ICP workspace
  const uint8_t *frame_ws;               // frame workspaces holding the match lists (jobs without a job list)
  size_t frame_stride, off_count, off_match;
  const FlPyrInfo *pyr;
  const int *class_first;
  const float *poses;
  const uint16_t *const *depth_ptrs;
  int *icp_order;                        // 2 * order_cap ints for the longest-first order, or null
  int order_cap;
};
int fl_launch_detection_tables(fl_context *ctx, const FlDetectionTables &t, int n_jobs, const fl_intrinsics *K, const fl_recognition_params *p,
                               const uint16_t *depth, size_t depth_stride, uint8_t *ws, size_t ws_stride, int ranks, const FlRefineJob *d_jobs,
                               fl_recognition_result *d_results, bool longest_first);
// render
// fl_render_views' checks of a host mesh (FL_ERR_INVALID with `who` in the text), and its launch part for one chunk of at most
// fl_render_chunk_views(w, h) views on arrays that are already on the device: clears the chunk's depth keys (8 bytes per
// pixel and view), rasterises, resolves into the outputs that are not null (views back to back).  light: unit vector.
struct FlRenderMesh { const float *vtx, *nrm; const uint8_t *col; const int32_t *tri; int n_t; };
// One mesh of several that share a vertex array and a triangle array (a tracker's, fl_track.hip): its triangles are
// tri_first .. tri_first + n_t - 1 of the triangle array, their vertex indices already rebased into the shared vertex array.
struct FlMeshRange { int32_t tri_first, n_t; };
int fl_render_check_mesh(fl_context *ctx, const char *who, const float *vertices, const float *normals, int n_vertices,
                         const int32_t *triangles, int n_triangles);
int fl_render_chunk_views(int w, int h);
int fl_launch_render_chunk(fl_context *ctx, const FlRenderMesh &mesh, const float *d_poses13, int n_views, int w, int h, float fx, float fy,
                           float cx, float cy, const float light[3], float ambient, unsigned long long *keys, uint8_t *bgr, uint16_t *depth,
                           uint8_t *mask, int32_t *tri, const FlMeshRange *ranges = nullptr, const int32_t *mesh_of = nullptr, int max_n_t = 0);
// With ranges (device, depth-only renders: nrm, col, bgr and tri null): view v of the chunk renders the triangles of
// ranges[mesh_of[v]] (mesh_of: device, the chunk's first view at [0]) and not mesh.tri .. mesh.n_t; max_n_t = the largest n_t of
// the table, which sizes the launch.  A depth key then carries the triangle's index inside its own mesh.
// verify
// k_verify_fused (fl_verify.hip): the mesh rendered at a pose into LDS and scored against the pose's frame, one workgroup per
// pose, on arrays that are already on the device.  Pose t is the 12 floats [R|t] (row-major, mm) at pose + t * pose_stride;
// its frame is the w * h u16 at frames + frame_stride * (frame_of ? frame_of[t] : t / per_frame).  With job_idx: pose t is
// live only when job_idx[t] >= 0, res[t].found == 1 and m = mesh_of[res[t].best.class_idx] >= 0 (mesh_of is then a map from
// the detector's classes to meshes, device memory); a pose that is not live leaves its accumulator as it is.  acc:
// FL_VERIFY_ACC_BYTES per pose, written whole for a live pose.
// The mesh of a pose: mesh.tri .. mesh.n_t when `ranges` is null (one mesh, the launch as it was before there were several).
// With ranges (device): the triangles of ranges[m], m as above for a recognition slot, m = mesh_of[t] without job_idx and
// m = mesh_of[u] with skip (mesh_of null: m = 0).
// With skip (the tracker's form, which needs frame_of and takes no job_idx): the launch is over n_poses workgroups of which the
// first `split` are items 0 .. split - 1 at `pose` and the rest are items 0 .. n_poses - split - 1 again at `pose_in`; workgroup
// t of item u reads frame_of[u], is live when skip[u] == 0 and writes acc[t].  A workgroup that is not live exits at once.
#define FL_VERIFY_FUSED_PX 36864   // pixels of a band: a 144 KiB z-buffer, one workgroup per CU
constexpr size_t FL_VERIFY_ACC_BYTES = 48;   // sizeof(FlVerifyAcc), which fl_verify.hip defines and asserts
struct FlVerifyFusedJob {
  int n_poses, w, h, tau;
  float fx, fy, cx, cy;
  FlRenderMesh mesh;                            // vtx, tri and n_t are read
  const float *pose;
  int pose_stride;                              // in floats
  const uint8_t *frames;
  size_t frame_stride;                          // in bytes
  const int32_t *frame_of;
  int per_frame;
  const int32_t *job_idx;
  const fl_recognition_result *res;
  const int32_t *mesh_of;                       // per class with job_idx, else per pose / item; see above
  void *acc;
  const int32_t *skip;                          // null: the liveness rule above
  int split;
  const float *pose_in;
  const FlMeshRange *ranges;                    // null: one mesh
};
int fl_launch_verify_fused(fl_context *ctx, const FlVerifyFusedJob &j);
// the records of n_poses accumulators (k_verify_finish: rect, ratios, accepted; best = accepted), and fl_verify_params' ranges
int fl_launch_verify_finish(fl_context *ctx, int n_poses, int w, int h, const fl_verify_params &P, const void *acc, fl_verify_result *out);
bool fl_verify_params_ok(const fl_verify_params &P);
#define FL_VERIFY_PARAMS_TEXT "fl_verify_params: tau_mm 0..65535, min_model_px >= 1, finite thresholds"
