// fl_instances.hip -- what reads the match lists fl_match.hip leaves in the frame workspaces: the top-k export and merge of
// template-sharded recognition, and the grouping of a frame's matches into instances.
#include "fl_internal.h"
#include <limits.h>
#include <string.h>
#include <algorithm>

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
