// cadreco_train.cpp -- CadRecoTrainViews and CadRecoTrainMesh (fealess_cadreco.h): one class trained on the handle's GPU and
// written as the directory AddObj reads.  Of the handle only its fl_context is used.
#include "cadreco_internal.h"

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <sstream>

namespace {
// One trained class, built up slab by slab from fl_extract_template_batch results.
struct ClassBuilder {
  fealess::DetectorFile df;
  std::vector<int> tov;        // per view: template id or -1
  std::vector<int> view_of;    // per template id: the view

  ClassBuilder(const string &class_id, int levels, const int *T, int n_views) : tov(n_views, -1)
  {
    df.pyramid_levels = levels;
    df.T.assign(T, T + levels);
    df.modalities = {"ColorGradient", "DepthNormal"};
    df.classes.resize(1);
    df.classes[0].class_id = class_id;
  }
  // views [v0, v0 + n) of the batch: tl / fl / st as fl_extract_template_batch wrote them for those n views
  void add(int v0, int n, const fl_template *tl, const fl_feature *fl, const int32_t *st, const float *poses13)
  {
    fealess::ObjectClass &c = df.classes[0];
    const int J = 2 * df.pyramid_levels;
    for (int i = 0; i < n; ++i) {
      const int v = v0 + i;
      if (st[i] != FL_OK) continue;                                          // addTemplate returned -1: no template id
      tov[v] = (int)c.template_pyramids.size();
      view_of.push_back(v);
      std::vector<fealess::Template> pyr(J);
      for (int k = 0; k < J; ++k) {
        const fl_template &t = tl[(size_t)i * J + k];
        pyr[k] = fealess::Template{t.width, t.height, t.offset_x, t.offset_y, t.pyramid_level, {}};
        for (int j = 0; j < t.feat_count; ++j) {
          const fl_feature &f = fl[(size_t)t.feat_begin + j];
          pyr[k].features.push_back(fealess::Feature{f.x, f.y, f.label});
        }
      }
      c.template_pyramids.push_back(pyr);
      c.poses.push_back(std::vector<float>(poses13 + (size_t)13 * v, poses13 + (size_t)13 * (v + 1)));
    }
  }
  // The directory AddObj reads: depth/<template_id>.png (the view's depth x 10 in 0.1 mm, saturating), then
  // linemod_templates.yml.  depth_of(first, count, px) fills px with the w x h depths (mm) of template ids
  // [first, first + count), back to back, and returns SUCCESS or an error code.
  template <class DepthOf>
  int write(const string &dir, int w, int h, int slab, DepthOf depth_of, std::vector<int> *template_of_view) const
  {
    // the renders first, the YAML last: AddObj never sees a template file whose depth images are still missing.  An error
    // once writing has begun removes what this call created (files, and the two directories if it made them).
    const std::string ddir = dir + "/depth";
    const bool made_dir = mkdir(dir.c_str(), 0755) == 0;
    if (!made_dir && errno != EEXIST) return (int)ERROR_OPEN_FILE_FAILED;
    const bool made_ddir = mkdir(ddir.c_str(), 0755) == 0;
    const int ddir_errno = errno;
    std::vector<std::string> created;
    auto undo = [&](int rc) {
      for (const std::string &f : created) std::remove(f.c_str());
      if (made_ddir) rmdir(ddir.c_str());
      if (made_dir) rmdir(dir.c_str());
      return rc;
    };
    if (!made_ddir && ddir_errno != EEXIST) return undo((int)ERROR_OPEN_FILE_FAILED);
    auto track = [&](const std::string &f) {                                  // a file that was not there is ours to remove
      struct stat st;
      if (stat(f.c_str(), &st) != 0) created.push_back(f);
    };
    const size_t px = (size_t)w * h, n = view_of.size();
    std::vector<unsigned short> dm, d01(px);
    for (size_t first = 0; first < n; first += slab) {
      const size_t cnt = std::min(n - first, (size_t)slab);
      dm.resize(cnt * px);
      const int rc = depth_of(first, cnt, dm.data());
      if (rc != SUCCESS) return undo(rc);
      for (size_t k = 0; k < cnt; ++k) {
        const unsigned short *d = dm.data() + k * px;
        for (size_t i = 0; i < px; ++i) d01[i] = (unsigned short)std::min(65535u, 10u * d[i]);   // 0.1 mm, saturating
        std::ostringstream fn;
        fn << ddir << "/" << first + k << ".png";                           // by template id, as Recognition reads them
        track(fn.str());
        std::string err;
        if (!fealess::WritePng16(fn.str(), d01.data(), w, h, &err)) return undo((int)ERROR_OPEN_FILE_FAILED);
      }
    }
    const std::string yml = dir + "/linemod_templates.yml";
    std::remove((yml + ".flbank").c_str());                                  // a stale cache could match the new file's size and mtime
    track(yml);
    if (!fealess::WriteLinemod(df, yml)) return undo((int)ERROR_OPEN_FILE_FAILED);
    if (template_of_view) *template_of_view = tov;
    return SUCCESS;
  }
};

bool train_args_ok(const string &dir, int levels, const int *T)
{
  if (dir.empty() || !T || levels < 1 || levels > 4) return false;
  for (int l = 0; l < levels; ++l)
    if (T[l] < 1) return false;
  return true;
}
}  // namespace

int CadRecoTrainViews(CObjRecoCAD *handle, const string &dir, const string &class_id, int n_views, const TImageU *bgr,
                      const TImageU16 *depth_mm, const TImageU *mask, const float *poses13, int levels, const int *T,
                      std::vector<int> *template_of_view)
{
  fl_context *ctx = nullptr;
  if (!cadreco_context(handle, &ctx) || n_views < 1 || !bgr || !depth_mm || !poses13 || !train_args_ok(dir, levels, T)) return (int)ERROR_INVALID_PARAM;
  const int w = bgr[0].nWidth, ht = bgr[0].nHeight;
  std::vector<const uint8_t *> bp(n_views), mp(n_views, nullptr);
  std::vector<const uint16_t *> dp(n_views);
  bool any_mask = false;
  for (int v = 0; v < n_views; ++v) {
    if (!bgr[v].pData || !depth_mm[v].pData || bgr[v].nWidth != w || bgr[v].nHeight != ht || depth_mm[v].nWidth != w ||
        depth_mm[v].nHeight != ht)
      return (int)ERROR_INVALID_PARAM;
    if (mask && mask[v].pData) {
      if (mask[v].nWidth != w || mask[v].nHeight != ht) return (int)ERROR_INVALID_PARAM;
      mp[v] = mask[v].pData;
      any_mask = true;
    }
    bp[v] = bgr[v].pData;
    dp[v] = depth_mm[v].pData;
  }
  if (!ctx) return (int)ERROR_UNKNOW;
  // Detector::addTemplate for every view (linemod_train.cpp:30-91), all of them in one batched call
  const int J = 2 * levels;
  std::vector<fl_template> tl((size_t)n_views * J);
  std::vector<fl_feature> fl((size_t)n_views * J * 63);
  std::vector<int32_t> bb((size_t)n_views * 4), st(n_views);
  const int rc = fl_extract_template_batch(ctx, n_views, bp.data(), dp.data(), any_mask ? mp.data() : nullptr, w, ht, levels, FL_MEM_HOST,
                                           tl.data(), fl.data(), bb.data(), st.data());
  if (rc == FL_ERR_INVALID) return (int)ERROR_INVALID_PARAM;
  if (rc != FL_OK) return fl_fail(ctx, (int)ERROR_UNKNOW);
  ClassBuilder cb(class_id, levels, T, n_views);
  cb.add(0, n_views, tl.data(), fl.data(), st.data(), poses13);
  if (cb.view_of.empty()) return (int)ERROR_INVALID_PARAM;
  const size_t px = (size_t)w * ht;
  return cb.write(dir, w, ht, 1, [&](size_t id, size_t, unsigned short *out) {
    std::copy(depth_mm[cb.view_of[id]].pData, depth_mm[cb.view_of[id]].pData + px, out);
    return (int)SUCCESS;
  }, template_of_view);
}

int CadRecoTrainMesh(CObjRecoCAD *handle, const string &dir, const string &class_id, const string &obj_path, float scale,
                     const CadRecoViewSphere &views, int levels, const int *T, std::vector<int> *template_of_view)
{
  fl_context *ctx = nullptr;
  if (!cadreco_context(handle, &ctx) || !train_args_ok(dir, levels, T) || views.distances_mm.empty()) return (int)ERROR_INVALID_PARAM;
  fealess::Mesh mesh;
  std::string err;
  int rc = fealess::ReadObj(obj_path, scale, mesh, &err);
  if (rc != SUCCESS) {
    fprintf(stderr, "[cadreco] %s\n", err.c_str());
    return rc;
  }
  const int n_v = (int)(mesh.vertices.size() / 3), n_t = (int)(mesh.triangles.size() / 3);
  if (n_v < 3 || n_v > FL_RENDER_MAX_PRIMS || n_t > FL_RENDER_MAX_PRIMS) return (int)ERROR_INVALID_PARAM;
  int n_views = 0;
  const CadRecoViewSphere &s = views;
  if (fl_view_sphere(s.subdivisions, s.upper_hemisphere, s.distances_mm.data(), (int)s.distances_mm.size(), s.n_inplane, s.inplane_deg,
                     nullptr, 0, &n_views) != FL_OK)
    return (int)ERROR_INVALID_PARAM;
  std::vector<float> poses((size_t)n_views * 13);
  if (fl_view_sphere(s.subdivisions, s.upper_hemisphere, s.distances_mm.data(), (int)s.distances_mm.size(), s.n_inplane, s.inplane_deg,
                     poses.data(), n_views, &n_views) != FL_OK)
    return (int)ERROR_INVALID_PARAM;
  if (!ctx) return (int)ERROR_UNKNOW;
  // initInternalMat (ICP/common.cpp:358): the K detection() back-projects the template depth with (ICP/detection.cpp:35-36)
  const int w = 640, ht = 480;
  const fl_intrinsics K = {w, ht, 608.0, 608.0, 320.0, 240.0};
  const float *nrm = mesh.normals.empty() ? nullptr : mesh.normals.data();
  const int slab = FL_EXTRACT_CHUNK_VIEWS, J = 2 * levels;
  const size_t px = (size_t)w * ht;
  auto render = [&](int n, const float *p13, uint8_t *bgr, uint16_t *depth, uint8_t *mask) {
    if (fl_render_views(ctx, mesh.vertices.data(), nrm, nullptr, n_v, mesh.triangles.data(), n_t, n, p13, &K, nullptr, FL_MEM_HOST, bgr, depth,
                        mask, nullptr) != FL_OK)
      return fl_fail(ctx, (int)ERROR_UNKNOW);
    return (int)SUCCESS;
  };
  // pass 1: render and extract, a slab of views at a time; only the templates are kept
  ClassBuilder cb(class_id, levels, T, n_views);
  {
    std::vector<uint8_t> bgr(slab * px * 3), mask(slab * px);
    std::vector<uint16_t> depth(slab * px);
    std::vector<fl_template> tl((size_t)slab * J);
    std::vector<fl_feature> fl((size_t)slab * J * 63);
    std::vector<int32_t> bb((size_t)slab * 4), st(slab);
    std::vector<const uint8_t *> bp(slab), mp(slab);
    std::vector<const uint16_t *> dp(slab);
    for (int v0 = 0; v0 < n_views; v0 += slab) {
      const int n = std::min(slab, n_views - v0);
      if ((rc = render(n, poses.data() + (size_t)13 * v0, bgr.data(), depth.data(), mask.data())) != SUCCESS) return rc;
      for (int i = 0; i < n; ++i) {
        bp[i] = bgr.data() + i * px * 3;
        dp[i] = depth.data() + i * px;
        mp[i] = mask.data() + i * px;
      }
      if (fl_extract_template_batch(ctx, n, bp.data(), dp.data(), mp.data(), w, ht, levels, FL_MEM_HOST, tl.data(), fl.data(), bb.data(),
                                    st.data()) != FL_OK)
        return fl_fail(ctx, (int)ERROR_UNKNOW);
      // feat_begin counts from the slab's first view
      cb.add(v0, n, tl.data(), fl.data(), st.data(), poses.data());
    }
  }
  if (cb.view_of.empty()) return (int)ERROR_INVALID_PARAM;
  // pass 2: the depth of the views that gave a template, rendered again (the same bits) and written as PNGs
  std::vector<float> sel;
  return cb.write(dir, w, ht, slab, [&](size_t first, size_t cnt, unsigned short *out) {
    sel.resize(cnt * 13);
    for (size_t k = 0; k < cnt; ++k) std::copy(poses.data() + (size_t)13 * cb.view_of[first + k], poses.data() + (size_t)13 * (cb.view_of[first + k] + 1), sel.data() + 13 * k);
    return render((int)cnt, sel.data(), nullptr, out, nullptr);
  }, template_of_view);
}
