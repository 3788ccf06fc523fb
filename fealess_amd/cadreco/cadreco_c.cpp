// cadreco_c.cpp -- the flat C shim of cadreco_c.h over the C++ facade, so that callers without a C++ compiler (the test
// suite, through ctypes) can drive it.  Argument refusals come first, before anything touches the handle.
#include "cadreco_c.h"
#include "cadreco_depth_c.h"

#include "cadreco_internal.h"

#include <algorithm>
#include <cstring>

namespace {
TImageU colour_image(const unsigned char *px, int w, int h, double ts) { return TImageU{ts, (unsigned char *)px, w, h}; }
TImageU16 depth_image(const unsigned short *px, int w, int h, double ts) { return TImageU16{ts, (unsigned short *)px, w, h}; }
TCamIntrinsicParam camera(int w, int h, double fx, double fy, double cx, double cy) { return TCamIntrinsicParam{w, h, fx, fy, cx, cy, {}}; }

// res: one entry per pose, filled with the poses (and their class ids, when tags is not NULL); false: a tag that is NULL
bool fill_results(std::vector<TObjRecoResult> &res, const float *poses16, const char *const *tags)
{
  for (int i = 0; i < (int)res.size(); ++i) {
    if (tags && !tags[i]) return false;
    if (tags) res[i].strObjTag = tags[i];
    memcpy(res[i].tWorld2Cam, poses16 + 16 * i, 16 * sizeof(float));
  }
  return true;
}

int verify(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n, const float *poses16,
           const char *const *tags, float tau_mm, void *out)
{
  if (n < 0 || (n > 0 && (!poses16 || !out))) return (int)ERROR_INVALID_PARAM;
  std::vector<TObjRecoResult> res(n);
  if (!fill_results(res, poses16, tags)) return (int)ERROR_INVALID_PARAM;
  std::vector<CadRecoVerifyResult> v;
  const int rc = CadRecoVerify((CObjRecoCAD *)h, depth_image(depth, w, h_, ts), camera(w, h_, fx, fy, cx, cy), res, tau_mm, &v);
  if (rc == SUCCESS && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(CadRecoVerifyResult));
  return rc;
}

void count(const fealess::DetectorFile &df, int *n_templates, int *n_features)
{
  *n_templates = *n_features = 0;
  for (auto &c : df.classes)
    for (auto &p : c.template_pyramids) {
      ++*n_templates;
      for (auto &t : p) *n_features += (int)t.features.size();
    }
}

int recognition(void *h, const unsigned char *bgr, const unsigned short *depth, int w, int h_, double ts, int kw, int kh, double fx, double fy,
                double cx, double cy, std::vector<TObjRecoResult> &out, int *n_results)
{
  const int rc = ((CObjRecoCAD *)h)->Recognition(colour_image(bgr, w, h_, ts), depth_image(depth, w, h_, ts), camera(kw, kh, fx, fy, cx, cy), out);
  *n_results = (int)out.size();
  return rc;
}
}  // namespace

extern "C" {
void *cadreco_create(int type) { return CObjRecoCAD::Create((CObjRecoCAD::EObjRecoType)type); }
void cadreco_destroy(void *h) { CObjRecoCAD::Destroy((CObjRecoCAD *)h); }
int cadreco_add_obj(void *h, const char *dir) { return ((CObjRecoCAD *)h)->AddObj(dir); }
const char *cadreco_version() { static std::string v = CObjRecoCAD::GetVersion(); return v.c_str(); }
int cadreco_set_params(void *h, float thr, int it, float dmean, float ddiff, int mode)
{
  return cadreco_set_recognition_params((CObjRecoCAD *)h, fl_recognition_params{thr, it, dmean, ddiff, mode}) ? 0 : -1;
}
int cadreco_set_multi_hypothesis(void *h, int k, float nms_dist_mm) { return CadRecoSetMultiHypothesis((CObjRecoCAD *)h, k, nms_dist_mm); }
int cadreco_set_multi_instance(void *h, int max_instances, int min_dist_px, int hyp_per_instance)
{
  return CadRecoSetMultiInstance((CObjRecoCAD *)h, max_instances, min_dist_px, hyp_per_instance);
}
int cadreco_set_verified_pick(void *h, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio)
{
  return CadRecoSetVerifiedPick((CObjRecoCAD *)h, on, tau_mm, min_inlier_ratio, max_behind_ratio);
}
int cadreco_set_verified_tracking(void *h, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio, int keep_input)
{
  return CadRecoSetVerifiedTracking((CObjRecoCAD *)h, on, tau_mm, min_inlier_ratio, max_behind_ratio, keep_input);
}
int cadreco_recognition(void *h, const unsigned char *bgr, const unsigned short *depth, int w, int h_, double ts, int kw, int kh,
                        double fx, double fy, double cx, double cy, int *n_results, float *pose16, char *tag, int tag_cap)
{
  std::vector<TObjRecoResult> out;
  const int rc = recognition(h, bgr, depth, w, h_, ts, kw, kh, fx, fy, cx, cy, out, n_results);
  if (!out.empty()) {
    memcpy(pose16, out[0].tWorld2Cam, 16 * sizeof(float));
    snprintf(tag, tag_cap, "%s", out[0].strObjTag.c_str());
  }
  return rc;
}
int cadreco_recognition_all(void *h, const unsigned char *bgr, const unsigned short *depth, int w, int h_, double ts, int kw, int kh,
                            double fx, double fy, double cx, double cy, int *n_results, float *poses16, int cap)
{
  std::vector<TObjRecoResult> out;
  const int rc = recognition(h, bgr, depth, w, h_, ts, kw, kh, fx, fy, cx, cy, out, n_results);
  for (int i = 0; i < (int)out.size() && i < cap; ++i) memcpy(poses16 + 16 * i, out[i].tWorld2Cam, 16 * sizeof(float));
  return rc;
}

int cadreco_set_depth_camera(void *h, int on, int dw, int dh, double fx, double fy, double cx, double cy, const float *R, const float *t,
                             int fill_cracks)
{
  if ((on != 0 && on != 1) || (on && (!R || !t))) return (int)ERROR_INVALID_PARAM;
  return CadRecoSetDepthCamera((CObjRecoCAD *)h, on, camera(dw, dh, fx, fy, cx, cy), R, t, fill_cracks);
}
int cadreco_recognition_depth(void *h, const unsigned char *bgr, int w, int h_, const unsigned short *depth, int dw, int dh_, double ts,
                              double fx, double fy, double cx, double cy, int *n_results, float *pose16, char *tag, int tag_cap)
{
  if (!h || !n_results || !pose16 || !tag) return (int)ERROR_INVALID_PARAM;
  std::vector<TObjRecoResult> out;
  const int rc = ((CObjRecoCAD *)h)->Recognition(colour_image(bgr, w, h_, ts), depth_image(depth, dw, dh_, ts), camera(w, h_, fx, fy, cx, cy), out);
  *n_results = (int)out.size();
  if (!out.empty()) {
    memcpy(pose16, out[0].tWorld2Cam, 16 * sizeof(float));
    snprintf(tag, tag_cap, "%s", out[0].strObjTag.c_str());
  }
  return rc;
}

int cadreco_set_tracking_mesh(void *h, const char *obj_path, float scale)
{
  if (!obj_path) return (int)ERROR_INVALID_PARAM;
  return CadRecoSetTrackingMesh((CObjRecoCAD *)h, obj_path, scale);
}
int cadreco_set_tracking_meshes(void *h, int n, const char *const *class_ids, const char *const *obj_paths, float scale)
{
  if (n < 1 || !class_ids || !obj_paths) return (int)ERROR_INVALID_PARAM;
  std::vector<std::pair<std::string, std::string>> v;
  for (int i = 0; i < n; ++i) {
    if (!class_ids[i] || !obj_paths[i]) return (int)ERROR_INVALID_PARAM;
    v.emplace_back(class_ids[i], obj_paths[i]);
  }
  return CadRecoSetTrackingMeshes((CObjRecoCAD *)h, v, scale);
}
int cadreco_track(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                  float *poses16, int *tracked)
{
  if (n < 0 || (n > 0 && (!poses16 || !tracked))) return (int)ERROR_INVALID_PARAM;
  std::vector<TObjRecoResult> res(n);
  fill_results(res, poses16, nullptr);
  std::vector<int> trk;
  const int rc = CadRecoTrack((CObjRecoCAD *)h, depth_image(depth, w, h_, ts), camera(w, h_, fx, fy, cx, cy), res, &trk);
  for (int i = 0; i < n; ++i) {
    memcpy(poses16 + 16 * i, res[i].tWorld2Cam, 16 * sizeof(float));
    tracked[i] = i < (int)trk.size() ? trk[i] : 0;
  }
  return rc;
}
int cadreco_verify(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                   const float *poses16, float tau_mm, void *out)
{
  return verify(h, depth, w, h_, ts, fx, fy, cx, cy, n, poses16, nullptr, tau_mm, out);
}
int cadreco_verify_tagged(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                          const float *poses16, const char *const *tags, float tau_mm, void *out)
{
  if (n > 0 && !tags) return (int)ERROR_INVALID_PARAM;
  return verify(h, depth, w, h_, ts, fx, fy, cx, cy, n, poses16, tags, tau_mm, out);
}
int cadreco_arbitrate(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                      const float *poses16, const char *const *tags, float tau_mm, float max_shared_ratio, void *out)
{
  if (n < 0 || (n > 0 && (!poses16 || !out))) return (int)ERROR_INVALID_PARAM;
  std::vector<TObjRecoResult> res(n);
  if (!fill_results(res, poses16, tags)) return (int)ERROR_INVALID_PARAM;
  std::vector<CadRecoSceneResult> v;
  const int rc = CadRecoArbitrate((CObjRecoCAD *)h, depth_image(depth, w, h_, ts), camera(w, h_, fx, fy, cx, cy), res, tau_mm, max_shared_ratio, &v);
  if (rc == SUCCESS && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(CadRecoSceneResult));
  return rc;
}

int cadreco_train_views(void *h, const char *dir, const char *class_id, int n, const unsigned char *const *bgr,
                        const unsigned short *const *depth, const unsigned char *const *mask, int w, int h_, const float *poses13,
                        int levels, const int *T, int *template_of_view)
{
  if (!dir || !class_id || n < 1 || !bgr || !depth) return (int)ERROR_INVALID_PARAM;
  std::vector<TImageU> b(n), m(mask ? n : 0);
  std::vector<TImageU16> d(n);
  for (int i = 0; i < n; ++i) {
    b[i] = colour_image(bgr[i], w, h_, 0.0);
    d[i] = depth_image(depth[i], w, h_, 0.0);
    if (mask) m[i] = colour_image(mask[i], w, h_, 0.0);
  }
  std::vector<int> tov;
  const int rc = CadRecoTrainViews((CObjRecoCAD *)h, dir, class_id, n, b.data(), d.data(), mask ? m.data() : nullptr, poses13, levels, T, &tov);
  if (rc == SUCCESS && template_of_view) std::copy(tov.begin(), tov.end(), template_of_view);
  return rc;
}
int cadreco_train_mesh(void *h, const char *dir, const char *class_id, const char *obj_path, float scale, int subdivisions, int upper_hemisphere,
                       const float *distances_mm, int n_distances, int n_inplane, float inplane_deg, int levels, const int *T,
                       int *template_of_view, int cap)
{
  if (!dir || !class_id || !obj_path || !distances_mm || n_distances < 1) return (int)ERROR_INVALID_PARAM;
  const CadRecoViewSphere vs = {subdivisions, upper_hemisphere, std::vector<float>(distances_mm, distances_mm + n_distances), n_inplane, inplane_deg};
  std::vector<int> tov;
  const int rc = CadRecoTrainMesh((CObjRecoCAD *)h, dir, class_id, obj_path, scale, vs, levels, T, &tov);
  if (rc == SUCCESS && template_of_view && (int)tov.size() <= cap) std::copy(tov.begin(), tov.end(), template_of_view);
  return rc;
}

int cadreco_read_obj(const char *path, float scale, int *n_vertices, int *n_triangles, int *has_normals, float *vertices, float *normals,
                     int *triangles, int cap_vertices, int cap_triangles)
{
  if (!path) return (int)ERROR_INVALID_PARAM;
  fealess::Mesh m;
  std::string err;
  const int rc = fealess::ReadObj(path, scale, m, &err);
  if (rc != SUCCESS) return rc;
  const int nv = (int)(m.vertices.size() / 3), nt = (int)(m.triangles.size() / 3);
  if (n_vertices) *n_vertices = nv;
  if (n_triangles) *n_triangles = nt;
  if (has_normals) *has_normals = !m.normals.empty();
  if (vertices && nv <= cap_vertices) std::copy(m.vertices.begin(), m.vertices.end(), vertices);
  if (normals && nv <= cap_vertices && !m.normals.empty()) std::copy(m.normals.begin(), m.normals.end(), normals);
  if (triangles && nt <= cap_triangles) std::copy(m.triangles.begin(), m.triangles.end(), triangles);
  return SUCCESS;
}
int cadreco_read_linemod(const char *path, int *levels, int *n_classes, int *n_templates, int *n_features)
{
  fealess::DetectorFile df;
  std::string err;
  if (!fealess::ReadLinemod(path, df, &err)) return -1;
  *levels = df.pyramid_levels;
  *n_classes = (int)df.classes.size();
  count(df, n_templates, n_features);
  return 0;
}
int cadreco_read_linemod_cached(const char *path, int *from_cache, int *n_templates, int *n_features)
{
  fealess::DetectorFile df;
  std::string err;
  bool fc = false;
  if (!fealess::ReadLinemodCached(path, df, &err, &fc)) return -1;
  *from_cache = fc ? 1 : 0;
  count(df, n_templates, n_features);
  return 0;
}
int cadreco_read_png16(const char *path, unsigned short *out, int cap, int *w, int *h)
{
  std::vector<unsigned short> px;
  std::string err;
  if (!fealess::ReadPng16(path, px, *w, *h, &err)) return -1;
  if ((int)px.size() > cap) return -2;
  memcpy(out, px.data(), px.size() * 2);
  return 0;
}
int cadreco_write_png16(const char *path, const unsigned short *px, int w, int h)
{
  std::string err;
  return fealess::WritePng16(path, px, w, h, &err) ? 0 : -1;
}
}
