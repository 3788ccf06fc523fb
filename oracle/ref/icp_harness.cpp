// icp_harness.cpp -- TEST INFRASTRUCTURE: the reference's own ICP sources (ICP/ICP.cpp, common.cpp, depth_to_3d.cpp,
// detection.cpp, NMS.cpp), compiled against the container-only opencv2/ stand-in beside this file, behind a small
// extern "C" surface over plain pointers that mirrors the oracle's ICP entry points (oracle/fealess_oracle.h) one to one.
// The reference's translation units are INCLUDED below by include path at build time (-I$(FEALESS_REFERENCE_ROOT)/ICP
// -I.../CadReco); no line of them is in this repository, and the library built from this file (oracle/_ref/) is never
// committed.
//
// WHAT IS PINNED by this library: the reference's text, compiled -- control flow, operand order, which sum runs over
// which vector, which threshold meets which distance: getMean without a validity check, copyPoints / transformPoints
// leaving invalid points at zero, the un-centred covariance, 3 * dist_mean against the index's squared distances and
// against cv::norm, the signed dist_diff, `continue` on a non-finite R / T after ++iter, iter = icp_it_thr on fewer
// than 3 pairs, dist_mean / nbr_inliers, detection()'s composition on default-constructed R, T when ICP refuses,
// depthTo3dNoMask's cached (x - ox) * inv_fx, rescaleDepth's NaN for depth 0, the 900 mm validity bound, NMS's 0.85 rule.
//
// WHAT STAYS UNPINNED: third-party arithmetic the reference only CALLS, restated by the stand-in (opencv2/*.hpp) or the
// oracle, item by item:
//   * cv::SVD::compute                      -> the oracle's orc_svd3 (OpenCV's JacobiSVDImpl_<float> restated; this library
//                                              links liboracle.so for it, so both sides run the same code);
//   * vt.t() * u.t()                         -> cv::gemm on CV_32F: double accumulators, k ascending, as the oracle states;
//   * cvflann::Index<L2_Simple<float> >     -> an exact 1-NN by exhaustion, freshly written: L2_Simple's float32
//                                              sequential squared distance, ties to the lowest index (FLANN's choice
//                                              among exact ties is unspecified: the tie_ cases are defined by this rule);
//   * Matx / Vec operators and products     -> OpenCV's matx.hpp semantics (s = 0; s += a(i,k) * b(k,j) in float);
//   * cv::norm(Vec3f), cv::norm(Mat, Mat)   -> squares accumulated in double, root in double;
//   * Mat::convertTo(CV_16U -> CV_32F, 1/1000.0) -> float(v) * float(1/1000.0);
//   * cv::checkRange                        -> every element finite; cv::add on Vec3f -> one float addition per element.
//
// `iter` is a local of icpCloudToCloud_Ex.  It is derived here from what the stand-in sees the loop do: every pass
// either reaches checkRange(R_optimal) or, from the second pass on, searches the index and then jumps to icp_it_thr;
// so with c = checkRange calls on a 3x3 and s = index searches, the last pass jumped iff s == c >= 1, and iter on exit is
// icp_it_thr if it jumped and c otherwise.  Per-iteration state is not exposed either: the state after pass i is the
// result of a call with icp_it_thr = i (tests/reference_cases.py runs the prefixes).
//
// Every entry point silences std::cout (the reference prints) and returns 0 or the oracle's refusal codes: -1 for clouds of
// fewer than 3 points (the reference's own return), -2 for n_model > n_ref (the reference would walk the ref iterator
// past its end: never called), -3 where a CV_Assert fired (a crop rectangle leaving the image) or the crop sizes differ
// (matToVec would walk the model iterator past its end: never called).
//
// icpCloudToCloud_Ex never frees the copy of the reference cloud it hands to the index (ICP.cpp:650): every call leaks
// 12 bytes per reference point.  That is the reference's; a leak checker on a program built from this file reports it.
#include "ICP.cpp"          // the reference's, found by include path
#include "common.cpp"
#include "depth_to_3d.cpp"
#include "detection.cpp"
#include "NMS.cpp"

#include <stdint.h>
#include <streambuf>

#include "../fealess_oracle.h"

void cv::SVD::compute(const cv::Matx33f &src, cv::Mat &w, cv::Mat &u, cv::Mat &vt)
{
  float W[3], U[9], Vt[9];
  orc_svd3(src.val, W, U, Vt);
  w.create(3, 1, CV_32FC1);
  u.create(3, 3, CV_32FC1);
  vt.create(3, 3, CV_32FC1);
  for (int i = 0; i < 3; ++i) {
    w.ptr<float>(i)[0] = W[i];
    for (int j = 0; j < 3; ++j) {
      u.ptr<float>(i)[j] = U[i * 3 + j];
      vt.ptr<float>(i)[j] = Vt[i * 3 + j];
    }
  }
}

namespace {

class NullBuf : public std::streambuf {
 protected:
  virtual int overflow(int c) { return c; }
};
struct Quiet {
  NullBuf nb;
  std::streambuf *old;
  Quiet() : old(std::cout.rdbuf(&nb)) {}
  ~Quiet() { std::cout.rdbuf(old); }
};

std::vector<cv::Vec3f> cloud(const float *p, int n)
{
  std::vector<cv::Vec3f> v((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; ++i) v[i] = cv::Vec3f(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
  return v;
}

void out_cloud(const std::vector<cv::Vec3f> &v, float *p)
{
  for (size_t i = 0; i < v.size(); ++i)
    for (int k = 0; k < 3; ++k) p[3 * i + k] = v[i][k];
}

cv::Mat depth_mat(const uint16_t *d, int w, int h)
{
  cv::Mat m(h, w, CV_16UC1);
  for (int r = 0; r < h; ++r) std::memcpy(m.ptr(r), d + (size_t)r * w, sizeof(uint16_t) * w);
  return m;
}

TCamIntrinsicParam intrinsics(int w, int h, double fx, double fy, double cx, double cy)
{
  TCamIntrinsicParam k;
  k.nWidth = w;
  k.nHeight = h;
  k.dFx = fx;
  k.dFy = fy;
  k.dCx = cx;
  k.dCy = cy;
  return k;
}

// icpCloudToCloud_Ex with the loop's final `iter` derived as the header comment states
int run_icp(const std::vector<cv::Vec3f> &ref, const std::vector<cv::Vec3f> &model, int icp_it_thr, float dist_mean_thr,
            float dist_diff_thr, orc_icp_result *res)
{
  std::memset(res, 0, sizeof(*res));
  res->n_corr_last = -1;  // not observable
  if (ref.size() >= 3 && model.size() >= 3 && model.size() > ref.size()) { res->dist_mean = -1.0f; return -2; }
  cv::Matx33f R;
  cv::Vec3f T;
  float px = 0.0f;
  cv::FealessRefCounters &cnt = cv::fealess_ref_counters();
  cnt.knn_searches = cnt.check_range_3x3 = 0;
  const float d = icpCloudToCloud_Ex(ref, model, R, T, px, icp_it_thr, dist_mean_thr, dist_diff_thr);
  std::memcpy(res->R, R.val, sizeof(res->R));
  std::memcpy(res->T, T.val, sizeof(res->T));
  res->dist_mean = d;
  res->px_ratio = px;
  const bool jumped = cnt.knn_searches >= 1 && cnt.knn_searches == cnt.check_range_3x3;
  res->iters = jumped ? icp_it_thr : (int)cnt.check_range_3x3;
  return (ref.size() < 3 || model.size() < 3) ? -1 : 0;
}

}  // namespace

extern "C" {

int ref_icp(const float *ref, int n_ref, const float *model, int n_model, int icp_it_thr, float dist_mean_thr, float dist_diff_thr,
            orc_icp_result *res)
{
  Quiet q;
  try {
    return run_icp(cloud(ref, n_ref), cloud(model, n_model), icp_it_thr, dist_mean_thr, dist_diff_thr, res);
  } catch (const cv::Exception &) { return -3; }
}

void ref_get_mean(const float *pts, int n, float out[3])
{
  cv::Vec3f c;
  getMean(cloud(pts, n), c);
  for (int k = 0; k < 3; ++k) out[k] = c[k];
}

// getL2distClouds(model, ref, dist_mean, dist_thr); n_ref >= n_model is the caller's to keep
float ref_l2dist_clouds(const float *model, int n_model, const float *ref, int n_ref, float dist_thr, float *dist_mean)
{
  return getL2distClouds(cloud(model, n_model), cloud(ref, n_ref), *dist_mean, dist_thr);
}

void ref_copy_points(const float *src, int n, float *dst)
{
  std::vector<cv::Vec3f> d;
  copyPoints(cloud(src, n), d);
  out_cloud(d, dst);
}

// in_place != 0: transformPoints(pts, pts, R, T), as the ICP loop calls it; else into a fresh vector
void ref_transform_points(const float *src, int n, const float R[9], const float T[3], float *dst, int in_place)
{
  std::vector<cv::Vec3f> s = cloud(src, n), d;
  const cv::Matx33f Rm(R[0], R[1], R[2], R[3], R[4], R[5], R[6], R[7], R[8]);
  const cv::Vec3f Tv(T[0], T[1], T[2]);
  if (in_place) transformPoints(s, s, Rm, Tv);
  else transformPoints(s, d, Rm, Tv);
  out_cloud(in_place ? s : d, dst);
}

// PointsCorresponding, the overload on a prebuilt index (the one icpCloudToCloud_Ex calls); returns the pair count
int ref_points_corresponding(const float *ref, int n_ref, const float *model, int n_model, float dist_thr, float *cor_ref, float *cor_model)
{
  std::vector<cv::Vec3f> r = cloud(ref, n_ref), m = cloud(model, n_model), cr, cm;
  std::vector<float> flat(ref, ref + 3 * (size_t)n_ref);
  cvflann::Matrix<float> data(flat.data(), (size_t)n_ref, 3);
  cvflann::Index<cvflann::L2_Simple<float> > index(data, cvflann::KDTreeSingleIndexParams(15));
  index.buildIndex();
  PointsCorresponding(r, m, index, cr, cm, dist_thr);
  out_cloud(cr, cor_ref);
  out_cloud(cm, cor_model);
  return (int)cm.size();
}

// cup_d2pc::depthTo3d on a CV_16UC1 image with K as setCamIntrinsic builds it; out = h * w * 3 floats (metres, NaN for depth 0)
int ref_depth_to_3d(const uint16_t *depth, int w, int h, double fx, double fy, double cx, double cy, float *out)
{
  try {
    cv::Mat_<float> K(3, 3, CV_32F);
    setCamIntrinsic(intrinsics(w, h, fx, fy, cx, cy), K);
    cv::Mat_<cv::Vec3f> pts;
    cup_d2pc::depthTo3d(depth_mat(depth, w, h), K, pts);
    for (int r = 0; r < h; ++r) std::memcpy(out + (size_t)r * w * 3, pts.ptr(r), sizeof(float) * 3 * w);
    return 0;
  } catch (const cv::Exception &) { return -3; }
}

// detection().  R_final and T_final are detection()'s own outputs.  n_points and icp are not outputs of it: they come
// from a second pass over the same compiled functions in the order detection() calls them (depthTo3d, scale_mat_vec3f,
// the two ROIs, matToVec, getMean, transformPoints, icpCloudToCloud_Ex).
int ref_detection(const uint16_t *model_depth, const uint16_t *scene_depth, int w, int h, double fx, double fy, double cx, double cy,
                  const int rect_model[4], const int rect_ref[4], int icp_it_thr, float dist_mean_thr, float dist_diff_thr,
                  const float r_match[9], const float t_match[3], orc_detection_result *res)
{
  Quiet q;
  std::memset(res, 0, sizeof(*res));
  if (rect_model[2] != rect_ref[2] || rect_model[3] != rect_ref[3]) return -3;
  try {
    const cv::Mat md = depth_mat(model_depth, w, h), sd = depth_mat(scene_depth, w, h);
    const TCamIntrinsicParam k = intrinsics(w, h, fx, fy, cx, cy);
    const cv::Rect_<int> rm(rect_model[0], rect_model[1], rect_model[2], rect_model[3]), rr(rect_ref[0], rect_ref[1], rect_ref[2], rect_ref[3]);
    const cv::Matx33f r(r_match[0], r_match[1], r_match[2], r_match[3], r_match[4], r_match[5], r_match[6], r_match[7], r_match[8]);
    const cv::Vec3f t(t_match[0], t_match[1], t_match[2]);
    cv::Vec3f T_final;
    cv::Matx33f R_final;
    detection(md, sd, k, rm, rr, icp_it_thr, dist_mean_thr, dist_diff_thr, r, t, 0.0f, T_final, R_final);
    std::memcpy(res->R_final, R_final.val, sizeof(res->R_final));
    std::memcpy(res->T_final, T_final.val, sizeof(res->T_final));

    cv::Mat_<cv::Vec3f> p_model, p_ref;
    cv::Mat_<float> K_ref(3, 3, CV_32F), K_model(3, 3, CV_32F);
    setCamIntrinsic(k, K_ref);
    cup_d2pc::depthTo3d(sd, K_ref, p_ref);
    initInternalMat(K_model);
    cup_d2pc::depthTo3d(md, K_model, p_model);
    scale_mat_vec3f(p_ref, 1000);
    scale_mat_vec3f(p_model, 1000);
    std::vector<cv::Vec3f> pts_ref, pts_mod;
    matToVec(p_ref(rr), p_model(rm), pts_ref, pts_mod);
    res->n_points = (int)pts_ref.size();
    cv::Vec3f mc, rc;
    getMean(pts_mod, mc);
    getMean(pts_ref, rc);
    transformPoints(pts_mod, pts_mod, cv::Matx33f::eye(), rc - mc);
    run_icp(pts_ref, pts_mod, icp_it_thr, dist_mean_thr, dist_diff_thr, &res->icp);
    return 0;
  } catch (const cv::Exception &) { return -3; }
}

// nonMaximumSuppression over n objects: object i has translation t[3 i ..], n_points[i] model points, ICP distance
// icp_dist[i] and match_class i, so that the object_id of a result is the index of the group's winner.  Writes the
// winners in the order of the results; returns their number.
int ref_nms(const float *t, const int *n_points, const float *icp_dist, int n, float th_obj_dist, int *winners)
{
  std::vector<obj_data> objs((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; ++i) {
    obj_data &o = objs[i];
    o.match_class = i;
    o.match_sim = 0.0f;
    o.r = cv::Mat(cv::Matx33f::eye());
    o.t = cv::Mat(cv::Vec3f(t[3 * i], t[3 * i + 1], t[3 * i + 2]));
    o.pts_model.resize((size_t)n_points[i]);
    o.icp_dist = icp_dist[i];
    o.check_done = false;
  }
  std::vector<PoseResult> out;
  nonMaximumSuppression(objs, th_obj_dist, out);
  for (size_t g = 0; g < out.size(); ++g) winners[g] = out[g].object_id();
  return (int)out.size();
}

}  // extern "C"
