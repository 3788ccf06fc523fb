// obj_reco_lmicp_hip.cpp -- the CadReco facade (CObjRecoCAD / CObjRecoLmICP) on top of the C ABI
// of libfealess_hip.so.  Mirrors, call for call, CadReco/obj_reco_lmicp.cpp:47-259 and
// CadReco/obj_reco_temp.cpp:6-35 of the reference: same entry points, argument meaning, return
// codes and defaults; the OpenCV-typed private members are gone (frames stay where the caller
// put them until the ABI uploads them to HBM).  Training is cadreco_train.cpp, the C shim cadreco_c.cpp.
#include "cadreco_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <sstream>

#define PROC_IMG_WIDTH 640      // obj_reco_lmicp.cpp:6
#define TRACK_IMG_HEIGHT 480    // with PROC_IMG_WIDTH: the image the model camera (608 / 608 / 320 / 240) belongs to

namespace {
template <class T>
bool check_image(const TImage<T> &t) { return t.dTimestamp >= 0 && t.nHeight > 0 && t.nWidth > 0 && t.pData; }     // CheckTImage :32-36
bool tau_ok(float tau_mm) { return tau_mm >= 0.f && tau_mm < 65536.f; }                 // 0..65535 as an integer; NaN is not
bool refined(const fl_recognition_result &r) { return r.status == FL_OK || r.status == FL_ERR_ASSERT; }
// the facade's code for a failed tracker call
int tracker_error(int rc) { return rc == FL_ERR_INVALID ? (int)ERROR_INVALID_PARAM : (int)ERROR_UNKNOW; }

// what Recognition() reports of a refined match, appended to a frame's results; nothing for a match that was not found
void append(vector<TObjRecoResult> &out, const fl_recognition_result &r, const std::vector<std::string> &class_ids)
{
  if (!r.found) return;                                                    // vtResult stays empty, return 0 (:106-109)
  TObjRecoResult o;
  o.strObjTag = class_ids[r.best.class_idx];                               // cur_match.class_id (:112)
  memcpy(o.tWorld2Cam, r.pose, sizeof(o.tWorld2Cam));                      // Convert() (:20-30,197)
  out.push_back(o);
}

// a fl_verify_result as the initialisers of CadRecoVerifyResult, which are the first eight of CadRecoSceneResult too
#define VERIFY_FIELDS(v) (v).accepted, (v).n_model, (v).n_missing, (v).n_inlier, (v).n_front, (v).n_behind, (v).inlier_ratio, (v).behind_ratio

// depth frames registered to the colour camera (CadRecoSetDepthCamera): the pixels and the images that borrow them
struct Registered {
  std::vector<uint16_t> px;
  std::vector<TImageU16> img;
};

// Batch's frames as the C ABI takes them: 640 wide already, or src_w x src_h for the call that zooms on the device
struct Frames {
  int n, src_w, src_h;
  bool zoom;
  std::vector<const uint8_t *> bgr;
  std::vector<const uint16_t *> depth;
  fl_intrinsics k;
};

// the entries of Track, Verify and Arbitrate as the C ABI takes them: all on the one frame, each with the mesh of its tag
struct MeshCall {
  int rc, n;                     // rc: what the call returns when BeginMeshCall says there is nothing to do
  std::vector<float> poses13;
  std::vector<int32_t> frame_of, mesh_of;
  fl_intrinsics k;
  const uint16_t *frame;
};
}  // namespace

class CObjRecoLmICPHip : public CObjRecoCAD {
 public:
  typedef std::vector<std::vector<TObjRecoResult> > FrameResults;

  CObjRecoLmICPHip()
  {
    if (fl_context_create(0, &m_ctx) != FL_OK) m_ctx = nullptr;    // no GPU: every call fails, no CPU path
  }
  ~CObjRecoLmICPHip() override
  {
    if (m_tracker) fl_tracker_destroy(m_tracker);
    if (m_det) fl_detector_destroy(m_det);
    if (m_ctx) fl_context_destroy(m_ctx);
  }
  int Train(const string &, const TScanPackage &, const TTrainParam &) override { return 0; }   // stub in the reference too (:62-65)
  int ClearObj() override { return 0; }                                                          // :76-79
  int SetROI(const TImageU &) override { return 0; }                                             // :81-84
  int SetAdvancedParam(const AdvancedParam &) override { return 0; }                             // :206-209
  int GetAdvancedParam(const string &, void *) override { return 0; }                            // :211-214

  // AddObj (:67-74): loads <dir>/linemod_templates.yml; the depth renders the reference re-reads
  // from <dir>/depth/<id>.png on every frame (:156-157) are uploaded to HBM here, once.
  int AddObj(const string str_feature_path) override
  {
    if (!m_ctx) return (int)ERROR_UNKNOW;
    fealess::DetectorFile df;
    std::string err;
    if (!fealess::ReadLinemodCached(str_feature_path + "/linemod_templates.yml", df, &err, nullptr) || df.classes.empty())
      return (int)ERROR_OPEN_FILE_FAILED;                                   // numClasses() == 0 (:71-72)
    if (m_det) { fl_detector_destroy(m_det); m_det = nullptr; }
    const int M = (int)df.modalities.size(), L = df.pyramid_levels;
    // the file is untrusted input: the C ABI reads T[0..L) and one 13-float pose per pyramid
    if (M < 1 || M > 2 || L < 1 || L > 4 || (int)df.T.size() < L) return (int)ERROR_VERSION_MISMATCH;
    for (auto &c : df.classes)
      if (c.poses.size() != c.template_pyramids.size()) return (int)ERROR_VERSION_MISMATCH;
    if (fl_detector_create(m_ctx, M, L, df.T.data(), &m_det) != FL_OK) return (int)ERROR_INVALID_PARAM;
    m_class_ids.clear();
    for (auto &c : df.classes) {
      std::vector<fl_template> tl;
      std::vector<fl_feature> fl;
      std::vector<float> poses;
      for (size_t p = 0; p < c.template_pyramids.size(); ++p) {
        for (auto &t : c.template_pyramids[p]) {
          fl_template h = {t.width, t.height, t.offset_x, t.offset_y, t.pyramid_level, (int)fl.size(), (int)t.features.size()};
          for (auto &f : t.features) fl.push_back(fl_feature{f.x, f.y, f.label});
          tl.push_back(h);
        }
        for (int k = 0; k < 13; ++k) poses.push_back(k < (int)c.poses[p].size() ? c.poses[p][k] : 0.f);
      }
      if ((int)tl.size() != (int)c.template_pyramids.size() * L * M) return (int)ERROR_VERSION_MISMATCH;
      if (fl_detector_add_class(m_det, c.class_id.c_str(), (int)c.template_pyramids.size(), tl.data(), fl.data(), (int)fl.size(),
                                poses.data()) != FL_OK)
        return (int)ERROR_INVALID_PARAM;
      m_class_ids.push_back(c.class_id);
    }
    std::sort(m_class_ids.begin(), m_class_ids.end());                      // class_idx = std::map order
    // depth renders (all classes share one directory in the reference: single-class use, Q6)
    for (size_t ci = 0; ci < df.classes.size(); ++ci) {
      int cidx = (int)(std::find(m_class_ids.begin(), m_class_ids.end(), df.classes[ci].class_id) - m_class_ids.begin());
      const int n = (int)df.classes[ci].template_pyramids.size();
      for (int p = 0; p < n; ++p) {
        std::ostringstream fn;
        fn << str_feature_path << "/depth/" << p << ".png";
        std::vector<unsigned short> px;
        int w = 0, h = 0;
        if (!fealess::ReadPng16(fn.str(), px, w, h, &err)) continue;        // imread failure surfaces at Recognition time
        if (fl_detector_set_model_depths(m_det, cidx, p, 1, px.data(), w, h, FL_MEM_HOST) != FL_OK) return (int)ERROR_INVALID_PARAM;
      }
    }
    m_w = m_h = 0;
    m_path = str_feature_path;
    return 0;
  }

  int Recognition(const TImageU &tRGB, const TImageU16 &tDepth, const TCamIntrinsicParam &K, vector<TObjRecoResult> &vtResult) override
  {
    FrameResults out;
    int rc = Batch(1, &tRGB, &tDepth, K, out);
    vtResult.clear();
    if (rc == 0 && !out.empty()) vtResult = out[0];
    return rc;
  }

  // frame_rc (optional): what Recognition() would have returned for each frame; the return value is the first non-zero
  // of them, and the frames that succeeded keep their results in `out` either way
  int Batch(int n, const TImageU *rgb, const TImageU16 *depth, const TCamIntrinsicParam &K, FrameResults &out, std::vector<int> *frame_rc = nullptr)
  {
    out.clear();
    if (frame_rc) frame_rc->assign(n > 0 ? n : 0, (int)ERROR_INVALID_PARAM);
    if (!m_ctx || !m_det || n <= 0) return (int)ERROR_INVALID_PARAM;
    Registered reg;                                                          // CadRecoSetDepthCamera: depth as the sensor delivers it
    if (m_depth_camera) {
      if (const int rc = RegisterDepth(n, depth, K, reg)) return rc;
      depth = reg.img.data();
    }
    // PrepareInputData (:216-259)
    for (int i = 0; i < n; ++i) {
      if (!check_image(rgb[i]) || !check_image(depth[i])) return (int)ERROR_INVALID_PARAM;
      if (rgb[i].nHeight != K.nHeight || rgb[i].nWidth != K.nWidth || depth[i].nHeight != K.nHeight || depth[i].nWidth != K.nWidth)
        return (int)ERROR_INVALID_PARAM;
    }
    // zoom to width 640 (:229-249): w = 640, h = H * 640 / W (integer), cv::resize(INTER_LINEAR) of both images
    const int w = PROC_IMG_WIDTH, h = K.nHeight * PROC_IMG_WIDTH / K.nWidth;
    if (h <= 0) return (int)ERROR_INVALID_PARAM;
    // NB: like the reference (:190) detection() gets the caller's UN-zoomed intrinsics together with the zoomed
    // depth image (the zoomed copy only feeds SetCamIntrinsic, :236-244); identical when the input is 640 wide
    Frames f = {n, K.nWidth, K.nHeight, K.nWidth != w, std::vector<const uint8_t *>(n), std::vector<const uint16_t *>(n),
                fl_intrinsics{w, h, K.dFx, K.dFy, K.dCx, K.dCy}};
    std::vector<std::vector<uint8_t> > zb;
    std::vector<std::vector<uint16_t> > zd;
    // the single-hypothesis path zooms on the device (fl_recognize_batch_zoom); only the multi-hypothesis and multi-instance
    // extensions still take the zoomed frames through host vectors
    if (f.zoom && (m_topk > 1 || multi_instance())) {
      zb.resize(n);
      zd.resize(n);
      for (int i = 0; i < n; ++i) {
        zb[i].resize((size_t)w * h * 3);
        zd[i].resize((size_t)w * h);
        if (fl_resize_linear_bgr8(m_ctx, rgb[i].pData, K.nWidth, K.nHeight, zb[i].data(), w, h, FL_MEM_HOST) != FL_OK ||
            fl_resize_linear_u16(m_ctx, depth[i].pData, K.nWidth, K.nHeight, zd[i].data(), w, h, FL_MEM_HOST) != FL_OK)
          return fl_fail(m_ctx, (int)ERROR_INVALID_PARAM);
        f.bgr[i] = zb[i].data();
        f.depth[i] = zd[i].data();
      }
    } else {
      for (int i = 0; i < n; ++i) { f.bgr[i] = rgb[i].pData; f.depth[i] = depth[i].pData; }     // zoomed on the device when `zoom`
    }
    if (m_w != w || m_h != h || n > m_batch) {
      if (fl_detector_finalize(m_det, w, h, n > m_batch ? n : m_batch, 0) != FL_OK) return fl_fail(m_ctx, (int)ERROR_INVALID_PARAM);
      m_w = w;
      m_h = h;
      if (n > m_batch) m_batch = n;
    }
    out.resize(n);
    if (m_topk > 1) return BatchTopK(f, out, frame_rc);
    if (multi_instance()) return m_verified ? BatchVerifiedInstances(f, out, frame_rc) : BatchInstances(f, out, frame_rc);
    return BatchSingle(f, out, frame_rc);
  }

  fl_context *Context() const { return m_ctx; }
  bool multi_instance() const { return m_instances.max_instances > 1 || m_instances.hyp_per_instance > 1; }

  // CadRecoSetTrackingMesh: the mesh goes to the device once; a second call replaces the tracker
  int SetTrackingMesh(const fealess::Mesh &mesh)
  {
    if (!m_ctx) return (int)ERROR_UNKNOW;
    fl_tracker *trk = nullptr;
    const int rc = fl_tracker_create(m_ctx, mesh.vertices.data(), (int)(mesh.vertices.size() / 3), mesh.triangles.data(),
                                     (int)(mesh.triangles.size() / 3), PROC_IMG_WIDTH, TRACK_IMG_HEIGHT, 1, FEALESS_TRACK_MAX_OBJECTS,
                                     FEALESS_TRACK_MAX_CROP_PX, &trk);
    return ReplaceTracker(rc, trk, std::vector<std::string>());
  }

  // CadRecoSetTrackingMeshes: one tracker of all the meshes, mesh i for the entries tagged ids[i]; replaces the tracker
  int SetTrackingMeshes(const std::vector<std::string> &ids, const std::vector<fealess::Mesh> &meshes)
  {
    if (!m_ctx) return (int)ERROR_UNKNOW;
    if (ids.empty() || ids.size() != meshes.size()) return (int)ERROR_INVALID_PARAM;
    for (size_t i = 0; i < ids.size(); ++i)
      if (std::find(ids.begin(), ids.begin() + i, ids[i]) != ids.begin() + i) return (int)ERROR_INVALID_PARAM;   // an id twice
    std::vector<fl_mesh> ms;
    for (const fealess::Mesh &m : meshes)
      ms.push_back(fl_mesh{m.vertices.data(), m.triangles.data(), (int32_t)(m.vertices.size() / 3), (int32_t)(m.triangles.size() / 3)});
    fl_tracker *trk = nullptr;
    const int rc = fl_tracker_create_meshes(m_ctx, ms.data(), (int)ms.size(), PROC_IMG_WIDTH, TRACK_IMG_HEIGHT, 1, FEALESS_TRACK_MAX_OBJECTS,
                                            FEALESS_TRACK_MAX_CROP_PX, &trk);
    return ReplaceTracker(rc, trk, ids);
  }

  // CadRecoTrack: one fl_track_batch_meshes over the previous frame's results, each with the mesh of its strObjTag, library defaults (point-to-plane, one pass); with
  // CadRecoSetVerifiedTracking one fl_track_batch_verified, whose `tracked` and pose are the verification's
  int Track(const TImageU16 &tDepth, const TCamIntrinsicParam &K, vector<TObjRecoResult> &vtResult, vector<int> *tracked)
  {
    if (tracked) tracked->assign(vtResult.size(), 0);
    MeshCall c;
    Registered reg;
    int rrc = SUCCESS;
    const TImageU16 &frame = Aligned(tDepth, K, reg, &rrc);
    if (!BeginMeshCall(frame, K, vtResult, rrc == SUCCESS, c)) return rrc != SUCCESS ? rrc : c.rc;
    std::vector<fl_track_result> res(c.n);
    int rc;
    if (m_verified_tracking) {
      std::vector<fl_verified_track_result> vres(c.n);
      rc = fl_track_batch_verified_meshes(m_tracker, 1, &c.frame, FL_MEM_HOST, c.n, c.frame_of.data(), c.mesh_of.data(), c.poses13.data(), 0, nullptr,
                                          &c.k, nullptr, &m_tvparams, vres.data());
      for (int i = 0; i < c.n; ++i) res[i] = vres[i].track;
    } else {
      rc = fl_track_batch_meshes(m_tracker, 1, &c.frame, FL_MEM_HOST, c.n, c.frame_of.data(), c.mesh_of.data(), c.poses13.data(), &c.k, nullptr,
                                 res.data());
    }
    if (rc != FL_OK) return fl_fail(m_ctx, tracker_error(rc));
    for (int i = 0; i < c.n; ++i) {
      if (!res[i].tracked) continue;                                          // lost: the entry keeps its pose
      memcpy(vtResult[i].tWorld2Cam, res[i].pose, sizeof(vtResult[i].tWorld2Cam));
      if (tracked) (*tracked)[i] = 1;
    }
    return SUCCESS;
  }

  // CadRecoVerify: one fl_verify_batch_meshes over the entries, each with the mesh of its strObjTag, every pose its own group, the library's default gates
  int Verify(const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult, float tau_mm,
             vector<CadRecoVerifyResult> *out)
  {
    if (out) out->clear();
    MeshCall c;
    Registered reg;
    int rrc = SUCCESS;
    const TImageU16 &frame = Aligned(tDepth, K, reg, &rrc);
    if (!BeginMeshCall(frame, K, vtResult, rrc == SUCCESS && out && tau_ok(tau_mm), c)) return rrc != SUCCESS ? rrc : c.rc;
    const fl_verify_params prm = {(int32_t)tau_mm, 1, 0.f, 0.f};
    std::vector<fl_verify_result> res(c.n);
    const int rc = fl_verify_batch_meshes(m_tracker, 1, &c.frame, FL_MEM_HOST, c.n, c.frame_of.data(), c.mesh_of.data(), c.poses13.data(), 0, nullptr, &c.k, &prm,
                                          res.data());
    if (rc != FL_OK) return fl_fail(m_ctx, tracker_error(rc));
    out->resize(c.n);
    for (int i = 0; i < c.n; ++i) (*out)[i] = CadRecoVerifyResult{VERIFY_FIELDS(res[i])};
    return SUCCESS;
  }

  // CadRecoArbitrate: one fl_verify_scene_batch over the entries, the frame one scene, each entry with the mesh of its strObjTag
  int Arbitrate(const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult, float tau_mm, float max_shared_ratio,
                vector<CadRecoSceneResult> *out)
  {
    if (out) out->clear();
    const bool ratio_ok = std::isfinite(max_shared_ratio) && max_shared_ratio > 0.f && max_shared_ratio <= 1.f;
    MeshCall c;
    Registered reg;
    int rrc = SUCCESS;
    const TImageU16 &frame = Aligned(tDepth, K, reg, &rrc);
    if (!BeginMeshCall(frame, K, vtResult, rrc == SUCCESS && out && tau_ok(tau_mm) && ratio_ok, c)) return rrc != SUCCESS ? rrc : c.rc;
    const fl_scene_params prm = {{(int32_t)tau_mm, 1, 0.f, 0.f}, max_shared_ratio, 1};
    const int32_t scene_first[2] = {0, c.n};
    std::vector<fl_scene_result> res(c.n);
    const int rc = fl_verify_scene_batch(m_tracker, 1, &c.frame, FL_MEM_HOST, c.n, c.frame_of.data(), c.mesh_of.data(), c.poses13.data(), 1,
                                         scene_first, &c.k, &prm, res.data());
    if (rc != FL_OK) return fl_fail(m_ctx, tracker_error(rc));
    out->resize(c.n);
    for (int i = 0; i < c.n; ++i) (*out)[i] = CadRecoSceneResult{VERIFY_FIELDS(res[i].verify), res[i].kept, res[i].rival, res[i].n_shared};
    return SUCCESS;
  }

  // CadRecoSetVerifiedPick: needs the multi-instance mode and a tracking mesh
  int SetVerifiedPick(int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio)
  {
    if (!on) { m_verified = false; return SUCCESS; }
    if (!m_ctx || !multi_instance() || !m_tracker || !tau_ok(tau_mm) || !std::isfinite(min_inlier_ratio) || !std::isfinite(max_behind_ratio))
      return (int)ERROR_INVALID_PARAM;
    m_vparams = fl_verify_params{(int32_t)tau_mm, 1, min_inlier_ratio, max_behind_ratio};
    m_verified = true;
    return SUCCESS;
  }

  // CadRecoSetVerifiedTracking: needs a tracking mesh
  int SetVerifiedTracking(int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio, int keep_input)
  {
    if (!on) { m_verified_tracking = false; return SUCCESS; }
    if (!m_ctx || !m_tracker || !tau_ok(tau_mm) || !std::isfinite(min_inlier_ratio) || !std::isfinite(max_behind_ratio) ||
        (keep_input != 0 && keep_input != 1))
      return (int)ERROR_INVALID_PARAM;
    m_tvparams = fl_track_verify_params{{(int32_t)tau_mm, 1, min_inlier_ratio, max_behind_ratio}, keep_input, 0};
    m_verified_tracking = true;
    return SUCCESS;
  }

  // CadRecoSetDepthCamera
  int SetDepthCamera(int on, const TCamIntrinsicParam &K_depth, const float *R, const float *t, int fill_cracks)
  {
    if (on != 0 && on != 1) return (int)ERROR_INVALID_PARAM;
    if (!on) { m_depth_camera = false; return SUCCESS; }
    if (!R || !t) return (int)ERROR_INVALID_PARAM;
    const fl_intrinsics k = {K_depth.nWidth, K_depth.nHeight, K_depth.dFx, K_depth.dFy, K_depth.dCx, K_depth.dCy};
    fl_extrinsics e;
    memcpy(e.R, R, sizeof(e.R));
    memcpy(e.t, t, sizeof(e.t));
    const fl_register_params p = {fill_cracks};
    if (fl_register_check(&k, nullptr, &e, &p) != FL_OK) return (int)ERROR_INVALID_PARAM;     // the library's own rules
    if (!m_ctx) return (int)ERROR_UNKNOW;
    m_k_depth = k;
    m_depth_to_color = e;
    m_register = p;
    m_depth_camera = true;
    return SUCCESS;
  }

  // constructor defaults of obj_reco_lmicp.cpp:47-56: matching_threshold, icp_it_thr, dist_mean_thr, dist_diff_thr; then icp_mode
  fl_recognition_params m_params = {75.0f, 10, 0.5f, 0.01f, FL_ICP_PARITY};
  bool m_verified = false;   // CadRecoSetVerifiedPick; leaving the multi-instance mode clears it
  fl_verify_params m_vparams = {10, 1, 0.f, 0.f};
  bool m_verified_tracking = false;   // CadRecoSetVerifiedTracking
  fl_track_verify_params m_tvparams = {{10, 1, 0.f, 0.f}, 0, 0};
  int m_topk = 1;            // > 1: multi-hypothesis mode (CadRecoSetMultiHypothesis)
  float m_nms_dist = 20.0f;  // th_obj_dist of nonMaximumSuppression, mm
  fl_instance_params m_instances = {1, 48, 1};   // max_instances or hyp_per_instance > 1: multi-instance mode (CadRecoSetMultiInstance)

 private:
  // ---- Batch, one method per mode.  Each sets frame_rc[i] = 0 once frame i's results are known to be usable. ----
  // opt-in extension (CadRecoSetMultiHypothesis): the first m_topk matches of every frame are refined and
  // nonMaximumSuppression (ICP/NMS.cpp:6-40) keeps one hypothesis per object position, best first
  CADRECO_LOCAL int BatchTopK(const Frames &f, FrameResults &out, std::vector<int> *frame_rc)
  {
    std::vector<fl_recognition_result> res((size_t)f.n * m_topk);
    std::vector<int> cnt(f.n), win(m_topk);
    if (fl_recognize_batch_topk(m_det, f.n, f.bgr.data(), f.depth.data(), FL_MEM_HOST, &f.k, &m_params, m_topk, res.data(), cnt.data()) != FL_OK)
      return fl_fail(m_ctx, (int)ERROR_INVALID_PARAM);
    for (int i = 0; i < f.n; ++i) {
      const fl_recognition_result *r = res.data() + (size_t)i * m_topk;
      if (cnt[i] > 0 && !refined(r[0])) return (int)ERROR_INVALID_PARAM;
      if (frame_rc) (*frame_rc)[i] = 0;
      int nw = 0;
      if (fl_nms(r, cnt[i], m_nms_dist, win.data(), &nw) != FL_OK) return (int)ERROR_INVALID_PARAM;
      for (int g = 0; g < nw; ++g) append(out[i], r[win[g]], m_class_ids);
    }
    return 0;
  }

  // opt-in extension (CadRecoSetMultiInstance): the match list grouped on the device, a few members of each group
  // refined, one result per group in group order
  CADRECO_LOCAL int BatchInstances(const Frames &f, FrameResults &out, std::vector<int> *frame_rc)
  {
    const int G = m_instances.max_instances;
    std::vector<int32_t> cnt(f.n), dropped(f.n);
    std::vector<fl_instance_result> res((size_t)f.n * G);
    if (fl_recognize_batch_instances(m_det, f.n, f.bgr.data(), f.depth.data(), FL_MEM_HOST, &f.k, &m_params, &m_instances, res.data(), cnt.data(),
                                     dropped.data()) != FL_OK)
      return fl_fail(m_ctx, (int)ERROR_INVALID_PARAM);
    for (int i = 0; i < f.n; ++i) {
      if (frame_rc) (*frame_rc)[i] = 0;
      for (int g = 0; g < cnt[i]; ++g) {
        const fl_recognition_result &h = res[(size_t)i * G + g].reco;
        if (!refined(h)) return (int)ERROR_INVALID_PARAM;
        append(out[i], h, m_class_ids);
      }
    }
    return 0;
  }

  // opt-in on top of it (CadRecoSetVerifiedPick): each group's member picked by its verification against the tracking mesh,
  // and only the accepted instances returned
  // With CadRecoSetTrackingMeshes every class whose id has a mesh is verified against it; the groups of the other classes
  // come back as the multi-instance mode returns them.
  CADRECO_LOCAL int BatchVerifiedInstances(const Frames &f, FrameResults &out, std::vector<int> *frame_rc)
  {
    const int G = m_instances.max_instances;
    std::vector<int32_t> cnt(f.n), dropped(f.n);
    std::vector<fl_verified_instance_result> vres((size_t)f.n * G);
    const fl_instance_verify_params vp = {m_vparams, -1, 0};
    std::vector<int32_t> mesh_of_class;
    for (const std::string &id : m_class_ids) mesh_of_class.push_back(MeshOfTag(id));
    if (fl_recognize_batch_instances_verified_meshes(m_det, m_tracker, f.n, f.bgr.data(), f.depth.data(), FL_MEM_HOST, &f.k, &m_params, &m_instances,
                                                     &vp, mesh_of_class.data(), vres.data(), cnt.data(), dropped.data(), nullptr) != FL_OK)
      return fl_fail(m_ctx, (int)ERROR_INVALID_PARAM);
    for (int i = 0; i < f.n; ++i) {
      if (frame_rc) (*frame_rc)[i] = 0;
      for (int g = 0; g < cnt[i]; ++g) {
        const fl_verified_instance_result &v = vres[(size_t)i * G + g];
        if (!refined(v.inst.reco)) return (int)ERROR_INVALID_PARAM;
        if (v.verified && !v.verify.accepted) continue;
        append(out[i], v.inst.reco, m_class_ids);
      }
    }
    return 0;
  }

  // the reference's Recognition(): matches[0] of every frame
  CADRECO_LOCAL int BatchSingle(const Frames &f, FrameResults &out, std::vector<int> *frame_rc)
  {
    std::vector<fl_recognition_result> res(f.n);
    const int rc = f.zoom ? fl_recognize_batch_zoom(m_det, f.n, f.bgr.data(), f.depth.data(), f.src_w, f.src_h, FL_MEM_HOST, &f.k, &m_params, res.data())
                          : fl_recognize_batch(m_det, f.n, f.bgr.data(), f.depth.data(), FL_MEM_HOST, &f.k, &m_params, res.data());
    if (rc != FL_OK) return fl_fail(m_ctx, (int)ERROR_INVALID_PARAM);
    int first_rc = 0;
    for (int i = 0; i < f.n; ++i) {
      // match() returned -1 / ROI assert / candidate buffers at a hard cap: that frame fails, the others keep their results
      const int frc = res[i].status != FL_OK ? (int)ERROR_INVALID_PARAM : 0;
      if (frame_rc) (*frame_rc)[i] = frc;
      if (frc) { if (!first_rc) first_rc = frc; continue; }
      append(out[i], res[i], m_class_ids);
    }
    return first_rc;
  }

  // While a depth camera is set: the n depth images, each of K_depth's size, registered to the camera K in one call; reg.img are
  // the images to go on with.  SUCCESS, or the code the entry point returns.
  CADRECO_LOCAL int RegisterDepth(int n, const TImageU16 *depth, const TCamIntrinsicParam &K, Registered &reg) const
  {
    if (!depth || K.nWidth < 1 || K.nHeight < 1 || K.nWidth > FL_RENDER_MAX_DIM || K.nHeight > FL_RENDER_MAX_DIM) return (int)ERROR_INVALID_PARAM;
    for (int i = 0; i < n; ++i)
      if (!check_image(depth[i]) || depth[i].nWidth != m_k_depth.width || depth[i].nHeight != m_k_depth.height) return (int)ERROR_INVALID_PARAM;
    const size_t px = (size_t)K.nWidth * K.nHeight;
    reg.px.resize(px * n);
    std::vector<const uint16_t *> in(n);
    std::vector<uint16_t *> out(n);
    for (int i = 0; i < n; ++i) {
      in[i] = depth[i].pData;
      out[i] = reg.px.data() + px * i;
      reg.img.push_back(TImageU16{depth[i].dTimestamp, out[i], K.nWidth, K.nHeight});
    }
    const fl_intrinsics kc = {K.nWidth, K.nHeight, K.dFx, K.dFy, K.dCx, K.dCy};
    const int rc = fl_register_depth_batch(m_ctx, n, in.data(), FL_MEM_HOST, &m_k_depth, &kc, &m_depth_to_color, &m_register, out.data());
    if (rc == FL_ERR_INVALID) return (int)ERROR_INVALID_PARAM;
    return rc == FL_OK ? (int)SUCCESS : fl_fail(m_ctx, (int)ERROR_UNKNOW);
  }

  // the frame Track, Verify and Arbitrate go on with: tDepth, or while a depth camera is set its registration to K, kept in reg
  // (*rc: RegisterDepth's code; on a failure tDepth itself comes back and the caller returns *rc)
  CADRECO_LOCAL const TImageU16 &Aligned(const TImageU16 &tDepth, const TCamIntrinsicParam &K, Registered &reg, int *rc) const
  {
    if (!m_depth_camera) return tDepth;
    *rc = RegisterDepth(1, &tDepth, K, reg);
    return *rc == SUCCESS ? reg.img[0] : tDepth;
  }

  // the tail of SetTrackingMesh and SetTrackingMeshes: rc and trk of the create call; ids: the class id of every mesh, or none
  CADRECO_LOCAL int ReplaceTracker(int rc, fl_tracker *trk, const std::vector<std::string> &ids)
  {
    if (rc == FL_ERR_INVALID) return (int)ERROR_INVALID_PARAM;
    if (rc != FL_OK) return fl_fail(m_ctx, (int)ERROR_UNKNOW);
    if (m_tracker) fl_tracker_destroy(m_tracker);
    m_tracker = trk;
    m_mesh_ids = ids;
    return SUCCESS;
  }

  // the tracker's mesh for an entry tagged `tag`: after CadRecoSetTrackingMesh the one mesh whatever the tag, after
  // CadRecoSetTrackingMeshes the tag's mesh or -1
  int MeshOfTag(const std::string &tag) const
  {
    if (m_mesh_ids.empty()) return 0;
    const auto it = std::find(m_mesh_ids.begin(), m_mesh_ids.end(), tag);
    return it == m_mesh_ids.end() ? -1 : (int)(it - m_mesh_ids.begin());
  }

  // What Track, Verify and Arbitrate begin with.  In this order: the handle has a tracker, the frame is a valid 640 x 480 image,
  // no more than FEALESS_TRACK_MAX_OBJECTS entries, and args_ok, the caller's own argument checks: ERROR_INVALID_PARAM; no entry:
  // SUCCESS; an entry whose tag has no mesh: ERROR_INVALID_PARAM.  false: return c.rc; true: c holds the call's arguments.
  CADRECO_LOCAL bool BeginMeshCall(const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult, bool args_ok,
                                   MeshCall &c) const
  {
    c.rc = (int)ERROR_INVALID_PARAM;
    if (!m_ctx || !m_tracker || !check_image(tDepth) || tDepth.nWidth != PROC_IMG_WIDTH || tDepth.nHeight != TRACK_IMG_HEIGHT ||
        (int)vtResult.size() > FEALESS_TRACK_MAX_OBJECTS || !args_ok)
      return false;
    c.n = (int)vtResult.size();
    if (c.n == 0) { c.rc = SUCCESS; return false; }
    c.poses13 = std::vector<float>((size_t)c.n * 13, 0.f);
    c.frame_of = std::vector<int32_t>(c.n, 0);
    for (int i = 0; i < c.n; ++i) {
      c.mesh_of.push_back(MeshOfTag(vtResult[i].strObjTag));
      if (c.mesh_of.back() < 0) return false;                                 // a tag without a mesh
      memcpy(c.poses13.data() + (size_t)13 * i, vtResult[i].tWorld2Cam, 12 * sizeof(float));
    }
    c.k = fl_intrinsics{PROC_IMG_WIDTH, TRACK_IMG_HEIGHT, K.dFx, K.dFy, K.dCx, K.dCy};
    c.frame = tDepth.pData;
    return true;
  }

  fl_context *m_ctx = nullptr;
  fl_detector *m_det = nullptr;
  std::vector<std::string> m_class_ids;
  std::string m_path;
  int m_w = 0, m_h = 0, m_batch = 1;
  fl_tracker *m_tracker = nullptr;   // CadRecoSetTrackingMesh, CadRecoSetTrackingMeshes
  bool m_depth_camera = false;       // CadRecoSetDepthCamera: depth images arrive in the depth sensor's own camera
  fl_intrinsics m_k_depth = {0, 0, 0.0, 0.0, 0.0, 0.0};
  fl_extrinsics m_depth_to_color = {{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}};
  fl_register_params m_register = {1};
  std::vector<std::string> m_mesh_ids;   // CadRecoSetTrackingMeshes: the class id of every mesh of the tracker; empty: one mesh for every tag
};

// ---- factory (CadReco/obj_reco_temp.cpp:6-35) -------------------------------------------------
#define LIB_VERSION "3.1.1-hip"
string CObjRecoCAD::GetVersion()
{
  std::stringstream s;
  s << "CAD-based 3D Object Recognition (MI355X / HIP build). Version " << LIB_VERSION << " Compile Time: " << __DATE__ << " " << __TIME__;
  return s.str();
}

CObjRecoCAD *CObjRecoCAD::Create(EObjRecoType eType)
{
  switch (eType) {
    case EObjReco_LmICP: return new CObjRecoLmICPHip();
    default: break;                // EObjReco_FEATURE / BB8 / PoseNet: unsupported in the reference as well
  }
  return nullptr;
}

void CObjRecoCAD::Destroy(CObjRecoCAD *pHandle) { delete pHandle; }

// ---- the CadReco* extensions on a handle of this library; any other handle (or none): nullptr ----
static CObjRecoLmICPHip *handle_of(CObjRecoCAD *handle) { return dynamic_cast<CObjRecoLmICPHip *>(handle); }

bool cadreco_context(CObjRecoCAD *handle, fl_context **ctx)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  if (h) *ctx = h->Context();
  return h != nullptr;
}

bool cadreco_set_recognition_params(CObjRecoCAD *handle, const fl_recognition_params &params)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  if (h) h->m_params = params;
  return h != nullptr;
}

int CadRecoRecognitionBatch(CObjRecoCAD *handle, int n_frames, const TImageU *rgb, const TImageU16 *depth,
                            const TCamIntrinsicParam &K, std::vector<std::vector<TObjRecoResult> > &out, std::vector<int> *frame_rc)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  return h ? h->Batch(n_frames, rgb, depth, K, out, frame_rc) : (int)ERROR_INVALID_PARAM;
}

int CadRecoSetMultiHypothesis(CObjRecoCAD *handle, int k, float nms_dist_mm)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  if (!h || k < 1 || k > 1024 || !(nms_dist_mm >= 0.f)) return (int)ERROR_INVALID_PARAM;
  h->m_topk = k;
  h->m_nms_dist = nms_dist_mm;
  h->m_instances.max_instances = h->m_instances.hyp_per_instance = 1;      // the two modes exclude each other
  h->m_verified = false;
  return 0;
}

int CadRecoSetMultiInstance(CObjRecoCAD *handle, int max_instances, int min_dist_px, int hyp_per_instance)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  if (!h || max_instances < 1 || max_instances > 64 || min_dist_px < 1 || min_dist_px > (1 << 30) || hyp_per_instance < 1 || hyp_per_instance > 64)
    return (int)ERROR_INVALID_PARAM;
  h->m_instances = fl_instance_params{max_instances, min_dist_px, hyp_per_instance};
  h->m_topk = 1;                                                             // the two modes exclude each other
  if (!h->multi_instance()) h->m_verified = false;
  return 0;
}

int CadRecoSetVerifiedPick(CObjRecoCAD *handle, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  return h ? h->SetVerifiedPick(on, tau_mm, min_inlier_ratio, max_behind_ratio) : (int)ERROR_INVALID_PARAM;
}

int CadRecoSetVerifiedTracking(CObjRecoCAD *handle, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio, int keep_input)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  return h ? h->SetVerifiedTracking(on, tau_mm, min_inlier_ratio, max_behind_ratio, keep_input) : (int)ERROR_INVALID_PARAM;
}

// fealess::ReadObj with its message on stderr
static int read_tracking_mesh(const string &obj_path, float scale, fealess::Mesh &mesh)
{
  std::string err;
  const int rc = fealess::ReadObj(obj_path, scale, mesh, &err);
  if (rc != SUCCESS) fprintf(stderr, "[cadreco] %s\n", err.c_str());
  return rc;
}

int CadRecoSetTrackingMesh(CObjRecoCAD *handle, const string &obj_path, float scale)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  fealess::Mesh mesh;
  const int rc = read_tracking_mesh(obj_path, scale, mesh);
  return rc != SUCCESS ? rc : h->SetTrackingMesh(mesh);
}

int CadRecoSetTrackingMeshes(CObjRecoCAD *handle, const vector<std::pair<string, string>> &class_id_and_obj_path, float scale)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  std::vector<std::string> ids;
  std::vector<fealess::Mesh> meshes(class_id_and_obj_path.size());
  for (size_t i = 0; i < class_id_and_obj_path.size(); ++i) {
    const int rc = read_tracking_mesh(class_id_and_obj_path[i].second, scale, meshes[i]);
    if (rc != SUCCESS) return rc;
    ids.push_back(class_id_and_obj_path[i].first);
  }
  return h->SetTrackingMeshes(ids, meshes);
}

int CadRecoTrack(CObjRecoCAD *handle, const TImageU16 &tDepth, const TCamIntrinsicParam &K, vector<TObjRecoResult> &vtResult,
                 vector<int> *tracked)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  return h ? h->Track(tDepth, K, vtResult, tracked) : (int)ERROR_INVALID_PARAM;
}

int CadRecoVerify(CObjRecoCAD *handle, const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult,
                  float tau_mm, vector<CadRecoVerifyResult> *out)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  return h ? h->Verify(tDepth, K, vtResult, tau_mm, out) : (int)ERROR_INVALID_PARAM;
}

int CadRecoArbitrate(CObjRecoCAD *handle, const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult,
                     float tau_mm, float max_shared_ratio, vector<CadRecoSceneResult> *out)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  return h ? h->Arbitrate(tDepth, K, vtResult, tau_mm, max_shared_ratio, out) : (int)ERROR_INVALID_PARAM;
}

int CadRecoSetDepthCamera(CObjRecoCAD *handle, int on, const TCamIntrinsicParam &K_depth, const float R[9], const float t[3], int fill_cracks)
{
  CObjRecoLmICPHip *h = handle_of(handle);
  return h ? h->SetDepthCamera(on, K_depth, R, t, fill_cracks) : (int)ERROR_INVALID_PARAM;
}
