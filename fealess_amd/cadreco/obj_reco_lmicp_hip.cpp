// obj_reco_lmicp_hip.cpp -- the CadReco facade (CObjRecoCAD / CObjRecoLmICP) on top of the C ABI
// of libfealess_hip.so.  Mirrors, call for call, CadReco/obj_reco_lmicp.cpp:47-259 and
// CadReco/obj_reco_temp.cpp:6-35 of the reference: same entry points, argument meaning, return
// codes and defaults; the OpenCV-typed private members are gone (frames stay where the caller
// put them until the ABI uploads them to HBM).
#include "fealess_cadreco.h"
#include "../../include/fealess_hip.h"

#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <sstream>

#define PROC_IMG_WIDTH 640      // obj_reco_lmicp.cpp:6
#define TRACK_IMG_HEIGHT 480    // with PROC_IMG_WIDTH: the image the model camera (608 / 608 / 320 / 240) belongs to

namespace {
int check_image_u8(const TImageU &t) { return t.dTimestamp >= 0 && t.nHeight > 0 && t.nWidth > 0 && t.pData; }     // CheckTImage :32-36
int check_image_u16(const TImageU16 &t) { return t.dTimestamp >= 0 && t.nHeight > 0 && t.nWidth > 0 && t.pData; }
}  // namespace

class CObjRecoLmICPHip : public CObjRecoCAD {
 public:
  CObjRecoLmICPHip()
  {
    // constructor defaults of obj_reco_lmicp.cpp:47-56
    m_params.matching_threshold = 75.0f;
    m_params.icp_it_thr = 10;
    m_params.dist_mean_thr = 0.5f;
    m_params.dist_diff_thr = 0.01f;
    m_params.icp_mode = FL_ICP_PARITY;
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
    std::vector<std::vector<unsigned short> > depth_banks;
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
    std::vector<std::vector<TObjRecoResult> > out;
    int rc = Batch(1, &tRGB, &tDepth, K, out);
    vtResult.clear();
    if (rc == 0 && !out.empty()) vtResult = out[0];
    return rc;
  }

  // frame_rc (optional): what Recognition() would have returned for each frame; the return value is the first non-zero
  // of them, and the frames that succeeded keep their results in `out` either way
  int Batch(int n, const TImageU *rgb, const TImageU16 *depth, const TCamIntrinsicParam &K, std::vector<std::vector<TObjRecoResult> > &out,
            std::vector<int> *frame_rc = nullptr)
  {
    out.clear();
    if (frame_rc) frame_rc->assign(n > 0 ? n : 0, (int)ERROR_INVALID_PARAM);
    if (!m_ctx || !m_det || n <= 0) return (int)ERROR_INVALID_PARAM;
    // PrepareInputData (:216-259)
    for (int i = 0; i < n; ++i) {
      if (!check_image_u8(rgb[i]) || !check_image_u16(depth[i])) return (int)ERROR_INVALID_PARAM;
      if (rgb[i].nHeight != K.nHeight || rgb[i].nWidth != K.nWidth || depth[i].nHeight != K.nHeight || depth[i].nWidth != K.nWidth)
        return (int)ERROR_INVALID_PARAM;
    }
    // zoom to width 640 (:229-249): w = 640, h = H * 640 / W (integer), cv::resize(INTER_LINEAR) of both images
    const int w = PROC_IMG_WIDTH, h = K.nHeight * PROC_IMG_WIDTH / K.nWidth;
    if (h <= 0) return (int)ERROR_INVALID_PARAM;
    std::vector<const uint8_t *> bp(n);
    std::vector<const uint16_t *> dp(n);
    std::vector<std::vector<uint8_t> > zb;
    std::vector<std::vector<uint16_t> > zd;
    const bool zoom = K.nWidth != w;
    // the single-hypothesis path zooms on the device (fl_recognize_batch_zoom); only the multi-hypothesis and multi-instance
    // extensions still take the zoomed frames through host vectors
    const bool multi_instance = m_instances.max_instances > 1 || m_instances.hyp_per_instance > 1;
    if (zoom && (m_topk > 1 || multi_instance)) {
      zb.resize(n);
      zd.resize(n);
      for (int i = 0; i < n; ++i) {
        zb[i].resize((size_t)w * h * 3);
        zd[i].resize((size_t)w * h);
        if (fl_resize_linear_bgr8(m_ctx, rgb[i].pData, K.nWidth, K.nHeight, zb[i].data(), w, h, FL_MEM_HOST) != FL_OK ||
            fl_resize_linear_u16(m_ctx, depth[i].pData, K.nWidth, K.nHeight, zd[i].data(), w, h, FL_MEM_HOST) != FL_OK) {
          fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
          return (int)ERROR_INVALID_PARAM;
        }
        bp[i] = zb[i].data();
        dp[i] = zd[i].data();
      }
    } else {
      for (int i = 0; i < n; ++i) { bp[i] = rgb[i].pData; dp[i] = depth[i].pData; }     // zoomed on the device when `zoom`
    }
    if (m_w != w || m_h != h || n > m_batch) {
      if (fl_detector_finalize(m_det, w, h, n > m_batch ? n : m_batch, 0) != FL_OK) {
        fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
        return (int)ERROR_INVALID_PARAM;
      }
      m_w = w;
      m_h = h;
      if (n > m_batch) m_batch = n;
    }
    // NB: like the reference (:190) detection() gets the caller's UN-zoomed intrinsics together with the zoomed
    // depth image (the zoomed copy only feeds SetCamIntrinsic, :236-244); identical when the input is 640 wide
    fl_intrinsics k = {w, h, K.dFx, K.dFy, K.dCx, K.dCy};
    out.resize(n);
    if (m_topk > 1) {
      // opt-in extension (CadRecoSetMultiHypothesis): the first m_topk matches of every frame are refined and
      // nonMaximumSuppression (ICP/NMS.cpp:6-40) keeps one hypothesis per object position, best first
      std::vector<fl_recognition_result> res((size_t)n * m_topk);
      std::vector<int> cnt(n), win(m_topk);
      if (fl_recognize_batch_topk(m_det, n, bp.data(), dp.data(), FL_MEM_HOST, &k, &m_params, m_topk, res.data(), cnt.data()) != FL_OK) {
        fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
        return (int)ERROR_INVALID_PARAM;
      }
      for (int i = 0; i < n; ++i) {
        const fl_recognition_result *r = res.data() + (size_t)i * m_topk;
        if (cnt[i] > 0 && r[0].status != FL_OK && r[0].status != FL_ERR_ASSERT) return (int)ERROR_INVALID_PARAM;
        if (frame_rc) (*frame_rc)[i] = 0;
        int nw = 0;
        if (fl_nms(r, cnt[i], m_nms_dist, win.data(), &nw) != FL_OK) return (int)ERROR_INVALID_PARAM;
        for (int g = 0; g < nw; ++g) {
          const fl_recognition_result &h = r[win[g]];
          if (!h.found) continue;
          TObjRecoResult o;
          o.strObjTag = m_class_ids[h.best.class_idx];
          memcpy(o.tWorld2Cam, h.pose, sizeof(o.tWorld2Cam));
          out[i].push_back(o);
        }
      }
      return 0;
    }
    if (multi_instance) {
      // opt-in extension (CadRecoSetMultiInstance): the match list grouped on the device, a few members of each group
      // refined, one result per group in group order
      const int G = m_instances.max_instances;
      std::vector<int32_t> cnt(n), dropped(n);
      if (m_verified) {
        // opt-in on top of it (CadRecoSetVerifiedPick): each group's member picked by its verification against the tracking mesh,
        // and only the accepted instances returned
        // With CadRecoSetTrackingMeshes every class whose id has a mesh is verified against it; the groups of the other classes
        // come back as the multi-instance mode returns them.
        std::vector<fl_verified_instance_result> vres((size_t)n * G);
        const fl_instance_verify_params vp = {m_vparams, -1, 0};
        std::vector<int32_t> mesh_of_class;
        for (const std::string &id : m_class_ids) mesh_of_class.push_back(MeshOfTag(id));
        if (fl_recognize_batch_instances_verified_meshes(m_det, m_tracker, n, bp.data(), dp.data(), FL_MEM_HOST, &k, &m_params, &m_instances, &vp,
                                                         mesh_of_class.data(), vres.data(), cnt.data(), dropped.data(), nullptr) != FL_OK) {
          fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
          return (int)ERROR_INVALID_PARAM;
        }
        for (int i = 0; i < n; ++i) {
          if (frame_rc) (*frame_rc)[i] = 0;
          for (int g = 0; g < cnt[i]; ++g) {
            const fl_verified_instance_result &v = vres[(size_t)i * G + g];
            const fl_recognition_result &h = v.inst.reco;
            if (h.status != FL_OK && h.status != FL_ERR_ASSERT) return (int)ERROR_INVALID_PARAM;
            if (!h.found || (v.verified && !v.verify.accepted)) continue;
            TObjRecoResult o;
            o.strObjTag = m_class_ids[h.best.class_idx];
            memcpy(o.tWorld2Cam, h.pose, sizeof(o.tWorld2Cam));
            out[i].push_back(o);
          }
        }
        return 0;
      }
      std::vector<fl_instance_result> res((size_t)n * G);
      if (fl_recognize_batch_instances(m_det, n, bp.data(), dp.data(), FL_MEM_HOST, &k, &m_params, &m_instances, res.data(), cnt.data(),
                                       dropped.data()) != FL_OK) {
        fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
        return (int)ERROR_INVALID_PARAM;
      }
      for (int i = 0; i < n; ++i) {
        if (frame_rc) (*frame_rc)[i] = 0;
        for (int g = 0; g < cnt[i]; ++g) {
          const fl_recognition_result &h = res[(size_t)i * G + g].reco;
          if (h.status != FL_OK && h.status != FL_ERR_ASSERT) return (int)ERROR_INVALID_PARAM;
          if (!h.found) continue;
          TObjRecoResult o;
          o.strObjTag = m_class_ids[h.best.class_idx];
          memcpy(o.tWorld2Cam, h.pose, sizeof(o.tWorld2Cam));
          out[i].push_back(o);
        }
      }
      return 0;
    }
    std::vector<fl_recognition_result> res(n);
    const int rc = zoom ? fl_recognize_batch_zoom(m_det, n, bp.data(), dp.data(), K.nWidth, K.nHeight, FL_MEM_HOST, &k, &m_params, res.data())
                        : fl_recognize_batch(m_det, n, bp.data(), dp.data(), FL_MEM_HOST, &k, &m_params, res.data());
    if (rc != FL_OK) {
      fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
      return (int)ERROR_INVALID_PARAM;
    }
    int first_rc = 0;
    for (int i = 0; i < n; ++i) {
      // match() returned -1 / ROI assert / candidate buffers at a hard cap: that frame fails, the others keep their results
      const int frc = res[i].status != FL_OK ? (int)ERROR_INVALID_PARAM : 0;
      if (frame_rc) (*frame_rc)[i] = frc;
      if (frc) { if (!first_rc) first_rc = frc; continue; }
      if (!res[i].found) continue;                                          // vtResult stays empty, return 0 (:106-109)
      TObjRecoResult r;
      r.strObjTag = m_class_ids[res[i].best.class_idx];                     // cur_match.class_id (:112)
      memcpy(r.tWorld2Cam, res[i].pose, sizeof(r.tWorld2Cam));              // Convert() (:20-30,197)
      out[i].push_back(r);
    }
    return first_rc;
  }

  fl_context *Context() const { return m_ctx; }

  // CadRecoSetTrackingMesh: the mesh goes to the device once; a second call replaces the tracker
  int SetTrackingMesh(const fealess::Mesh &mesh)
  {
    if (!m_ctx) return (int)ERROR_UNKNOW;
    fl_tracker *trk = nullptr;
    const int rc = fl_tracker_create(m_ctx, mesh.vertices.data(), (int)(mesh.vertices.size() / 3), mesh.triangles.data(),
                                     (int)(mesh.triangles.size() / 3), PROC_IMG_WIDTH, TRACK_IMG_HEIGHT, 1, FEALESS_TRACK_MAX_OBJECTS,
                                     FEALESS_TRACK_MAX_CROP_PX, &trk);
    if (rc == FL_ERR_INVALID) return (int)ERROR_INVALID_PARAM;
    if (rc != FL_OK) {
      fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
      return (int)ERROR_UNKNOW;
    }
    if (m_tracker) fl_tracker_destroy(m_tracker);
    m_tracker = trk;
    m_mesh_ids.clear();
    return SUCCESS;
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
    if (rc == FL_ERR_INVALID) return (int)ERROR_INVALID_PARAM;
    if (rc != FL_OK) {
      fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
      return (int)ERROR_UNKNOW;
    }
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
  // one mesh index per entry; false: an entry's tag has no mesh
  bool MeshesOf(const vector<TObjRecoResult> &vtResult, std::vector<int32_t> &mesh_of) const
  {
    mesh_of.clear();
    for (const TObjRecoResult &r : vtResult) {
      mesh_of.push_back(MeshOfTag(r.strObjTag));
      if (mesh_of.back() < 0) return false;
    }
    return true;
  }

  // CadRecoTrack: one fl_track_batch_meshes over the previous frame's results, each with the mesh of its strObjTag, library defaults (point-to-plane, one pass); with
  // CadRecoSetVerifiedTracking one fl_track_batch_verified, whose `tracked` and pose are the verification's
  int Track(const TImageU16 &tDepth, const TCamIntrinsicParam &K, vector<TObjRecoResult> &vtResult, vector<int> *tracked)
  {
    if (tracked) tracked->assign(vtResult.size(), 0);
    if (!m_ctx || !m_tracker || !check_image_u16(tDepth) || tDepth.nWidth != PROC_IMG_WIDTH || tDepth.nHeight != TRACK_IMG_HEIGHT ||
        (int)vtResult.size() > FEALESS_TRACK_MAX_OBJECTS)
      return (int)ERROR_INVALID_PARAM;
    const int n = (int)vtResult.size();
    if (n == 0) return SUCCESS;
    std::vector<float> poses((size_t)n * 13, 0.f);
    std::vector<int32_t> frame_of(n, 0), mesh_of;
    if (!MeshesOf(vtResult, mesh_of)) return (int)ERROR_INVALID_PARAM;         // a tag without a mesh
    for (int i = 0; i < n; ++i) memcpy(poses.data() + (size_t)13 * i, vtResult[i].tWorld2Cam, 12 * sizeof(float));
    const fl_intrinsics k = {PROC_IMG_WIDTH, TRACK_IMG_HEIGHT, K.dFx, K.dFy, K.dCx, K.dCy};
    const uint16_t *frame = tDepth.pData;
    std::vector<fl_track_result> res(n);
    int rc;
    if (m_verified_tracking) {
      std::vector<fl_verified_track_result> vres(n);
      rc = fl_track_batch_verified_meshes(m_tracker, 1, &frame, FL_MEM_HOST, n, frame_of.data(), mesh_of.data(), poses.data(), 0, nullptr, &k,
                                          nullptr, &m_tvparams, vres.data());
      for (int i = 0; i < n; ++i) res[i] = vres[i].track;
    } else {
      rc = fl_track_batch_meshes(m_tracker, 1, &frame, FL_MEM_HOST, n, frame_of.data(), mesh_of.data(), poses.data(), &k, nullptr, res.data());
    }
    if (rc != FL_OK) {
      fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
      return rc == FL_ERR_INVALID ? (int)ERROR_INVALID_PARAM : (int)ERROR_UNKNOW;
    }
    for (int i = 0; i < n; ++i) {
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
    if (!out || !m_ctx || !m_tracker || !check_image_u16(tDepth) || tDepth.nWidth != PROC_IMG_WIDTH || tDepth.nHeight != TRACK_IMG_HEIGHT ||
        (int)vtResult.size() > FEALESS_TRACK_MAX_OBJECTS || !(tau_mm >= 0.f && tau_mm < 65536.f))
      return (int)ERROR_INVALID_PARAM;
    const int n = (int)vtResult.size();
    if (n == 0) return SUCCESS;
    std::vector<float> poses((size_t)n * 13, 0.f);
    std::vector<int32_t> frame_of(n, 0), mesh_of;
    if (!MeshesOf(vtResult, mesh_of)) return (int)ERROR_INVALID_PARAM;         // a tag without a mesh
    for (int i = 0; i < n; ++i) memcpy(poses.data() + (size_t)13 * i, vtResult[i].tWorld2Cam, 12 * sizeof(float));
    const fl_intrinsics k = {PROC_IMG_WIDTH, TRACK_IMG_HEIGHT, K.dFx, K.dFy, K.dCx, K.dCy};
    const uint16_t *frame = tDepth.pData;
    const fl_verify_params prm = {(int32_t)tau_mm, 1, 0.f, 0.f};
    std::vector<fl_verify_result> res(n);
    const int rc = fl_verify_batch_meshes(m_tracker, 1, &frame, FL_MEM_HOST, n, frame_of.data(), mesh_of.data(), poses.data(), 0, nullptr, &k, &prm,
                                          res.data());
    if (rc != FL_OK) {
      fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
      return rc == FL_ERR_INVALID ? (int)ERROR_INVALID_PARAM : (int)ERROR_UNKNOW;
    }
    out->resize(n);
    for (int i = 0; i < n; ++i)
      (*out)[i] = CadRecoVerifyResult{res[i].accepted, res[i].n_model, res[i].n_missing, res[i].n_inlier, res[i].n_front, res[i].n_behind,
                                      res[i].inlier_ratio, res[i].behind_ratio};
    return SUCCESS;
  }

  // CadRecoArbitrate: one fl_verify_scene_batch over the entries, the frame one scene, each entry with the mesh of its strObjTag
  int Arbitrate(const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult, float tau_mm, float max_shared_ratio,
                vector<CadRecoSceneResult> *out)
  {
    if (out) out->clear();
    if (!out || !m_ctx || !m_tracker || !check_image_u16(tDepth) || tDepth.nWidth != PROC_IMG_WIDTH || tDepth.nHeight != TRACK_IMG_HEIGHT ||
        (int)vtResult.size() > FEALESS_TRACK_MAX_OBJECTS || !(tau_mm >= 0.f && tau_mm < 65536.f) ||
        !(std::isfinite(max_shared_ratio) && max_shared_ratio > 0.f && max_shared_ratio <= 1.f))
      return (int)ERROR_INVALID_PARAM;
    const int n = (int)vtResult.size();
    if (n == 0) return SUCCESS;
    std::vector<float> poses((size_t)n * 13, 0.f);
    std::vector<int32_t> frame_of(n, 0), mesh_of;
    if (!MeshesOf(vtResult, mesh_of)) return (int)ERROR_INVALID_PARAM;         // a tag without a mesh
    for (int i = 0; i < n; ++i) memcpy(poses.data() + (size_t)13 * i, vtResult[i].tWorld2Cam, 12 * sizeof(float));
    const fl_intrinsics k = {PROC_IMG_WIDTH, TRACK_IMG_HEIGHT, K.dFx, K.dFy, K.dCx, K.dCy};
    const uint16_t *frame = tDepth.pData;
    const fl_scene_params prm = {{(int32_t)tau_mm, 1, 0.f, 0.f}, max_shared_ratio, 1};
    const int32_t scene_first[2] = {0, n};
    std::vector<fl_scene_result> res(n);
    const int rc = fl_verify_scene_batch(m_tracker, 1, &frame, FL_MEM_HOST, n, frame_of.data(), mesh_of.data(), poses.data(), 1, scene_first, &k, &prm,
                                         res.data());
    if (rc != FL_OK) {
      fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(m_ctx));
      return rc == FL_ERR_INVALID ? (int)ERROR_INVALID_PARAM : (int)ERROR_UNKNOW;
    }
    out->resize(n);
    for (int i = 0; i < n; ++i) {
      const fl_verify_result &v = res[i].verify;
      (*out)[i] = CadRecoSceneResult{v.accepted, v.n_model, v.n_missing, v.n_inlier, v.n_front, v.n_behind, v.inlier_ratio, v.behind_ratio,
                                     res[i].kept, res[i].rival, res[i].n_shared};
    }
    return SUCCESS;
  }

  // CadRecoSetVerifiedPick: needs the multi-instance mode and a tracking mesh
  int SetVerifiedPick(int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio)
  {
    if (!on) { m_verified = false; return SUCCESS; }
    const bool multi_instance = m_instances.max_instances > 1 || m_instances.hyp_per_instance > 1;
    if (!m_ctx || !multi_instance || !m_tracker || !(tau_mm >= 0.f && tau_mm < 65536.f) || !std::isfinite(min_inlier_ratio) ||
        !std::isfinite(max_behind_ratio))
      return (int)ERROR_INVALID_PARAM;
    m_vparams = fl_verify_params{(int32_t)tau_mm, 1, min_inlier_ratio, max_behind_ratio};
    m_verified = true;
    return SUCCESS;
  }

  // CadRecoSetVerifiedTracking: needs a tracking mesh
  int SetVerifiedTracking(int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio, int keep_input)
  {
    if (!on) { m_verified_tracking = false; return SUCCESS; }
    if (!m_ctx || !m_tracker || !(tau_mm >= 0.f && tau_mm < 65536.f) || !std::isfinite(min_inlier_ratio) || !std::isfinite(max_behind_ratio) ||
        (keep_input != 0 && keep_input != 1))
      return (int)ERROR_INVALID_PARAM;
    m_tvparams = fl_track_verify_params{{(int32_t)tau_mm, 1, min_inlier_ratio, max_behind_ratio}, keep_input, 0};
    m_verified_tracking = true;
    return SUCCESS;
  }

  fl_recognition_params m_params;
  bool m_verified = false;   // CadRecoSetVerifiedPick; leaving the multi-instance mode clears it
  fl_verify_params m_vparams = {10, 1, 0.f, 0.f};
  bool m_verified_tracking = false;   // CadRecoSetVerifiedTracking
  fl_track_verify_params m_tvparams = {{10, 1, 0.f, 0.f}, 0, 0};
  int m_topk = 1;            // > 1: multi-hypothesis mode (CadRecoSetMultiHypothesis)
  float m_nms_dist = 20.0f;  // th_obj_dist of nonMaximumSuppression, mm
  fl_instance_params m_instances = {1, 48, 1};   // max_instances or hyp_per_instance > 1: multi-instance mode (CadRecoSetMultiInstance)

 private:
  fl_context *m_ctx = nullptr;
  fl_detector *m_det = nullptr;
  std::vector<std::string> m_class_ids;
  std::string m_path;
  int m_w = 0, m_h = 0, m_batch = 1;
  fl_tracker *m_tracker = nullptr;   // CadRecoSetTrackingMesh, CadRecoSetTrackingMeshes
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

int CadRecoRecognitionBatch(CObjRecoCAD *handle, int n_frames, const TImageU *rgb, const TImageU16 *depth,
                            const TCamIntrinsicParam &K, std::vector<std::vector<TObjRecoResult> > &out, std::vector<int> *frame_rc)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  return h->Batch(n_frames, rgb, depth, K, out, frame_rc);
}

int CadRecoSetMultiHypothesis(CObjRecoCAD *handle, int k, float nms_dist_mm)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h || k < 1 || k > 1024 || !(nms_dist_mm >= 0.f)) return (int)ERROR_INVALID_PARAM;
  h->m_topk = k;
  h->m_nms_dist = nms_dist_mm;
  h->m_instances.max_instances = h->m_instances.hyp_per_instance = 1;      // the two modes exclude each other
  h->m_verified = false;
  return 0;
}

int CadRecoSetMultiInstance(CObjRecoCAD *handle, int max_instances, int min_dist_px, int hyp_per_instance)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h || max_instances < 1 || max_instances > 64 || min_dist_px < 1 || min_dist_px > (1 << 30) || hyp_per_instance < 1 || hyp_per_instance > 64)
    return (int)ERROR_INVALID_PARAM;
  h->m_instances.max_instances = max_instances;
  h->m_instances.min_dist_px = min_dist_px;
  h->m_instances.hyp_per_instance = hyp_per_instance;
  h->m_topk = 1;                                                             // the two modes exclude each other
  if (max_instances == 1 && hyp_per_instance == 1) h->m_verified = false;
  return 0;
}

int CadRecoSetVerifiedPick(CObjRecoCAD *handle, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  return h->SetVerifiedPick(on, tau_mm, min_inlier_ratio, max_behind_ratio);
}

int CadRecoSetVerifiedTracking(CObjRecoCAD *handle, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio, int keep_input)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  return h->SetVerifiedTracking(on, tau_mm, min_inlier_ratio, max_behind_ratio, keep_input);
}

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
        pyr[k].width = t.width;
        pyr[k].height = t.height;
        pyr[k].offset_x = t.offset_x;
        pyr[k].offset_y = t.offset_y;
        pyr[k].pyramid_level = t.pyramid_level;
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
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h || n_views < 1 || !bgr || !depth_mm || !poses13 || !train_args_ok(dir, levels, T)) return (int)ERROR_INVALID_PARAM;
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
  if (!h->Context()) return (int)ERROR_UNKNOW;
  // Detector::addTemplate for every view (linemod_train.cpp:30-91), all of them in one batched call
  const int J = 2 * levels;
  std::vector<fl_template> tl((size_t)n_views * J);
  std::vector<fl_feature> fl((size_t)n_views * J * 63);
  std::vector<int32_t> bb((size_t)n_views * 4), st(n_views);
  const int rc = fl_extract_template_batch(h->Context(), n_views, bp.data(), dp.data(), any_mask ? mp.data() : nullptr, w, ht, levels,
                                           FL_MEM_HOST, tl.data(), fl.data(), bb.data(), st.data());
  if (rc == FL_ERR_INVALID) return (int)ERROR_INVALID_PARAM;
  if (rc != FL_OK) {
    fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(h->Context()));
    return (int)ERROR_UNKNOW;
  }
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
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h || !train_args_ok(dir, levels, T) || views.distances_mm.empty()) return (int)ERROR_INVALID_PARAM;
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
  fl_context *ctx = h->Context();
  if (!ctx) return (int)ERROR_UNKNOW;
  // initInternalMat (ICP/common.cpp:358): the K detection() back-projects the template depth with (ICP/detection.cpp:35-36)
  const int w = 640, ht = 480;
  const fl_intrinsics K = {w, ht, 608.0, 608.0, 320.0, 240.0};
  const float *nrm = mesh.normals.empty() ? nullptr : mesh.normals.data();
  const int slab = FL_EXTRACT_CHUNK_VIEWS, J = 2 * levels;
  const size_t px = (size_t)w * ht;
  auto render = [&](int n, const float *p13, uint8_t *bgr, uint16_t *depth, uint8_t *mask) {
    if (fl_render_views(ctx, mesh.vertices.data(), nrm, nullptr, n_v, mesh.triangles.data(), n_t, n, p13, &K, nullptr, FL_MEM_HOST, bgr, depth,
                        mask, nullptr) != FL_OK) {
      fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(ctx));
      return (int)ERROR_UNKNOW;
    }
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
                                    st.data()) != FL_OK) {
        fprintf(stderr, "[fealess_hip] %s\n", fl_last_error(ctx));
        return (int)ERROR_UNKNOW;
      }
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

int CadRecoSetTrackingMesh(CObjRecoCAD *handle, const string &obj_path, float scale)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  fealess::Mesh mesh;
  std::string err;
  const int rc = fealess::ReadObj(obj_path, scale, mesh, &err);
  if (rc != SUCCESS) {
    fprintf(stderr, "[cadreco] %s\n", err.c_str());
    return rc;
  }
  return h->SetTrackingMesh(mesh);
}

int CadRecoSetTrackingMeshes(CObjRecoCAD *handle, const vector<std::pair<string, string>> &class_id_and_obj_path, float scale)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  std::vector<std::string> ids;
  std::vector<fealess::Mesh> meshes(class_id_and_obj_path.size());
  for (size_t i = 0; i < class_id_and_obj_path.size(); ++i) {
    std::string err;
    const int rc = fealess::ReadObj(class_id_and_obj_path[i].second, scale, meshes[i], &err);
    if (rc != SUCCESS) {
      fprintf(stderr, "[cadreco] %s\n", err.c_str());
      return rc;
    }
    ids.push_back(class_id_and_obj_path[i].first);
  }
  return h->SetTrackingMeshes(ids, meshes);
}

int CadRecoTrack(CObjRecoCAD *handle, const TImageU16 &tDepth, const TCamIntrinsicParam &K, vector<TObjRecoResult> &vtResult,
                 vector<int> *tracked)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  return h->Track(tDepth, K, vtResult, tracked);
}

int CadRecoVerify(CObjRecoCAD *handle, const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult,
                  float tau_mm, vector<CadRecoVerifyResult> *out)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  return h->Verify(tDepth, K, vtResult, tau_mm, out);
}

int CadRecoArbitrate(CObjRecoCAD *handle, const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult,
                     float tau_mm, float max_shared_ratio, vector<CadRecoSceneResult> *out)
{
  CObjRecoLmICPHip *h = dynamic_cast<CObjRecoLmICPHip *>(handle);
  if (!h) return (int)ERROR_INVALID_PARAM;
  return h->Arbitrate(tDepth, K, vtResult, tau_mm, max_shared_ratio, out);
}

// ---- flat C shim so that the pytest harness (ctypes) can drive the C++ facade -------------------
extern "C" {
// CadRecoVerify on n poses (n 4x4 matrices); out: n CadRecoVerifyResult records (8 x 4 bytes each)
int cadreco_verify(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                   const float *poses16, float tau_mm, void *out)
{
  if (n < 0 || (n > 0 && (!poses16 || !out))) return (int)ERROR_INVALID_PARAM;
  TImageU16 d = {ts, (unsigned short *)depth, w, h_};
  TCamIntrinsicParam K;
  K.nWidth = w; K.nHeight = h_; K.dFx = fx; K.dFy = fy; K.dCx = cx; K.dCy = cy;
  std::vector<TObjRecoResult> res(n);
  for (int i = 0; i < n; ++i) memcpy(res[i].tWorld2Cam, poses16 + 16 * i, 16 * sizeof(float));
  std::vector<CadRecoVerifyResult> v;
  const int rc = CadRecoVerify((CObjRecoCAD *)h, d, K, res, tau_mm, &v);
  if (rc == SUCCESS && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(CadRecoVerifyResult));
  return rc;
}
// CadRecoArbitrate on n poses (n 4x4 matrices; tags: n class ids, or NULL for none); out: n CadRecoSceneResult records (11 x 4
// bytes each)
int cadreco_arbitrate(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                      const float *poses16, const char *const *tags, float tau_mm, float max_shared_ratio, void *out)
{
  if (n < 0 || (n > 0 && (!poses16 || !out))) return (int)ERROR_INVALID_PARAM;
  TImageU16 d = {ts, (unsigned short *)depth, w, h_};
  TCamIntrinsicParam K;
  K.nWidth = w; K.nHeight = h_; K.dFx = fx; K.dFy = fy; K.dCx = cx; K.dCy = cy;
  std::vector<TObjRecoResult> res(n);
  for (int i = 0; i < n; ++i) {
    if (tags && !tags[i]) return (int)ERROR_INVALID_PARAM;
    if (tags) res[i].strObjTag = tags[i];
    memcpy(res[i].tWorld2Cam, poses16 + 16 * i, 16 * sizeof(float));
  }
  std::vector<CadRecoSceneResult> v;
  const int rc = CadRecoArbitrate((CObjRecoCAD *)h, d, K, res, tau_mm, max_shared_ratio, &v);
  if (rc == SUCCESS && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(CadRecoSceneResult));
  return rc;
}
// cadreco_verify with a class id per pose (tags: n strings): what picks each pose's mesh after cadreco_set_tracking_meshes
int cadreco_verify_tagged(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                          const float *poses16, const char *const *tags, float tau_mm, void *out)
{
  if (n < 0 || (n > 0 && (!poses16 || !tags || !out))) return (int)ERROR_INVALID_PARAM;
  TImageU16 d = {ts, (unsigned short *)depth, w, h_};
  TCamIntrinsicParam K;
  K.nWidth = w; K.nHeight = h_; K.dFx = fx; K.dFy = fy; K.dCx = cx; K.dCy = cy;
  std::vector<TObjRecoResult> res(n);
  for (int i = 0; i < n; ++i) {
    if (!tags[i]) return (int)ERROR_INVALID_PARAM;
    res[i].strObjTag = tags[i];
    memcpy(res[i].tWorld2Cam, poses16 + 16 * i, 16 * sizeof(float));
  }
  std::vector<CadRecoVerifyResult> v;
  const int rc = CadRecoVerify((CObjRecoCAD *)h, d, K, res, tau_mm, &v);
  if (rc == SUCCESS && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(CadRecoVerifyResult));
  return rc;
}
// CadRecoSetTrackingMeshes on n (class id, OBJ path) pairs
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
int cadreco_set_verified_pick(void *h, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio)
{
  return CadRecoSetVerifiedPick((CObjRecoCAD *)h, on, tau_mm, min_inlier_ratio, max_behind_ratio);
}
int cadreco_set_verified_tracking(void *h, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio, int keep_input)
{
  return CadRecoSetVerifiedTracking((CObjRecoCAD *)h, on, tau_mm, min_inlier_ratio, max_behind_ratio, keep_input);
}
int cadreco_set_tracking_mesh(void *h, const char *obj_path, float scale)
{
  if (!obj_path) return (int)ERROR_INVALID_PARAM;
  return CadRecoSetTrackingMesh((CObjRecoCAD *)h, obj_path, scale);
}
// CadRecoTrack on n results: poses16 (n 4x4 matrices) goes in as the previous poses and comes out updated; tracked: n ints
int cadreco_track(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                  float *poses16, int *tracked)
{
  if (n < 0 || (n > 0 && (!poses16 || !tracked))) return (int)ERROR_INVALID_PARAM;
  TImageU16 d = {ts, (unsigned short *)depth, w, h_};
  TCamIntrinsicParam K;
  K.nWidth = w; K.nHeight = h_; K.dFx = fx; K.dFy = fy; K.dCx = cx; K.dCy = cy;
  std::vector<TObjRecoResult> res(n);
  for (int i = 0; i < n; ++i) memcpy(res[i].tWorld2Cam, poses16 + 16 * i, 16 * sizeof(float));
  std::vector<int> trk;
  const int rc = CadRecoTrack((CObjRecoCAD *)h, d, K, res, &trk);
  for (int i = 0; i < n; ++i) {
    memcpy(poses16 + 16 * i, res[i].tWorld2Cam, 16 * sizeof(float));
    tracked[i] = i < (int)trk.size() ? trk[i] : 0;
  }
  return rc;
}
int cadreco_write_png16(const char *path, const unsigned short *px, int w, int h)
{
  std::string err;
  return fealess::WritePng16(path, px, w, h, &err) ? 0 : -1;
}
// CadRecoTrainViews on host views of one size w x h_; mask: NULL or n pointers (each may be NULL); template_of_view: n ints
// (may be NULL), written on success
int cadreco_train_views(void *h, const char *dir, const char *class_id, int n, const unsigned char *const *bgr,
                        const unsigned short *const *depth, const unsigned char *const *mask, int w, int h_, const float *poses13,
                        int levels, const int *T, int *template_of_view)
{
  if (!dir || !class_id || n < 1 || !bgr || !depth) return (int)ERROR_INVALID_PARAM;
  std::vector<TImageU> b(n), m(mask ? n : 0);
  std::vector<TImageU16> d(n);
  for (int i = 0; i < n; ++i) {
    b[i] = TImageU{0.0, (unsigned char *)bgr[i], w, h_};
    d[i] = TImageU16{0.0, (unsigned short *)depth[i], w, h_};
    if (mask) m[i] = TImageU{0.0, (unsigned char *)mask[i], w, h_};
  }
  std::vector<int> tov;
  const int rc = CadRecoTrainViews((CObjRecoCAD *)h, dir, class_id, n, b.data(), d.data(), mask ? m.data() : nullptr, poses13, levels, T, &tov);
  if (rc == SUCCESS && template_of_view) std::copy(tov.begin(), tov.end(), template_of_view);
  return rc;
}
// fealess::ReadObj: counts always (on success); the arrays when non-NULL and their caps hold them
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
// CadRecoTrainMesh; template_of_view: cap ints (may be NULL), written on success when they hold every view
int cadreco_train_mesh(void *h, const char *dir, const char *class_id, const char *obj_path, float scale, int subdivisions, int upper_hemisphere,
                       const float *distances_mm, int n_distances, int n_inplane, float inplane_deg, int levels, const int *T,
                       int *template_of_view, int cap)
{
  if (!dir || !class_id || !obj_path || !distances_mm || n_distances < 1) return (int)ERROR_INVALID_PARAM;
  CadRecoViewSphere vs;
  vs.subdivisions = subdivisions;
  vs.upper_hemisphere = upper_hemisphere;
  vs.distances_mm.assign(distances_mm, distances_mm + n_distances);
  vs.n_inplane = n_inplane;
  vs.inplane_deg = inplane_deg;
  std::vector<int> tov;
  const int rc = CadRecoTrainMesh((CObjRecoCAD *)h, dir, class_id, obj_path, scale, vs, levels, T, &tov);
  if (rc == SUCCESS && template_of_view && (int)tov.size() <= cap) std::copy(tov.begin(), tov.end(), template_of_view);
  return rc;
}
int cadreco_set_multi_hypothesis(void *h, int k, float nms_dist_mm) { return CadRecoSetMultiHypothesis((CObjRecoCAD *)h, k, nms_dist_mm); }
int cadreco_set_multi_instance(void *h, int max_instances, int min_dist_px, int hyp_per_instance)
{
  return CadRecoSetMultiInstance((CObjRecoCAD *)h, max_instances, min_dist_px, hyp_per_instance);
}
// Recognition() returning every result: poses16 receives min(*n_results, cap) 4x4 matrices
int cadreco_recognition_all(void *h, const unsigned char *bgr, const unsigned short *depth, int w, int h_, double ts, int kw, int kh,
                            double fx, double fy, double cx, double cy, int *n_results, float *poses16, int cap)
{
  TImageU rgb = {ts, (unsigned char *)bgr, w, h_};
  TImageU16 dep = {ts, (unsigned short *)depth, w, h_};
  TCamIntrinsicParam K;
  K.nWidth = kw; K.nHeight = kh; K.dFx = fx; K.dFy = fy; K.dCx = cx; K.dCy = cy;
  vector<TObjRecoResult> out;
  const int rc = ((CObjRecoCAD *)h)->Recognition(rgb, dep, K, out);
  *n_results = (int)out.size();
  for (int i = 0; i < (int)out.size() && i < cap; ++i) memcpy(poses16 + 16 * i, out[i].tWorld2Cam, 16 * sizeof(float));
  return rc;
}
void *cadreco_create(int type) { return CObjRecoCAD::Create((CObjRecoCAD::EObjRecoType)type); }
void cadreco_destroy(void *h) { CObjRecoCAD::Destroy((CObjRecoCAD *)h); }
int cadreco_add_obj(void *h, const char *dir) { return ((CObjRecoCAD *)h)->AddObj(dir); }
int cadreco_set_params(void *h, float thr, int it, float dmean, float ddiff, int mode)
{
  CObjRecoLmICPHip *p = dynamic_cast<CObjRecoLmICPHip *>((CObjRecoCAD *)h);
  if (!p) return -1;
  p->m_params.matching_threshold = thr;
  p->m_params.icp_it_thr = it;
  p->m_params.dist_mean_thr = dmean;
  p->m_params.dist_diff_thr = ddiff;
  p->m_params.icp_mode = mode;
  return 0;
}
// returns Recognition()'s code; *n_results = vtResult.size(); pose16 / tag filled for result 0
int cadreco_recognition(void *h, const unsigned char *bgr, const unsigned short *depth, int w, int h_, double ts, int kw, int kh,
                        double fx, double fy, double cx, double cy, int *n_results, float *pose16, char *tag, int tag_cap)
{
  TImageU rgb = {ts, (unsigned char *)bgr, w, h_};
  TImageU16 d = {ts, (unsigned short *)depth, w, h_};
  TCamIntrinsicParam K;
  K.nWidth = kw; K.nHeight = kh; K.dFx = fx; K.dFy = fy; K.dCx = cx; K.dCy = cy;
  std::vector<TObjRecoResult> out;
  int rc = ((CObjRecoCAD *)h)->Recognition(rgb, d, K, out);
  *n_results = (int)out.size();
  if (!out.empty()) {
    memcpy(pose16, out[0].tWorld2Cam, 16 * sizeof(float));
    snprintf(tag, tag_cap, "%s", out[0].strObjTag.c_str());
  }
  return rc;
}
int cadreco_read_linemod_cached(const char *path, int *from_cache, int *n_templates, int *n_features)
{
  fealess::DetectorFile df;
  std::string err;
  bool fc = false;
  if (!fealess::ReadLinemodCached(path, df, &err, &fc)) return -1;
  *from_cache = fc ? 1 : 0;
  *n_templates = 0;
  *n_features = 0;
  for (auto &c : df.classes)
    for (auto &p : c.template_pyramids) {
      ++*n_templates;
      for (auto &t : p) *n_features += (int)t.features.size();
    }
  return 0;
}
int cadreco_read_linemod(const char *path, int *levels, int *n_classes, int *n_templates, int *n_features)
{
  fealess::DetectorFile df;
  std::string err;
  if (!fealess::ReadLinemod(path, df, &err)) return -1;
  *levels = df.pyramid_levels;
  *n_classes = (int)df.classes.size();
  int nt = 0, nf = 0;
  for (auto &c : df.classes)
    for (auto &p : c.template_pyramids) { ++nt; for (auto &t : p) nf += (int)t.features.size(); }
  *n_templates = nt;
  *n_features = nf;
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
const char *cadreco_version() { static std::string v = CObjRecoCAD::GetVersion(); return v.c_str(); }
}
