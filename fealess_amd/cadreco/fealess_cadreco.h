// fealess_cadreco.h -- C++ host surface of the MI355X implementation: the CadReco facade
// (reference: CadReco/obj_reco_temp.h:6-30, CadReco/lotus_common.h, CadReco/obj_reco_lmicp.h) and
// the OpenCV-free parts of linemod/linemod_if.h, re-declared without any OpenCV type so that a
// CadReco caller links against libcadreco_hip.so instead of the reference's static libraries.
//
// Types keep the reference's names, member order and meaning, so they are layout-compatible
// with code compiled against the reference's own lotus_common.h / obj_reco_temp.h (that code may
// keep including its own headers).
#ifndef FEALESS_CADRECO_H
#define FEALESS_CADRECO_H

#include <string>
#include <utility>
#include <vector>

#ifndef __COMMON_H__            // the reference's lotus_common.h guard: do not redefine its types
#define SUCCESS 0
#define ERROR_INVALID_PARAM    0x80000001
#define ERROR_OPEN_FILE_FAILED 0x80000002
#define ERROR_VERSION_MISMATCH 0x80000003
#define ERROR_NEW_FAILED       0x80000004
#define ERROR_UNKNOW           0x80000005

using std::string;
using std::vector;

template <typename T>
struct TImage {                 // borrowed pixel buffer; BGR8 interleaved for the colour frame
  double dTimestamp;            // ms; negative = invalid
  T *pData;
  int nWidth;
  int nHeight;
};
typedef TImage<unsigned char> TImageU;
typedef TImage<unsigned short int> TImageU16;
typedef TImage<float> TImageF;

struct TCamIntrinsicParam {     // pinhole K = [fx 0 cx; 0 fy cy; 0 0 1]
  int nWidth;
  int nHeight;
  double dFx;
  double dFy;
  double dCx;
  double dCy;
  vector<double> vdDistCoeff;
};

typedef float Mat4x4F[16];

struct TScanFrame {
  TImageU tGrayImg;
  TImageU tMask;
  Mat4x4F tWorld2Cam;
  TImageF tDepthImg;
};

struct TScanPackage {
  string strObjTag;
  Mat4x4F tGLPrjMatrix;
  vector<float> bounding_box;
  vector<TScanFrame> vtScanFrame;
};

struct TObjRecoResult {
  string strObjTag;             // class_id of the best match
  Mat4x4F tWorld2Cam;           // row-major 4x4, last row 0 0 0 1
};

struct AdvancedParam {
  bool bEnablePoseBinFrameMatching;
  bool bEnablePreprocessing;
};

struct TTrainParam {
  int nType;
  int nMethod;
  bool bPreprocessing;
  float img_physical_width;
};
#endif  // __COMMON_H__

#ifndef __OBJ_RECO_TEMP__       // the reference's obj_reco_temp.h guard
class CObjRecoCAD {
 public:
  enum EObjRecoType { EObjReco_FEATURE, EObjReco_LmICP, EObjReco_BB8, EObjReco_PoseNet };
  virtual ~CObjRecoCAD() {}
  static string GetVersion();
  static CObjRecoCAD *Create(EObjRecoType eType = EObjReco_LmICP);   // nullptr for unsupported types
  static void Destroy(CObjRecoCAD *pHandle);
  virtual int Train(const string &strDataBase, const TScanPackage &tScanPackage, const TTrainParam &tObjTrainParam) = 0;
  virtual int AddObj(const string pObjModel) = 0;
  virtual int ClearObj() = 0;
  virtual int SetROI(const TImageU &tROI) = 0;
  virtual int Recognition(const TImageU &tRGB, const TImageU16 &tDepth, const TCamIntrinsicParam &tCamIntrinsic,
                          vector<TObjRecoResult> &vtResult) = 0;
  virtual int SetAdvancedParam(const AdvancedParam &advancedParam) = 0;
  virtual int GetAdvancedParam(const string &strKey, void *pvValue) = 0;
};
#endif

// ---- template bank files (linemod/linemod_if.h readLinemod / writeLinemod, without cv::Ptr) ----
namespace fealess {

struct Feature { int x, y, label; };
struct Template {
  int width, height, offset_x, offset_y, pyramid_level;
  std::vector<Feature> features;
};
struct ObjectClass {
  std::string class_id;
  std::vector<std::vector<Template> > template_pyramids;   // [template_id][l*M + m]
  std::vector<std::vector<float> > poses;                   // [template_id][13]
};
struct DetectorFile {            // what linemod_templates.yml holds (linemod.cpp:1681-1794)
  int pyramid_levels = 0;
  std::vector<int> T;
  std::vector<std::string> modalities;                       // "ColorGradient", "DepthNormal"
  std::vector<ObjectClass> classes;
};

// readLinemod (linemod_if.cpp:36-47): OpenCV FileStorage YAML 1.0 subset; false + err on failure
bool ReadLinemod(const std::string &filename, DetectorFile &out, std::string *err);
// writeLinemod (linemod_if.cpp:49-63)
bool WriteLinemod(const DetectorFile &det, const std::string &filename);
// packed binary cache of the same content (<yml>.flbank, keyed by the YAML's size and mtime); ReadLinemodCached =
// readLinemod that uses / refreshes it
bool WriteBankCache(const DetectorFile &det, const std::string &filename, unsigned long long yml_size, long long yml_mtime);
bool ReadBankCache(const std::string &filename, DetectorFile &out, unsigned long long yml_size, long long yml_mtime);
bool ReadLinemodCached(const std::string &filename, DetectorFile &out, std::string *err, bool *from_cache);
// imread(path, -1) for the 16-bit single-channel depth PNGs (obj_reco_lmicp.cpp:157)
bool ReadPng16(const std::string &filename, std::vector<unsigned short> &pixels, int &w, int &h, std::string *err);
// its mirror: 16-bit greyscale, non-interlaced, zlib (what imwrite gives a CV_16U image); false + err on failure
bool WritePng16(const std::string &filename, const unsigned short *pixels, int w, int h, std::string *err);

// Wavefront OBJ (not in the reference, whose CModelMesh::Load(file, model_scale) goes through a mesh library,
// test/model_mesh.cpp): v (extra components ignored), vn, and f in the forms i, i/j, i//k, i/j/k with 1-based or negative
// (relative) indices; polygons are fan-triangulated; every other record is ignored.  Coordinates are multiplied by
// `scale`.  Normals are kept only when every face corner has one: then each distinct (position, normal) pair becomes one
// vertex, in order of first use; otherwise `normals` is empty and the positions keep their order.
struct Mesh {
  std::vector<float> vertices, normals;   // 3 floats per vertex (normals: empty, or one per vertex)
  std::vector<int> triangles;             // 3 vertex indices per triangle, 0-based
};
// SUCCESS; ERROR_OPEN_FILE_FAILED (unreadable); ERROR_INVALID_PARAM (index 0 or out of range, a non-numeric token, a
// face of fewer than three corners, no face, a scale that is not finite and > 0)
int ReadObj(const std::string &path, float scale, Mesh &out, std::string *err);

}  // namespace fealess

// Extensions of the MI355X build (not in the reference): batch entry point on the same object.
class CObjRecoLmICPHip;
// out[i] = what Recognition() puts into vtResult for frame i; frame_rc (optional) = what it would return for frame i.
// Returns the first non-zero frame code: a frame that fails does not take the others' results with it.
int CadRecoRecognitionBatch(CObjRecoCAD *handle, int n_frames, const TImageU *rgb, const TImageU16 *depth,
                            const TCamIntrinsicParam &K, std::vector<std::vector<TObjRecoResult> > &out,
                            std::vector<int> *frame_rc = nullptr);

// Opt-in, not in the reference (its Recognition() only ever looks at matches[0]): refine the first k matches of every
// frame and return the nonMaximumSuppression (ICP/NMS.cpp:6-40, th_obj_dist = nms_dist_mm) winners, best first, in
// vtResult.  k = 1 restores the reference behaviour.
int CadRecoSetMultiHypothesis(CObjRecoCAD *handle, int k, float nms_dist_mm);

// Opt-in, not in the reference: every instance in the frame.  The match list is grouped in image space on the device
// (box centres closer than min_dist_px to a group's first match, same class; at most max_instances groups, 1..64), the
// first hyp_per_instance (1..64) members of each group are refined in one ICP launch, and nonMaximumSuppression's rule
// (ICP/NMS.cpp:6-40) picks one of them per group (fl_recognize_batch_instances, include/fealess_hip.h).  Recognition() and
// CadRecoRecognitionBatch then return one TObjRecoResult per instance, in group order (the group of matches[0] first).
// max_instances = 1 with hyp_per_instance = 1 restores the reference behaviour.  This mode and CadRecoSetMultiHypothesis
// exclude each other: setting one clears the other.
int CadRecoSetMultiInstance(CObjRecoCAD *handle, int max_instances, int min_dist_px, int hyp_per_instance);

// Not in the reference, where Train() is a stub and a data directory comes from the test/linemod_train.cpp demo
// (OpenCV, Detector::addTemplate per frame, writeLinemod): train one class on the handle's GPU, batched, and write the
// directory AddObj() reads.  Views: bgr[v] (BGR8), depth_mm[v] (mm), all of one size; mask: NULL, or per view an
// object mask whose pData may be NULL (no mask).  poses13: 13 floats per view; levels, T[levels]: the pyramid.
// Writes <dir>/depth/<template_id>.png (the view's depth x 10 in 0.1 mm, saturating: Recognition's convertTo(CV_16U,
// 0.1) gives back the view's millimetres) and then <dir>/linemod_templates.yml (ColorGradient + DepthNormal).
// Template ids count the views that produced a template; template_of_view (optional) gets that id or -1 per view.
// linemod_train names the PNGs by frame number while Recognition reads them by template id, so its directories are
// only right when no view fails; here the PNGs follow the template ids.
// Returns SUCCESS; ERROR_INVALID_PARAM (views of different sizes, a bad pointer or argument, no view yields a
// template: nothing written); ERROR_OPEN_FILE_FAILED (a file cannot be written: what the call created is removed again);
// ERROR_UNKNOW (no GPU, HIP error).
int CadRecoTrainViews(CObjRecoCAD *handle, const string &dir, const string &class_id, int n_views, const TImageU *bgr,
                      const TImageU16 *depth_mm, const TImageU *mask, const float *poses13, int levels, const int *T,
                      std::vector<int> *template_of_view);

// The view sphere of fl_view_sphere (include/fealess_hip.h): icosphere points (subdivisions 0..6, optionally z >= 0 only)
// x distances_mm x n_inplane angles over [-inplane_deg, +inplane_deg], every camera looking at the object origin.
struct CadRecoViewSphere {
  int subdivisions = 2;
  int upper_hemisphere = 1;
  std::vector<float> distances_mm;
  int n_inplane = 1;
  float inplane_deg = 0.f;
};
// Not in the reference (its CObjRecoCAD::Train(..., TScanPackage, ...) is a stub and linemod_train reads views another
// tool rendered): train one class from a CAD mesh on the handle's GPU.  Reads the OBJ (fealess::ReadObj, `scale` as
// CModelMesh::Load's model_scale), renders every view of the sphere with fl_render_views at 640x480 and
// K = 608 / 608 / 320 / 240 -- initInternalMat (ICP/common.cpp:358), the K detection() back-projects a template's depth
// with (ICP/detection.cpp:35-36): any other K would give Recognition's ICP a wrongly scaled model cloud -- and writes the
// directory CadRecoTrainViews writes (the render's mask is the view's object mask; template_pose = the view-sphere pose;
// depth/<template_id>.png = the render x 10, saturating; linemod_templates.yml last).  Views go through in slabs of 64,
// so host memory stays bounded.  template_of_view (optional): per view of the sphere, its template id or -1.
// Returns SUCCESS; ERROR_OPEN_FILE_FAILED (unreadable OBJ, or a file cannot be written); ERROR_INVALID_PARAM (malformed
// OBJ, bad arguments, no view yields a template); ERROR_UNKNOW (no GPU, HIP error).  On every error nothing is left
// behind: an error once writing has begun (a file that cannot be written, a HIP error while the depths are rendered again)
// removes the files and directories the call created (depth PNGs it replaced in an existing directory stay replaced).
// The host path: views are rendered to host memory and extracted from there (the facade holds no device memory); the
// Python route Context.render_views(mem=FL_MEM_DEVICE) -> extract_template_batch keeps them in HBM.
int CadRecoTrainMesh(CObjRecoCAD *handle, const string &dir, const string &class_id, const string &obj_path, float scale,
                     const CadRecoViewSphere &views, int levels, const int *T, std::vector<int> *template_of_view);

// ---- tracking between recognitions (not in the reference, which links a KCF box tracker it never calls:
// test/linemod_acq.cpp:108-150) -------------------------------------------------------------------------------------------
// Recognition() costs a front-end, a scan of the whole bank and a 20-iteration ICP per frame.  Between recognitions an object
// can be FOLLOWED instead: render the CAD mesh at the previous frame's pose, crop both depth images around the render and
// run detection() from that pose (fl_track_batch, include/fealess_hip.h: point-to-plane ICP, one pass, the library's defaults).
// CadRecoSetTrackingMesh reads the OBJ (fealess::ReadObj -- the file and scale CadRecoTrainMesh trained from) and uploads it;
// a second call replaces the mesh.  SUCCESS; ReadObj's codes; ERROR_INVALID_PARAM (mesh limits); ERROR_UNKNOW (no GPU, HIP).
// CadRecoTrack: vtResult comes in as the previous frame's results (from Recognition or from CadRecoTrack) and goes out
// updated; (*tracked)[i] (optional) = 1 where entry i was followed, 0 where it was lost -- out of view, too few points, a crop
// of more than FEALESS_TRACK_MAX_CROP_PX pixels -- and then the entry keeps its pose: call Recognition again.  The depth frame
// must be 640 x 480 (the image of the model camera 608 / 608 / 320 / 240 that detection() assumes for the render); K is the
// frame's camera.  ERROR_INVALID_PARAM: no mesh set, another frame size, an invalid image, more than
// FEALESS_TRACK_MAX_OBJECTS entries.  An empty vtResult is SUCCESS.
// CadRecoSetTrackingMeshes: several object types on one table.  One (class id, OBJ path) pair per type, every OBJ read with
// fealess::ReadObj at `scale`; ONE tracker holds all the meshes (fl_tracker_create_meshes: they share its frame slot, render
// images and ICP workspaces), and it replaces the tracker of an earlier call of either kind.  CadRecoTrack and CadRecoVerify
// then take each entry's mesh from its strObjTag -- an entry whose tag has no mesh: ERROR_INVALID_PARAM, nothing tracked -- and
// CadRecoSetVerifiedPick verifies the groups of every class whose id has a mesh against that mesh; groups of the other classes
// are returned as the multi-instance mode returns them.  CadRecoSetTrackingMesh keeps its meaning: one mesh, used for every
// tag.  ERROR_INVALID_PARAM also for an empty list, an id given twice, or meshes beyond the library's limits.
#define FEALESS_TRACK_MAX_OBJECTS 16
#define FEALESS_TRACK_MAX_CROP_PX (320 * 240)
int CadRecoSetTrackingMesh(CObjRecoCAD *handle, const string &obj_path, float scale);
int CadRecoSetTrackingMeshes(CObjRecoCAD *handle, const vector<std::pair<string, string>> &class_id_and_obj_path, float scale);
int CadRecoTrack(CObjRecoCAD *handle, const TImageU16 &tDepth, const TCamIntrinsicParam &K, vector<TObjRecoResult> &vtResult,
                 vector<int> *tracked);

// ---- verification: is an object where its result says it is? ---------------------------------------------------------------
// CadRecoVerify renders the mesh of CadRecoSetTrackingMesh at every entry's tWorld2Cam with the frame's camera K and lays the
// render over the depth frame (fl_verify_batch, include/fealess_hip.h, which states the per-pixel rule).  Per entry: the
// rendered pixels (n_model), how many of them the frame supports within tau_mm (n_inlier), has no depth for (n_missing), shows
// something nearer at -- an occluder, which is allowed -- (n_front), or sees THROUGH the object at, which is impossible
// (n_behind), and the two ratios n_inlier / n_model and n_behind / n_model.  accepted = 1 when anything was rendered (the
// library's default gates); callers put their own thresholds on the ratios.  vtResult is not changed; *out gets one record per
// entry.  The same limits and error codes as CadRecoTrack; tau_mm outside 0..65535 (as an integer): ERROR_INVALID_PARAM.
struct CadRecoVerifyResult {
  int accepted;
  int n_model, n_missing, n_inlier, n_front, n_behind;
  float inlier_ratio, behind_ratio;
};
int CadRecoVerify(CObjRecoCAD *handle, const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult,
                  float tau_mm, vector<CadRecoVerifyResult> *out);

// ---- arbitration: which of the results explain the same surface? ---------------------------------------------------------------
// Two classes that fire on one physical object (a bracket whose mesh is part of a housing) both verify well.  CadRecoArbitrate
// verifies every entry as CadRecoVerify does, each with the mesh of its strObjTag, and then treats the frame as ONE scene of
// fl_verify_scene_batch (include/fealess_hip.h, which states the rule): the accepted entries in the order of their n_inlier, an
// entry suppressed (kept = 0) when an entry kept before it shares at least max_shared_ratio of the frame pixels that support
// it.  rival = the index in vtResult of the entry that suppressed it -- for a kept entry, of the kept entry it shares most
// with -- or -1; n_shared = the pixels the two share.  Recognise verified (CadRecoSetVerifiedPick), then arbitrate, then keep
// the entries with kept = 1.  vtResult is not changed.  The same limits and error codes as CadRecoVerify; max_shared_ratio not
// finite or outside (0, 1]: ERROR_INVALID_PARAM.
struct CadRecoSceneResult {
  int accepted;
  int n_model, n_missing, n_inlier, n_front, n_behind;
  float inlier_ratio, behind_ratio;
  int kept, rival, n_shared;
};
int CadRecoArbitrate(CObjRecoCAD *handle, const TImageU16 &tDepth, const TCamIntrinsicParam &K, const vector<TObjRecoResult> &vtResult,
                     float tau_mm, float max_shared_ratio, vector<CadRecoSceneResult> *out);

// Opt-in: the verification decides what the multi-instance mode returns (fl_recognize_batch_instances_verified,
// include/fealess_hip.h).  Every refined member of every group is verified against the mesh of CadRecoSetTrackingMesh behind the
// frame's one ICP launch, with tau_mm and the two gates (<= 0: no test) as CadRecoVerify and fl_verify_params state them; a
// group's member is picked by the verification, and Recognition() / CadRecoRecognitionBatch return only the instances whose
// picked member was accepted, in group order.  Needs CadRecoSetMultiInstance (more than {1, ., 1}) and CadRecoSetTrackingMesh
// first, and frames that are 640 x 480 after the zoom: ERROR_INVALID_PARAM otherwise, as for tau_mm outside 0..65535 or a
// threshold that is not finite.  on = 0 switches it off, and Recognition() is again what the multi-instance mode returns;
// leaving the multi-instance mode switches it off too.
int CadRecoSetVerifiedPick(CObjRecoCAD *handle, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio);

// Opt-in: the verification decides what CadRecoTrack reports (fl_track_batch_verified, include/fealess_hip.h).  After the ICP the
// pose every followed entry came out with is verified against the depth frame on the device, with tau_mm and the two gates
// (<= 0: no test) as CadRecoVerify and fl_verify_params state them; (*tracked)[i] = 1 only where a pose was accepted, and an
// entry whose pose was not keeps the pose it came in with, like any lost entry.  keep_input = 1: the pose an entry came in with
// is verified too and kept (tracked = 1) where it verifies strictly better than the ICP's -- an object that stands still then
// does not jitter.  Needs CadRecoSetTrackingMesh first: ERROR_INVALID_PARAM otherwise, as for tau_mm outside 0..65535, a
// threshold that is not finite or keep_input outside {0, 1}.  on = 0 switches it off, and CadRecoTrack is again fl_track_batch.
int CadRecoSetVerifiedTracking(CObjRecoCAD *handle, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio, int keep_input);

// ---- a depth camera of its own (the reference's callers run rs2::align(RS2_STREAM_COLOR) on every frameset before
// Recognition: test/linemod_recon.cpp:38-51, test/linemod_acq.cpp:24-42) ----------------------------------------------------------
// Every entry point above takes a depth image that is pixel-aligned with the colour image and expressed in tCamIntrinsic.  No
// sensor delivers that.  With on = 1 the handle takes the depth image as the depth sensor delivers it: tDepth must then have
// K_depth's size instead of tCamIntrinsic's, and is registered to tCamIntrinsic on the GPU (fl_register_depth_batch,
// include/fealess_hip.h, which states the rule; host memory in and out) before anything else happens -- in Recognition,
// CadRecoRecognitionBatch, CadRecoTrack, CadRecoVerify and CadRecoArbitrate.  R (9 floats, row-major) and t (3 floats, mm) take a
// point of the depth camera to the colour camera, X_colour = R * X_depth + t; fill_cracks (0 / 1) as fl_register_params.  Lens
// distortion is out of scope (vdDistCoeff is ignored, as everywhere).  on = 0 restores the behaviour without a depth camera byte
// for byte; the other arguments are then ignored.  ERROR_INVALID_PARAM: not a handle of this library, on or fill_cracks outside
// {0, 1}, and what fl_register_depth_batch refuses of a camera (a size outside 1..8192, fx or fy not finite and > 0, cx or cy not
// finite, a null or non-finite R or t, an R that is not a rotation); while it is on, a tDepth that is not of K_depth's size.
// ERROR_UNKNOW: no GPU, or a HIP error while a frame is registered.
int CadRecoSetDepthCamera(CObjRecoCAD *handle, int on, const TCamIntrinsicParam &K_depth, const float R[9], const float t[3], int fill_cracks);

#endif  // FEALESS_CADRECO_H
