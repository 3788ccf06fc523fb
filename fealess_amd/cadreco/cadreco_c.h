/* cadreco_c.h -- the flat C shim of libcadreco_hip.so: the C++ facade (fealess_cadreco.h) for callers without a C++ compiler,
 * which is how the test suite drives it (tests/cadreco_py.py holds the matching ctypes table).  A handle is the CObjRecoCAD *
 * of cadreco_create.  An image is (pixels, w, h_, ts); a camera is (fx, fy, cx, cy), of the image's size unless kw, kh are
 * given.  Poses are row-major 4x4 float matrices, 16 floats each.  Return values are the facade's codes unless stated. */
#ifndef FEALESS_CADRECO_C_H
#define FEALESS_CADRECO_C_H

#ifdef __cplusplus
extern "C" {
#endif

/* CObjRecoCAD::Create / Destroy / AddObj / GetVersion */
void *cadreco_create(int type);
void cadreco_destroy(void *h);
int cadreco_add_obj(void *h, const char *dir);
const char *cadreco_version(void);
/* the recognition parameters of the handle (fl_recognition_params); -1: not a handle of this library */
int cadreco_set_params(void *h, float thr, int it, float dmean, float ddiff, int mode);
int cadreco_set_multi_hypothesis(void *h, int k, float nms_dist_mm);
int cadreco_set_multi_instance(void *h, int max_instances, int min_dist_px, int hyp_per_instance);
int cadreco_set_verified_pick(void *h, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio);
int cadreco_set_verified_tracking(void *h, int on, float tau_mm, float min_inlier_ratio, float max_behind_ratio, int keep_input);
/* returns Recognition()'s code; *n_results = vtResult.size(); pose16 / tag filled for result 0 */
int cadreco_recognition(void *h, const unsigned char *bgr, const unsigned short *depth, int w, int h_, double ts, int kw, int kh,
                        double fx, double fy, double cx, double cy, int *n_results, float *pose16, char *tag, int tag_cap);
/* Recognition() returning every result: poses16 receives min(*n_results, cap) 4x4 matrices */
int cadreco_recognition_all(void *h, const unsigned char *bgr, const unsigned short *depth, int w, int h_, double ts, int kw, int kh,
                            double fx, double fy, double cx, double cy, int *n_results, float *poses16, int cap);

int cadreco_set_tracking_mesh(void *h, const char *obj_path, float scale);
/* CadRecoSetTrackingMeshes on n (class id, OBJ path) pairs */
int cadreco_set_tracking_meshes(void *h, int n, const char *const *class_ids, const char *const *obj_paths, float scale);
/* CadRecoTrack on n results: poses16 (n 4x4 matrices) goes in as the previous poses and comes out updated; tracked: n ints */
int cadreco_track(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                  float *poses16, int *tracked);
/* CadRecoVerify on n poses (n 4x4 matrices); out: n CadRecoVerifyResult records (8 x 4 bytes each) */
int cadreco_verify(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                   const float *poses16, float tau_mm, void *out);
/* cadreco_verify with a class id per pose (tags: n strings): what picks each pose's mesh after cadreco_set_tracking_meshes */
int cadreco_verify_tagged(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                          const float *poses16, const char *const *tags, float tau_mm, void *out);
/* CadRecoArbitrate on n poses (n 4x4 matrices; tags: n class ids, or NULL for none); out: n CadRecoSceneResult records (11 x 4
 * bytes each) */
int cadreco_arbitrate(void *h, const unsigned short *depth, int w, int h_, double ts, double fx, double fy, double cx, double cy, int n,
                      const float *poses16, const char *const *tags, float tau_mm, float max_shared_ratio, void *out);

/* CadRecoTrainViews on host views of one size w x h_; mask: NULL or n pointers (each may be NULL); template_of_view: n ints
 * (may be NULL), written on success */
int cadreco_train_views(void *h, const char *dir, const char *class_id, int n, const unsigned char *const *bgr,
                        const unsigned short *const *depth, const unsigned char *const *mask, int w, int h_, const float *poses13,
                        int levels, const int *T, int *template_of_view);
/* CadRecoTrainMesh; template_of_view: cap ints (may be NULL), written on success when they hold every view */
int cadreco_train_mesh(void *h, const char *dir, const char *class_id, const char *obj_path, float scale, int subdivisions, int upper_hemisphere,
                       const float *distances_mm, int n_distances, int n_inplane, float inplane_deg, int levels, const int *T,
                       int *template_of_view, int cap);

/* fealess::ReadObj: counts always (on success); the arrays when non-NULL and their caps hold them */
int cadreco_read_obj(const char *path, float scale, int *n_vertices, int *n_triangles, int *has_normals, float *vertices, float *normals,
                     int *triangles, int cap_vertices, int cap_triangles);
/* the file readers and the PNG writer of fealess_cadreco.h: 0, or -1 on failure (cadreco_read_png16: -2 when cap is too small) */
int cadreco_read_linemod(const char *path, int *levels, int *n_classes, int *n_templates, int *n_features);
int cadreco_read_linemod_cached(const char *path, int *from_cache, int *n_templates, int *n_features);
int cadreco_read_png16(const char *path, unsigned short *out, int cap, int *w, int *h);
int cadreco_write_png16(const char *path, const unsigned short *px, int w, int h);

#ifdef __cplusplus
}
#endif
#endif /* FEALESS_CADRECO_C_H */
