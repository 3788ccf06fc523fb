/* cadreco_depth_c.h -- the flat C shim of CadRecoSetDepthCamera (fealess_cadreco.h), exported from libcadreco_hip.so beside the
 * functions of cadreco_c.h and with their conventions (tests/cadreco_depth_py.py holds the matching ctypes table). */
#ifndef FEALESS_CADRECO_DEPTH_C_H
#define FEALESS_CADRECO_DEPTH_C_H

#ifdef __cplusplus
extern "C" {
#endif

/* CadRecoSetDepthCamera: the depth camera is (dw, dh, fx, fy, cx, cy); R (9 floats, row-major) and t (3 floats, mm) take a point
 * of the depth camera to the colour camera.  on outside {0, 1}, or a null R or t with on = 1: ERROR_INVALID_PARAM before anything
 * touches the handle. */
int cadreco_set_depth_camera(void *h, int on, int dw, int dh, double fx, double fy, double cx, double cy, const float *R, const float *t,
                             int fill_cracks);
/* cadreco_recognition (cadreco_c.h) with a depth image of its own size dw x dh_: what Recognition() takes while a depth camera
 * is set.  The colour image and the camera (fx, fy, cx, cy) are w x h_. */
int cadreco_recognition_depth(void *h, const unsigned char *bgr, int w, int h_, const unsigned short *depth, int dw, int dh_, double ts,
                              double fx, double fy, double cx, double cy, int *n_results, float *pose16, char *tag, int tag_cap);

#ifdef __cplusplus
}
#endif
#endif /* FEALESS_CADRECO_DEPTH_C_H */
