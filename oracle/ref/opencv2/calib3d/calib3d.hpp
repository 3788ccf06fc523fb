// Stand-in of <opencv2/calib3d/calib3d.hpp>: Rodrigues, which the reference's ICP/pose_result.h names for a rotation
// given as a 3-vector (nonMaximumSuppression hands it 3x3 matrices).  Declared only.
#ifndef FEALESS_REF_OPENCV_CALIB3D_CALIB3D_HPP
#define FEALESS_REF_OPENCV_CALIB3D_CALIB3D_HPP
#include "opencv2/calib3d.hpp"

namespace cv {

inline void Rodrigues(const Mat &, Mat &) { FEALESS_REF_UNPINNED("Rodrigues"); }

}  // namespace cv
#endif
