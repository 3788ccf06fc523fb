// Stand-in of <opencv2/calib3d.hpp>: the reference's linemod/linemod.cpp includes it and uses nothing from it.
#ifndef FEALESS_REF_OPENCV_CALIB3D_HPP
#define FEALESS_REF_OPENCV_CALIB3D_HPP
#include "opencv2/core.hpp"
#endif
