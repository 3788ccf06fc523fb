// Stand-in of <opencv2/imgproc/imgproc.hpp>: the reference's ICP/detection.cpp includes it and uses nothing from it
// outside its TEST_DETECT blocks, which are not compiled.
#ifndef FEALESS_REF_OPENCV_IMGPROC_IMGPROC_HPP
#define FEALESS_REF_OPENCV_IMGPROC_IMGPROC_HPP
#include "opencv2/imgproc.hpp"
#endif
