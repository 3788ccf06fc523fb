// Stand-in of <opencv2/core/core.hpp> (the OpenCV 2 spelling the reference's ICP sources use): everything is in opencv2/core.hpp.
#ifndef FEALESS_REF_OPENCV_CORE_CORE_HPP
#define FEALESS_REF_OPENCV_CORE_CORE_HPP
#include "opencv2/core.hpp"
#endif
