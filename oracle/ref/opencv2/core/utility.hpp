// Stand-in of <opencv2/core/utility.hpp>: checkHardwareSupport, alignSize and format live in opencv2/core.hpp here.
#ifndef FEALESS_REF_OPENCV_CORE_UTILITY_HPP
#define FEALESS_REF_OPENCV_CORE_UTILITY_HPP
#include "opencv2/core.hpp"
#endif
