// forwards to the stand-in beside it (linemod_if.h includes it); see opencv2/core.hpp
#include "opencv2/imgproc.hpp"
