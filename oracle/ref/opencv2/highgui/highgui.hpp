// Stand-in of <opencv2/highgui/highgui.hpp>: the window functions that the reference's ICP/common.cpp names in
// show_image(), which nothing that is compared ever calls.  Declared only.
#ifndef FEALESS_REF_OPENCV_HIGHGUI_HIGHGUI_HPP
#define FEALESS_REF_OPENCV_HIGHGUI_HIGHGUI_HPP
#include "opencv2/core.hpp"

#define CV_WINDOW_AUTOSIZE 1

namespace cv {

inline void namedWindow(const String &, int = 1) { FEALESS_REF_UNPINNED("namedWindow"); }
inline void imshow(const String &, const Mat &) { FEALESS_REF_UNPINNED("imshow"); }
inline int waitKey(int = 0) { FEALESS_REF_UNPINNED("waitKey"); }

}  // namespace cv
#endif
