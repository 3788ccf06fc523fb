// Stand-in of <opencv2/imgproc.hpp> for compiling the reference's linemod/linemod.cpp; see opencv2/core.hpp beside it.
// One operation is defined (medianBlur with ksize 5 on CV_8UC1: the plain median of 25 values, replicated border: ours,
// and unambiguous).  Every filter whose kernel, work type or rounding is OpenCV's choice is declared only and aborts.
#ifndef FEALESS_REF_OPENCV_IMGPROC_HPP
#define FEALESS_REF_OPENCV_IMGPROC_HPP
#include "opencv2/core.hpp"

namespace cv {

enum InterpolationFlags { INTER_NEAREST = 0, INTER_LINEAR = 1 };
enum DistanceTypes { DIST_L1 = 1, DIST_L2 = 2, DIST_C = 3 };

inline void medianBlur(const Mat &src, Mat &dst, int ksize)
{
  if (ksize != 5 || src.type() != CV_8UC1) FEALESS_REF_UNPINNED("medianBlur (other than ksize 5 on CV_8UC1)");
  Mat in = src.clone();  // the reference calls it in place
  dst.create(in.rows, in.cols, CV_8UC1);
  for (int y = 0; y < in.rows; ++y)
    for (int x = 0; x < in.cols; ++x) {
      uchar v[25];
      int n = 0;
      for (int dy = -2; dy <= 2; ++dy)
        for (int dx = -2; dx <= 2; ++dx) {
          const int yy = std::min(std::max(y + dy, 0), in.rows - 1), xx = std::min(std::max(x + dx, 0), in.cols - 1);
          v[n++] = in.ptr(yy)[xx];
        }
      std::nth_element(v, v + 12, v + 25);
      dst.ptr(y)[x] = v[12];
    }
}

inline void GaussianBlur(const Mat &, Mat &, Size, double, double, int) { FEALESS_REF_UNPINNED("GaussianBlur"); }
inline void Sobel(const Mat &, Mat &, int, int, int, int, double, double, int) { FEALESS_REF_UNPINNED("Sobel"); }
inline void pyrDown(const Mat &, Mat &, const Size &) { FEALESS_REF_UNPINNED("pyrDown"); }
inline void resize(const Mat &, Mat &, Size, double, double, int) { FEALESS_REF_UNPINNED("resize"); }
inline void erode(const Mat &, Mat &, const Mat &, Point, int, int) { FEALESS_REF_UNPINNED("erode"); }
inline void distanceTransform(const Mat &, Mat &, int, int) { FEALESS_REF_UNPINNED("distanceTransform"); }
inline void cvtColor(const Mat &, Mat &, int) { FEALESS_REF_UNPINNED("cvtColor"); }

}  // namespace cv
#endif
