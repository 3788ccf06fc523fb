// Stand-in of <opencv2/imgproc.hpp> for compiling the reference's linemod/linemod.cpp; see opencv2/core.hpp beside it.
// One operation is defined here as OURS (medianBlur with ksize 5 on CV_8UC1: the plain median of 25 values, replicated
// border, unambiguous).  The filters of template extraction, whose kernel, work type or rounding is OpenCV's choice, are
// DELEGATED to the oracle's restatement of them in ../liboracle.so, for exactly the argument patterns linemod.cpp uses:
//   GaussianBlur(8UC3, Size(7,7), 0, 0, BORDER_REPLICATE)            -> orc_gaussian7_bgr          (linemod.cpp:247)
//   Sobel(8UC3, CV_16S, 1|0, 0|1, 3, 1.0, 0.0, BORDER_REPLICATE)     -> orc_sobel3_bgr             (:248-249)
//   pyrDown(8UC3, Size(cols / 2, rows / 2))                          -> orc_pyrdown_bgr            (:443)
//   resize(8UC1, Size(cols / 2, rows / 2), 0, 0, INTER_NEAREST)      -> orc_resize_nn_half         (:448, :731, :736)
//   erode(8UC1, Mat(), Point(-1,-1), 1|2, BORDER_REPLICATE)          -> orc_erode_rect             (:467, :753)
//   distanceTransform(8UC1, DIST_C, 3)                               -> orc_distance_transform_c3  (:764)
// The oracle and the compiled reference then run the SAME code for these, so their arithmetic is NOT PINNED by any
// comparison of the two; every other argument pattern, and cvtColor, aborts with its name (FEALESS_REF_UNPINNED).
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

// A Mat's rows back to back (a ROI has gaps between them), and back into a fresh Mat: the oracle works on plain arrays
template <typename T> inline std::vector<T> fealess_packed(const Mat &m)
{
  const size_t row = (size_t)m.cols * m.channels();
  std::vector<T> v(row * (size_t)m.rows);
  for (int r = 0; r < m.rows; ++r) std::memcpy(v.data() + row * r, m.ptr(r), row * sizeof(T));
  return v;
}
template <typename T> inline void fealess_unpack(const std::vector<T> &v, int rows, int cols, int type, Mat &dst)
{
  Mat out(rows, cols, type);  // not dst.create(): dst may be the source
  const size_t row = (size_t)cols * CV_MAT_CN(type);
  for (int r = 0; r < rows; ++r) std::memcpy(out.ptr(r), v.data() + row * r, row * sizeof(T));
  dst = out;
}

inline void GaussianBlur(const Mat &src, Mat &dst, Size ksize, double sigma_x, double sigma_y, int border)
{
  if (src.empty() || src.type() != CV_8UC3 || ksize.width != 7 || ksize.height != 7 || sigma_x != 0 || sigma_y != 0 || border != BORDER_REPLICATE)
    FEALESS_REF_UNPINNED("GaussianBlur (other than 7x7, sigma 0, BORDER_REPLICATE on CV_8UC3)");
  const std::vector<uchar> in = fealess_packed<uchar>(src);
  std::vector<uchar> out(in.size());
  orc_gaussian7_bgr(in.data(), src.cols, src.rows, out.data());
  fealess_unpack(out, src.rows, src.cols, CV_8UC3, dst);
}

inline void Sobel(const Mat &src, Mat &dst, int ddepth, int dx, int dy, int ksize, double scale, double delta, int border)
{
  if (src.empty() || src.type() != CV_8UC3 || ddepth != CV_16S || !((dx == 1 && dy == 0) || (dx == 0 && dy == 1)) || ksize != 3 || scale != 1.0 ||
      delta != 0.0 || border != BORDER_REPLICATE)
    FEALESS_REF_UNPINNED("Sobel (other than first order, CV_16S, ksize 3, BORDER_REPLICATE on CV_8UC3)");
  const std::vector<uchar> in = fealess_packed<uchar>(src);
  std::vector<short> out(in.size());
  orc_sobel3_bgr(in.data(), src.cols, src.rows, dy, out.data());
  fealess_unpack(out, src.rows, src.cols, CV_16SC3, dst);
}

inline void pyrDown(const Mat &src, Mat &dst, const Size &size)
{
  if (src.empty() || src.type() != CV_8UC3 || size.width != src.cols / 2 || size.height != src.rows / 2 || size.width < 1 || size.height < 1)
    FEALESS_REF_UNPINNED("pyrDown (other than CV_8UC3 to Size(cols / 2, rows / 2))");
  const std::vector<uchar> in = fealess_packed<uchar>(src);
  std::vector<uchar> out((size_t)size.width * size.height * 3);
  orc_pyrdown_bgr(in.data(), src.cols, src.rows, out.data());
  fealess_unpack(out, size.height, size.width, CV_8UC3, dst);
}

inline void resize(const Mat &src, Mat &dst, Size size, double fx, double fy, int interpolation)
{
  if (src.empty() || src.type() != CV_8UC1 || size.width != src.cols / 2 || size.height != src.rows / 2 || size.width < 1 || size.height < 1 ||
      fx != 0.0 || fy != 0.0 || interpolation != INTER_NEAREST)
    FEALESS_REF_UNPINNED("resize (other than INTER_NEAREST of CV_8UC1 to Size(cols / 2, rows / 2))");
  const std::vector<uchar> in = fealess_packed<uchar>(src);
  std::vector<uchar> out((size_t)size.width * size.height);
  orc_resize_nn_half(in.data(), src.cols, src.rows, out.data());
  fealess_unpack(out, size.height, size.width, CV_8UC1, dst);
}

inline void erode(const Mat &src, Mat &dst, const Mat &kernel, Point anchor, int iterations, int border)
{
  if (src.empty() || src.type() != CV_8UC1 || !kernel.empty() || anchor.x != -1 || anchor.y != -1 || iterations < 1 || iterations > 2 ||
      border != BORDER_REPLICATE)
    FEALESS_REF_UNPINNED("erode (other than the default 3x3 rectangle, 1 or 2 iterations, BORDER_REPLICATE on CV_8UC1)");
  const std::vector<uchar> in = fealess_packed<uchar>(src);
  std::vector<uchar> out(in.size());
  orc_erode_rect(in.data(), src.cols, src.rows, iterations, out.data());
  fealess_unpack(out, src.rows, src.cols, CV_8UC1, dst);
}

inline void distanceTransform(const Mat &src, Mat &dst, int distance_type, int mask_size)
{
  if (src.empty() || src.type() != CV_8UC1 || distance_type != DIST_C || mask_size != 3)
    FEALESS_REF_UNPINNED("distanceTransform (other than DIST_C, 3 on CV_8UC1)");
  const std::vector<uchar> in = fealess_packed<uchar>(src);
  std::vector<float> out(in.size());
  orc_distance_transform_c3(in.data(), src.cols, src.rows, out.data());
  fealess_unpack(out, src.rows, src.cols, CV_32FC1, dst);
}

inline void cvtColor(const Mat &, Mat &, int) { FEALESS_REF_UNPINNED("cvtColor"); }

// cv::circle draws NOTHING here: it appends its arguments to a process-wide log that the caller reads and clears
// (tests/dropin/tu_cv_caller.cpp compares the order and arguments of drawResponse's calls; rasterisation is OpenCV's)
struct FealessCircleCall {
  Point center;
  int radius;
  Scalar color;
  int thickness;
};
inline std::vector<FealessCircleCall> &fealess_circle_log()
{
  static std::vector<FealessCircleCall> log;
  return log;
}
inline void circle(Mat &, Point center, int radius, const Scalar &color, int thickness = 1, int = 8, int = 0)
{
  const FealessCircleCall c = {center, radius, color, thickness};
  fealess_circle_log().push_back(c);
}

}  // namespace cv
#endif
