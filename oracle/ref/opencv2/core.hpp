// Container-only stand-in of <opencv2/core.hpp>, written from scratch for ONE purpose: to compile the reference's
// linemod/linemod.cpp and its ICP sources (ICP.cpp, common.cpp, depth_to_3d.cpp, detection.cpp, NMS.cpp) unchanged
// (oracle/ref/ref_harness.cpp and oracle/ref/icp_harness.cpp include them by include path at build time) on a machine
// without OpenCV, so that the oracle and the HIP kernels can be compared with the reference's own compiled arithmetic.
// TEST INFRASTRUCTURE ONLY; nothing here is part of the product, and nothing here is copied from OpenCV or the reference.
//
// What is real here, and what is not:
//
//  * CONTAINERS have real definitions: Mat (reference counted; rows/cols/data/step, type(), ptr<T>(r), at<T>(r,c),
//    step1(), create, zeros, clone, copyTo, setTo, size(), total(), empty(), ROI operator()(Rect)), Mat_<T>, Size, Point,
//    Rect, Vec3b, Ptr/makePtr, String, CV_Assert/CV_Error (throw cv::Exception), alignSize, checkHardwareSupport,
//    OutputArrayOfArrays/noArray() with needed/create/getMatRef.  The arithmetic linemod.cpp does on them is its own C++.
//    For the OpenCV-typed adapter header and the caller that runs it against the compiled reference
//    (tests/dropin/tu_cv_caller.cpp): Mat(rows, cols, type, data, step) over caller memory (no ownership, no guard),
//    Mat::isContinuous(), Mat::copyTo(OutputArray) for a Mat target, Error::StsError and Exception::code, Scalar(b, g, r)
//    and CV_RGB, convertTo CV_32F -> CV_64F and CV_64F -> CV_64F with alpha 1 (exact), empty forwarding headers for what
//    linemod_if.h includes (imgproc/imgproc_c.h, objdetect.hpp, highgui.hpp), and a cv::circle (opencv2/imgproc.hpp) that
//    draws nothing and appends its arguments to a process-wide log: the calls are compared, OpenCV's rasterisation is
//    not restated.  FileStorage stays declared only.
//
//  * THE OPERATIONS the pinned functions call are defined here, because each has one possible answer:
//      - Mat::convertTo(CV_8U -> CV_16U) widens every byte (addSimilarities with one modality, linemod.cpp:1326);
//      - Mat::convertTo(CV_32F -> CV_8U, alpha) is saturate_cast<uchar>(cvRound(x * alpha)): the product formed in
//        double, rounded half to even, clamped to [0, 255] (hysteresisGradient, linemod.cpp:314).  A library that forms
//        the product in float instead agrees with this on every float in [0, 360] for alpha = 16/360 except two,
//        123.749992 and 213.749985 (exhaustive search over all 1 135 869 953 of them); the tests keep those two out of
//        their inputs by construction and assert it, so this definition decides nothing that is checked;
//      - medianBlur(src, dst, 5) on CV_8UC1 is the plain median of the 25 values of the 5x5 window with a replicated
//        border (quantizedNormals, linemod.cpp:684).  A median of 25 values has no rounding and no tie to break.
//      - subtract (saturating), bitwise_and, countNonZero and Mat::setTo(value, mask) on CV_8UC1 (the two
//        extractTemplate methods, linemod.cpp:468, :761-762, :815): integer operations per element, nothing to round.
//    They are OURS, not OpenCV's code, and are named here so that nobody takes them for more than that.
//
//  * THE OPERATIONS OF TEMPLATE EXTRACTION whose kernel, work type or rounding is OpenCV's choice are DELEGATED to the
//    oracle's restatement in ../liboracle.so, for exactly the argument patterns linemod.cpp uses (anything else aborts):
//    phase in degrees -> orc_fast_atan2 (here); GaussianBlur 7x7 -> orc_gaussian7_bgr, Sobel CV_16S ksize 3 ->
//    orc_sobel3_bgr, pyrDown -> orc_pyrdown_bgr, resize INTER_NEAREST to exact halves -> orc_resize_nn_half, erode 3x3 ->
//    orc_erode_rect, distanceTransform(DIST_C, 3) -> orc_distance_transform_c3 (opencv2/imgproc.hpp).  Both sides then
//    run the same code for them: that arithmetic is NOT PINNED.  What the compiled reference pins around them is its own
//    control flow, comparisons, operand order and conversions (oracle/ref/ref_harness.cpp lists both, item by item).
//
//  * EVERYTHING ELSE linemod.cpp names is DECLARED ONLY and given a body that aborts with its name (FEALESS_REF_UNPINNED):
//    add, cvtColor, every other Mat::convertTo, every other argument pattern of the operations above, FileStorage/FileNode
//    I/O and format.  This stand-in does not re-implement OpenCV arithmetic a second time and call it a reference.
//
//  * FOR THE ICP SOURCES (oracle/ref/icp_harness.cpp lists, item by item, which of these is OpenCV's header text restated
//    and which is a choice of ours): Vec<T,n> and Matx<T,m,n> with the element-wise operators and the products of
//    OpenCV's matx.hpp (s = 0; s += a(i,k) * b(k,j), in T); Mat_<T> with ROIs, element access and iterators that walk a
//    ROI row by row; Rect_<T>; _InputArray / _OutputArray over a Mat; cv::norm (squares accumulated in double), cv::add
//    on Vec, cv::checkRange (every element finite), Mat == scalar, setTo(value, mask) on CV_32FC1, getTickCount, and
//    the conversions CV_16U -> CV_32F with a scale (float(v) * float(alpha)), CV_64F -> CV_32F and same-type copies;
//    Mat * Mat on CV_32FC1 (double accumulators, as cv::gemm) and Mat::t().  cv::SVD::compute is declared here and
//    defined by icp_harness.cpp on the oracle's orc_svd3.  The Mat expression arithmetic of depthTo3d_from_uvz, merge,
//    split, reshape, resize(n), Mat(std::vector), Rodrigues and the window functions are declared only.
//
//  * THE ALLOCATOR zero-fills every buffer and puts a zeroed guard of two rows plus 4 KiB after it.  The reference reads
//    past the last grid row of a linear memory (quirk Q2): undefined behaviour there, deterministic here, with the value
//    the project already defined for it (reads 0).
#ifndef FEALESS_REF_OPENCV_CORE_HPP
#define FEALESS_REF_OPENCV_CORE_HPP

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#ifndef CV_SSE2
#define CV_SSE2 0
#endif
#ifndef CV_SSE3
#define CV_SSE3 0
#endif
#ifndef CV_SSSE3
#define CV_SSSE3 0
#endif
#if CV_SSE2
#include <emmintrin.h>
#endif
#if CV_SSE3
#include <pmmintrin.h>
#endif
#if CV_SSSE3
#include <tmmintrin.h>
#endif

typedef unsigned char uchar;
typedef unsigned short ushort;
#include <stdint.h>
typedef int64_t int64;
#include "../../fealess_oracle.h"  // the orc_* restatements that the delegated operations call (../liboracle.so)

#define CV_MAJOR_VERSION 3

#define CV_8U 0
#define CV_8S 1
#define CV_16U 2
#define CV_16S 3
#define CV_32S 4
#define CV_32F 5
#define CV_64F 6
#define CV_MAT_DEPTH(t) ((t) & 7)
#define CV_MAT_CN(t) ((((t) >> 3) & 511) + 1)
#define CV_MAKETYPE(depth, cn) (CV_MAT_DEPTH(depth) + (((cn) - 1) << 3))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_16UC1 CV_MAKETYPE(CV_16U, 1)
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_16UC3 CV_MAKETYPE(CV_16U, 3)
#define CV_16SC1 CV_MAKETYPE(CV_16S, 1)
#define CV_16SC3 CV_MAKETYPE(CV_16S, 3)
#define CV_32FC2 CV_MAKETYPE(CV_32F, 2)
#define CV_32FC3 CV_MAKETYPE(CV_32F, 3)
#define CV_64FC1 CV_MAKETYPE(CV_64F, 1)

#define CV_CPU_SSE2 3
#define CV_CPU_SSE3 4
#define CV_CPU_SSSE3 5

#define CV_DECL_ALIGNED(x) __attribute__((aligned(x)))

#define FEALESS_REF_UNPINNED(name)                                                                          \
  do {                                                                                                      \
    std::fprintf(stderr, "oracle/ref stand-in: %s is declared only (OpenCV arithmetic stays unpinned)\n", name); \
    std::abort();                                                                                           \
  } while (0)

inline int cvIsNaN(double v) { return std::isnan(v) ? 1 : 0; }

namespace cv {

typedef std::string String;

// What the reference's ICP loop does not return but the stand-in sees it do (oracle/ref/icp_harness.cpp derives the
// loop's final `iter` from them): searches of the cvflann index, and checkRange calls on a 3x3 matrix.
struct FealessRefCounters { long knn_searches, check_range_3x3; };
inline FealessRefCounters &fealess_ref_counters()
{
  static FealessRefCounters c = {0, 0};
  return c;
}

class Exception : public std::runtime_error {
 public:
  explicit Exception(const std::string &what_, int code_ = 0) : std::runtime_error(what_), code(code_) {}
  int code;  // the cv::Error::Code it was raised with
};
namespace Error { enum Code { StsError = -2, StsBadArg = -5, StsAssert = -215 }; }
[[noreturn]] inline void error(int code, const String &msg, const char *file, int line)
{
  throw Exception(String(file) + ":" + std::to_string(line) + ": error " + std::to_string(code) + ": " + msg, code);
}

#define CV_Error(code, msg) cv::error((code), (msg), __FILE__, __LINE__)
#define CV_Assert(expr) do { if (!(expr)) cv::error(cv::Error::StsAssert, #expr, __FILE__, __LINE__); } while (0)
#define CV_DbgAssert(expr) do { } while (0)

enum { CPU_SSE2 = CV_CPU_SSE2, CPU_SSE3 = CV_CPU_SSE3, CPU_SSSE3 = CV_CPU_SSSE3 };
// the SIMD build of the harness is the build whose host has the three extensions; the scalar build never asks
inline bool checkHardwareSupport(int) { return CV_SSE2 != 0; }

inline size_t alignSize(size_t sz, int n) { return (sz + n - 1) & ~(size_t)(n - 1); }

template <typename T> using Ptr = std::shared_ptr<T>;
template <typename T, typename... A> inline Ptr<T> makePtr(A &&...a) { return std::make_shared<T>(std::forward<A>(a)...); }

struct Size {
  int width, height;
  Size() : width(0), height(0) {}
  Size(int w, int h) : width(w), height(h) {}
  bool operator==(const Size &o) const { return width == o.width && height == o.height; }
  bool operator!=(const Size &o) const { return !(*this == o); }
  int area() const { return width * height; }
};
struct Point {
  int x, y;
  Point() : x(0), y(0) {}
  Point(int x_, int y_) : x(x_), y(y_) {}
};
template <typename T> struct Rect_ {
  T x, y, width, height;
  Rect_() : x(0), y(0), width(0), height(0) {}
  Rect_(T x_, T y_, T w, T h) : x(x_), y(y_), width(w), height(h) {}
};
typedef Rect_<int> Rect;
struct Vec3b {
  uchar val[3];
  Vec3b() { val[0] = val[1] = val[2] = 0; }
  Vec3b(uchar a, uchar b, uchar c) { val[0] = a; val[1] = b; val[2] = c; }
  uchar &operator[](int i) { return val[i]; }
  const uchar &operator[](int i) const { return val[i]; }
};
struct Scalar {
  double val[4];
  Scalar(double a = 0, double b = 0, double c = 0, double d = 0) { val[0] = a; val[1] = b; val[2] = c; val[3] = d; }
};
#define CV_RGB(r, g, b) cv::Scalar((b), (g), (r), 0)

enum BorderTypes { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4 };

// ---- Matx / Vec: small fixed-size matrices, as OpenCV's matx.hpp states them ----------------------------------------------
// Default construction zeroes; a product is `s = 0; s += a(i,k) * b(k,j)` in T, k ascending; the element-wise operators
// are one T operation per element.
template <typename T, int m, int n> class Matx {
 public:
  enum { rows = m, cols = n, channels = m * n };
  T val[m * n];
  Matx() { for (int i = 0; i < m * n; ++i) val[i] = T(0); }
  Matx(T v0, T v1) { static_assert(m * n >= 2, "Matx"); zero(); val[0] = v0; val[1] = v1; }
  Matx(T v0, T v1, T v2) { static_assert(m * n >= 3, "Matx"); zero(); val[0] = v0; val[1] = v1; val[2] = v2; }
  Matx(T v0, T v1, T v2, T v3, T v4, T v5, T v6, T v7, T v8)
  {
    static_assert(m * n >= 9, "Matx");
    zero();
    val[0] = v0; val[1] = v1; val[2] = v2; val[3] = v3; val[4] = v4; val[5] = v5; val[6] = v6; val[7] = v7; val[8] = v8;
  }
  static Matx eye()
  {
    Matx M;
    for (int i = 0; i < (m < n ? m : n); ++i) M(i, i) = T(1);
    return M;
  }
  T &operator()(int i, int j) { return val[i * n + j]; }
  const T &operator()(int i, int j) const { return val[i * n + j]; }
  T &operator()(int i) { return val[i]; }
  const T &operator()(int i) const { return val[i]; }
  Matx<T, n, m> t() const
  {
    Matx<T, n, m> r;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < n; ++j) r(j, i) = (*this)(i, j);
    return r;
  }

 private:
  void zero() { for (int i = 0; i < m * n; ++i) val[i] = T(0); }
};

template <typename T, int cn> class Vec : public Matx<T, cn, 1> {
 public:
  Vec() {}
  Vec(T v0, T v1) : Matx<T, cn, 1>(v0, v1) {}
  Vec(T v0, T v1, T v2) : Matx<T, cn, 1>(v0, v1, v2) {}
  Vec(const Matx<T, cn, 1> &a) : Matx<T, cn, 1>(a) {}
  T &operator[](int i) { return this->val[i]; }
  const T &operator[](int i) const { return this->val[i]; }
};
typedef Vec<float, 2> Vec2f;
typedef Vec<float, 3> Vec3f;
typedef Vec<double, 3> Vec3d;
typedef Matx<float, 3, 3> Matx33f;
typedef Matx<double, 3, 3> Matx33d;

template <typename T, int m, int n> inline Matx<T, m, n> &operator+=(Matx<T, m, n> &a, const Matx<T, m, n> &b)
{
  for (int i = 0; i < m * n; ++i) a.val[i] = a.val[i] + b.val[i];
  return a;
}
template <typename T, int m, int n> inline Matx<T, m, n> &operator-=(Matx<T, m, n> &a, const Matx<T, m, n> &b)
{
  for (int i = 0; i < m * n; ++i) a.val[i] = a.val[i] - b.val[i];
  return a;
}
template <typename T, int m, int n> inline Matx<T, m, n> operator-(const Matx<T, m, n> &a)
{
  Matx<T, m, n> r;
  for (int i = 0; i < m * n; ++i) r.val[i] = -a.val[i];
  return r;
}
template <typename T, int cn> inline Vec<T, cn> operator+(const Vec<T, cn> &a, const Vec<T, cn> &b)
{
  Vec<T, cn> r;
  for (int i = 0; i < cn; ++i) r.val[i] = a.val[i] + b.val[i];
  return r;
}
template <typename T, int cn> inline Vec<T, cn> operator-(const Vec<T, cn> &a, const Vec<T, cn> &b)
{
  Vec<T, cn> r;
  for (int i = 0; i < cn; ++i) r.val[i] = a.val[i] - b.val[i];
  return r;
}
// Vec *= int multiplies in T (matx.hpp: saturate_cast<T>(a[i] * alpha), the int promoted to T)
template <typename T, int cn> inline Vec<T, cn> &operator*=(Vec<T, cn> &a, int alpha)
{
  for (int i = 0; i < cn; ++i) a.val[i] = a.val[i] * (T)alpha;
  return a;
}
template <typename T, int m, int l, int n> inline Matx<T, m, n> operator*(const Matx<T, m, l> &a, const Matx<T, l, n> &b)
{
  Matx<T, m, n> r;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) {
      T s = 0;
      for (int k = 0; k < l; ++k) s += a(i, k) * b(k, j);
      r(i, j) = s;
    }
  return r;
}
template <typename T, int m, int n> inline Vec<T, m> operator*(const Matx<T, m, n> &a, const Vec<T, n> &b)
{
  return Vec<T, m>(a * static_cast<const Matx<T, n, 1> &>(b));
}
// cv::norm of a Matx: the squares accumulated in double in element order, the root in double
template <typename T, int m, int n> inline double norm(const Matx<T, m, n> &a)
{
  double s = 0;
  for (int i = 0; i < m * n; ++i) s += (double)a.val[i] * a.val[i];
  return std::sqrt(s);
}
template <typename T, int cn> inline void add(const Vec<T, cn> &a, const Vec<T, cn> &b, Vec<T, cn> &c) { c = a + b; }
// cv::checkRange with its default bounds (-DBL_MAX, DBL_MAX): every element finite
template <typename T, int m, int n> inline bool checkRange(const Matx<T, m, n> &a)
{
  if (m == 3 && n == 3) ++fealess_ref_counters().check_range_3x3;
  for (int i = 0; i < m * n; ++i)
    if (!std::isfinite(a.val[i])) return false;
  return true;
}

template <typename T> struct DataType;
template <> struct DataType<uchar> { enum { depth = CV_8U, type = CV_8UC1 }; };
template <> struct DataType<ushort> { enum { depth = CV_16U, type = CV_16UC1 }; };
template <> struct DataType<short> { enum { depth = CV_16S, type = CV_16SC1 }; };
template <> struct DataType<int> { enum { depth = CV_32S, type = CV_MAKETYPE(CV_32S, 1) }; };
template <> struct DataType<float> { enum { depth = CV_32F, type = CV_32FC1 }; };
template <> struct DataType<double> { enum { depth = CV_64F, type = CV_64FC1 }; };
template <typename T, int cn> struct DataType<Vec<T, cn> > { enum { depth = DataType<T>::depth, type = CV_MAKETYPE(DataType<T>::depth, cn) }; };

class Mat;
template <typename T> class MatConstIterator_;
template <typename T> class MatIterator_;
// Mat::size: callable (m.size()) and comparable (a.size == b.size)
struct MSize {
  const Mat *m;
  explicit MSize(const Mat *m_) : m(m_) {}
  inline Size operator()() const;
  inline bool operator==(const MSize &o) const;
  bool operator!=(const MSize &o) const { return !(*this == o); }
};

class Mat {
 public:
  int rows, cols;
  uchar *data;
  size_t step;  // bytes per row
  MSize size;

  Mat() : rows(0), cols(0), data(NULL), step(0), size(this), type_(0) {}
  Mat(int r, int c, int type) : rows(0), cols(0), data(NULL), step(0), size(this), type_(0) { create(r, c, type); }
  Mat(Size s, int type) : rows(0), cols(0), data(NULL), step(0), size(this), type_(0) { create(s.height, s.width, type); }
  // a header over the caller's memory: no ownership, no guard behind it; step 0 = rows back to back
  Mat(int r, int c, int type, void *data_, size_t step_ = 0)
      : rows(r), cols(c), data(static_cast<uchar *>(data_)), step(step_ ? step_ : (size_t)c * depthSize(type) * CV_MAT_CN(type)), size(this), type_(type)
  {
  }
  Mat(const Mat &m) : rows(m.rows), cols(m.cols), data(m.data), step(m.step), size(this), type_(m.type_), buf_(m.buf_) {}
  Mat &operator=(const Mat &m)
  {
    assignFrom(m);
    return *this;
  }
  template <typename T, int m, int n> explicit Mat(const Matx<T, m, n> &M) : rows(0), cols(0), data(NULL), step(0), size(this), type_(0)
  {
    create(m, n, DataType<T>::type);
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < n; ++j) ptr<T>(i)[j] = M(i, j);
  }
  template <typename T> explicit Mat(const std::vector<T> &) : rows(0), cols(0), data(NULL), step(0), size(this), type_(0)
  {
    FEALESS_REF_UNPINNED("Mat(std::vector)");
  }
  template <typename T, int m, int n> operator Matx<T, m, n>() const
  {
    CV_Assert(rows == m && cols == n && type_ == (int)DataType<T>::type);
    Matx<T, m, n> M;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < n; ++j) M(i, j) = ptr<T>(i)[j];
    return M;
  }

  static size_t depthSize(int type)
  {
    static const size_t sz[8] = {1, 1, 2, 2, 4, 4, 8, 0};
    return sz[CV_MAT_DEPTH(type)];
  }
  int type() const { return type_; }
  int depth() const { return CV_MAT_DEPTH(type_); }
  int channels() const { return CV_MAT_CN(type_); }
  size_t elemSize1() const { return depthSize(type_); }
  size_t elemSize() const { return depthSize(type_) * CV_MAT_CN(type_); }
  size_t step1() const { return step / elemSize1(); }
  size_t total() const { return (size_t)rows * cols; }
  bool empty() const { return data == NULL || rows == 0 || cols == 0; }
  bool isContinuous() const { return rows <= 1 || step == (size_t)cols * elemSize(); }

  // A fresh buffer unless the shape and type already fit (as cv::Mat::create).  Zero-filled, 64-byte aligned, followed
  // by a zeroed guard of two rows + 4 KiB (see the header comment: quirk Q2).
  void create(int r, int c, int type)
  {
    if (data && r == rows && c == cols && type == type_ && step == (size_t)c * elemSize()) return;
    type_ = type;
    rows = r;
    cols = c;
    step = (size_t)c * elemSize();
    const size_t bytes = step * (size_t)r, guard = 2 * step + 4096;
    void *p = NULL;
    if (posix_memalign(&p, 64, alignSize(bytes + guard, 64)) != 0) throw std::bad_alloc();
    std::memset(p, 0, alignSize(bytes + guard, 64));
    buf_ = std::shared_ptr<void>(p, std::free);
    data = static_cast<uchar *>(p);
  }
  void create(Size s, int type) { create(s.height, s.width, type); }
  static Mat zeros(int r, int c, int type)
  {
    Mat m;
    m.create(r, c, type);  // a Mat() has no buffer, so create() allocates, and allocation zero-fills
    return m;
  }
  static Mat zeros(Size s, int type) { return zeros(s.height, s.width, type); }

  template <typename T> T *ptr(int r = 0) { return reinterpret_cast<T *>(data + step * (size_t)r); }
  template <typename T> const T *ptr(int r = 0) const { return reinterpret_cast<const T *>(data + step * (size_t)r); }
  uchar *ptr(int r = 0) { return data + step * (size_t)r; }
  const uchar *ptr(int r = 0) const { return data + step * (size_t)r; }
  template <typename T> T &at(int r, int c) { return ptr<T>(r)[c]; }
  template <typename T> const T &at(int r, int c) const { return ptr<T>(r)[c]; }
  template <typename T> T *ptr(int r, int c) { return ptr<T>(r) + c; }
  template <typename T> const T *ptr(int r, int c) const { return ptr<T>(r) + c; }
  template <typename T> inline MatIterator_<T> begin();
  template <typename T> inline MatIterator_<T> end();
  template <typename T> inline MatConstIterator_<T> begin() const;
  template <typename T> inline MatConstIterator_<T> end() const;

  // a ROI that leaves the matrix is refused, as cv::Mat's constructor asserts
  Mat operator()(const Rect &roi) const
  {
    CV_Assert(0 <= roi.x && 0 <= roi.width && roi.x + roi.width <= cols && 0 <= roi.y && 0 <= roi.height && roi.y + roi.height <= rows);
    Mat m(*this);
    m.data = data + step * (size_t)roi.y + elemSize() * (size_t)roi.x;
    m.rows = roi.height;
    m.cols = roi.width;
    return m;
  }
  Mat clone() const
  {
    Mat m;
    copyTo(m);
    return m;
  }
  void copyTo(Mat &dst) const
  {
    if (empty()) { dst = Mat(); return; }
    if (dst.data == data && dst.rows == rows && dst.cols == cols) return;
    dst.create(rows, cols, type_);
    for (int r = 0; r < rows; ++r) std::memcpy(dst.ptr(r), ptr(r), (size_t)cols * elemSize());
  }
  // elements of *this where mask (CV_8UC1, same size) is non-zero; an empty mask copies everything
  void copyTo(Mat &dst, const Mat &mask) const
  {
    if (mask.empty()) { copyTo(dst); return; }
    CV_Assert(mask.rows == rows && mask.cols == cols && mask.type() == CV_8UC1);
    if (dst.rows != rows || dst.cols != cols || dst.type() != type_) dst = zeros(rows, cols, type_);
    const size_t es = elemSize();
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c)
        if (mask.ptr(r)[c]) std::memcpy(dst.ptr(r) + es * c, ptr(r) + es * c, es);
  }
  Mat &setTo(const Scalar &v, const Mat &mask = Mat())
  {
    CV_Assert(type_ == CV_8UC1 || type_ == CV_32FC1);
    CV_Assert(mask.empty() || (mask.rows == rows && mask.cols == cols && mask.type() == CV_8UC1));
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c)
        if (mask.empty() || mask.ptr(r)[c]) {
          if (type_ == CV_8UC1) ptr(r)[c] = (uchar)v.val[0];
          else ptr<float>(r)[c] = (float)v.val[0];
        }
    return *this;
  }
  // defined for CV_8U -> CV_16U (alpha 1) and CV_32F -> CV_8U (any alpha), beta 0, one channel (see the header comment),
  // and for what the ICP sources convert: a copy (same depth, alpha 1), CV_64F -> CV_32F (alpha 1) and CV_16U -> CV_32F
  // with a scale, float(v) * float(alpha): the scale narrowed to the destination's type before the product, which is
  // what a cv::Mat::convertTo to CV_32F does; and CV_32F -> CV_64F (alpha 1), which is exact (the adapter header widens
  // K with it).  Any other conversion is OpenCV's
  void convertTo(Mat &dst, int rtype, double alpha = 1, double beta = 0) const
  {
    const int ddepth = CV_MAT_DEPTH(rtype), cn = channels();
    if (beta == 0 && !empty() && ((ddepth == depth() && alpha == 1) || (depth() == CV_64F && ddepth == CV_32F && alpha == 1) ||
                                  (depth() == CV_32F && ddepth == CV_64F && alpha == 1) || (depth() == CV_16U && ddepth == CV_32F))) {
      Mat src(*this);                                      // dst may be *this
      dst.create(src.rows, src.cols, CV_MAKETYPE(ddepth, cn));
      const float a = (float)alpha;
      for (int r = 0; r < src.rows; ++r)
        for (int c = 0; c < src.cols * cn; ++c) {
          if (ddepth == src.depth()) std::memmove(dst.ptr(r) + src.elemSize1() * c, src.ptr(r) + src.elemSize1() * c, src.elemSize1());
          else if (src.depth() == CV_64F) dst.ptr<float>(r)[c] = (float)src.ptr<double>(r)[c];
          else if (src.depth() == CV_32F) dst.ptr<double>(r)[c] = (double)src.ptr<float>(r)[c];
          else dst.ptr<float>(r)[c] = (float)src.ptr<ushort>(r)[c] * a;
        }
      return;
    }
    if (depth() == CV_32F && channels() == 1 && CV_MAT_DEPTH(rtype) == CV_8U && beta == 0) {
      Mat out(rows, cols, CV_8UC1);  // not dst.create(): dst may be *this
      for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) {
          const double v = std::nearbyint((double)ptr<float>(r)[c] * alpha);  // default rounding mode: half to even
          out.ptr(r)[c] = (uchar)(v < 0 ? 0 : (v > 255 ? 255 : v));
        }
      dst.assignFrom(out);
      return;
    }
    if (!(depth() == CV_8U && channels() == 1 && CV_MAT_DEPTH(rtype) == CV_16U && alpha == 1 && beta == 0))
      FEALESS_REF_UNPINNED("Mat::convertTo (other than CV_8U -> CV_16U and CV_32F -> CV_8U)");
    dst.create(rows, cols, CV_16UC1);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) dst.ptr<ushort>(r)[c] = ptr(r)[c];
  }
  // header copy that keeps the static type of a Mat_<T> target
  void assignFrom(const Mat &m) { rows = m.rows; cols = m.cols; data = m.data; step = m.step; type_ = m.type_; buf_ = m.buf_; }
  // the transpose of a one-channel CV_32F matrix (a copy: nothing to round)
  Mat t() const
  {
    if (type_ != CV_32FC1) FEALESS_REF_UNPINNED("Mat::t (other than CV_32FC1)");
    Mat o(cols, rows, type_);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c) o.ptr<float>(c)[r] = ptr<float>(r)[c];
    return o;
  }
  Mat mul(const Mat &) const { FEALESS_REF_UNPINNED("Mat::mul"); }
  void resize(size_t) { FEALESS_REF_UNPINNED("Mat::resize"); }
  Mat reshape(int, int) const { FEALESS_REF_UNPINNED("Mat::reshape"); }
  inline void copyTo(const class _OutputArray &dst) const;

 protected:
  int type_;
  std::shared_ptr<void> buf_;
};

inline Size MSize::operator()() const { return Size(m->cols, m->rows); }
inline bool MSize::operator==(const MSize &o) const { return m->rows == o.m->rows && m->cols == o.m->cols; }

// Iterators over a Mat or a ROI of one: row by row, each row left to right, as cv::MatConstIterator_
template <typename T> class MatConstIterator_ {
 public:
  MatConstIterator_() : m_(NULL), r_(0), c_(0) {}
  MatConstIterator_(const Mat *m, bool at_end) : m_(m), r_(at_end || m->cols == 0 ? m->rows : 0), c_(0) {}
  const T &operator*() const { return m_->template ptr<T>(r_)[c_]; }
  MatConstIterator_ &operator++()
  {
    if (++c_ >= m_->cols) { c_ = 0; ++r_; }
    return *this;
  }
  bool operator==(const MatConstIterator_ &o) const { return r_ == o.r_ && c_ == o.c_; }
  bool operator!=(const MatConstIterator_ &o) const { return !(*this == o); }

 protected:
  const Mat *m_;
  int r_, c_;
};
template <typename T> class MatIterator_ : public MatConstIterator_<T> {
 public:
  MatIterator_() {}
  MatIterator_(Mat *m, bool at_end) : MatConstIterator_<T>(m, at_end) {}
  T &operator*() const { return const_cast<T &>(MatConstIterator_<T>::operator*()); }
  MatIterator_ &operator++()
  {
    MatConstIterator_<T>::operator++();
    return *this;
  }
};
template <typename T> inline MatIterator_<T> Mat::begin() { return MatIterator_<T>(this, false); }
template <typename T> inline MatIterator_<T> Mat::end() { return MatIterator_<T>(this, true); }
template <typename T> inline MatConstIterator_<T> Mat::begin() const { return MatConstIterator_<T>(this, false); }
template <typename T> inline MatConstIterator_<T> Mat::end() const { return MatConstIterator_<T>(this, true); }

// A Mat whose element type is fixed: an empty one already has it, and a Mat of another depth is converted on the way in
template <typename T> class Mat_ : public Mat {
 public:
  typedef MatIterator_<T> iterator;
  typedef MatConstIterator_<T> const_iterator;
  Mat_() : Mat() { type_ = DataType<T>::type; }
  Mat_(int r, int c) : Mat(r, c, DataType<T>::type) {}
  Mat_(int r, int c, const T &v) : Mat(r, c, DataType<T>::type)
  {
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < c; ++j) (*this)(i, j) = v;
  }
  explicit Mat_(Size s) : Mat(s.height, s.width, DataType<T>::type) {}
  Mat_(const Mat &m) : Mat() { type_ = DataType<T>::type; *this = m; }
  Mat_(const Mat_ &m) : Mat(m) {}
  Mat_ &operator=(const Mat_ &m)
  {
    assignFrom(m);
    return *this;
  }
  Mat_ &operator=(const Mat &m)
  {
    if (m.type() == (int)DataType<T>::type) assignFrom(m);
    else if (m.empty()) { Mat e; assignFrom(e); type_ = DataType<T>::type; }
    else if (m.channels() == CV_MAT_CN((int)DataType<T>::type)) m.convertTo(*this, DataType<T>::type);
    else FEALESS_REF_UNPINNED("Mat_ = Mat with another channel count");
    return *this;
  }
  T &operator()(int r, int c) { return this->template ptr<T>(r)[c]; }
  const T &operator()(int r, int c) const { return this->template ptr<T>(r)[c]; }
  // one index: into a single row or a single column
  T &operator()(int i) { return rows == 1 ? (*this)(0, i) : (*this)(i / cols, i % cols); }
  const T &operator()(int i) const { return rows == 1 ? (*this)(0, i) : (*this)(i / cols, i % cols); }
  T *operator[](int r) { return this->template ptr<T>(r); }
  const T *operator[](int r) const { return this->template ptr<T>(r); }
  Mat_ operator()(const Rect &roi) const { return Mat_(Mat::operator()(roi)); }
  iterator begin() { return Mat::begin<T>(); }
  iterator end() { return Mat::end<T>(); }
  const_iterator begin() const { return Mat::begin<T>(); }
  const_iterator end() const { return Mat::end<T>(); }
};

// An argument that is a Mat (or nothing); as an output also a std::vector<Mat> to be filled, which is all that
// Detector::match asks of its optional output
class _InputArray {
 public:
  _InputArray() : in_(NULL) {}
  _InputArray(const Mat &m) : in_(&m) {}
  Mat getMat() const { return in_ ? *in_ : Mat(); }

 protected:
  const Mat *in_;
};
class _OutputArray : public _InputArray {
 public:
  _OutputArray() : vec_(NULL), out_(NULL) {}
  _OutputArray(std::vector<Mat> &v) : vec_(&v), out_(NULL) {}
  _OutputArray(Mat &m) : _InputArray(m), vec_(NULL), out_(&m) {}
  _OutputArray(const Mat &m) : _InputArray(m), vec_(NULL), out_(const_cast<Mat *>(&m)) {}
  bool needed() const { return vec_ != NULL || out_ != NULL; }
  void create(int r, int c, int type) const
  {
    if (vec_) vec_->resize((size_t)r * c);
    else if (out_) out_->create(r, c, type);
  }
  void create(Size s, int type) const { create(s.height, s.width, type); }
  Mat &getMatRef(int i) const { return (*vec_)[i]; }
  Mat *fealessMatTarget() const { return out_; }  // the Mat this output stands for, NULL for a vector or for nothing

 private:
  std::vector<Mat> *vec_;
  Mat *out_;
};
typedef const _InputArray &InputArray;
typedef const _OutputArray &OutputArray;
typedef const _OutputArray &OutputArrayOfArrays;
inline const _OutputArray &noArray()
{
  static const _OutputArray none;
  return none;
}
inline void Mat::copyTo(const _OutputArray &dst) const
{
  if (!dst.fealessMatTarget()) FEALESS_REF_UNPINNED("Mat::copyTo(OutputArray) (other than a Mat target)");
  copyTo(*dst.fealessMatTarget());
}

// ---- defined for the ICP sources -----------------------------------------------------------------------------------
// Mat * Mat on one-channel CV_32F: cv::gemm keeps double accumulators for float matrices, k ascending
inline Mat operator*(const Mat &a, const Mat &b)
{
  if (a.type() != CV_32FC1 || b.type() != CV_32FC1 || a.cols != b.rows) FEALESS_REF_UNPINNED("Mat * Mat (other than CV_32FC1)");
  Mat o(a.rows, b.cols, CV_32FC1);
  for (int i = 0; i < a.rows; ++i)
    for (int j = 0; j < b.cols; ++j) {
      double s = 0;
      for (int k = 0; k < a.cols; ++k) s += (double)a.ptr<float>(i)[k] * (double)b.ptr<float>(k)[j];
      o.ptr<float>(i)[j] = (float)s;
    }
  return o;
}
// Mat == value on CV_16UC1: 255 where equal, 0 elsewhere
inline Mat operator==(const Mat &a, double v)
{
  if (a.type() != CV_16UC1) FEALESS_REF_UNPINNED("Mat == scalar (other than CV_16UC1)");
  Mat o(a.rows, a.cols, CV_8UC1);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) o.ptr(r)[c] = (double)a.ptr<ushort>(r)[c] == v ? 255 : 0;
  return o;
}
// cv::norm(a, b), NORM_L2, of two CV_32F matrices of one shape: the differences taken in double, their squares
// accumulated in double in element order (the oracle's statement of it; OpenCV's own order of the subtraction and the
// widening is not pinned, and the tests keep to coordinates on which the two agree)
inline double norm(const Mat &a, const Mat &b)
{
  if (a.depth() != CV_32F || a.type() != b.type() || a.rows != b.rows || a.cols != b.cols) FEALESS_REF_UNPINNED("norm(Mat, Mat) (other than CV_32F)");
  double s = 0;
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols * a.channels(); ++c) {
      const double d = (double)a.ptr<float>(r)[c] - (double)b.ptr<float>(r)[c];
      s += d * d;
    }
  return std::sqrt(s);
}
inline int64 getTickCount()
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (int64)ts.tv_sec * 1000000000 + ts.tv_nsec;
}
inline double getTickFrequency() { return 1e9; }
// defined by oracle/ref/icp_harness.cpp on the oracle's orc_svd3 (OpenCV's JacobiSVD restated there: unpinned)
struct SVD {
  static void compute(const Matx33f &src, Mat &w, Mat &u, Mat &vt);
};

// ---- declared only: the Mat expression arithmetic of depthTo3d_from_uvz and what else the dead paths name -----------------
inline Mat operator+(const Mat &, const Mat &) { FEALESS_REF_UNPINNED("Mat + Mat"); }
inline Mat operator+(const Mat &, double) { FEALESS_REF_UNPINNED("Mat + scalar"); }
inline Mat operator-(const Mat &, double) { FEALESS_REF_UNPINNED("Mat - scalar"); }
inline Mat operator*(const Mat &, double) { FEALESS_REF_UNPINNED("Mat * scalar"); }
inline Mat operator*(double, const Mat &) { FEALESS_REF_UNPINNED("scalar * Mat"); }
inline Mat operator/(const Mat &, double) { FEALESS_REF_UNPINNED("Mat / scalar"); }
inline Mat operator|(const Mat &, const Mat &) { FEALESS_REF_UNPINNED("Mat | Mat"); }
inline void merge(const std::vector<Mat> &, Mat &) { FEALESS_REF_UNPINNED("merge"); }
inline void split(const Mat &, std::vector<Mat> &) { FEALESS_REF_UNPINNED("split"); }

// ---- declared only: persistence ---------------------------------------------------------------------------------
class FileNode;
class FileNodeIterator {
 public:
  FileNode operator*() const;
  FileNodeIterator &operator++() { FEALESS_REF_UNPINNED("FileNodeIterator"); }
  bool operator!=(const FileNodeIterator &) const { FEALESS_REF_UNPINNED("FileNodeIterator"); }
  template <typename T> FileNodeIterator &operator>>(T &) { FEALESS_REF_UNPINNED("FileNodeIterator"); }
};
class FileNode {
 public:
  FileNode operator[](const char *) const { FEALESS_REF_UNPINNED("FileNode"); }
  FileNodeIterator begin() const { FEALESS_REF_UNPINNED("FileNode"); }
  FileNodeIterator end() const { FEALESS_REF_UNPINNED("FileNode"); }
  size_t size() const { FEALESS_REF_UNPINNED("FileNode"); }
  operator int() const { FEALESS_REF_UNPINNED("FileNode"); }
  operator float() const { FEALESS_REF_UNPINNED("FileNode"); }
  operator String() const { FEALESS_REF_UNPINNED("FileNode"); }
};
inline FileNode FileNodeIterator::operator*() const { FEALESS_REF_UNPINNED("FileNodeIterator"); }
template <typename T> inline void operator>>(const FileNode &, std::vector<T> &) { FEALESS_REF_UNPINNED("FileNode"); }
class FileStorage {
 public:
  enum Mode { READ = 0, WRITE = 1 };
  FileStorage(const String &, int) { FEALESS_REF_UNPINNED("FileStorage"); }
  FileNode operator[](const char *) const { FEALESS_REF_UNPINNED("FileStorage"); }
  FileNode root() const { FEALESS_REF_UNPINNED("FileStorage"); }
};
template <typename T> inline FileStorage &operator<<(FileStorage &, const T &) { FEALESS_REF_UNPINNED("FileStorage"); }
inline String format(const char *, ...) { FEALESS_REF_UNPINNED("format"); }

// ---- array arithmetic of template extraction: CV_8UC1 only, each with one possible answer ---------------------------
inline bool fealess_same_8u(const Mat &a, const Mat &b)
{
  return !a.empty() && a.type() == CV_8UC1 && b.type() == CV_8UC1 && a.rows == b.rows && a.cols == b.cols;
}
// saturating a - b; dst may be a or b (ColorGradientPyramid::extractTemplate, linemod.cpp:468)
inline void subtract(const Mat &a, const Mat &b, Mat &dst)
{
  if (!fealess_same_8u(a, b)) FEALESS_REF_UNPINNED("subtract (other than CV_8UC1 of one size)");
  Mat out(a.rows, a.cols, CV_8UC1);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) {
      const int v = (int)a.ptr(r)[c] - (int)b.ptr(r)[c];
      out.ptr(r)[c] = (uchar)(v < 0 ? 0 : v);
    }
  dst = out;
}
// a & b; dst may be a or b (DepthNormalPyramid::extractTemplate, linemod.cpp:762)
inline void bitwise_and(const Mat &a, const Mat &b, Mat &dst)
{
  if (!fealess_same_8u(a, b)) FEALESS_REF_UNPINNED("bitwise_and (other than CV_8UC1 of one size)");
  Mat out(a.rows, a.cols, CV_8UC1);
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) out.ptr(r)[c] = (uchar)(a.ptr(r)[c] & b.ptr(r)[c]);
  dst = out;
}
inline int countNonZero(const Mat &a)
{
  if (a.type() != CV_8UC1) FEALESS_REF_UNPINNED("countNonZero (other than CV_8UC1)");
  int n = 0;
  for (int r = 0; r < a.rows; ++r)
    for (int c = 0; c < a.cols; ++c) n += a.ptr(r)[c] != 0;
  return n;
}
inline void add(const Mat &, const Mat &, Mat &, const _OutputArray &, int) { FEALESS_REF_UNPINNED("add"); }

// ---- delegated to the oracle (../liboracle.so): OpenCV's arithmetic, restated there and NOT pinned --------------------
// cv::phase(x, y, angle, true) on CV_32FC1 -> orc_fast_atan2(y, x) per element (quantizedOrientations, linemod.cpp:303)
inline void phase(const Mat &x, const Mat &y, Mat &angle, bool degrees)
{
  if (!degrees || x.empty() || x.type() != CV_32FC1 || y.type() != CV_32FC1 || x.rows != y.rows || x.cols != y.cols)
    FEALESS_REF_UNPINNED("phase (other than CV_32FC1 in degrees)");
  Mat out(x.rows, x.cols, CV_32FC1);
  for (int r = 0; r < x.rows; ++r)
    for (int c = 0; c < x.cols; ++c) out.ptr<float>(r)[c] = orc_fast_atan2(y.ptr<float>(r)[c], x.ptr<float>(r)[c]);
  angle = out;
}

}  // namespace cv
#endif
