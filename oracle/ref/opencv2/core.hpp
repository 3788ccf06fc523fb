// Container-only stand-in of <opencv2/core.hpp>, written from scratch for ONE purpose: to compile the reference's
// linemod/linemod.cpp unchanged (oracle/ref/ref_harness.cpp includes it by include path at build time) on a machine
// without OpenCV, so that the oracle and the HIP kernels can be compared with the reference's own compiled arithmetic.
// TEST INFRASTRUCTURE ONLY; nothing here is part of the product, and nothing here is copied from OpenCV or the reference.
//
// What is real here, and what is not:
//
//  * CONTAINERS have real definitions: Mat (reference counted; rows/cols/data/step, type(), ptr<T>(r), at<T>(r,c),
//    step1(), create, zeros, clone, copyTo, setTo, size(), total(), empty(), ROI operator()(Rect)), Mat_<T>, Size, Point,
//    Rect, Vec3b, Ptr/makePtr, String, CV_Assert/CV_Error (throw cv::Exception), alignSize, checkHardwareSupport,
//    OutputArrayOfArrays/noArray() with needed/create/getMatRef.  The arithmetic linemod.cpp does on them is its own C++.
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
//    They are OURS, not OpenCV's code, and are named here so that nobody takes them for more than that.
//
//  * EVERYTHING ELSE linemod.cpp names is DECLARED ONLY and given a body that aborts with its name (FEALESS_REF_UNPINNED):
//    GaussianBlur, Sobel, phase, pyrDown, resize, erode, subtract, bitwise_and, add, distanceTransform, countNonZero,
//    every other Mat::convertTo, FileStorage/FileNode I/O and format.  OpenCV's choice of kernels, work types and
//    roundings for those stays UNPINNED; this stand-in does not re-implement OpenCV arithmetic a second time and call it
//    a reference.
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

#define CV_CPU_SSE2 3
#define CV_CPU_SSE3 4
#define CV_CPU_SSSE3 5

#define CV_DECL_ALIGNED(x) __attribute__((aligned(x)))

#define FEALESS_REF_UNPINNED(name)                                                                          \
  do {                                                                                                      \
    std::fprintf(stderr, "oracle/ref stand-in: %s is declared only (OpenCV arithmetic stays unpinned)\n", name); \
    std::abort();                                                                                           \
  } while (0)

namespace cv {

typedef std::string String;

class Exception : public std::runtime_error {
 public:
  explicit Exception(const std::string &what_) : std::runtime_error(what_) {}
};
namespace Error { enum Code { StsBadArg = -5, StsAssert = -215 }; }
[[noreturn]] inline void error(int code, const String &msg, const char *file, int line)
{
  throw Exception(String(file) + ":" + std::to_string(line) + ": error " + std::to_string(code) + ": " + msg);
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
struct Rect {
  int x, y, width, height;
  Rect() : x(0), y(0), width(0), height(0) {}
  Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};
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

enum BorderTypes { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4 };

class Mat {
 public:
  int rows, cols;
  uchar *data;
  size_t step;  // bytes per row

  Mat() : rows(0), cols(0), data(NULL), step(0), type_(0) {}
  Mat(int r, int c, int type) : rows(0), cols(0), data(NULL), step(0), type_(0) { create(r, c, type); }
  Mat(Size s, int type) : rows(0), cols(0), data(NULL), step(0), type_(0) { create(s.height, s.width, type); }

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
  Size size() const { return Size(cols, rows); }
  size_t total() const { return (size_t)rows * cols; }
  bool empty() const { return data == NULL || rows == 0 || cols == 0; }

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

  Mat operator()(const Rect &roi) const
  {
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
    CV_Assert(type_ == CV_8UC1);
    for (int r = 0; r < rows; ++r)
      for (int c = 0; c < cols; ++c)
        if (mask.empty() || mask.ptr(r)[c]) ptr(r)[c] = (uchar)v.val[0];
    return *this;
  }
  // defined for CV_8U -> CV_16U (alpha 1) and CV_32F -> CV_8U (any alpha), beta 0, one channel (see the header comment);
  // any other conversion is OpenCV's
  void convertTo(Mat &dst, int rtype, double alpha = 1, double beta = 0) const
  {
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

 protected:
  int type_;
  std::shared_ptr<void> buf_;
};

template <typename T> class Mat_ : public Mat {
 public:
  Mat_() : Mat() {}
  T &operator()(int r, int c) { return this->template ptr<T>(r)[c]; }
  const T &operator()(int r, int c) const { return this->template ptr<T>(r)[c]; }
};

// noArray() or a std::vector<Mat> to be filled: all that Detector::match asks of its optional output
class _OutputArray {
 public:
  _OutputArray() : vec_(NULL) {}
  _OutputArray(std::vector<Mat> &v) : vec_(&v) {}
  bool needed() const { return vec_ != NULL; }
  void create(int r, int c, int /*type*/) const { if (vec_) vec_->resize((size_t)r * c); }
  Mat &getMatRef(int i) const { return (*vec_)[i]; }

 private:
  std::vector<Mat> *vec_;
};
typedef const _OutputArray &OutputArray;
typedef const _OutputArray &OutputArrayOfArrays;
typedef const _OutputArray &InputArray;
inline const _OutputArray &noArray()
{
  static const _OutputArray none;
  return none;
}

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
  FileNode root() const { FEALESS_REF_UNPINNED("FileStorage"); }
};
template <typename T> inline FileStorage &operator<<(FileStorage &, const T &) { FEALESS_REF_UNPINNED("FileStorage"); }
inline String format(const char *, ...) { FEALESS_REF_UNPINNED("format"); }

// ---- declared only: array arithmetic ----------------------------------------------------------------------------
inline void subtract(const Mat &, const Mat &, Mat &) { FEALESS_REF_UNPINNED("subtract"); }
inline void bitwise_and(const Mat &, const Mat &, Mat &) { FEALESS_REF_UNPINNED("bitwise_and"); }
inline void add(const Mat &, const Mat &, Mat &, const _OutputArray &, int) { FEALESS_REF_UNPINNED("add"); }
inline int countNonZero(const Mat &) { FEALESS_REF_UNPINNED("countNonZero"); }
inline void phase(const Mat &, const Mat &, Mat &, bool) { FEALESS_REF_UNPINNED("phase"); }

}  // namespace cv
#endif
