// Stand-in of <opencv2/flann/flann.hpp> for the reference's ICP/ICP.cpp, written from scratch: cvflann::Matrix, and an
// Index<L2_Simple<float>> whose knnSearch is an EXACT 1-nearest-neighbour search by exhaustion.  FLANN's
// KDTreeSingleIndex is exact too (its SearchParams have no effect on a single tree with eps = 0), so the neighbour is
// the same wherever it is unique; WHICH of several points at exactly the same float distance FLANN would return
// depends on its tree and is unspecified.  Here a tie goes to the lowest index.  The distance is L2_Simple's own
// statement: result = 0; diff = a[i] - b[i]; result += diff * diff, for i = 0, 1, 2 in float.  A query no distance to
// which compares below the running best (a NaN coordinate) gets index -1 and distance NaN; FLANN's result set keeps
// a NaN distance as well, and the caller's `dist <= thr` then drops the pair either way.
#ifndef FEALESS_REF_OPENCV_FLANN_FLANN_HPP
#define FEALESS_REF_OPENCV_FLANN_FLANN_HPP
#include "opencv2/core.hpp"

namespace cvflann {

template <typename T> struct Matrix {
  size_t rows, cols;
  T *data;
  Matrix() : rows(0), cols(0), data(NULL) {}
  Matrix(T *data_, size_t rows_, size_t cols_) : rows(rows_), cols(cols_), data(data_) {}
  T *operator[](size_t i) const { return data + i * cols; }
};

template <typename T> struct L2_Simple {
  typedef T ElementType;
  typedef float ResultType;
  ResultType operator()(const T *a, const T *b, size_t size) const
  {
    ResultType result = ResultType();
    for (size_t i = 0; i < size; ++i) {
      const ResultType diff = *a++ - *b++;
      result += diff * diff;
    }
    return result;
  }
};

struct IndexParams {};
struct KDTreeSingleIndexParams : IndexParams {
  explicit KDTreeSingleIndexParams(int = 10, bool = true, int = -1) {}
};
struct SearchParams {
  explicit SearchParams(int = 32, float = 0, bool = true) {}
};

template <typename Distance> class Index {
 public:
  typedef typename Distance::ElementType ElementType;
  typedef typename Distance::ResultType DistanceType;
  Index(const Matrix<ElementType> &features, const IndexParams &, Distance d = Distance()) : data_(features), dist_(d) {}
  void buildIndex() {}
  void knnSearch(const Matrix<ElementType> &queries, Matrix<int> &indices, Matrix<DistanceType> &dists, int knn, const SearchParams &)
  {
    if (knn != 1) FEALESS_REF_UNPINNED("cvflann::Index::knnSearch (knn other than 1)");
    ++cv::fealess_ref_counters().knn_searches;
    for (size_t q = 0; q < queries.rows; ++q) {
      int best = -1;
      DistanceType bd = std::numeric_limits<DistanceType>::infinity();
      for (size_t j = 0; j < data_.rows; ++j) {
        const DistanceType d = dist_(queries[q], data_[j], data_.cols);
        if (d < bd) { bd = d; best = (int)j; }
      }
      indices[q][0] = best;
      dists[q][0] = best >= 0 ? bd : std::numeric_limits<DistanceType>::quiet_NaN();
    }
  }

 private:
  Matrix<ElementType> data_;
  Distance dist_;
};

}  // namespace cvflann
#endif
