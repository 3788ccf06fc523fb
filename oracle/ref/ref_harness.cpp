// ref_harness.cpp -- TEST INFRASTRUCTURE: the reference's own linemod/linemod.cpp, compiled against the container-only
// opencv2/ stand-in beside this file, behind a small extern "C" surface over plain pointers that mirrors the oracle's
// stage entry points (oracle/fealess_oracle.h) one to one.  The reference's translation unit is INCLUDED below by
// include path at build time (-I$(FEALESS_REFERENCE_ROOT)/linemod), so that its file-static functions are visible; no
// line of it is in this repository, and the libraries built from this file (oracle/_ref/) are never committed.
//
// Every entry point returns 0, or -1 when the reference threw (CV_Assert / CV_Error).  Inputs are copied into Mats of
// the stand-in, whose allocator appends a zeroed guard (opencv2/core.hpp): reads past the last grid row of a linear
// memory (quirk Q2) are undefined behaviour in the reference and read 0 here.
#include "linemod.cpp"  // the reference's, found by include path

#include <map>
#include <stdint.h>

#include "../fealess_oracle.h"

using namespace cup_linemod;

namespace {

Mat mat_u8(const uint8_t *p, int w, int h)
{
  Mat m(h, w, CV_8U);
  for (int r = 0; r < h; ++r) std::memcpy(m.ptr(r), p + (size_t)r * w, (size_t)w);
  return m;
}

void out_u8(const Mat &m, uint8_t *dst)
{
  for (int r = 0; r < m.rows; ++r) std::memcpy(dst + (size_t)r * m.cols, m.ptr(r), (size_t)m.cols);
}

// the 8 linear memories of one (level, modality) from the project's padded layout [label][T*T][W*H] + pad per label
std::vector<Mat> linear_memories(const uint8_t *lm8, size_t label_stride, int w, int h, int T)
{
  const int WH = (w / T) * (h / T);
  std::vector<Mat> lms(8);
  for (int l = 0; l < 8; ++l) {
    lms[l].create(T * T, WH, CV_8U);
    std::memcpy(lms[l].data, lm8 + (size_t)l * label_stride, (size_t)T * T * WH);
  }
  return lms;
}

Template make_template(const orc_template *t, const orc_feature *feats)
{
  Template out;
  out.width = t->width;
  out.height = t->height;
  out.offset_x = t->offset_x;
  out.offset_y = t->offset_y;
  out.pyramid_level = t->pyramid_level;
  for (int i = 0; i < t->feat_count; ++i) {
    const orc_feature &f = feats[t->feat_begin + i];
    out.features.push_back(Feature(f.x, f.y, f.label));
  }
  return out;
}

// A modality that hands the caller's quantized images to Detector::match: level l of modality m is images[l * M + m].
class GivenPyramid : public QuantizedPyramid {
 public:
  GivenPyramid(const std::vector<Mat> *images, int modality, int modalities) : images_(images), m_(modality), M_(modalities), level_(0) {}
  virtual void quantize(Mat &dst) const { (*images_)[(size_t)level_ * M_ + m_].copyTo(dst); }
  virtual bool extractTemplate(Template &) const { return false; }
  virtual void pyrDown() { ++level_; }

 private:
  const std::vector<Mat> *images_;
  int m_, M_, level_;
};

class GivenModality : public Modality {
 public:
  GivenModality(const std::vector<Mat> *images, int modality, int modalities) : images_(images), m_(modality), M_(modalities) {}
  virtual String name() const { return "Given"; }
  virtual void read(const FileNode &) {}
  virtual void write(FileStorage &) const {}

 protected:
  virtual Ptr<QuantizedPyramid> processImpl(const Mat &, const Mat &) const { return makePtr<GivenPyramid>(images_, m_, M_); }

 private:
  const std::vector<Mat> *images_;
  int m_, M_;
};

// Detector with its protected matchClass reachable: the list BEFORE std::sort / std::unique, made with the reference's
// own statics in the order Detector::match calls them (linemod.cpp:1383-1434).
class OpenDetector : public Detector {
 public:
  OpenDetector(const std::vector<Ptr<Modality> > &mods, const std::vector<int> &T) : Detector(mods, T) {}
  void raw_matches(const std::vector<Mat> &images, float threshold, const std::vector<String> &class_ids, std::vector<Match> &matches) const
  {
    const int M = (int)modalities.size();
    LinearMemoryPyramid lm_pyramid(pyramid_levels, std::vector<LinearMemories>(M, LinearMemories(8)));
    std::vector<Size> sizes;
    for (int l = 0; l < pyramid_levels; ++l) {
      const int T = T_at_level[l];
      Mat spread_quantized;
      std::vector<Mat> response_maps;
      for (int i = 0; i < M; ++i) {
        spread(images[(size_t)l * M + i], spread_quantized, T);
        computeResponseMaps(spread_quantized, response_maps);
        for (int j = 0; j < 8; ++j) linearize(response_maps[j], lm_pyramid[l][i][j], T);
      }
      sizes.push_back(images[(size_t)l * M + M - 1].size());
    }
    matches.clear();
    if (class_ids.empty()) {
      for (TemplatesMap::const_iterator it = class_templates.begin(); it != class_templates.end(); ++it)
        matchClass(lm_pyramid, sizes, threshold, matches, it->first, it->second);
    } else {
      for (size_t i = 0; i < class_ids.size(); ++i) {
        TemplatesMap::const_iterator it = class_templates.find(class_ids[i]);
        if (it != class_templates.end()) matchClass(lm_pyramid, sizes, threshold, matches, it->first, it->second);
      }
    }
  }
};

int copy_matches(const std::vector<Match> &ms, const std::map<String, int> &index, orc_match *out, int cap)
{
  int n = 0;
  for (size_t i = 0; i < ms.size() && n < cap; ++i, ++n) {
    out[n].x = ms[i].x;
    out[n].y = ms[i].y;
    out[n].similarity = ms[i].similarity;
    out[n].class_idx = index.find(ms[i].class_id)->second;
    out[n].template_id = ms[i].template_id;
  }
  return n;
}

}  // namespace

extern "C" {

// 1 when this library was built with the reference's SSE2 / SSE3 / SSSE3 branches, 0 for its scalar branches
int ref_is_simd(void) { return CV_SSE2 && CV_SSE3 && CV_SSSE3; }

int ref_spread(const uint8_t *src, int w, int h, int T, uint8_t *dst)
{
  try {
    Mat s = mat_u8(src, w, h), d;
    spread(s, d, T);
    out_u8(d, dst);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

// maps8 = 8 * w * h bytes
int ref_response_maps(const uint8_t *spread_img, int w, int h, uint8_t *maps8)
{
  try {
    Mat s = mat_u8(spread_img, w, h);
    std::vector<Mat> maps;
    computeResponseMaps(s, maps);
    for (int i = 0; i < 8; ++i) out_u8(maps[i], maps8 + (size_t)i * w * h);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

// out = T * T rows of (w / T) * (h / T) bytes
int ref_linearize(const uint8_t *map, int w, int h, int T, uint8_t *out)
{
  try {
    Mat m = mat_u8(map, w, h), lin;
    linearize(m, lin, T);
    out_u8(lin, out);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

// lm8: the 8 labels of one (level, modality), label_stride bytes apart, each T*T rows of (w/T)*(h/T) bytes
int ref_similarity(const uint8_t *lm8, size_t label_stride, const orc_template *t, const orc_feature *feats, int w, int h, int T,
                   uint8_t *dst)
{
  try {
    std::vector<Mat> lms = linear_memories(lm8, label_stride, w, h, T);
    Mat d;
    similarity(lms, make_template(t, feats), d, Size(w, h), T);
    out_u8(d, dst);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

int ref_similarity_local(const uint8_t *lm8, size_t label_stride, const orc_template *t, const orc_feature *feats, int w, int h,
                         int T, int cx, int cy, uint8_t *dst)
{
  try {
    std::vector<Mat> lms = linear_memories(lm8, label_stride, w, h, T);
    Mat d;
    similarityLocal(lms, make_template(t, feats), d, Size(w, h), T, Point(cx, cy));
    out_u8(d, dst);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

// sims[m]: rows * cols u8; M is 1 or 2 (a third modality goes through cv::add, which stays unpinned)
int ref_add_similarities(const uint8_t *const *sims, int M, int rows, int cols, uint16_t *dst)
{
  if (M < 1 || M > 2) return -1;
  try {
    std::vector<Mat> s;
    for (int m = 0; m < M; ++m) s.push_back(mat_u8(sims[m], cols, rows));
    Mat d;
    addSimilarities(s, d);
    for (int r = 0; r < rows; ++r) std::memcpy(dst + (size_t)r * cols, d.ptr<ushort>(r), sizeof(uint16_t) * cols);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

// Detector::match on caller-supplied quantized images.  banks[c] / class_names[c]: the classes in the order they are
// to be inserted with addSyntheticTemplate; class_idx of the outputs is c.  filter (n_filter > 0): the class_ids
// argument of Detector::match.  out_final: Detector::match's own result; out_raw: the list before std::sort /
// std::unique.  *n_final / *n_raw get the full counts; at most cap_* entries are written.
int ref_match_quantized(const uint8_t *const *quantized, int w0, int h0, int levels, int modalities, const int *T_at_level,
                        const orc_bank *banks, const char *const *class_names, int n_classes, const char *const *filter,
                        int n_filter, float threshold, orc_match *out_final, int cap_final, int *n_final, orc_match *out_raw,
                        int cap_raw, int *n_raw)
{
  if (modalities < 1 || modalities > 2) return -1;
  try {
    std::vector<Mat> images;
    for (int l = 0; l < levels; ++l)
      for (int m = 0; m < modalities; ++m) images.push_back(mat_u8(quantized[l * modalities + m], w0 >> l, h0 >> l));
    std::vector<Ptr<Modality> > mods;
    for (int m = 0; m < modalities; ++m) mods.push_back(makePtr<GivenModality>(&images, m, modalities));
    OpenDetector det(mods, std::vector<int>(T_at_level, T_at_level + levels));
    std::map<String, int> index;
    for (int c = 0; c < n_classes; ++c) {
      index[class_names[c]] = c;
      const orc_bank &b = banks[c];
      const int LM = b.levels * b.modalities;
      for (int p = 0; p < b.n_pyramids; ++p) {
        std::vector<Template> tp;
        for (int k = 0; k < LM; ++k) tp.push_back(make_template(&b.templates[(size_t)p * LM + k], b.features));
        det.addSyntheticTemplate(tp, class_names[c]);
      }
    }
    std::vector<String> ids(filter, filter + n_filter);
    std::vector<Mat> sources(modalities);
    std::vector<Match> fin, raw;
    if (det.match(sources, threshold, fin, ids) != 0) return -1;
    det.raw_matches(images, threshold, ids, raw);
    *n_final = (int)fin.size();
    *n_raw = (int)raw.size();
    copy_matches(fin, index, out_final, cap_final);
    copy_matches(raw, index, out_raw, cap_raw);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

int ref_quantized_normals(const uint16_t *depth, int w, int h, int distance_threshold, int difference_threshold, uint8_t *dst)
{
  try {
    Mat src(h, w, CV_16U), d;
    for (int r = 0; r < h; ++r) std::memcpy(src.ptr(r), depth + (size_t)r * w, sizeof(uint16_t) * w);
    quantizedNormals(src, d, distance_threshold, difference_threshold);
    out_u8(d, dst);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

// hysteresisGradient(magnitude, quantized_angle, angle, threshold): threshold is compared with magnitude as given
int ref_hysteresis_gradient(const float *magnitude, const float *angle, int w, int h, float threshold, uint8_t *dst)
{
  try {
    Mat mag(h, w, CV_32F), ang(h, w, CV_32F), q;
    for (int r = 0; r < h; ++r) {
      std::memcpy(mag.ptr(r), magnitude + (size_t)r * w, sizeof(float) * w);
      std::memcpy(ang.ptr(r), angle + (size_t)r * w, sizeof(float) * w);
    }
    hysteresisGradient(mag, q, ang, threshold);
    out_u8(q, dst);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

// cropTemplates on n templates sharing one flat feature array, in place; bb = {x, y, width, height}
int ref_crop_templates(orc_template *t, int n, orc_feature *feats, int bb[4])
{
  try {
    std::vector<Template> tp;
    for (int i = 0; i < n; ++i) tp.push_back(make_template(&t[i], feats));
    Rect r = cropTemplates(tp);
    for (int i = 0; i < n; ++i) {
      t[i].width = tp[i].width;
      t[i].height = tp[i].height;
      t[i].offset_x = tp[i].offset_x;
      t[i].offset_y = tp[i].offset_y;
      for (int j = 0; j < t[i].feat_count; ++j) {
        feats[t[i].feat_begin + j].x = tp[i].features[j].x;
        feats[t[i].feat_begin + j].y = tp[i].features[j].y;
      }
    }
    bb[0] = r.x; bb[1] = r.y; bb[2] = r.width; bb[3] = r.height;
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

}  // extern "C"
