// ref_harness.cpp -- TEST INFRASTRUCTURE: the reference's own linemod/linemod.cpp, compiled against the container-only
// opencv2/ stand-in beside this file, behind a small extern "C" surface over plain pointers that mirrors the oracle's
// stage entry points (oracle/fealess_oracle.h) one to one.  The reference's translation unit is INCLUDED below by
// include path at build time (-I$(FEALESS_REFERENCE_ROOT)/linemod), so that its file-static functions are visible; no
// line of it is in this repository, and the libraries built from this file (oracle/_ref/) are never committed.
//
// TEMPLATE EXTRACTION runs here too: quantizedOrientations, std::stable_sort + selectScatteredFeatures, the two
// extractTemplate methods on caller-supplied images, Detector::addTemplate.
// WHAT IS PINNED by it: the reference's text, compiled -- `score > threshold_sq` (strong^2 itself is no candidate),
// `score >= extract_threshold`, labels 0 and 255 left out, mask - erode(mask) as the colour mask, candidates.size() /
// num_features + 1 in size_t, sqrtf(area) / sqrtf(num_features) + 1.5f with area = total() or countNonZero of the eroded
// mask, the relaxation loop of selectScatteredFeatures (distance -= 1.0f through fractions and below zero) and its `>=`
// keep rule on an int compared with a float, std::stable_sort on Candidate::operator<, score /= label_counts[label],
// num_features /= 2 and extract_threshold /= 2 per level, the else-if chain that picks a colour channel on equal
// magnitudes (mag1 >= mag2 && mag1 >= mag3, then mag2), `min_x % 2 == 1` in cropTemplates, the order in which
// addTemplate walks modalities and levels and gives up.
// WHAT STAYS UNPINNED: OpenCV arithmetic the reference only CALLS, which the stand-in delegates to the oracle's
// restatement in ../liboracle.so (this library links it, so both sides run the same code), item by item:
//   * cv::GaussianBlur 7x7, sigma 0, BORDER_REPLICATE, 8UC3   -> orc_gaussian7_bgr;
//   * cv::Sobel CV_16S, ksize 3, BORDER_REPLICATE, 8UC3        -> orc_sobel3_bgr;
//   * cv::phase in degrees                                      -> orc_fast_atan2 per element;
//   * cv::pyrDown 8UC3 to exact halves                          -> orc_pyrdown_bgr;
//   * cv::resize INTER_NEAREST 8UC1 to exact halves             -> orc_resize_nn_half;
//   * cv::erode, default 3x3, 1 or 2 iterations, replicated     -> orc_erode_rect;
//   * cv::distanceTransform(DIST_C, 3)                          -> orc_distance_transform_c3.
// Plain code of the stand-in, each with one possible answer: subtract (saturating u8), bitwise_and, countNonZero,
// Mat::setTo(value, mask), and the two conversions and the median that opencv2/core.hpp describes.
//
// Every entry point returns 0, or -1 when the reference threw (CV_Assert / CV_Error); the extraction entries return the
// oracle's 1 (features written) / 0 (too few candidates) and -1 for a throw; ref_add_template returns addTemplate's -1.
// Inputs are copied into Mats of the stand-in, whose allocator appends a zeroed guard (opencv2/core.hpp): reads past the
// last grid row of a linear memory (quirk Q2) are undefined behaviour in the reference and read 0 here.
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

void out_features(const std::vector<Feature> &fs, orc_feature *out)
{
  for (size_t i = 0; i < fs.size(); ++i) {
    out[i].x = fs[i].x;
    out[i].y = fs[i].y;
    out[i].label = fs[i].label;
  }
}

// Candidate and selectScatteredFeatures are protected in QuantizedPyramid: reached from a derived class.  The sort is
// the one both extractTemplate methods run (std::stable_sort on Candidate::operator<, linemod.cpp:501, :812).
class OpenSelection : public GivenPyramid {
 public:
  static void run(const int *x, const int *y, const int *label, const float *score, int n, int num_features, float distance,
                  std::vector<Feature> &features)
  {
    std::vector<Candidate> candidates;
    for (int i = 0; i < n; ++i) candidates.push_back(Candidate(x[i], y[i], label[i], score[i]));
    std::stable_sort(candidates.begin(), candidates.end());
    selectScatteredFeatures(candidates, features, (size_t)num_features, distance);
  }
};

// The two pyramids with their protected members replaced by the caller's images: constructed on a small blank source
// (the constructors quantize it), then assigned.
class OpenColorPyramid : public ColorGradientPyramid {
 public:
  OpenColorPyramid(const Mat &quantized, const Mat &magnitude_, const Mat &mask_, float strong, int nf)
      : ColorGradientPyramid(Mat::zeros(8, 8, CV_8UC3), Mat(), 10.0f, (size_t)nf, strong)
  {
    angle = quantized;
    magnitude = magnitude_;
    mask = mask_;
    num_features = (size_t)nf;
    strong_threshold = strong;
    pyramid_level = 0;
  }
};

class OpenDepthPyramid : public DepthNormalPyramid {
 public:
  OpenDepthPyramid(const Mat &normal_, const Mat &mask_, int extract, int nf)
      : DepthNormalPyramid(Mat::zeros(16, 16, CV_16UC1), Mat(), 2000, 50, (size_t)nf, extract)
  {
    normal = normal_;
    mask = mask_;
    num_features = (size_t)nf;
    extract_threshold = extract;
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

// quantizedOrientations (the file-static, linemod.cpp:230-305): the quantized image and the squared magnitude
int ref_quantized_orientations(const uint8_t *bgr, int w, int h, float weak_threshold, uint8_t *dst, float *magnitude)
{
  try {
    Mat src(h, w, CV_8UC3), mag, q;
    for (int r = 0; r < h; ++r) std::memcpy(src.ptr(r), bgr + (size_t)r * w * 3, (size_t)w * 3);
    quantizedOrientations(src, mag, q, weak_threshold);
    out_u8(q, dst);
    if (magnitude)
      for (int r = 0; r < h; ++r) std::memcpy(magnitude + (size_t)r * w, mag.ptr<float>(r), sizeof(float) * w);
    return 0;
  } catch (const cv::Exception &) { return -1; }
}

// std::stable_sort on Candidate::operator<, then selectScatteredFeatures (linemod.cpp:135-164), on a candidate list in
// arrival order.  1, or 0 when n < num_features or num_features < 1: the reference's callers guard that (:498, :802);
// unguarded it would index past the list, so the refusal is made here, before the reference is entered.  -1: it threw
int ref_select_scattered_list(const int *x, const int *y, const int *label, const float *score, int n, int num_features,
                              float distance, orc_feature *out)
{
  if (num_features < 1 || n < num_features) return 0;
  try {
    std::vector<Feature> fs;
    OpenSelection::run(x, y, label, score, n, num_features, distance, fs);
    out_features(fs, out);
    return 1;
  } catch (const cv::Exception &) { return -1; }
}

// ColorGradientPyramid::extractTemplate (linemod.cpp:461-513) on the caller's quantized image, squared magnitude and
// mask (NULL: empty).  1 / 0 (too few candidates) / -1 (threw: getLabel on a byte that is not one-hot)
int ref_extract_template_color(const uint8_t *quantized, const float *magnitude, const uint8_t *mask, int w, int h,
                               float strong_threshold, int num_features, orc_feature *out)
{
  if (num_features < 1) return 0;
  try {
    Mat mag(h, w, CV_32F);
    for (int r = 0; r < h; ++r) std::memcpy(mag.ptr(r), magnitude + (size_t)r * w, sizeof(float) * w);
    OpenColorPyramid p(mat_u8(quantized, w, h), mag, mask ? mat_u8(mask, w, h) : Mat(), strong_threshold, num_features);
    Template t;
    if (!p.extractTemplate(t)) return 0;
    out_features(t.features, out);
    return 1;
  } catch (const cv::Exception &) { return -1; }
}

// DepthNormalPyramid::extractTemplate (linemod.cpp:747-825) on the caller's quantized normals and mask (NULL: empty)
int ref_extract_template_depth(const uint8_t *normal, const uint8_t *mask, int w, int h, int extract_threshold, int num_features,
                               orc_feature *out)
{
  if (num_features < 1) return 0;
  try {
    OpenDepthPyramid p(mat_u8(normal, w, h), mask ? mat_u8(mask, w, h) : Mat(), extract_threshold, num_features);
    Template t;
    if (!p.extractTemplate(t)) return 0;
    out_features(t.features, out);
    return 1;
  } catch (const cv::Exception &) { return -1; }
}

// Detector::addTemplate (linemod.cpp:1579-1615) with the two default modalities, ColorGradient() and DepthNormal()
// (:515-519, :827-832); mask NULL: empty.  templates[levels * 2] ordered [l * 2 + m] and the bounding box are read back
// with getTemplates; the feature slot of template k is feats + 63 * k.  0, or -1 where addTemplate returned -1 (too few
// candidates at some level: a result, recorded) or the reference threw
int ref_add_template(const uint8_t *bgr, const uint16_t *depth, const uint8_t *mask, int w0, int h0, int levels,
                     orc_template *templates, orc_feature *feats, int bb[4])
{
  if (levels < 1 || levels > 3) return -1;
  try {
    std::vector<Mat> sources(2);
    sources[0].create(h0, w0, CV_8UC3);
    sources[1].create(h0, w0, CV_16UC1);
    for (int r = 0; r < h0; ++r) {
      std::memcpy(sources[0].ptr(r), bgr + (size_t)r * w0 * 3, (size_t)w0 * 3);
      std::memcpy(sources[1].ptr(r), depth + (size_t)r * w0, sizeof(uint16_t) * w0);
    }
    std::vector<Ptr<Modality> > mods;
    mods.push_back(makePtr<ColorGradient>());
    mods.push_back(makePtr<DepthNormal>());
    Detector det(mods, std::vector<int>(levels, 4));       // T plays no part in training
    const float pose[13] = {0};
    Rect box;
    const int id = det.addTemplate(sources, "obj", mask ? mat_u8(mask, w0, h0) : Mat(), pose, &box);
    if (id < 0) return -1;
    const std::vector<Template> &tp = det.getTemplates("obj", id);
    for (size_t k = 0; k < tp.size(); ++k) {
      orc_template &t = templates[k];
      t.width = tp[k].width;
      t.height = tp[k].height;
      t.offset_x = tp[k].offset_x;
      t.offset_y = tp[k].offset_y;
      t.pyramid_level = tp[k].pyramid_level;
      t.feat_begin = (int)k * 63;
      t.feat_count = (int)tp[k].features.size();
      out_features(tp[k].features, feats + t.feat_begin);
    }
    bb[0] = box.x; bb[1] = box.y; bb[2] = box.width; bb[3] = box.height;
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
