// A caller written against the reference's OpenCV-typed names only -- cup_linemod::{Detector, Match, Template, Feature}, the
// global drawResponse (x2), detection, icpCloudToCloud_Ex and cup_d2pc::depthTo3d -- compiled twice from this one source:
//   * with -DFL_REFERENCE_HEADERS against the reference's own headers (linemod_if.h, ICP.h, detection.h, depth_to_3d.h, found
//     by include path) and linked to its compiled code (oracle/_ref/libfealess_ref.so, libfealess_ref_icp.so and
//     linemod_if.cpp): oracle/ref/Makefile builds that as oracle/_ref/ref_cv_caller;
//   * against include/fealess_opencv_adapter.hpp and libfealess_hip.so / libcadreco_hip.so: the tests build that
//     (tests/test_cv_caller_cpu.py, tests/test_gpu_cv_caller.py).
// Both run on the containers of oracle/ref/opencv2 (a stand-in, not OpenCV).  The two builds differ in ONE function,
// obtain_detector(): the adapter reads <dir>/<det>/linemod_templates.yml with readLinemod; the reference's readLinemod needs
// cv::FileStorage, which the stand-in does not have, so that build makes the detector (getDefaultLINEMOD() where it fits) and
// fills it with addSyntheticTemplate / addPoseInfo from <dir>/<det>/bank.bin, the same bank in a plain binary file.
//
// usage: tu_cv_caller <case dir> <out dir> [kind]      (kind: run only the cases of that kind, e.g. "draw": no GPU needed)
// <case dir>/manifest.txt has one case per line, "kind name key=value ...", every value an integer (floats and doubles as
// their bit patterns) or a file stem; arrays are raw files in <case dir>.  Every output is a raw file
// <out dir>/<name>.<key>.<i32|u8|f32|f64>; <name>.status.i32 is {0, returned value} or {1, code == StsAssert} when a
// cv::Exception came out.  tests/cv_caller_cases.py writes the directory and reads the outputs.
#ifdef FL_REFERENCE_HEADERS
#include "linemod_if.h"
#include "ICP.h"
#include "detection.h"
#include "depth_to_3d.h"
#else
#include "fealess_opencv_adapter.hpp"
#endif

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <stdint.h>
#include <streambuf>
#include <string>
#include <vector>

namespace {

std::string g_in, g_out;

[[noreturn]] void die(const std::string &what)
{
  std::fprintf(stderr, "tu_cv_caller: %s\n", what.c_str());
  std::exit(2);
}

std::vector<uint8_t> load(const std::string &file)
{
  std::ifstream f((g_in + "/" + file).c_str(), std::ios::binary);
  if (!f) die("cannot read " + file);
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

void put(const std::string &name, const std::string &key, const char *ext, const void *p, size_t bytes)
{
  std::ofstream f((g_out + "/" + name + "." + key + "." + ext).c_str(), std::ios::binary);
  f.write(static_cast<const char *>(p), (std::streamsize)bytes);
  if (!f) die("cannot write " + name + "." + key);
}
void put_i32(const std::string &name, const std::string &key, const std::vector<int32_t> &v) { put(name, key, "i32", v.data(), 4 * v.size()); }

struct Args {
  std::string kind, name;
  std::map<std::string, std::string> kv;
  bool has(const std::string &k) const { return kv.count(k) != 0; }
  std::string s(const std::string &k, const std::string &dflt = "") const { return has(k) ? kv.find(k)->second : dflt; }
  long long i(const std::string &k, long long dflt = 0) const { return has(k) ? std::strtoll(kv.find(k)->second.c_str(), NULL, 10) : dflt; }
  float f32(const std::string &k) const
  {
    const uint32_t b = (uint32_t)std::strtoull(s(k, "0").c_str(), NULL, 10);
    float v;
    std::memcpy(&v, &b, 4);
    return v;
  }
  double f64(const std::string &k) const
  {
    const uint64_t b = std::strtoull(s(k, "0").c_str(), NULL, 10);
    double v;
    std::memcpy(&v, &b, 8);
    return v;
  }
};

// ---- the bank file: int32 words -- M, L, T[L], n_classes, then per class: name length, one word per character, n pyramids,
// and per pyramid 13 pose words (float bit patterns) and L * M templates (width, height, offset_x, offset_y, pyramid_level,
// n features, then x, y, label per feature)
struct BankClass {
  std::string name;
  std::vector<std::vector<cup_linemod::Template> > pyramids;
  std::vector<std::vector<float> > poses;
};
struct Bank {
  int M, L;
  std::vector<int> T;
  std::vector<BankClass> classes;
};

size_t read_templates(const int32_t *w, size_t o, int count, std::vector<cup_linemod::Template> &out)
{
  out.resize((size_t)count);
  for (int k = 0; k < count; ++k) {
    cup_linemod::Template &t = out[(size_t)k];
    t.width = w[o]; t.height = w[o + 1]; t.offset_x = w[o + 2]; t.offset_y = w[o + 3]; t.pyramid_level = w[o + 4];
    const int nf = w[o + 5];
    o += 6;
    for (int i = 0; i < nf; ++i, o += 3) {
      cup_linemod::Feature f;
      f.x = w[o]; f.y = w[o + 1]; f.label = w[o + 2];
      t.features.push_back(f);
    }
  }
  return o;
}

void write_templates(const std::vector<cup_linemod::Template> &tp, std::vector<int32_t> &out)
{
  for (size_t k = 0; k < tp.size(); ++k) {
    const int32_t hdr[6] = {tp[k].width, tp[k].height, tp[k].offset_x, tp[k].offset_y, tp[k].pyramid_level, (int32_t)tp[k].features.size()};
    out.insert(out.end(), hdr, hdr + 6);
    for (size_t i = 0; i < tp[k].features.size(); ++i) {
      out.push_back(tp[k].features[i].x);
      out.push_back(tp[k].features[i].y);
      out.push_back(tp[k].features[i].label);
    }
  }
}

Bank read_bank(const std::string &det)
{
  const std::vector<uint8_t> raw = load(det + "/bank.bin");
  const int32_t *w = reinterpret_cast<const int32_t *>(raw.data());
  Bank b;
  size_t o = 0;
  b.M = w[o++];
  b.L = w[o++];
  for (int l = 0; l < b.L; ++l) b.T.push_back(w[o++]);
  b.classes.resize((size_t)w[o++]);
  for (size_t c = 0; c < b.classes.size(); ++c) {
    BankClass &bc = b.classes[c];
    const int len = w[o++];
    for (int i = 0; i < len; ++i) bc.name.push_back((char)w[o++]);
    const int np = w[o++];
    bc.pyramids.resize((size_t)np);
    for (int p = 0; p < np; ++p) {
      std::vector<float> pose(13);
      std::memcpy(pose.data(), w + o, 13 * 4);
      o += 13;
      bc.poses.push_back(pose);
      o = read_templates(w, o, b.L * b.M, bc.pyramids[(size_t)p]);
    }
  }
  if (o * 4 != raw.size()) die("bank.bin of " + det + " is malformed");
  return b;
}

// ---- THE ONE FUNCTION in which the two builds differ -------------------------------------------------------------------
#ifdef FL_REFERENCE_HEADERS
cv::Ptr<cup_linemod::Detector> obtain_detector(const std::string &, const Bank &bank)
{
  cv::Ptr<cup_linemod::Detector> d;
  if (bank.M == 2 && bank.L == 2 && bank.T[0] == 5 && bank.T[1] == 8) {
    d = cup_linemod::getDefaultLINEMOD();
  } else {                                   // colour only, or another T: the same modalities with their default parameters
    std::vector<cv::Ptr<cup_linemod::Modality> > mods;
    mods.push_back(cv::makePtr<cup_linemod::ColorGradient>());
    if (bank.M == 2) mods.push_back(cv::makePtr<cup_linemod::DepthNormal>());
    d = cv::makePtr<cup_linemod::Detector>(mods, bank.T);
  }
  for (size_t c = 0; c < bank.classes.size(); ++c)          // file order, as readClass would meet them (linemod.cpp:1739-1760)
    for (size_t p = 0; p < bank.classes[c].pyramids.size(); ++p) {
      d->addSyntheticTemplate(bank.classes[c].pyramids[p], bank.classes[c].name);
      d->addPoseInfo(bank.classes[c].poses[p].data());
    }
  return d;
}
#else
cv::Ptr<cup_linemod::Detector> obtain_detector(const std::string &dir, const Bank &)
{
  return readLinemod(dir + "/linemod_templates.yml");
}
#endif

struct Loaded {
  Bank bank;
  cv::Ptr<cup_linemod::Detector> det;
};
Loaded &detector(const std::string &det)
{
  static std::map<std::string, Loaded> all;
  std::map<std::string, Loaded>::iterator it = all.find(det);
  if (it == all.end()) {
    Loaded l;
    l.bank = read_bank(det);
    l.det = obtain_detector(g_in + "/" + det, l.bank);
    it = all.insert(std::make_pair(det, l)).first;
  }
  return it->second;
}

// m itself, or a copy of it inside a larger matrix of 0xA5 bytes, returned as a ROI of that (not continuous)
cv::Mat placed(const cv::Mat &m, bool roi)
{
  if (!roi) return m;
  cv::Mat big(m.rows + 5, m.cols + 7, m.type());
  for (int r = 0; r < big.rows; ++r) std::memset(big.ptr(r), 0xA5, (size_t)big.cols * big.elemSize());
  cv::Mat view = big(cv::Rect(3, 2, m.cols, m.rows));
  for (int r = 0; r < m.rows; ++r) std::memcpy(view.ptr(r), m.ptr(r), (size_t)m.cols * m.elemSize());
  return view;
}

void put_mat(const std::string &name, const std::string &key, const cv::Mat &m, const char *ext)
{
  std::vector<uint8_t> bytes;
  for (int r = 0; r < m.rows && !m.empty(); ++r) bytes.insert(bytes.end(), m.ptr(r), m.ptr(r) + (size_t)m.cols * m.elemSize());
  put(name, key, ext, bytes.data(), bytes.size());
  const int32_t dims[3] = {m.empty() ? 0 : m.rows, m.empty() ? 0 : m.cols, m.empty() ? -1 : m.type()};
  put(name, key + "_dims", "i32", dims, sizeof(dims));
}

std::vector<std::string> split(const std::string &s, char sep)
{
  std::vector<std::string> out;
  std::stringstream ss(s);
  std::string item;
  while (std::getline(ss, item, sep)) out.push_back(item);
  return out;
}

// ---- the cases: each returns what the call returned; outputs that exist after a throw are written by the caller of these ----
struct MatchState {
  std::vector<cup_linemod::Match> matches;
  std::vector<cv::Mat> quantized;
};

int class_index(const Bank &bank, const cv::String &class_id)      // index in the bank file's order, -1 for an unknown name
{
  for (size_t c = 0; c < bank.classes.size(); ++c)
    if (bank.classes[c].name == std::string(class_id)) return (int)c;
  return -1;
}

int run_match(const Args &a, Loaded &ld, MatchState &st)
{
  const int w = (int)a.i("w"), h = (int)a.i("h");
  const bool roi = a.i("roi") != 0;
  std::vector<uint8_t> bgr = load(a.s("src") + ".bgr"), d16 = load(a.s("src") + ".d16");
  if (bgr.size() != (size_t)w * h * 3 || d16.size() != (size_t)w * h * 2) die("source size of " + a.name);
  std::vector<cv::Mat> sources;
  sources.push_back(placed(cv::Mat(h, w, CV_8UC3, bgr.data()), roi));
  if (a.i("nsrc", 2) == 2) sources.push_back(placed(cv::Mat(h, w, CV_16UC1, d16.data()), roi));
  std::vector<std::vector<uint8_t> > mask_bytes((size_t)a.i("nmask"));
  std::vector<cv::Mat> masks;
  for (size_t i = 0; i < mask_bytes.size(); ++i) {
    const std::string file = a.s("mask" + std::to_string(i), "-");
    if (file == "-") { masks.push_back(cv::Mat()); continue; }
    mask_bytes[i] = load(file);
    masks.push_back(placed(cv::Mat(h, w, CV_8UC1, mask_bytes[i].data()), roi));
  }
  std::vector<cv::String> ids;
  const std::vector<std::string> flt = split(a.s("filter"), ',');
  for (size_t i = 0; i < flt.size(); ++i) ids.push_back(flt[i]);
  const float threshold = a.f32("thr");
  const int r = a.i("quant") ? ld.det->match(sources, threshold, st.matches, ids, st.quantized, masks)
                             : ld.det->match(sources, threshold, st.matches, ids, cv::noArray(), masks);
  if (a.i("tpl") && !st.matches.empty()) {
    // the first match in the project's canonical order (similarity descending, template id ascending, then class in the bank
    // file's order, y, x): matches[0] itself is any one of the entries that tie in Match::operator<, the sort being unstable
    size_t first = 0;
    for (size_t i = 1; i < st.matches.size(); ++i) {
      const cup_linemod::Match &p = st.matches[i], &q = st.matches[first];
      const int pc = class_index(ld.bank, p.class_id), qc = class_index(ld.bank, q.class_id);
      if (p.similarity != q.similarity ? p.similarity > q.similarity
          : p.template_id != q.template_id ? p.template_id < q.template_id
          : pc != qc ? pc < qc : p.y != q.y ? p.y < q.y : p.x < q.x)
        first = i;
    }
    const cup_linemod::Match &m = st.matches[first];
    std::vector<int32_t> tw;
    write_templates(ld.det->getTemplates(m.class_id, m.template_id), tw);
    put_i32(a.name, "templates", tw);
    std::vector<float> poses;
    for (int t = 0; t < ld.det->numTemplates(); ++t) {      // the table is global (linemod.cpp:1617-1634, :1748)
      const std::vector<float> p = ld.det->getPoseInfo(t);
      poses.push_back((float)p.size());
      poses.insert(poses.end(), p.begin(), p.end());
    }
    put(a.name, "poses", "f32", poses.data(), 4 * poses.size());
    std::vector<int32_t> info;
    info.push_back(ld.det->numClasses());
    info.push_back(ld.det->numTemplates());
    info.push_back(ld.det->pyramidLevels());
    for (int l = 0; l < ld.det->pyramidLevels(); ++l) info.push_back(ld.det->getT(l));
    put_i32(a.name, "info", info);
    std::string names;
    const std::vector<cv::String> cls = ld.det->classIds();
    for (size_t i = 0; i < cls.size(); ++i) names += std::string(cls[i]) + "\n";
    put(a.name, "class_ids", "u8", names.data(), names.size());
  }
  return r;
}

void put_match_state(const Args &a, const Loaded &ld, const MatchState &st)
{
  std::vector<int32_t> out;
  for (size_t i = 0; i < st.matches.size(); ++i) {
    const cup_linemod::Match &m = st.matches[i];
    const int32_t cls = class_index(ld.bank, m.class_id);
    int32_t sim;
    std::memcpy(&sim, &m.similarity, 4);
    const int32_t row[5] = {m.x, m.y, sim, cls, m.template_id};
    out.insert(out.end(), row, row + 5);
  }
  put_i32(a.name, "matches", out);
  const int32_t nq = (int32_t)st.quantized.size();
  put(a.name, "n_quantized", "i32", &nq, 4);
  for (size_t i = 0; i < st.quantized.size(); ++i) put_mat(a.name, "quantized" + std::to_string(i), st.quantized[i], "u8");
}

int run_detection(const Args &a)
{
  const int mw = (int)a.i("mw"), mh = (int)a.i("mh"), sw = (int)a.i("sw"), sh = (int)a.i("sh");
  const bool roi = a.i("roi") != 0;
  std::vector<uint8_t> md = load(a.name + ".model.d16"), sd = load(a.name + ".scene.d16"), rt = load(a.name + ".rt.f32");
  if (md.size() != (size_t)mw * mh * 2 || sd.size() != (size_t)sw * sh * 2 || rt.size() != 48) die("input size of " + a.name);
  const cv::Mat model = placed(cv::Mat(mh, mw, CV_16UC1, md.data()), roi), scene = placed(cv::Mat(sh, sw, CV_16UC1, sd.data()), roi);
  TCamIntrinsicParam k;
  k.nWidth = sw; k.nHeight = sh;
  k.dFx = a.f64("fx"); k.dFy = a.f64("fy"); k.dCx = a.f64("cx"); k.dCy = a.f64("cy");
  const cv::Rect_<int> rm((int)a.i("rm0"), (int)a.i("rm1"), (int)a.i("rm2"), (int)a.i("rm3"));
  const cv::Rect_<int> rr((int)a.i("rr0"), (int)a.i("rr1"), (int)a.i("rr2"), (int)a.i("rr3"));
  const float *f = reinterpret_cast<const float *>(rt.data());
  const cv::Matx33f r_match(f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]);
  const cv::Vec3f t_match(f[9], f[10], f[11]);
  cv::Vec3f T_final;
  cv::Matx33f R_final;
  detection(model, scene, k, rm, rr, (int)a.i("it"), a.f32("dist_mean_thr"), a.f32("dist_diff_thr"), r_match, t_match, 0.0f, T_final, R_final);
  float pose[12];
  std::memcpy(pose, R_final.val, 36);
  std::memcpy(pose + 9, T_final.val, 12);
  put(a.name, "pose", "f32", pose, sizeof(pose));
  return 0;
}

int run_icp(const Args &a)
{
  const std::vector<uint8_t> rb = load(a.name + ".ref.f32"), mb = load(a.name + ".model.f32");
  std::vector<cv::Vec3f> ref(rb.size() / 12), model(mb.size() / 12);
  for (size_t i = 0; i < ref.size(); ++i) std::memcpy(ref[i].val, rb.data() + 12 * i, 12);
  for (size_t i = 0; i < model.size(); ++i) std::memcpy(model[i].val, mb.data() + 12 * i, 12);
  // what the reference leaves alone when it refuses (fewer than 3 points) must stay as the caller had it
  cv::Matx33f R(7.f, 7.f, 7.f, 7.f, 7.f, 7.f, 7.f, 7.f, 7.f);
  cv::Vec3f T(7.f, 7.f, 7.f);
  float px = 7.f;
  const float d = a.has("it") ? icpCloudToCloud_Ex(ref, model, R, T, px, (int)a.i("it"), a.f32("dist_mean_thr"), a.f32("dist_diff_thr"))
                              : icpCloudToCloud_Ex(ref, model, R, T, px);          // the defaults of ICP.h:170-172
  float out[14];
  std::memcpy(out, R.val, 36);
  std::memcpy(out + 9, T.val, 12);
  out[12] = px;
  out[13] = d;
  put(a.name, "result", "f32", out, sizeof(out));
  return 0;
}

int run_depth3d(const Args &a)
{
  const int w = (int)a.i("w"), h = (int)a.i("h"), kr = (int)a.i("krows"), kc = (int)a.i("kcols");
  std::vector<uint8_t> db = load(a.name + ".depth.d16"), kb = load(a.name + ".K.f64");
  if (db.size() != (size_t)w * h * 2 || kb.size() != (size_t)kr * kc * 8) die("input size of " + a.name);
  const cv::Mat depth = placed(cv::Mat(h, w, CV_16UC1, db.data()), a.i("roi") != 0);
  cv::Mat K(kr, kc, CV_64FC1, kb.data());
  if (a.i("ktype") == CV_32F) {
    cv::Mat Kf;
    K.convertTo(Kf, CV_32F);
    K = Kf;
  }
  cv::Mat points;
  cup_d2pc::depthTo3d(depth, K, points);
  put_mat(a.name, "points", points, "f32");
  return 0;
}

// both drawResponse overloads: dst (CV_8UC3, given) afterwards, and cv::circle's log
int run_draw(const Args &a)
{
  const int rows = (int)a.i("rows"), cols = (int)a.i("cols"), M = (int)a.i("m");
  std::vector<uint8_t> db = load(a.name + ".dst.u8"), tb = load(a.name + ".templates.i32");
  if (db.size() != (size_t)rows * cols * 3) die("input size of " + a.name);
  std::vector<cup_linemod::Template> tp;
  if (read_templates(reinterpret_cast<const int32_t *>(tb.data()), 0, (int)a.i("ntempl"), tp) * 4 != tb.size()) die("templates of " + a.name);
  cv::Mat dst(rows, cols, CV_8UC3, db.data());
  const cv::Point offset((int)a.i("offx"), (int)a.i("offy"));
  cv::fealess_circle_log().clear();
  if (a.i("six")) {
    const int cr = (int)a.i("ctrows"), cc = (int)a.i("ctcols");
    std::vector<uint8_t> cb = load(a.name + ".ct.u8");
    if (cb.size() != (size_t)cr * cc * 3) die("input size of " + a.name);
    drawResponse(tp, M, dst, offset, (int)a.i("t"), cv::Mat(cr, cc, CV_8UC3, cb.data()));
  } else {
    drawResponse(tp, M, dst, offset, (int)a.i("t"));
  }
  put_mat(a.name, "dst", dst, "u8");
  std::vector<double> log;
  const std::vector<cv::FealessCircleCall> &calls = cv::fealess_circle_log();
  for (size_t i = 0; i < calls.size(); ++i) {
    const double row[8] = {(double)calls[i].center.x, (double)calls[i].center.y, (double)calls[i].radius, calls[i].color.val[0],
                           calls[i].color.val[1], calls[i].color.val[2], calls[i].color.val[3], (double)calls[i].thickness};
    log.insert(log.end(), row, row + 8);
  }
  put(a.name, "circles", "f64", log.data(), 8 * log.size());
  return 0;
}

class NullBuf : public std::streambuf {
 protected:
  virtual int overflow(int c) { return c; }
};

}  // namespace

int main(int argc, char **argv)
{
  if (argc < 3) die("usage: tu_cv_caller <case dir> <out dir> [kind]");
  g_in = argv[1];
  g_out = argv[2];
  const std::string only = argc > 3 ? argv[3] : "";
  NullBuf quiet;                                   // the reference's ICP sources print to std::cout
  std::streambuf *old = std::cout.rdbuf(&quiet);
  std::ifstream mf((g_in + "/manifest.txt").c_str());
  if (!mf) die("no manifest.txt");
  std::string line;
  int n_run = 0;
  while (std::getline(mf, line)) {
    if (line.empty() || line[0] == '#') continue;
    const std::vector<std::string> tok = split(line, ' ');
    Args a;
    a.kind = tok[0];
    a.name = tok[1];
    for (size_t i = 2; i < tok.size(); ++i) {
      const size_t eq = tok[i].find('=');
      if (eq == std::string::npos) die("manifest: " + line);
      a.kv[tok[i].substr(0, eq)] = tok[i].substr(eq + 1);
    }
    if (!only.empty() && a.kind != only) continue;
    int32_t status[2] = {0, 0};
    MatchState st;
    Loaded *ld = a.kind == "match" ? &detector(a.s("det")) : NULL;
    try {
      if (a.kind == "match") status[1] = run_match(a, *ld, st);
      else if (a.kind == "detection") status[1] = run_detection(a);
      else if (a.kind == "icp") status[1] = run_icp(a);
      else if (a.kind == "depth3d") status[1] = run_depth3d(a);
      else if (a.kind == "draw") status[1] = run_draw(a);
      else die("manifest: unknown kind " + a.kind);
    } catch (const cv::Exception &e) {
      status[0] = 1;
      status[1] = e.code == cv::Error::StsAssert ? 1 : 0;
    }
    if (ld) put_match_state(a, *ld, st);          // also after a throw or a -1: what the call left in its outputs
    put(a.name, "status", "i32", status, sizeof(status));
    ++n_run;
  }
  std::cout.rdbuf(old);
  std::printf("cases %d\n", n_run);
  return 0;
}
