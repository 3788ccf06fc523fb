// mesh_io.cpp -- fealess::ReadObj: the Wavefront OBJ subset a CAD export needs (positions, normals, polygons).
#include "fealess_cadreco.h"

#include <cmath>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <utility>

namespace fealess {
namespace {

bool parse_float(const std::string &tok, float &v)
{
  if (tok.empty()) return false;
  const char *s = tok.c_str();
  char *end = nullptr;
  v = std::strtof(s, &end);
  return end == s + tok.size() && std::isfinite(v);
}

// "12", "-3": a 1-based or relative index resolved against `count` (the number defined so far); 0 on failure
long parse_index(const std::string &tok, long count)
{
  if (tok.empty()) return 0;
  const char *s = tok.c_str();
  char *end = nullptr;
  const long i = std::strtol(s, &end, 10);
  if (end != s + tok.size() || i == 0) return 0;
  return i > 0 ? i : count + 1 + i;      // -1 = the last one defined so far; <= 0 when it reaches before the first
}

int fail(std::string *err, int code, const std::string &msg)
{
  if (err) *err = msg;
  return code;
}

}  // namespace

int ReadObj(const std::string &path, float scale, Mesh &out, std::string *err)
{
  if (!(std::isfinite(scale) && scale > 0.f)) return fail(err, (int)ERROR_INVALID_PARAM, "scale must be finite and > 0");
  std::ifstream in(path.c_str());
  if (!in) return fail(err, (int)ERROR_OPEN_FILE_FAILED, "cannot open " + path);
  std::vector<float> pos, nrm;
  std::vector<std::pair<long, long> > corners;   // (position, normal or 0), 1-based, 3 per triangle
  bool all_normals = true;
  std::string line;
  int lineno = 0;
  while (std::getline(in, line)) {
    ++lineno;
    std::istringstream ls(line);
    std::string kw;
    if (!(ls >> kw)) continue;
    const std::string where = path + ":" + std::to_string(lineno);
    if (kw == "v" || kw == "vn") {
      std::string tok;
      float c[3];
      for (int k = 0; k < 3; ++k)
        if (!(ls >> tok) || !parse_float(tok, c[k])) return fail(err, (int)ERROR_INVALID_PARAM, where + ": bad " + kw + " record");
      std::vector<float> &dst = kw == "v" ? pos : nrm;
      for (int k = 0; k < 3; ++k) dst.push_back(kw == "v" ? c[k] * scale : c[k]);
    } else if (kw == "f") {
      std::vector<std::pair<long, long> > poly;
      std::string tok;
      while (ls >> tok) {
        const size_t s1 = tok.find('/');
        const size_t s2 = s1 == std::string::npos ? std::string::npos : tok.find('/', s1 + 1);
        const long vi = parse_index(tok.substr(0, s1), (long)pos.size() / 3);
        if (vi <= 0) return fail(err, (int)ERROR_INVALID_PARAM, where + ": bad vertex index '" + tok + "'");
        if (s1 != std::string::npos && s2 == std::string::npos) {            // i/j: the texture index is checked, not used
          const std::string tj = tok.substr(s1 + 1);
          char *end = nullptr;
          if (tj.empty() || (std::strtol(tj.c_str(), &end, 10), end != tj.c_str() + tj.size()))
            return fail(err, (int)ERROR_INVALID_PARAM, where + ": bad face corner '" + tok + "'");
        }
        long ni = 0;
        if (s2 != std::string::npos) {
          const std::string tj = tok.substr(s1 + 1, s2 - s1 - 1);
          char *end = nullptr;
          if (!tj.empty() && (std::strtol(tj.c_str(), &end, 10), end != tj.c_str() + tj.size()))
            return fail(err, (int)ERROR_INVALID_PARAM, where + ": bad face corner '" + tok + "'");
          ni = parse_index(tok.substr(s2 + 1), (long)nrm.size() / 3);
          if (ni <= 0) return fail(err, (int)ERROR_INVALID_PARAM, where + ": bad normal index '" + tok + "'");
        }
        if (ni == 0) all_normals = false;
        poly.emplace_back(vi, ni);
      }
      if (poly.size() < 3) return fail(err, (int)ERROR_INVALID_PARAM, where + ": a face needs three corners");
      for (size_t k = 1; k + 1 < poly.size(); ++k) {                         // fan
        corners.push_back(poly[0]);
        corners.push_back(poly[k]);
        corners.push_back(poly[k + 1]);
      }
    }
  }
  if (corners.empty()) return fail(err, (int)ERROR_INVALID_PARAM, path + ": no faces");
  const long nv = (long)pos.size() / 3, nn = (long)nrm.size() / 3;
  for (auto &c : corners)
    if (c.first > nv || c.second > nn) return fail(err, (int)ERROR_INVALID_PARAM, path + ": face index out of range");
  Mesh m;
  if (all_normals) {
    std::map<std::pair<long, long>, int> id;                                // (position, normal) -> output vertex
    for (auto &c : corners) {
      auto it = id.find(c);
      if (it == id.end()) {
        it = id.emplace(c, (int)(m.vertices.size() / 3)).first;
        for (int k = 0; k < 3; ++k) {
          m.vertices.push_back(pos[3 * (c.first - 1) + k]);
          m.normals.push_back(nrm[3 * (c.second - 1) + k]);
        }
      }
      m.triangles.push_back(it->second);
    }
  } else {
    m.vertices = pos;
    for (auto &c : corners) m.triangles.push_back((int)(c.first - 1));
  }
  out = std::move(m);
  return SUCCESS;
}

}  // namespace fealess
