// The judge, host code above the C ABI: Evaluator / statistics / formats
// (Evaluator.zig:90-156, Evaluator/statistics.zig:85-284, formats.zig:7-36).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fvad.h"

namespace {
struct Seg {
  float from, to;
  std::vector<size_t> opp;
};
float overlap_with(float af, float at, float bf, float bt) {
  const float max_from = af > bf ? af : bf;
  const float min_to = at < bt ? at : bt;
  return min_to - max_from;
}
void sort_by_start(std::vector<Seg> &v) {
  std::stable_sort(v.begin(), v.end(), [](const Seg &a, const Seg &b) { return a.from < b.from; });
}
float false_positive(const Seg &v, const std::vector<Seg> &refs, const fvad_stat_config &c) {
  // extrudeSegments (statistics.zig:191-218) + calcOverlapMany
  const size_t n = v.opp.size();
  std::vector<float> f(n), t(n);
  for (size_t i = 0; i < n; i++) {
    f[i] = refs[v.opp[i]].from;
    t[i] = refs[v.opp[i]].to;
  }
  if (n > 0) {
    f[0] -= c.extrude_start;
    t[n - 1] += c.extrude_end;
    for (size_t i = 0; i + 1 < n; i++)
      if (f[i + 1] - t[i] <= c.fill_gaps) t[i] = f[i + 1];
  }
  float ov = 0.0f;
  for (size_t i = 0; i < n; i++) {
    const float o = overlap_with(v.from, v.to, f[i], t[i]);
    ov += 0.0f > o ? 0.0f : o;
  }
  return (v.to - v.from) - ov;
}
float f_score(float beta, float p, float r) {
  const float b2 = beta * beta;  // std.math.pow(f32, beta, 2)
  return (1 + b2) * (p * r) / (b2 * p + r);
}
}  // namespace

extern "C" int fvad_eval_stats(const float *vad, size_t nv, const float *ref, size_t nr, const fvad_stat_config *cfg,
                               fvad_single_stats *out) {
  if ((!vad && nv) || (!ref && nr) || !cfg || !out) return FVAD_EINVAL;
  std::vector<Seg> vs(nv), rs(nr);
  for (size_t i = 0; i < nv; i++) vs[i] = {vad[2 * i], vad[2 * i + 1], {}};
  for (size_t i = 0; i < nr; i++) rs[i] = {ref[2 * i], ref[2 * i + 1], {}};
  sort_by_start(vs);
  sort_by_start(rs);
  for (auto &v : vs)
    for (size_t j = 0; j < rs.size(); j++)
      if (overlap_with(v.from, v.to, rs[j].from, rs[j].to) > 0.0f) v.opp.push_back(j);
  for (auto &r : rs)
    for (size_t j = 0; j < vs.size(); j++)
      if (overlap_with(r.from, r.to, vs[j].from, vs[j].to) > 0.0f) r.opp.push_back(j);
  fvad_single_stats s;
  std::memset(&s, 0, sizeof(s));
  for (const auto &v : vs) {
    s.false_positives_sec += false_positive(v, rs, *cfg);
    const float tp = (v.to - v.from) - false_positive(v, rs, *cfg);
    s.true_positives_sec += tp;
    s.total_positives_sec += tp;
  }
  for (const auto &r : rs) {
    if ((r.to - r.from) < cfg->ignore_shorter_than_sec) continue;
    float ov = 0.0f;
    for (size_t j : r.opp) {
      const float o = overlap_with(r.from, r.to, vs[j].from, vs[j].to);
      ov += 0.0f > o ? 0.0f : o;
    }
    const float fn = (r.to - r.from) - ov;
    s.false_negatives_sec += fn;
    s.total_positives_sec += fn;
  }
  s.true_positive_rate = s.true_positives_sec / s.total_positives_sec;
  s.false_negative_rate = s.false_negatives_sec / s.total_positives_sec;
  s.false_discovery_rate = s.false_positives_sec / (s.false_positives_sec + s.true_positives_sec);
  s.precision = s.true_positives_sec / (s.true_positives_sec + s.false_positives_sec);
  s.f_score_beta = 0.7f;
  s.f_score = f_score(s.f_score_beta, s.precision, s.true_positive_rate);
  s.fm_index = std::sqrt(s.precision * s.true_positive_rate);
  *out = s;
  return FVAD_OK;
}

extern "C" void fvad_eval_aggregate(const fvad_single_stats *st, size_t n, fvad_aggregate_stats *a) {
  std::memset(a, 0, sizeof(*a));
  fvad_agg_stat *aggs[4] = {&a->true_positive_rate, &a->false_negative_rate, &a->false_discovery_rate, &a->precision};
  for (auto *x : aggs) {
    x->min = 2;
    x->max = -2;
  }
  float sums[4] = {0, 0, 0, 0};
  for (size_t i = 0; i < n; i++) {
    const fvad_single_stats &s = st[i];
    a->total_positives_sec += s.total_positives_sec;
    a->true_positives_sec += s.true_positives_sec;
    a->false_positives_sec += s.false_positives_sec;
    a->false_negatives_sec += s.false_negatives_sec;
    const float vals[4] = {s.true_positive_rate, s.false_negative_rate, s.false_discovery_rate, s.precision};
    for (int k = 0; k < 4; k++) {
      sums[k] += vals[k];
      if (vals[k] < aggs[k]->min) aggs[k]->min = vals[k];
      if (vals[k] > aggs[k]->max) aggs[k]->max = vals[k];
    }
  }
  const float nf = (float)n;
  a->true_positive_rate.overall = a->true_positives_sec / a->total_positives_sec;
  a->false_negative_rate.overall = a->false_negatives_sec / a->total_positives_sec;
  a->false_discovery_rate.overall = a->false_positives_sec / (a->false_positives_sec + a->true_positives_sec);
  a->precision.overall = a->true_positives_sec / (a->true_positives_sec + a->false_positives_sec);
  for (int k = 0; k < 4; k++) aggs[k]->avg = sums[k] / nf;
  a->f_score_beta = 0.7f;
  a->f_score = f_score(a->f_score_beta, a->precision.overall, a->true_positive_rate.overall);
  a->fm_index = std::sqrt(a->precision.overall * a->true_positive_rate.overall);
}

extern "C" long fvad_parse_audacity(const char *txt, size_t len, float *out, size_t cap) {
  // formats.parseAudacitySegments: split the raw text on '\n' (CRs are NOT
  // stripped, formats.zig:11-14), each line on '\t'; lines with < 2 fields are
  // skipped, an unparsable from/to field is an error.
  long n = 0;
  size_t pos = 0;
  while (pos <= len) {
    size_t e = pos;
    while (e < len && txt[e] != '\n') e++;
    size_t t1 = pos;
    while (t1 < e && txt[t1] != '\t') t1++;
    if (t1 < e) {
      size_t t2 = t1 + 1;
      while (t2 < e && txt[t2] != '\t') t2++;
      const std::string a(txt + pos, t1 - pos), b(txt + t1 + 1, t2 - t1 - 1);
      if (a.empty() || b.empty()) return FVAD_EFORMAT;
      char *end = nullptr;
      const float from = std::strtof(a.c_str(), &end);
      if (*end) return FVAD_EFORMAT;
      const float to = std::strtof(b.c_str(), &end);
      if (*end) return FVAD_EFORMAT;
      if ((size_t)n < cap && out) {
        out[2 * n] = from;
        out[2 * n + 1] = to;
      }
      n++;
    }
    pos = e + 1;
  }
  return n;
}
