// fvad_eval_core.h's eval_lane (the code k_sweep_score compiles, here as plain
// C++) against fvad_eval_stats (libfvad.so, the oracle) on random cases, by the
// eleven statistics' bits, NaN for NaN.  Segment lists are machine-like: samples
// in time order, padded by 2 s, so neighbours overlap.  Labels are unsorted,
// overlap, are zero-length, repeat a start, or touch a segment's edge exactly;
// every combination of the four stat-config fields being zero or not occurs.
// Then the sortedness check: a list with one start below its predecessor's
// gives kEvalUnsorted wherever the pair stands, and equal starts do not.
// Run by tests/test_sweep_score_cpu.py.  Usage: eval_core_harness [cases]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "fvad_eval_core.h"

int main(int argc, char **argv) {
  const long cases = argc > 1 ? std::atol(argv[1]) : 200000;
  std::mt19937 rng(12345);
  auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
  long bad = 0, nan_fields = 0, opponents2 = 0;
  for (long it = 0; it < cases; it++) {
    const int nv = rng() % 12, nr = rng() % 10;
    std::vector<unsigned long long> sf, st;
    unsigned long long t = rng() % 100000;
    for (int i = 0; i < nv; i++) {
      t += rng() % 150000;
      const unsigned long long len = rng() % 300000;
      sf.push_back(t > 96000 ? t - 96000 : 0);
      st.push_back(t + len + 96000);
      if (rng() % 3) t += len;
    }
    std::vector<float> vs, rs;
    for (int i = 0; i < nv; i++) {
      vs.push_back((float)sf[i] / 48000.0f);
      vs.push_back((float)st[i] / 48000.0f);
    }
    for (int j = 0; j < nr; j++) {
      float a = U(0, 30), b = a + U(0, 4);
      const int k = rng() % 8;
      if (k == 0) b = a;                                // zero length
      if (k == 1 && !rs.empty()) a = rs[rs.size() - 2];  // the previous label's start
      if (k == 2 && nv) {                                // ends exactly at a segment's start
        b = vs[2 * (rng() % nv)];
        a = b - U(0, 2);
      }
      if (k == 3 && nv) {  // starts exactly at a segment's end
        a = vs[2 * (rng() % nv) + 1];
        b = a + U(0, 2);
      }
      rs.push_back(a);
      rs.push_back(b);
    }
    fvad_stat_config c;
    const unsigned m = rng() % 16;
    c.ignore_shorter_than_sec = m & 1 ? U(0, 1) : 0;
    c.extrude_start = m & 2 ? U(0, 1) : 0;
    c.extrude_end = m & 4 ? U(0, 2) : 0;
    c.fill_gaps = m & 8 ? U(0, 1) : 0;
    fvad_single_stats ref, got;
    if (fvad_eval_stats(vs.data(), nv, rs.data(), nr, &c, &ref) != FVAD_OK) return 2;
    std::vector<std::pair<float, float>> lab;  // the caller's part: stably sorted by start
    for (int j = 0; j < nr; j++) lab.emplace_back(rs[2 * j], rs[2 * j + 1]);
    std::stable_sort(lab.begin(), lab.end(),
                     [](const std::pair<float, float> &a, const std::pair<float, float> &b) { return a.first < b.first; });
    std::vector<float> ls;
    for (const auto &l : lab) {
      ls.push_back(l.first);
      ls.push_back(l.second);
    }
    for (int i = 0; i < nv; i++) {
      int opp = 0;
      for (int j = 0; j < nr; j++) opp += fvad::eval_overlap(vs[2 * i], vs[2 * i + 1], rs[2 * j], rs[2 * j + 1]) > 0.0f;
      opponents2 += opp >= 2;
    }
    const auto seg = [&](size_t i, float *from, float *to) {
      *from = (float)sf[i] / 48000.0f;
      *to = (float)st[i] / 48000.0f;
    };
    if (fvad::eval_lane(seg, (size_t)nv, ls.data(), (size_t)nr, c, &got) != fvad::kEvalScored) {
      bad++;
      continue;
    }
    const float *a = &ref.total_positives_sec, *b = &got.total_positives_sec;
    for (int k = 0; k < 11; k++) {
      if (a[k] != a[k]) {
        nan_fields++;
        bad += b[k] == b[k];
      } else {
        bad += std::memcmp(a + k, b + k, 4) != 0;
      }
    }
  }
  std::printf("%ld / %ld mismatches, %ld NaN fields, %ld segments with two or more opponents\n", bad, cases, nan_fields,
              opponents2);
  // the sortedness check
  long unsorted_bad = 0;
  const fvad_stat_config z{0, 0, 0, 0};
  const float lab[2] = {1.0f, 2.0f};
  for (int n = 2; n <= 9; n++)
    for (int at = 1; at < n; at++)
      for (int equal = 0; equal < 2; equal++) {
        std::vector<float> from(n);
        for (int i = 0; i < n; i++) from[i] = 0.5f * (float)i;
        from[at] = equal ? from[at - 1] : from[at - 1] - 0.25f;
        fvad_single_stats out;
        const unsigned rc = fvad::eval_lane(
            [&](size_t i, float *f, float *t) {
              *f = from[i];
              *t = from[i] + 1.0f;
            },
            (size_t)n, lab, 1, z, &out);
        unsorted_bad += rc != (equal ? fvad::kEvalScored : fvad::kEvalUnsorted);
      }
  std::printf("sortedness: %ld wrong\n", unsorted_bad);
  return bad != 0 || unsorted_bad != 0 || opponents2 == 0;
}
