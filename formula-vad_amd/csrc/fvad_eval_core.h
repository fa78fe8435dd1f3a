// The evaluator's statistics of one lane (fvad_eval_stats, fvad_host.cpp, the
// oracle), without allocation and for host and device: k_sweep_score
// (fvad_sweep_score.hip) and the host-only fvad_sweep_run_score run this code.
// Every sum is taken in fvad_eval_stats' order, so the eleven statistics are
// its bits.
//
// What makes one pass enough.  fvad_eval_stats collects a segment's opponents
// (the labels that overlap it, in sorted order) into arrays, extrudes them --
// first start minus extrude_start, last end plus extrude_end, an end pulled up
// to the next start where the gap is at most fill_gaps -- and then sums the
// overlaps.  An opponent's extruded interval is final once the next opponent
// is known (the gap rule reads the next one's untouched start) or the list
// ends (extrude_end), so the loop below keeps one pending interval and adds
// its overlap when the next opponent arrives, in the same order as the
// array's sum.  The false negatives need no list at all: a label's opponents
// are the segments with a positive overlap, and those are the terms it adds.
//
// Requirements, as fvad_eval_stats establishes them by sorting: the labels
// stably sorted by start (the caller's, once per stream), the segment starts
// non-decreasing (a VADMachine's are: vadm_fsm emits in time order, so the
// oracle's stable sort of them is the identity).  The second is checked here:
// kEvalUnsorted and no score.
#pragma once
#pragma clang fp contract(off)
#include <cmath>
#include <cstddef>

#include "../../include/fvad.h"
#include "fvad_exact.h"

namespace fvad {

enum : unsigned { kEvalScored = 0, kEvalOverCapacity = 1, kEvalUnsorted = 2 };

FVAD_HD inline float eval_overlap(float af, float at, float bf, float bt) {
  const float max_from = af > bf ? af : bf;
  const float min_to = at < bt ? at : bt;
  return min_to - max_from;
}

FVAD_HD inline float eval_f_score(float beta, float p, float r) {
  const float b2 = beta * beta;
  return (1 + b2) * (p * r) / (b2 * p + r);
}

// seg(i, &from, &to): segment i of n_seg in seconds.  lab: n_lab (from, to)
// pairs.  Returns kEvalScored with *out written, or kEvalUnsorted.
template <class SegFn>
FVAD_HD inline unsigned eval_lane(SegFn &&seg, size_t n_seg, const float *lab, size_t n_lab,
                                  const fvad_stat_config &c, fvad_single_stats *out) {
  float total = 0.0f, tps = 0.0f, fps = 0.0f, fns = 0.0f, prev = 0.0f;
  for (size_t i = 0; i < n_seg; i++) {
    float vf, vt;
    seg(i, &vf, &vt);
    if (i > 0 && !(vf >= prev)) return kEvalUnsorted;
    prev = vf;
    bool have = false;
    float pf = 0.0f, pt = 0.0f, ov = 0.0f;  // the pending opponent, extruded so far
    for (size_t j = 0; j < n_lab; j++) {
      const float rf = lab[2 * j], rt = lab[2 * j + 1];
      if (rf >= vt) break;  // sorted by start: this label and every later one overlap by <= 0
      if (!(eval_overlap(vf, vt, rf, rt) > 0.0f)) continue;
      if (!have) {
        pf = rf - c.extrude_start;
        have = true;
      } else {
        if (rf - pt <= c.fill_gaps) pt = rf;
        const float o = eval_overlap(vf, vt, pf, pt);
        ov += 0.0f > o ? 0.0f : o;
        pf = rf;
      }
      pt = rt;
    }
    if (have) {
      pt += c.extrude_end;
      const float o = eval_overlap(vf, vt, pf, pt);
      ov += 0.0f > o ? 0.0f : o;
    }
    const float fp = (vt - vf) - ov;
    fps += fp;
    const float tp = (vt - vf) - fp;
    tps += tp;
    total += tp;
  }
  for (size_t j = 0; j < n_lab; j++) {
    const float rf = lab[2 * j], rt = lab[2 * j + 1];
    if ((rt - rf) < c.ignore_shorter_than_sec) continue;
    float ov = 0.0f;
    for (size_t i = 0; i < n_seg; i++) {
      float vf, vt;
      seg(i, &vf, &vt);
      if (vf >= rt) break;  // non-decreasing starts: no later segment overlaps
      const float o = eval_overlap(rf, rt, vf, vt);
      if (o > 0.0f) ov += o;
    }
    const float fn = (rt - rf) - ov;
    fns += fn;
    total += fn;
  }
  fvad_single_stats s;
  s.total_positives_sec = total;
  s.true_positives_sec = tps;
  s.false_positives_sec = fps;
  s.false_negatives_sec = fns;
  s.true_positive_rate = tps / total;
  s.false_negative_rate = fns / total;
  s.false_discovery_rate = fps / (fps + tps);
  s.precision = tps / (tps + fps);
  s.f_score_beta = 0.7f;
  s.f_score = eval_f_score(s.f_score_beta, s.precision, s.true_positive_rate);
  s.fm_index = sqrtf(s.precision * s.true_positive_rate);
  *out = s;
  return kEvalScored;
}

}  // namespace fvad
