// fvad_rnnfeat_core.h (the feature formulas k_rnn3 / k_rnn3f / k_gru16 /
// k_fused16 compile, here as plain C++) against a direct model of rnnoise's
// compute_frame_features: the cepstral row write, the deltas from rows mem_id,
// mem_id - 1, mem_id - 2, all 8 x 8 distances recomputed from the cepstral
// memory, the rows' minima and sv / 8 - 2.1.  The core is driven the way the
// kernels drive it: per active frame its 37 items in a shuffled order (the
// kernels run them side by side), then the eight row minima, their sum in row
// order, and the mem_id advance; an inactive frame calls nothing.  Compared by
// bits after every frame: features 0..41, the whole cepstral memory, the whole
// distance matrix, mem_id.  Sequences start from a fresh stream's all-zero
// state and hold at least 40 active frames (mem_id wraps five times), inactive
// frames at random positions, repeated rows (ties, zero distances), values of
// mixed sign and magnitude and -0.0f.  gain_smooth is compared with
// max(.6f * lastg, g) on random pairs, equal ones included.
// Built with -fsanitize=address,undefined by tests/test_rnnfeat_cpu.py.
// Usage: rnnfeat_core_harness [sequences]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>

#include "fvad_rnnfeat_core.h"

using namespace fvad;
constexpr int kRaw = kBands + 7;  // Lyf[22], features 34..40
static_assert(kFeat == 42, "feature count");

struct State {
  float ceps[kCeps * kBands], dist[kCeps * kCeps];
  int memid;
};

// the C algorithm, every distance from the memory
static void model_frame(State &m, const float *raw, float *feat) {
  float(*mem)[kBands] = reinterpret_cast<float(*)[kBands]>(m.ceps);
  float *c0 = mem[m.memid];
  const float *c1 = mem[m.memid < 1 ? kCeps + m.memid - 1 : m.memid - 1];
  const float *c2 = mem[m.memid < 2 ? kCeps + m.memid - 2 : m.memid - 2];
  for (int i = 0; i < kBands; i++) feat[i] = c0[i] = raw[i];
  m.memid++;
  for (int i = 0; i < 6; i++) {
    feat[i] = c0[i] + c1[i] + c2[i];
    feat[kBands + i] = c0[i] - c2[i];
    feat[kBands + 6 + i] = c0[i] - 2 * c1[i] + c2[i];
  }
  if (m.memid == kCeps) m.memid = 0;
  for (int i = 0; i < 7; i++) feat[34 + i] = raw[kBands + i];
  float sv = 0;
  for (int i = 0; i < kCeps; i++) {
    float mindist = 1e15f;
    for (int j = 0; j < kCeps; j++) {
      float d = 0;
      for (int k = 0; k < kBands; k++) {
        const float tmp = mem[i][k] - mem[j][k];
        d += tmp * tmp;
      }
      m.dist[i * kCeps + j] = d;
      if (j != i) mindist = mindist < d ? mindist : d;
    }
    sv += mindist;
  }
  feat[41] = sv / kCeps - 2.1;
}

int main(int argc, char **argv) {
  const long seqs = argc > 1 ? std::atol(argv[1]) : 300;
  std::mt19937 rng(20240921);
  auto U = [&](unsigned n) { return (int)(rng() % n); };
  auto value = [&]() -> float {
    if (U(16) == 0) return U(2) ? 0.0f : -0.0f;
    const float mag = std::ldexp(1.0f + (rng() & 0xffffff) / 16777216.0f, U(30) - 20);  // 2^-20 .. 2^10
    return U(2) ? mag : -mag;
  };
  long bad = 0, frames = 0, idle = 0, repeats = 0, wraps = 0, zero_d = 0, ties = 0;
  for (long q = 0; q < seqs; q++) {
    State c{}, m{};  // all zero: a fresh stream
    float raw[kRaw] = {};
    for (int active = 0, n = 0; active < 40 + (int)(q % 25); n++) {
      if (n > 0 && U(8) == 0) {  // an inactive frame: no call, nothing moves
        idle++;
      } else {
        const int kind = U(6);  // 0: the previous row again; 1: a row of the memory; else a new one
        if (kind == 1) std::memcpy(raw, c.ceps + U(kCeps) * kBands, kBands * sizeof(float));
        if (kind > 1 || n == 0)
          for (float &v : raw) v = value();
        repeats += kind <= 1;
        float fc[kFeat] = {}, fm[kFeat] = {};
        int order[rnnfeat::kItems];
        std::iota(order, order + rnnfeat::kItems, 0);
        std::shuffle(order, order + rnnfeat::kItems, rng);
        for (int i : order) rnnfeat::feat_item(raw, c.ceps, c.dist, c.memid, i, [&](int k, float v) { fc[k] = v; });
        float mins[kCeps], sv = 0;
        for (int i = kCeps - 1; i >= 0; i--) mins[i] = rnnfeat::dist_row_min(c.dist, i);
        for (int i = 0; i < kCeps; i++) sv += mins[i];
        fc[41] = rnnfeat::spec_variability(sv);
        c.memid = rnnfeat::memid_next(c.memid);
        wraps += c.memid == 0;
        model_frame(m, raw, fm);
        if (std::memcmp(fc, fm, sizeof fc)) {
          if (bad < 10) std::printf("features differ: sequence %ld frame %d\n", q, n);
          bad++;
        }
        for (int i = 0; i < kCeps; i++)
          for (int j = 0; j < i; j++) {
            zero_d += c.dist[i * kCeps + j] == 0;
            ties += j > 0 && c.dist[i * kCeps + j] == c.dist[i * kCeps + j - 1];
          }
        active++;
      }
      frames++;
      if (std::memcmp(c.ceps, m.ceps, sizeof c.ceps) || std::memcmp(c.dist, m.dist, sizeof c.dist) ||
          c.memid != m.memid) {
        if (bad < 10) std::printf("state differs: sequence %ld frame %d\n", q, n);
        bad++;
      }
    }
  }
  // gain smoothing: gains and their memory lie in [0, 1]
  const long pairs = 100000;
  long equal = 0;
  for (long it = 0; it < pairs; it++) {
    const float lastg = U(10) == 0 ? 0.0f : (rng() & 0xffffff) / 16777216.0f;
    const float g = U(4) == 0 ? .6f * lastg : (rng() & 0xffffff) / 16777216.0f;
    const float got = rnnfeat::gain_smooth(g, lastg), want = std::max(.6f * lastg, g);
    equal += g == .6f * lastg;
    if (std::memcmp(&got, &want, sizeof got)) bad++;
  }
  std::printf("%ld frames (%ld inactive, %ld repeated rows), %ld mem_id wraps, %ld zero distances, %ld ties; "
              "%ld gain pairs (%ld equal)\n", frames, idle, repeats, wraps, zero_d, ties, pairs, equal);
  const bool vacuous = !idle || !repeats || wraps < 5 * seqs || !zero_d || !ties || !equal;
  if (vacuous) std::printf("FAIL: a kind of case never occurred\n");
  std::printf("%ld / %ld mismatches\n", bad, frames + pairs);
  return bad || vacuous ? 1 : 0;
}
