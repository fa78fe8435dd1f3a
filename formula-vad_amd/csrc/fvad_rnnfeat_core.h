// The recurrence's feature formulas, for host and device: what k_rnn3 /
// k_rnn3f (fvad_rnn3.hip) and k_gru16 / k_fused16 (fvad_gru16.hip) compute
// beside the GRU stack on their serial frame loop.  The kernels reach this code
// through fvad_rnnfeat.h; tests/rnnfeat_core_harness.cpp checks it as plain
// C++ against a direct model.  No LDS, no HIP types, no lane ids.  Bit-exact
// code: every expression and its evaluation order is compute_frame_features'
// (rnnoise denoise.c), compiled with -ffp-contract=off.
//
// Per stream: ceps[kCeps][kBands] is the cepstral memory, row mi (mem_id) the
// one a frame overwrites; dist[kCeps][kCeps] the squared distances between its
// rows, kept incrementally: a frame changes row mi only, so only row and
// column mi are recomputed.  (k_frame, fvad_kernels.hip, recomputes all of
// them per frame as the C source does and stays independent of this file.)
#pragma once
#include "fvad_exact.h"  // FVAD_HD
#include "fvad_internal.h"

#define FVAD_HDI FVAD_HD inline __attribute__((always_inline))

namespace fvad {
namespace rnnfeat {

constexpr int kItems = kBands + 7 + kCeps;  // items of one frame's features (feat_item)

// One of an active frame's 37 items, in any order and side by side; c0 is the
// frame's raw feature row (Lyf[22], then features 34..40), put(k, v) takes
// feature k.
//   i < 22     cepstral row mi, element i; feature i (i < 6: and the deltas
//              22 + i, 28 + i from rows mi, mi - 1, mi - 2)
//   22..28     features 34..40
//   29..36     distance of row j = i - 29 to the new row mi -> [mi][j], [j][mi]
// (items < 22 write ceps row mi, items >= 29 read the other rows and c0 only)
template <class Put>
FVAD_HDI void feat_item(const float *c0, float *ceps, float *dist, int mi, int i, Put put) {
  if (i < kBands) {
    ceps[mi * kBands + i] = c0[i];
    if (i < 6) {
      const float *c1 = ceps + ((mi < 1) ? kCeps + mi - 1 : mi - 1) * kBands;
      const float *c2 = ceps + ((mi < 2) ? kCeps + mi - 2 : mi - 2) * kBands;
      put(i, c0[i] + c1[i] + c2[i]);
      put(kBands + i, c0[i] - c2[i]);
      put(kBands + 6 + i, c0[i] - 2 * c1[i] + c2[i]);
    } else {
      put(i, c0[i]);
    }
  } else if (i < kBands + 7) {
    put(34 + i - kBands, c0[i]);
  } else {
    const int j = i - kBands - 7;
    if (j != mi) {
      const float *cj = ceps + j * kBands;
      float d = 0;
#pragma unroll
      for (int k = 0; k < kBands; k++) {
        const float tmp = c0[k] - cj[k];
        d += tmp * tmp;
      }
      dist[mi * kCeps + j] = d;
      dist[j * kCeps + mi] = d;
    }
  }
}

// smallest distance of row i to another row, in j order
FVAD_HDI float dist_row_min(const float *dist, int i) {
  float mindist = 1e15f;
#pragma unroll
  for (int j = 0; j < kCeps; j++)
    if (j != i) mindist = (mindist < dist[i * kCeps + j]) ? mindist : dist[i * kCeps + j];
  return mindist;
}
// feature 41 from the sum of the rows' minima, added in row order
FVAD_HDI float spec_variability(float sv) { return (float)(sv / kCeps - 2.1); }
FVAD_HDI int memid_next(int mi) { return mi + 1 == kCeps ? 0 : mi + 1; }

// gain smoothing g = max(g, .6 * lastg) (denoise.c)
FVAD_HDI float gain_smooth(float gi, float lastg) {
  const float al = .6f * lastg;
  return (gi > al) ? gi : al;
}

}  // namespace rnnfeat
}  // namespace fvad
