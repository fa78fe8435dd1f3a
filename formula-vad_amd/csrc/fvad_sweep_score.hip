// Config sweep, the scores (fvad_sweep_run_score):
//
//   k_sweep_score  lane/(stream, config)  the evaluator's statistics
//                                         (fvad_eval_core.h: fvad_eval_stats'
//                                         bits) of the lane's segments against
//                                         its stream's labels
//
// k_vadm_sweep's grid: a wave is 64 configs of one stream, so the labels (all
// streams' in one array, each stream's stably sorted by start) are
// wave-uniform loads.  It runs on the sweep's stream directly after a chunk's
// k_vadm_sweep and reads that chunk's VadmState.n_segs and VadmSeg rows where
// they lie; only the statistics and a status word per lane go back to the
// host.  A lane's row is contiguous, the rows of a wave are seg_cap * 24 bytes
// apart, and the label loop walks the row once per label (up to the first
// segment that starts past the label).  The row is read and converted to
// seconds in place each time, through the caches: a form that converted it
// once into LDS as [segment][lane] was measured and was slower for what the
// LDS costs in resident waves.  Lanes past n_cfgs leave
// at once; a lane whose total exceeds seg_cap writes its status and leaves.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>

#include "fvad_eval_core.h"
#include "fvad_sweep.h"

namespace fvad {

__global__ void __launch_bounds__(64) k_sweep_score(ScoreArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x, s = blockIdx.y;
  if (c >= a.n_cfgs) return;
  const size_t lane = (size_t)s * a.n_cfgs + c;
  const unsigned n = a.st[lane].n_segs;
  if (n > (unsigned)a.seg_cap) {
    a.status[lane] = kEvalOverCapacity;
    return;
  }
  const VadmSeg *seg = a.seg + lane * (size_t)a.seg_cap;
  const long long l0 = a.lab_off[s], l1 = a.lab_off[s + 1];
  const fvad_stat_config sc = a.stat[(size_t)c * a.stat_stride];
  fvad_single_stats out;
  const unsigned rc = eval_lane(
      [&](size_t i, float *from, float *to) {
        *from = (float)seg[i].sample_from / 48000.0f;
        *to = (float)seg[i].sample_to / 48000.0f;
      },
      n, a.lab + 2 * l0, (size_t)(l1 - l0), sc, &out);
  a.status[lane] = rc;
  if (rc == kEvalScored) a.single[lane] = out;
}

hipError_t launch_sweep_score(const ScoreArgs &a, hipStream_t stream) {
  if (a.n_cfgs <= 0 || a.n_streams <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sweep_score, dim3((unsigned)((a.n_cfgs + 63) / 64), (unsigned)a.n_streams), dim3(64), 0, stream,
                     a);
  return hipGetLastError();
}

}  // namespace fvad
