// Clip capture: the plan's decisions, for host and device.  k_cap_plan
// (fvad_capture.hip) runs this code; tests/capture_core_harness.cpp checks it
// as plain C++ against a direct model.  Integer arithmetic only.
//
// A clip is a machine segment [from, to) of a stream, waiting in the stream's
// pending queue until the stream holds `to` samples.  At the end of a push the
// stream is at sample `pos` and the history ring holds [max(base, pos -
// history), pos): `base` is the stream's first sample of this life (0, or the
// position of its last reset or restore).  A due clip is cut to what is held.
#pragma once
#include <cmath>

#include "fvad_exact.h"  // FVAD_HD

namespace fvad {
namespace cap {

constexpr int kQueue = 4;  // pending clips per stream
// fvad_clip.flags (include/fvad.h)
constexpr unsigned kHeadShort = 1, kTailShort = 2, kNoAudio = 4;

struct Pend {  // one pending clip
  unsigned long long from, to;
  unsigned seq, pad;
};
struct Cut {  // what of a due clip is delivered: [first, first + n)
  unsigned long long first, n;
  unsigned flags;
};

// A capture of the denoised rows works in samples of the clip rate R = 48000
// L / M (fvad_resample_core.h's describe, kOut; L = M = 1 for the 48 kHz
// signals): 48 kHz sample x is covered from clip-rate sample ceil(x L / M) on,
// so the segment [from, to) covers [to_rate(from), to_rate(to)), the r with
// from <= r M / L < to.  x < 2^56 (L <= 147).  A stream's position, a multiple
// of 480, maps exactly (480 L / M = R / 100), so a clip is due in the same
// push in either unit: to_rate(to) <= pos L / M iff to <= pos.
FVAD_HD inline unsigned long long to_rate(unsigned long long x, unsigned L, unsigned M) {
  return (x * L + (M - 1)) / M;
}

// f32 -> 16-bit PCM: clamp(rint(x * 32768), -32768, 32767), ties to even (the
// product is exact, a power of two), NaN -> 0
FVAD_HD inline short to_s16(float x) {
  float y = rintf(x * 32768.0f);
  if (!(y == y)) return 0;
  y = y < -32768.0f ? -32768.0f : y;
  y = y > 32767.0f ? 32767.0f : y;
  return (short)(int)y;
}

// the stream holds the clip's last sample (or a flush ends it now)
FVAD_HD inline bool due(unsigned long long to, unsigned long long pos, bool flush) { return flush || to <= pos; }

// the held part of [from, to) of a stream at `pos`.  Nothing held (the clip
// lies wholly before the held range, or is empty): n = 0 and kNoAudio.
FVAD_HD inline Cut cut(unsigned long long from, unsigned long long to, unsigned long long pos,
                       unsigned long long base, unsigned long long history) {
  unsigned long long lo = pos > history ? pos - history : 0ull;
  if (lo < base) lo = base;
  Cut c;
  c.flags = 0;
  c.first = from;
  if (c.first < lo) {
    c.first = lo;
    c.flags |= kHeadShort;
  }
  unsigned long long end = to;
  if (end > pos) {  // (only a flush cuts a clip before its end)
    end = pos;
    c.flags |= kTailShort;
  }
  if (end <= c.first) {
    c.first = c.first < pos ? c.first : pos;
    c.n = 0;
    c.flags |= kNoAudio;
  } else {
    c.n = end - c.first;
  }
  return c;
}

// a new clip into a stream's queue of *n entries; false: the queue is full
// and the new clip, the newest, is the one lost
FVAD_HD inline bool queue_push(Pend *q, unsigned *n, const Pend &p) {
  if (*n >= (unsigned)kQueue) return false;
  q[(*n)++] = p;
  return true;
}

// Free entries of a ring of `cap` behind the write cursor `wr`, given a read
// cursor `rd` that is never ahead of the reader's true one
FVAD_HD inline unsigned long long ring_room(unsigned long long wr, unsigned long long rd, unsigned long long cap) {
  const unsigned long long used = wr - rd;
  return used < cap ? cap - used : 0ull;
}

// A pass places its due clips in list order; `before` is the total length of
// the clips ahead of this one in the pass, placed or not, so the clips that
// get room are a prefix of the list: once one does not fit, no newer one is
// placed in this pass either.
FVAD_HD inline bool fits(unsigned long long before, unsigned long long len, unsigned long long room) {
  return len <= room && before <= room - len;
}

}  // namespace cap
}  // namespace fvad
