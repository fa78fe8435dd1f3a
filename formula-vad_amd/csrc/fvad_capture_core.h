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
