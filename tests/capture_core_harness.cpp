// fvad_capture_core.h (the decisions k_cap_plan compiles, here as plain C++)
// against a direct model on random cases: the due test, the cut of a clip to
// the held range, the pending queue's overflow, ring room and the placement
// rule.  The model works in 128-bit signed integers on interval ends, the
// header in unsigned 64-bit cursors.  Cases cluster at the edges: a clip ending
// exactly at the stream's position, starting exactly at the held range's
// start, a base inside the clip, a history longer than the stream, empty
// clips, cursors near 2^64 (a ring's cursors only ever enter as differences).
// Built with -fsanitize=address,undefined by tests/test_capture_cpu.py.
// Usage: capture_core_harness [cases]
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <vector>

#include "fvad_capture_core.h"

namespace cap = fvad::cap;
typedef __int128 i128;
typedef unsigned long long u64;

int main(int argc, char **argv) {
  const long cases = argc > 1 ? std::atol(argv[1]) : 200000;
  std::mt19937_64 rng(20240607);
  auto U = [&](u64 n) { return n ? rng() % n : 0ull; };
  long bad = 0, head = 0, tail = 0, none = 0, whole = 0;

  // due + cut
  for (long it = 0; it < cases; it++) {
    const u64 history = 192000 + U(700000);
    const u64 pos = U(4) == 0 ? U(history) : U(3000000);
    const u64 base = U(3) == 0 ? U(pos + 1) : 0;
    u64 from, to;
    switch (U(6)) {
      case 0: from = U(pos + 1); to = pos; break;                                  // ends at the position
      case 1: from = pos > history ? pos - history : 0; to = from + U(400000); break;  // starts at the held start
      case 2: from = base; to = base + U(400000); break;
      case 3: from = U(pos + 1); to = from; break;                                  // empty
      default: from = U(pos + 200000); to = from + U(600000); break;
    }
    const bool flush = U(4) == 0;
    const bool d = cap::due(to, pos, flush);
    if (d != (flush || (i128)to <= (i128)pos)) bad++;
    if (!d) continue;
    const cap::Cut c = cap::cut(from, to, pos, base, history);
    const i128 lo = std::max<i128>((i128)base, std::max<i128>(0, (i128)pos - (i128)history));
    const i128 a = std::max<i128>((i128)from, lo), b = std::min<i128>((i128)to, (i128)pos);
    const i128 n = std::max<i128>(0, b - a);
    unsigned flags = 0;
    if ((i128)from < lo) flags |= cap::kHeadShort;
    if ((i128)to > (i128)pos) flags |= cap::kTailShort;
    if (n == 0) flags |= cap::kNoAudio;
    const i128 first = n > 0 ? a : std::min<i128>(a, (i128)pos);
    if ((i128)c.n != n || c.flags != flags || (i128)c.first != first) {
      if (bad < 10)
        std::printf("cut: from %llu to %llu pos %llu base %llu history %llu -> first %llu n %llu flags %u\n", from, to,
                    pos, base, history, c.first, c.n, c.flags);
      bad++;
    }
    // what is delivered lies inside the clip and inside the held range
    if (c.n && !(c.first >= from && c.first + c.n <= to && (i128)c.first >= lo && c.first + c.n <= pos)) bad++;
    head += !!(c.flags & cap::kHeadShort);
    tail += !!(c.flags & cap::kTailShort);
    none += !!(c.flags & cap::kNoAudio);
    whole += c.flags == 0;
  }

  // the pending queue: pushes and removals of due entries against a deque
  long overflow = 0;
  for (long it = 0; it < cases / 20; it++) {
    cap::Pend q[cap::kQueue];
    unsigned n = 0;
    std::deque<unsigned> model;
    unsigned seq = 0;
    for (int step = 0; step < 40; step++) {
      if (U(3)) {
        cap::Pend p{U(1000), U(1000), seq, 0};
        const bool ok = cap::queue_push(q, &n, p);
        const bool want = model.size() < (size_t)cap::kQueue;
        if (want) model.push_back(seq);
        overflow += !want;
        if (ok != want) bad++;
        seq++;
      } else if (n) {  // the plan's compaction: entries leave, the rest keep their order
        unsigned keep = 0;
        std::deque<unsigned> left;
        for (unsigned i = 0; i < n; i++) {
          if (U(2)) {
            q[keep++] = q[i];
            left.push_back(model[i]);
          }
        }
        n = keep;
        model = left;
      }
      if (n != model.size()) bad++;
      for (unsigned i = 0; i < n && i < model.size(); i++)
        if (q[i].seq != model[i]) bad++;
    }
  }

  // ring room and placement: cursors anywhere in 64 bits, the read cursor at
  // most `cap` behind; the placed clips are a prefix and never exceed the room
  long placed_some = 0, refused_some = 0;
  for (long it = 0; it < cases / 10; it++) {
    const u64 capy = 1 + U(U(2) ? 2000000 : 50);
    const u64 used = U(capy + (U(5) == 0 ? 10 : 1));
    const u64 wr = U(2) ? rng() : U(1000000) + used, rd = wr - used;
    const u64 room = cap::ring_room(wr, rd, capy);
    const i128 want_room = std::max<i128>(0, (i128)capy - (i128)used);
    if ((i128)room != want_room) bad++;
    u64 before = 0;
    i128 sum = 0;
    bool stopped = false;
    for (int k = 0; k < 12; k++) {
      const u64 len = U(U(2) ? capy / 3 + 2 : 2 * capy + 2);
      const bool f = cap::fits(before, len, room);
      if (f != ((i128)before + (i128)len <= (i128)room)) bad++;
      if (f && stopped && len > 0) bad++;  // (an empty clip takes no room wherever it stands)
      if (f) sum = (i128)before + len;
      else stopped = true;
      placed_some += f;
      refused_some += !f;
      before += len;
    }
    if (sum > (i128)room) bad++;
  }
  // fits must not wrap: lengths and offsets near 2^64
  if (cap::fits(~0ull - 5, 10, 100) || cap::fits(5, ~0ull - 2, 100) || !cap::fits(0, 100, 100) || cap::fits(1, 100, 100))
    bad++;

  std::printf("cut cases: %ld head-short, %ld tail-short, %ld without audio, %ld whole; queue overflows %ld; "
              "placed %ld refused %ld\n", head, tail, none, whole, overflow, placed_some, refused_some);
  const bool vacuous = !head || !tail || !none || !whole || !overflow || !placed_some || !refused_some;
  if (vacuous) std::printf("FAIL: a kind of case never occurred\n");
  std::printf("%ld / %ld mismatches\n", bad, cases);
  return bad || vacuous ? 1 : 0;
}
