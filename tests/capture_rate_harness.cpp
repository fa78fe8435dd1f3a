// fvad_capture_core.h's clip-rate arithmetic as plain C++ against a direct
// model on random cases: cap::to_rate (ceil(x L / M) in 128-bit integers, and
// by its definition: the first clip-rate sample r with r M / L >= x), the due
// test in either unit for positions that are multiples of 480, the cut of a
// converted segment in clip-rate units, and cap::to_s16 against lrint in
// double.  The seven rates are the engine's: 48000 and rs::describe's six.
// Built with -fsanitize=address,undefined by tests/test_capture_den_cpu.py.
// Usage: capture_rate_harness [cases]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "fvad_capture_core.h"

namespace cap = fvad::cap;
typedef __int128 i128;
typedef unsigned long long u64;

static u64 gcd64(u64 a, u64 b) { return b ? gcd64(b, a % b) : a; }

int main(int argc, char **argv) {
  const long cases = argc > 1 ? std::atol(argv[1]) : 200000;
  std::mt19937_64 rng(20240915);
  auto U = [&](u64 n) { return n ? rng() % n : 0ull; };
  const int rates[7] = {48000, 8000, 16000, 24000, 32000, 44100, 96000};
  long bad = 0, head = 0, tail = 0, none = 0, whole = 0, due_n = 0;

  for (long it = 0; it < cases; it++) {
    const int rate = rates[U(7)];
    const u64 g = gcd64(48000, (u64)rate);
    const unsigned L = (unsigned)(rate / g), M = (unsigned)(48000 / g);
    // to_rate against the model, up to 2^56 / L
    const u64 x = U(4) == 0 ? U(1ull << 48) : U(4000000);
    const u64 r = cap::to_rate(x, L, M);
    const i128 want = ((i128)x * L + (M - 1)) / M;
    if ((i128)r != want) bad++;
    // r is the first clip-rate sample at or after x: r M >= x L > (r - 1) M
    if (!((i128)r * M >= (i128)x * L && (r == 0 || (i128)(r - 1) * M < (i128)x * L))) bad++;
    if (rate == 48000 && r != x) bad++;

    // a stream `ticks` ticks in: at pos 48 kHz samples and pos L / M clip-rate samples
    const u64 frame = (u64)rate / 100, ticks = U(7000), pos = ticks * 480, pos_r = ticks * frame;
    if ((i128)pos * L != (i128)pos_r * M) bad++;
    const double hsec = 4.0 + (double)U(1000) / 100.0;
    const u64 history = (u64)std::floor((double)rate * hsec);
    const u64 base_t = U(3) == 0 ? U(ticks + 1) : 0, base_r = base_t * frame;
    u64 from, to;
    switch (U(6)) {
      case 0: from = U(pos + 1); to = pos; break;                          // ends at the position
      case 1: from = U(pos + 1); to = pos + 1; break;                      // ends one 48 kHz sample past it
      case 2: from = U(pos + 1); to = pos ? pos - 1 : 0; if (from > to) from = to; break;
      case 3: from = U(pos + 1); to = from; break;                         // empty
      default: from = U(pos + 200000); to = from + U(600000); break;
    }
    const u64 from_r = cap::to_rate(from, L, M), to_r = cap::to_rate(to, L, M);
    // a clip is due in the same push in either unit
    if (cap::due(to_r, pos_r, false) != cap::due(to, pos, false)) {
      if (bad < 10) std::printf("due: rate %d to %llu pos %llu -> to_r %llu pos_r %llu\n", rate, to, pos, to_r, pos_r);
      bad++;
    }
    const bool flush = U(4) == 0;
    if (!cap::due(to_r, pos_r, flush)) continue;
    due_n++;
    // the cut in clip-rate units against the model: the samples r of the held
    // range [lo, pos_r) with from <= r M / L < to
    const cap::Cut c = cap::cut(from_r, to_r, pos_r, base_r, history);
    const i128 lo = std::max<i128>((i128)base_r, std::max<i128>(0, (i128)pos_r - (i128)history));
    const i128 a = std::max<i128>((i128)from_r, lo), b = std::min<i128>((i128)to_r, (i128)pos_r);
    const i128 n = std::max<i128>(0, b - a);
    unsigned flags = 0;
    if ((i128)from_r < lo) flags |= cap::kHeadShort;
    if ((i128)to_r > (i128)pos_r) flags |= cap::kTailShort;
    if (n == 0) flags |= cap::kNoAudio;
    const i128 first = n > 0 ? a : std::min<i128>(a, (i128)pos_r);
    if ((i128)c.n != n || c.flags != flags || (i128)c.first != first) {
      if (bad < 10)
        std::printf("cut: rate %d from %llu to %llu pos %llu base %llu history %llu -> first %llu n %llu flags %u\n", rate,
                    from_r, to_r, pos_r, base_r, history, c.first, c.n, c.flags);
      bad++;
    }
    if (c.n) {  // every delivered sample lies in the segment, by the definition, and the ones beside it do not
      const u64 r0 = c.first, r1 = c.first + c.n - 1;
      if (!((i128)r0 * M >= (i128)from * L && (i128)r1 * M < (i128)to * L)) bad++;
      if (!(c.flags & cap::kHeadShort) && r0 > 0 && (i128)(r0 - 1) * M >= (i128)from * L) bad++;
      if (!(c.flags & cap::kTailShort) && (i128)(r1 + 1) * M < (i128)to * L) bad++;
    }
    head += !!(c.flags & cap::kHeadShort);
    tail += !!(c.flags & cap::kTailShort);
    none += !!(c.flags & cap::kNoAudio);
    whole += c.flags == 0;
  }

  // to_s16 against round-half-even in double (the product is exact there too)
  long s16_bad = 0;
  auto model = [](float x) -> int {
    if (std::isnan(x)) return 0;
    const double y = std::nearbyint((double)x * 32768.0);  // (the default rounding mode: to nearest even)
    return (int)std::min(32767.0, std::max(-32768.0, y));
  };
  std::uniform_real_distribution<float> dist(-1.5f, 1.5f);
  for (long it = 0; it < cases; it++) {
    const float x = dist(rng);
    if (cap::to_s16(x) != model(x)) s16_bad++;
  }
  for (int k = -40000; k <= 40000; k++) {
    const float x = ((float)k + 0.5f) / 32768.0f;
    if (cap::to_s16(x) != model(x)) s16_bad++;
  }
  const float inf = std::numeric_limits<float>::infinity();
  const float edge[] = {1.0f, -1.0f, 0.0f, -0.0f, std::numeric_limits<float>::quiet_NaN(), inf, -inf, 1e30f, -1e30f,
                        std::numeric_limits<float>::denorm_min()};
  for (float x : edge)
    if (cap::to_s16(x) != model(x)) s16_bad++;
  if (cap::to_s16(1.0f) != 32767 || cap::to_s16(-1.0f) != -32768 || cap::to_s16(inf) != 32767 ||
      cap::to_s16(-inf) != -32768 || cap::to_s16(edge[4]) != 0 || cap::to_s16(0.5f / 32768.0f) != 0 ||
      cap::to_s16(1.5f / 32768.0f) != 2 || cap::to_s16(-2.5f / 32768.0f) != -2)
    s16_bad++;

  std::printf("due %ld: whole %ld head %ld tail %ld none %ld\n", due_n, whole, head, tail, none);
  std::printf("%ld / %ld mismatches, %ld s16 mismatches\n", bad, cases, s16_bad);
  // the cases must have exercised every outcome
  const bool vacuous = !(whole > 100 && head > 100 && tail > 100 && none > 100);
  return bad || s16_bad || vacuous ? 1 : 0;
}
