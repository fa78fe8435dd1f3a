// Input resampling to 48 kHz (fvad_engine_config.input_rate; DESIGN.md section
// 7, "Input resampling"): the index arithmetic and the accumulate loop, for
// host and device.  k_resample (fvad_resample.hip) and fvad_resample_host
// (fvad_resample.cpp) both run this code, so they agree by the bits.
//
// A tick is 10 ms: n = rate / 100 input samples give 480 output samples.
// With g = gcd(48000, rate), L = 48000 / g and M = rate / g, output r of a
// tick reads the K inputs ending at i = floor(r M / L) through phase
// p = r M mod L of a polyphase FIR of L x K taps; 480 M / L = n, so every
// tick starts at phase 0 and the arithmetic never needs an absolute index.
#pragma once
#pragma clang fp contract(off)
#include "fvad_exact.h"  // FVAD_HD

namespace fvad {
namespace rs {

constexpr int kOut = 480;      // output samples per tick
constexpr int kRates = 6;      // the closed list of input rates
constexpr int kMaxTaps = 160 * 48;  // L * K at 44.1 kHz, the largest table
constexpr int kMaxTail = 95;   // K - 1 at 96 kHz, the longest history

// One description serves both directions (fvad_engine_config.input_rate brings
// `rate` to 48 kHz, denoised_rate brings 48 kHz to `rate`): n = rate / 100 is a
// tick's samples at the rate that is not 48000.
struct Desc {
  int rate, L, M, K, n;
};
enum class Dir { kIn, kOut };  // to 48 kHz; from 48 kHz

FVAD_HD inline int gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// The closed list of rates, 48000 among them: a per-stream engine's stream has
// a listed rate or 48000, which is not resampled.  The index of a rate in
// ascending order, -1 off the list.
constexpr int kPsRates = kRates + 1;
constexpr int kPsIndex48 = 5;

FVAD_HD inline int rate_index(int rate) {
  switch (rate) {
    case 8000: return 0;
    case 16000: return 1;
    case 24000: return 2;
    case 32000: return 3;
    case 44100: return 4;
    case 48000: return kPsIndex48;
    case 96000: return 6;
    default: return -1;
  }
}

FVAD_HD inline int index_rate(int index) {
  constexpr int r[kPsRates] = {8000, 16000, 24000, 32000, 44100, 48000, 96000};
  return r[index];
}

// A rate that is resampled; false off the list and at 48000.  kIn: L = 48000 /
// g, M = rate / g.  kOut, the decimating direction (DESIGN.md section 7,
// "Output rate of the denoised PCM"): a tick's 480 denoised samples give n,
// L = rate / g, M = 48000 / g; output r reads the K 48 kHz samples ending at
// i = floor(r M / L) through phase p = r M mod L, and 480 L / M = n, so a tick
// starts at phase 0 there too.
FVAD_HD inline bool describe(int rate, Dir dir, Desc &d) {
  if (rate_index(rate) < 0 || rate == 48000) return false;
  const int g = gcd(48000, rate);
  d.rate = rate;
  d.L = (dir == Dir::kIn ? 48000 : rate) / g;
  d.M = (dir == Dir::kIn ? rate : 48000) / g;
  d.K = 48 * ((d.M + d.L - 1) / d.L);  // 48 max(1, ceil(M / L))
  d.n = rate / 100;
  return true;
}

// a per-stream engine's rate: describe, and 48000 as the identity L = M = K = 1
// (no filter, no history), in either direction
FVAD_HD inline bool describe_ps(int rate, Dir dir, Desc &d) {
  if (rate != 48000) return describe(rate, dir, d);
  d.rate = 48000;
  d.L = d.M = d.K = 1;
  d.n = kOut;
  return true;
}

constexpr int kIn = 480;            // 48 kHz samples per tick
constexpr int kMaxTapsOut = 147 * 96;  // kOut: L * K at 44.1 kHz, the largest table
constexpr int kMaxTailOut = 287;    // kOut: K - 1 at 8 kHz, the longest history (<= 480: inside one tick)

// output r of a tick: the newest input it reads (relative to the tick's first
// sample) and its phase.  r M <= 479 * 147 (kIn), 440 * 160 (kOut).
FVAD_HD inline void position(int r, int L, int M, int &i, int &p) {
  const int rm = r * M;
  i = rm / L;
  p = rm - i * L;
}

// 16-bit input k: k_pcm16's conversion, exact in f32
FVAD_HD inline float sample(float v) { return v; }
FVAD_HD inline float sample(short v) { return (float)v * (1.0f / 32768.0f); }

// N outputs of one phase: acc[n] = sum over k ascending of tap(k) * x(n, k),
// x(n, k) the input k samples before output n's newest.  The product is
// rounded to f32, then the sum; nothing fused (the pragma above, and the
// host's -ffp-contract=off), nothing re-associated.
template <int N, typename Tap, typename X>
FVAD_HD inline void accumulate(int K, Tap tap, X x, float (&acc)[N]) {
  for (int n = 0; n < N; n++) acc[n] = 0.0f;
  for (int k = 0; k < K; k++) {
    const float t = tap(k);
    for (int n = 0; n < N; n++) acc[n] = acc[n] + t * x(n, k);
  }
}

}  // namespace rs
}  // namespace fvad
