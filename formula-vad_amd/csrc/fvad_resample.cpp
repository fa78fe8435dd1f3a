// Resampling to and from 48 kHz, host side: the tap design (f64, once per rate
// and direction) and fvad_resample_host / fvad_resample_out_host, the mirrors
// of k_resample / k_resample_out the tests hold the kernels to
// (fvad_resample_core.h is the arithmetic they share).  No GPU.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/fvad.h"
#include "fvad_hip_own.h"  // fvad::set_error
#include "fvad_resample.h"

namespace {

// modified Bessel function of the first kind, order 0: sum ((x/2)^k / k!)^2
double bessel_i0(double x) {
  const double q = x * x / 4.0;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; k++) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

// Kaiser-windowed sinc of L phases x K taps at the prototype rate Fp = L * src,
// src the rate of the samples it reads (the input rate; 48000 for the
// decimating direction): A = 80 dB, the stop band from min(rate, 48000) / 2 on,
// rate the rate that is not 48000, the transition below it; scaled so the taps
// sum to L (each phase then has unit gain at DC, nearly)
void design(int L, int K, int src, int rate, std::vector<float> &taps) {
  const double kPi = 3.14159265358979323846;
  const int N = L * K;
  const double A = 80.0, beta = 0.1102 * (A - 8.7), Fp = (double)L * src;
  const double df = (A - 8.0) / (2.285 * (N - 1)) * Fp / (2.0 * kPi);
  const double f_stop = (rate < 48000 ? rate : 48000) / 2.0, fc = f_stop - df / 2.0;
  std::vector<double> proto((size_t)N);
  const double i0b = bessel_i0(beta);
  double sum = 0.0;
  for (int j = 0; j < N; j++) {
    const double x = 2.0 * fc / Fp * ((double)j - (N - 1) / 2.0);
    const double sinc = x == 0.0 ? 1.0 : std::sin(kPi * x) / (kPi * x);
    const double w = 2.0 * j / (double)(N - 1) - 1.0, in = 1.0 - w * w;
    proto[j] = sinc * bessel_i0(beta * std::sqrt(in > 0.0 ? in : 0.0)) / i0b;
    sum += proto[j];
  }
  taps.resize((size_t)N);
  for (int p = 0; p < L; p++)
    for (int k = 0; k < K; k++) taps[(size_t)p * K + k] = (float)(proto[(size_t)k * L + p] * ((double)L / sum));
}

int rate_slot(int rate) {
  const int rates[fvad::rs::kRates] = {8000, 16000, 24000, 32000, 44100, 96000};
  for (int i = 0; i < fvad::rs::kRates; i++)
    if (rates[i] == rate) return i;
  return -1;
}

}  // namespace

// the [L][K] table of a listed rate, designed on first use and kept; the
// filter reads samples at the rate itself (kIn) or at 48000 (kOut)
const std::vector<float> &fvad::resample_table(rs::Dir dir, const rs::Desc &d) {
  static std::vector<float> tables[2][rs::kRates];
  static std::once_flag once[2][rs::kRates];
  const int o = dir == rs::Dir::kOut, i = rate_slot(d.rate);
  std::call_once(once[o][i], [&] { design(d.L, d.K, o ? 48000 : d.rate, d.rate, tables[o][i]); });
  return tables[o][i];
}

namespace {
using fvad::rs::Dir;
const char *const kInRates = "input_rate must be 8000, 16000, 24000, 32000, 44100 or 96000";
const char *const kOutRates = "denoised_rate must be 8000, 16000, 24000, 32000, 44100 or 96000";

// fvad_resample_taps / fvad_resample_out_taps
size_t taps_of(int rate, Dir dir, const char *rates, float *out, size_t cap) {
  fvad::rs::Desc d;
  if (!fvad::rs::describe(rate, dir, d)) {
    fvad::set_error(FVAD_ERATE, rates);
    return 0;
  }
  const std::vector<float> &t = fvad::resample_table(dir, d);
  if (out) std::memcpy(out, t.data(), sizeof(float) * (t.size() < cap ? t.size() : cap));
  return t.size();
}

// fvad_resample_host / fvad_resample_out_host, the mirrors of k_resample and
// k_resample_out: one row tick by tick, n_src samples in and n_dst out a tick
// (d.n and 480, or 480 and d.n)
int mirror(int rate, Dir dir, const char *rates, const float *in, size_t n_ticks, float *tail, float *out) {
  fvad::rs::Desc d;
  if (!fvad::rs::describe(rate, dir, d)) return fvad::set_error(FVAD_ERATE, rates);
  if (n_ticks == 0) return FVAD_OK;
  if (!in || !out) return fvad::set_error(FVAD_EINVAL, "null argument");
  const float *taps = fvad::resample_table(dir, d).data();
  const int hist = d.K - 1, n_src = dir == Dir::kIn ? d.n : fvad::rs::kIn, n_dst = dir == Dir::kIn ? fvad::rs::kOut : d.n;
  // [the K - 1 samples before the tick | the tick]
  std::vector<float> x((size_t)hist + n_src, 0.0f);
  if (tail) std::memcpy(x.data(), tail, sizeof(float) * hist);
  for (size_t t = 0; t < n_ticks; t++) {
    std::memcpy(x.data() + hist, in + t * n_src, sizeof(float) * n_src);
    for (int r = 0; r < n_dst; r++) {
      int i, p;
      fvad::rs::position(r, d.L, d.M, i, p);
      float acc[1];
      fvad::rs::accumulate<1>(
          d.K, [&](int k) { return taps[(size_t)p * d.K + k]; }, [&](int, int k) { return x[(size_t)hist + i - k]; }, acc);
      out[t * n_dst + r] = acc[0];
    }
    std::memmove(x.data(), x.data() + n_src, sizeof(float) * hist);
  }
  if (tail) std::memcpy(tail, x.data(), sizeof(float) * hist);
  return FVAD_OK;
}
}  // namespace

extern "C" int fvad_resample_info(int input_rate, fvad_resample_desc *out) {
  if (!out) return fvad::set_error(FVAD_EINVAL, "null argument");
  fvad::rs::Desc d;
  if (!fvad::rs::describe(input_rate, Dir::kIn, d)) return fvad::set_error(FVAD_ERATE, kInRates);
  out->input_rate = d.rate;
  out->L = d.L;
  out->M = d.M;
  out->taps_per_phase = d.K;
  out->frame_in = d.n;
  out->delay = ((double)d.L * d.K - 1.0) / (2.0 * d.M);
  return FVAD_OK;
}

extern "C" size_t fvad_resample_taps(int input_rate, float *out, size_t cap) {
  return taps_of(input_rate, Dir::kIn, kInRates, out, cap);
}

extern "C" int fvad_resample_host(int input_rate, const float *in, size_t n_ticks, float *tail, float *out) {
  return mirror(input_rate, Dir::kIn, kInRates, in, n_ticks, tail, out);
}

// The decimating direction: 48 kHz to denoised_rate (include/fvad.h section 2d)
extern "C" int fvad_resample_out_info(int rate, fvad_resample_out_desc *out) {
  if (!out) return fvad::set_error(FVAD_EINVAL, "null argument");
  fvad::rs::Desc d;
  if (!fvad::rs::describe(rate, Dir::kOut, d)) return fvad::set_error(FVAD_ERATE, kOutRates);
  out->rate = d.rate;
  out->L = d.L;
  out->M = d.M;
  out->taps_per_phase = d.K;
  out->frame_out = d.n;
  out->delay = ((double)d.L * d.K - 1.0) / (2.0 * d.L);
  return FVAD_OK;
}

extern "C" size_t fvad_resample_out_taps(int rate, float *out, size_t cap) {
  return taps_of(rate, Dir::kOut, kOutRates, out, cap);
}

extern "C" int fvad_resample_out_host(int rate, const float *in48, size_t n_ticks, float *tail, float *out) {
  return mirror(rate, Dir::kOut, kOutRates, in48, n_ticks, tail, out);
}
