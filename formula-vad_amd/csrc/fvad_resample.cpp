// Input resampling to 48 kHz, host side: the tap design (f64, once per rate)
// and fvad_resample_host, the mirror of k_resample the tests hold the kernel
// to (fvad_resample_core.h is the arithmetic they share); and the same for the
// decimating direction (denoised_rate): fvad_resample_out_host mirrors
// k_resample_out.  No GPU.
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/fvad.h"
#include "fvad_hip_own.h"  // fvad::set_error
#include "fvad_resample.h"
#include "fvad_resample_out.h"
#include "fvad_resample_core.h"

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

// the [L][K] table of a listed rate, designed on first use and kept
const std::vector<float> &fvad::resample_table(const rs::Desc &d) {
  static std::vector<float> tables[rs::kRates];
  static std::once_flag once[rs::kRates];
  const int i = rate_slot(d.rate);
  std::call_once(once[i], [&] { design(d.L, d.K, d.rate, d.rate, tables[i]); });
  return tables[i];
}

// the decimating direction's [L][K] table (48 kHz to d.rate), likewise
const std::vector<float> &fvad::resample_out_table(const rs::DescOut &d) {
  static std::vector<float> tables[rs::kRates];
  static std::once_flag once[rs::kRates];
  const int i = rate_slot(d.rate);
  std::call_once(once[i], [&] { design(d.L, d.K, 48000, d.rate, tables[i]); });
  return tables[i];
}

extern "C" int fvad_resample_info(int input_rate, fvad_resample_desc *out) {
  if (!out) return fvad::set_error(FVAD_EINVAL, "null argument");
  fvad::rs::Desc d;
  if (!fvad::rs::describe(input_rate, d))
    return fvad::set_error(FVAD_ERATE, "input_rate must be 8000, 16000, 24000, 32000, 44100 or 96000");
  out->input_rate = d.rate;
  out->L = d.L;
  out->M = d.M;
  out->taps_per_phase = d.K;
  out->frame_in = d.n_in;
  out->delay = ((double)d.L * d.K - 1.0) / (2.0 * d.M);
  return FVAD_OK;
}

extern "C" size_t fvad_resample_taps(int input_rate, float *out, size_t cap) {
  fvad::rs::Desc d;
  if (!fvad::rs::describe(input_rate, d)) {
    fvad::set_error(FVAD_ERATE, "input_rate must be 8000, 16000, 24000, 32000, 44100 or 96000");
    return 0;
  }
  const std::vector<float> &t = fvad::resample_table(d);
  if (out) std::memcpy(out, t.data(), sizeof(float) * (t.size() < cap ? t.size() : cap));
  return t.size();
}

extern "C" int fvad_resample_host(int input_rate, const float *in, size_t n_ticks, float *tail, float *out) {
  fvad::rs::Desc d;
  if (!fvad::rs::describe(input_rate, d))
    return fvad::set_error(FVAD_ERATE, "input_rate must be 8000, 16000, 24000, 32000, 44100 or 96000");
  if (n_ticks == 0) return FVAD_OK;
  if (!in || !out) return fvad::set_error(FVAD_EINVAL, "null argument");
  const float *taps = fvad::resample_table(d).data();
  const int hist = d.K - 1;
  // [the K - 1 samples before the tick | the tick]
  std::vector<float> x((size_t)hist + d.n_in, 0.0f);
  if (tail) std::memcpy(x.data(), tail, sizeof(float) * hist);
  for (size_t t = 0; t < n_ticks; t++) {
    std::memcpy(x.data() + hist, in + t * d.n_in, sizeof(float) * d.n_in);
    for (int r = 0; r < fvad::rs::kOut; r++) {
      int i, p;
      fvad::rs::position(r, d.L, d.M, i, p);
      float acc[1];
      fvad::rs::accumulate<1>(
          d.K, [&](int k) { return taps[(size_t)p * d.K + k]; }, [&](int, int k) { return x[(size_t)hist + i - k]; }, acc);
      out[t * fvad::rs::kOut + r] = acc[0];
    }
    std::memmove(x.data(), x.data() + d.n_in, sizeof(float) * hist);
  }
  if (tail) std::memcpy(tail, x.data(), sizeof(float) * hist);
  return FVAD_OK;
}

// ---------------------------------------------------------------------------
// The decimating direction: 48 kHz to denoised_rate (include/fvad.h section 2d)
// ---------------------------------------------------------------------------
namespace {
const char *const kOutRates = "denoised_rate must be 8000, 16000, 24000, 32000, 44100 or 96000";
}

extern "C" int fvad_resample_out_info(int rate, fvad_resample_out_desc *out) {
  if (!out) return fvad::set_error(FVAD_EINVAL, "null argument");
  fvad::rs::DescOut d;
  if (!fvad::rs::describe_out(rate, d)) return fvad::set_error(FVAD_ERATE, kOutRates);
  out->rate = d.rate;
  out->L = d.L;
  out->M = d.M;
  out->taps_per_phase = d.K;
  out->frame_out = d.n_out;
  out->delay = ((double)d.L * d.K - 1.0) / (2.0 * d.L);
  return FVAD_OK;
}

extern "C" size_t fvad_resample_out_taps(int rate, float *out, size_t cap) {
  fvad::rs::DescOut d;
  if (!fvad::rs::describe_out(rate, d)) {
    fvad::set_error(FVAD_ERATE, kOutRates);
    return 0;
  }
  const std::vector<float> &t = fvad::resample_out_table(d);
  if (out) std::memcpy(out, t.data(), sizeof(float) * (t.size() < cap ? t.size() : cap));
  return t.size();
}

extern "C" int fvad_resample_out_host(int rate, const float *in48, size_t n_ticks, float *tail, float *out) {
  fvad::rs::DescOut d;
  if (!fvad::rs::describe_out(rate, d)) return fvad::set_error(FVAD_ERATE, kOutRates);
  if (n_ticks == 0) return FVAD_OK;
  if (!in48 || !out) return fvad::set_error(FVAD_EINVAL, "null argument");
  const float *taps = fvad::resample_out_table(d).data();
  const int hist = d.K - 1;
  // [the K - 1 samples before the tick | the tick]
  std::vector<float> y((size_t)hist + fvad::rs::kIn, 0.0f);
  if (tail) std::memcpy(y.data(), tail, sizeof(float) * hist);
  for (size_t t = 0; t < n_ticks; t++) {
    std::memcpy(y.data() + hist, in48 + t * fvad::rs::kIn, sizeof(float) * fvad::rs::kIn);
    for (int r = 0; r < d.n_out; r++) {
      int i, p;
      fvad::rs::position(r, d.L, d.M, i, p);
      float acc[1];
      fvad::rs::accumulate<1>(
          d.K, [&](int k) { return taps[(size_t)p * d.K + k]; }, [&](int, int k) { return y[(size_t)hist + i - k]; }, acc);
      out[t * d.n_out + r] = acc[0];
    }
    std::memmove(y.data(), y.data() + fvad::rs::kIn, sizeof(float) * hist);
  }
  if (tail) std::memcpy(tail, y.data(), sizeof(float) * hist);
  return FVAD_OK;
}
