// example_spec.cpp — a mel spectrogram through the C ABI of the spectrogram add-on (include/tfft_spec.h): frames of 1024 samples,
// hop 256, of one real signal under a Hann window, each reduced to the energies of 40 triangular mel bands (HTK scale, 16 kHz), in
// one kernel. Neither the complex STFT nor the power spectrum reaches memory.
//
// The signal is a chirp that rises from 200 Hz to 6 kHz. The strongest band of every frame is printed (it never falls), and three
// frames are compared with a host fp64 restatement: the DFT / 1024 of the binary16 products w[j] * x[j], its squared magnitudes
// times the gain n^2, and the weighted sums. exit 0 / 1.
//
// usage: example_spec [frames = 16]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfft_spec.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_SPEC(c)                                                        \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, tfft_spec_last_error());                   \
      return 1;                                                              \
    }                                                                        \
  } while (0)

static double hz_to_mel(double f) { return 2595.0 * std::log10(1.0 + f / 700.0); }
static double mel_to_hz(double m) { return 700.0 * (std::pow(10.0, m / 2595.0) - 1.0); }

int main(int argc, char** argv) {
  const unsigned long long want_frames = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 16;
  const unsigned long long n = 1024, hop = 256, bins = n / 2 + 1;
  const uint32_t nbands = 40;
  const double rate = 16000.0;
  if (want_frames < 3 || want_frames > 4096) {
    std::printf("frames must be 3 .. 4096\n");
    return 1;
  }
  const unsigned long long L = n + (want_frames - 1) * hop;
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));

  // 40 triangles between 0 Hz and 8 kHz, equally spaced in mel: each band is its nonzero bins
  std::vector<double> edge(nbands + 2);
  for (uint32_t j = 0; j < nbands + 2; ++j) edge[j] = mel_to_hz(hz_to_mel(rate / 2) * j / (nbands + 1));
  std::vector<uint32_t> starts, counts;
  std::vector<float> weights;
  for (uint32_t j = 0; j < nbands; ++j) {
    uint32_t first = 0, last = 0;
    bool any = false;
    std::vector<float> row(bins);
    for (unsigned long long k = 0; k < bins; ++k) {
      const double f = k * rate / n;
      const double up = (f - edge[j]) / (edge[j + 1] - edge[j]), down = (edge[j + 2] - f) / (edge[j + 2] - edge[j + 1]);
      row[k] = static_cast<float>(std::fmax(0.0, std::fmin(up, down)));
      if (row[k] != 0.0f) {
        if (!any) first = static_cast<uint32_t>(k);
        last = static_cast<uint32_t>(k);
        any = true;
      }
    }
    if (!any) {
      std::printf("band %u is empty\n", j);
      return 1;
    }
    starts.push_back(first);
    counts.push_back(last - first + 1);
    weights.insert(weights.end(), row.begin() + first, row.begin() + last + 1);
  }

  char text[128];
  uint64_t frames = 0;
  CHECK_SPEC(tfft_spec_geometry(n, L, hop, 0, &frames));
  CHECK_SPEC(tfft_spec_describe(n, L, hop, 0, 1, 0, text, sizeof(text)));
  tfft_spec_opts opts = TFFT_SPEC_OPTS_INIT;
  opts.bands = nbands;
  opts.gain = static_cast<float>(n) * static_cast<float>(n);       // undoes the 1 / n of the transform: a power of two, rounds nothing
  tfft_spec_plan* plan = nullptr;
  CHECK_SPEC(tfft_spec_plan_create(n, 1, L, hop, 0, dev, &opts, &plan));
  std::printf("L = %llu, hop = %llu: %llu frames: %s, %u mel bands, %d launch\n", L, hop, static_cast<unsigned long long>(frames), text, nbands,
              tfft_spec_plan_num_launches(plan));

  std::vector<__half> sig(L), win(n);
  for (unsigned long long t = 0; t < L; ++t) {      // phase of a linear chirp 200 Hz -> 6 kHz over the signal
    const double s = static_cast<double>(t) / rate, T = static_cast<double>(L) / rate;
    sig[t] = __float2half(static_cast<float>(0.5 * std::sin(2.0 * M_PI * (200.0 * s + 0.5 * (6000.0 - 200.0) / T * s * s))));
  }
  for (unsigned long long j = 0; j < n; ++j)        // the periodic Hann window
    win[j] = __float2half(static_cast<float>(0.5 - 0.5 * std::cos(2.0 * M_PI * static_cast<double>(j) / static_cast<double>(n))));

  __half *x = nullptr, *w = nullptr;
  float* out = nullptr;
  const size_t out_floats = static_cast<size_t>(frames) * nbands;
  CHECK_HIP(hipMalloc(&x, L * sizeof(__half)));
  CHECK_HIP(hipMalloc(&w, n * sizeof(__half)));
  CHECK_HIP(hipMalloc(&out, out_floats * sizeof(float)));
  CHECK_HIP(hipMemcpy(x, sig.data(), L * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(w, win.data(), n * sizeof(__half), hipMemcpyHostToDevice));

  CHECK_SPEC(tfft_spec_plan_set_window(plan, w, nullptr));
  // an execution without bands is refused, and says why
  const bool refused = tfft_spec_exec(plan, x, out, nullptr) == TFFT_ERR_ARG;
  std::printf("before set_bands: %s\n", refused ? tfft_spec_last_error() : "NOT refused");
  CHECK_SPEC(tfft_spec_plan_set_bands(plan, nbands, starts.data(), counts.data(), weights.data(), nullptr));
  CHECK_SPEC(tfft_spec_exec(plan, x, out, nullptr));
  CHECK_HIP(hipDeviceSynchronize());
  (void)hipFree(w);           // the plan holds its own copy
  std::vector<float> back(out_floats);
  CHECK_HIP(hipMemcpy(back.data(), out, out_floats * sizeof(float), hipMemcpyDeviceToHost));

  bool rising = true;
  uint32_t before = 0;
  std::printf("strongest band per frame:");
  for (unsigned long long f = 0; f < frames; ++f) {
    uint32_t peak = 0;
    for (uint32_t j = 1; j < nbands; ++j)
      if (back[f * nbands + j] > back[f * nbands + peak]) peak = j;
    std::printf(" %u", peak);
    if (peak < before) rising = false;
    before = peak;
  }
  std::printf("\n");
  if (before == 0) rising = false;           // the chirp has left the first band by the last frame

  // the definition, in fp64, on the first, a middle and the last frame
  double worst = 0;
  const unsigned long long picks[3] = {0, frames / 2, frames - 1};
  std::vector<double> u(n), cs(n), sn(n), pw(bins);
  for (unsigned long long j = 0; j < n; ++j) {
    cs[j] = std::cos(2.0 * M_PI * static_cast<double>(j) / static_cast<double>(n));
    sn[j] = std::sin(2.0 * M_PI * static_cast<double>(j) / static_cast<double>(n));
  }
  for (unsigned long long f : picks) {
    for (unsigned long long j = 0; j < n; ++j) u[j] = __half2float(__float2half(__half2float(win[j]) * __half2float(sig[f * hop + j])));
    double total = 0;
    for (unsigned long long k = 0; k < bins; ++k) {
      double wr = 0, wi = 0;
      for (unsigned long long j = 0; j < n; ++j) {
        const unsigned long long a = (j * k) & (n - 1);
        wr += u[j] * cs[a];
        wi -= u[j] * sn[a];
      }
      pw[k] = wr * wr + wi * wi;           // (|DFT| / n)^2 * n^2
      total += pw[k];
    }
    double err = 0;
    size_t at = 0;
    for (uint32_t j = 0; j < nbands; ++j) {
      double e = 0;
      for (uint32_t c = 0; c < counts[j]; ++c) e += static_cast<double>(weights[at + c]) * pw[starts[j] + c];
      at += counts[j];
      err += std::fabs(back[f * nbands + j] - e);
    }
    worst = std::fmax(worst, err / total);
  }
  std::printf("worst sum of band errors of a checked frame against fp64, relative to the frame's power: %.2e\n", worst);
  tfft_spec_plan_destroy(plan);
  (void)hipFree(x);
  (void)hipFree(out);
  // the bound of the real-input transforms, eps = 1.5e-3 in rel-L2 of a half spectrum, is eps (2 + eps) on the sum of its powers, and
  // neighbouring triangles add up to at most 1 in every bin
  const bool ok = worst <= 1.5e-3 * (2 + 1.5e-3) + 1e-6 && rising && refused;
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
