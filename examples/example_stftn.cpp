// example_stftn.cpp — a spectrogram through the C ABI of the short-frame STFT add-on (include/tfft_stftn.h): frames of 1024 samples,
// hop 256, of one long real signal, each multiplied by a Hann window and transformed to bins 0 .. 512, in one kernel. The framing,
// the window multiply, the pairing of two frames into one complex transform and the split into half spectra are the plan's business.
//
// The signal holds two tones; the second, stronger one starts halfway. The peak bin of every frame is printed (the second tone
// takes over where the frames reach it), and three frames are compared with a host fp64 DFT / 1024 of the same binary16 products
// w[j] * x[j]. exit 0 / 1.
//
// usage: example_stftn [frames = 16]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfft_stftn.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_STFTN(c)                                                        \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, tfft_stftn_last_error());                   \
      return 1;                                                              \
    }                                                                        \
  } while (0)

int main(int argc, char** argv) {
  const unsigned long long want_frames = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 16;
  const unsigned long long n = 1024, hop = 256, bins = n / 2 + 1, pitch = (bins + 7) / 8 * 8;      // pitch: tfft_rplan_spectrum_pitch(n) = 520
  if (want_frames < 3 || want_frames > 4096) {
    std::printf("frames must be 3 .. 4096\n");
    return 1;
  }
  const unsigned long long L = n + (want_frames - 1) * hop;
  const int tone_a = 50, tone_b = 225;           // in bins of the frame length
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));

  char text[128];
  uint64_t frames = 0;
  CHECK_STFTN(tfft_stftn_geometry(n, L, hop, 0, &frames));
  CHECK_STFTN(tfft_stftn_describe(n, L, hop, 0, 1, 0, text, sizeof(text)));
  tfft_stftn_plan* plan = nullptr;
  CHECK_STFTN(tfft_stftn_plan_create(n, 1, L, hop, 0, dev, nullptr, &plan));
  std::printf("L = %llu, hop = %llu: %llu frames: %s, %d launch\n", L, hop, static_cast<unsigned long long>(frames), text,
              tfft_stftn_plan_num_launches(plan));

  std::vector<__half> sig(L), win(n);
  for (unsigned long long t = 0; t < L; ++t) {
    double v = 0.3 * std::cos(2.0 * M_PI * tone_a * static_cast<double>(t) / static_cast<double>(n));
    if (t >= L / 2) v += 0.6 * std::sin(2.0 * M_PI * tone_b * static_cast<double>(t) / static_cast<double>(n));
    sig[t] = __float2half(static_cast<float>(v));
  }
  for (unsigned long long j = 0; j < n; ++j)     // the periodic Hann window
    win[j] = __float2half(static_cast<float>(0.5 - 0.5 * std::cos(2.0 * M_PI * static_cast<double>(j) / static_cast<double>(n))));

  __half *x = nullptr, *w = nullptr, *out = nullptr;
  const size_t out_halves = static_cast<size_t>(frames) * 2 * pitch;          // frame g: [RE 520 | IM 520]
  CHECK_HIP(hipMalloc(&x, L * sizeof(__half)));
  CHECK_HIP(hipMalloc(&w, n * sizeof(__half)));
  CHECK_HIP(hipMalloc(&out, out_halves * sizeof(__half)));
  CHECK_HIP(hipMemcpy(x, sig.data(), L * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(w, win.data(), n * sizeof(__half), hipMemcpyHostToDevice));

  // an execution without a window is refused, and says why
  const bool refused = tfft_stftn_exec(plan, x, out, out + pitch, nullptr) == TFFT_ERR_ARG;
  std::printf("before set_window: %s\n", refused ? tfft_stftn_last_error() : "NOT refused");
  CHECK_STFTN(tfft_stftn_plan_set_window(plan, w, nullptr));
  CHECK_STFTN(tfft_stftn_exec(plan, x, out, out + pitch, nullptr));
  CHECK_HIP(hipDeviceSynchronize());
  (void)hipFree(w);           // the plan holds its own copy
  std::vector<__half> back(out_halves);
  CHECK_HIP(hipMemcpy(back.data(), out, out_halves * sizeof(__half), hipMemcpyDeviceToHost));

  bool peaks_ok = true;
  std::printf("peak bin per frame:");
  for (unsigned long long f = 0; f < frames; ++f) {
    const __half* re = back.data() + f * 2 * pitch;
    const __half* im = re + pitch;
    unsigned long long peak = 0;
    double best = -1;
    for (unsigned long long k = 0; k < bins; ++k) {
      const double p = static_cast<double>(__half2float(re[k])) * __half2float(re[k]) + static_cast<double>(__half2float(im[k])) * __half2float(im[k]);
      if (p > best) {
        best = p;
        peak = k;
      }
    }
    std::printf(" %llu", peak);
    if (peak != static_cast<unsigned long long>(tone_a) && peak != static_cast<unsigned long long>(tone_b)) peaks_ok = false;
    if (f == 0 && peak != static_cast<unsigned long long>(tone_a)) peaks_ok = false;       // the second tone has not started yet
    if (f == frames - 1 && peak != static_cast<unsigned long long>(tone_b)) peaks_ok = false;   // ... and is the stronger one once it has
  }
  std::printf("\n");

  // the definition, in fp64, on the first, a middle and the last frame: DFT / 1024 of the binary16 products (a product of two
  // binary16 values is exact in fp32, so the conversion back is the one rounding)
  double worst = 0;
  const unsigned long long picks[3] = {0, frames / 2, frames - 1};
  std::vector<double> u(n), cs(n), sn(n);
  for (unsigned long long j = 0; j < n; ++j) {
    cs[j] = std::cos(2.0 * M_PI * static_cast<double>(j) / static_cast<double>(n));
    sn[j] = std::sin(2.0 * M_PI * static_cast<double>(j) / static_cast<double>(n));
  }
  for (unsigned long long f : picks) {
    for (unsigned long long j = 0; j < n; ++j) u[j] = __half2float(__float2half(__half2float(win[j]) * __half2float(sig[f * hop + j])));
    const __half* re = back.data() + f * 2 * pitch;
    const __half* im = re + pitch;
    double err2 = 0, ref2 = 0;
    for (unsigned long long k = 0; k < bins; ++k) {
      double wr = 0, wi = 0;
      for (unsigned long long j = 0; j < n; ++j) {
        const unsigned long long a = (j * k) & (n - 1);
        wr += u[j] * cs[a];
        wi -= u[j] * sn[a];
      }
      wr /= static_cast<double>(n);
      wi /= static_cast<double>(n);
      const double dr = __half2float(re[k]) - wr, di = __half2float(im[k]) - wi;
      err2 += dr * dr + di * di;
      ref2 += wr * wr + wi * wi;
    }
    worst = std::fmax(worst, std::sqrt(err2 / ref2));
  }
  std::printf("worst rel-L2 error of a checked frame against fp64: %.2e\n", worst);
  tfft_stftn_plan_destroy(plan);
  (void)hipFree(x);
  (void)hipFree(out);
  const bool ok = worst <= 1.5e-3 && peaks_ok && refused;      // the bound of the real-input transforms
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
