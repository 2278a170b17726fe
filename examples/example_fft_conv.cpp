// example_fft_conv.cpp — FFT convolution through the C ABI of the add-on (include/tfft_conv.h): what example_spectral_filter.cpp
// writes by hand (two plans, a pointwise kernel that knows the transposed index map, the scale bookkeeping, a spectrum buffer) as
// ONE plan. At N = 4096 it is one kernel and one pass over HBM.
//
// The layout is depthwise: signal b = [sample][channel] takes the filter of channel b mod channels. Here every channel's filter is
// a circular delay, exp(-2 pi i k shift_c / N) on bin k with a DIFFERENT shift per channel, so the result must be each input
// rolled by its channel's shift, which the program checks (a wrong filter index or bin map is a wrong roll). exit 0 / 1.
//
// usage: example_fft_conv [log2_N = 12] [batch = 64] [channels = 4] [composed = 0]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfft_conv.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_CONV(c)                                                        \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, tfft_conv_last_error());                   \
      return 1;                                                              \
    }                                                                        \
  } while (0)

int main(int argc, char** argv) {
  const int lg = argc > 1 ? std::atoi(argv[1]) : 12;
  const unsigned batch = argc > 2 ? static_cast<unsigned>(std::atoi(argv[2])) : 64;
  const unsigned channels = argc > 3 ? static_cast<unsigned>(std::atoi(argv[3])) : 4;
  const int flags = (argc > 4 && std::atoi(argv[4])) ? TFFT_CONV_COMPOSED : 0;
  const unsigned long long n = 1ull << lg;
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));

  char text[512];
  CHECK_CONV(tfft_conv_describe(n, batch, channels, flags, text, sizeof(text)));
  tfft_conv_plan* plan = nullptr;
  CHECK_CONV(tfft_conv_plan_create(n, batch, channels, dev, 0, 0, flags, &plan));
  CHECK_CONV(tfft_conv_plan_prepare(plan));
  std::printf("N = 2^%d, batch %u, %u channels: %s, %d launches, workspace %zu KiB\n", lg, batch, channels, text,
              tfft_conv_plan_num_launches(plan), tfft_conv_plan_workspace_bytes(plan) >> 10);

  // the filters: natural bin order, unscaled, two planes of channels * n halves
  auto shift_of = [&](unsigned c) { return (5ull + 37ull * c) % n; };
  std::vector<__half> h_re(channels * n), h_im(channels * n);
  for (unsigned c = 0; c < channels; ++c)
    for (unsigned long long k = 0; k < n; ++k) {
      const double a = -2.0 * M_PI * static_cast<double>((k * shift_of(c)) % n) / static_cast<double>(n);
      h_re[c * n + k] = __float2half(static_cast<float>(std::cos(a)));
      h_im[c * n + k] = __float2half(static_cast<float>(std::sin(a)));
    }
  __half *d_hre = nullptr, *d_him = nullptr;
  CHECK_HIP(hipMalloc(&d_hre, h_re.size() * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_him, h_im.size() * sizeof(__half)));
  CHECK_HIP(hipMemcpy(d_hre, h_re.data(), h_re.size() * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(d_him, h_im.data(), h_im.size() * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_CONV(tfft_conv_plan_set_filter(plan, d_hre, d_him, nullptr));
  (void)hipFree(d_hre);      // the plan holds its own image
  (void)hipFree(d_him);

  const size_t halves = static_cast<size_t>(batch) * 2 * n;       // [RE | IM] block per signal
  std::vector<__half> host(halves), back(halves);
  unsigned s = 2463534242u;
  for (size_t i = 0; i < halves; ++i) {
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    host[i] = __float2half(static_cast<float>(s >> 8) / 8388608.0f - 1.0f);
  }
  __half *x = nullptr, *y = nullptr;
  CHECK_HIP(hipMalloc(&x, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&y, halves * sizeof(__half)));
  CHECK_HIP(hipMemcpy(x, host.data(), halves * sizeof(__half), hipMemcpyHostToDevice));

  hipEvent_t e0, e1;
  CHECK_HIP(hipEventCreate(&e0));
  CHECK_HIP(hipEventCreate(&e1));
  const int reps = 5;
  for (int r = -1; r < reps; ++r) {            // one untimed round first
    if (r == 0) CHECK_HIP(hipEventRecord(e0, nullptr));
    CHECK_CONV(tfft_conv_exec(plan, x, x + n, y, y + n, nullptr));
  }
  CHECK_HIP(hipEventRecord(e1, nullptr));
  CHECK_HIP(hipEventSynchronize(e1));
  float ms = 0;
  CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
  ms /= reps;
  CHECK_HIP(hipMemcpy(back.data(), y, halves * sizeof(__half), hipMemcpyDeviceToHost));

  // y_b[t] = x_b[t - shift of channel b mod channels], both planes
  double worst = 0;
  for (unsigned b = 0; b < batch; ++b) {
    const unsigned long long shift = shift_of(b % channels);
    double err2 = 0, ref2 = 0;
    for (int plane = 0; plane < 2; ++plane) {
      const __half* in = host.data() + (static_cast<size_t>(b) * 2 + plane) * n;
      const __half* out = back.data() + (static_cast<size_t>(b) * 2 + plane) * n;
      for (unsigned long long t = 0; t < n; ++t) {
        const double want = __half2float(in[(t + n - shift) % n]), got = __half2float(out[t]);
        err2 += (got - want) * (got - want);
        ref2 += want * want;
      }
    }
    worst = std::fmax(worst, std::sqrt(err2 / ref2));
  }
  std::printf("%.3f ms per batch = %.1f Gsamples/s through forward, filter and inverse; worst rel-L2 error of a rolled signal %.2e\n", ms,
              static_cast<double>(n) * batch / ms / 1e6, worst);
  tfft_conv_plan_destroy(plan);
  (void)hipFree(x);
  (void)hipFree(y);
  const bool ok = worst < 3e-3;        // two transforms, the rounding of the filtered spectrum and of the binary16 filter itself
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
