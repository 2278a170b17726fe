// example_long_conv.cpp — the causal depthwise convolution of LONG real sequences through the C ABI of the overlap-save add-on
// (include/tfft_sconv.h): y[b][c][t] = sum over j <= t, j < K of h[c][j] x[b][c][t - j], any L, K <= 2049, in one kernel. The plan
// cuts every sequence into segments of hop = 4096 - halo output samples and runs each, with the halo in front of it, through the
// 4096-point circular convolution; zero padding, the filter spectrum, the pairing of two real rows into one complex transform and
// the segment bookkeeping are the plan's business. Input and output must not overlap.
//
// The result is checked against the same sum in fp64 on the host, on a sample of the sequences. exit 0 / 1.
//
// usage: example_long_conv [L = 16384] [K = 2049] [rows = 9] [channels = 4]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfft_sconv.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_SCONV(c)                                                       \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, tfft_sconv_last_error());                  \
      return 1;                                                              \
    }                                                                        \
  } while (0)

int main(int argc, char** argv) {
  const unsigned long long L = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 16384;
  const unsigned long long K = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 2049;
  const unsigned rows = argc > 3 ? static_cast<unsigned>(std::atoi(argv[3])) : 9;
  const unsigned channels = argc > 4 ? static_cast<unsigned>(std::atoi(argv[4])) : 4;
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));

  char text[128];
  uint64_t halo = 0, hop = 0, segments = 0;
  CHECK_SCONV(tfft_sconv_geometry(L, K, &halo, &hop, &segments));
  CHECK_SCONV(tfft_sconv_describe(L, K, rows, channels, 0, text, sizeof(text)));
  tfft_sconv_plan* plan = nullptr;
  CHECK_SCONV(tfft_sconv_plan_create(rows, channels, L, K, dev, nullptr, &plan));
  std::printf("L = %llu, K = %llu, %u x %u sequences: halo %llu, hop %llu, %llu segments per sequence: %s, %d launch\n", L, K, rows, channels,
              static_cast<unsigned long long>(halo), static_cast<unsigned long long>(hop), static_cast<unsigned long long>(segments), text,
              tfft_sconv_plan_num_launches(plan));

  unsigned s = 2463534242u;
  auto uniform = [&]() {
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    return static_cast<float>(s >> 8) / 8388608.0f - 1.0f;
  };
  // the taps: an exponentially decaying random kernel per channel, normalised to sum |h| = 1 so that |y| <= 1
  std::vector<__half> taps(static_cast<size_t>(channels) * K);
  for (unsigned c = 0; c < channels; ++c) {
    std::vector<double> h(K);
    double sum = 0;
    for (unsigned long long j = 0; j < K; ++j) {
      h[j] = uniform() * std::exp(-static_cast<double>(j) * (4.0 + c) / static_cast<double>(K));
      sum += std::fabs(h[j]);
    }
    for (unsigned long long j = 0; j < K; ++j) taps[c * K + j] = __float2half(static_cast<float>(h[j] / sum));
  }
  __half* d_taps = nullptr;
  CHECK_HIP(hipMalloc(&d_taps, taps.size() * sizeof(__half)));
  CHECK_HIP(hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_SCONV(tfft_sconv_plan_set_taps(plan, d_taps, nullptr));
  (void)hipFree(d_taps);      // the plan holds its own spectrum

  const size_t halves = static_cast<size_t>(rows) * channels * L;
  std::vector<__half> host(halves), back(halves);
  for (size_t i = 0; i < halves; ++i) host[i] = __float2half(uniform());
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
    CHECK_SCONV(tfft_sconv_exec(plan, x, y, nullptr));
  }
  CHECK_HIP(hipEventRecord(e1, nullptr));
  CHECK_HIP(hipEventSynchronize(e1));
  float ms = 0;
  CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
  ms /= reps;
  CHECK_HIP(hipMemcpy(back.data(), y, halves * sizeof(__half), hipMemcpyDeviceToHost));

  // the definition, in fp64, on the first, a middle and the last row of every channel (the last row of an odd count has no partner)
  double worst = 0;
  const unsigned picks[3] = {0, rows / 2, rows - 1};
  for (unsigned c = 0; c < channels; ++c)
    for (unsigned b : picks) {
      const __half* in = host.data() + (static_cast<size_t>(b) * channels + c) * L;
      const __half* out = back.data() + (static_cast<size_t>(b) * channels + c) * L;
      double err2 = 0, ref2 = 0;
      for (unsigned long long t = 0; t < L; ++t) {
        double want = 0;
        for (unsigned long long j = 0; j <= t && j < K; ++j) want += static_cast<double>(__half2float(taps[c * K + j])) * __half2float(in[t - j]);
        const double got = __half2float(out[t]);
        err2 += (got - want) * (got - want);
        ref2 += want * want;
      }
      worst = std::fmax(worst, std::sqrt(err2 / ref2));
    }
  std::printf("%.3f ms per execution = %.1f Gsamples/s of real input; worst rel-L2 error of a checked sequence %.2e\n", ms,
              static_cast<double>(halves) / ms / 1e6, worst);
  // in-place execution is refused, and says why
  const bool refused = tfft_sconv_exec(plan, x, x, nullptr) == TFFT_ERR_ARG;
  std::printf("in place: %s\n", refused ? tfft_sconv_last_error() : "NOT refused");
  tfft_sconv_plan_destroy(plan);
  (void)hipFree(x);
  (void)hipFree(y);
  const bool ok = worst < 3e-3 && refused;        // two transforms, the rounding of the filtered spectrum and of the binary16 spectrum itself
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
