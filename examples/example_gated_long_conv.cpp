// example_gated_long_conv.cpp — the gated causal convolution of sequence-model operators (H3, Hyena) at LONG sequence lengths through
// the C ABI of the add-on (include/tfft_gsconv.h):
//
//     u = p * x        y[b][c][t] = g[b][c][t] * ( sum over j <= t, j < K of h[c][j] u[b][c][t - j]  +  d[c] u[b][c][t] )
//
// One plan, one kernel per execution at any L (overlap-save at transform length 4096, K <= 2049). The skip weight d costs nothing
// on the device: the plan adds it to tap 0 when it builds the filter spectrum. The output may not overlap the input or a gate; the
// example shows the refusal.
//
// The result is checked against the same sum in fp64 on the host (u rounded to binary16 as the plan rounds it), on a sample of the
// sequences. exit 0 / 1.
//
// usage: example_gated_long_conv [L = 8192] [K = 2049] [rows = 5] [channels = 2]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfft_gsconv.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_GSCONV(c)                                                      \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, tfft_gsconv_last_error());                 \
      return 1;                                                              \
    }                                                                        \
  } while (0)

int main(int argc, char** argv) {
  const unsigned long long L = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 8192;
  const unsigned long long K = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 2049;
  const unsigned rows = argc > 3 ? static_cast<unsigned>(std::atoi(argv[3])) : 5;
  const unsigned channels = argc > 4 ? static_cast<unsigned>(std::atoi(argv[4])) : 2;
  tfft_gsconv_opts opts = TFFT_GSCONV_OPTS_INIT;
  opts.flags = TFFT_GSCONV_PRE_GATE | TFFT_GSCONV_POST_GATE;
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));

  char text[128];
  uint64_t halo = 0, hop = 0, segments = 0;
  CHECK_GSCONV(tfft_gsconv_describe(L, K, rows, channels, opts.flags, text, sizeof(text)));
  CHECK_GSCONV(tfft_gsconv_geometry(L, K, &halo, &hop, &segments));
  tfft_gsconv_plan* plan = nullptr;
  CHECK_GSCONV(tfft_gsconv_plan_create(rows, channels, L, K, dev, &opts, &plan));
  std::printf("L = %llu, K = %llu, %u x %u sequences: %s (halo %llu, hop %llu), %d launch\n", L, K, rows, channels, text,
              static_cast<unsigned long long>(halo), static_cast<unsigned long long>(hop), tfft_gsconv_plan_num_launches(plan));

  unsigned s = 2463534242u;
  auto uniform = [&]() {
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    return static_cast<float>(s >> 8) / 8388608.0f - 1.0f;
  };
  // the taps: an exponentially decaying random kernel per channel, normalised to sum |h| = 1/2; the skip weights +-1/2, +-3/8, ...:
  // |z| <= 1
  std::vector<__half> taps(static_cast<size_t>(channels) * K), skip(channels);
  for (unsigned c = 0; c < channels; ++c) {
    std::vector<double> h(K);
    double sum = 0;
    for (unsigned long long j = 0; j < K; ++j) {
      h[j] = uniform() * std::exp(-static_cast<double>(j) * (4.0 + c) / static_cast<double>(K));
      sum += std::fabs(h[j]);
    }
    for (unsigned long long j = 0; j < K; ++j) taps[c * K + j] = __float2half(static_cast<float>(0.5 * h[j] / sum));
    skip[c] = __float2half((0.5f - 0.125f * (c % 4)) * ((c & 1) ? -1.0f : 1.0f));
  }
  __half *d_taps = nullptr, *d_skip = nullptr;
  CHECK_HIP(hipMalloc(&d_taps, taps.size() * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_skip, skip.size() * sizeof(__half)));
  CHECK_HIP(hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(d_skip, skip.data(), skip.size() * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_GSCONV(tfft_gsconv_plan_set_taps(plan, d_taps, d_skip, nullptr));
  (void)hipFree(d_taps);      // the plan holds its own spectrum
  (void)hipFree(d_skip);

  const size_t halves = static_cast<size_t>(rows) * channels * L;
  std::vector<__half> host(halves), pre(halves), post(halves), back(halves);
  for (size_t i = 0; i < halves; ++i) host[i] = __float2half(uniform());
  for (size_t i = 0; i < halves; ++i) pre[i] = __float2half(uniform());
  for (size_t i = 0; i < halves; ++i) post[i] = __float2half(uniform());
  __half *x = nullptr, *p = nullptr, *g = nullptr, *y = nullptr;
  CHECK_HIP(hipMalloc(&x, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&p, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&g, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&y, halves * sizeof(__half)));
  CHECK_HIP(hipMemcpy(x, host.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(p, pre.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(g, post.data(), halves * sizeof(__half), hipMemcpyHostToDevice));

  // an overlap-save plan cannot run in place, and a gate cannot be the output: both are refused before anything is launched
  const int in_place = tfft_gsconv_exec(plan, x, p, g, x, nullptr);
  std::printf("in place: %s\n", in_place == TFFT_OK ? "accepted (unexpected)" : tfft_gsconv_last_error());
  if (in_place == TFFT_OK) return 1;

  hipEvent_t e0, e1;
  CHECK_HIP(hipEventCreate(&e0));
  CHECK_HIP(hipEventCreate(&e1));
  const int reps = 5;
  for (int r = -1; r < reps; ++r) {            // one untimed round first
    if (r == 0) CHECK_HIP(hipEventRecord(e0, nullptr));
    CHECK_GSCONV(tfft_gsconv_exec(plan, x, p, g, y, nullptr));
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
  std::vector<double> u(L);
  for (unsigned c = 0; c < channels; ++c)
    for (unsigned b : picks) {
      const size_t at = (static_cast<size_t>(b) * channels + c) * L;
      for (unsigned long long t = 0; t < L; ++t) u[t] = __half2float(__float2half(__half2float(pre[at + t]) * __half2float(host[at + t])));
      double err2 = 0, ref2 = 0;
      for (unsigned long long t = 0; t < L; ++t) {
        double z = static_cast<double>(__half2float(skip[c])) * u[t];
        for (unsigned long long j = 0; j <= t && j < K; ++j) z += static_cast<double>(__half2float(taps[c * K + j])) * u[t - j];
        const double want = static_cast<double>(__half2float(post[at + t])) * z;
        const double got = __half2float(back[at + t]);
        err2 += (got - want) * (got - want);
        ref2 += want * want;
      }
      worst = std::fmax(worst, std::sqrt(err2 / ref2));
    }
  std::printf("%.3f ms per execution = %.1f Gsamples/s of real input; worst rel-L2 error of a checked sequence %.2e\n", ms,
              static_cast<double>(halves) / ms / 1e6, worst);
  tfft_gsconv_plan_destroy(plan);
  (void)hipFree(x);
  (void)hipFree(p);
  (void)hipFree(g);
  (void)hipFree(y);
  const bool ok = worst < 3e-3;        // example_gated_conv's bound: two transforms and the roundings of the spectra; the gates add one each
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
