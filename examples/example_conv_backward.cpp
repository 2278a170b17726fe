// example_conv_backward.cpp — the two gradients of the causal depthwise convolution of long real sequences through the C ABI of the
// gradient add-on (include/tfft_bconv.h). With y[b][c][t] = sum over j <= t, j < K of h[c][j] x[b][c][t - j] and g = d loss / d y:
//
//     dx[b][c][t] = sum over j < K, t + j < L of h[c][j] g[b][c][t + j]            tfft_bconv_exec_input_grad (binary16)
//     dh[c][j]    = sum over b and t >= j     of g[b][c][t] x[b][c][t - j]         tfft_bconv_exec_tap_grad   (fp32)
//
// One plan serves both. The input gradient needs the taps (set_taps) and no workspace; the tap gradient needs no taps and a workspace
// for its partial sums, allocated here by tfft_bconv_plan_prepare so that the executions only launch kernels.
//
// Both results are checked against the same sums in fp64 on the host (dx on a sample of the sequences). exit 0 / 1.
//
// usage: example_conv_backward [L = 16384] [K = 2049] [rows = 9] [channels = 4]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfft_bconv.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_BCONV(c)                                                       \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, tfft_bconv_last_error());                  \
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
  uint64_t halo = 0, hop = 0, segments = 0, partials = 0;
  CHECK_BCONV(tfft_bconv_geometry(L, K, rows, channels, 0, &halo, &hop, &segments, &partials));
  CHECK_BCONV(tfft_bconv_describe(L, K, rows, channels, 0, 0, text, sizeof(text)));
  tfft_bconv_plan* plan = nullptr;
  CHECK_BCONV(tfft_bconv_plan_create(rows, channels, L, K, dev, nullptr, &plan));
  CHECK_BCONV(tfft_bconv_plan_prepare(plan));
  std::printf("L = %llu, K = %llu, %u x %u sequences: halo %llu, hop %llu, %llu segments, %llu partial sums per channel: %s, workspace %zu bytes\n", L, K,
              rows, channels, static_cast<unsigned long long>(halo), static_cast<unsigned long long>(hop), static_cast<unsigned long long>(segments),
              static_cast<unsigned long long>(partials), text, tfft_bconv_plan_workspace_bytes(plan));

  unsigned s = 2463534242u;
  auto uniform = [&]() {
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    return static_cast<float>(s >> 8) / 8388608.0f - 1.0f;
  };
  // the taps: an exponentially decaying random kernel per channel, normalised to sum |h| = 1
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

  const size_t halves = static_cast<size_t>(rows) * channels * L;
  std::vector<__half> hx(halves), hg(halves), hdx(halves);
  for (size_t i = 0; i < halves; ++i) hx[i] = __float2half(uniform());
  for (size_t i = 0; i < halves; ++i) hg[i] = __float2half(uniform());
  std::vector<float> hdh(static_cast<size_t>(channels) * K);
  __half *x = nullptr, *g = nullptr, *dx = nullptr;
  float* dh = nullptr;
  CHECK_HIP(hipMalloc(&x, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&g, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&dx, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&dh, hdh.size() * sizeof(float)));
  CHECK_HIP(hipMemcpy(x, hx.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(g, hg.data(), halves * sizeof(__half), hipMemcpyHostToDevice));

  // the tap gradient works before any set_taps; the input gradient does not, and says so
  CHECK_BCONV(tfft_bconv_exec_tap_grad(plan, x, g, dh, nullptr));
  const bool needs_taps = tfft_bconv_exec_input_grad(plan, g, dx, nullptr) == TFFT_ERR_ARG;
  std::printf("input gradient before set_taps: %s\n", needs_taps ? tfft_bconv_last_error() : "NOT refused");
  CHECK_BCONV(tfft_bconv_plan_set_taps(plan, d_taps, nullptr));
  (void)hipFree(d_taps);      // the plan holds its own spectrum
  CHECK_BCONV(tfft_bconv_exec_input_grad(plan, g, dx, nullptr));
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(hdx.data(), dx, halves * sizeof(__half), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hdh.data(), dh, hdh.size() * sizeof(float), hipMemcpyDeviceToHost));

  // dx: the definition, in fp64, on the first, a middle and the last row of every channel
  double worst_dx = 0;
  const unsigned picks[3] = {0, rows / 2, rows - 1};
  for (unsigned c = 0; c < channels; ++c)
    for (unsigned b : picks) {
      const __half* in = hg.data() + (static_cast<size_t>(b) * channels + c) * L;
      const __half* out = hdx.data() + (static_cast<size_t>(b) * channels + c) * L;
      double err2 = 0, ref2 = 0;
      for (unsigned long long t = 0; t < L; ++t) {
        double want = 0;
        for (unsigned long long j = 0; j < K && t + j < L; ++j) want += static_cast<double>(__half2float(taps[c * K + j])) * __half2float(in[t + j]);
        const double got = __half2float(out[t]);
        err2 += (got - want) * (got - want);
        ref2 += want * want;
      }
      worst_dx = std::fmax(worst_dx, std::sqrt(err2 / ref2));
    }
  // dh: every tap of every channel
  double worst_dh = 0;
  for (unsigned c = 0; c < channels; ++c) {
    double err2 = 0, ref2 = 0;
    for (unsigned long long j = 0; j < K; ++j) {
      double want = 0;
      for (unsigned b = 0; b < rows; ++b) {
        const __half* px = hx.data() + (static_cast<size_t>(b) * channels + c) * L;
        const __half* pg = hg.data() + (static_cast<size_t>(b) * channels + c) * L;
        for (unsigned long long t = j; t < L; ++t) want += static_cast<double>(__half2float(pg[t])) * __half2float(px[t - j]);
      }
      const double got = hdh[c * K + j];
      err2 += (got - want) * (got - want);
      ref2 += want * want;
    }
    worst_dh = std::fmax(worst_dh, std::sqrt(err2 / ref2));
  }
  std::printf("worst rel-L2 error: dx %.2e (of a checked sequence), dh %.2e (of a channel)\n", worst_dx, worst_dh);
  // in-place execution of the input gradient is refused, and says why
  const bool refused = tfft_bconv_exec_input_grad(plan, g, g, nullptr) == TFFT_ERR_ARG;
  std::printf("in place: %s\n", refused ? tfft_bconv_last_error() : "NOT refused");
  tfft_bconv_plan_destroy(plan);
  (void)hipFree(x);
  (void)hipFree(g);
  (void)hipFree(dx);
  (void)hipFree(dh);
  // dx: two transforms and the binary16 spectrum, as the forward pass. dh: white noise against white noise, so every tap is a sum
  // of about rows * L products that largely cancel, while every item's rounding is relative to its peak: a few 1e-3 of the rms tap
  const bool ok = worst_dx < 3e-3 && worst_dh < 1e-2 && refused && needs_taps;
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
