// example_gated_conv_backward.cpp — the gradients of the gated causal depthwise convolution of long real sequences through the C ABI
// of the gated gradient add-on (include/tfft_gbconv.h). The forward operator is tfft_gsconv.h's, with both gates and a skip:
//
//     u = pre * x,   z[b][c][t] = sum over j <= t, j < K of h'[c][j] u[b][c][t - j],   y = post * z        h'[c][0] = h[c][0] + d[c]
//
// and with gy = d loss / d y and gz = post * gy:
//
//     du[b][c][t] = sum over j < K, t + j < L of h'[c][j] gz[b][c][t + j]
//     dx = pre * du,  dpre = x * du                                                   tfft_gbconv_exec_input_grad (binary16, one launch)
//     dh[c][j]    = sum over b and t >= j     of gz[b][c][t] u[b][c][t - j]           tfft_gbconv_exec_tap_grad   (fp32)
//     dskip[c]    = dh[c][0]                                                          (the same call)
//
// One plan serves both. The input gradient needs the taps and the skip (set_taps) and no workspace; the tap gradient needs neither
// and a workspace for its partial sums, allocated here by tfft_gbconv_plan_prepare so that the executions only launch kernels.
//
// All results are checked against the same sums in fp64 on the host (dx and dpre on a sample of the sequences). exit 0 / 1.
//
// usage: example_gated_conv_backward [L = 16384] [K = 2049] [rows = 9] [channels = 4]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tfft_gbconv.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_GBCONV(c)                                                      \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, tfft_gbconv_last_error());                 \
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
  const int flags = TFFT_GBCONV_PRE_GATE | TFFT_GBCONV_POST_GATE;
  CHECK_GBCONV(tfft_gbconv_geometry(L, K, rows, channels, 0, &halo, &hop, &segments, &partials));
  CHECK_GBCONV(tfft_gbconv_describe(L, K, rows, channels, 0, flags, text, sizeof(text)));
  tfft_gbconv_opts opts = TFFT_GBCONV_OPTS_INIT;
  opts.flags = flags;
  tfft_gbconv_plan* plan = nullptr;
  CHECK_GBCONV(tfft_gbconv_plan_create(rows, channels, L, K, dev, &opts, &plan));
  CHECK_GBCONV(tfft_gbconv_plan_prepare(plan));
  std::printf("L = %llu, K = %llu, %u x %u sequences: halo %llu, hop %llu, %llu segments, %llu partial sums per channel: %s, workspace %zu bytes\n", L, K,
              rows, channels, static_cast<unsigned long long>(halo), static_cast<unsigned long long>(hop), static_cast<unsigned long long>(segments),
              static_cast<unsigned long long>(partials), text, tfft_gbconv_plan_workspace_bytes(plan));

  unsigned s = 2463534242u;
  auto uniform = [&]() {
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    return static_cast<float>(s >> 8) / 8388608.0f - 1.0f;
  };
  // the taps: an exponentially decaying random kernel per channel, normalised to sum |h| = 1; the skip weights in (-0.5, 0.5)
  std::vector<__half> taps(static_cast<size_t>(channels) * K), skip(channels);
  for (unsigned c = 0; c < channels; ++c) {
    std::vector<double> h(K);
    double sum = 0;
    for (unsigned long long j = 0; j < K; ++j) {
      h[j] = uniform() * std::exp(-static_cast<double>(j) * (4.0 + c) / static_cast<double>(K));
      sum += std::fabs(h[j]);
    }
    for (unsigned long long j = 0; j < K; ++j) taps[c * K + j] = __float2half(static_cast<float>(h[j] / sum));
    skip[c] = __float2half(0.5f * uniform());
  }
  __half *d_taps = nullptr, *d_skip = nullptr;
  CHECK_HIP(hipMalloc(&d_taps, taps.size() * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_skip, skip.size() * sizeof(__half)));
  CHECK_HIP(hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(d_skip, skip.data(), skip.size() * sizeof(__half), hipMemcpyHostToDevice));

  const size_t halves = static_cast<size_t>(rows) * channels * L;
  std::vector<__half> hx(halves), hpre(halves), hgy(halves), hpost(halves), hdx(halves), hdpre(halves);
  for (std::vector<__half>* v : {&hx, &hpre, &hgy, &hpost})
    for (size_t i = 0; i < halves; ++i) (*v)[i] = __float2half(uniform());
  std::vector<float> hdh(static_cast<size_t>(channels) * K), hdskip(channels);
  __half *x = nullptr, *pre = nullptr, *gy = nullptr, *post = nullptr, *dx = nullptr, *dpre = nullptr;
  float *dh = nullptr, *dskip = nullptr;
  for (__half** p : {&x, &pre, &gy, &post, &dx, &dpre}) CHECK_HIP(hipMalloc(p, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&dh, hdh.size() * sizeof(float)));
  CHECK_HIP(hipMalloc(&dskip, hdskip.size() * sizeof(float)));
  CHECK_HIP(hipMemcpy(x, hx.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(pre, hpre.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(gy, hgy.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(post, hpost.data(), halves * sizeof(__half), hipMemcpyHostToDevice));

  // the tap gradient works before any set_taps; the input gradient does not, and says so
  CHECK_GBCONV(tfft_gbconv_exec_tap_grad(plan, x, pre, gy, post, dh, dskip, nullptr));
  const bool needs_taps = tfft_gbconv_exec_input_grad(plan, gy, post, x, pre, dx, dpre, nullptr) == TFFT_ERR_ARG;
  std::printf("input gradient before set_taps: %s\n", needs_taps ? tfft_gbconv_last_error() : "NOT refused");
  CHECK_GBCONV(tfft_gbconv_plan_set_taps(plan, d_taps, d_skip, nullptr));
  (void)hipFree(d_taps);      // the plan holds its own spectrum
  (void)hipFree(d_skip);
  CHECK_GBCONV(tfft_gbconv_exec_input_grad(plan, gy, post, x, pre, dx, dpre, nullptr));
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(hdx.data(), dx, halves * sizeof(__half), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hdpre.data(), dpre, halves * sizeof(__half), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hdh.data(), dh, hdh.size() * sizeof(float), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(hdskip.data(), dskip, hdskip.size() * sizeof(float), hipMemcpyDeviceToHost));

  auto val = [](const __half& v) { return static_cast<double>(__half2float(v)); };
  // dx and dpre: the definition, in fp64, on the first, a middle and the last row of every channel
  double worst_dx = 0, worst_dpre = 0;
  const unsigned picks[3] = {0, rows / 2, rows - 1};
  std::vector<double> gz(L);
  for (unsigned c = 0; c < channels; ++c)
    for (unsigned b : picks) {
      const size_t at = (static_cast<size_t>(b) * channels + c) * L;
      for (unsigned long long t = 0; t < L; ++t) gz[t] = val(hpost[at + t]) * val(hgy[at + t]);
      double err_x = 0, ref_x = 0, err_p = 0, ref_p = 0;
      for (unsigned long long t = 0; t < L; ++t) {
        double du = val(skip[c]) * gz[t];
        for (unsigned long long j = 0; j < K && t + j < L; ++j) du += val(taps[c * K + j]) * gz[t + j];
        const double want_x = val(hpre[at + t]) * du, want_p = val(hx[at + t]) * du;
        err_x += (val(hdx[at + t]) - want_x) * (val(hdx[at + t]) - want_x);
        ref_x += want_x * want_x;
        err_p += (val(hdpre[at + t]) - want_p) * (val(hdpre[at + t]) - want_p);
        ref_p += want_p * want_p;
      }
      worst_dx = std::fmax(worst_dx, std::sqrt(err_x / ref_x));
      worst_dpre = std::fmax(worst_dpre, std::sqrt(err_p / ref_p));
    }
  // dh: every tap of every channel; dskip: the bits of dh[c][0]
  double worst_dh = 0;
  bool skip_bits = true;
  std::vector<double> u(static_cast<size_t>(rows) * L), g(static_cast<size_t>(rows) * L);
  for (unsigned c = 0; c < channels; ++c) {
    for (unsigned b = 0; b < rows; ++b) {
      const size_t at = (static_cast<size_t>(b) * channels + c) * L;
      for (unsigned long long t = 0; t < L; ++t) {
        u[b * L + t] = val(hpre[at + t]) * val(hx[at + t]);
        g[b * L + t] = val(hpost[at + t]) * val(hgy[at + t]);
      }
    }
    double err2 = 0, ref2 = 0;
    for (unsigned long long j = 0; j < K; ++j) {
      double want = 0;
      for (unsigned b = 0; b < rows; ++b)
        for (unsigned long long t = j; t < L; ++t) want += g[b * L + t] * u[b * L + t - j];
      const double got = hdh[c * K + j];
      err2 += (got - want) * (got - want);
      ref2 += want * want;
    }
    worst_dh = std::fmax(worst_dh, std::sqrt(err2 / ref2));
    skip_bits = skip_bits && std::memcmp(&hdskip[c], &hdh[c * K], sizeof(float)) == 0;
  }
  std::printf("worst rel-L2 error: dx %.2e, dpre %.2e (of a checked sequence), dh %.2e (of a channel); dskip %s dh[c][0]\n", worst_dx, worst_dpre,
              worst_dh, skip_bits ? "has the bits of" : "DIFFERS from");
  // in-place execution of the input gradient is refused, and says why
  const bool refused = tfft_gbconv_exec_input_grad(plan, gy, post, x, pre, gy, dpre, nullptr) == TFFT_ERR_ARG;
  std::printf("in place: %s\n", refused ? tfft_gbconv_last_error() : "NOT refused");
  tfft_gbconv_plan_destroy(plan);
  for (__half* p : {x, pre, gy, post, dx, dpre}) (void)hipFree(p);
  (void)hipFree(dh);
  (void)hipFree(dskip);
  // dx, dpre: two transforms and the binary16 spectrum, as the forward pass, and one binary16 product at either end. dh: gated
  // noise against gated noise, so every tap is a sum of about rows * L products that largely cancel, while every item's rounding
  // is relative to its peak: a few 1e-3 of the rms tap
  const bool ok = worst_dx < 4e-3 && worst_dpre < 4e-3 && worst_dh < 1e-2 && skip_bits && refused && needs_taps;
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
