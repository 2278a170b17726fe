// example_chunked_conv.cpp — streaming a long sequence through the causal convolution in chunks, through the C ABI of the carried
// convolution add-on (include/tfft_cconv.h). The whole signal lies in ONE buffer; chunk k is the view [k * Lc, (k + 1) * Lc) of
// every sequence, and its history is the view of the Hn samples in front of it: hist = in - Hn with the buffer's own sequence
// stride. Nothing is copied, padded or sliced; the first chunk passes hist = NULL, which reads as zeros.
//
// With Lc a multiple of hop and Hn = halo the three chunks transform exactly the windows the whole-sequence plan (tfft_sconv.h)
// transforms, so the joined output is compared with that plan's BIT FOR BIT. exit 0 / 1.
//
// usage: example_chunked_conv [K = 130] [rows = 5] [channels = 3] [hops per chunk = 2]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tfft_cconv.h"
#include "tfft_sconv.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_CCONV(c)                                                       \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, tfft_cconv_last_error());                  \
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
  const unsigned long long K = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 130;
  const unsigned rows = argc > 2 ? static_cast<unsigned>(std::atoi(argv[2])) : 5;
  const unsigned channels = argc > 3 ? static_cast<unsigned>(std::atoi(argv[3])) : 3;
  const unsigned hops = argc > 4 ? static_cast<unsigned>(std::atoi(argv[4])) : 2;
  const unsigned chunks = 3;
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));

  uint64_t halo = 0, hop = 0, segments = 0, carry_min = 0;
  CHECK_CCONV(tfft_cconv_geometry(8, K, &halo, &hop, nullptr, &carry_min));
  const uint64_t Lc = hops * hop, L = chunks * Lc;                       // a chunk, the whole sequence
  CHECK_CCONV(tfft_cconv_geometry(Lc, K, nullptr, nullptr, &segments, nullptr));
  std::printf("K = %llu: halo %llu, hop %llu, carry_min %llu; %u x %u sequences of %llu samples in %u chunks of %llu (%llu segments each)\n", K,
              static_cast<unsigned long long>(halo), static_cast<unsigned long long>(hop), static_cast<unsigned long long>(carry_min), rows, channels,
              static_cast<unsigned long long>(L), chunks, static_cast<unsigned long long>(Lc), static_cast<unsigned long long>(segments));

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

  const size_t halves = static_cast<size_t>(rows) * channels * L;
  std::vector<__half> host(halves), whole(halves), streamed(halves);
  for (size_t i = 0; i < halves; ++i) host[i] = __float2half(uniform());
  __half *x = nullptr, *y_whole = nullptr, *y_stream = nullptr;
  CHECK_HIP(hipMalloc(&x, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&y_whole, halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&y_stream, halves * sizeof(__half)));
  CHECK_HIP(hipMemcpy(x, host.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemset(y_stream, 0xff, halves * sizeof(__half)));

  // the reference: the long plan on the whole sequence
  tfft_sconv_plan* long_plan = nullptr;
  CHECK_SCONV(tfft_sconv_plan_create(rows, channels, L, K, dev, nullptr, &long_plan));
  CHECK_SCONV(tfft_sconv_plan_set_taps(long_plan, d_taps, nullptr));
  CHECK_SCONV(tfft_sconv_exec(long_plan, x, y_whole, nullptr));

  // the stream: one plan for all chunks. Sequences are L halves apart in both buffers; the history has the input's stride
  tfft_cconv_opts opts = TFFT_CCONV_OPTS_INIT;
  opts.in_seq_stride = L;
  opts.out_seq_stride = L;
  opts.history = halo;
  opts.hist_seq_stride = halo ? L : 0;
  tfft_cconv_plan* plan = nullptr;
  CHECK_CCONV(tfft_cconv_plan_create(rows, channels, Lc, K, dev, &opts, &plan));
  CHECK_CCONV(tfft_cconv_plan_set_taps(plan, d_taps, nullptr));
  (void)hipFree(d_taps);      // the plans hold their own spectra
  for (unsigned k = 0; k < chunks; ++k) {
    const __half* in = x + k * Lc;
    const __half* hist = (k && halo) ? in - halo : nullptr;       // a view into the previous chunk; NULL: zeros in front of sample 0
    CHECK_CCONV(tfft_cconv_exec(plan, in, hist, y_stream + k * Lc, nullptr));
  }
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(whole.data(), y_whole, halves * sizeof(__half), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(streamed.data(), y_stream, halves * sizeof(__half), hipMemcpyDeviceToHost));
  const bool same = std::memcmp(whole.data(), streamed.data(), halves * sizeof(__half)) == 0;
  std::printf("three chunks against the whole-sequence plan: %s\n", same ? "identical in every bit" : "DIFFERENT");

  // the definition, in fp64, on the first and the last row of every channel, across the chunk boundaries
  double worst = 0;
  const unsigned picks[2] = {0, rows - 1};
  for (unsigned c = 0; c < channels; ++c)
    for (unsigned b : picks) {
      const __half* in = host.data() + (static_cast<size_t>(b) * channels + c) * L;
      const __half* out = streamed.data() + (static_cast<size_t>(b) * channels + c) * L;
      double err2 = 0, ref2 = 0;
      for (unsigned long long t = Lc - 64; t < Lc + 2 * K && t < L; ++t) {
        double want = 0;
        for (unsigned long long j = 0; j <= t && j < K; ++j) want += static_cast<double>(__half2float(taps[c * K + j])) * __half2float(in[t - j]);
        const double got = __half2float(out[t]);
        err2 += (got - want) * (got - want);
        ref2 += want * want;
      }
      worst = std::fmax(worst, std::sqrt(err2 / ref2));
    }
  std::printf("worst rel-L2 error around the first chunk boundary against the fp64 sum: %.2e\n", worst);

  // an output on top of the history is refused, and says why
  const bool refused = halo == 0 || tfft_cconv_exec(plan, x + Lc, x + Lc - halo, x + Lc - halo, nullptr) == TFFT_ERR_ARG;
  std::printf("output on the history: %s\n", refused ? (halo ? tfft_cconv_last_error() : "(no halo)") : "NOT refused");
  tfft_cconv_plan_destroy(plan);
  tfft_sconv_plan_destroy(long_plan);
  (void)hipFree(x);
  (void)hipFree(y_whole);
  (void)hipFree(y_stream);
  const bool ok = same && worst < 3e-3 && refused;
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
