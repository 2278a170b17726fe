// example_gated_chunked_conv.cpp — streaming a long sequence through the GATED causal convolution y = post (.) (h' * (pre (.) x))
// in chunks, through the C ABI of the gated carried convolution add-on (include/tfft_gcconv.h). The whole signal and the whole pre
// gate lie in ONE buffer each; chunk k is the view [k * Lc, (k + 1) * Lc) of every sequence, and its histories are the views of the
// Hn samples in front of it: hist = in - Hn and pre_hist = pre - Hn with the buffers' own sequence strides. Nothing is copied,
// multiplied in a pass of its own, padded or sliced; the first chunk passes NULL histories, which read as zeros.
//
// With Lc a multiple of hop and Hn = halo the three chunks transform exactly the windows the whole-sequence gated plan
// (tfft_gsconv.h) transforms, so the joined output is compared with that plan's BIT FOR BIT. exit 0 / 1.
//
// usage: example_gated_chunked_conv [K = 130] [rows = 5] [channels = 3] [hops per chunk = 2]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tfft_gcconv.h"
#include "tfft_gsconv.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_GCCONV(c)                                                      \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, tfft_gcconv_last_error());                 \
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
  const unsigned long long K = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 130;
  const unsigned rows = argc > 2 ? static_cast<unsigned>(std::atoi(argv[2])) : 5;
  const unsigned channels = argc > 3 ? static_cast<unsigned>(std::atoi(argv[3])) : 3;
  const unsigned hops = argc > 4 ? static_cast<unsigned>(std::atoi(argv[4])) : 2;
  const unsigned chunks = 3;
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));

  uint64_t halo = 0, hop = 0, segments = 0, carry_min = 0;
  CHECK_GCCONV(tfft_gcconv_geometry(8, K, &halo, &hop, nullptr, &carry_min));
  const uint64_t Lc = hops * hop, L = chunks * Lc;                       // a chunk, the whole sequence
  CHECK_GCCONV(tfft_gcconv_geometry(Lc, K, nullptr, nullptr, &segments, nullptr));
  std::printf("K = %llu: halo %llu, hop %llu, carry_min %llu; %u x %u sequences of %llu samples in %u chunks of %llu (%llu segments each)\n", K,
              static_cast<unsigned long long>(halo), static_cast<unsigned long long>(hop), static_cast<unsigned long long>(carry_min), rows, channels,
              static_cast<unsigned long long>(L), chunks, static_cast<unsigned long long>(Lc), static_cast<unsigned long long>(segments));

  unsigned s = 2463534242u;
  auto uniform = [&]() {
    s ^= s << 13; s ^= s >> 17; s ^= s << 5;
    return static_cast<float>(s >> 8) / 8388608.0f - 1.0f;
  };
  // the taps: an exponentially decaying random kernel per channel, normalised to sum |h| = 1/2, and a skip weight of 1/4: |z| <= 3/4
  std::vector<__half> taps(static_cast<size_t>(channels) * K), skip(channels);
  for (unsigned c = 0; c < channels; ++c) {
    std::vector<double> h(K);
    double sum = 0;
    for (unsigned long long j = 0; j < K; ++j) {
      h[j] = uniform() * std::exp(-static_cast<double>(j) * (4.0 + c) / static_cast<double>(K));
      sum += std::fabs(h[j]);
    }
    for (unsigned long long j = 0; j < K; ++j) taps[c * K + j] = __float2half(static_cast<float>(0.5 * h[j] / sum));
    skip[c] = __float2half(c % 2 ? -0.25f : 0.25f);
  }
  __half *d_taps = nullptr, *d_skip = nullptr;
  CHECK_HIP(hipMalloc(&d_taps, taps.size() * sizeof(__half)));
  CHECK_HIP(hipMalloc(&d_skip, skip.size() * sizeof(__half)));
  CHECK_HIP(hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(d_skip, skip.data(), skip.size() * sizeof(__half), hipMemcpyHostToDevice));

  const size_t halves = static_cast<size_t>(rows) * channels * L;
  std::vector<__half> host(halves), gate_in(halves), gate_out(halves), whole(halves), streamed(halves);
  for (size_t i = 0; i < halves; ++i) {
    host[i] = __float2half(uniform());
    gate_in[i] = __float2half(uniform());
    gate_out[i] = __float2half(uniform());
  }
  __half *x = nullptr, *pre = nullptr, *post = nullptr, *y_whole = nullptr, *y_stream = nullptr;
  for (__half** p : {&x, &pre, &post, &y_whole, &y_stream}) CHECK_HIP(hipMalloc(p, halves * sizeof(__half)));
  CHECK_HIP(hipMemcpy(x, host.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(pre, gate_in.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(post, gate_out.data(), halves * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemset(y_stream, 0xff, halves * sizeof(__half)));

  // the reference: the gated long plan on the whole sequence
  tfft_gsconv_opts long_opts = TFFT_GSCONV_OPTS_INIT;
  long_opts.flags = TFFT_GSCONV_PRE_GATE | TFFT_GSCONV_POST_GATE;
  tfft_gsconv_plan* long_plan = nullptr;
  CHECK_GSCONV(tfft_gsconv_plan_create(rows, channels, L, K, dev, &long_opts, &long_plan));
  CHECK_GSCONV(tfft_gsconv_plan_set_taps(long_plan, d_taps, d_skip, nullptr));
  CHECK_GSCONV(tfft_gsconv_exec(long_plan, x, pre, post, y_whole, nullptr));

  // the stream: one plan for all chunks. Sequences are L halves apart in every buffer; the histories have their buffers' stride
  tfft_gcconv_opts opts = TFFT_GCCONV_OPTS_INIT;
  opts.flags = TFFT_GCCONV_PRE_GATE | TFFT_GCCONV_POST_GATE;
  opts.in_seq_stride = opts.out_seq_stride = opts.pre_seq_stride = opts.post_seq_stride = L;
  opts.history = halo;
  opts.hist_seq_stride = opts.pre_hist_seq_stride = halo ? L : 0;
  tfft_gcconv_plan* plan = nullptr;
  CHECK_GCCONV(tfft_gcconv_plan_create(rows, channels, Lc, K, dev, &opts, &plan));
  CHECK_GCCONV(tfft_gcconv_plan_set_taps(plan, d_taps, d_skip, nullptr));
  (void)hipFree(d_taps);      // the plans hold their own spectra
  (void)hipFree(d_skip);
  for (unsigned k = 0; k < chunks; ++k) {
    const __half *in = x + k * Lc, *gate = pre + k * Lc;
    const bool carried = k && halo;                                    // views into the previous chunk; NULL: zeros in front of sample 0
    CHECK_GCCONV(tfft_gcconv_exec(plan, in, gate, post + k * Lc, carried ? in - halo : nullptr, carried ? gate - halo : nullptr,
                                  y_stream + k * Lc, nullptr));
  }
  CHECK_HIP(hipDeviceSynchronize());
  CHECK_HIP(hipMemcpy(whole.data(), y_whole, halves * sizeof(__half), hipMemcpyDeviceToHost));
  CHECK_HIP(hipMemcpy(streamed.data(), y_stream, halves * sizeof(__half), hipMemcpyDeviceToHost));
  const bool same = std::memcmp(whole.data(), streamed.data(), halves * sizeof(__half)) == 0;
  std::printf("three chunks against the whole-sequence gated plan: %s\n", same ? "identical in every bit" : "DIFFERENT");

  // the definition, in fp64, on the first and the last row of every channel, across the first chunk boundary
  double worst = 0;
  const unsigned picks[2] = {0, rows - 1};
  for (unsigned c = 0; c < channels; ++c)
    for (unsigned b : picks) {
      const size_t at = (static_cast<size_t>(b) * channels + c) * L;
      double err2 = 0, ref2 = 0;
      for (unsigned long long t = Lc - 64; t < Lc + 2 * K && t < L; ++t) {
        double z = static_cast<double>(__half2float(skip[c])) * __half2float(gate_in[at + t]) * __half2float(host[at + t]);
        for (unsigned long long j = 0; j <= t && j < K; ++j)
          z += static_cast<double>(__half2float(taps[c * K + j])) * __half2float(gate_in[at + t - j]) * __half2float(host[at + t - j]);
        const double want = z * __half2float(gate_out[at + t]), got = __half2float(streamed[at + t]);
        err2 += (got - want) * (got - want);
        ref2 += want * want;
      }
      worst = std::fmax(worst, std::sqrt(err2 / ref2));
    }
  std::printf("worst rel-L2 error around the first chunk boundary against the fp64 sum: %.2e\n", worst);

  // a gate's history without the sequence's is refused, and so is an output on top of a history; both say why
  bool refused = true;
  if (halo) {
    refused = tfft_gcconv_exec(plan, x + Lc, pre + Lc, post + Lc, nullptr, pre + Lc - halo, y_stream + Lc, nullptr) == TFFT_ERR_ARG;
    std::printf("pre_hist without hist: %s\n", refused ? tfft_gcconv_last_error() : "NOT refused");
    const bool on_top = tfft_gcconv_exec(plan, x + Lc, pre + Lc, post + Lc, x + Lc - halo, pre + Lc - halo, pre + Lc - halo, nullptr) == TFFT_ERR_ARG;
    std::printf("output on the pre gate and its history: %s\n", on_top ? tfft_gcconv_last_error() : "NOT refused");
    refused = refused && on_top;
  }
  tfft_gcconv_plan_destroy(plan);
  tfft_gsconv_plan_destroy(long_plan);
  for (__half* p : {x, pre, post, y_whole, y_stream}) (void)hipFree(p);
  const bool ok = same && worst < 3e-3 && refused;
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
