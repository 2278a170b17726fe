// example_masked_istft.cpp — masking in the STFT domain at frame length 1024 through the C ABI of the short-frame STFT add-on and
// the masked inverse (include/tfft_stftn.h, include/tfft_mistftn.h): a two-tone signal goes through STFT (Hann window, hop 256, pad
// 512: torch's center=True), and a masked ISTFT plan with a 0 / 1 mask on the device brings one tone back. Where example_istftn.cpp
// writes zeros into the spectra before the inverse, nothing is written here: the plan reads the spectra as the STFT plan left them
// and the mask beside them, and multiplies inside its merge. The mask is per bin (TFFT_MISTFTN_MASK_PER_BIN): one mask of 513 halves
// serves every frame.
//
// Printed: the residual of the removed tone (the amplitude of it that is left in the result), its threshold, and the worst error on
// the kept tone, both over the samples that lie under full frames only. exit 0 / 1.
//
// usage: example_masked_istft [length = 16384]
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfft_mistftn.h"
#include "tfft_stftn.h"

#define CHECK_HIP(c)                                                         \
  do {                                                                       \
    hipError_t e_ = (c);                                                     \
    if (e_ != hipSuccess) {                                                  \
      std::printf("%s: %s\n", #c, hipGetErrorString(e_));                    \
      return 1;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_TFFT(c, last_error)                                            \
  do {                                                                       \
    if ((c) != TFFT_OK) {                                                    \
      std::printf("%s: %s\n", #c, last_error());                             \
      return 1;                                                              \
    }                                                                        \
  } while (0)

int main(int argc, char** argv) {
  const unsigned long long L = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 16384;
  const uint32_t n = 1024;
  const unsigned long long hop = 256, pad = 512, pitch = 520;     // pitch: tfft_rplan_spectrum_pitch(1024)
  if (L < 3 * n || L % 8 || L > (1ull << 22)) {
    std::printf("length must be a multiple of 8 in 3072 .. 2^22\n");
    return 1;
  }
  const int keep = 50, drop = 225;               // the two tones, in bins of the frame length
  const double amp = 0.3;
  int dev = 0;
  CHECK_HIP(hipGetDevice(&dev));

  char text[128];
  uint64_t frames = 0;
  tfft_mistftn_opts opts = TFFT_MISTFTN_OPTS_INIT;
  opts.flags = TFFT_MISTFTN_MASK_PER_BIN;
  CHECK_TFFT(tfft_mistftn_geometry(n, L, hop, pad, &frames), tfft_mistftn_last_error);
  CHECK_TFFT(tfft_mistftn_describe(n, L, hop, pad, 1, opts.flags, text, sizeof(text)), tfft_mistftn_last_error);
  tfft_stftn_plan* fwd = nullptr;
  tfft_mistftn_plan* inv = nullptr;
  CHECK_TFFT(tfft_stftn_plan_create(n, 1, L, hop, pad, dev, nullptr, &fwd), tfft_stftn_last_error);
  CHECK_TFFT(tfft_mistftn_plan_create(n, 1, L, hop, pad, dev, &opts, &inv), tfft_mistftn_last_error);
  std::printf("n = %u, L = %llu, hop = %llu, pad = %llu: %llu frames: %s, %d launches, workspace %zu bytes\n", n, L, hop, pad,
              static_cast<unsigned long long>(frames), text, tfft_mistftn_plan_num_launches(inv), tfft_mistftn_plan_workspace_bytes(inv));

  std::vector<__half> sig(L), win(n), gate(pitch);
  for (unsigned long long t = 0; t < L; ++t) {
    const double ph = 2.0 * M_PI * static_cast<double>(t) / static_cast<double>(n);
    sig[t] = __float2half(static_cast<float>(amp * std::cos(keep * ph) + amp * std::sin(drop * ph)));
  }
  for (uint32_t j = 0; j < n; ++j)               // the periodic Hann window
    win[j] = __float2half(static_cast<float>(0.5 - 0.5 * std::cos(2.0 * M_PI * static_cast<double>(j) / static_cast<double>(n))));
  // the mask: 0 on bins drop - 8 .. drop + 8 (a Hann-windowed line on a bin occupies three bins), 1 elsewhere
  for (unsigned long long k = 0; k < pitch; ++k)
    gate[k] = __float2half(std::llabs(static_cast<long long>(k) - drop) <= 8 ? 0.0f : 1.0f);

  __half *x = nullptr, *w = nullptr, *spec = nullptr, *mask = nullptr, *y = nullptr;
  const size_t spec_halves = static_cast<size_t>(frames) * 2 * pitch;         // frame g: [RE 520 | IM 520]
  CHECK_HIP(hipMalloc(&x, L * sizeof(__half)));
  CHECK_HIP(hipMalloc(&w, n * sizeof(__half)));
  CHECK_HIP(hipMalloc(&spec, spec_halves * sizeof(__half)));
  CHECK_HIP(hipMalloc(&mask, pitch * sizeof(__half)));
  CHECK_HIP(hipMalloc(&y, L * sizeof(__half)));
  CHECK_HIP(hipMemcpy(x, sig.data(), L * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(w, win.data(), n * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_HIP(hipMemcpy(mask, gate.data(), pitch * sizeof(__half), hipMemcpyHostToDevice));
  CHECK_TFFT(tfft_stftn_plan_set_window(fwd, w, nullptr), tfft_stftn_last_error);
  CHECK_TFFT(tfft_mistftn_plan_set_window(inv, w, nullptr), tfft_mistftn_last_error);

  CHECK_TFFT(tfft_stftn_exec(fwd, x, spec, spec + pitch, nullptr), tfft_stftn_last_error);
  // the output must not meet the mask, and the plan says so
  const bool refused = tfft_mistftn_exec(inv, spec, spec + pitch, mask, mask, nullptr) == TFFT_ERR_ARG;
  std::printf("output on the mask: %s\n", refused ? tfft_mistftn_last_error() : "NOT refused");
  CHECK_TFFT(tfft_mistftn_exec(inv, spec, spec + pitch, mask, y, nullptr), tfft_mistftn_last_error);
  CHECK_HIP(hipDeviceSynchronize());
  std::vector<__half> back(L);
  CHECK_HIP(hipMemcpy(back.data(), y, L * sizeof(__half), hipMemcpyDeviceToHost));

  // over the samples under full frames only: what is left of the removed tone (its amplitude, by projection), and the worst error
  // on the kept one
  double pc = 0, ps = 0, worst = 0;
  const unsigned long long t0 = n, t1 = L - n;
  for (unsigned long long t = t0; t < t1; ++t) {
    const double ph = 2.0 * M_PI * static_cast<double>(t) / static_cast<double>(n);
    const double e = static_cast<double>(__half2float(back[t])) - amp * std::cos(keep * ph);
    worst = std::fmax(worst, std::fabs(e));
    pc += e * std::cos(drop * ph);
    ps += e * std::sin(drop * ph);
  }
  const double left = 2.0 * std::sqrt(pc * pc + ps * ps) / static_cast<double>(t1 - t0);
  // binary16 carries 11 bits: 1 % of a tone's amplitude for what is left of the removed one, 2 % for the worst sample of the kept one
  const double threshold = 0.01 * amp;
  std::printf("residual of the removed tone (amplitude %.2f): %.3e (threshold %.3e); kept tone (amplitude %.2f): worst error %.2e\n", amp, left,
              threshold, amp, worst);
  tfft_stftn_plan_destroy(fwd);
  tfft_mistftn_plan_destroy(inv);
  (void)hipFree(x);
  (void)hipFree(w);
  (void)hipFree(spec);
  (void)hipFree(mask);
  (void)hipFree(y);
  const bool ok = refused && left <= threshold && worst <= 0.02 * amp;
  std::printf(ok ? "OK\n" : "FAILED\n");
  return ok ? 0 : 1;
}
