// tfft_stft.hip — host side and C ABI (include/tfft_stft.h) of the short-time Fourier transform add-on, libtfft_stft.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp and rsplit.hpp, header only, for the device helpers and the constant tables of
// the kernel (the add-on uploads a copy of its own). Every refusal, the plan-create sequence, the window and the checks of an
// execution come from conv/stft_host.hpp, which the four STFT libraries share; here are the plan struct, the kernel's LDS opt-in,
// the launch and the two texts. tests/test_gpu_stft.py holds the plan to tfft_exec_r2c bit for bit.
#include "../../include/tfft_stft.h"
#include "stft4096.hpp"
#include "../conv/stft_host.hpp"

struct tfft_stft_plan {
  uint64_t n = 0, rows = 0, length = 0, hop = 0, pad = 0, frames = 0, total = 0, items = 0, in_stride = 0, out_stride = 0;
  uint32_t launch_iters = 0;
  int device = 0, num_cus = 256;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_window = nullptr;      // 4096 halves, the plan's own copy
  bool have_window = false;
};

namespace {

static_assert(TFFT_STFT_N == kN && TFFT_STFT_BINS == bins_of(kN) && TFFT_STFT_PITCH == pitch_of(kN),
              "include/tfft_stft.h and the host headers under conv/ disagree on the frame length");
constexpr stft_rules kRules = {"stft", false, 0, "must be 0", nullptr};

int create_device(tfft_stft_plan* p, const tfft_stft_opts&) {
  p->items = (p->total + 1) / 2;
  std::vector<uint8_t> blob;
  k4096::build_tables(blob);
  const int rc = create_device_base(p, blob, k4096::kOffF1n);
  if (rc) return rc;
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(stft4096::stft4096_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  return TFFT_OK;
}

}  // namespace

extern "C" {

const char* tfft_stft_last_error(void) { return g_err.c_str(); }

int tfft_stft_geometry(uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  g_err.clear();
  return check_geometry(kN, length, hop, pad, frames);
}

int tfft_stft_describe(uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  uint64_t frames = 0;
  const int rc = check_shape(kRules, kN, rows, length, hop, pad, flags, &frames);
  if (rc) return rc;
  return copy_text("stft4096:4096 x " + std::to_string(frames), buf, bytes);
}

int tfft_stft_plan_create(uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id, const tfft_stft_opts* opts,
                          tfft_stft_plan** out) {
  return create_plan(kRules, kN, rows, length, hop, pad, device_id, opts, tfft_stft_opts TFFT_STFT_OPTS_INIT, &tfft_stft_opts::in_sig_stride,
                     &tfft_stft_opts::out_frame_stride, out, tfft_stft_plan_destroy, create_device);
}

void tfft_stft_plan_destroy(tfft_stft_plan* p) {
  if (!p) return;
  destroy_device_base(p);
  delete p;
}

int tfft_stft_plan_set_window(tfft_stft_plan* p, const void* window, void* stream) { return set_window(p, window, stream); }

int tfft_stft_exec(const tfft_stft_plan* p, const void* in, void* out_re, void* out_im, void* stream) {
  const int rc = check_exec_forward(kRules, p, in, out_re, out_im);
  if (rc) return rc;
  const stft4096::geometry geo = {static_cast<int32_t>(p->length / 8), p->frames > 1 ? static_cast<int32_t>(p->hop / 8) : 0,
                                  static_cast<int32_t>(p->pad / 8), static_cast<uint32_t>(p->frames)};
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipLaunchKernelGGL(stft4096::stft4096_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(in), static_cast<const uint16_t*>(p->d_window), static_cast<uint16_t*>(out_re),
                     static_cast<uint16_t*>(out_im), p->in_stride, p->out_stride, geo, static_cast<uint32_t>(p->total),
                     static_cast<uint32_t>(p->items), live, static_cast<const uint8_t*>(p->d_tables));
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_stft_plan_num_launches(const tfft_stft_plan* p) { return p ? 1 : 0; }

int tfft_stft_plan_kernels(const tfft_stft_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("stft4096::stft4096_kernel\n", 1, buf, bytes);
}

}  // extern "C"
