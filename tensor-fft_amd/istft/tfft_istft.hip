// tfft_istft.hip — host side and C ABI (include/tfft_istft.h) of the inverse short-time Fourier transform add-on, libtfft_istft.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp and rsplit.hpp, header only, for the device helpers and the constant tables of
// the frames kernel (the add-on uploads a copy of its own). Every refusal, the plan-create sequence, the window, the checks of an
// execution and the grid of the overlap-add come from conv/stft_host.hpp, which the four STFT libraries share, and the workspace
// rules from conv/host_plumbing.hpp; here are the plan struct, the frames kernel's LDS opt-in, the two launches and the two texts.
// tests/test_gpu_istft.py holds the frames to tfft_exec_inverse and the output to the numpy overlap-add, bit for bit.
#include "../../include/tfft_istft.h"
#include "istft4096.hpp"
#include "ola.hpp"
#include "../conv/stft_host.hpp"

struct tfft_istft_plan {
  uint64_t n = 0, rows = 0, length = 0, hop = 0, pad = 0, frames = 0, total = 0, items = 0, in_stride = 0, out_stride = 0;
  uint32_t launch_iters = 0;
  int flags = 0, device = 0, num_cus = 256;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_window = nullptr;      // 4096 halves, the plan's own copy
  bool have_window = false;
  size_t ws_need = 0;                // rows * frames * 4096 halves: the time-domain frames
  mutable std::mutex ws_mutex;
  mutable void* ws = nullptr;
  mutable bool ws_owned = false;
};

namespace {

static_assert(TFFT_ISTFT_N == kN && TFFT_ISTFT_BINS == bins_of(kN) && TFFT_ISTFT_PITCH == pitch_of(kN),
              "include/tfft_istft.h and the host headers under conv/ disagree on the frame length");
constexpr stft_rules kRules = {"istft", true, TFFT_ISTFT_RAW_SUM, "must be 0 or TFFT_ISTFT_RAW_SUM", nullptr};

int create_device(tfft_istft_plan* p, const tfft_istft_opts& o) {
  p->items = (p->total + 1) / 2;
  p->flags = o.flags;
  p->ws_need = static_cast<size_t>(p->total * kN * 2);
  std::vector<uint8_t> blob;
  k4096::build_tables(blob);
  const int rc = create_device_base(p, blob, k4096::kOffF1n);
  if (rc) return rc;
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(istft4096::frames_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  return TFFT_OK;
}

}  // namespace

extern "C" {

const char* tfft_istft_last_error(void) { return g_err.c_str(); }

int tfft_istft_geometry(uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  g_err.clear();
  return check_geometry(kN, length, hop, pad, frames);
}

int tfft_istft_describe(uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  uint64_t frames = 0;
  const int rc = check_shape(kRules, kN, rows, length, hop, pad, flags, &frames);
  if (rc) return rc;
  return copy_text("istft4096:4096 x " + std::to_string(frames) + " + ola", buf, bytes);
}

int tfft_istft_plan_create(uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id, const tfft_istft_opts* opts,
                           tfft_istft_plan** out) {
  return create_plan(kRules, kN, rows, length, hop, pad, device_id, opts, tfft_istft_opts TFFT_ISTFT_OPTS_INIT, &tfft_istft_opts::out_sig_stride,
                     &tfft_istft_opts::in_frame_stride, out, tfft_istft_plan_destroy, create_device);
}

void tfft_istft_plan_destroy(tfft_istft_plan* p) {
  if (!p) return;
  destroy_device_base(p);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_istft_plan_set_window(tfft_istft_plan* p, const void* window, void* stream) { return set_window(p, window, stream); }

size_t tfft_istft_plan_workspace_bytes(const tfft_istft_plan* p) { return p ? p->ws_need : 0; }

int tfft_istft_plan_set_workspace(tfft_istft_plan* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_set(p, device_ptr, bytes);
}

int tfft_istft_plan_prepare(tfft_istft_plan* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_prepare(p);
}

int tfft_istft_exec(const tfft_istft_plan* p, const void* in_re, const void* in_im, void* out, void* stream) {
  const int rc = check_exec_inverse(kRules, p, in_re, in_im, out);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint16_t* const frames = static_cast<uint16_t*>(p->ws);
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipLaunchKernelGGL(istft4096::frames_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, s, static_cast<const uint16_t*>(in_re),
                     static_cast<const uint16_t*>(in_im), frames, p->in_stride, static_cast<uint32_t>(p->total), static_cast<uint32_t>(p->items), live,
                     static_cast<const uint8_t*>(p->d_tables));
  CONV_HIP(hipGetLastError());
  const istft4096::ola_geometry geo = {p->rows, p->length / 8, ola_hop(p), p->out_stride, static_cast<uint32_t>(p->pad), static_cast<uint32_t>(p->frames)};
  hipLaunchKernelGGL(istft4096::ola_kernel, dim3(ola_grid(p, istft4096::kOlaBlock)), dim3(istft4096::kOlaBlock), 0, s, static_cast<const uint16_t*>(frames),
                     static_cast<const uint16_t*>(p->d_window), static_cast<uint16_t*>(out), geo, (p->flags & TFFT_ISTFT_RAW_SUM) ? 1 : 0);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_istft_plan_num_launches(const tfft_istft_plan* p) { return p ? 2 : 0; }

int tfft_istft_plan_kernels(const tfft_istft_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("istft4096::frames_kernel\nistft4096::ola_kernel\n", 2, buf, bytes);
}

}  // extern "C"
