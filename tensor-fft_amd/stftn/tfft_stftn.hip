// tfft_stftn.hip — host side and C ABI (include/tfft_stftn.h) of the short-frame STFT add-on, libtfft_stftn.so: the plans of
// include/tfft_stft.h at the frame lengths 512, 1024 and 2048.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp and rsplit.hpp, header only, for the device helpers, and k256r.hpp, in the host
// pass, for the constant tables of the kernel (the add-on uploads a copy of its own). Every refusal but that of n, the plan-create
// sequence, the window, the checks of an execution and the hold on k256r.hpp come from conv/stft_host.hpp, which the four STFT
// libraries share; here are the plan struct, check_n, the kernels' LDS opt-in, the launch and the two texts.
// tests/test_gpu_stftn.py holds the plan to tfft_exec_r2c bit for bit.
#include "../../include/tfft_stftn.h"
#include "stft256r.hpp"
#define STFT_HOST_256R stft256r
#include "../conv/stft_host.hpp"

struct tfft_stftn_plan {
  uint64_t n = 0, rows = 0, length = 0, hop = 0, pad = 0, frames = 0, total = 0, batch = 0, groups = 0, in_stride = 0, out_stride = 0;
  uint32_t launch_iters = 0;
  int radix = 0;                     // R = n / 256
  int device = 0, num_cus = 256;
  void* d_tables = nullptr;          // k256r::build_tables(R)
  uint16_t* d_window = nullptr;      // n halves, the plan's own copy
  bool have_window = false;
};

namespace {

int check_n(uint32_t n) {
  if (n == 4096) return fail(TFFT_ERR_ARG, "n = 4096 is the plan of include/tfft_stft.h: use tfft_stft_plan_create");
  if (n != 512 && n != 1024 && n != 2048) return fail(TFFT_ERR_ARG, "n must be 512, 1024 or 2048 (" + std::to_string(n) + ")");
  return TFFT_OK;
}
constexpr stft_rules kRules = {"stftn", false, 0, "must be 0", check_n};

template <int R>
int create_device(tfft_stftn_plan* p) {
  std::vector<uint8_t> blob;
  k256r_host::build_tables(R, blob);
  const int rc = create_device_base(p, blob, blob.size());
  if (rc) return rc;
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(stft256r::stft256r_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               stft256r::lds_bytes<R>()));
  return TFFT_OK;
}

template <int R>
void launch(const tfft_stftn_plan* p, const void* in, void* out_re, void* out_im, hipStream_t stream) {
  const stft256r::geometry geo = {static_cast<int32_t>(p->length / 8), p->frames > 1 ? static_cast<int32_t>(p->hop / 8) : 0,
                                  static_cast<int32_t>(p->pad / 8), static_cast<uint32_t>(p->frames)};
  uint32_t live, grid;
  conv_shape(p->groups, p->num_cus, p->launch_iters, live, grid);
  hipLaunchKernelGGL(stft256r::stft256r_kernel<R>, dim3(grid), dim3(k4096::kThreads), stft256r::lds_bytes<R>(), stream,
                     static_cast<const uint16_t*>(in), static_cast<const uint16_t*>(p->d_window), static_cast<uint16_t*>(out_re),
                     static_cast<uint16_t*>(out_im), p->in_stride, p->out_stride, geo, static_cast<uint32_t>(p->total),
                     static_cast<uint32_t>(p->batch), live, static_cast<const uint8_t*>(p->d_tables));
}

}  // namespace

extern "C" {

const char* tfft_stftn_last_error(void) { return g_err.c_str(); }

int tfft_stftn_geometry(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  g_err.clear();
  const int rc = check_n(n);
  return rc ? rc : check_geometry(n, length, hop, pad, frames);
}

int tfft_stftn_describe(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  uint64_t frames = 0;
  const int rc = check_shape(kRules, n, rows, length, hop, pad, flags, &frames);
  if (rc) return rc;
  return copy_text("stft256r" + std::to_string(n / 256) + ":" + std::to_string(n) + " x " + std::to_string(frames), buf, bytes);
}

int tfft_stftn_plan_create(uint32_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id, const tfft_stftn_opts* opts,
                           tfft_stftn_plan** out) {
  return create_plan(kRules, n, rows, length, hop, pad, device_id, opts, tfft_stftn_opts TFFT_STFTN_OPTS_INIT, &tfft_stftn_opts::in_sig_stride,
                     &tfft_stftn_opts::out_frame_stride, out, tfft_stftn_plan_destroy, [](tfft_stftn_plan* p, const tfft_stftn_opts&) {
                       p->radix = static_cast<int>(p->n / 256);
                       p->batch = (p->total + 1) / 2;
                       const uint64_t per_wave = 16 / p->radix;                 // transforms a wave takes per iteration
                       p->groups = (p->batch + per_wave - 1) / per_wave;
                       return p->radix == 2 ? create_device<2>(p) : p->radix == 4 ? create_device<4>(p) : create_device<8>(p);
                     });
}

void tfft_stftn_plan_destroy(tfft_stftn_plan* p) {
  if (!p) return;
  destroy_device_base(p);
  delete p;
}

int tfft_stftn_plan_set_window(tfft_stftn_plan* p, const void* window, void* stream) { return set_window(p, window, stream); }

int tfft_stftn_exec(const tfft_stftn_plan* p, const void* in, void* out_re, void* out_im, void* stream) {
  const int rc = check_exec_forward(kRules, p, in, out_re, out_im);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (p->radix == 2) launch<2>(p, in, out_re, out_im, s);
  else if (p->radix == 4) launch<4>(p, in, out_re, out_im, s);
  else launch<8>(p, in, out_re, out_im, s);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_stftn_plan_num_launches(const tfft_stftn_plan* p) { return p ? 1 : 0; }

int tfft_stftn_plan_kernels(const tfft_stftn_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("stft256r::stft256r_kernel<" + std::to_string(p->radix) + ">\n", 1, buf, bytes);
}

}  // extern "C"
