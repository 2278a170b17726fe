// tfft_sconv.hip — host side and C ABI (include/tfft_sconv.h) of the overlap-save causal convolution add-on, libtfft_sconv.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp, header only, for the device helpers and the constant tables of the kernel
// (the add-on uploads a copy of its own). It does not link libtfft_lconv.so: the fp64 spectrum builder, the geometry, the refusals
// and the launch shape come from conv/host_math.hpp and conv/host_plumbing.hpp, the two headers every convolution library
// includes, and tests/test_gpu_sconv.py holds the plan's spectrum to tfft_lconv_spectrum_host bit for bit.
#include "../../include/tfft_sconv.h"
#include "sconv4096.hpp"
#include "../conv/host_plumbing.hpp"

namespace {

static_assert(TFFT_SCONV_MAX_TAPS == kMaxTaps, "include/tfft_sconv.h and conv/host_math.hpp disagree on the longest filter");
constexpr shape_rules kRules = {0, "must be 0", "tfft_lconv_plan_create"};

}  // namespace

struct tfft_sconv_plan {
  uint64_t rows = 0, channels = 0, length = 0, taps = 0, halo = 0, hop = 0, segments = 0, items = 0, in_stride = 0, out_stride = 0;
  uint32_t launch_iters = 0;
  int device = 0, num_cus = 256;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // [channels][RE 4096 | IM 4096] in filter_slot order
  uint16_t* d_spec = nullptr;        // [RE: channels x 4096 | IM: channels x 4096], natural bin order (tfft_sconv_plan_spectrum)
  bool have_taps = false;
};

namespace {

int create_device(tfft_sconv_plan* p) {
  const int rc = create_base(p);
  if (rc) return rc;
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(sconv4096::sconv4096_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  return TFFT_OK;
}

}  // namespace

extern "C" {

const char* tfft_sconv_last_error(void) { return g_err.c_str(); }

int tfft_sconv_geometry(uint64_t length, uint64_t taps, uint64_t* halo, uint64_t* hop, uint64_t* segments) {
  g_err.clear();
  const int rc = check_length_taps(length, taps, kRules);
  if (rc) return rc;
  if (halo) *halo = halo_of(taps);
  if (hop) *hop = hop_of(taps);
  if (segments) *segments = segments_of(length, taps);
  return TFFT_OK;
}

int tfft_sconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_sconv_opts", kRules);
  if (rc) return rc;
  return copy_text("sconv4096:4096 x " + std::to_string(segments_of(length, taps)), buf, bytes);
}

int tfft_sconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_sconv_opts* opts,
                           tfft_sconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_sconv_opts o = TFFT_SCONV_OPTS_INIT;
  int rc = take_opts(opts, "tfft_sconv_opts", o);
  if (rc) return rc;
  rc = check_shape(rows, channels, length, taps, o.flags, "tfft_sconv_opts", kRules);
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.in_seq_stride, "in");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.out_seq_stride, "out");
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_sconv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_sconv_plan* p = new tfft_sconv_plan;
  p->rows = rows;
  p->channels = channels;
  p->length = length;
  p->taps = taps;
  p->halo = halo_of(taps);
  p->hop = hop_of(taps);
  p->segments = segments_of(length, taps);
  p->items = (rows + 1) / 2 * p->segments * channels;
  p->in_stride = o.in_seq_stride ? o.in_seq_stride : length;
  p->out_stride = o.out_seq_stride ? o.out_seq_stride : length;
  p->launch_iters = o.launch_iters;
  p->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
  rc = create_device(p);
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_sconv_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_sconv_plan_destroy(tfft_sconv_plan* p) {
  if (!p) return;
  destroy_base(p);
  delete p;
}

int tfft_sconv_plan_set_taps(tfft_sconv_plan* p, const void* taps, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return set_taps(p, taps, nullptr, stream, false);
}

int tfft_sconv_plan_spectrum(const tfft_sconv_plan* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return copy_spectrum(p, h_re, h_im, "tfft_sconv_plan_set_taps");
}

int tfft_sconv_exec(const tfft_sconv_plan* p, const void* in, void* out, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_sconv_plan_set_taps first");
  if (!in || !out) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  // a segment's halo is the end of the stretch its predecessor writes, and segments run in no defined order: no in-place execution
  if (in == out || seqs_overlap(in, p->in_stride, p->length, out, p->out_stride, p->length, p->rows * p->channels))
    return fail(TFFT_ERR_ARG, "input and output overlap (an overlap-save plan cannot run in place: a segment reads the halo its predecessor overwrites)");
  const int rc = check_current(p->device);
  if (rc) return rc;
  const sconv4096::geometry geo = {static_cast<int32_t>(p->length / 8), static_cast<int32_t>(p->halo / 8), static_cast<int32_t>(p->hop / 8),
                                   static_cast<int32_t>(p->segments)};
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipLaunchKernelGGL(sconv4096::sconv4096_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(in), static_cast<uint16_t*>(out), p->in_stride, p->out_stride, static_cast<uint32_t>(p->rows),
                     static_cast<uint32_t>(p->channels), geo, static_cast<uint32_t>(p->items), live, static_cast<const uint8_t*>(p->d_tables),
                     p->d_filter);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_sconv_plan_num_launches(const tfft_sconv_plan* p) { return p ? 1 : 0; }

int tfft_sconv_plan_kernels(const tfft_sconv_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("sconv4096::sconv4096_kernel\n", 1, buf, bytes);
}

}  // extern "C"
