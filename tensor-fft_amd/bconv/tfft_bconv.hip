// tfft_bconv.hip — host side and C ABI (include/tfft_bconv.h) of the gradient add-on of the overlap-save causal convolution,
// libtfft_bconv.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp, header only. It does not link libtfft_sconv.so: the geometry, the checks, the
// launch shapes and the fp64 spectrum builder come from conv/host_math.hpp and conv/host_plumbing.hpp, the two headers every
// convolution library includes, and tests/test_bconv_host.py and tests/test_gpu_bconv.py hold them to the shipped code (the
// geometry and the refusals on the host, the spectrum to tfft_lconv_spectrum_host bit for bit).
#include "../../include/tfft_bconv.h"
#include "bconv4096.hpp"
#include "../conv/host_plumbing.hpp"

namespace {

static_assert(TFFT_BCONV_MAX_TAPS == kMaxTaps, "include/tfft_bconv.h and conv/host_math.hpp disagree on the longest filter");
constexpr shape_rules kRules = {0, "must be 0", "tfft_lconv_plan_create"};

}  // namespace

struct tfft_bconv_plan {
  uint64_t rows = 0, channels = 0, length = 0, taps = 0, halo = 0, hop = 0, segments = 0, items = 0;
  uint64_t x_stride = 0, g_stride = 0, dx_stride = 0, partials = 0, per_channel = 0, kpad = 0;
  uint32_t launch_iters = 0;
  int device = 0, num_cus = 256;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // conj(H): [channels][RE 4096 | IM 4096] in filter_slot order (input gradient)
  uint16_t* d_spec = nullptr;        // H: [RE: channels x 4096 | IM: channels x 4096], natural bin order (tfft_bconv_plan_spectrum)
  bool have_taps = false;
  size_t ws_need = 0;                // channels * partials * kpad floats
  mutable std::mutex ws_mutex;
  mutable void* ws = nullptr;
  mutable bool ws_owned = false;
};

namespace {

int create_device(tfft_bconv_plan* p) {
  const int rc = create_base(p);
  if (rc) return rc;
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bconv4096::dgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bconv4096::wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bconv4096::kWgradLdsBytes));
  return TFFT_OK;
}

bconv4096::geometry geometry_of(const tfft_bconv_plan* p) {
  return {static_cast<int32_t>(p->length / 8), static_cast<int32_t>(p->halo / 8), static_cast<int32_t>(p->hop / 8), static_cast<int32_t>(p->segments)};
}

}  // namespace

extern "C" {

const char* tfft_bconv_last_error(void) { return g_err.c_str(); }

int tfft_bconv_geometry(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, uint64_t* halo, uint64_t* hop,
                        uint64_t* segments, uint64_t* partials_out) {
  g_err.clear();
  const int rc = check_shape(rows, channels, length, taps, 0, "tfft_bconv_opts", kRules);
  if (rc) return rc;
  if (halo) *halo = halo_of(taps);
  if (hop) *hop = hop_of(taps);
  if (segments) *segments = segments_of(length, taps);
  if (partials_out) *partials_out = partials_of(rows, channels, length, taps, partials);
  return TFFT_OK;
}

int tfft_bconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_bconv_opts", kRules);
  if (rc) return rc;
  return copy_text("bconv4096:4096 x " + std::to_string(segments_of(length, taps)) + " | partials " +
                       std::to_string(partials_of(rows, channels, length, taps, partials)),
                   buf, bytes);
}

int tfft_bconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_bconv_opts* opts,
                           tfft_bconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_bconv_opts o = TFFT_BCONV_OPTS_INIT;
  int rc = take_opts(opts, "tfft_bconv_opts", o);
  if (rc) return rc;
  rc = check_shape(rows, channels, length, taps, o.flags, "tfft_bconv_opts", kRules);
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.x_seq_stride, "x");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.g_seq_stride, "g");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.dx_seq_stride, "dx");
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_bconv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_bconv_plan* p = new tfft_bconv_plan;
  p->rows = rows;
  p->channels = channels;
  p->length = length;
  p->taps = taps;
  p->halo = halo_of(taps);
  p->hop = hop_of(taps);
  p->segments = segments_of(length, taps);
  p->per_channel = (rows + 1) / 2 * p->segments;
  p->items = p->per_channel * channels;
  p->partials = partials_of(rows, channels, length, taps, o.partials);
  p->kpad = kpad_of(taps);
  p->ws_need = static_cast<size_t>(channels * p->partials * p->kpad * 4);
  p->x_stride = o.x_seq_stride ? o.x_seq_stride : length;
  p->g_stride = o.g_seq_stride ? o.g_seq_stride : length;
  p->dx_stride = o.dx_seq_stride ? o.dx_seq_stride : length;
  p->launch_iters = o.launch_iters;
  p->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
  rc = create_device(p);
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_bconv_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_bconv_plan_destroy(tfft_bconv_plan* p) {
  if (!p) return;
  destroy_base(p);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_bconv_plan_set_taps(tfft_bconv_plan* p, const void* taps, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return set_taps(p, taps, nullptr, stream, true);
}

int tfft_bconv_plan_spectrum(const tfft_bconv_plan* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return copy_spectrum(p, h_re, h_im, "tfft_bconv_plan_set_taps");
}

size_t tfft_bconv_plan_workspace_bytes(const tfft_bconv_plan* p) { return p ? p->ws_need : 0; }

int tfft_bconv_plan_set_workspace(tfft_bconv_plan* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_set(p, device_ptr, bytes);
}

int tfft_bconv_plan_prepare(tfft_bconv_plan* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_prepare(p);
}

int tfft_bconv_exec_input_grad(const tfft_bconv_plan* p, const void* g, void* dx, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_bconv_plan_set_taps first");
  if (!g || !dx) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(dx)) & 15) return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  // segment s reads, beyond its hop, the start of the stretch segment s + 1 writes, and segments run in no defined order
  if (g == dx || seqs_overlap(g, p->g_stride, p->length, dx, p->dx_stride, p->length, p->rows * p->channels))
    return fail(TFFT_ERR_ARG, "g and dx overlap (the input gradient cannot run in place: a segment reads what its successor overwrites)");
  const int rc = check_current(p->device);
  if (rc) return rc;
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipLaunchKernelGGL(bconv4096::dgrad_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(g), static_cast<uint16_t*>(dx), p->g_stride, p->dx_stride, static_cast<uint32_t>(p->rows),
                     static_cast<uint32_t>(p->channels), geometry_of(p), static_cast<uint32_t>(p->items), live,
                     static_cast<const uint8_t*>(p->d_tables), p->d_filter);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_bconv_exec_tap_grad(const tfft_bconv_plan* p, const void* x, const void* g, void* dh, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!x || !g || !dh) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g)) & 15) return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(dh) & 3) return fail(TFFT_ERR_ARG, "the tap gradient must be 4-byte aligned");
  const uint64_t seqs = p->rows * p->channels, dh_bytes = p->channels * p->taps * 4;
  if (block_overlaps(dh, dh_bytes, x, p->x_stride, seqs, p->length) || block_overlaps(dh, dh_bytes, g, p->g_stride, seqs, p->length))
    return fail(TFFT_ERR_ARG, "the tap gradient overlaps x or g");
  int rc = check_current(p->device);
  if (rc == TFFT_OK) rc = ws_ensure(p);
  if (rc) return rc;
  if (block_overlaps(p->ws, p->ws_need, x, p->x_stride, seqs, p->length) || block_overlaps(p->ws, p->ws_need, g, p->g_stride, seqs, p->length) ||
      blocks_overlap(dh, dh_bytes, p->ws, p->ws_need))
    return fail(TFFT_ERR_ARG, "the workspace overlaps x, g or the tap gradient");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t live, grid;
  wgrad_shape(p->channels * p->partials, p->num_cus, bconv4096::kWgradWaves, live, grid);
  hipLaunchKernelGGL(bconv4096::wgrad_kernel, dim3(grid), dim3(bconv4096::kWgradThreads), bconv4096::kWgradLdsBytes, s, static_cast<const uint16_t*>(x),
                     static_cast<const uint16_t*>(g), p->x_stride, p->g_stride, static_cast<uint32_t>(p->rows), static_cast<uint32_t>(p->channels),
                     geometry_of(p), static_cast<uint32_t>(p->partials), static_cast<uint32_t>(p->per_channel),
                     static_cast<uint32_t>(p->channels * p->partials), live, static_cast<int32_t>(p->kpad / 8), static_cast<uint32_t>(p->kpad),
                     static_cast<const uint8_t*>(p->d_tables), static_cast<float*>(p->ws));
  CONV_HIP(hipGetLastError());
  const uint64_t total = p->channels * p->taps;
  hipLaunchKernelGGL(bconv4096::wreduce_kernel, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(p->ws),
                     static_cast<float*>(dh), static_cast<uint32_t>(p->channels), static_cast<uint32_t>(p->taps), static_cast<uint32_t>(p->partials),
                     static_cast<uint32_t>(p->kpad));
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_bconv_plan_num_launches(const tfft_bconv_plan* p) { return p ? 3 : 0; }

int tfft_bconv_plan_kernels(const tfft_bconv_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("bconv4096::dgrad_kernel\nbconv4096::wgrad_kernel\nbconv4096::wreduce_kernel\n", 3, buf, bytes);
}

}  // extern "C"
