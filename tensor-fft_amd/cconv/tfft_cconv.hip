// tfft_cconv.hip — host side and C ABI (include/tfft_cconv.h) of the carried convolution add-on, libtfft_cconv.so: the forward
// plan of tfft_sconv.hip and the gradient plan of tfft_bconv.hip with a history in front of x and a future behind g.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp, header only. It links neither libtfft_sconv.so nor libtfft_bconv.so: the
// geometry, the checks, the launch shapes and the fp64 spectrum builder come from conv/host_math.hpp and
// conv/host_plumbing.hpp, the two headers every convolution library includes, and tests/test_cconv_host.py and
// tests/test_gpu_cconv.py hold them to the shipped code (the geometry and the refusals on the host; without a context every
// result to the shipped plans' bit for bit).
#include "../../include/tfft_cconv.h"
#include "cconv4096.hpp"
#include "../conv/host_plumbing.hpp"

namespace {

static_assert(TFFT_CCONV_MAX_TAPS == kMaxTaps, "include/tfft_cconv.h and conv/host_math.hpp disagree on the longest filter");
constexpr shape_rules kRules = {0, "must be 0", "tfft_lconv_plan_create"};

// what the two plan types share: the shape, the geometry and the device memory of tfft_sconv_plan
struct plan_base {
  uint64_t rows = 0, channels = 0, length = 0, taps = 0, halo = 0, hop = 0, segments = 0, items = 0;
  uint32_t launch_iters = 0;
  int device = 0, num_cus = 256;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // [channels][RE 4096 | IM 4096] in filter_slot order: H (forward), conj(H) (gradient)
  uint16_t* d_spec = nullptr;        // H: [RE: channels x 4096 | IM: channels x 4096], natural bin order
  bool have_taps = false;
};

void set_shape(plan_base* p, uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, uint32_t launch_iters, int device_id) {
  p->rows = rows;
  p->channels = channels;
  p->length = length;
  p->taps = taps;
  p->halo = halo_of(taps);
  p->hop = hop_of(taps);
  p->segments = segments_of(length, taps);
  p->items = (rows + 1) / 2 * p->segments * channels;
  p->launch_iters = launch_iters;
  p->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
}

cconv4096::geometry geometry_of(const plan_base* p) {
  return {static_cast<int32_t>(p->length / 8), static_cast<int32_t>(p->halo / 8), static_cast<int32_t>(p->hop / 8), static_cast<int32_t>(p->segments)};
}

}  // namespace

struct tfft_cconv_plan : plan_base {
  uint64_t in_stride = 0, out_stride = 0, history = 0, hist_stride = 0;
};

struct tfft_cconv_grad : plan_base {
  uint64_t x_stride = 0, g_stride = 0, dx_stride = 0, partials = 0, per_channel = 0, kpad = 0;
  uint64_t history = 0, hist_stride = 0, future = 0, fut_stride = 0;
  size_t ws_need = 0;                // channels * partials * kpad floats
  mutable std::mutex ws_mutex;
  mutable void* ws = nullptr;
  mutable bool ws_owned = false;
};

extern "C" {

const char* tfft_cconv_last_error(void) { return g_err.c_str(); }

// ---- the forward plan

int tfft_cconv_geometry(uint64_t length, uint64_t taps, uint64_t* halo, uint64_t* hop, uint64_t* segments, uint64_t* carry_min) {
  g_err.clear();
  const int rc = check_length_taps(length, taps, kRules);
  if (rc) return rc;
  if (halo) *halo = halo_of(taps);
  if (hop) *hop = hop_of(taps);
  if (segments) *segments = segments_of(length, taps);
  if (carry_min) *carry_min = carry_min_of(taps);
  return TFFT_OK;
}

int tfft_cconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_cconv_opts", kRules);
  if (rc) return rc;
  return copy_text("cconv4096:4096 x " + std::to_string(segments_of(length, taps)), buf, bytes);
}

int tfft_cconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_cconv_opts* opts,
                           tfft_cconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_cconv_opts o = TFFT_CCONV_OPTS_INIT;
  int rc = take_opts(opts, "tfft_cconv_opts", o);
  if (rc) return rc;
  rc = check_shape(rows, channels, length, taps, o.flags, "tfft_cconv_opts", kRules);
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.in_seq_stride, "in");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.out_seq_stride, "out");
  if (rc == TFFT_OK) rc = check_context(taps, o.history, "history");
  if (rc == TFFT_OK) rc = check_context_stride(o.history, o.hist_seq_stride, "history", "hist");
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_cconv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_cconv_plan* p = new tfft_cconv_plan;
  set_shape(p, rows, channels, length, taps, o.launch_iters, device_id);
  p->in_stride = o.in_seq_stride ? o.in_seq_stride : length;
  p->out_stride = o.out_seq_stride ? o.out_seq_stride : length;
  p->history = o.history;
  p->hist_stride = o.hist_seq_stride ? o.hist_seq_stride : o.history;
  rc = create_base(p);
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  if (rc == TFFT_OK && hipFuncSetAttribute(reinterpret_cast<const void*>(cconv4096::cconv4096_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           k4096::kLdsBytes) != hipSuccess)
    rc = fail(TFFT_ERR_HIP, "hipFuncSetAttribute(cconv4096_kernel) failed");
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_cconv_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_cconv_plan_destroy(tfft_cconv_plan* p) {
  if (!p) return;
  destroy_base(p);
  delete p;
}

int tfft_cconv_plan_set_taps(tfft_cconv_plan* p, const void* taps, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return set_taps(p, taps, nullptr, stream, false);
}

int tfft_cconv_plan_spectrum(const tfft_cconv_plan* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return copy_spectrum(p, h_re, h_im, "tfft_cconv_plan_set_taps");
}

int tfft_cconv_exec(const tfft_cconv_plan* p, const void* in, const void* hist, void* out, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_cconv_plan_set_taps first");
  if (!in || !out) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) & 15) return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  if (hist && p->history == 0) return fail(TFFT_ERR_ARG, "hist must be NULL: the plan was created with history = 0");
  if (reinterpret_cast<uintptr_t>(hist) & 15) return fail(TFFT_ERR_ARG, "hist must be 16-byte aligned");
  const uint64_t seqs = p->rows * p->channels;
  // a segment's halo is the end of the stretch its predecessor writes, and segments run in no defined order: no in-place execution
  if (in == out || seqs_overlap(in, p->in_stride, p->length, out, p->out_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "input and output overlap (an overlap-save plan cannot run in place: a segment reads the halo its predecessor overwrites)");
  if (hist && seqs_overlap(hist, p->hist_stride, p->history, out, p->out_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "hist and output overlap (the history may alias the input, never the output)");
  const int rc = check_current(p->device);
  if (rc) return rc;
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  // without a history the kernel gets 0 chunks of it and never forms an address from the second base
  hipLaunchKernelGGL(cconv4096::cconv4096_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(in), static_cast<const uint16_t*>(hist ? hist : in), static_cast<uint16_t*>(out), p->in_stride,
                     hist ? p->hist_stride : p->in_stride, p->out_stride, static_cast<uint32_t>(p->rows), static_cast<uint32_t>(p->channels),
                     geometry_of(p), static_cast<int32_t>(hist ? p->history / 8 : 0), static_cast<uint32_t>(p->items), live,
                     static_cast<const uint8_t*>(p->d_tables), p->d_filter);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_cconv_plan_num_launches(const tfft_cconv_plan* p) { return p ? 1 : 0; }

int tfft_cconv_plan_kernels(const tfft_cconv_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("cconv4096::cconv4096_kernel\n", 1, buf, bytes);
}

// ---- the gradient plan

int tfft_cconv_grad_geometry(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, uint64_t* halo, uint64_t* hop,
                             uint64_t* segments, uint64_t* partials_out, uint64_t* carry_min) {
  g_err.clear();
  const int rc = check_shape(rows, channels, length, taps, 0, "tfft_cconv_grad_opts", kRules);
  if (rc) return rc;
  if (halo) *halo = halo_of(taps);
  if (hop) *hop = hop_of(taps);
  if (segments) *segments = segments_of(length, taps);
  if (partials_out) *partials_out = partials_of(rows, channels, length, taps, partials);
  if (carry_min) *carry_min = carry_min_of(taps);
  return TFFT_OK;
}

int tfft_cconv_grad_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_cconv_grad_opts", kRules);
  if (rc) return rc;
  return copy_text("cconv4096:4096 x " + std::to_string(segments_of(length, taps)) + " | partials " +
                       std::to_string(partials_of(rows, channels, length, taps, partials)),
                   buf, bytes);
}

int tfft_cconv_grad_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_cconv_grad_opts* opts,
                           tfft_cconv_grad** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_cconv_grad_opts o = TFFT_CCONV_GRAD_OPTS_INIT;
  int rc = take_opts(opts, "tfft_cconv_grad_opts", o);
  if (rc) return rc;
  rc = check_shape(rows, channels, length, taps, o.flags, "tfft_cconv_grad_opts", kRules);
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.x_seq_stride, "x");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.g_seq_stride, "g");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.dx_seq_stride, "dx");
  if (rc == TFFT_OK) rc = check_context(taps, o.history, "history");
  if (rc == TFFT_OK) rc = check_context_stride(o.history, o.hist_seq_stride, "history", "hist");
  if (rc == TFFT_OK) rc = check_context(taps, o.future, "future");
  if (rc == TFFT_OK) rc = check_context_stride(o.future, o.fut_seq_stride, "future", "fut");
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_cconv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_cconv_grad* p = new tfft_cconv_grad;
  set_shape(p, rows, channels, length, taps, o.launch_iters, device_id);
  p->per_channel = (rows + 1) / 2 * p->segments;
  p->partials = partials_of(rows, channels, length, taps, o.partials);
  p->kpad = kpad_of(taps);
  p->ws_need = static_cast<size_t>(channels * p->partials * p->kpad * 4);
  p->x_stride = o.x_seq_stride ? o.x_seq_stride : length;
  p->g_stride = o.g_seq_stride ? o.g_seq_stride : length;
  p->dx_stride = o.dx_seq_stride ? o.dx_seq_stride : length;
  p->history = o.history;
  p->hist_stride = o.hist_seq_stride ? o.hist_seq_stride : o.history;
  p->future = o.future;
  p->fut_stride = o.fut_seq_stride ? o.fut_seq_stride : o.future;
  rc = create_base(p);
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  if (rc == TFFT_OK && (hipFuncSetAttribute(reinterpret_cast<const void*>(cconv4096::dgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            k4096::kLdsBytes) != hipSuccess ||
                        hipFuncSetAttribute(reinterpret_cast<const void*>(cconv4096::wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            cconv4096::kWgradLdsBytes) != hipSuccess))
    rc = fail(TFFT_ERR_HIP, "hipFuncSetAttribute(dgrad_kernel / wgrad_kernel) failed");
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_cconv_grad_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_cconv_grad_destroy(tfft_cconv_grad* p) {
  if (!p) return;
  destroy_base(p);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_cconv_grad_set_taps(tfft_cconv_grad* p, const void* taps, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return set_taps(p, taps, nullptr, stream, true);
}

int tfft_cconv_grad_spectrum(const tfft_cconv_grad* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return copy_spectrum(p, h_re, h_im, "tfft_cconv_grad_set_taps");
}

size_t tfft_cconv_grad_workspace_bytes(const tfft_cconv_grad* p) { return p ? p->ws_need : 0; }

int tfft_cconv_grad_set_workspace(tfft_cconv_grad* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_set(p, device_ptr, bytes);
}

int tfft_cconv_grad_prepare(tfft_cconv_grad* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_prepare(p);
}

int tfft_cconv_grad_exec_input_grad(const tfft_cconv_grad* p, const void* g, const void* fut, void* dx, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_cconv_grad_set_taps first");
  if (!g || !dx) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(dx)) & 15) return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  if (fut && p->future == 0) return fail(TFFT_ERR_ARG, "g_future must be NULL: the plan was created with future = 0");
  if (reinterpret_cast<uintptr_t>(fut) & 15) return fail(TFFT_ERR_ARG, "g_future must be 16-byte aligned");
  const uint64_t seqs = p->rows * p->channels;
  // segment s reads, beyond its hop, the start of the stretch segment s + 1 writes, and segments run in no defined order
  if (g == dx || seqs_overlap(g, p->g_stride, p->length, dx, p->dx_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "g and dx overlap (the input gradient cannot run in place: a segment reads what its successor overwrites)");
  if (fut && seqs_overlap(fut, p->fut_stride, p->future, dx, p->dx_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "g_future and dx overlap (the future may alias g, never dx)");
  const int rc = check_current(p->device);
  if (rc) return rc;
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipLaunchKernelGGL(cconv4096::dgrad_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(g), static_cast<const uint16_t*>(fut ? fut : g), static_cast<uint16_t*>(dx), p->g_stride,
                     fut ? p->fut_stride : p->g_stride, p->dx_stride, static_cast<uint32_t>(p->rows), static_cast<uint32_t>(p->channels),
                     geometry_of(p), static_cast<int32_t>(fut ? p->future / 8 : 0), static_cast<uint32_t>(p->items), live,
                     static_cast<const uint8_t*>(p->d_tables), p->d_filter);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_cconv_grad_exec_tap_grad(const tfft_cconv_grad* p, const void* x, const void* hist, const void* g, void* dh, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!x || !g || !dh) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(g)) & 15) return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(dh) & 3) return fail(TFFT_ERR_ARG, "the tap gradient must be 4-byte aligned");
  if (hist && p->history == 0) return fail(TFFT_ERR_ARG, "x_hist must be NULL: the plan was created with history = 0");
  if (reinterpret_cast<uintptr_t>(hist) & 15) return fail(TFFT_ERR_ARG, "x_hist must be 16-byte aligned");
  const uint64_t seqs = p->rows * p->channels, dh_bytes = p->channels * p->taps * 4;
  if (block_overlaps(dh, dh_bytes, x, p->x_stride, seqs, p->length) || block_overlaps(dh, dh_bytes, g, p->g_stride, seqs, p->length) ||
      block_overlaps(dh, dh_bytes, hist, p->hist_stride, seqs, p->history))
    return fail(TFFT_ERR_ARG, "the tap gradient overlaps x, x_hist or g");
  int rc = check_current(p->device);
  if (rc == TFFT_OK) rc = ws_ensure(p);
  if (rc) return rc;
  if (block_overlaps(p->ws, p->ws_need, x, p->x_stride, seqs, p->length) || block_overlaps(p->ws, p->ws_need, g, p->g_stride, seqs, p->length) ||
      block_overlaps(p->ws, p->ws_need, hist, p->hist_stride, seqs, p->history) ||
      blocks_overlap(dh, dh_bytes, p->ws, p->ws_need))
    return fail(TFFT_ERR_ARG, "the workspace overlaps x, x_hist, g or the tap gradient");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t live, grid;
  wgrad_shape(p->channels * p->partials, p->num_cus, cconv4096::kWgradWaves, live, grid);
  hipLaunchKernelGGL(cconv4096::wgrad_kernel, dim3(grid), dim3(cconv4096::kWgradThreads), cconv4096::kWgradLdsBytes, s, static_cast<const uint16_t*>(x),
                     static_cast<const uint16_t*>(hist ? hist : x), static_cast<const uint16_t*>(g), p->x_stride, hist ? p->hist_stride : p->x_stride,
                     p->g_stride, static_cast<uint32_t>(p->rows), static_cast<uint32_t>(p->channels), geometry_of(p),
                     static_cast<int32_t>(hist ? p->history / 8 : 0), static_cast<uint32_t>(p->partials), static_cast<uint32_t>(p->per_channel),
                     static_cast<uint32_t>(p->channels * p->partials), live, static_cast<int32_t>(p->kpad / 8), static_cast<uint32_t>(p->kpad),
                     static_cast<const uint8_t*>(p->d_tables), static_cast<float*>(p->ws));
  CONV_HIP(hipGetLastError());
  const uint64_t total = p->channels * p->taps;
  hipLaunchKernelGGL(cconv4096::wreduce_kernel, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(p->ws),
                     static_cast<float*>(dh), static_cast<uint32_t>(p->channels), static_cast<uint32_t>(p->taps), static_cast<uint32_t>(p->partials),
                     static_cast<uint32_t>(p->kpad));
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_cconv_grad_num_launches(const tfft_cconv_grad* p) { return p ? 3 : 0; }

int tfft_cconv_grad_kernels(const tfft_cconv_grad* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("cconv4096::dgrad_kernel\ncconv4096::wgrad_kernel\ncconv4096::wreduce_kernel\n", 3, buf, bytes);
}

}  // extern "C"
