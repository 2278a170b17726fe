// tfft_gbconv.hip — host side and C ABI (include/tfft_gbconv.h) of the gradient add-on of the GATED overlap-save causal
// convolution, libtfft_gbconv.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp, header only. It links neither libtfft_bconv.so nor libtfft_gsconv.so: the
// geometry, the checks, the launch shapes and the fp64 spectrum builder (the skip folded into tap 0) come from
// conv/host_math.hpp and conv/host_plumbing.hpp, the two headers every convolution library includes, and
// tests/test_gbconv_host.py and tests/test_gpu_gbconv.py hold them to the shipped code (the geometry and the refusals on the
// host, the spectrum to tfft_gconv_spectrum_host bit for bit).
#include "../../include/tfft_gbconv.h"
#include "gbconv4096.hpp"
#include "../conv/host_plumbing.hpp"

namespace {

static_assert(TFFT_GBCONV_MAX_TAPS == kMaxTaps, "include/tfft_gbconv.h and conv/host_math.hpp disagree on the longest filter");
constexpr int kGates = TFFT_GBCONV_PRE_GATE | TFFT_GBCONV_POST_GATE;
constexpr shape_rules kRules = {kGates, "takes TFFT_GBCONV_PRE_GATE and TFFT_GBCONV_POST_GATE only", "tfft_gconv_plan_create"};

std::string gate_text(int flags) {
  if (!(flags & kGates)) return "";
  return std::string(":") + ((flags & TFFT_GBCONV_PRE_GATE) ? "pre" : "") + ((flags & kGates) == kGates ? "+" : "") +
         ((flags & TFFT_GBCONV_POST_GATE) ? "post" : "");
}

}  // namespace

struct tfft_gbconv_plan {
  uint64_t rows = 0, channels = 0, length = 0, taps = 0, halo = 0, hop = 0, segments = 0, items = 0;
  uint64_t x_stride = 0, pre_stride = 0, gy_stride = 0, post_stride = 0, dx_stride = 0, dpre_stride = 0;
  uint64_t partials = 0, per_channel = 0, kpad = 0;
  uint32_t launch_iters = 0;
  int device = 0, num_cus = 256;
  bool pre = false, post = false;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // conj(H'): [channels][RE 4096 | IM 4096] in filter_slot order (input gradient)
  uint16_t* d_spec = nullptr;        // H': [RE: channels x 4096 | IM: channels x 4096], natural bin order (tfft_gbconv_plan_spectrum)
  bool have_taps = false;
  size_t ws_need = 0;                // channels * partials * kpad floats
  mutable std::mutex ws_mutex;
  mutable void* ws = nullptr;
  mutable bool ws_owned = false;
};

namespace {

// the instantiations a plan launches
const void* plan_dgrad(const tfft_gbconv_plan* p) {
  if (p->pre)
    return p->post ? reinterpret_cast<const void*>(gbconv4096::dgrad_kernel<true, true>)
                   : reinterpret_cast<const void*>(gbconv4096::dgrad_kernel<true, false>);
  return p->post ? reinterpret_cast<const void*>(gbconv4096::dgrad_kernel<false, true>)
                 : reinterpret_cast<const void*>(gbconv4096::dgrad_kernel<false, false>);
}
const void* plan_wgrad(const tfft_gbconv_plan* p) {
  if (p->pre)
    return p->post ? reinterpret_cast<const void*>(gbconv4096::wgrad_kernel<true, true>)
                   : reinterpret_cast<const void*>(gbconv4096::wgrad_kernel<true, false>);
  return p->post ? reinterpret_cast<const void*>(gbconv4096::wgrad_kernel<false, true>)
                 : reinterpret_cast<const void*>(gbconv4096::wgrad_kernel<false, false>);
}

int create_device(tfft_gbconv_plan* p) {
  const int rc = create_base(p);
  if (rc) return rc;
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(plan_dgrad(p), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  CONV_HIP(hipFuncSetAttribute(plan_wgrad(p), hipFuncAttributeMaxDynamicSharedMemorySize, gbconv4096::kWgradLdsBytes));
  return TFFT_OK;
}

gbconv4096::geometry geometry_of(const tfft_gbconv_plan* p) {
  return {static_cast<int32_t>(p->length / 8), static_cast<int32_t>(p->halo / 8), static_cast<int32_t>(p->hop / 8), static_cast<int32_t>(p->segments)};
}

}  // namespace

extern "C" {

const char* tfft_gbconv_last_error(void) { return g_err.c_str(); }

int tfft_gbconv_geometry(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, uint64_t* halo, uint64_t* hop,
                        uint64_t* segments, uint64_t* partials_out) {
  g_err.clear();
  const int rc = check_shape(rows, channels, length, taps, 0, "tfft_gbconv_opts", kRules);
  if (rc) return rc;
  if (halo) *halo = halo_of(taps);
  if (hop) *hop = hop_of(taps);
  if (segments) *segments = segments_of(length, taps);
  if (partials_out) *partials_out = partials_of(rows, channels, length, taps, partials);
  return TFFT_OK;
}

int tfft_gbconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_gbconv_opts", kRules);
  if (rc) return rc;
  return copy_text("gbconv4096:4096" + gate_text(flags) + " x " + std::to_string(segments_of(length, taps)) + " | partials " +
                       std::to_string(partials_of(rows, channels, length, taps, partials)),
                   buf, bytes);
}

int tfft_gbconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_gbconv_opts* opts,
                           tfft_gbconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_gbconv_opts o = TFFT_GBCONV_OPTS_INIT;
  int rc = take_opts(opts, "tfft_gbconv_opts", o);
  if (rc) return rc;
  rc = check_shape(rows, channels, length, taps, o.flags, "tfft_gbconv_opts", kRules);
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.x_seq_stride, "x");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.pre_seq_stride, "pre");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.gy_seq_stride, "gy");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.post_seq_stride, "post");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.dx_seq_stride, "dx");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.dpre_seq_stride, "dpre");
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_gbconv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_gbconv_plan* p = new tfft_gbconv_plan;
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
  p->pre_stride = o.pre_seq_stride ? o.pre_seq_stride : length;
  p->gy_stride = o.gy_seq_stride ? o.gy_seq_stride : length;
  p->post_stride = o.post_seq_stride ? o.post_seq_stride : length;
  p->dx_stride = o.dx_seq_stride ? o.dx_seq_stride : length;
  p->dpre_stride = o.dpre_seq_stride ? o.dpre_seq_stride : length;
  p->pre = (o.flags & TFFT_GBCONV_PRE_GATE) != 0;
  p->post = (o.flags & TFFT_GBCONV_POST_GATE) != 0;
  p->launch_iters = o.launch_iters;
  p->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
  rc = create_device(p);
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_gbconv_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_gbconv_plan_destroy(tfft_gbconv_plan* p) {
  if (!p) return;
  destroy_base(p);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_gbconv_plan_set_taps(tfft_gbconv_plan* p, const void* taps, const void* skip, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return set_taps(p, taps, skip, stream, true);
}

int tfft_gbconv_plan_spectrum(const tfft_gbconv_plan* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return copy_spectrum(p, h_re, h_im, "tfft_gbconv_plan_set_taps");
}

size_t tfft_gbconv_plan_workspace_bytes(const tfft_gbconv_plan* p) { return p ? p->ws_need : 0; }

int tfft_gbconv_plan_set_workspace(tfft_gbconv_plan* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_set(p, device_ptr, bytes);
}

int tfft_gbconv_plan_prepare(tfft_gbconv_plan* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_prepare(p);
}

int tfft_gbconv_exec_input_grad(const tfft_gbconv_plan* p, const void* gy, const void* post, const void* x, const void* pre, void* dx,
                                void* dpre, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_gbconv_plan_set_taps first");
  if (!gy || !dx) return fail(TFFT_ERR_ARG, "null data pointer");
  if (p->post && !post) return fail(TFFT_ERR_ARG, "the plan has a post gate (TFFT_GBCONV_POST_GATE) and the post pointer is null");
  if (!p->post && post) return fail(TFFT_ERR_ARG, "the plan has no post gate and the post pointer is not null");
  if (p->pre && !pre) return fail(TFFT_ERR_ARG, "the plan has a pre gate (TFFT_GBCONV_PRE_GATE) and the pre pointer is null");
  if (p->pre && !x) return fail(TFFT_ERR_ARG, "the plan has a pre gate (TFFT_GBCONV_PRE_GATE) and the x pointer is null");
  if (!p->pre && pre) return fail(TFFT_ERR_ARG, "the plan has no pre gate and the pre pointer is not null");
  if (!p->pre && x) return fail(TFFT_ERR_ARG, "the plan has no pre gate and the x pointer is not null");
  if (!p->pre && dpre) return fail(TFFT_ERR_ARG, "the plan has no pre gate and the dpre pointer is not null");
  if ((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(post) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(pre) |
       reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dpre)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  const uint64_t seqs = p->rows * p->channels;
  // segment s reads, beyond its hop, the start of the stretch segment s + 1 writes, and segments run in no defined order; a gate is
  // read while other items' results are written: no output shares a half with an input or with the other output
  struct seq_set {
    const void* ptr;
    uint64_t stride;
    const char* name;
  };
  const seq_set inputs[4] = {{gy, p->gy_stride, "gy"}, {post, p->post_stride, "post"}, {x, p->x_stride, "x"}, {pre, p->pre_stride, "pre"}};
  const seq_set outputs[2] = {{dx, p->dx_stride, "dx"}, {dpre, p->dpre_stride, "dpre"}};
  for (const seq_set& o : outputs) {
    if (!o.ptr) continue;
    for (const seq_set& i : inputs)
      if (i.ptr && (i.ptr == o.ptr || seqs_overlap(i.ptr, i.stride, p->length, o.ptr, o.stride, p->length, seqs)))
        return fail(TFFT_ERR_ARG, std::string(i.name) + " and " + o.name +
                                      " overlap (the input gradient cannot run in place: a segment reads what its successor overwrites)");
  }
  if (dpre && (dx == dpre || seqs_overlap(dx, p->dx_stride, p->length, dpre, p->dpre_stride, p->length, seqs))) return fail(TFFT_ERR_ARG, "dx and dpre overlap");
  const int rc = check_current(p->device);
  if (rc) return rc;
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const gbconv4096::dgrad_strides strides = {p->gy_stride, p->post_stride, p->x_stride, p->pre_stride, p->dx_stride, p->dpre_stride};
  const gbconv4096::geometry geo = geometry_of(p);
  const uint32_t rows = static_cast<uint32_t>(p->rows), channels = static_cast<uint32_t>(p->channels), items = static_cast<uint32_t>(p->items);
  const uint8_t* const tables = static_cast<const uint8_t*>(p->d_tables);
#define GBCONV_LAUNCH(PRE, POST)                                                                                                           \
  hipLaunchKernelGGL((gbconv4096::dgrad_kernel<PRE, POST>), dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, s,                        \
                     static_cast<const uint16_t*>(gy), static_cast<const uint16_t*>(post), static_cast<const uint16_t*>(x),                \
                     static_cast<const uint16_t*>(pre), static_cast<uint16_t*>(dx), static_cast<uint16_t*>(dpre), strides, rows, channels, \
                     geo, items, live, tables, p->d_filter)
  if (p->pre && p->post)
    GBCONV_LAUNCH(true, true);
  else if (p->pre)
    GBCONV_LAUNCH(true, false);
  else if (p->post)
    GBCONV_LAUNCH(false, true);
  else
    GBCONV_LAUNCH(false, false);
#undef GBCONV_LAUNCH
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_gbconv_exec_tap_grad(const tfft_gbconv_plan* p, const void* x, const void* pre, const void* gy, const void* post, void* dh, void* dskip,
                              void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!x || !gy || !dh) return fail(TFFT_ERR_ARG, "null data pointer");
  if (p->pre && !pre) return fail(TFFT_ERR_ARG, "the plan has a pre gate (TFFT_GBCONV_PRE_GATE) and the pre pointer is null");
  if (p->post && !post) return fail(TFFT_ERR_ARG, "the plan has a post gate (TFFT_GBCONV_POST_GATE) and the post pointer is null");
  if (!p->pre && pre) return fail(TFFT_ERR_ARG, "the plan has no pre gate and the pre pointer is not null");
  if (!p->post && post) return fail(TFFT_ERR_ARG, "the plan has no post gate and the post pointer is not null");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(pre) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(post)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(dh) | reinterpret_cast<uintptr_t>(dskip)) & 3) return fail(TFFT_ERR_ARG, "the tap gradient and the skip gradient must be 4-byte aligned");
  const uint64_t seqs = p->rows * p->channels, dh_bytes = p->channels * p->taps * 4, dskip_bytes = p->channels * 4;
  struct seq_set {
    const void* ptr;
    uint64_t stride;
  };
  const seq_set inputs[4] = {{x, p->x_stride}, {pre, p->pre_stride}, {gy, p->gy_stride}, {post, p->post_stride}};
  for (const seq_set& i : inputs) {
    if (!i.ptr) continue;
    if (block_overlaps(dh, dh_bytes, i.ptr, i.stride, seqs, p->length)) return fail(TFFT_ERR_ARG, "the tap gradient overlaps x, pre, gy or post");
    if (dskip && block_overlaps(dskip, dskip_bytes, i.ptr, i.stride, seqs, p->length))
      return fail(TFFT_ERR_ARG, "the skip gradient overlaps x, pre, gy or post");
  }
  if (dskip && blocks_overlap(dh, dh_bytes, dskip, dskip_bytes)) return fail(TFFT_ERR_ARG, "the tap gradient and the skip gradient overlap");
  int rc = check_current(p->device);
  if (rc == TFFT_OK) rc = ws_ensure(p);
  if (rc) return rc;
  for (const seq_set& i : inputs)
    if (i.ptr && block_overlaps(p->ws, p->ws_need, i.ptr, i.stride, seqs, p->length))
      return fail(TFFT_ERR_ARG, "the workspace overlaps x, pre, gy, post, the tap gradient or the skip gradient");
  if (blocks_overlap(p->ws, p->ws_need, dh, dh_bytes) || (dskip && blocks_overlap(p->ws, p->ws_need, dskip, dskip_bytes)))
    return fail(TFFT_ERR_ARG, "the workspace overlaps x, pre, gy, post, the tap gradient or the skip gradient");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t live, grid;
  wgrad_shape(p->channels * p->partials, p->num_cus, gbconv4096::kWgradWaves, live, grid);
  const gbconv4096::wgrad_strides strides = {p->x_stride, p->pre_stride, p->gy_stride, p->post_stride};
  const gbconv4096::geometry geo = geometry_of(p);
  const uint32_t rows = static_cast<uint32_t>(p->rows), channels = static_cast<uint32_t>(p->channels);
  const uint8_t* const tables = static_cast<const uint8_t*>(p->d_tables);
#define GBCONV_LAUNCH(PRE, POST)                                                                                                              \
  hipLaunchKernelGGL((gbconv4096::wgrad_kernel<PRE, POST>), dim3(grid), dim3(gbconv4096::kWgradThreads), gbconv4096::kWgradLdsBytes, s,       \
                     static_cast<const uint16_t*>(x), static_cast<const uint16_t*>(pre), static_cast<const uint16_t*>(gy),                    \
                     static_cast<const uint16_t*>(post), strides, rows, channels, geo, static_cast<uint32_t>(p->partials),                    \
                     static_cast<uint32_t>(p->per_channel), static_cast<uint32_t>(p->channels * p->partials), live,                           \
                     static_cast<int32_t>(p->kpad / 8), static_cast<uint32_t>(p->kpad), tables, static_cast<float*>(p->ws))
  if (p->pre && p->post)
    GBCONV_LAUNCH(true, true);
  else if (p->pre)
    GBCONV_LAUNCH(true, false);
  else if (p->post)
    GBCONV_LAUNCH(false, true);
  else
    GBCONV_LAUNCH(false, false);
#undef GBCONV_LAUNCH
  CONV_HIP(hipGetLastError());
  const uint64_t total = p->channels * p->taps;
  hipLaunchKernelGGL(gbconv4096::wreduce_kernel, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(p->ws),
                     static_cast<float*>(dh), static_cast<float*>(dskip), channels, static_cast<uint32_t>(p->taps),
                     static_cast<uint32_t>(p->partials), static_cast<uint32_t>(p->kpad));
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_gbconv_plan_num_launches(const tfft_gbconv_plan* p) { return p ? 3 : 0; }

int tfft_gbconv_plan_kernels(const tfft_gbconv_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  const std::string inst = std::string("<") + tf_text(p->pre) + ", " + tf_text(p->post) + ">\n";
  return kernel_names("gbconv4096::dgrad_kernel" + inst + "gbconv4096::wgrad_kernel" + inst + "gbconv4096::wreduce_kernel\n", 3, buf, bytes);
}

}  // extern "C"
