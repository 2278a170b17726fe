// tfft_gconv.hip — host side and C ABI (include/tfft_gconv.h) of the gated causal convolution add-on, libtfft_gconv.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (the sub-plan of the composed path,
// tfft_device_check, tfft_abi_version); from csrc/ it takes k4096.hpp, header only, for the device helpers and
// the constant tables of the fused kernel (the add-on uploads a copy of its own). The host code is that of lconv/tfft_lconv.hip
// (which this library does not link) with the gates, their strides and the skip weight added; what the two share (the fp64
// spectrum builder, the overlap test, the error plumbing, the launch shape) comes from conv/host_math.hpp and
// conv/host_plumbing.hpp, the two headers every convolution library includes.
#include "../../include/tfft_gconv.h"
#include "gconv4096.hpp"
#include "gate_copy.hpp"
#include "../conv/host_plumbing.hpp"

namespace {

int check_shape(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int flags) {
  if (length < 8 || length % 8) return fail(TFFT_ERR_ARG, "length must be a multiple of 8 and at least 8");
  if (taps == 0) return fail(TFFT_ERR_ARG, "taps must be at least 1");
  if (flags & ~(TFFT_GCONV_PRE_GATE | TFFT_GCONV_POST_GATE | TFFT_GCONV_COMPOSED)) return fail(TFFT_ERR_ARG, "unknown flag bits (" + std::to_string(flags) + ")");
  const int rc = check_rows_channels(rows, channels);
  if (rc) return rc;
  if (!fft_length(length, taps))
    return fail(TFFT_ERR_ARG, "the transform length (the power of two >= length + taps - 1) must not exceed 2^26");
  return TFFT_OK;
}

// the fused kernel takes every shape that fits its 4096-point transform with the kept half in front: it moves L halves per sequence
// and gate each way whatever the padding, so a shorter transform (three steps and two copies) has nothing to offer
inline bool fused_shape(uint64_t length, uint64_t taps, int flags) {
  return length <= 2048 && length + taps - 1 <= 4096 && !(flags & TFFT_GCONV_COMPOSED);
}
inline uint64_t plan_length(uint64_t length, uint64_t taps, int flags) { return fused_shape(length, taps, flags) ? 4096 : fft_length(length, taps); }

}  // namespace

struct tfft_gconv_plan {
  uint64_t rows = 0, channels = 0, length = 0, taps = 0, n = 0, items = 0, in_stride = 0, out_stride = 0, pre_stride = 0, post_stride = 0;
  uint32_t launch_iters = 0;
  int device = 0, flags = 0, num_cus = 256;
  bool fused = false, pre = false, post = false;
  void* d_tables = nullptr;          // fused: F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // fused: [channels][RE 4096 | IM 4096] in filter_slot order
  uint16_t* d_spec = nullptr;        // [RE: channels x n | IM: channels x n], natural bin order (tfft_gconv_plan_spectrum)
  bool have_taps = false;
  tfft_conv_plan* sub = nullptr;     // composed: in place on the blocks
  size_t block_bytes = 0, sub_bytes = 0;       // workspace = [blocks: items x (RE n | IM n)] [the sub-plan's workspace]
  mutable std::mutex ws_mutex;
  mutable void* ws = nullptr;
  mutable size_t ws_bytes = 0;
  mutable bool ws_owned = false;
};

namespace {

int bind_workspace(const tfft_gconv_plan* p) {
  if (!p->sub_bytes) return TFFT_OK;
  return pass_conv(tfft_conv_plan_set_workspace(p->sub, static_cast<uint8_t*>(p->ws) + p->block_bytes, p->sub_bytes));
}

int ensure_workspace(const tfft_gconv_plan* p) {
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  const size_t need = p->block_bytes + p->sub_bytes;
  if (!need || p->ws) return TFFT_OK;
  void* mem = nullptr;
  CONV_HIP(hipMalloc(&mem, need));
  p->ws = mem;
  p->ws_bytes = need;
  p->ws_owned = true;
  return bind_workspace(p);
}

// the instantiation a plan launches
const void* fused_kernel(const tfft_gconv_plan* p) {
  if (p->pre) return p->post ? reinterpret_cast<const void*>(gconv4096::gconv4096_kernel<true, true>) : reinterpret_cast<const void*>(gconv4096::gconv4096_kernel<true, false>);
  return p->post ? reinterpret_cast<const void*>(gconv4096::gconv4096_kernel<false, true>) : reinterpret_cast<const void*>(gconv4096::gconv4096_kernel<false, false>);
}

int create_fused(tfft_gconv_plan* p) {
  std::vector<uint8_t> blob;
  k4096::build_tables(blob);
  CONV_HIP(hipMalloc(&p->d_tables, k4096::kOffF1n));
  CONV_HIP(hipMemcpy(p->d_tables, blob.data(), k4096::kOffF1n, hipMemcpyHostToDevice));
  CONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_filter), static_cast<size_t>(p->channels) * 8192 * 2));
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(fused_kernel(p), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  return TFFT_OK;
}

int create_composed(tfft_gconv_plan* p) {
  const int rc = pass_conv(tfft_conv_plan_create(p->n, p->items, p->channels, p->device, 0, 0, 0, &p->sub));
  if (rc) return rc;
  p->block_bytes = round256(static_cast<size_t>(p->items) * p->n * 4);
  p->sub_bytes = round256(tfft_conv_plan_workspace_bytes(p->sub));
  return TFFT_OK;
}

uint32_t copy_grid(const tfft_gconv_plan* p, uint64_t total) {
  return static_cast<uint32_t>(std::min<uint64_t>((total + gate_copy::kThreads - 1) / gate_copy::kThreads, static_cast<uint64_t>(p->num_cus) * 32));
}

}  // namespace

extern "C" {

const char* tfft_gconv_last_error(void) { return g_err.c_str(); }

uint64_t tfft_gconv_fft_length(uint64_t length, uint64_t taps) { return fft_length(length, taps); }

int tfft_gconv_spectrum_host(const uint16_t* taps, uint64_t num_taps, const uint16_t* skip, uint64_t n, uint16_t* out_re, uint16_t* out_im) {
  g_err.clear();
  if (!taps || !out_re || !out_im) return fail(TFFT_ERR_ARG, "null pointer");
  if (!is_pow2(n) || n < 2 || n > kMaxN) return fail(TFFT_ERR_ARG, "n must be a power of two in 2 .. 2^26");
  if (num_taps == 0 || num_taps > n) return fail(TFFT_ERR_ARG, "the number of taps must be in [1, n]");
  spectrum(taps, num_taps, skip ? *skip : uint16_t{0}, n, out_re, out_im);
  return TFFT_OK;
}

int tfft_gconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  int rc = check_shape(rows, channels, length, taps, flags);
  if (rc) return rc;
  const uint64_t n = plan_length(length, taps, flags);
  std::string out;
  if (fused_shape(length, taps, flags)) {
    out = "gconv4096:4096";
    if (flags & (TFFT_GCONV_PRE_GATE | TFFT_GCONV_POST_GATE))
      out += std::string(":") + ((flags & TFFT_GCONV_PRE_GATE) ? "pre" : "") + ((flags & TFFT_GCONV_PRE_GATE) && (flags & TFFT_GCONV_POST_GATE) ? "+" : "") +
             ((flags & TFFT_GCONV_POST_GATE) ? "post" : "");
  } else {
    char sub[512];
    rc = pass_conv(tfft_conv_describe(n, (rows + 1) / 2 * channels, channels, 0, sub, sizeof(sub)));
    if (rc) return rc;
    out = std::string((flags & TFFT_GCONV_PRE_GATE) ? "pack:pre | " : "pack | ") + sub + ((flags & TFFT_GCONV_POST_GATE) ? " | crop:post" : " | crop");
  }
  return copy_text(out, buf, bytes);
}

int tfft_gconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_gconv_opts* opts,
                           tfft_gconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_gconv_opts o = TFFT_GCONV_OPTS_INIT;
  int rc = take_opts(opts, "tfft_gconv_opts", o);
  if (rc) return rc;
  rc = check_shape(rows, channels, length, taps, o.flags);
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.in_seq_stride, "in");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.out_seq_stride, "out");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.pre_seq_stride, "pre");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.post_seq_stride, "post");
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_gconv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_gconv_plan* p = new tfft_gconv_plan;
  p->rows = rows;
  p->channels = channels;
  p->length = length;
  p->taps = taps;
  p->n = plan_length(length, taps, o.flags);
  p->items = (rows + 1) / 2 * channels;
  p->in_stride = o.in_seq_stride ? o.in_seq_stride : length;
  p->out_stride = o.out_seq_stride ? o.out_seq_stride : length;
  p->pre_stride = o.pre_seq_stride ? o.pre_seq_stride : length;
  p->post_stride = o.post_seq_stride ? o.post_seq_stride : length;
  p->pre = (o.flags & TFFT_GCONV_PRE_GATE) != 0;
  p->post = (o.flags & TFFT_GCONV_POST_GATE) != 0;
  p->launch_iters = o.launch_iters;
  p->device = device_id;
  p->flags = o.flags;
  p->fused = fused_shape(length, taps, o.flags);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
  rc = p->fused ? create_fused(p) : create_composed(p);
  if (rc == TFFT_OK) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_spec), static_cast<size_t>(channels) * p->n * 4);
    if (e != hipSuccess) rc = hip_fail(e, "hipMalloc(filter spectrum)");
  }
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_gconv_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_gconv_plan_destroy(tfft_gconv_plan* p) {
  if (!p) return;
  tfft_conv_plan_destroy(p->sub);
  destroy_base(p);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_gconv_plan_set_taps(tfft_gconv_plan* p, const void* taps, const void* skip, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!taps) return fail(TFFT_ERR_ARG, "null taps pointer");
  const int cur_rc = check_current(p->device);
  if (cur_rc) return cur_rc;
  const size_t plane = static_cast<size_t>(p->channels) * p->n;
  std::vector<uint16_t> h(static_cast<size_t>(p->channels) * p->taps), d(p->channels, 0), spec(2 * plane);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // through the host: the spectrum is built once per filter, not per execution. Everything enqueued on `stream` before the call
  // (the kernel that produced the taps) is waited for; executions still in flight keep reading the old spectrum until then, so the
  // device is drained before it is replaced.
  CONV_HIP(hipMemcpyAsync(h.data(), taps, h.size() * 2, hipMemcpyDeviceToHost, s));
  if (skip) CONV_HIP(hipMemcpyAsync(d.data(), skip, d.size() * 2, hipMemcpyDeviceToHost, s));
  CONV_HIP(hipStreamSynchronize(s));
  for (uint64_t c = 0; c < p->channels; ++c) spectrum(h.data() + c * p->taps, p->taps, d[c], p->n, spec.data() + c * p->n, spec.data() + plane + c * p->n);
  if (p->have_taps) CONV_HIP(hipDeviceSynchronize());
  CONV_HIP(hipMemcpy(p->d_spec, spec.data(), spec.size() * 2, hipMemcpyHostToDevice));
  if (p->fused) {
    std::vector<uint16_t> img(2 * plane);
    for (uint64_t c = 0; c < p->channels; ++c) filter_image(spec.data() + c * 4096, spec.data() + plane + c * 4096, false, img.data() + c * 8192);
    CONV_HIP(hipMemcpy(p->d_filter, img.data(), img.size() * 2, hipMemcpyHostToDevice));
  } else {
    const int rc = pass_conv(tfft_conv_plan_set_filter(p->sub, p->d_spec, p->d_spec + plane, stream));
    if (rc) return rc;
  }
  p->have_taps = true;
  return TFFT_OK;
}

int tfft_gconv_plan_spectrum(const tfft_gconv_plan* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!h_re || !h_im) return fail(TFFT_ERR_ARG, "null spectrum pointer");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_gconv_plan_set_taps first");
  const size_t plane = static_cast<size_t>(p->channels) * p->n;
  CONV_HIP(hipMemcpy(h_re, p->d_spec, plane * 2, hipMemcpyDeviceToDevice));
  CONV_HIP(hipMemcpy(h_im, p->d_spec + plane, plane * 2, hipMemcpyDeviceToDevice));
  CONV_HIP(hipDeviceSynchronize());
  return TFFT_OK;
}

uint64_t tfft_gconv_plan_fft_length(const tfft_gconv_plan* p) { return p ? p->n : 0; }

size_t tfft_gconv_plan_workspace_bytes(const tfft_gconv_plan* p) { return p ? p->block_bytes + p->sub_bytes : 0; }

int tfft_gconv_plan_set_workspace(tfft_gconv_plan* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  const size_t need = p->block_bytes + p->sub_bytes;
  if (device_ptr && bytes < need) return fail(TFFT_ERR_WORKSPACE, "workspace too small: " + std::to_string(need) + " bytes needed");
  if (reinterpret_cast<uintptr_t>(device_ptr) & 255) return fail(TFFT_ERR_ARG, "the workspace must be 256-byte aligned");
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  p->ws = need ? device_ptr : nullptr;
  p->ws_bytes = p->ws ? bytes : 0;
  p->ws_owned = false;
  return p->ws ? bind_workspace(p) : TFFT_OK;
}

int tfft_gconv_plan_prepare(tfft_gconv_plan* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (p->fused) return TFFT_OK;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(p->device));
  int rc = ensure_workspace(p);
  if (rc == TFFT_OK) rc = pass_conv(tfft_conv_plan_prepare(p->sub));
  (void)hipSetDevice(prev);
  return rc;
}

int tfft_gconv_exec(const tfft_gconv_plan* p, const void* in, const void* pre, const void* post, void* out, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_gconv_plan_set_taps first");
  if (!in || !out) return fail(TFFT_ERR_ARG, "null data pointer");
  if (p->pre && !pre) return fail(TFFT_ERR_ARG, "the plan has a pre gate (TFFT_GCONV_PRE_GATE) and the pre pointer is null");
  if (p->post && !post) return fail(TFFT_ERR_ARG, "the plan has a post gate (TFFT_GCONV_POST_GATE) and the post pointer is null");
  if (!p->pre && pre) return fail(TFFT_ERR_ARG, "the plan has no pre gate and the pre pointer is not null");
  if (!p->post && post) return fail(TFFT_ERR_ARG, "the plan has no post gate and the post pointer is not null");
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(pre) | reinterpret_cast<uintptr_t>(post)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  const uint64_t seqs = p->rows * p->channels;
  if (in == out) {
    if (p->in_stride != p->out_stride) return fail(TFFT_ERR_ARG, "in-place execution needs equal input and output sequence strides");
  } else if (seqs_overlap(in, p->in_stride, p->length, out, p->out_stride, p->length, seqs)) {
    return fail(TFFT_ERR_ARG, "input and output overlap without being identical (only exact in-place or disjoint sequences are supported)");
  }
  // a gate is read while other items' results are written: it shares no half with the output, not even in place
  if (pre && seqs_overlap(pre, p->pre_stride, p->length, out, p->out_stride, p->length, seqs)) return fail(TFFT_ERR_ARG, "the pre gate and the output overlap");
  if (post && seqs_overlap(post, p->post_stride, p->length, out, p->out_stride, p->length, seqs)) return fail(TFFT_ERR_ARG, "the post gate and the output overlap");
  const int cur_rc = check_current(p->device);
  if (cur_rc) return cur_rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t chunks = static_cast<uint32_t>(p->length / 8);
  const uint16_t* const x = static_cast<const uint16_t*>(in);
  const uint16_t* const gp = static_cast<const uint16_t*>(pre);
  const uint16_t* const gq = static_cast<const uint16_t*>(post);
  uint16_t* const y = static_cast<uint16_t*>(out);
  const uint32_t rows = static_cast<uint32_t>(p->rows), channels = static_cast<uint32_t>(p->channels);
  if (p->fused) {
    uint32_t live, grid;
    conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
    const uint32_t items = static_cast<uint32_t>(p->items);
    const uint8_t* const tables = static_cast<const uint8_t*>(p->d_tables);
#define GCONV_LAUNCH(PRE, POST)                                                                                                                  \
  hipLaunchKernelGGL((gconv4096::gconv4096_kernel<PRE, POST>), dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, s, x, gp, gq, y, p->in_stride, \
                     p->pre_stride, p->post_stride, p->out_stride, rows, channels, chunks, items, live, tables, p->d_filter)
    if (p->pre && p->post)
      GCONV_LAUNCH(true, true);
    else if (p->pre)
      GCONV_LAUNCH(true, false);
    else if (p->post)
      GCONV_LAUNCH(false, true);
    else
      GCONV_LAUNCH(false, false);
#undef GCONV_LAUNCH
    CONV_HIP(hipGetLastError());
    return TFFT_OK;
  }
  int rc = ensure_workspace(p);
  if (rc) return rc;
  uint16_t* const blocks = static_cast<uint16_t*>(p->ws);
  const uint32_t log_n8 = static_cast<uint32_t>(ilog2(p->n / 8));
  const uint64_t total_in = p->items * 2 * (p->n / 8), total_out = seqs * chunks;
  const dim3 grid_in(copy_grid(p, total_in)), grid_out(copy_grid(p, total_out)), block(gate_copy::kThreads);
  if (p->pre)
    hipLaunchKernelGGL(gate_copy::pack_kernel<true>, grid_in, block, 0, s, x, gp, blocks, p->in_stride, p->pre_stride, rows, channels, chunks, log_n8, total_in);
  else
    hipLaunchKernelGGL(gate_copy::pack_kernel<false>, grid_in, block, 0, s, x, gp, blocks, p->in_stride, p->pre_stride, rows, channels, chunks, log_n8, total_in);
  CONV_HIP(hipGetLastError());
  rc = pass_conv(tfft_conv_exec(p->sub, blocks, blocks + p->n, blocks, blocks + p->n, s));
  if (rc) return rc;
  if (p->post)
    hipLaunchKernelGGL(gate_copy::crop_kernel<true>, grid_out, block, 0, s, blocks, gq, y, p->post_stride, p->out_stride, channels, chunks, log_n8, total_out);
  else
    hipLaunchKernelGGL(gate_copy::crop_kernel<false>, grid_out, block, 0, s, blocks, gq, y, p->post_stride, p->out_stride, channels, chunks, log_n8, total_out);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_gconv_plan_num_launches(const tfft_gconv_plan* p) {
  if (!p) return 0;
  return p->fused ? 1 : 2 + tfft_conv_plan_num_launches(p->sub);
}

int tfft_gconv_plan_kernels(const tfft_gconv_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  std::string out;
  int lines = 1;
  if (p->fused) {
    out = std::string("gconv4096::gconv4096_kernel<") + tf_text(p->pre) + ", " + tf_text(p->post) + ">\n";
  } else {
    std::vector<char> tmp(1 << 16);
    const int a = tfft_conv_plan_kernels(p->sub, tmp.data(), tmp.size());
    if (a < 0) return pass_conv(a);
    out = std::string("gate_copy::pack_kernel<") + tf_text(p->pre) + ">\n" + tmp.data() + "gate_copy::crop_kernel<" + tf_text(p->post) + ">\n";
    lines = a + 2;
  }
  return kernel_names(out, lines, buf, bytes);
}

}  // extern "C"
