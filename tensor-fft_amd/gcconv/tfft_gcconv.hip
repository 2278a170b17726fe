// tfft_gcconv.hip — host side and C ABI (include/tfft_gcconv.h) of the gated carried convolution add-on, libtfft_gcconv.so: the
// forward plan of tfft_gsconv.hip and the gradient plan of tfft_gbconv.hip with a history in front of x and the pre gate and a
// future behind gy and the post gate, as tfft_cconv.hip carries them for the ungated operator.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp, header only. It links none of the other add-ons: the geometry, the checks, the
// launch shapes and the fp64 spectrum builder (the skip folded into tap 0) come from conv/host_math.hpp and
// conv/host_plumbing.hpp, the two headers every convolution library includes, and tests/test_gcconv_host.py and
// tests/test_gpu_gcconv.py hold them to the shipped code (the geometry and the refusals on the host; every result to the shipped
// plans' bit for bit).
#include "../../include/tfft_gcconv.h"
#include "gcconv4096.hpp"
#include "../conv/host_plumbing.hpp"

namespace {

static_assert(TFFT_GCCONV_MAX_TAPS == kMaxTaps, "include/tfft_gcconv.h and conv/host_math.hpp disagree on the longest filter");
constexpr int kGates = TFFT_GCCONV_PRE_GATE | TFFT_GCCONV_POST_GATE;
constexpr shape_rules kRules = {kGates, "takes TFFT_GCCONV_PRE_GATE and TFFT_GCCONV_POST_GATE only", "tfft_gconv_plan_create"};

// a set of sequences an execution reads or writes: `len` halves each, `stride` halves apart; a null ptr is no set
struct seq_set {
  const void* ptr;
  uint64_t stride, len;
  const char* name;
};

std::string gate_text(int flags) {
  if (!(flags & kGates)) return "";
  return std::string(":") + ((flags & TFFT_GCCONV_PRE_GATE) ? "pre" : "") + ((flags & kGates) == kGates ? "+" : "") +
         ((flags & TFFT_GCCONV_POST_GATE) ? "post" : "");
}

// what the two plan types share: the shape, the geometry, the gates and the device memory of tfft_gsconv_plan
struct plan_base {
  uint64_t rows = 0, channels = 0, length = 0, taps = 0, halo = 0, hop = 0, segments = 0, items = 0;
  uint32_t launch_iters = 0;
  int device = 0, num_cus = 256;
  bool pre = false, post = false;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // [channels][RE 4096 | IM 4096] in filter_slot order: H' (forward), conj(H') (gradient)
  uint16_t* d_spec = nullptr;        // H': [RE: channels x 4096 | IM: channels x 4096], natural bin order
  bool have_taps = false;
};

void set_shape(plan_base* p, uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, uint32_t launch_iters, int flags, int device_id) {
  p->rows = rows;
  p->channels = channels;
  p->length = length;
  p->taps = taps;
  p->halo = halo_of(taps);
  p->hop = hop_of(taps);
  p->segments = segments_of(length, taps);
  p->items = (rows + 1) / 2 * p->segments * channels;
  p->launch_iters = launch_iters;
  p->pre = (flags & TFFT_GCCONV_PRE_GATE) != 0;
  p->post = (flags & TFFT_GCCONV_POST_GATE) != 0;
  p->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
}

gcconv4096::geometry geometry_of(const plan_base* p) {
  return {static_cast<int32_t>(p->length / 8), static_cast<int32_t>(p->halo / 8), static_cast<int32_t>(p->hop / 8), static_cast<int32_t>(p->segments)};
}

// the gate pointers of a call against the gates of the plan: the messages of tfft_gsconv_exec
int check_gate(bool has, const void* ptr, const char* which, const char* flag) {
  if (has && !ptr) return fail(TFFT_ERR_ARG, std::string("the plan has a ") + which + " gate (" + flag + ") and the " + which + " pointer is null");
  if (!has && ptr) return fail(TFFT_ERR_ARG, std::string("the plan has no ") + which + " gate and the " + which + " pointer is not null");
  return TFFT_OK;
}

// a context pointer and its gate's: `ctx` needs a plan with n > 0; `gate_ctx` is non-NULL exactly when ctx is and the plan has the gate
int check_context_ptrs(const void* ctx, const void* gate_ctx, uint64_t n, bool has_gate, const char* ctx_name, const char* gate_ctx_name,
                       const char* field, const char* gate) {
  if (ctx && n == 0) return fail(TFFT_ERR_ARG, std::string(ctx_name) + " must be NULL: the plan was created with " + field + " = 0");
  if (gate_ctx && !has_gate) return fail(TFFT_ERR_ARG, std::string(gate_ctx_name) + " must be NULL: the plan has no " + gate + " gate");
  if (gate_ctx && !ctx) return fail(TFFT_ERR_ARG, std::string(gate_ctx_name) + " must be NULL when " + ctx_name + " is NULL: one " + field + " serves both");
  if (ctx && has_gate && !gate_ctx)
    return fail(TFFT_ERR_ARG, std::string(gate_ctx_name) + " is NULL but " + ctx_name + " is not and the plan has a " + gate + " gate: one " + field + " serves both");
  if ((reinterpret_cast<uintptr_t>(ctx) | reinterpret_cast<uintptr_t>(gate_ctx)) & 15)
    return fail(TFFT_ERR_ARG, std::string(ctx_name) + " and " + gate_ctx_name + " must be 16-byte aligned");
  return TFFT_OK;
}

}  // namespace

struct tfft_gcconv_plan : plan_base {
  uint64_t in_stride = 0, out_stride = 0, pre_stride = 0, post_stride = 0, history = 0, hist_stride = 0, pre_hist_stride = 0;
};

struct tfft_gcconv_grad : plan_base {
  uint64_t x_stride = 0, pre_stride = 0, gy_stride = 0, post_stride = 0, dx_stride = 0, dpre_stride = 0;
  uint64_t partials = 0, per_channel = 0, kpad = 0;
  uint64_t history = 0, hist_stride = 0, pre_hist_stride = 0, future = 0, fut_stride = 0, post_fut_stride = 0;
  size_t ws_need = 0;                // channels * partials * kpad floats
  mutable std::mutex ws_mutex;
  mutable void* ws = nullptr;
  mutable bool ws_owned = false;
};

namespace {

// the instantiations a plan launches
#define GCCONV_PICK(KERNEL)                                                                                        \
  (p->pre ? (p->post ? reinterpret_cast<const void*>(gcconv4096::KERNEL<true, true>)                               \
                     : reinterpret_cast<const void*>(gcconv4096::KERNEL<true, false>))                             \
          : (p->post ? reinterpret_cast<const void*>(gcconv4096::KERNEL<false, true>)                              \
                     : reinterpret_cast<const void*>(gcconv4096::KERNEL<false, false>)))
const void* plan_fwd(const plan_base* p) { return GCCONV_PICK(fwd_kernel); }
const void* plan_dgrad(const plan_base* p) { return GCCONV_PICK(dgrad_kernel); }
const void* plan_wgrad(const plan_base* p) { return GCCONV_PICK(wgrad_kernel); }
#undef GCCONV_PICK

}  // namespace

extern "C" {

const char* tfft_gcconv_last_error(void) { return g_err.c_str(); }

// ---- the forward plan

int tfft_gcconv_geometry(uint64_t length, uint64_t taps, uint64_t* halo, uint64_t* hop, uint64_t* segments, uint64_t* carry_min) {
  g_err.clear();
  const int rc = check_length_taps(length, taps, kRules);
  if (rc) return rc;
  if (halo) *halo = halo_of(taps);
  if (hop) *hop = hop_of(taps);
  if (segments) *segments = segments_of(length, taps);
  if (carry_min) *carry_min = carry_min_of(taps);
  return TFFT_OK;
}

int tfft_gcconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_gcconv_opts", kRules);
  if (rc) return rc;
  return copy_text("gcconv4096:4096" + gate_text(flags) + " x " + std::to_string(segments_of(length, taps)), buf, bytes);
}

int tfft_gcconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_gcconv_opts* opts,
                            tfft_gcconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_gcconv_opts o = TFFT_GCCONV_OPTS_INIT;
  int rc = take_opts(opts, "tfft_gcconv_opts", o);
  if (rc) return rc;
  rc = check_shape(rows, channels, length, taps, o.flags, "tfft_gcconv_opts", kRules);
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.in_seq_stride, "in");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.out_seq_stride, "out");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.pre_seq_stride, "pre");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.post_seq_stride, "post");
  if (rc == TFFT_OK) rc = check_context(taps, o.history, "history");
  if (rc == TFFT_OK) rc = check_context_stride(o.history, o.hist_seq_stride, "history", "hist");
  if (rc == TFFT_OK) rc = check_context_stride(o.history, o.pre_hist_seq_stride, "history", "pre_hist");
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_gcconv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_gcconv_plan* p = new tfft_gcconv_plan;
  set_shape(p, rows, channels, length, taps, o.launch_iters, o.flags, device_id);
  p->in_stride = o.in_seq_stride ? o.in_seq_stride : length;
  p->out_stride = o.out_seq_stride ? o.out_seq_stride : length;
  p->pre_stride = o.pre_seq_stride ? o.pre_seq_stride : length;
  p->post_stride = o.post_seq_stride ? o.post_seq_stride : length;
  p->history = o.history;
  p->hist_stride = o.hist_seq_stride ? o.hist_seq_stride : o.history;
  p->pre_hist_stride = o.pre_hist_seq_stride ? o.pre_hist_seq_stride : o.history;
  rc = create_base(p);
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  if (rc == TFFT_OK && hipFuncSetAttribute(plan_fwd(p), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes) != hipSuccess)
    rc = fail(TFFT_ERR_HIP, "hipFuncSetAttribute(fwd_kernel) failed");
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_gcconv_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_gcconv_plan_destroy(tfft_gcconv_plan* p) {
  if (!p) return;
  destroy_base(p);
  delete p;
}

int tfft_gcconv_plan_set_taps(tfft_gcconv_plan* p, const void* taps, const void* skip, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return set_taps(p, taps, skip, stream, false);
}

int tfft_gcconv_plan_spectrum(const tfft_gcconv_plan* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return copy_spectrum(p, h_re, h_im, "tfft_gcconv_plan_set_taps");
}

int tfft_gcconv_exec(const tfft_gcconv_plan* p, const void* in, const void* pre, const void* post, const void* hist, const void* pre_hist,
                     void* out, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_gcconv_plan_set_taps first");
  if (!in || !out) return fail(TFFT_ERR_ARG, "null data pointer");
  int rc = check_gate(p->pre, pre, "pre", "TFFT_GCCONV_PRE_GATE");
  if (rc == TFFT_OK) rc = check_gate(p->post, post, "post", "TFFT_GCCONV_POST_GATE");
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(pre) | reinterpret_cast<uintptr_t>(post)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  rc = check_context_ptrs(hist, pre_hist, p->history, p->pre, "hist", "pre_hist", "history", "pre");
  if (rc) return rc;
  const uint64_t seqs = p->rows * p->channels;
  // a segment's halo is the end of the stretch its predecessor writes, and segments run in no defined order: no in-place execution;
  // a gate or a context is read while other items' results are written: none shares a half with the output
  if (in == out || seqs_overlap(in, p->in_stride, p->length, out, p->out_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "input and output overlap (an overlap-save plan cannot run in place: a segment reads the halo its predecessor overwrites)");
  if (pre && seqs_overlap(pre, p->pre_stride, p->length, out, p->out_stride, p->length, seqs)) return fail(TFFT_ERR_ARG, "the pre gate and the output overlap");
  if (post && seqs_overlap(post, p->post_stride, p->length, out, p->out_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "the post gate and the output overlap");
  if (hist && seqs_overlap(hist, p->hist_stride, p->history, out, p->out_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "hist and output overlap (the history may alias the input, never the output)");
  if (pre_hist && seqs_overlap(pre_hist, p->pre_hist_stride, p->history, out, p->out_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "pre_hist and output overlap (the history may alias the pre gate, never the output)");
  rc = check_current(p->device);
  if (rc) return rc;
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // without a history the kernel gets 0 chunks of it and never forms an address from the second bases
  const gcconv4096::fwd_strides strides = {p->in_stride, p->pre_stride, hist ? p->hist_stride : p->in_stride,
                                           pre_hist ? p->pre_hist_stride : p->pre_stride, p->post_stride, p->out_stride};
  const gcconv4096::fwd_params params = {static_cast<const uint16_t*>(in),
                                         static_cast<const uint16_t*>(pre),
                                         static_cast<const uint16_t*>(hist ? hist : in),
                                         static_cast<const uint16_t*>(pre_hist ? pre_hist : pre),
                                         static_cast<const uint16_t*>(post),
                                         static_cast<uint16_t*>(out),
                                         strides,
                                         static_cast<uint32_t>(p->rows),
                                         static_cast<uint32_t>(p->channels),
                                         geometry_of(p),
                                         static_cast<int32_t>(hist ? p->history / 8 : 0),
                                         static_cast<uint32_t>(p->items),
                                         live,
                                         static_cast<const uint8_t*>(p->d_tables),
                                         p->d_filter};
#define GCCONV_LAUNCH(PRE, POST) \
  hipLaunchKernelGGL((gcconv4096::fwd_kernel<PRE, POST>), dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, s, params)
  if (p->pre && p->post)
    GCCONV_LAUNCH(true, true);
  else if (p->pre)
    GCCONV_LAUNCH(true, false);
  else if (p->post)
    GCCONV_LAUNCH(false, true);
  else
    GCCONV_LAUNCH(false, false);
#undef GCCONV_LAUNCH
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_gcconv_plan_num_launches(const tfft_gcconv_plan* p) { return p ? 1 : 0; }

int tfft_gcconv_plan_kernels(const tfft_gcconv_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names(std::string("gcconv4096::fwd_kernel<") + tf_text(p->pre) + ", " + tf_text(p->post) + ">\n", 1, buf, bytes);
}

// ---- the gradient plan

int tfft_gcconv_grad_geometry(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, uint64_t* halo, uint64_t* hop,
                              uint64_t* segments, uint64_t* partials_out, uint64_t* carry_min) {
  g_err.clear();
  const int rc = check_shape(rows, channels, length, taps, 0, "tfft_gcconv_grad_opts", kRules);
  if (rc) return rc;
  if (halo) *halo = halo_of(taps);
  if (hop) *hop = hop_of(taps);
  if (segments) *segments = segments_of(length, taps);
  if (partials_out) *partials_out = partials_of(rows, channels, length, taps, partials);
  if (carry_min) *carry_min = carry_min_of(taps);
  return TFFT_OK;
}

int tfft_gcconv_grad_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_gcconv_grad_opts", kRules);
  if (rc) return rc;
  return copy_text("gcconv4096:4096" + gate_text(flags) + " x " + std::to_string(segments_of(length, taps)) + " | partials " +
                       std::to_string(partials_of(rows, channels, length, taps, partials)),
                   buf, bytes);
}

int tfft_gcconv_grad_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_gcconv_grad_opts* opts,
                            tfft_gcconv_grad** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_gcconv_grad_opts o = TFFT_GCCONV_GRAD_OPTS_INIT;
  int rc = take_opts(opts, "tfft_gcconv_grad_opts", o);
  if (rc) return rc;
  rc = check_shape(rows, channels, length, taps, o.flags, "tfft_gcconv_grad_opts", kRules);
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.x_seq_stride, "x");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.pre_seq_stride, "pre");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.gy_seq_stride, "gy");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.post_seq_stride, "post");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.dx_seq_stride, "dx");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.dpre_seq_stride, "dpre");
  if (rc == TFFT_OK) rc = check_context(taps, o.history, "history");
  if (rc == TFFT_OK) rc = check_context_stride(o.history, o.hist_seq_stride, "history", "hist");
  if (rc == TFFT_OK) rc = check_context_stride(o.history, o.pre_hist_seq_stride, "history", "pre_hist");
  if (rc == TFFT_OK) rc = check_context(taps, o.future, "future");
  if (rc == TFFT_OK) rc = check_context_stride(o.future, o.fut_seq_stride, "future", "fut");
  if (rc == TFFT_OK) rc = check_context_stride(o.future, o.post_fut_seq_stride, "future", "post_fut");
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_gcconv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_gcconv_grad* p = new tfft_gcconv_grad;
  set_shape(p, rows, channels, length, taps, o.launch_iters, o.flags, device_id);
  p->per_channel = (rows + 1) / 2 * p->segments;
  p->partials = partials_of(rows, channels, length, taps, o.partials);
  p->kpad = kpad_of(taps);
  p->ws_need = static_cast<size_t>(channels * p->partials * p->kpad * 4);
  p->x_stride = o.x_seq_stride ? o.x_seq_stride : length;
  p->pre_stride = o.pre_seq_stride ? o.pre_seq_stride : length;
  p->gy_stride = o.gy_seq_stride ? o.gy_seq_stride : length;
  p->post_stride = o.post_seq_stride ? o.post_seq_stride : length;
  p->dx_stride = o.dx_seq_stride ? o.dx_seq_stride : length;
  p->dpre_stride = o.dpre_seq_stride ? o.dpre_seq_stride : length;
  p->history = o.history;
  p->hist_stride = o.hist_seq_stride ? o.hist_seq_stride : o.history;
  p->pre_hist_stride = o.pre_hist_seq_stride ? o.pre_hist_seq_stride : o.history;
  p->future = o.future;
  p->fut_stride = o.fut_seq_stride ? o.fut_seq_stride : o.future;
  p->post_fut_stride = o.post_fut_seq_stride ? o.post_fut_seq_stride : o.future;
  rc = create_base(p);
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  if (rc == TFFT_OK && (hipFuncSetAttribute(plan_dgrad(p), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes) != hipSuccess ||
                        hipFuncSetAttribute(plan_wgrad(p), hipFuncAttributeMaxDynamicSharedMemorySize, gcconv4096::kWgradLdsBytes) != hipSuccess))
    rc = fail(TFFT_ERR_HIP, "hipFuncSetAttribute(dgrad_kernel / wgrad_kernel) failed");
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_gcconv_grad_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_gcconv_grad_destroy(tfft_gcconv_grad* p) {
  if (!p) return;
  destroy_base(p);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_gcconv_grad_set_taps(tfft_gcconv_grad* p, const void* taps, const void* skip, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return set_taps(p, taps, skip, stream, true);
}

int tfft_gcconv_grad_spectrum(const tfft_gcconv_grad* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return copy_spectrum(p, h_re, h_im, "tfft_gcconv_grad_set_taps");
}

size_t tfft_gcconv_grad_workspace_bytes(const tfft_gcconv_grad* p) { return p ? p->ws_need : 0; }

int tfft_gcconv_grad_set_workspace(tfft_gcconv_grad* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_set(p, device_ptr, bytes);
}

int tfft_gcconv_grad_prepare(tfft_gcconv_grad* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_prepare(p);
}

int tfft_gcconv_grad_exec_input_grad(const tfft_gcconv_grad* p, const void* gy, const void* post, const void* fut, const void* post_fut,
                                     const void* x, const void* pre, void* dx, void* dpre, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_gcconv_grad_set_taps first");
  if (!gy || !dx) return fail(TFFT_ERR_ARG, "null data pointer");
  int rc = check_gate(p->post, post, "post", "TFFT_GCCONV_POST_GATE");
  if (rc == TFFT_OK) rc = check_gate(p->pre, pre, "pre", "TFFT_GCCONV_PRE_GATE");
  if (rc) return rc;
  if (p->pre && !x) return fail(TFFT_ERR_ARG, "the plan has a pre gate (TFFT_GCCONV_PRE_GATE) and the x pointer is null");
  if (!p->pre && x) return fail(TFFT_ERR_ARG, "the plan has no pre gate and the x pointer is not null");
  if (!p->pre && dpre) return fail(TFFT_ERR_ARG, "the plan has no pre gate and the dpre pointer is not null");
  if ((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(post) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(pre) |
       reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dpre)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  rc = check_context_ptrs(fut, post_fut, p->future, p->post, "gy_future", "post_future", "future", "post");
  if (rc) return rc;
  const uint64_t seqs = p->rows * p->channels;
  // segment s reads, beyond its hop, the start of the stretch segment s + 1 writes, and segments run in no defined order; a gate or
  // a context is read while other items' results are written: no output shares a half with an input or with the other output
  const seq_set inputs[6] = {{gy, p->gy_stride, p->length, "gy"},           {post, p->post_stride, p->length, "post"},
                             {x, p->x_stride, p->length, "x"},              {pre, p->pre_stride, p->length, "pre"},
                             {fut, p->fut_stride, p->future, "gy_future"},  {post_fut, p->post_fut_stride, p->future, "post_future"}};
  const seq_set outputs[2] = {{dx, p->dx_stride, p->length, "dx"}, {dpre, p->dpre_stride, p->length, "dpre"}};
  for (const seq_set& o : outputs) {
    if (!o.ptr) continue;
    for (const seq_set& i : inputs)
      if (i.ptr && (i.ptr == o.ptr || seqs_overlap(i.ptr, i.stride, i.len, o.ptr, o.stride, o.len, seqs)))
        return fail(TFFT_ERR_ARG, std::string(i.name) + " and " + o.name +
                                      " overlap (the input gradient cannot run in place: a segment reads what its successor overwrites)");
  }
  if (dpre && (dx == dpre || seqs_overlap(dx, p->dx_stride, p->length, dpre, p->dpre_stride, p->length, seqs)))
    return fail(TFFT_ERR_ARG, "dx and dpre overlap");
  rc = check_current(p->device);
  if (rc) return rc;
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // without a future the kernel gets 0 chunks of it and never forms an address from the second bases
  const gcconv4096::dgrad_strides strides = {p->gy_stride, p->post_stride, fut ? p->fut_stride : p->gy_stride,
                                             post_fut ? p->post_fut_stride : p->post_stride, p->x_stride, p->pre_stride, p->dx_stride, p->dpre_stride};
  const gcconv4096::dgrad_params params = {static_cast<const uint16_t*>(gy),
                                           static_cast<const uint16_t*>(post),
                                           static_cast<const uint16_t*>(fut ? fut : gy),
                                           static_cast<const uint16_t*>(post_fut ? post_fut : post),
                                           static_cast<const uint16_t*>(x),
                                           static_cast<const uint16_t*>(pre),
                                           static_cast<uint16_t*>(dx),
                                           static_cast<uint16_t*>(dpre),
                                           strides,
                                           static_cast<uint32_t>(p->rows),
                                           static_cast<uint32_t>(p->channels),
                                           geometry_of(p),
                                           static_cast<int32_t>(fut ? p->future / 8 : 0),
                                           static_cast<uint32_t>(p->items),
                                           live,
                                           static_cast<const uint8_t*>(p->d_tables),
                                           p->d_filter};
#define GCCONV_LAUNCH(PRE, POST) \
  hipLaunchKernelGGL((gcconv4096::dgrad_kernel<PRE, POST>), dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, s, params)
  if (p->pre && p->post)
    GCCONV_LAUNCH(true, true);
  else if (p->pre)
    GCCONV_LAUNCH(true, false);
  else if (p->post)
    GCCONV_LAUNCH(false, true);
  else
    GCCONV_LAUNCH(false, false);
#undef GCCONV_LAUNCH
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_gcconv_grad_exec_tap_grad(const tfft_gcconv_grad* p, const void* x, const void* pre, const void* hist, const void* pre_hist,
                                   const void* gy, const void* post, void* dh, void* dskip, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!x || !gy || !dh) return fail(TFFT_ERR_ARG, "null data pointer");
  int rc = check_gate(p->pre, pre, "pre", "TFFT_GCCONV_PRE_GATE");
  if (rc == TFFT_OK) rc = check_gate(p->post, post, "post", "TFFT_GCCONV_POST_GATE");
  if (rc) return rc;
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(pre) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(post)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  if ((reinterpret_cast<uintptr_t>(dh) | reinterpret_cast<uintptr_t>(dskip)) & 3) return fail(TFFT_ERR_ARG, "the tap gradient and the skip gradient must be 4-byte aligned");
  rc = check_context_ptrs(hist, pre_hist, p->history, p->pre, "x_hist", "pre_hist", "history", "pre");
  if (rc) return rc;
  const uint64_t seqs = p->rows * p->channels, dh_bytes = p->channels * p->taps * 4, dskip_bytes = p->channels * 4;
  const seq_set inputs[6] = {{x, p->x_stride, p->length, "x"},          {pre, p->pre_stride, p->length, "pre"},
                             {gy, p->gy_stride, p->length, "gy"},       {post, p->post_stride, p->length, "post"},
                             {hist, p->hist_stride, p->history, "x_hist"}, {pre_hist, p->pre_hist_stride, p->history, "pre_hist"}};
  for (const seq_set& i : inputs) {
    if (block_overlaps(dh, dh_bytes, i.ptr, i.stride, seqs, i.len))
      return fail(TFFT_ERR_ARG, "the tap gradient overlaps x, pre, gy, post, x_hist or pre_hist");
    if (dskip && block_overlaps(dskip, dskip_bytes, i.ptr, i.stride, seqs, i.len))
      return fail(TFFT_ERR_ARG, "the skip gradient overlaps x, pre, gy, post, x_hist or pre_hist");
  }
  if (dskip && blocks_overlap(dh, dh_bytes, dskip, dskip_bytes)) return fail(TFFT_ERR_ARG, "the tap gradient and the skip gradient overlap");
  rc = check_current(p->device);
  if (rc == TFFT_OK) rc = ws_ensure(p);
  if (rc) return rc;
  for (const seq_set& i : inputs)
    if (block_overlaps(p->ws, p->ws_need, i.ptr, i.stride, seqs, i.len))
      return fail(TFFT_ERR_ARG, "the workspace overlaps an input, a context, the tap gradient or the skip gradient");
  if (blocks_overlap(p->ws, p->ws_need, dh, dh_bytes) || (dskip && blocks_overlap(p->ws, p->ws_need, dskip, dskip_bytes)))
    return fail(TFFT_ERR_ARG, "the workspace overlaps an input, a context, the tap gradient or the skip gradient");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t live, grid;
  wgrad_shape(p->channels * p->partials, p->num_cus, gcconv4096::kWgradWaves, live, grid);
  const gcconv4096::wgrad_strides strides = {p->x_stride, p->pre_stride, hist ? p->hist_stride : p->x_stride,
                                             pre_hist ? p->pre_hist_stride : p->pre_stride, p->gy_stride, p->post_stride};
  const uint32_t channels = static_cast<uint32_t>(p->channels);
  const gcconv4096::wgrad_params params = {static_cast<const uint16_t*>(x),
                                           static_cast<const uint16_t*>(pre),
                                           static_cast<const uint16_t*>(hist ? hist : x),
                                           static_cast<const uint16_t*>(pre_hist ? pre_hist : pre),
                                           static_cast<const uint16_t*>(gy),
                                           static_cast<const uint16_t*>(post),
                                           strides,
                                           static_cast<uint32_t>(p->rows),
                                           channels,
                                           geometry_of(p),
                                           static_cast<int32_t>(hist ? p->history / 8 : 0),
                                           static_cast<uint32_t>(p->partials),
                                           static_cast<uint32_t>(p->per_channel),
                                           static_cast<uint32_t>(p->channels * p->partials),
                                           live,
                                           static_cast<int32_t>(p->kpad / 8),
                                           static_cast<uint32_t>(p->kpad),
                                           static_cast<const uint8_t*>(p->d_tables),
                                           static_cast<float*>(p->ws)};
#define GCCONV_LAUNCH(PRE, POST) \
  hipLaunchKernelGGL((gcconv4096::wgrad_kernel<PRE, POST>), dim3(grid), dim3(gcconv4096::kWgradThreads), gcconv4096::kWgradLdsBytes, s, params)
  if (p->pre && p->post)
    GCCONV_LAUNCH(true, true);
  else if (p->pre)
    GCCONV_LAUNCH(true, false);
  else if (p->post)
    GCCONV_LAUNCH(false, true);
  else
    GCCONV_LAUNCH(false, false);
#undef GCCONV_LAUNCH
  CONV_HIP(hipGetLastError());
  const uint64_t total = p->channels * p->taps;
  hipLaunchKernelGGL(gcconv4096::wreduce_kernel, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(p->ws),
                     static_cast<float*>(dh), static_cast<float*>(dskip), channels, static_cast<uint32_t>(p->taps),
                     static_cast<uint32_t>(p->partials), static_cast<uint32_t>(p->kpad));
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_gcconv_grad_num_launches(const tfft_gcconv_grad* p) { return p ? 3 : 0; }

int tfft_gcconv_grad_kernels(const tfft_gcconv_grad* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  const std::string inst = std::string("<") + tf_text(p->pre) + ", " + tf_text(p->post) + ">\n";
  return kernel_names("gcconv4096::dgrad_kernel" + inst + "gcconv4096::wgrad_kernel" + inst + "gcconv4096::wreduce_kernel\n", 3, buf, bytes);
}

}  // extern "C"
