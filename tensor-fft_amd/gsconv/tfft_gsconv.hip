// tfft_gsconv.hip — host side and C ABI (include/tfft_gsconv.h) of the gated overlap-save causal convolution add-on,
// libtfft_gsconv.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp, header only, for the device helpers and the constant tables of the kernel
// (the add-on uploads a copy of its own). It links neither libtfft_sconv.so nor libtfft_gconv.so: the geometry, the launch shape
// and the fp64 spectrum builder (the skip folded into tap 0) come from conv/host_math.hpp and conv/host_plumbing.hpp, the two
// headers every convolution library includes, and tests/test_gsconv_host.py and tests/test_gpu_gsconv.py hold them to
// tfft_sconv_geometry and tfft_gconv_spectrum_host.
#include "../../include/tfft_gsconv.h"
#include "gsconv4096.hpp"
#include "../conv/host_plumbing.hpp"

namespace {

static_assert(TFFT_GSCONV_MAX_TAPS == kMaxTaps, "include/tfft_gsconv.h and conv/host_math.hpp disagree on the longest filter");
constexpr int kGates = TFFT_GSCONV_PRE_GATE | TFFT_GSCONV_POST_GATE;
constexpr shape_rules kRules = {kGates, "takes TFFT_GSCONV_PRE_GATE and TFFT_GSCONV_POST_GATE only", "tfft_gconv_plan_create"};

std::string gate_text(int flags) {
  if (!(flags & kGates)) return "";
  return std::string(":") + ((flags & TFFT_GSCONV_PRE_GATE) ? "pre" : "") + ((flags & kGates) == kGates ? "+" : "") +
         ((flags & TFFT_GSCONV_POST_GATE) ? "post" : "");
}

}  // namespace

struct tfft_gsconv_plan {
  uint64_t rows = 0, channels = 0, length = 0, taps = 0, halo = 0, hop = 0, segments = 0, items = 0;
  uint64_t in_stride = 0, out_stride = 0, pre_stride = 0, post_stride = 0;
  uint32_t launch_iters = 0;
  int device = 0, num_cus = 256;
  bool pre = false, post = false;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // [channels][RE 4096 | IM 4096] in filter_slot order
  uint16_t* d_spec = nullptr;        // [RE: channels x 4096 | IM: channels x 4096], natural bin order (tfft_gsconv_plan_spectrum)
  bool have_taps = false;
};

namespace {

// the instantiation a plan launches
const void* plan_kernel(const tfft_gsconv_plan* p) {
  if (p->pre)
    return p->post ? reinterpret_cast<const void*>(gsconv4096::gsconv4096_kernel<true, true>)
                   : reinterpret_cast<const void*>(gsconv4096::gsconv4096_kernel<true, false>);
  return p->post ? reinterpret_cast<const void*>(gsconv4096::gsconv4096_kernel<false, true>)
                 : reinterpret_cast<const void*>(gsconv4096::gsconv4096_kernel<false, false>);
}

int create_device(tfft_gsconv_plan* p) {
  const int rc = create_base(p);
  if (rc) return rc;
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(plan_kernel(p), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  return TFFT_OK;
}

}  // namespace

extern "C" {

const char* tfft_gsconv_last_error(void) { return g_err.c_str(); }

int tfft_gsconv_geometry(uint64_t length, uint64_t taps, uint64_t* halo, uint64_t* hop, uint64_t* segments) {
  g_err.clear();
  const int rc = check_length_taps(length, taps, kRules);
  if (rc) return rc;
  if (halo) *halo = halo_of(taps);
  if (hop) *hop = hop_of(taps);
  if (segments) *segments = segments_of(length, taps);
  return TFFT_OK;
}

int tfft_gsconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_gsconv_opts", kRules);
  if (rc) return rc;
  return copy_text("gsconv4096:4096" + gate_text(flags) + " x " + std::to_string(segments_of(length, taps)), buf, bytes);
}

int tfft_gsconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_gsconv_opts* opts,
                            tfft_gsconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_gsconv_opts o = TFFT_GSCONV_OPTS_INIT;
  int rc = take_opts(opts, "tfft_gsconv_opts", o);
  if (rc) return rc;
  rc = check_shape(rows, channels, length, taps, o.flags, "tfft_gsconv_opts", kRules);
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.in_seq_stride, "in");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.out_seq_stride, "out");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.pre_seq_stride, "pre");
  if (rc == TFFT_OK) rc = check_seq_stride(length, o.post_seq_stride, "post");
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_gsconv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_gsconv_plan* p = new tfft_gsconv_plan;
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
  p->pre_stride = o.pre_seq_stride ? o.pre_seq_stride : length;
  p->post_stride = o.post_seq_stride ? o.post_seq_stride : length;
  p->pre = (o.flags & TFFT_GSCONV_PRE_GATE) != 0;
  p->post = (o.flags & TFFT_GSCONV_POST_GATE) != 0;
  p->launch_iters = o.launch_iters;
  p->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
  rc = create_device(p);
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_gsconv_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_gsconv_plan_destroy(tfft_gsconv_plan* p) {
  if (!p) return;
  destroy_base(p);
  delete p;
}

int tfft_gsconv_plan_set_taps(tfft_gsconv_plan* p, const void* taps, const void* skip, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return set_taps(p, taps, skip, stream, false);
}

int tfft_gsconv_plan_spectrum(const tfft_gsconv_plan* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return copy_spectrum(p, h_re, h_im, "tfft_gsconv_plan_set_taps");
}

int tfft_gsconv_exec(const tfft_gsconv_plan* p, const void* in, const void* pre, const void* post, void* out, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_gsconv_plan_set_taps first");
  if (!in || !out) return fail(TFFT_ERR_ARG, "null data pointer");
  if (p->pre && !pre) return fail(TFFT_ERR_ARG, "the plan has a pre gate (TFFT_GSCONV_PRE_GATE) and the pre pointer is null");
  if (p->post && !post) return fail(TFFT_ERR_ARG, "the plan has a post gate (TFFT_GSCONV_POST_GATE) and the post pointer is null");
  if (!p->pre && pre) return fail(TFFT_ERR_ARG, "the plan has no pre gate and the pre pointer is not null");
  if (!p->post && post) return fail(TFFT_ERR_ARG, "the plan has no post gate and the post pointer is not null");
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(pre) | reinterpret_cast<uintptr_t>(post)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  const uint64_t seqs = p->rows * p->channels;
  // a segment's halo is the end of the stretch its predecessor writes, and segments run in no defined order: no in-place execution
  if (in == out || seqs_overlap(in, p->in_stride, p->length, out, p->out_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "input and output overlap (an overlap-save plan cannot run in place: a segment reads the halo its predecessor overwrites)");
  // a gate is read while other items' results are written: it shares no half with the output
  if (pre && seqs_overlap(pre, p->pre_stride, p->length, out, p->out_stride, p->length, seqs)) return fail(TFFT_ERR_ARG, "the pre gate and the output overlap");
  if (post && seqs_overlap(post, p->post_stride, p->length, out, p->out_stride, p->length, seqs))
    return fail(TFFT_ERR_ARG, "the post gate and the output overlap");
  const int rc = check_current(p->device);
  if (rc) return rc;
  const gsconv4096::geometry geo = {static_cast<int32_t>(p->length / 8), static_cast<int32_t>(p->halo / 8), static_cast<int32_t>(p->hop / 8),
                                    static_cast<int32_t>(p->segments)};
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint16_t* const x = static_cast<const uint16_t*>(in);
  const uint16_t* const gp = static_cast<const uint16_t*>(pre);
  const uint16_t* const gq = static_cast<const uint16_t*>(post);
  uint16_t* const y = static_cast<uint16_t*>(out);
  const uint32_t rows = static_cast<uint32_t>(p->rows), channels = static_cast<uint32_t>(p->channels), items = static_cast<uint32_t>(p->items);
  const uint8_t* const tables = static_cast<const uint8_t*>(p->d_tables);
#define GSCONV_LAUNCH(PRE, POST)                                                                                                                     \
  hipLaunchKernelGGL((gsconv4096::gsconv4096_kernel<PRE, POST>), dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, s, x, gp, gq, y, p->in_stride, \
                     p->pre_stride, p->post_stride, p->out_stride, rows, channels, geo, items, live, tables, p->d_filter)
  if (p->pre && p->post)
    GSCONV_LAUNCH(true, true);
  else if (p->pre)
    GSCONV_LAUNCH(true, false);
  else if (p->post)
    GSCONV_LAUNCH(false, true);
  else
    GSCONV_LAUNCH(false, false);
#undef GSCONV_LAUNCH
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_gsconv_plan_num_launches(const tfft_gsconv_plan* p) { return p ? 1 : 0; }

int tfft_gsconv_plan_kernels(const tfft_gsconv_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names(std::string("gsconv4096::gsconv4096_kernel<") + tf_text(p->pre) + ", " + tf_text(p->post) + ">\n", 1, buf, bytes);
}

}  // extern "C"
