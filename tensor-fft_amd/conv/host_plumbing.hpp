// host_plumbing.hpp — what the host side of every convolution library does the same way over HIP and include/tfft.h /
// tfft_conv.h: the last-error string and the ways to fill it, the ABI check, the refusals of a shape, a stride and a context, the
// two launch shapes, and the parts of a one-pass plan (tables, spectrum, filter image, gradient workspace) whose code does not
// depend on which plan it is.
//
// Header only, everything in an unnamed namespace: each library is one translation unit built with -fvisibility=hidden and keeps
// an error string of its own. Including it links nothing; the layering (an add-on links libtfft_conv.so and libtfft.so, never a
// sibling) is untouched. The templates take any plan struct that has the fields they name.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfft_conv.h"
#include "../csrc/k4096.hpp"
#include "host_math.hpp"

namespace {

using namespace host_math;

// ---- the error string of the calling thread, and the ways to fill it
thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
inline int hip_fail(hipError_t e, const char* what) { return fail(TFFT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
// a failing call into libtfft.so / libtfft_conv.so: its message becomes ours
inline int pass_tfft(int rc) {
  if (rc != TFFT_OK) g_err = tfft_last_error();
  return rc;
}
inline int pass_conv(int rc) {
  if (rc != TFFT_OK) g_err = tfft_conv_last_error();
  return rc;
}
#define CONV_HIP(call)                                \
  do {                                                \
    const hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) return hip_fail(e_, #call); \
  } while (0)

// `lib_name` as in "libtfft_sconv.so"
inline int check_abi(const char* lib_name) {
  static const int version = tfft_abi_version();
  if (version != TFFT_ABI_VERSION)
    return fail(TFFT_ERR_ARG, "libtfft.so speaks ABI " + std::to_string(version) + ", " + lib_name + " was built against ABI " +
                                  std::to_string(TFFT_ABI_VERSION) + ": rebuild the add-on");
  return TFFT_OK;
}

// the options of a create call: defaults when `opts` is null, else a struct of the one layout this library knows. `name` as in
// "tfft_sconv_opts"; `o` holds the defaults on entry
template <class Opts>
int take_opts(const Opts* opts, const char* name, Opts& o) {
  if (!opts) return TFFT_OK;
  if (opts->struct_size != sizeof(Opts))
    return fail(TFFT_ERR_ARG, std::string(name) + ".struct_size = " + std::to_string(opts->struct_size) +
                                  " is not the size of a layout this library knows (" + std::to_string(sizeof(Opts)) + ")");
  if (opts->reserved_) return fail(TFFT_ERR_ARG, std::string(name) + ".reserved_ must be 0");
  o = *opts;
  return TFFT_OK;
}

// ---- refusals
inline int check_rows_channels(uint64_t rows, uint64_t channels) {
  if (rows == 0 || rows > 0xffffffffull) return fail(TFFT_ERR_ARG, "rows must be in [1, 2^32)");
  if (channels == 0 || channels > 0xffffffffull) return fail(TFFT_ERR_ARG, "channels must be in [1, 2^32)");
  if (rows * channels > 0xffffffffull) return fail(TFFT_ERR_ARG, "rows * channels must be below 2^32");
  return TFFT_OK;
}
inline int check_seq_stride(uint64_t length, uint64_t stride, const char* which) {
  if (stride && (stride % 8 || stride < length))
    return fail(TFFT_ERR_ARG, std::string(which) + "_seq_stride must be 0 or a multiple of 8 that is >= length");
  return TFFT_OK;
}
inline int check_launch_iters(uint32_t launch_iters) {
  if (launch_iters > TFFT_LAUNCH_PERSISTENT) return fail(TFFT_ERR_ARG, "launch_iters must be 0 .. 65535");
  return TFFT_OK;
}

// what differs between the overlap-save libraries in the refusal of a shape: the flag bits a plan takes, how the message states
// that rule (after "<opts name>.flags "), and the create call a filter too long for a window is sent to
struct shape_rules {
  int flag_mask;
  const char* flags_rule;
  const char* longer_through;
};

inline int check_length_taps(uint64_t length, uint64_t taps, const shape_rules& rules) {
  if (length < 8 || length % 8) return fail(TFFT_ERR_ARG, "length must be a multiple of 8 and at least 8");
  if (length > kMaxLength) return fail(TFFT_ERR_ARG, "length must not exceed 2^26");
  if (taps == 0) return fail(TFFT_ERR_ARG, "taps must be at least 1");
  if (taps > kMaxTaps)
    return fail(TFFT_ERR_ARG, std::string("taps must not exceed 2049 (the halo of a 4096-sample window): longer filters run through ") +
                                  rules.longer_through);
  return TFFT_OK;
}
// the shape of an overlap-save plan; `opts_name` as in "tfft_cconv_grad_opts"
inline int check_shape(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int flags, const char* opts_name, const shape_rules& rules) {
  int rc = check_length_taps(length, taps, rules);
  if (rc) return rc;
  if (flags & ~rules.flag_mask)
    return fail(TFFT_ERR_ARG, "unknown flag bits (" + std::to_string(flags) + "): " + opts_name + ".flags " + rules.flags_rule);
  rc = check_rows_channels(rows, channels);
  if (rc) return rc;
  // pairs * channels < 2^32 and segments <= 2^15: the product cannot overflow 64 bits
  if ((rows + 1) / 2 * channels * segments_of(length, taps) > 0xffffffffull)
    return fail(TFFT_ERR_ARG, "the item count ceil(rows / 2) * segments * channels must be below 2^32");
  return TFFT_OK;
}
// a context of `n` samples per sequence: `which` = "history" / "future"
inline int check_context(uint64_t taps, uint64_t n, const char* which) {
  if (n % 8) return fail(TFFT_ERR_ARG, std::string(which) + " must be a multiple of 8");
  if (n > halo_of(taps))
    return fail(TFFT_ERR_ARG, std::string(which) + " must not exceed the halo (" + std::to_string(halo_of(taps)) + " samples for " +
                                  std::to_string(taps) + " taps): no window reaches further");
  return TFFT_OK;
}
// the sequence stride of a context: `short_name` = "hist" / "pre_hist" / "fut" / "post_fut"
inline int check_context_stride(uint64_t n, uint64_t stride, const char* which, const char* short_name) {
  if (stride && (stride % 8 || stride < n))
    return fail(TFFT_ERR_ARG, std::string(short_name) + "_seq_stride must be 0 or a multiple of 8 that is >= " + which);
  return TFFT_OK;
}
inline int check_current(int device) {
  int cur = 0;
  CONV_HIP(hipGetDevice(&cur));
  if (cur != device) return fail(TFFT_ERR_ARG, "plan was created for another device than the current one");
  return TFFT_OK;
}

// ---- launch shapes
// Every fused forward and input-gradient kernel, one wave per item: that of fft4096_kernel<kStageOut | kNonTemporal> (tfft.hip,
// live_waves / k4096_shape). One wave per SIMD on as many CUs as there are for a count that does not fill the chip, else 8 waves
// per workgroup; about two items per wave and the hardware dispatcher handing out workgroups as CUs drain once the count is four
// chips' worth. launch_iters as the options structs state it (0: that default).
inline void conv_shape(uint64_t items, int num_cus, uint32_t launch_iters, uint32_t& live, uint32_t& grid) {
  const uint64_t cus = static_cast<uint64_t>(num_cus);
  live = 8;
  for (uint32_t l = 1; l <= 4; l *= 2)
    if (items <= cus * l) {
      live = l;
      break;
    }
  const uint64_t blocks = (items + live - 1) / live;
  if (launch_iters >= TFFT_LAUNCH_PERSISTENT) {
    grid = static_cast<uint32_t>(std::min(blocks, cus));
  } else if (launch_iters) {
    grid = static_cast<uint32_t>((blocks + launch_iters - 1) / launch_iters);
  } else {
    const uint64_t iters = blocks >= 4 * cus ? 2 : 1;
    grid = static_cast<uint32_t>(std::max<uint64_t>(std::min<uint64_t>(blocks, cus), (blocks + iters - 1) / iters));
  }
}
// The tap gradient: every work unit (c, q) is one wave of its own, in workgroups of up to `waves` (one per SIMD); as few per
// workgroup as still cover the units with one workgroup per CU, as the shape above. The units, not the launch, fix the order of
// the additions.
inline void wgrad_shape(uint64_t units, int num_cus, uint32_t waves, uint32_t& live, uint32_t& grid) {
  const uint64_t cus = static_cast<uint64_t>(num_cus);
  live = waves;
  for (uint32_t l = 1; l < live; l *= 2)
    if (units <= cus * l) {
      live = l;
      break;
    }
  grid = static_cast<uint32_t>((units + live - 1) / live);
}

// ---- texts
inline int copy_text(const std::string& out, char* buf, size_t bytes) {
  if (out.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return TFFT_OK;
}
inline int kernel_names(const std::string& out, int lines, char* buf, size_t bytes) {
  if (!buf || out.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small (" + std::to_string(out.size() + 1) + " bytes needed)");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return lines;
}
inline const char* tf_text(bool v) { return v ? "true" : "false"; }      // a template argument as a kernel's name spells it

template <class Plan>
int fail_create(Plan* p, int rc, void (*destroy)(Plan*)) {
  const std::string keep = g_err;
  destroy(p);
  g_err = keep;
  return rc;
}

// ---- the device memory of a one-pass plan. Plan has: channels, taps, device, d_tables (F / twiddle / G / H of
// k4096::build_tables), d_filter ([channels][RE 4096 | IM 4096] in filter_slot order), d_spec ([RE: channels x 4096 | IM: channels
// x 4096], natural bin order), have_taps.
template <class Plan>
int create_base(Plan* p) {
  std::vector<uint8_t> blob;
  k4096::build_tables(blob);
  CONV_HIP(hipMalloc(&p->d_tables, k4096::kOffF1n));
  CONV_HIP(hipMemcpy(p->d_tables, blob.data(), k4096::kOffF1n, hipMemcpyHostToDevice));
  CONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_filter), static_cast<size_t>(p->channels) * 8192 * 2));
  CONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_spec), static_cast<size_t>(p->channels) * kN * 4));
  return TFFT_OK;
}
template <class Plan>
void destroy_base(Plan* p) {
  if (p->d_tables) (void)hipFree(p->d_tables);
  if (p->d_filter) (void)hipFree(p->d_filter);
  if (p->d_spec) (void)hipFree(p->d_spec);
}

// The taps of a plan, `skip` null for none: the spectrum H' and the filter image, H' for a forward plan and conj(H') for a gradient
// plan (`conjugate`). Through the host: both are built once per filter, not per execution. Everything enqueued on `stream` before
// the call (the kernel that produced the taps) is waited for; executions still in flight keep reading the old spectrum until then,
// so the device is drained before it is replaced.
template <class Plan>
int set_taps(Plan* p, const void* taps, const void* skip, void* stream, bool conjugate) {
  if (!taps) return fail(TFFT_ERR_ARG, "null taps pointer");
  const int rc = check_current(p->device);
  if (rc) return rc;
  const size_t plane = static_cast<size_t>(p->channels) * kN;
  std::vector<uint16_t> h(static_cast<size_t>(p->channels) * p->taps), d(p->channels, 0), spec(2 * plane), img(2 * plane);
  hipStream_t s = static_cast<hipStream_t>(stream);
  CONV_HIP(hipMemcpyAsync(h.data(), taps, h.size() * 2, hipMemcpyDeviceToHost, s));
  if (skip) CONV_HIP(hipMemcpyAsync(d.data(), skip, d.size() * 2, hipMemcpyDeviceToHost, s));
  CONV_HIP(hipStreamSynchronize(s));
  for (uint64_t c = 0; c < p->channels; ++c) {
    spectrum(h.data() + c * p->taps, p->taps, d[c], kN, spec.data() + c * kN, spec.data() + plane + c * kN);
    filter_image(spec.data() + c * kN, spec.data() + plane + c * kN, conjugate, img.data() + c * 8192);
  }
  if (p->have_taps) CONV_HIP(hipDeviceSynchronize());
  CONV_HIP(hipMemcpy(p->d_spec, spec.data(), spec.size() * 2, hipMemcpyHostToDevice));
  CONV_HIP(hipMemcpy(p->d_filter, img.data(), img.size() * 2, hipMemcpyHostToDevice));
  p->have_taps = true;
  return TFFT_OK;
}

// `set_taps_name` as in "tfft_sconv_plan_set_taps"
template <class Plan>
int copy_spectrum(const Plan* p, void* h_re, void* h_im, const char* set_taps_name) {
  if (!h_re || !h_im) return fail(TFFT_ERR_ARG, "null spectrum pointer");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, std::string("no taps: call ") + set_taps_name + " first");
  const size_t plane = static_cast<size_t>(p->channels) * kN;
  CONV_HIP(hipMemcpy(h_re, p->d_spec, plane * 2, hipMemcpyDeviceToDevice));
  CONV_HIP(hipMemcpy(h_im, p->d_spec + plane, plane * 2, hipMemcpyDeviceToDevice));
  CONV_HIP(hipDeviceSynchronize());
  return TFFT_OK;
}

// ---- the workspace of a gradient plan (the partial sums of the tap gradient). Plan has: device, ws_need, and mutable ws_mutex,
// ws, ws_owned. The rule of tfft_conv.h: the workspace is settled once, by the caller, by prepare or by the first execution.
template <class Plan>
int ws_ensure(const Plan* p) {
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  if (p->ws) return TFFT_OK;
  void* mem = nullptr;
  CONV_HIP(hipMalloc(&mem, p->ws_need));
  p->ws = mem;
  p->ws_owned = true;
  return TFFT_OK;
}
template <class Plan>
int ws_set(Plan* p, void* device_ptr, size_t bytes) {
  if (device_ptr && bytes < p->ws_need) return fail(TFFT_ERR_WORKSPACE, "workspace too small: " + std::to_string(p->ws_need) + " bytes needed");
  if (reinterpret_cast<uintptr_t>(device_ptr) & 255) return fail(TFFT_ERR_ARG, "the workspace must be 256-byte aligned");
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  p->ws = device_ptr;
  p->ws_owned = false;
  return TFFT_OK;
}
template <class Plan>
int ws_prepare(Plan* p) {
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(p->device));
  const int rc = ws_ensure(p);
  (void)hipSetDevice(prev);
  return rc;
}

}  // namespace
