// tfft_stft.hip — host side and C ABI (include/tfft_stft.h) of the short-time Fourier transform add-on, libtfft_stft.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp and rsplit.hpp, header only, for the device helpers and the constant tables of
// the kernel (the add-on uploads a copy of its own). The error string, the HIP check, the ABI check, the launch_iters rule and the
// launch shape come from conv/host_plumbing.hpp; tests/test_gpu_stft.py holds the plan to tfft_exec_r2c bit for bit.
#include "../../include/tfft_stft.h"
#include "stft4096.hpp"
#include "../conv/host_plumbing.hpp"

namespace {

static_assert(TFFT_STFT_N == kN, "include/tfft_stft.h and conv/host_math.hpp disagree on the frame length");
constexpr uint64_t kBins = TFFT_STFT_BINS, kPitch = TFFT_STFT_PITCH;
constexpr uint64_t kMaxExtent = uint64_t{1} << 62;       // halves: a byte offset then fits 64 bits

// the frames per signal; `frames` may be null
int check_geometry(uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  if (length < 8 || length % 8) return fail(TFFT_ERR_ARG, "length must be a multiple of 8 and at least 8");
  if (length > kMaxLength) return fail(TFFT_ERR_ARG, "length must not exceed 2^26");
  if (hop < 8 || hop % 8) return fail(TFFT_ERR_ARG, "hop must be a multiple of 8 and at least 8");
  if (pad % 8 || pad >= kN) return fail(TFFT_ERR_ARG, "pad must be a multiple of 8 and below 4096");
  if (length + 2 * pad < kN) return fail(TFFT_ERR_ARG, "length + 2 * pad must be at least 4096: there is no frame");
  if (frames) *frames = 1 + (length + 2 * pad - kN) / hop;
  return TFFT_OK;
}

int check_shape(uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int flags, uint64_t* frames) {
  uint64_t f = 0;
  const int rc = check_geometry(length, hop, pad, &f);
  if (rc) return rc;
  if (flags) return fail(TFFT_ERR_ARG, "unknown flag bits (" + std::to_string(flags) + "): tfft_stft_opts.flags must be 0");
  if (rows == 0 || rows > 0xffffffffull) return fail(TFFT_ERR_ARG, "rows must be in [1, 2^32)");
  // frames <= 2^24 + 1: the product cannot overflow 64 bits. A frame index 2 i + 1 of item i must fit 32 bits
  if (rows * f > 0xffffffffull) return fail(TFFT_ERR_ARG, "the frame count rows * frames must be below 2^32");
  if (frames) *frames = f;
  return TFFT_OK;
}

// (count - 1) * stride + len below 2^62 halves, without overflow
bool extent_fits(uint64_t count, uint64_t stride, uint64_t len) { return count == 1 || stride <= (kMaxExtent - len - 1) / (count - 1); }

int check_strides(uint64_t rows, uint64_t length, uint64_t frames, uint64_t in_stride, uint64_t out_stride) {
  if (in_stride && (in_stride % 8 || in_stride < length))
    return fail(TFFT_ERR_ARG, "in_sig_stride must be 0 or a multiple of 8 that is >= length");
  if (out_stride && (out_stride % 8 || out_stride < kBins))
    return fail(TFFT_ERR_ARG, "out_frame_stride must be 0 or a multiple of 8 that is >= 2049");
  if (!extent_fits(rows, in_stride ? in_stride : length, length))
    return fail(TFFT_ERR_ARG, "the input extent (rows - 1) * in_sig_stride + length must be below 2^62 halves");
  if (!extent_fits(rows * frames, out_stride ? out_stride : 2 * kPitch, kBins))
    return fail(TFFT_ERR_ARG, "the output extent (rows * frames - 1) * out_frame_stride + 2049 must be below 2^62 halves");
  return TFFT_OK;
}

}  // namespace

struct tfft_stft_plan {
  uint64_t rows = 0, length = 0, hop = 0, pad = 0, frames = 0, total = 0, items = 0, in_stride = 0, out_stride = 0;
  uint32_t launch_iters = 0;
  int device = 0, num_cus = 256;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_window = nullptr;      // 4096 halves, the plan's own copy
  bool have_window = false;
};

namespace {

int create_device(tfft_stft_plan* p) {
  std::vector<uint8_t> blob;
  k4096::build_tables(blob);
  CONV_HIP(hipMalloc(&p->d_tables, k4096::kOffF1n));
  CONV_HIP(hipMemcpy(p->d_tables, blob.data(), k4096::kOffF1n, hipMemcpyHostToDevice));
  CONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_window), kN * 2));
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(stft4096::stft4096_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  return TFFT_OK;
}

}  // namespace

extern "C" {

const char* tfft_stft_last_error(void) { return g_err.c_str(); }

int tfft_stft_geometry(uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  g_err.clear();
  return check_geometry(length, hop, pad, frames);
}

int tfft_stft_describe(uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  uint64_t frames = 0;
  const int rc = check_shape(rows, length, hop, pad, flags, &frames);
  if (rc) return rc;
  return copy_text("stft4096:4096 x " + std::to_string(frames), buf, bytes);
}

int tfft_stft_plan_create(uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id, const tfft_stft_opts* opts,
                          tfft_stft_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_stft_opts o = TFFT_STFT_OPTS_INIT;
  int rc = take_opts(opts, "tfft_stft_opts", o);
  if (rc) return rc;
  uint64_t frames = 0;
  rc = check_shape(rows, length, hop, pad, o.flags, &frames);
  if (rc == TFFT_OK) rc = check_strides(rows, length, frames, o.in_sig_stride, o.out_frame_stride);
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_stft.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_stft_plan* p = new tfft_stft_plan;
  p->rows = rows;
  p->length = length;
  p->hop = hop;
  p->pad = pad;
  p->frames = frames;
  p->total = rows * frames;
  p->items = (p->total + 1) / 2;
  p->in_stride = o.in_sig_stride ? o.in_sig_stride : length;
  p->out_stride = o.out_frame_stride ? o.out_frame_stride : 2 * kPitch;
  p->launch_iters = o.launch_iters;
  p->device = device_id;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
  rc = create_device(p);
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_stft_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_stft_plan_destroy(tfft_stft_plan* p) {
  if (!p) return;
  if (p->d_tables) (void)hipFree(p->d_tables);
  if (p->d_window) (void)hipFree(p->d_window);
  delete p;
}

int tfft_stft_plan_set_window(tfft_stft_plan* p, const void* window, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!window) return fail(TFFT_ERR_ARG, "null window pointer");
  const int rc = check_current(p->device);
  if (rc) return rc;
  CONV_HIP(hipMemcpyAsync(p->d_window, window, kN * 2, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  p->have_window = true;
  return TFFT_OK;
}

int tfft_stft_exec(const tfft_stft_plan* p, const void* in, void* out_re, void* out_im, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_window) return fail(TFFT_ERR_ARG, "no window: call tfft_stft_plan_set_window first");
  if (!in || !out_re || !out_im) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out_re) | reinterpret_cast<uintptr_t>(out_im)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  // frames of one signal overlap, and frames are work items of different waves that run in no defined order: the input's extent
  // (gaps included) must stay clear of both output planes' extents
  const uint64_t in_bytes = 2 * ((p->rows - 1) * p->in_stride + p->length), out_bytes = 2 * ((p->total - 1) * p->out_stride + kBins);
  if (blocks_overlap(in, in_bytes, out_re, out_bytes) || blocks_overlap(in, in_bytes, out_im, out_bytes))
    return fail(TFFT_ERR_ARG, "input and output overlap (an STFT plan cannot run in place: frames share input samples)");
  // the two planes may interleave ([RE h | IM h] blocks); their written parts, 2049 halves per frame, may not share a half
  if (seqs_overlap(out_re, p->out_stride, kBins, out_im, p->out_stride, kBins, p->total))
    return fail(TFFT_ERR_ARG, "the RE and IM output planes overlap");
  const int rc = check_current(p->device);
  if (rc) return rc;
  const stft4096::geometry geo = {static_cast<int32_t>(p->length / 8), p->frames > 1 ? static_cast<int32_t>(p->hop / 8) : 0,
                                  static_cast<int32_t>(p->pad / 8), static_cast<uint32_t>(p->frames)};
  uint32_t live, grid;
  conv_shape(p->items, p->num_cus, p->launch_iters, live, grid);
  hipLaunchKernelGGL(stft4096::stft4096_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(in), static_cast<const uint16_t*>(p->d_window), static_cast<uint16_t*>(out_re),
                     static_cast<uint16_t*>(out_im), p->in_stride, p->out_stride, geo, static_cast<uint32_t>(p->total),
                     static_cast<uint32_t>(p->items), live, static_cast<const uint8_t*>(p->d_tables));
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_stft_plan_num_launches(const tfft_stft_plan* p) { return p ? 1 : 0; }

int tfft_stft_plan_kernels(const tfft_stft_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("stft4096::stft4096_kernel\n", 1, buf, bytes);
}

}  // extern "C"
