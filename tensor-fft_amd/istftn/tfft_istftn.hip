// tfft_istftn.hip — host side and C ABI (include/tfft_istftn.h) of the short-frame inverse STFT add-on, libtfft_istftn.so: the
// plans of include/tfft_istft.h at the frame lengths 512, 1024 and 2048.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp and rsplit.hpp, header only, for the device helpers, and k256r.hpp, in the host
// pass, for the constant tables of the frames kernel (the add-on uploads a copy of its own). The error string, the HIP check, the
// ABI check, the launch_iters rule, the launch shape and the workspace rules come from conv/host_plumbing.hpp;
// tests/test_gpu_istftn.py holds the frames to tfft_exec_inverse and the output to the numpy overlap-add, bit for bit.
#include "../../include/tfft_istftn.h"
#include "istft256r.hpp"
#include "olan.hpp"
#include "../conv/host_plumbing.hpp"

// csrc/k256r.hpp for the host pass alone: build_tables, and what istft256r.hpp restates of it, held to the original below. In the
// device pass the header would add stockham::copy_kernel, which is no template, to this library's code object; that pass parses
// the host code too, so what it calls is declared for both.
namespace k256r_host {
void build_tables(int R, std::vector<uint8_t>& blob);       // k256r::build_tables(R, blob): sequential scaling, the default plan's
}
#if !defined(__HIP_DEVICE_COMPILE__)
#include "../csrc/k256r.hpp"

void k256r_host::build_tables(int R, std::vector<uint8_t>& blob) { k256r::build_tables(R, blob); }

static_assert(istft256r::kDataBytes == k256r::kDataBytes && istft256r::kOffFa == k256r::kOffFa && istft256r::kOffFb == k256r::kOffFb &&
                  istft256r::kOffS == k256r::kOffS,
              "istft256r.hpp and csrc/k256r.hpp disagree on the table blob");
template <int R>
constexpr bool same_layout() {
  for (int n1 = 0; n1 < 16; ++n1)
    if (istft256r::swz(R, n1) != k256r::swz(R, n1)) return false;
  // slot_of is a permutation of the chunks of a plane and its own inverse
  for (uint32_t j = 0; j < 32u * R; ++j)
    if (istft256r::slot_of(R, j) >= 32u * R || istft256r::slot_of(R, istft256r::slot_of(R, j)) != j) return false;
  return istft256r::table_bytes<R>() == k256r::table_bytes<R>() && istft256r::lds_bytes<R>() == k256r::lds_bytes<R>();
}
static_assert(same_layout<2>() && same_layout<4>() && same_layout<8>(), "istft256r.hpp and csrc/k256r.hpp disagree on the LDS image");
#endif

namespace {

constexpr uint64_t kMaxExtent = uint64_t{1} << 62;       // halves: a byte offset then fits 64 bits

inline uint64_t bins_of(uint64_t n) { return n / 2 + 1; }
inline uint64_t pitch_of(uint64_t n) { return (bins_of(n) + 7) & ~uint64_t{7}; }      // tfft_rplan_spectrum_pitch(n)

int check_n(uint32_t n) {
  if (n == 4096) return fail(TFFT_ERR_ARG, "n = 4096 is the plan of include/tfft_istft.h: use tfft_istft_plan_create");
  if (n != 512 && n != 1024 && n != 2048) return fail(TFFT_ERR_ARG, "n must be 512, 1024 or 2048 (" + std::to_string(n) + ")");
  return TFFT_OK;
}

// the frames per signal; `frames` may be null. The refusals of tfft_stftn.h
int check_geometry(uint32_t n32, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  const int rc = check_n(n32);
  if (rc) return rc;
  const uint64_t n = n32;
  if (length < 8 || length % 8) return fail(TFFT_ERR_ARG, "length must be a multiple of 8 and at least 8");
  if (length > kMaxLength) return fail(TFFT_ERR_ARG, "length must not exceed 2^26");
  if (hop < 8 || hop % 8) return fail(TFFT_ERR_ARG, "hop must be a multiple of 8 and at least 8");
  if (pad % 8 || pad >= n) return fail(TFFT_ERR_ARG, "pad must be a multiple of 8 and below " + std::to_string(n));
  if (length + 2 * pad < n) return fail(TFFT_ERR_ARG, "length + 2 * pad must be at least " + std::to_string(n) + ": there is no frame");
  if (frames) *frames = 1 + (length + 2 * pad - n) / hop;
  return TFFT_OK;
}

int check_shape(uint32_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int flags, uint64_t* frames) {
  uint64_t f = 0;
  const int rc = check_geometry(n, length, hop, pad, &f);
  if (rc) return rc;
  if (flags & ~TFFT_ISTFTN_RAW_SUM)
    return fail(TFFT_ERR_ARG, "unknown flag bits (" + std::to_string(flags) + "): tfft_istftn_opts.flags must be 0 or TFFT_ISTFTN_RAW_SUM");
  if (rows == 0 || rows > 0xffffffffull) return fail(TFFT_ERR_ARG, "rows must be in [1, 2^32)");
  // frames <= 2^23 + 1: the product cannot overflow 64 bits. A frame index 2 b + 1 of transform b must fit 32 bits
  if (rows * f > 0xffffffffull) return fail(TFFT_ERR_ARG, "the frame count rows * frames must be below 2^32");
  if (frames) *frames = f;
  return TFFT_OK;
}

// (count - 1) * stride + len below 2^62 halves, without overflow
bool extent_fits(uint64_t count, uint64_t stride, uint64_t len) { return count == 1 || stride <= (kMaxExtent - len - 1) / (count - 1); }

int check_strides(uint64_t n, uint64_t rows, uint64_t length, uint64_t frames, uint64_t in_stride, uint64_t out_stride) {
  const std::string bins = std::to_string(bins_of(n));
  if (in_stride && (in_stride % 8 || in_stride < bins_of(n)))
    return fail(TFFT_ERR_ARG, "in_frame_stride must be 0 or a multiple of 8 that is >= " + bins);
  if (out_stride && (out_stride % 8 || out_stride < length))
    return fail(TFFT_ERR_ARG, "out_sig_stride must be 0 or a multiple of 8 that is >= length");
  if (!extent_fits(rows * frames, in_stride ? in_stride : 2 * pitch_of(n), bins_of(n)))
    return fail(TFFT_ERR_ARG, "the input extent (rows * frames - 1) * in_frame_stride + " + bins + " must be below 2^62 halves");
  if (!extent_fits(rows, out_stride ? out_stride : length, length))
    return fail(TFFT_ERR_ARG, "the output extent (rows - 1) * out_sig_stride + length must be below 2^62 halves");
  return TFFT_OK;
}

}  // namespace

struct tfft_istftn_plan {
  uint64_t n = 0, rows = 0, length = 0, hop = 0, pad = 0, frames = 0, total = 0, batch = 0, groups = 0, in_stride = 0, out_stride = 0;
  uint32_t launch_iters = 0;
  int radix = 0;                     // R = n / 256
  int flags = 0, device = 0, num_cus = 256;
  void* d_tables = nullptr;          // k256r::build_tables(R)
  uint16_t* d_window = nullptr;      // n halves, the plan's own copy
  bool have_window = false;
  size_t ws_need = 0;                // rows * frames * n halves: the time-domain frames
  mutable std::mutex ws_mutex;
  mutable void* ws = nullptr;
  mutable bool ws_owned = false;
};

namespace {

template <int R>
int create_device(tfft_istftn_plan* p) {
  std::vector<uint8_t> blob;
  k256r_host::build_tables(R, blob);
  CONV_HIP(hipMalloc(&p->d_tables, blob.size()));
  CONV_HIP(hipMemcpy(p->d_tables, blob.data(), blob.size(), hipMemcpyHostToDevice));
  CONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_window), p->n * 2));
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(istft256r::frames_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               istft256r::lds_bytes<R>()));
  return TFFT_OK;
}

template <int R>
void launch_frames(const tfft_istftn_plan* p, const void* in_re, const void* in_im, uint16_t* frames, hipStream_t stream) {
  uint32_t live, grid;
  conv_shape(p->groups, p->num_cus, p->launch_iters, live, grid);
  hipLaunchKernelGGL(istft256r::frames_kernel<R>, dim3(grid), dim3(k4096::kThreads), istft256r::lds_bytes<R>(), stream,
                     static_cast<const uint16_t*>(in_re), static_cast<const uint16_t*>(in_im), frames, p->in_stride,
                     static_cast<uint32_t>(p->total), static_cast<uint32_t>(p->batch), live, static_cast<const uint8_t*>(p->d_tables));
}

}  // namespace

extern "C" {

const char* tfft_istftn_last_error(void) { return g_err.c_str(); }

int tfft_istftn_geometry(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  g_err.clear();
  return check_geometry(n, length, hop, pad, frames);
}

int tfft_istftn_describe(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  uint64_t frames = 0;
  const int rc = check_shape(n, rows, length, hop, pad, flags, &frames);
  if (rc) return rc;
  return copy_text("istft256r" + std::to_string(n / 256) + ":" + std::to_string(n) + " x " + std::to_string(frames) + " + ola", buf, bytes);
}

int tfft_istftn_plan_create(uint32_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id, const tfft_istftn_opts* opts,
                            tfft_istftn_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_istftn_opts o = TFFT_ISTFTN_OPTS_INIT;
  int rc = take_opts(opts, "tfft_istftn_opts", o);
  if (rc) return rc;
  uint64_t frames = 0;
  rc = check_shape(n, rows, length, hop, pad, o.flags, &frames);
  if (rc == TFFT_OK) rc = check_strides(n, rows, length, frames, o.in_frame_stride, o.out_sig_stride);
  if (rc == TFFT_OK) rc = check_launch_iters(o.launch_iters);
  if (rc == TFFT_OK) rc = check_abi("libtfft_istftn.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_istftn_plan* p = new tfft_istftn_plan;
  p->n = n;
  p->radix = static_cast<int>(n / 256);
  p->rows = rows;
  p->length = length;
  p->hop = hop;
  p->pad = pad;
  p->frames = frames;
  p->total = rows * frames;
  p->batch = (p->total + 1) / 2;
  const uint64_t per_wave = 16 / p->radix;                 // transforms a wave takes per iteration
  p->groups = (p->batch + per_wave - 1) / per_wave;
  p->in_stride = o.in_frame_stride ? o.in_frame_stride : 2 * pitch_of(n);
  p->out_stride = o.out_sig_stride ? o.out_sig_stride : length;
  p->launch_iters = o.launch_iters;
  p->flags = o.flags;
  p->device = device_id;
  p->ws_need = static_cast<size_t>(p->total * n * 2);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
  rc = p->radix == 2 ? create_device<2>(p) : p->radix == 4 ? create_device<4>(p) : create_device<8>(p);
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_istftn_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_istftn_plan_destroy(tfft_istftn_plan* p) {
  if (!p) return;
  if (p->d_tables) (void)hipFree(p->d_tables);
  if (p->d_window) (void)hipFree(p->d_window);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_istftn_plan_set_window(tfft_istftn_plan* p, const void* window, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!window) return fail(TFFT_ERR_ARG, "null window pointer");
  const int rc = check_current(p->device);
  if (rc) return rc;
  CONV_HIP(hipMemcpyAsync(p->d_window, window, p->n * 2, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  p->have_window = true;
  return TFFT_OK;
}

size_t tfft_istftn_plan_workspace_bytes(const tfft_istftn_plan* p) { return p ? p->ws_need : 0; }

int tfft_istftn_plan_set_workspace(tfft_istftn_plan* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_set(p, device_ptr, bytes);
}

int tfft_istftn_plan_prepare(tfft_istftn_plan* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_prepare(p);
}

int tfft_istftn_exec(const tfft_istftn_plan* p, const void* in_re, const void* in_im, void* out, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_window) return fail(TFFT_ERR_ARG, "no window: call tfft_istftn_plan_set_window first");
  if (!in_re || !in_im || !out) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(in_re) | reinterpret_cast<uintptr_t>(in_im) | reinterpret_cast<uintptr_t>(out)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  // whole extents, gaps included (conservative): the inputs are never written, and frames are work items that run in no defined order
  const uint64_t in_bytes = 2 * ((p->total - 1) * p->in_stride + bins_of(p->n)), out_bytes = 2 * ((p->rows - 1) * p->out_stride + p->length);
  if (blocks_overlap(out, out_bytes, in_re, in_bytes) || blocks_overlap(out, out_bytes, in_im, in_bytes))
    return fail(TFFT_ERR_ARG, "output and input overlap (an ISTFT plan cannot run in place)");
  int rc = check_current(p->device);
  if (rc == TFFT_OK) rc = ws_ensure(p);
  if (rc) return rc;
  if (blocks_overlap(p->ws, p->ws_need, out, out_bytes)) return fail(TFFT_ERR_ARG, "the workspace overlaps the output");
  if (blocks_overlap(p->ws, p->ws_need, in_re, in_bytes) || blocks_overlap(p->ws, p->ws_need, in_im, in_bytes))
    return fail(TFFT_ERR_ARG, "the workspace overlaps the input");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint16_t* const frames = static_cast<uint16_t*>(p->ws);
  if (p->radix == 2) launch_frames<2>(p, in_re, in_im, frames, s);
  else if (p->radix == 4) launch_frames<4>(p, in_re, in_im, frames, s);
  else launch_frames<8>(p, in_re, in_im, frames, s);
  CONV_HIP(hipGetLastError());
  // The kernel's frame range is signed 64-bit arithmetic on hop. With more than one frame per signal (F - 1) * hop <= L + 2 pad - n
  // < 2^27; a plan with ONE frame may have any hop up to 2^64 - 8, and all the kernel needs of it is that no second frame starts
  // inside the padded signal: such a plan passes L + 2 pad, which is what every hop beyond L + 2 pad - n amounts to
  const uint64_t ola_hop = p->frames > 1 ? p->hop : p->length + 2 * p->pad;
  const olan::ola_geometry geo = {p->rows, p->length / 8, ola_hop, p->out_stride, static_cast<uint32_t>(p->pad), static_cast<uint32_t>(p->frames),
                                  static_cast<uint32_t>(p->n)};
  const uint64_t blocks = (p->rows * (p->length / 8) + olan::kOlaBlock - 1) / olan::kOlaBlock;
  const uint32_t ola_grid = static_cast<uint32_t>(std::min<uint64_t>(blocks, static_cast<uint64_t>(p->num_cus) * 32));
  hipLaunchKernelGGL(olan::ola_kernel, dim3(ola_grid), dim3(olan::kOlaBlock), 0, s, static_cast<const uint16_t*>(frames),
                     static_cast<const uint16_t*>(p->d_window), static_cast<uint16_t*>(out), geo, (p->flags & TFFT_ISTFTN_RAW_SUM) ? 1 : 0);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_istftn_plan_num_launches(const tfft_istftn_plan* p) { return p ? 2 : 0; }

int tfft_istftn_plan_kernels(const tfft_istftn_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("istft256r::frames_kernel<" + std::to_string(p->radix) + ">\nolan::ola_kernel\n", 2, buf, bytes);
}

}  // extern "C"
