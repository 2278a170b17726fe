// tfft_gconv.hip — host side and C ABI (include/tfft_gconv.h) of the gated causal convolution add-on, libtfft_gconv.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (the sub-plan of the composed path,
// tfft_device_check, tfft_abi_version); from csrc/ it takes k4096.hpp, header only, for the device helpers and
// the constant tables of the fused kernel (the add-on uploads a copy of its own). The host code is that of lconv/tfft_lconv.hip
// (which this library does not link) with the gates, their strides and the skip weight added.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfft_gconv.h"
#include "gconv4096.hpp"
#include "gate_copy.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int hip_fail(hipError_t e, const char* what) { return fail(TFFT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
// a failing call into libtfft_conv.so / libtfft.so: its message becomes ours
int pass_conv(int rc) {
  if (rc != TFFT_OK) g_err = tfft_conv_last_error();
  return rc;
}
int pass_tfft(int rc) {
  if (rc != TFFT_OK) g_err = tfft_last_error();
  return rc;
}
#define GCONV_HIP(call)                               \
  do {                                                \
    const hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) return hip_fail(e_, #call); \
  } while (0)

inline bool is_pow2(uint64_t v) { return v && !(v & (v - 1)); }
inline int ilog2(uint64_t v) {
  int l = 0;
  while (v >>= 1) ++l;
  return l;
}
inline size_t round256(size_t v) { return (v + 255) & ~size_t{255}; }

constexpr uint64_t kMinN = 256, kMaxN = uint64_t{1} << 26;

int check_abi() {
  static const int version = tfft_abi_version();
  if (version != TFFT_ABI_VERSION)
    return fail(TFFT_ERR_ARG, "libtfft.so speaks ABI " + std::to_string(version) + ", libtfft_gconv.so was built against ABI " +
                                  std::to_string(TFFT_ABI_VERSION) + ": rebuild the add-on");
  return TFFT_OK;
}

uint64_t fft_length(uint64_t length, uint64_t taps) {
  if (!length || !taps || length > kMaxN || taps > kMaxN) return 0;
  const uint64_t need = std::max(length + taps - 1, kMinN);
  uint64_t n = kMinN;
  while (n < need) n *= 2;
  return n > kMaxN ? 0 : n;
}

int check_shape(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int flags) {
  if (length < 8 || length % 8) return fail(TFFT_ERR_ARG, "length must be a multiple of 8 and at least 8");
  if (taps == 0) return fail(TFFT_ERR_ARG, "taps must be at least 1");
  if (flags & ~(TFFT_GCONV_PRE_GATE | TFFT_GCONV_POST_GATE | TFFT_GCONV_COMPOSED)) return fail(TFFT_ERR_ARG, "unknown flag bits (" + std::to_string(flags) + ")");
  if (rows == 0 || rows > 0xffffffffull) return fail(TFFT_ERR_ARG, "rows must be in [1, 2^32)");
  if (channels == 0 || channels > 0xffffffffull) return fail(TFFT_ERR_ARG, "channels must be in [1, 2^32)");
  if (rows * channels > 0xffffffffull) return fail(TFFT_ERR_ARG, "rows * channels must be below 2^32");
  if (!fft_length(length, taps))
    return fail(TFFT_ERR_ARG, "the transform length (the power of two >= length + taps - 1) must not exceed 2^26");
  return TFFT_OK;
}
int check_stride(uint64_t length, uint64_t stride, const char* which) {
  if (stride && (stride % 8 || stride < length))
    return fail(TFFT_ERR_ARG, std::string(which) + "_seq_stride must be 0 or a multiple of 8 that is >= length");
  return TFFT_OK;
}

// the fused kernel takes every shape that fits its 4096-point transform with the kept half in front: it moves L halves per sequence
// and gate each way whatever the padding, so a shorter transform (three steps and two copies) has nothing to offer
inline bool fused_shape(uint64_t length, uint64_t taps, int flags) {
  return length <= 2048 && length + taps - 1 <= 4096 && !(flags & TFFT_GCONV_COMPOSED);
}
inline uint64_t plan_length(uint64_t length, uint64_t taps, int flags) { return fused_shape(length, taps, flags) ? 4096 : fft_length(length, taps); }

// Element-exact test whether two sets of sequences (count blocks of len halves, `stride` halves apart) share a half: the test of
// tfft_conv_exec.
bool seqs_overlap(const void* pa, uint64_t sa, const void* pb, uint64_t sb, uint64_t count, uint64_t len) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(pa), b = reinterpret_cast<uintptr_t>(pb);
  const uintptr_t a_end = a + 2 * ((count - 1) * sa + len), b_end = b + 2 * ((count - 1) * sb + len);
  if (a_end <= b || b_end <= a) return false;
  if (count == 1 || sa != sb) return true;            // different strides: conservative
  const uint64_t d = static_cast<uint64_t>(a > b ? a - b : b - a) / 2 % sa;
  return d < len || sa - d < len;
}

// ---- binary16 on the host, bit by bit (round to nearest even, one rounding from fp64)
double from_half(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 1023;
  double v;
  if (e == 0)
    v = std::ldexp(static_cast<double>(m), -24);
  else if (e == 31)
    v = m ? NAN : INFINITY;
  else
    v = std::ldexp(static_cast<double>(m + 1024), e - 25);
  return (h & 0x8000) ? -v : v;
}
uint16_t to_half(double v) {
  const uint16_t sign = std::signbit(v) ? 0x8000 : 0;
  if (v != v) return sign | 0x7e00;
  const double a = std::fabs(v);
  if (a >= 65520.0) return sign | 0x7c00;
  if (a == 0.0) return sign;
  int e2;
  (void)std::frexp(a, &e2);                                 // a = f * 2^e2, f in [0.5, 1)
  const int e = std::max(e2 - 1, -14);                      // the binade whose spacing applies (subnormals share the lowest)
  const long r = std::lrint(std::ldexp(a, 10 - e));         // exact scaling, then the one rounding (to nearest even)
  if (e == -14 && r < 1024) return sign | static_cast<uint16_t>(r);
  return sign | static_cast<uint16_t>(((e + 15) << 10) + (r - 1024));    // r = 2048 carries into the exponent
}

// in-place radix-2 fp64 FFT (forward, unscaled). Twiddles w^k = A[k >> s] B[k & mask] from two tables of about sqrt(n) entries,
// each entry from sin / cos directly: one product per twiddle, no error growth along a recurrence.
void fft64(std::vector<std::complex<double>>& a) {
  const uint64_t n = a.size();
  const int lg = ilog2(n);
  for (uint64_t i = 1, j = 0; i < n; ++i) {
    uint64_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  const int s = lg / 2;
  const uint64_t lo_n = uint64_t{1} << s, hi_n = std::max<uint64_t>(n >> s, 1);
  std::vector<std::complex<double>> ta(hi_n), tb(lo_n);
  const double step = -2.0 * M_PI / static_cast<double>(n);
  for (uint64_t i = 0; i < hi_n; ++i) ta[i] = {std::cos(step * static_cast<double>(i << s)), std::sin(step * static_cast<double>(i << s))};
  for (uint64_t i = 0; i < lo_n; ++i) tb[i] = {std::cos(step * static_cast<double>(i)), std::sin(step * static_cast<double>(i))};
  for (uint64_t m = 2; m <= n; m *= 2) {
    const uint64_t half = m / 2, mul = n / m;
    for (uint64_t k = 0; k < n; k += m)
      for (uint64_t j = 0; j < half; ++j) {
        const uint64_t idx = j * mul;
        const std::complex<double> w = ta[idx >> s] * tb[idx & (lo_n - 1)];
        const std::complex<double> u = a[k + j], t = w * a[k + j + half];
        a[k + j] = u + t;
        a[k + j + half] = u - t;
      }
  }
}

// one filter: H' = FFT of the zero-padded taps with the skip weight added to tap 0 in fp64, each component rounded once; exactly
// Hermitian, Im of bins 0 and n / 2 exactly 0. A skip of zero adds nothing, not even to the sign of a zero tap: the result is then
// bit for bit tfft_lconv_spectrum_host's.
void spectrum(const uint16_t* taps, uint64_t num_taps, uint16_t skip, uint64_t n, uint16_t* out_re, uint16_t* out_im) {
  std::vector<std::complex<double>> a(n);
  for (uint64_t j = 0; j < num_taps; ++j) a[j] = from_half(taps[j]);
  if (skip & 0x7fff) a[0] += from_half(skip);
  fft64(a);
  for (uint64_t k = 0; k <= n / 2; ++k) {
    const uint16_t re = to_half(a[k].real());
    const uint16_t im = (k == 0 || k == n / 2) ? 0 : to_half(a[k].imag());
    out_re[k] = re;
    out_im[k] = im;
    if (k && k < n / 2) {
      out_re[n - k] = re;
      out_im[n - k] = (im & 0x7fff) ? (im ^ 0x8000) : 0;        // conj; a zero stays +0
    }
  }
}

}  // namespace

struct tfft_gconv_plan {
  uint64_t rows = 0, channels = 0, length = 0, taps = 0, n = 0, items = 0, in_stride = 0, out_stride = 0, pre_stride = 0, post_stride = 0;
  uint32_t launch_iters = 0;
  int device = 0, flags = 0, num_cus = 256;
  bool fused = false, pre = false, post = false;
  void* d_tables = nullptr;          // fused: F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // fused: [channels][RE 4096 | IM 4096] in conv4096::filter_slot order
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
  GCONV_HIP(hipMalloc(&mem, need));
  p->ws = mem;
  p->ws_bytes = need;
  p->ws_owned = true;
  return bind_workspace(p);
}

// launch shape of the fused kernel: conv4096_kernel's (tfft_conv.hip, conv4096_shape) applied to the item count; launch_iters as
// tfft_gconv_opts states it
void gconv4096_shape(const tfft_gconv_plan* p, uint32_t& live, uint32_t& grid) {
  const uint64_t cus = static_cast<uint64_t>(p->num_cus);
  live = 8;
  for (uint32_t l = 1; l <= 4; l *= 2)
    if (p->items <= cus * l) {
      live = l;
      break;
    }
  const uint64_t blocks = (p->items + live - 1) / live;
  if (p->launch_iters >= TFFT_LAUNCH_PERSISTENT) {
    grid = static_cast<uint32_t>(std::min(blocks, cus));
  } else if (p->launch_iters) {
    grid = static_cast<uint32_t>((blocks + p->launch_iters - 1) / p->launch_iters);
  } else {
    const uint64_t iters = blocks >= 4 * cus ? 2 : 1;
    grid = static_cast<uint32_t>(std::max<uint64_t>(std::min<uint64_t>(blocks, cus), (blocks + iters - 1) / iters));
  }
}

// the instantiation a plan launches
const void* fused_kernel(const tfft_gconv_plan* p) {
  if (p->pre) return p->post ? reinterpret_cast<const void*>(gconv4096::gconv4096_kernel<true, true>) : reinterpret_cast<const void*>(gconv4096::gconv4096_kernel<true, false>);
  return p->post ? reinterpret_cast<const void*>(gconv4096::gconv4096_kernel<false, true>) : reinterpret_cast<const void*>(gconv4096::gconv4096_kernel<false, false>);
}
const char* tf_text(bool v) { return v ? "true" : "false"; }

int create_fused(tfft_gconv_plan* p) {
  std::vector<uint8_t> blob;
  k4096::build_tables(blob);
  GCONV_HIP(hipMalloc(&p->d_tables, k4096::kOffF1n));
  GCONV_HIP(hipMemcpy(p->d_tables, blob.data(), k4096::kOffF1n, hipMemcpyHostToDevice));
  GCONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_filter), static_cast<size_t>(p->channels) * 8192 * 2));
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  GCONV_HIP(hipFuncSetAttribute(fused_kernel(p), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
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
  if (out.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return TFFT_OK;
}

int tfft_gconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_gconv_opts* opts,
                           tfft_gconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_gconv_opts o = TFFT_GCONV_OPTS_INIT;
  if (opts) {
    if (opts->struct_size != sizeof(tfft_gconv_opts))
      return fail(TFFT_ERR_ARG, "tfft_gconv_opts.struct_size = " + std::to_string(opts->struct_size) + " is not the size of a layout this library knows (" +
                                    std::to_string(sizeof(tfft_gconv_opts)) + ")");
    if (opts->reserved_) return fail(TFFT_ERR_ARG, "tfft_gconv_opts.reserved_ must be 0");
    o = *opts;
  }
  int rc = check_shape(rows, channels, length, taps, o.flags);
  if (rc == TFFT_OK) rc = check_stride(length, o.in_seq_stride, "in");
  if (rc == TFFT_OK) rc = check_stride(length, o.out_seq_stride, "out");
  if (rc == TFFT_OK) rc = check_stride(length, o.pre_seq_stride, "pre");
  if (rc == TFFT_OK) rc = check_stride(length, o.post_seq_stride, "post");
  if (rc == TFFT_OK && o.launch_iters > TFFT_LAUNCH_PERSISTENT) rc = fail(TFFT_ERR_ARG, "launch_iters must be 0 .. 65535");
  if (rc == TFFT_OK) rc = check_abi();
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  GCONV_HIP(hipGetDevice(&prev));
  GCONV_HIP(hipSetDevice(device_id));
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
  if (rc) {
    const std::string keep = g_err;
    tfft_gconv_plan_destroy(p);
    g_err = keep;
    return rc;
  }
  *out = p;
  return TFFT_OK;
}

void tfft_gconv_plan_destroy(tfft_gconv_plan* p) {
  if (!p) return;
  tfft_conv_plan_destroy(p->sub);
  if (p->d_tables) (void)hipFree(p->d_tables);
  if (p->d_filter) (void)hipFree(p->d_filter);
  if (p->d_spec) (void)hipFree(p->d_spec);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_gconv_plan_set_taps(tfft_gconv_plan* p, const void* taps, const void* skip, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!taps) return fail(TFFT_ERR_ARG, "null taps pointer");
  int cur = 0;
  GCONV_HIP(hipGetDevice(&cur));
  if (cur != p->device) return fail(TFFT_ERR_ARG, "plan was created for another device than the current one");
  const size_t plane = static_cast<size_t>(p->channels) * p->n;
  std::vector<uint16_t> h(static_cast<size_t>(p->channels) * p->taps), d(p->channels, 0), spec(2 * plane);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // through the host: the spectrum is built once per filter, not per execution. Everything enqueued on `stream` before the call
  // (the kernel that produced the taps) is waited for; executions still in flight keep reading the old spectrum until then, so the
  // device is drained before it is replaced.
  GCONV_HIP(hipMemcpyAsync(h.data(), taps, h.size() * 2, hipMemcpyDeviceToHost, s));
  if (skip) GCONV_HIP(hipMemcpyAsync(d.data(), skip, d.size() * 2, hipMemcpyDeviceToHost, s));
  GCONV_HIP(hipStreamSynchronize(s));
  for (uint64_t c = 0; c < p->channels; ++c) spectrum(h.data() + c * p->taps, p->taps, d[c], p->n, spec.data() + c * p->n, spec.data() + plane + c * p->n);
  if (p->have_taps) GCONV_HIP(hipDeviceSynchronize());
  GCONV_HIP(hipMemcpy(p->d_spec, spec.data(), spec.size() * 2, hipMemcpyHostToDevice));
  if (p->fused) {
    std::vector<uint16_t> img(2 * plane);
    for (uint64_t c = 0; c < p->channels; ++c)
      for (uint32_t k = 0; k < 4096; ++k) {
        const uint32_t slot = gconv4096::filter_slot(k);
        img[c * 8192 + slot] = spec[c * 4096 + k];
        img[c * 8192 + 4096 + slot] = spec[plane + c * 4096 + k];
      }
    GCONV_HIP(hipMemcpy(p->d_filter, img.data(), img.size() * 2, hipMemcpyHostToDevice));
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
  GCONV_HIP(hipMemcpy(h_re, p->d_spec, plane * 2, hipMemcpyDeviceToDevice));
  GCONV_HIP(hipMemcpy(h_im, p->d_spec + plane, plane * 2, hipMemcpyDeviceToDevice));
  GCONV_HIP(hipDeviceSynchronize());
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
  GCONV_HIP(hipGetDevice(&prev));
  GCONV_HIP(hipSetDevice(p->device));
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
  } else if (seqs_overlap(in, p->in_stride, out, p->out_stride, seqs, p->length)) {
    return fail(TFFT_ERR_ARG, "input and output overlap without being identical (only exact in-place or disjoint sequences are supported)");
  }
  // a gate is read while other items' results are written: it shares no half with the output, not even in place
  if (pre && seqs_overlap(pre, p->pre_stride, out, p->out_stride, seqs, p->length)) return fail(TFFT_ERR_ARG, "the pre gate and the output overlap");
  if (post && seqs_overlap(post, p->post_stride, out, p->out_stride, seqs, p->length)) return fail(TFFT_ERR_ARG, "the post gate and the output overlap");
  int cur = 0;
  GCONV_HIP(hipGetDevice(&cur));
  if (cur != p->device) return fail(TFFT_ERR_ARG, "plan was created for another device than the current one");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t chunks = static_cast<uint32_t>(p->length / 8);
  const uint16_t* const x = static_cast<const uint16_t*>(in);
  const uint16_t* const gp = static_cast<const uint16_t*>(pre);
  const uint16_t* const gq = static_cast<const uint16_t*>(post);
  uint16_t* const y = static_cast<uint16_t*>(out);
  const uint32_t rows = static_cast<uint32_t>(p->rows), channels = static_cast<uint32_t>(p->channels);
  if (p->fused) {
    uint32_t live, grid;
    gconv4096_shape(p, live, grid);
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
    GCONV_HIP(hipGetLastError());
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
  GCONV_HIP(hipGetLastError());
  rc = pass_conv(tfft_conv_exec(p->sub, blocks, blocks + p->n, blocks, blocks + p->n, s));
  if (rc) return rc;
  if (p->post)
    hipLaunchKernelGGL(gate_copy::crop_kernel<true>, grid_out, block, 0, s, blocks, gq, y, p->post_stride, p->out_stride, channels, chunks, log_n8, total_out);
  else
    hipLaunchKernelGGL(gate_copy::crop_kernel<false>, grid_out, block, 0, s, blocks, gq, y, p->post_stride, p->out_stride, channels, chunks, log_n8, total_out);
  GCONV_HIP(hipGetLastError());
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
  if (!buf || out.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small (" + std::to_string(out.size() + 1) + " bytes needed)");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return lines;
}

}  // extern "C"
