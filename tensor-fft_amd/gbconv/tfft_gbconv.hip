// tfft_gbconv.hip — host side and C ABI (include/tfft_gbconv.h) of the gradient add-on of the GATED overlap-save causal
// convolution, libtfft_gbconv.so.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp, header only. It links neither libtfft_bconv.so nor libtfft_gsconv.so: the
// geometry, the checks and the launch shapes of tfft_bconv.hip and the fp64 spectrum builder of tfft_gsconv.hip (the skip folded
// into tap 0) are restated below, and tests/test_gbconv_host.py and tests/test_gpu_gbconv.py hold them to the shipped code (the
// geometry and the refusals on the host, the spectrum to tfft_gconv_spectrum_host bit for bit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfft_gbconv.h"
#include "gbconv4096.hpp"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int hip_fail(hipError_t e, const char* what) { return fail(TFFT_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
// a failing call into libtfft.so: its message becomes ours
int pass_tfft(int rc) {
  if (rc != TFFT_OK) g_err = tfft_last_error();
  return rc;
}
#define GBCONV_HIP(call)                               \
  do {                                                \
    const hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) return hip_fail(e_, #call); \
  } while (0)

constexpr uint64_t kN = 4096, kMaxLength = uint64_t{1} << 26;      // the transform length; the longest sequence of tfft_sconv.h
constexpr uint64_t kWaves = 2048;                                  // 256 CUs x 8 waves: the work units the default P aims at
constexpr int kGates = TFFT_GBCONV_PRE_GATE | TFFT_GBCONV_POST_GATE;

int check_abi() {
  static const int version = tfft_abi_version();
  if (version != TFFT_ABI_VERSION)
    return fail(TFFT_ERR_ARG, "libtfft.so speaks ABI " + std::to_string(version) + ", libtfft_gbconv.so was built against ABI " +
                                  std::to_string(TFFT_ABI_VERSION) + ": rebuild the add-on");
  return TFFT_OK;
}

// the geometry of tfft_sconv_geometry, fixed by the number of taps alone
inline uint64_t halo_of(uint64_t taps) { return (taps - 1 + 63) / 64 * 64; }
inline uint64_t hop_of(uint64_t taps) { return kN - halo_of(taps); }
inline uint64_t segments_of(uint64_t length, uint64_t taps) { return (length + hop_of(taps) - 1) / hop_of(taps); }
// partial sums per channel of the tap gradient: one per item until the chip's waves are all busy, capped by the caller
inline uint64_t partials_of(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, uint64_t cap) {
  const uint64_t per_channel = (rows + 1) / 2 * segments_of(length, taps);
  const uint64_t p = std::min(per_channel, (kWaves + channels - 1) / channels);
  return cap ? std::min(p, cap) : p;
}
inline uint64_t kpad_of(uint64_t taps) { return (taps + 7) / 8 * 8; }

int check_length_taps(uint64_t length, uint64_t taps) {
  if (length < 8 || length % 8) return fail(TFFT_ERR_ARG, "length must be a multiple of 8 and at least 8");
  if (length > kMaxLength) return fail(TFFT_ERR_ARG, "length must not exceed 2^26");
  if (taps == 0) return fail(TFFT_ERR_ARG, "taps must be at least 1");
  if (taps > TFFT_GBCONV_MAX_TAPS)
    return fail(TFFT_ERR_ARG, "taps must not exceed 2049 (the halo of a 4096-sample window): longer filters run through tfft_gconv_plan_create");
  return TFFT_OK;
}

int check_shape(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int flags) {
  const int rc = check_length_taps(length, taps);
  if (rc) return rc;
  if (flags & ~kGates)
    return fail(TFFT_ERR_ARG, "unknown flag bits (" + std::to_string(flags) + "): tfft_gbconv_opts.flags takes TFFT_GBCONV_PRE_GATE and TFFT_GBCONV_POST_GATE only");
  if (rows == 0 || rows > 0xffffffffull) return fail(TFFT_ERR_ARG, "rows must be in [1, 2^32)");
  if (channels == 0 || channels > 0xffffffffull) return fail(TFFT_ERR_ARG, "channels must be in [1, 2^32)");
  if (rows * channels > 0xffffffffull) return fail(TFFT_ERR_ARG, "rows * channels must be below 2^32");
  // pairs * channels < 2^32 and segments <= 2^15: the product cannot overflow 64 bits
  if ((rows + 1) / 2 * channels * segments_of(length, taps) > 0xffffffffull)
    return fail(TFFT_ERR_ARG, "the item count ceil(rows / 2) * segments * channels must be below 2^32");
  return TFFT_OK;
}
int check_stride(uint64_t length, uint64_t stride, const char* which) {
  if (stride && (stride % 8 || stride < length))
    return fail(TFFT_ERR_ARG, std::string(which) + "_seq_stride must be 0 or a multiple of 8 that is >= length");
  return TFFT_OK;
}

// Element-exact test whether two sets of sequences (count blocks of len halves, `stride` halves apart) share a half: the test of
// tfft_sconv_exec.
bool seqs_overlap(const void* pa, uint64_t sa, const void* pb, uint64_t sb, uint64_t count, uint64_t len) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(pa), b = reinterpret_cast<uintptr_t>(pb);
  const uintptr_t a_end = a + 2 * ((count - 1) * sa + len), b_end = b + 2 * ((count - 1) * sb + len);
  if (a_end <= b || b_end <= a) return false;
  if (count == 1 || sa != sb) return true;            // different strides: conservative
  const uint64_t d = static_cast<uint64_t>(a > b ? a - b : b - a) / 2 % sa;
  return d < len || sa - d < len;
}
// a block of `bytes` against the whole extent of a set of sequences, gaps included (conservative)
bool block_overlaps(const void* block, uint64_t bytes, const void* seqs, uint64_t stride, uint64_t count, uint64_t len) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(block), b = reinterpret_cast<uintptr_t>(seqs);
  return a < b + 2 * ((count - 1) * stride + len) && b < a + bytes;
}

// two blocks of bytes
bool blocks_overlap(const void* pa, uint64_t bytes_a, const void* pb, uint64_t bytes_b) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(pa), b = reinterpret_cast<uintptr_t>(pb);
  return a < b + bytes_b && b < a + bytes_a;
}

// ---- binary16 on the host, bit by bit (round to nearest even, one rounding from fp64): tfft_gconv.hip's
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

// in-place radix-2 fp64 FFT of 4096 points (forward, unscaled): fft64 of tfft_sconv.hip
void fft64(std::vector<std::complex<double>>& a) {
  const uint64_t n = kN;
  for (uint64_t i = 1, j = 0; i < n; ++i) {
    uint64_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  const int s = 6;
  const uint64_t lo_n = uint64_t{1} << s, hi_n = n >> s;
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
// Hermitian, Im of bins 0 and n / 2 exactly 0. A skip of zero adds nothing, not even to the sign of a zero tap. (spectrum of
// tfft_gsconv.hip, statement by statement.)
void spectrum(const uint16_t* taps, uint64_t num_taps, uint16_t skip, uint16_t* out_re, uint16_t* out_im) {
  const uint64_t n = kN;
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
  uint16_t* d_filter = nullptr;      // conj(H'): [channels][RE 4096 | IM 4096] in conv4096::filter_slot order (input gradient)
  uint16_t* d_spec = nullptr;        // H': [RE: channels x 4096 | IM: channels x 4096], natural bin order (tfft_gbconv_plan_spectrum)
  bool have_taps = false;
  size_t ws_need = 0;                // channels * partials * kpad floats
  mutable std::mutex ws_mutex;
  mutable void* ws = nullptr;
  mutable bool ws_owned = false;
};

namespace {

// launch shape of the input gradient: sconv4096_kernel's (tfft_sconv.hip, sconv4096_shape)
void dgrad_shape(const tfft_gbconv_plan* p, uint32_t& live, uint32_t& grid) {
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

// launch shape of the tap gradient: every work unit (c, q) is one wave of its own, in workgroups of up to four (one per SIMD); as
// few per workgroup as still cover the units with one workgroup per CU, as the shape above. The units, not the launch, fix the
// order of the additions.
void wgrad_shape(const tfft_gbconv_plan* p, uint32_t& live, uint32_t& grid) {
  const uint64_t cus = static_cast<uint64_t>(p->num_cus), units = p->channels * p->partials;
  live = gbconv4096::kWgradWaves;
  for (uint32_t l = 1; l < live; l *= 2)
    if (units <= cus * l) {
      live = l;
      break;
    }
  grid = static_cast<uint32_t>((units + live - 1) / live);
}

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
const char* tf_text(bool v) { return v ? "true" : "false"; }

int create_device(tfft_gbconv_plan* p) {
  std::vector<uint8_t> blob;
  k4096::build_tables(blob);
  GBCONV_HIP(hipMalloc(&p->d_tables, k4096::kOffF1n));
  GBCONV_HIP(hipMemcpy(p->d_tables, blob.data(), k4096::kOffF1n, hipMemcpyHostToDevice));
  GBCONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_filter), static_cast<size_t>(p->channels) * 8192 * 2));
  GBCONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_spec), static_cast<size_t>(p->channels) * kN * 4));
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  GBCONV_HIP(hipFuncSetAttribute(plan_dgrad(p), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  GBCONV_HIP(hipFuncSetAttribute(plan_wgrad(p), hipFuncAttributeMaxDynamicSharedMemorySize, gbconv4096::kWgradLdsBytes));
  return TFFT_OK;
}

// the rule of tfft_conv.h: the workspace is settled once, by the caller, by prepare or by the first execution
int ensure_workspace(const tfft_gbconv_plan* p) {
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  if (p->ws) return TFFT_OK;
  void* mem = nullptr;
  GBCONV_HIP(hipMalloc(&mem, p->ws_need));
  p->ws = mem;
  p->ws_owned = true;
  return TFFT_OK;
}

int check_current(const tfft_gbconv_plan* p) {
  int cur = 0;
  GBCONV_HIP(hipGetDevice(&cur));
  if (cur != p->device) return fail(TFFT_ERR_ARG, "plan was created for another device than the current one");
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
  const int rc = check_shape(rows, channels, length, taps, 0);
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
  const int rc = check_shape(rows, channels, length, taps, flags);
  if (rc) return rc;
  const std::string out = "gbconv4096:4096" + gate_text(flags) + " x " + std::to_string(segments_of(length, taps)) + " | partials " +
                          std::to_string(partials_of(rows, channels, length, taps, partials));
  if (out.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return TFFT_OK;
}

int tfft_gbconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_gbconv_opts* opts,
                           tfft_gbconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_gbconv_opts o = TFFT_GBCONV_OPTS_INIT;
  if (opts) {
    if (opts->struct_size != sizeof(tfft_gbconv_opts))
      return fail(TFFT_ERR_ARG, "tfft_gbconv_opts.struct_size = " + std::to_string(opts->struct_size) + " is not the size of a layout this library knows (" +
                                    std::to_string(sizeof(tfft_gbconv_opts)) + ")");
    if (opts->reserved_) return fail(TFFT_ERR_ARG, "tfft_gbconv_opts.reserved_ must be 0");
    o = *opts;
  }
  int rc = check_shape(rows, channels, length, taps, o.flags);
  if (rc == TFFT_OK) rc = check_stride(length, o.x_seq_stride, "x");
  if (rc == TFFT_OK) rc = check_stride(length, o.pre_seq_stride, "pre");
  if (rc == TFFT_OK) rc = check_stride(length, o.gy_seq_stride, "gy");
  if (rc == TFFT_OK) rc = check_stride(length, o.post_seq_stride, "post");
  if (rc == TFFT_OK) rc = check_stride(length, o.dx_seq_stride, "dx");
  if (rc == TFFT_OK) rc = check_stride(length, o.dpre_seq_stride, "dpre");
  if (rc == TFFT_OK && o.launch_iters > TFFT_LAUNCH_PERSISTENT) rc = fail(TFFT_ERR_ARG, "launch_iters must be 0 .. 65535");
  if (rc == TFFT_OK) rc = check_abi();
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  GBCONV_HIP(hipGetDevice(&prev));
  GBCONV_HIP(hipSetDevice(device_id));
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
  if (rc) {
    const std::string keep = g_err;
    tfft_gbconv_plan_destroy(p);
    g_err = keep;
    return rc;
  }
  *out = p;
  return TFFT_OK;
}

void tfft_gbconv_plan_destroy(tfft_gbconv_plan* p) {
  if (!p) return;
  if (p->d_tables) (void)hipFree(p->d_tables);
  if (p->d_filter) (void)hipFree(p->d_filter);
  if (p->d_spec) (void)hipFree(p->d_spec);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_gbconv_plan_set_taps(tfft_gbconv_plan* p, const void* taps, const void* skip, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!taps) return fail(TFFT_ERR_ARG, "null taps pointer");
  const int rc = check_current(p);
  if (rc) return rc;
  const size_t plane = static_cast<size_t>(p->channels) * kN;
  std::vector<uint16_t> h(static_cast<size_t>(p->channels) * p->taps), d(p->channels, 0), spec(2 * plane), img(2 * plane);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // through the host, as tfft_gsconv_plan_set_taps: everything enqueued on `stream` before the call is waited for; executions still
  // in flight keep reading the old spectrum until then, so the device is drained before it is replaced
  GBCONV_HIP(hipMemcpyAsync(h.data(), taps, h.size() * 2, hipMemcpyDeviceToHost, s));
  if (skip) GBCONV_HIP(hipMemcpyAsync(d.data(), skip, d.size() * 2, hipMemcpyDeviceToHost, s));
  GBCONV_HIP(hipStreamSynchronize(s));
  for (uint64_t c = 0; c < p->channels; ++c) {
    spectrum(h.data() + c * p->taps, p->taps, d[c], spec.data() + c * kN, spec.data() + plane + c * kN);
    for (uint32_t k = 0; k < kN; ++k) {
      const uint32_t slot = gbconv4096::filter_slot(k);
      const uint16_t im = spec[plane + c * kN + k];
      img[c * 8192 + slot] = spec[c * kN + k];
      // conj(H): the sign bit flipped, exact; a zero stays +0, so the image is as exactly Hermitian as H is
      img[c * 8192 + 4096 + slot] = (im & 0x7fff) ? (im ^ 0x8000) : 0;
    }
  }
  if (p->have_taps) GBCONV_HIP(hipDeviceSynchronize());
  GBCONV_HIP(hipMemcpy(p->d_spec, spec.data(), spec.size() * 2, hipMemcpyHostToDevice));
  GBCONV_HIP(hipMemcpy(p->d_filter, img.data(), img.size() * 2, hipMemcpyHostToDevice));
  p->have_taps = true;
  return TFFT_OK;
}

int tfft_gbconv_plan_spectrum(const tfft_gbconv_plan* p, void* h_re, void* h_im) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!h_re || !h_im) return fail(TFFT_ERR_ARG, "null spectrum pointer");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, "no taps: call tfft_gbconv_plan_set_taps first");
  const size_t plane = static_cast<size_t>(p->channels) * kN;
  GBCONV_HIP(hipMemcpy(h_re, p->d_spec, plane * 2, hipMemcpyDeviceToDevice));
  GBCONV_HIP(hipMemcpy(h_im, p->d_spec + plane, plane * 2, hipMemcpyDeviceToDevice));
  GBCONV_HIP(hipDeviceSynchronize());
  return TFFT_OK;
}

size_t tfft_gbconv_plan_workspace_bytes(const tfft_gbconv_plan* p) { return p ? p->ws_need : 0; }

int tfft_gbconv_plan_set_workspace(tfft_gbconv_plan* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (device_ptr && bytes < p->ws_need) return fail(TFFT_ERR_WORKSPACE, "workspace too small: " + std::to_string(p->ws_need) + " bytes needed");
  if (reinterpret_cast<uintptr_t>(device_ptr) & 255) return fail(TFFT_ERR_ARG, "the workspace must be 256-byte aligned");
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  p->ws = device_ptr;
  p->ws_owned = false;
  return TFFT_OK;
}

int tfft_gbconv_plan_prepare(tfft_gbconv_plan* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  int prev = 0;
  GBCONV_HIP(hipGetDevice(&prev));
  GBCONV_HIP(hipSetDevice(p->device));
  const int rc = ensure_workspace(p);
  (void)hipSetDevice(prev);
  return rc;
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
      if (i.ptr && (i.ptr == o.ptr || seqs_overlap(i.ptr, i.stride, o.ptr, o.stride, seqs, p->length)))
        return fail(TFFT_ERR_ARG, std::string(i.name) + " and " + o.name +
                                      " overlap (the input gradient cannot run in place: a segment reads what its successor overwrites)");
  }
  if (dpre && (dx == dpre || seqs_overlap(dx, p->dx_stride, dpre, p->dpre_stride, seqs, p->length))) return fail(TFFT_ERR_ARG, "dx and dpre overlap");
  const int rc = check_current(p);
  if (rc) return rc;
  uint32_t live, grid;
  dgrad_shape(p, live, grid);
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
  GBCONV_HIP(hipGetLastError());
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
  int rc = check_current(p);
  if (rc == TFFT_OK) rc = ensure_workspace(p);
  if (rc) return rc;
  for (const seq_set& i : inputs)
    if (i.ptr && block_overlaps(p->ws, p->ws_need, i.ptr, i.stride, seqs, p->length))
      return fail(TFFT_ERR_ARG, "the workspace overlaps x, pre, gy, post, the tap gradient or the skip gradient");
  if (blocks_overlap(p->ws, p->ws_need, dh, dh_bytes) || (dskip && blocks_overlap(p->ws, p->ws_need, dskip, dskip_bytes)))
    return fail(TFFT_ERR_ARG, "the workspace overlaps x, pre, gy, post, the tap gradient or the skip gradient");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t live, grid;
  wgrad_shape(p, live, grid);
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
  GBCONV_HIP(hipGetLastError());
  const uint64_t total = p->channels * p->taps;
  hipLaunchKernelGGL(gbconv4096::wreduce_kernel, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(p->ws),
                     static_cast<float*>(dh), static_cast<float*>(dskip), channels, static_cast<uint32_t>(p->taps),
                     static_cast<uint32_t>(p->partials), static_cast<uint32_t>(p->kpad));
  GBCONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_gbconv_plan_num_launches(const tfft_gbconv_plan* p) { return p ? 3 : 0; }

int tfft_gbconv_plan_kernels(const tfft_gbconv_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  const std::string inst = std::string("<") + tf_text(p->pre) + ", " + tf_text(p->post) + ">\n";
  const std::string out = "gbconv4096::dgrad_kernel" + inst + "gbconv4096::wgrad_kernel" + inst + "gbconv4096::wreduce_kernel\n";
  if (!buf || out.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small (" + std::to_string(out.size() + 1) + " bytes needed)");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return 3;
}

}  // extern "C"
