// tfft_cconv.hip — host side and C ABI (include/tfft_cconv.h) of the carried convolution add-on, libtfft_cconv.so: the forward
// plan of tfft_sconv.hip and the gradient plan of tfft_bconv.hip with a history in front of x and a future behind g.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version); from csrc/ it takes k4096.hpp, header only. It links neither libtfft_sconv.so nor libtfft_bconv.so: the
// geometry, the checks, the launch shapes and the fp64 spectrum builder of those two files are restated below, and
// tests/test_cconv_host.py and tests/test_gpu_cconv.py hold them to the shipped code (the geometry and the refusals on the host;
// without a context every result to the shipped plans' bit for bit).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/tfft_cconv.h"
#include "cconv4096.hpp"

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
#define CCONV_HIP(call)                               \
  do {                                                \
    const hipError_t e_ = (call);                     \
    if (e_ != hipSuccess) return hip_fail(e_, #call); \
  } while (0)

constexpr uint64_t kN = 4096, kMaxLength = uint64_t{1} << 26;      // the transform length; the longest sequence of tfft_sconv.h
constexpr uint64_t kWaves = 2048;                                  // 256 CUs x 8 waves: the work units the default P aims at

int check_abi() {
  static const int version = tfft_abi_version();
  if (version != TFFT_ABI_VERSION)
    return fail(TFFT_ERR_ARG, "libtfft.so speaks ABI " + std::to_string(version) + ", libtfft_cconv.so was built against ABI " +
                                  std::to_string(TFFT_ABI_VERSION) + ": rebuild the add-on");
  return TFFT_OK;
}

// the geometry of tfft_sconv_geometry, fixed by the number of taps alone; the context does not change it
inline uint64_t halo_of(uint64_t taps) { return (taps - 1 + 63) / 64 * 64; }
inline uint64_t hop_of(uint64_t taps) { return kN - halo_of(taps); }
inline uint64_t segments_of(uint64_t length, uint64_t taps) { return (length + hop_of(taps) - 1) / hop_of(taps); }
inline uint64_t carry_min_of(uint64_t taps) { return (taps - 1 + 7) / 8 * 8; }
// partial sums per channel of the tap gradient: tfft_bconv_geometry's
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
  if (taps > TFFT_CCONV_MAX_TAPS)
    return fail(TFFT_ERR_ARG, "taps must not exceed 2049 (the halo of a 4096-sample window): longer filters run through tfft_lconv_plan_create");
  return TFFT_OK;
}

int check_shape(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int flags, const char* opts_name) {
  const int rc = check_length_taps(length, taps);
  if (rc) return rc;
  if (flags) return fail(TFFT_ERR_ARG, "unknown flag bits (" + std::to_string(flags) + "): " + opts_name + ".flags must be 0");
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
// a context of `n` samples per sequence, `stride` halves apart: `which` = "history" / "future", `short_name` = "hist" / "fut"
int check_context(uint64_t taps, uint64_t n, uint64_t stride, const char* which, const char* short_name) {
  if (n % 8) return fail(TFFT_ERR_ARG, std::string(which) + " must be a multiple of 8");
  if (n > halo_of(taps))
    return fail(TFFT_ERR_ARG, std::string(which) + " must not exceed the halo (" + std::to_string(halo_of(taps)) + " samples for " +
                                  std::to_string(taps) + " taps): no window reaches further");
  if (stride && (stride % 8 || stride < n))
    return fail(TFFT_ERR_ARG, std::string(short_name) + "_seq_stride must be 0 or a multiple of 8 that is >= " + which);
  return TFFT_OK;
}

// Element-exact test whether two sets of sequences share a half: `count` blocks of la halves, sa halves apart, at pa, against
// `count` blocks of lb halves, sb apart, at pb. seqs_overlap of tfft_sconv.hip with a length per side, since a context has its own.
bool seqs_overlap(const void* pa, uint64_t sa, uint64_t la, const void* pb, uint64_t sb, uint64_t lb, uint64_t count) {
  if (la == 0 || lb == 0) return false;
  const uintptr_t a = reinterpret_cast<uintptr_t>(pa), b = reinterpret_cast<uintptr_t>(pb);
  const uintptr_t a_end = a + 2 * ((count - 1) * sa + la), b_end = b + 2 * ((count - 1) * sb + lb);
  if (a_end <= b || b_end <= a) return false;
  if (count == 1 || sa != sb) return true;            // different strides: conservative
  // one period: a block of la halves starting d halves behind the start of a block of lb halves, both repeating every sa
  const uint64_t d = a >= b ? static_cast<uint64_t>(a - b) / 2 % sa : (sa - static_cast<uint64_t>(b - a) / 2 % sa) % sa;
  return d < lb || d + la > sa;
}
// a block of `bytes` against the whole extent of a set of sequences, gaps included (conservative)
bool block_overlaps(const void* block, uint64_t bytes, const void* seqs, uint64_t stride, uint64_t count, uint64_t len) {
  if (!seqs || len == 0) return false;
  const uintptr_t a = reinterpret_cast<uintptr_t>(block), b = reinterpret_cast<uintptr_t>(seqs);
  return a < b + 2 * ((count - 1) * stride + len) && b < a + bytes;
}

// ---- binary16 on the host, bit by bit (round to nearest even, one rounding from fp64): tfft_lconv.hip's
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

// one filter: H = FFT of the zero-padded taps, each component rounded once; exactly Hermitian, Im of bins 0 and n / 2 exactly 0
void spectrum(const uint16_t* taps, uint64_t num_taps, uint16_t* out_re, uint16_t* out_im) {
  const uint64_t n = kN;
  std::vector<std::complex<double>> a(n);
  for (uint64_t j = 0; j < num_taps; ++j) a[j] = from_half(taps[j]);
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

// what the two plan types share: the shape, the geometry and the device memory of tfft_sconv_plan
struct plan_base {
  uint64_t rows = 0, channels = 0, length = 0, taps = 0, halo = 0, hop = 0, segments = 0, items = 0;
  uint32_t launch_iters = 0;
  int device = 0, num_cus = 256;
  void* d_tables = nullptr;          // F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // [channels][RE 4096 | IM 4096] in conv4096::filter_slot order: H (forward), conj(H) (gradient)
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

int create_base(plan_base* p) {
  std::vector<uint8_t> blob;
  k4096::build_tables(blob);
  CCONV_HIP(hipMalloc(&p->d_tables, k4096::kOffF1n));
  CCONV_HIP(hipMemcpy(p->d_tables, blob.data(), k4096::kOffF1n, hipMemcpyHostToDevice));
  CCONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_filter), static_cast<size_t>(p->channels) * 8192 * 2));
  CCONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_spec), static_cast<size_t>(p->channels) * kN * 4));
  return TFFT_OK;
}

void destroy_base(plan_base* p) {
  if (p->d_tables) (void)hipFree(p->d_tables);
  if (p->d_filter) (void)hipFree(p->d_filter);
  if (p->d_spec) (void)hipFree(p->d_spec);
}

int check_current(const plan_base* p) {
  int cur = 0;
  CCONV_HIP(hipGetDevice(&cur));
  if (cur != p->device) return fail(TFFT_ERR_ARG, "plan was created for another device than the current one");
  return TFFT_OK;
}

// tfft_sconv_plan_set_taps (conjugate = false) and tfft_bconv_plan_set_taps (true: the filter image holds conj(H))
int set_taps(plan_base* p, const void* taps, void* stream, bool conjugate) {
  if (!taps) return fail(TFFT_ERR_ARG, "null taps pointer");
  const int rc = check_current(p);
  if (rc) return rc;
  const size_t plane = static_cast<size_t>(p->channels) * kN;
  std::vector<uint16_t> h(static_cast<size_t>(p->channels) * p->taps), spec(2 * plane), img(2 * plane);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // through the host, as tfft_sconv_plan_set_taps: everything enqueued on `stream` before the call is waited for; executions still
  // in flight keep reading the old spectrum until then, so the device is drained before it is replaced
  CCONV_HIP(hipMemcpyAsync(h.data(), taps, h.size() * 2, hipMemcpyDeviceToHost, s));
  CCONV_HIP(hipStreamSynchronize(s));
  for (uint64_t c = 0; c < p->channels; ++c) {
    spectrum(h.data() + c * p->taps, p->taps, spec.data() + c * kN, spec.data() + plane + c * kN);
    for (uint32_t k = 0; k < kN; ++k) {
      const uint32_t slot = cconv4096::filter_slot(k);
      const uint16_t im = spec[plane + c * kN + k];
      img[c * 8192 + slot] = spec[c * kN + k];
      // conj(H): the sign bit flipped, exact; a zero stays +0, so the image is as exactly Hermitian as H is
      img[c * 8192 + 4096 + slot] = !conjugate ? im : (im & 0x7fff) ? (im ^ 0x8000) : 0;
    }
  }
  if (p->have_taps) CCONV_HIP(hipDeviceSynchronize());
  CCONV_HIP(hipMemcpy(p->d_spec, spec.data(), spec.size() * 2, hipMemcpyHostToDevice));
  CCONV_HIP(hipMemcpy(p->d_filter, img.data(), img.size() * 2, hipMemcpyHostToDevice));
  p->have_taps = true;
  return TFFT_OK;
}

int copy_spectrum(const plan_base* p, void* h_re, void* h_im, const char* set_taps_name) {
  if (!h_re || !h_im) return fail(TFFT_ERR_ARG, "null spectrum pointer");
  if (!p->have_taps) return fail(TFFT_ERR_ARG, std::string("no taps: call ") + set_taps_name + " first");
  const size_t plane = static_cast<size_t>(p->channels) * kN;
  CCONV_HIP(hipMemcpy(h_re, p->d_spec, plane * 2, hipMemcpyDeviceToDevice));
  CCONV_HIP(hipMemcpy(h_im, p->d_spec + plane, plane * 2, hipMemcpyDeviceToDevice));
  CCONV_HIP(hipDeviceSynchronize());
  return TFFT_OK;
}

// launch shape of the forward pass and the input gradient: sconv4096_kernel's (tfft_sconv.hip, sconv4096_shape)
void conv_shape(const plan_base* p, uint32_t& live, uint32_t& grid) {
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

cconv4096::geometry geometry_of(const plan_base* p) {
  return {static_cast<int32_t>(p->length / 8), static_cast<int32_t>(p->halo / 8), static_cast<int32_t>(p->hop / 8), static_cast<int32_t>(p->segments)};
}

int copy_text(const std::string& out, char* buf, size_t bytes) {
  if (out.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return TFFT_OK;
}

int kernel_names(const std::string& out, int lines, char* buf, size_t bytes) {
  if (!buf || out.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small (" + std::to_string(out.size() + 1) + " bytes needed)");
  std::memcpy(buf, out.c_str(), out.size() + 1);
  return lines;
}

template <class Plan>
int fail_create(Plan* p, int rc, void (*destroy)(Plan*)) {
  const std::string keep = g_err;
  destroy(p);
  g_err = keep;
  return rc;
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

namespace {

// launch shape of the tap gradient: tfft_bconv.hip's wgrad_shape
void wgrad_shape(const tfft_cconv_grad* p, uint32_t& live, uint32_t& grid) {
  const uint64_t cus = static_cast<uint64_t>(p->num_cus), units = p->channels * p->partials;
  live = cconv4096::kWgradWaves;
  for (uint32_t l = 1; l < live; l *= 2)
    if (units <= cus * l) {
      live = l;
      break;
    }
  grid = static_cast<uint32_t>((units + live - 1) / live);
}

// the rule of tfft_conv.h: the workspace is settled once, by the caller, by prepare or by the first execution
int ensure_workspace(const tfft_cconv_grad* p) {
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  if (p->ws) return TFFT_OK;
  void* mem = nullptr;
  CCONV_HIP(hipMalloc(&mem, p->ws_need));
  p->ws = mem;
  p->ws_owned = true;
  return TFFT_OK;
}

}  // namespace

extern "C" {

const char* tfft_cconv_last_error(void) { return g_err.c_str(); }

// ---- the forward plan

int tfft_cconv_geometry(uint64_t length, uint64_t taps, uint64_t* halo, uint64_t* hop, uint64_t* segments, uint64_t* carry_min) {
  g_err.clear();
  const int rc = check_length_taps(length, taps);
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
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_cconv_opts");
  if (rc) return rc;
  return copy_text("cconv4096:4096 x " + std::to_string(segments_of(length, taps)), buf, bytes);
}

int tfft_cconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id, const tfft_cconv_opts* opts,
                           tfft_cconv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_cconv_opts o = TFFT_CCONV_OPTS_INIT;
  if (opts) {
    if (opts->struct_size != sizeof(tfft_cconv_opts))
      return fail(TFFT_ERR_ARG, "tfft_cconv_opts.struct_size = " + std::to_string(opts->struct_size) + " is not the size of a layout this library knows (" +
                                    std::to_string(sizeof(tfft_cconv_opts)) + ")");
    if (opts->reserved_) return fail(TFFT_ERR_ARG, "tfft_cconv_opts.reserved_ must be 0");
    o = *opts;
  }
  int rc = check_shape(rows, channels, length, taps, o.flags, "tfft_cconv_opts");
  if (rc == TFFT_OK) rc = check_stride(length, o.in_seq_stride, "in");
  if (rc == TFFT_OK) rc = check_stride(length, o.out_seq_stride, "out");
  if (rc == TFFT_OK) rc = check_context(taps, o.history, o.hist_seq_stride, "history", "hist");
  if (rc == TFFT_OK && o.launch_iters > TFFT_LAUNCH_PERSISTENT) rc = fail(TFFT_ERR_ARG, "launch_iters must be 0 .. 65535");
  if (rc == TFFT_OK) rc = check_abi();
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CCONV_HIP(hipGetDevice(&prev));
  CCONV_HIP(hipSetDevice(device_id));
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
  return set_taps(p, taps, stream, false);
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
  const int rc = check_current(p);
  if (rc) return rc;
  uint32_t live, grid;
  conv_shape(p, live, grid);
  // without a history the kernel gets 0 chunks of it and never forms an address from the second base
  hipLaunchKernelGGL(cconv4096::cconv4096_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(in), static_cast<const uint16_t*>(hist ? hist : in), static_cast<uint16_t*>(out), p->in_stride,
                     hist ? p->hist_stride : p->in_stride, p->out_stride, static_cast<uint32_t>(p->rows), static_cast<uint32_t>(p->channels),
                     geometry_of(p), static_cast<int32_t>(hist ? p->history / 8 : 0), static_cast<uint32_t>(p->items), live,
                     static_cast<const uint8_t*>(p->d_tables), p->d_filter);
  CCONV_HIP(hipGetLastError());
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
  const int rc = check_shape(rows, channels, length, taps, 0, "tfft_cconv_grad_opts");
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
  const int rc = check_shape(rows, channels, length, taps, flags, "tfft_cconv_grad_opts");
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
  if (opts) {
    if (opts->struct_size != sizeof(tfft_cconv_grad_opts))
      return fail(TFFT_ERR_ARG, "tfft_cconv_grad_opts.struct_size = " + std::to_string(opts->struct_size) +
                                    " is not the size of a layout this library knows (" + std::to_string(sizeof(tfft_cconv_grad_opts)) + ")");
    if (opts->reserved_) return fail(TFFT_ERR_ARG, "tfft_cconv_grad_opts.reserved_ must be 0");
    o = *opts;
  }
  int rc = check_shape(rows, channels, length, taps, o.flags, "tfft_cconv_grad_opts");
  if (rc == TFFT_OK) rc = check_stride(length, o.x_seq_stride, "x");
  if (rc == TFFT_OK) rc = check_stride(length, o.g_seq_stride, "g");
  if (rc == TFFT_OK) rc = check_stride(length, o.dx_seq_stride, "dx");
  if (rc == TFFT_OK) rc = check_context(taps, o.history, o.hist_seq_stride, "history", "hist");
  if (rc == TFFT_OK) rc = check_context(taps, o.future, o.fut_seq_stride, "future", "fut");
  if (rc == TFFT_OK && o.launch_iters > TFFT_LAUNCH_PERSISTENT) rc = fail(TFFT_ERR_ARG, "launch_iters must be 0 .. 65535");
  if (rc == TFFT_OK) rc = check_abi();
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CCONV_HIP(hipGetDevice(&prev));
  CCONV_HIP(hipSetDevice(device_id));
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
  return set_taps(p, taps, stream, true);
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
  if (device_ptr && bytes < p->ws_need) return fail(TFFT_ERR_WORKSPACE, "workspace too small: " + std::to_string(p->ws_need) + " bytes needed");
  if (reinterpret_cast<uintptr_t>(device_ptr) & 255) return fail(TFFT_ERR_ARG, "the workspace must be 256-byte aligned");
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  p->ws = device_ptr;
  p->ws_owned = false;
  return TFFT_OK;
}

int tfft_cconv_grad_prepare(tfft_cconv_grad* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  int prev = 0;
  CCONV_HIP(hipGetDevice(&prev));
  CCONV_HIP(hipSetDevice(p->device));
  const int rc = ensure_workspace(p);
  (void)hipSetDevice(prev);
  return rc;
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
  const int rc = check_current(p);
  if (rc) return rc;
  uint32_t live, grid;
  conv_shape(p, live, grid);
  hipLaunchKernelGGL(cconv4096::dgrad_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, static_cast<hipStream_t>(stream),
                     static_cast<const uint16_t*>(g), static_cast<const uint16_t*>(fut ? fut : g), static_cast<uint16_t*>(dx), p->g_stride,
                     fut ? p->fut_stride : p->g_stride, p->dx_stride, static_cast<uint32_t>(p->rows), static_cast<uint32_t>(p->channels),
                     geometry_of(p), static_cast<int32_t>(fut ? p->future / 8 : 0), static_cast<uint32_t>(p->items), live,
                     static_cast<const uint8_t*>(p->d_tables), p->d_filter);
  CCONV_HIP(hipGetLastError());
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
  int rc = check_current(p);
  if (rc == TFFT_OK) rc = ensure_workspace(p);
  if (rc) return rc;
  if (block_overlaps(p->ws, p->ws_need, x, p->x_stride, seqs, p->length) || block_overlaps(p->ws, p->ws_need, g, p->g_stride, seqs, p->length) ||
      block_overlaps(p->ws, p->ws_need, hist, p->hist_stride, seqs, p->history) ||
      (reinterpret_cast<uintptr_t>(dh) < reinterpret_cast<uintptr_t>(p->ws) + p->ws_need &&
       reinterpret_cast<uintptr_t>(p->ws) < reinterpret_cast<uintptr_t>(dh) + dh_bytes))
    return fail(TFFT_ERR_ARG, "the workspace overlaps x, x_hist, g or the tap gradient");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint32_t live, grid;
  wgrad_shape(p, live, grid);
  hipLaunchKernelGGL(cconv4096::wgrad_kernel, dim3(grid), dim3(cconv4096::kWgradThreads), cconv4096::kWgradLdsBytes, s, static_cast<const uint16_t*>(x),
                     static_cast<const uint16_t*>(hist ? hist : x), static_cast<const uint16_t*>(g), p->x_stride, hist ? p->hist_stride : p->x_stride,
                     p->g_stride, static_cast<uint32_t>(p->rows), static_cast<uint32_t>(p->channels), geometry_of(p),
                     static_cast<int32_t>(hist ? p->history / 8 : 0), static_cast<uint32_t>(p->partials), static_cast<uint32_t>(p->per_channel),
                     static_cast<uint32_t>(p->channels * p->partials), live, static_cast<int32_t>(p->kpad / 8), static_cast<uint32_t>(p->kpad),
                     static_cast<const uint8_t*>(p->d_tables), static_cast<float*>(p->ws));
  CCONV_HIP(hipGetLastError());
  const uint64_t total = p->channels * p->taps;
  hipLaunchKernelGGL(cconv4096::wreduce_kernel, dim3(static_cast<uint32_t>((total + 255) / 256)), dim3(256), 0, s, static_cast<const float*>(p->ws),
                     static_cast<float*>(dh), static_cast<uint32_t>(p->channels), static_cast<uint32_t>(p->taps), static_cast<uint32_t>(p->partials),
                     static_cast<uint32_t>(p->kpad));
  CCONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_cconv_grad_num_launches(const tfft_cconv_grad* p) { return p ? 3 : 0; }

int tfft_cconv_grad_kernels(const tfft_cconv_grad* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("cconv4096::dgrad_kernel\ncconv4096::wgrad_kernel\ncconv4096::wreduce_kernel\n", 3, buf, bytes);
}

}  // extern "C"
