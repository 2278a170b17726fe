// tfft_conv.hip — host side and C ABI (include/tfft_conv.h) of the FFT convolution add-on, libtfft_conv.so.
//
// Layered on libtfft.so through include/tfft.h only (sub-plans of the composed path, tfft_device_check, tfft_abi_version); from
// csrc/ it takes k4096.hpp, header only, for the device helpers and the constant tables of the fused kernel (the add-on
// uploads a copy of its own). The error plumbing, the ABI check, the overlap test, filter_slot and the launch shape are those of
// host_math.hpp and host_plumbing.hpp beside this file, the two headers every convolution library includes.
#include "../../include/tfft_conv.h"
#include "cmul.hpp"
#include "conv4096.hpp"
#include "host_plumbing.hpp"

namespace {

int check_shape(uint64_t n, uint64_t batch, uint64_t filters, int flags) {
  if (!is_pow2(n)) return fail(TFFT_ERR_ARG, "n must be a power of two");
  if (n < kMinN || n > kMaxN) return fail(TFFT_ERR_ARG, "n must lie in 256 .. 2^26");
  if (flags & ~TFFT_CONV_COMPOSED) return fail(TFFT_ERR_ARG, "unknown flag bits (" + std::to_string(flags) + ")");
  if (batch == 0 || batch > 0xffffffffull) return fail(TFFT_ERR_ARG, "batch must be in [1, 2^32)");
  if (filters == 0 || filters > batch) return fail(TFFT_ERR_ARG, "filters must be in [1, batch]");
  return TFFT_OK;
}
int check_stride(uint64_t n, uint64_t stride, const char* which) {
  if (stride && (stride % 8 || stride < 2 * n))
    return fail(TFFT_ERR_ARG, std::string(which) + "_batch_stride must be 0 or a multiple of 8 that is >= 2 n");
  return TFFT_OK;
}

inline bool fused_shape(uint64_t n, int flags) { return n == 4096 && !(flags & TFFT_CONV_COMPOSED); }

// slot of bin k in a plane of the filter image (include/tfft_conv.h)
uint64_t filter_slot(uint64_t n, int flags, uint64_t k) {
  if (fused_shape(n, flags)) return host_math::filter_slot(static_cast<uint32_t>(k));
  const uint64_t n2 = tfft_plan_transposed_n2(n);
  if (!n2) return k;
  const uint64_t n1 = n / n2;
  return (k % n1) * n2 + k / n1;
}

// The transform chain tfft_plan_create gives a plan of this shape, in the words of tfft_plan_describe. tfft.h has no describe call
// for the transposed orders, so their two sub-plans (tfft.hip, create_transposed / create_transposed_in) are described one by one;
// tests/test_gpu_conv.py holds the text to tfft_conv_plan_kernels of a real plan, case by case.
int describe_chain(uint64_t n, uint64_t batch, bool inverse, std::string& out) {
  char a[256], b[256];
  const uint64_t n2 = tfft_plan_transposed_n2(n);
  if (!n2) {
    // (the planner bits a variant-0 plan of this batch gets: small batches take other splits)
    const int rc = pass_tfft(tfft_plan_describe(n, 1, tfft_plan_default_variant(n, 1, batch), a, sizeof(a)));
    out = a;
    return rc;
  }
  const uint64_t n1 = n / n2;
  int rc = pass_tfft(tfft_plan_describe(n1, n2, n1 == 512 ? TFFT_VARIANT_RADIX512_ONE_PASS : 0, a, sizeof(a)));
  if (rc == TFFT_OK) rc = pass_tfft(tfft_plan_describe(n2, 1, 0, b, sizeof(b)));
  if (rc) return rc;
  out = inverse ? std::string(b) + " " + a : std::string(a) + " " + b;      // transposed input: rows first, then the column pass
  return TFFT_OK;
}

}  // namespace

struct tfft_conv_plan {
  uint64_t n = 0, batch = 0, filters = 0, in_stride = 0, out_stride = 0;
  int device = 0, flags = 0, num_cus = 256;
  bool fused = false;
  void* d_tables = nullptr;          // fused: F / twiddle / G / H of k4096::build_tables
  uint16_t* d_filter = nullptr;      // [filters][RE n | IM n] in the plan's slot order
  bool have_filter = false;
  tfft_plan* fwd = nullptr;          // composed: natural in -> spectrum block (transposed order where the length has one)
  tfft_plan* inv = nullptr;          //           spectrum block -> natural out, run through tfft_exec_inverse
  size_t spec_bytes = 0, sub_bytes = 0;      // workspace = [spectra: batch x (RE n | IM n)] [scratch shared by the two sub-plans]
  mutable std::mutex ws_mutex;
  mutable void* ws = nullptr;
  mutable size_t ws_bytes = 0;
  mutable bool ws_owned = false;
};

namespace {

// hands the sub-plans their share of the workspace (they run one after the other on one stream and share it)
int bind_workspace(const tfft_conv_plan* p) {
  if (!p->sub_bytes) return TFFT_OK;
  void* sub = static_cast<uint8_t*>(p->ws) + p->spec_bytes;
  int rc = pass_tfft(tfft_plan_set_workspace(p->fwd, tfft_plan_workspace_bytes(p->fwd) ? sub : nullptr, p->sub_bytes));
  if (rc == TFFT_OK) rc = pass_tfft(tfft_plan_set_workspace(p->inv, tfft_plan_workspace_bytes(p->inv) ? sub : nullptr, p->sub_bytes));
  return rc;
}

int ensure_workspace(const tfft_conv_plan* p) {
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  const size_t need = p->spec_bytes + p->sub_bytes;
  if (!need || p->ws) return TFFT_OK;
  void* mem = nullptr;
  CONV_HIP(hipMalloc(&mem, need));
  p->ws = mem;
  p->ws_bytes = need;
  p->ws_owned = true;
  return bind_workspace(p);
}

int create_fused(tfft_conv_plan* p) {
  std::vector<uint8_t> blob;
  k4096::build_tables(blob);
  CONV_HIP(hipMalloc(&p->d_tables, k4096::kOffF1n));
  CONV_HIP(hipMemcpy(p->d_tables, blob.data(), k4096::kOffF1n, hipMemcpyHostToDevice));
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(conv4096::conv4096_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, k4096::kLdsBytes));
  return TFFT_OK;
}

int create_composed(tfft_conv_plan* p) {
  const bool transposed = tfft_plan_transposed_n2(p->n) != 0;
  tfft_plan_opts fo = TFFT_PLAN_OPTS_INIT;
  fo.in_batch_stride = p->in_stride;
  fo.out_batch_stride = 2 * p->n;
  fo.preserve_input = 1;
  fo.output_order = transposed ? TFFT_ORDER_TRANSPOSED : TFFT_ORDER_NATURAL;
  tfft_plan_opts io = TFFT_PLAN_OPTS_INIT;
  io.in_batch_stride = 2 * p->n;
  io.out_batch_stride = p->out_stride;
  io.input_order = transposed ? TFFT_ORDER_TRANSPOSED : TFFT_ORDER_NATURAL;
  int rc = pass_tfft(tfft_plan_create(p->n, p->batch, p->device, &fo, &p->fwd));
  if (rc == TFFT_OK) rc = pass_tfft(tfft_plan_create(p->n, p->batch, p->device, &io, &p->inv));
  if (rc) return rc;
  p->spec_bytes = round256(static_cast<size_t>(p->batch) * p->n * 4);
  p->sub_bytes = round256(std::max(tfft_plan_workspace_bytes(p->fwd), tfft_plan_workspace_bytes(p->inv)));
  return TFFT_OK;
}

}  // namespace

extern "C" {

const char* tfft_conv_last_error(void) { return g_err.c_str(); }

uint64_t tfft_conv_filter_slot(uint64_t n, int flags, uint64_t k) {
  if (!is_pow2(n) || n < kMinN || n > kMaxN || (flags & ~TFFT_CONV_COMPOSED) || k >= n) return UINT64_MAX;
  return filter_slot(n, flags, k);
}

int tfft_conv_describe(uint64_t n, uint64_t batch, uint64_t filters, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  int rc = check_shape(n, batch, filters, flags);
  if (rc) return rc;
  std::string out;
  if (fused_shape(n, flags)) {
    out = "conv4096:4096";
  } else {
    std::string f, i;
    rc = describe_chain(n, batch, false, f);
    if (rc == TFFT_OK) rc = describe_chain(n, batch, true, i);
    if (rc) return rc;
    out = f + " | cmul | " + i;
  }
  return copy_text(out, buf, bytes);
}

int tfft_conv_plan_create(uint64_t n, uint64_t batch, uint64_t filters, int device_id, uint64_t in_batch_stride,
                          uint64_t out_batch_stride, int flags, tfft_conv_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  int rc = check_shape(n, batch, filters, flags);
  if (rc == TFFT_OK) rc = check_stride(n, in_batch_stride, "in");
  if (rc == TFFT_OK) rc = check_stride(n, out_batch_stride, "out");
  if (rc == TFFT_OK) rc = check_abi("libtfft_conv.so");
  if (rc == TFFT_OK) rc = pass_tfft(tfft_device_check(device_id));
  if (rc) return rc;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(device_id));
  tfft_conv_plan* p = new tfft_conv_plan;
  p->n = n;
  p->batch = batch;
  p->filters = filters;
  p->in_stride = in_batch_stride ? in_batch_stride : 2 * n;
  p->out_stride = out_batch_stride ? out_batch_stride : 2 * n;
  p->device = device_id;
  p->flags = flags;
  p->fused = fused_shape(n, flags);
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) p->num_cus = prop.multiProcessorCount;
  rc = p->fused ? create_fused(p) : create_composed(p);
  if (rc == TFFT_OK) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_filter), static_cast<size_t>(filters) * n * 4);
    if (e != hipSuccess) rc = hip_fail(e, "hipMalloc(filter image)");
  }
  (void)hipSetDevice(prev);
  if (rc) return fail_create(p, rc, tfft_conv_plan_destroy);
  *out = p;
  return TFFT_OK;
}

void tfft_conv_plan_destroy(tfft_conv_plan* p) {
  if (!p) return;
  tfft_plan_destroy(p->fwd);
  tfft_plan_destroy(p->inv);
  if (p->d_tables) (void)hipFree(p->d_tables);
  if (p->d_filter) (void)hipFree(p->d_filter);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_conv_plan_set_filter(tfft_conv_plan* p, const void* h_re, const void* h_im, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!h_re || !h_im) return fail(TFFT_ERR_ARG, "null filter pointer");
  const int cur_rc = check_current(p->device);
  if (cur_rc) return cur_rc;
  const size_t plane = static_cast<size_t>(p->filters) * p->n;
  std::vector<uint16_t> re(plane), im(plane), img(2 * plane);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // through the host: the permutation runs once per filter, not per execution. Everything enqueued on `stream` before the call
  // (the kernel that produced the filter) is waited for; executions still in flight keep reading the old image until then, so the
  // device is drained before the image is replaced.
  CONV_HIP(hipMemcpyAsync(re.data(), h_re, plane * 2, hipMemcpyDeviceToHost, s));
  CONV_HIP(hipMemcpyAsync(im.data(), h_im, plane * 2, hipMemcpyDeviceToHost, s));
  CONV_HIP(hipStreamSynchronize(s));
  for (uint64_t f = 0; f < p->filters; ++f)
    for (uint64_t k = 0; k < p->n; ++k) {
      const uint64_t slot = filter_slot(p->n, p->flags, k);
      img[f * 2 * p->n + slot] = re[f * p->n + k];
      img[f * 2 * p->n + p->n + slot] = im[f * p->n + k];
    }
  if (p->have_filter) CONV_HIP(hipDeviceSynchronize());
  CONV_HIP(hipMemcpy(p->d_filter, img.data(), img.size() * 2, hipMemcpyHostToDevice));
  p->have_filter = true;
  return TFFT_OK;
}

size_t tfft_conv_plan_workspace_bytes(const tfft_conv_plan* p) { return p ? p->spec_bytes + p->sub_bytes : 0; }

int tfft_conv_plan_set_workspace(tfft_conv_plan* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  const size_t need = p->spec_bytes + p->sub_bytes;
  if (device_ptr && bytes < need) return fail(TFFT_ERR_WORKSPACE, "workspace too small: " + std::to_string(need) + " bytes needed");
  if (reinterpret_cast<uintptr_t>(device_ptr) & 255) return fail(TFFT_ERR_ARG, "the workspace must be 256-byte aligned");
  std::lock_guard<std::mutex> lock(p->ws_mutex);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  p->ws = need ? device_ptr : nullptr;
  p->ws_bytes = p->ws ? bytes : 0;
  p->ws_owned = false;
  return p->ws ? bind_workspace(p) : TFFT_OK;
}

int tfft_conv_plan_prepare(tfft_conv_plan* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (p->fused) return TFFT_OK;
  int prev = 0;
  CONV_HIP(hipGetDevice(&prev));
  CONV_HIP(hipSetDevice(p->device));
  int rc = ensure_workspace(p);
  if (rc == TFFT_OK) rc = pass_tfft(tfft_plan_prepare(p->fwd));
  if (rc == TFFT_OK) rc = pass_tfft(tfft_plan_prepare(p->inv));
  (void)hipSetDevice(prev);
  return rc;
}

int tfft_conv_exec(const tfft_conv_plan* p, const void* in_re, const void* in_im, void* out_re, void* out_im, void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->have_filter) return fail(TFFT_ERR_ARG, "no filter: call tfft_conv_plan_set_filter first");
  if (!in_re || !in_im || !out_re || !out_im) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(in_re) | reinterpret_cast<uintptr_t>(in_im) | reinterpret_cast<uintptr_t>(out_re) |
       reinterpret_cast<uintptr_t>(out_im)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  const bool same_re = in_re == out_re, same_im = in_im == out_im;
  if ((same_re || same_im) && p->in_stride != p->out_stride)
    return fail(TFFT_ERR_ARG, "in-place execution needs equal input and output batch strides");
  if ((!same_re && seqs_overlap(in_re, p->in_stride, p->n, out_re, p->out_stride, p->n, p->batch)) ||
      (!same_im && seqs_overlap(in_im, p->in_stride, p->n, out_im, p->out_stride, p->n, p->batch)) ||
      seqs_overlap(in_re, p->in_stride, p->n, out_im, p->out_stride, p->n, p->batch) ||
      seqs_overlap(in_im, p->in_stride, p->n, out_re, p->out_stride, p->n, p->batch) ||
      seqs_overlap(out_re, p->out_stride, p->n, out_im, p->out_stride, p->n, p->batch))
    return fail(TFFT_ERR_ARG, "input and output planes overlap without being identical (only exact in-place or disjoint planes are supported)");
  const int cur_rc = check_current(p->device);
  if (cur_rc) return cur_rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (p->fused) {
    uint32_t live, grid;
    conv_shape(p->batch, p->num_cus, 0, live, grid);      // no launch_iters in this ABI: the default shape
    hipLaunchKernelGGL(conv4096::conv4096_kernel, dim3(grid), dim3(k4096::kThreads), k4096::kLdsBytes, s, static_cast<const uint16_t*>(in_re),
                       static_cast<const uint16_t*>(in_im), static_cast<uint16_t*>(out_re), static_cast<uint16_t*>(out_im), p->in_stride,
                       p->out_stride, static_cast<uint32_t>(p->batch), live, static_cast<uint32_t>(p->filters),
                       static_cast<const uint8_t*>(p->d_tables), p->d_filter);
    CONV_HIP(hipGetLastError());
    return TFFT_OK;
  }
  int rc = ensure_workspace(p);
  if (rc) return rc;
  uint16_t* const spec = static_cast<uint16_t*>(p->ws);
  rc = pass_tfft(tfft_exec(p->fwd, in_re, in_im, spec, spec + p->n, s));
  if (rc) return rc;
  const uint64_t total = p->batch * (p->n / 8);
  const uint32_t grid = static_cast<uint32_t>(std::min<uint64_t>((total + cmul::kThreads - 1) / cmul::kThreads, static_cast<uint64_t>(p->num_cus) * 32));
  hipLaunchKernelGGL(cmul::cmul_kernel, dim3(grid), dim3(cmul::kThreads), 0, s, spec, p->d_filter, static_cast<uint32_t>(ilog2(p->n / 8)), total,
                     static_cast<uint32_t>(p->filters), static_cast<float>(p->n));
  CONV_HIP(hipGetLastError());
  return pass_tfft(tfft_exec_inverse(p->inv, spec, spec + p->n, out_re, out_im, s));
}

int tfft_conv_plan_num_launches(const tfft_conv_plan* p) {
  if (!p) return 0;
  return p->fused ? 1 : tfft_plan_num_launches(p->fwd) + 1 + tfft_plan_num_launches(p->inv);
}

int tfft_conv_plan_kernels(const tfft_conv_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  std::string out;
  int lines = 1;
  if (p->fused) {
    out = "conv4096::conv4096_kernel\n";
  } else {
    std::vector<char> tmp(1 << 16);
    const int a = tfft_plan_kernels(p->fwd, tmp.data(), tmp.size());
    if (a < 0) return pass_tfft(a);
    out = tmp.data();
    out += "cmul::cmul_kernel\n";
    const int b = tfft_plan_kernels(p->inv, tmp.data(), tmp.size());
    if (b < 0) return pass_tfft(b);
    out += tmp.data();
    lines = a + 1 + b;
  }
  return kernel_names(out, lines, buf, bytes);
}

}  // extern "C"
