// tfft_mistftn.hip — host side and C ABI (include/tfft_mistftn.h) of the masked short-frame inverse STFT add-on,
// libtfft_mistftn.so: the plans of include/tfft_istftn.h with a real binary16 mask inside the merge.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only (status codes, tfft_device_check,
// tfft_abi_version), never on a sibling: the overlap-add is istftn/olan.hpp, a header, included as it is. From csrc/ it takes
// k4096.hpp and rsplit.hpp, header only, for the device helpers, and k256r.hpp, in the host pass, for the constant tables of the
// frames kernel. Every refusal tfft_istftn.h shares, the plan-create sequence, the window, the checks of an execution and the grid
// of the overlap-add come from conv/stft_host.hpp, the workspace rules from conv/host_plumbing.hpp; here are the plan struct,
// check_n, the refusals of the mask (its stride, per-bin mode, its extent, its alignment and what it must not meet), the frames
// kernels' LDS opt-in, the two launches and the two texts. tests/test_gpu_mistftn.py holds the frames to tfft_exec_inverse on the
// numpy masked merge and the output to the numpy overlap-add, bit for bit.
#include "../../include/tfft_mistftn.h"
#include "mistft256r.hpp"
#include "../istftn/olan.hpp"
#define STFT_HOST_256R mistft256r
#include "../conv/stft_host.hpp"

struct tfft_mistftn_plan {
  uint64_t n = 0, rows = 0, length = 0, hop = 0, pad = 0, frames = 0, total = 0, batch = 0, groups = 0, in_stride = 0, out_stride = 0;
  uint64_t mask_stride = 0;          // halves between the masks of consecutive frames as the kernel takes it: 0 in per-bin mode
  uint64_t mask_halves = 0;          // the mask's extent: (R F - 1) * mask_stride + n / 2 + 1
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

// slot_of is a permutation of the chunks of a plane and its own inverse
template <int R>
constexpr bool slots_pair_up() {
  for (uint32_t j = 0; j < 32u * R; ++j)
    if (mistft256r::slot_of(R, j) >= 32u * R || mistft256r::slot_of(R, mistft256r::slot_of(R, j)) != j) return false;
  return true;
}
static_assert(slots_pair_up<2>() && slots_pair_up<4>() && slots_pair_up<8>(), "mistft256r.hpp: slot_of is no involution");

int check_n(uint32_t n) {
  if (n == 4096) return fail(TFFT_ERR_ARG, "n = 4096 is the plan of include/tfft_istft.h, which takes no mask: use tfft_istft_plan_create");
  if (n != 512 && n != 1024 && n != 2048) return fail(TFFT_ERR_ARG, "n must be 512, 1024 or 2048 (" + std::to_string(n) + ")");
  return TFFT_OK;
}
constexpr stft_rules kRules = {"mistftn", true, TFFT_MISTFTN_RAW_SUM | TFFT_MISTFTN_MASK_PER_BIN,
                               "must be 0 or a combination of TFFT_MISTFTN_RAW_SUM and TFFT_MISTFTN_MASK_PER_BIN", check_n};

// what is wrong with the mask's options, for a shape that check_shape has passed
int check_mask(uint64_t n, uint64_t total, const tfft_mistftn_opts& o) {
  const uint64_t bins = bins_of(n);
  if (o.flags & TFFT_MISTFTN_MASK_PER_BIN) {
    if (o.mask_frame_stride) return fail(TFFT_ERR_ARG, "mask_frame_stride must be 0 with TFFT_MISTFTN_MASK_PER_BIN: one mask serves every frame");
    return TFFT_OK;
  }
  if (o.mask_frame_stride && (o.mask_frame_stride % 8 || o.mask_frame_stride < bins))
    return fail(TFFT_ERR_ARG, "mask_frame_stride must be 0 or a multiple of 8 that is >= " + std::to_string(bins));
  if (!extent_fits(total, o.mask_frame_stride ? o.mask_frame_stride : pitch_of(n), bins))
    return fail(TFFT_ERR_ARG, "the mask extent (rows * frames - 1) * mask_frame_stride + " + std::to_string(bins) + " must be below 2^62 halves");
  return TFFT_OK;
}

template <int R>
int create_device(tfft_mistftn_plan* p) {
  std::vector<uint8_t> blob;
  k256r_host::build_tables(R, blob);
  const int rc = create_device_base(p, blob, blob.size());
  if (rc) return rc;
  // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
  CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(mistft256r::frames_kernel<R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               mistft256r::lds_bytes<R>()));
  return TFFT_OK;
}

template <int R>
void launch_frames(const tfft_mistftn_plan* p, const void* in_re, const void* in_im, const void* mask, uint16_t* frames, hipStream_t stream) {
  uint32_t live, grid;
  conv_shape(p->groups, p->num_cus, p->launch_iters, live, grid);
  hipLaunchKernelGGL(mistft256r::frames_kernel<R>, dim3(grid), dim3(k4096::kThreads), mistft256r::lds_bytes<R>(), stream,
                     static_cast<const uint16_t*>(in_re), static_cast<const uint16_t*>(in_im), static_cast<const uint16_t*>(mask), frames,
                     p->in_stride, p->mask_stride, static_cast<uint32_t>(p->total), static_cast<uint32_t>(p->batch), live,
                     static_cast<const uint8_t*>(p->d_tables));
}

}  // namespace

extern "C" {

const char* tfft_mistftn_last_error(void) { return g_err.c_str(); }

int tfft_mistftn_geometry(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  g_err.clear();
  const int rc = check_n(n);
  return rc ? rc : check_geometry(n, length, hop, pad, frames);
}

int tfft_mistftn_describe(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  uint64_t frames = 0;
  const int rc = check_shape(kRules, n, rows, length, hop, pad, flags, &frames);
  if (rc) return rc;
  return copy_text("mistft256r" + std::to_string(n / 256) + ":" + std::to_string(n) + " x " + std::to_string(frames) + " + ola", buf, bytes);
}

int tfft_mistftn_plan_create(uint32_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id, const tfft_mistftn_opts* opts,
                             tfft_mistftn_plan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  // the mask's own refusals, after those of the options struct and the shape (create_plan makes these two again) and before the
  // device is touched
  tfft_mistftn_opts o = TFFT_MISTFTN_OPTS_INIT;
  int rc = take_opts(opts, "tfft_mistftn_opts", o);
  uint64_t frames = 0;
  if (rc == TFFT_OK) rc = check_shape(kRules, n, rows, length, hop, pad, o.flags, &frames);
  if (rc == TFFT_OK) rc = check_mask(n, rows * frames, o);
  if (rc) return rc;
  return create_plan(kRules, n, rows, length, hop, pad, device_id, opts, tfft_mistftn_opts TFFT_MISTFTN_OPTS_INIT, &tfft_mistftn_opts::out_sig_stride,
                     &tfft_mistftn_opts::in_frame_stride, out, tfft_mistftn_plan_destroy, [](tfft_mistftn_plan* p, const tfft_mistftn_opts& o) {
                       p->radix = static_cast<int>(p->n / 256);
                       p->batch = (p->total + 1) / 2;
                       const uint64_t per_wave = 16 / p->radix;                 // transforms a wave takes per iteration
                       p->groups = (p->batch + per_wave - 1) / per_wave;
                       p->flags = o.flags;
                       p->mask_stride = (o.flags & TFFT_MISTFTN_MASK_PER_BIN) ? 0 : o.mask_frame_stride ? o.mask_frame_stride : pitch_of(p->n);
                       p->mask_halves = (p->total - 1) * p->mask_stride + bins_of(p->n);
                       p->ws_need = static_cast<size_t>(p->total * p->n * 2);
                       return p->radix == 2 ? create_device<2>(p) : p->radix == 4 ? create_device<4>(p) : create_device<8>(p);
                     });
}

void tfft_mistftn_plan_destroy(tfft_mistftn_plan* p) {
  if (!p) return;
  destroy_device_base(p);
  if (p->ws && p->ws_owned) (void)hipFree(p->ws);
  delete p;
}

int tfft_mistftn_plan_set_window(tfft_mistftn_plan* p, const void* window, void* stream) { return set_window(p, window, stream); }

size_t tfft_mistftn_plan_workspace_bytes(const tfft_mistftn_plan* p) { return p ? p->ws_need : 0; }

int tfft_mistftn_plan_set_workspace(tfft_mistftn_plan* p, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_set(p, device_ptr, bytes);
}

int tfft_mistftn_plan_prepare(tfft_mistftn_plan* p) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return ws_prepare(p);
}

int tfft_mistftn_exec(const tfft_mistftn_plan* p, const void* in_re, const void* in_im, const void* mask, void* out, void* stream) {
  // the plan, the window and the three pointers tfft_istftn_exec takes, then the mask's pointer, before anything is settled
  int rc = check_exec_args(kRules, p, in_re, in_im, out);
  if (rc) return rc;
  if (!mask) return fail(TFFT_ERR_ARG, "null mask pointer");
  if (reinterpret_cast<uintptr_t>(mask) & 15) return fail(TFFT_ERR_ARG, "the mask must be 16-byte aligned");
  rc = check_exec_inverse(kRules, p, in_re, in_im, out);
  if (rc) return rc;
  // the mask is only read: it may alias the spectra, but not what is written
  const uint64_t mask_bytes = 2 * p->mask_halves, out_bytes = 2 * ((p->rows - 1) * p->out_stride + p->length);
  if (blocks_overlap(out, out_bytes, mask, mask_bytes)) return fail(TFFT_ERR_ARG, "output and mask overlap");
  if (blocks_overlap(p->ws, p->ws_need, mask, mask_bytes)) return fail(TFFT_ERR_ARG, "the workspace overlaps the mask");
  hipStream_t s = static_cast<hipStream_t>(stream);
  uint16_t* const frames = static_cast<uint16_t*>(p->ws);
  if (p->radix == 2) launch_frames<2>(p, in_re, in_im, mask, frames, s);
  else if (p->radix == 4) launch_frames<4>(p, in_re, in_im, mask, frames, s);
  else launch_frames<8>(p, in_re, in_im, mask, frames, s);
  CONV_HIP(hipGetLastError());
  const olan::ola_geometry geo = {p->rows, p->length / 8, ola_hop(p), p->out_stride, static_cast<uint32_t>(p->pad), static_cast<uint32_t>(p->frames),
                                  static_cast<uint32_t>(p->n)};
  hipLaunchKernelGGL(olan::ola_kernel, dim3(ola_grid(p, olan::kOlaBlock)), dim3(olan::kOlaBlock), 0, s, static_cast<const uint16_t*>(frames),
                     static_cast<const uint16_t*>(p->d_window), static_cast<uint16_t*>(out), geo, (p->flags & TFFT_MISTFTN_RAW_SUM) ? 1 : 0);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_mistftn_plan_num_launches(const tfft_mistftn_plan* p) { return p ? 2 : 0; }

int tfft_mistftn_plan_kernels(const tfft_mistftn_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("mistft256r::frames_kernel<" + std::to_string(p->radix) + ">\nolan::ola_kernel\n", 2, buf, bytes);
}

}  // extern "C"
