// tfft_spec.hip — host side and C ABI (include/tfft_spec.h) of the spectrogram add-on, libtfft_spec.so: the power spectrogram and
// band energies of the short-frame STFT at the frame lengths 512, 1024 and 2048.
//
// Layered on libtfft_conv.so and libtfft.so through their public headers only; from csrc/ it takes k4096.hpp and rsplit.hpp, header
// only, for the device helpers, and k256r.hpp, in the host pass, for the constant tables of the kernel. The geometry, shape and
// stride refusals, the plan-create sequence, the window and the hold on k256r.hpp come from conv/stft_host.hpp, which the STFT
// libraries share (the float frame side goes through its frame_layout); here are the plan struct, check_n, the options of its own
// (bands, gain), the bands, the check of an execution with one fp32 output, the kernels' LDS opt-in, the launch and the two texts.
// tests/test_gpu_spec.py holds both modes to a float32 restatement on what tfft_stftn_exec writes, bit for bit.
#include "../../include/tfft_spec.h"
#include "spec256r.hpp"
#define STFT_HOST_256R spec256r
#include "../conv/stft_host.hpp"

#include <cmath>

struct tfft_spec_plan {
  uint64_t n = 0, rows = 0, length = 0, hop = 0, pad = 0, frames = 0, total = 0, batch = 0, groups = 0, in_stride = 0, out_stride = 0;
  uint32_t launch_iters = 0;
  int radix = 0;                     // R = n / 256
  int device = 0, num_cus = 256;
  uint32_t bands = 0;                // 0: power mode
  float gain = 1.0f;
  void* d_tables = nullptr;          // k256r::build_tables(R)
  uint16_t* d_window = nullptr;      // n halves, the plan's own copy
  spec256r::band* d_bands = nullptr; // `bands` descriptors
  float* d_weights = nullptr;        // the weights of all bands back to back; at most bands * (n / 2 + 1)
  bool have_window = false, have_bands = false;
};

namespace {

static_assert(spec256r::kMaxBands == TFFT_SPEC_MAX_BANDS, "spec256r.hpp and tfft_spec.h disagree on the band count");

int check_n(uint32_t n) {
  if (n == 4096)
    return fail(TFFT_ERR_ARG, "n = 4096: the spectrogram plans stop at 2048; the STFT at 4096 is tfft_stft_plan_create (include/tfft_stft.h)");
  if (n != 512 && n != 1024 && n != 2048) return fail(TFFT_ERR_ARG, "n must be 512, 1024 or 2048 (" + std::to_string(n) + ")");
  return TFFT_OK;
}
constexpr stft_rules kRules = {"spec", false, 0, "must be 0", check_n};

// the options of this library's own, and what a frame of the output is
int frame_side(uint64_t n, const tfft_spec_opts& o, frame_layout& layout) {
  if (o.bands > TFFT_SPEC_MAX_BANDS)
    return fail(TFFT_ERR_ARG, "tfft_spec_opts.bands must be 0 (power mode) or 1 .. 1024 (" + std::to_string(o.bands) + ")");
  if (!std::isfinite(o.gain) || !(o.gain > 0.0f)) return fail(TFFT_ERR_ARG, "tfft_spec_opts.gain must be finite and > 0");
  layout = o.bands ? frame_layout{o.bands, o.bands, 1, 4, "floats"} : frame_layout{bins_of(n), pitch_of(n), 4, 4, "floats"};
  return TFFT_OK;
}

template <int R>
int create_device(tfft_spec_plan* p) {
  std::vector<uint8_t> blob;
  k256r_host::build_tables(R, blob);
  const int rc = create_device_base(p, blob, blob.size());
  if (rc) return rc;
  if (p->bands) {
    CONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_bands), p->bands * sizeof(spec256r::band)));
    CONV_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_weights), p->bands * bins_of(p->n) * sizeof(float)));
    // more than 64 KiB of dynamic LDS: opt in now, so that an execution is a pure launch
    CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(spec256r::spec_kernel<R, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 spec256r::spec_lds_bytes<R, true>()));
  } else {
    CONV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(spec256r::spec_kernel<R, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 spec256r::spec_lds_bytes<R, false>()));
  }
  return TFFT_OK;
}

template <int R, bool kBands>
void launch(const tfft_spec_plan* p, const void* in, void* out, hipStream_t stream) {
  const spec256r::geometry geo = {static_cast<int32_t>(p->length / 8), p->frames > 1 ? static_cast<int32_t>(p->hop / 8) : 0,
                                  static_cast<int32_t>(p->pad / 8), static_cast<uint32_t>(p->frames)};
  uint32_t live, grid;
  conv_shape(p->groups, p->num_cus, p->launch_iters, live, grid);
  constexpr int lds = spec256r::spec_lds_bytes<R, kBands>();
  hipLaunchKernelGGL((spec256r::spec_kernel<R, kBands>), dim3(grid), dim3(k4096::kThreads), lds, stream,
                     static_cast<const uint16_t*>(in), static_cast<const uint16_t*>(p->d_window), static_cast<float*>(out), p->in_stride,
                     p->out_stride, geo, static_cast<uint32_t>(p->total), static_cast<uint32_t>(p->batch), live,
                     static_cast<const uint8_t*>(p->d_tables), p->gain, p->bands, static_cast<const spec256r::band*>(p->d_bands),
                     static_cast<const float*>(p->d_weights));
}

template <int R>
void launch_mode(const tfft_spec_plan* p, const void* in, void* out, hipStream_t stream) {
  if (p->bands) launch<R, true>(p, in, out, stream);
  else launch<R, false>(p, in, out, stream);
}

}  // namespace

extern "C" {

const char* tfft_spec_last_error(void) { return g_err.c_str(); }

int tfft_spec_geometry(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames) {
  g_err.clear();
  const int rc = check_n(n);
  return rc ? rc : check_geometry(n, length, hop, pad, frames);
}

int tfft_spec_describe(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  uint64_t frames = 0;
  const int rc = check_shape(kRules, n, rows, length, hop, pad, flags, &frames);
  if (rc) return rc;
  return copy_text("spec256r" + std::to_string(n / 256) + ":" + std::to_string(n) + " x " + std::to_string(frames), buf, bytes);
}

int tfft_spec_plan_create(uint32_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id, const tfft_spec_opts* opts,
                          tfft_spec_plan** out) {
  return create_plan(
      kRules, n, rows, length, hop, pad, device_id, opts, tfft_spec_opts TFFT_SPEC_OPTS_INIT, &tfft_spec_opts::in_sig_stride,
      &tfft_spec_opts::out_frame_stride, out, tfft_spec_plan_destroy,
      [](tfft_spec_plan* p, const tfft_spec_opts& o) {
        p->radix = static_cast<int>(p->n / 256);
        p->batch = (p->total + 1) / 2;
        const uint64_t per_wave = 16 / p->radix;                 // transforms a wave takes per iteration
        p->groups = (p->batch + per_wave - 1) / per_wave;
        p->bands = o.bands;
        p->gain = o.gain;
        return p->radix == 2 ? create_device<2>(p) : p->radix == 4 ? create_device<4>(p) : create_device<8>(p);
      },
      frame_side);
}

void tfft_spec_plan_destroy(tfft_spec_plan* p) {
  if (!p) return;
  destroy_device_base(p);
  if (p->d_bands) (void)hipFree(p->d_bands);
  if (p->d_weights) (void)hipFree(p->d_weights);
  delete p;
}

int tfft_spec_plan_set_window(tfft_spec_plan* p, const void* window, void* stream) { return set_window(p, window, stream); }

int tfft_spec_plan_set_bands(tfft_spec_plan* p, uint32_t nbands, const uint32_t* starts, const uint32_t* counts, const float* weights,
                             void* stream) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  if (!p->bands) return fail(TFFT_ERR_ARG, "a power plan (tfft_spec_opts.bands = 0) takes no bands");
  if (nbands != p->bands)
    return fail(TFFT_ERR_ARG, "nbands = " + std::to_string(nbands) + ", but the plan was created for " + std::to_string(p->bands) + " bands");
  if (!starts || !counts || !weights) return fail(TFFT_ERR_ARG, "null band pointer");
  const uint64_t bins = bins_of(p->n);
  std::vector<spec256r::band> desc(nbands);
  uint64_t offset = 0;
  for (uint32_t j = 0; j < nbands; ++j) {
    if (counts[j] == 0) return fail(TFFT_ERR_ARG, "band " + std::to_string(j) + " has count 0: a band holds at least one bin");
    if (starts[j] >= bins || counts[j] > bins - starts[j])
      return fail(TFFT_ERR_ARG, "band " + std::to_string(j) + " (bins " + std::to_string(starts[j]) + " .. " +
                                    std::to_string(static_cast<uint64_t>(starts[j]) + counts[j] - 1) + ") reaches past bin n / 2 = " +
                                    std::to_string(bins - 1));
    desc[j] = {starts[j], counts[j], static_cast<uint32_t>(offset), 0};
    offset += counts[j];                                       // at most 1024 * 1025
  }
  for (uint64_t i = 0; i < offset; ++i)
    if (!std::isfinite(weights[i])) return fail(TFFT_ERR_ARG, "weight " + std::to_string(i) + " is not finite");
  const int rc = check_current(p->device);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // executions in flight keep reading the old bands: the device is drained before they are replaced
  if (p->have_bands) CONV_HIP(hipDeviceSynchronize());
  CONV_HIP(hipMemcpyAsync(p->d_bands, desc.data(), desc.size() * sizeof(spec256r::band), hipMemcpyHostToDevice, s));
  CONV_HIP(hipMemcpyAsync(p->d_weights, weights, offset * sizeof(float), hipMemcpyHostToDevice, s));
  CONV_HIP(hipStreamSynchronize(s));                           // the host arrays are the caller's again
  p->have_bands = true;
  return TFFT_OK;
}

int tfft_spec_exec(const tfft_spec_plan* p, const void* in, void* out, void* stream) {
  int rc = check_exec_args(kRules, p, in, out, out);
  if (rc) return rc;
  if (p->bands && !p->have_bands) return fail(TFFT_ERR_ARG, "no bands: call tfft_spec_plan_set_bands first");
  // frames of one signal overlap, and frames are work items of different waves that run in no defined order
  const uint64_t per_frame = p->bands ? p->bands : bins_of(p->n);
  const uint64_t in_bytes = 2 * ((p->rows - 1) * p->in_stride + p->length), out_bytes = 4 * ((p->total - 1) * p->out_stride + per_frame);
  if (blocks_overlap(in, in_bytes, out, out_bytes))
    return fail(TFFT_ERR_ARG, "input and output overlap (a spectrogram plan cannot run in place: frames share input samples)");
  rc = check_current(p->device);
  if (rc) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (p->radix == 2) launch_mode<2>(p, in, out, s);
  else if (p->radix == 4) launch_mode<4>(p, in, out, s);
  else launch_mode<8>(p, in, out, s);
  CONV_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_spec_plan_num_launches(const tfft_spec_plan* p) { return p ? 1 : 0; }

int tfft_spec_plan_kernels(const tfft_spec_plan* p, char* buf, size_t bytes) {
  g_err.clear();
  if (!p) return fail(TFFT_ERR_ARG, "null plan");
  return kernel_names("spec256r::spec_kernel<" + std::to_string(p->radix) + ", " + tf_text(p->bands != 0) + ">\n", 1, buf, bytes);
}

}  // extern "C"
