/* tfft_spec.h — C ABI of the spectrogram add-on (libtfft_spec.so) of the MI355X (gfx950) tensor-core FFT library: the power
 * spectrogram and band energies (mel, bark, third-octave, any filterbank) of the short-frame STFT of tfft_stftn.h, at the frame
 * lengths n = 512, 1024 and 2048, in one kernel and one pass over memory. The complex STFT never reaches memory.
 *
 * The contract is arithmetic on what a tfft_stftn plan writes. Let (re, im) be the binary16 bins 0 .. n / 2 that
 * tfft_stftn_exec leaves for the same n, rows, length, hop, pad, input and window: rfft(w * frame) / n. The framing, the pad, the
 * frame order g = r * F + f and the pairing of frames 2b and 2b + 1 are that header's, and so is its INPUT CONDITION.
 *
 * Power mode (tfft_spec_opts.bands == 0). For k = 0 .. n / 2
 *
 *     P[g][k] = fp32(gain * fp32(fp32(re)^2 + fp32(im)^2))
 *
 * The squares of binary16 values are exact in fp32, so the sum is rounded once and the product with the gain once more. A power
 * of two such as gain = n^2, which undoes the family's 1 / n scaling, rounds nothing short of overflow; beyond fp32's range the
 * product is +inf, never a NaN. Not pinned: a product gain * (re^2 + im^2) below 2^-126 (the device may flush it). The output is fp32 and
 * frame-major: frame g at out + g * out_frame_stride floats. The stride defaults to tfft_rplan_spectrum_pitch(n) (264, 520, 1032);
 * otherwise it is a multiple of 4 that is at least n / 2 + 1. Floats behind bin n / 2 of a frame are never written.
 *
 * Band mode (bands = B, 1 <= B <= 1024). The plan holds B bands, set once with tfft_spec_plan_set_bands. Band j has a first bin
 * start[j], a count[j] >= 1 with start[j] + count[j] <= n / 2 + 1, and count[j] fp32 weights w. Its output is
 *
 *     acc = fp32(w[0] * P[start]);   acc = fp32(acc + fp32(w[i] * P[start + i]))   for i = 1 .. count - 1 in ascending order
 *
 * with every product and every sum rounded on its own (no fused multiply-add), no atomics and an order that does not depend on the
 * launch shape: a float32 restatement in numpy reproduces every bit. Not pinned: products w[i] * P below 2^-126 (the device may
 * flush them). The output is fp32, frame g at out + g * out_frame_stride floats, B floats; the stride defaults to B and may be
 * anything >= B. P itself is never written. Bands may overlap, come in any order and leave bins unused.
 *
 * Left out on purpose: magnitude, log and dB. The device's sqrt and log are not correctly rounded, so their bits cannot be pinned
 * to a restatement; on a band output of B floats per frame the caller's own elementwise operation costs little.
 *
 * Shapes and input as tfft_stftn.h: n one of 512, 1024, 2048 (4096 is refused: the spectrogram plans stop at 2048, and
 * tfft_stft_plan_create gives the STFT there); L a multiple of 8, 8 .. 2^26; hop a multiple of 8; pad a multiple of 8 below n with
 * L + 2 pad >= n; real binary16 signals, signal r at in + r * in_sig_stride halves (0 = L, else a multiple of 8 that is >= L).
 * Pointers are 16-byte aligned. Input and output must not overlap (TFFT_ERR_ARG). The window, the bands and the weights are copied
 * into the plan.
 *
 * Life cycle. One kernel, spec256r::spec_kernel<R, bands> with R = n / 256, per execution and no workspace: an execution only
 * launches, is legal under stream capture, and executions of one plan may overlap in time. tfft_spec_exec before
 * tfft_spec_plan_set_window, or on a band plan before tfft_spec_plan_set_bands, is refused.
 *
 * Layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): status codes and conventions are theirs.
 */
#ifndef TFFT_SPEC_H_
#define TFFT_SPEC_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_SPEC_API __attribute__((visibility("default")))
#else
#define TFFT_SPEC_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_spec_plan tfft_spec_plan;

#define TFFT_SPEC_MAX_BANDS 1024

typedef struct tfft_spec_opts {
  uint32_t struct_size;      /* sizeof(tfft_spec_opts) as the caller was compiled (TFFT_SPEC_OPTS_INIT sets it); the struct grows only
                                by appending fields. Any other value is refused (TFFT_ERR_ARG) */
  uint32_t reserved_;        /* must be 0 */
  uint64_t in_sig_stride;    /* halves between consecutive signals of the input: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t out_frame_stride; /* FLOATS between consecutive frames of the output. Power mode: 0 (= tfft_rplan_spectrum_pitch(n)) or a
                                multiple of 4 that is >= n / 2 + 1. Band mode: 0 (= bands) or anything >= bands */
  uint32_t launch_iters;     /* launch shape, as tfft_stftn_opts.launch_iters. Never changes results */
  int flags;                 /* no flag is defined yet: must be 0 */
  uint32_t bands;            /* 0: power mode; B = 1 .. TFFT_SPEC_MAX_BANDS: band mode with B bands */
  float gain;                /* the factor of every power: finite and > 0 (TFFT_SPEC_OPTS_INIT: 1) */
} tfft_spec_opts;
#define TFFT_SPEC_OPTS_INIT {(uint32_t)sizeof(tfft_spec_opts), 0, 0, 0, 0, 0, 0, 1.0f}

/* Host only: the frames per signal, as tfft_stftn_geometry; the pointer may be NULL. */
TFFT_SPEC_API int tfft_spec_geometry(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames);

/* opts: NULL (power mode, gain 1, default strides) or a tfft_spec_opts. TFFT_ERR_ARG for anything outside the shapes above, checked
 * before the device is touched; TFFT_ERR_DEVICE / TFFT_ERR_HIP as tfft_plan_create: without a GPU a plan is an error, never a
 * fallback. */
TFFT_SPEC_API int tfft_spec_plan_create(uint32_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id,
                                        const tfft_spec_opts* opts, tfft_spec_plan** out);
TFFT_SPEC_API void tfft_spec_plan_destroy(tfft_spec_plan* plan);

/* Copies the n binary16 window values at `window` (device memory) into the plan, ordered on `stream`, as
 * tfft_stftn_plan_set_window. */
TFFT_SPEC_API int tfft_spec_plan_set_window(tfft_spec_plan* plan, const void* window, void* stream);

/* The bands of a band plan, from HOST memory: `starts` and `counts` hold nbands values each, `weights` the
 * counts[0] + counts[1] + ... fp32 weights of band 0, band 1, ... back to back. Refused (TFFT_ERR_ARG): a power plan, nbands other
 * than the plan's, a count of 0, a band that reaches past bin n / 2, a weight that is not finite. The arrays are copied to the
 * device on `stream` and are the caller's again on return. May be called again: executions in flight are waited for first. */
TFFT_SPEC_API int tfft_spec_plan_set_bands(tfft_spec_plan* plan, uint32_t nbands, const uint32_t* starts, const uint32_t* counts,
                                           const float* weights, void* stream);

/* Enqueues all frames on `stream` (NULL = default stream); does not synchronise. in: binary16 signals; out: fp32, see above. The
 * plan's device must be current. A refused call launches nothing. */
TFFT_SPEC_API int tfft_spec_exec(const tfft_spec_plan* plan, const void* in, void* out, void* stream);

/* Kernel launches of one execution (1; 0 for NULL), and their names one per line ("spec256r::spec_kernel<R, false>" for a power
 * plan, "<R, true>" for a band plan). _kernels returns the number of lines, or TFFT_ERR_ARG when `bytes` is too small. */
TFFT_SPEC_API int tfft_spec_plan_num_launches(const tfft_spec_plan* plan);
TFFT_SPEC_API int tfft_spec_plan_kernels(const tfft_spec_plan* plan, char* buf, size_t bytes);

/* Host only: what tfft_spec_plan_create would build, as text: "spec256r<R>:n x F" with R = n / 256 and F the frames per signal.
 * Refuses what tfft_spec_plan_create refuses on the same shape and flags. */
TFFT_SPEC_API int tfft_spec_describe(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes);

/* Message of the last failure of a tfft_spec_* call on this thread ("" if none). */
TFFT_SPEC_API const char* tfft_spec_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_SPEC_H_ */
