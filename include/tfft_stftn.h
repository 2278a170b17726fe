/* tfft_stftn.h — C ABI of the short-frame STFT add-on (libtfft_stftn.so) of the MI355X (gfx950) tensor-core FFT library: the plans
 * of tfft_stft.h at the frame lengths n = 512, 1024 and 2048, each in one kernel and one pass over memory.
 *
 * A plan takes `rows` R REAL signals of `length` L samples and a frame length n, the leading argument of every call. With a `hop`
 * and a `pad`, every signal has
 *
 *     F = 1 + floor((L + 2 pad - n) / hop)           frames (tfft_stftn_geometry reports it),
 *
 * and frame f of signal r is the window of n samples that starts at sample f * hop - pad of that signal. Samples outside [0, L)
 * read as zero and are never loaded. pad = 0 is the framing of torch.stft(center=False), pad = n / 2 that of center=True with
 * pad_mode="constant". Every sample j of a frame is multiplied by window value w[j]:
 *
 *     u[j] = fp16(w[j] * x[f * hop - pad + j])       one binary16 multiply, round to nearest even, subnormals kept
 *
 * and the frame's output is bins 0 .. n / 2 of DFT(u) / n, by the arithmetic of tfft_exec_r2c (include/tfft.h) at that n.
 *
 * The add-on is layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): it links against both and uses
 * their status codes (TFFT_OK, TFFT_ERR_*) and conventions. Only plain pointers and sizes cross this boundary: device pointers
 * are raw HIP device addresses, `stream` is a hipStream_t passed as void*.
 *
 * Shapes. n one of 512, 1024, 2048 (4096 is tfft_stft.h's, and is refused here with a pointer to it); L a multiple of 8,
 * 8 .. 2^26; hop a multiple of 8 and >= 8 (it may exceed n: frames then skip samples); pad a multiple of 8, 0 <= pad < n, with
 * L + 2 pad >= n; R >= 1 and R F below 2^32.
 *
 * Data contract. Real binary16; signal r at in + r * in_sig_stride halves, L samples; a stride of 0 means L, otherwise it is a
 * multiple of 8 and >= L. Frames are numbered g = r * F + f. Frame g leaves as two planes of n / 2 + 1 halves, its real parts at
 * out_re + g * out_frame_stride and its imaginary parts at out_im + g * out_frame_stride. A stride of 0 means 2 h with
 * h = tfft_rplan_spectrum_pitch(n) (264, 520, 1032): with out_im = out_re + h the frames are [RE h | IM h] blocks. Otherwise the
 * stride is a multiple of 8 that is at least n / 2 + 1. Halves beyond bin n / 2 of a frame are never written. Pointers are 16-byte
 * aligned. The extents (R - 1) * in_sig_stride + L and (R F - 1) * out_frame_stride + n / 2 + 1 must stay below 2^62 halves.
 *
 * Pairing, which is part of the contract. Frames 2b and 2b + 1 of the flat order g are the RE and the IM plane of ONE complex
 * transform b, whose spectrum is split into the two half spectra; a pair straddles two signals when F is odd. An odd total R F
 * pairs its last frame with itself and writes only that frame. This is exactly a tfft_rplan of n and batch R F (default options)
 * run on the frames u laid out in the order g, and the two agree in every bit. The accuracy is that plan's: per pair, as
 * include/tfft.h states it (a weak frame paired with a strong one carries the strong one's rounding noise).
 *
 * INPUT CONDITION: |u_2b[j] + i u_2b+1[j]| <= 64512 for every sample j of every pair, the TFFT_SCALE_SEQUENTIAL bound of
 * include/tfft.h on the complex sample the pair forms. The condition is on the products u, not on x or w alone. Both frames of a pair
 * may reach 45600 (64512 / sqrt 2) at once. A self-paired last frame counts as its OWN partner, not as a frame beside zeros, so its
 * limit is 45600 too and not 65504. Beyond the limit the result may hold inf / nan; nothing is refused: the condition is on the data.
 * Downwards there is no condition: subnormal x, w and u are kept, but spectra DFT(u) / n below 2^-14 are subnormal binary16 numbers
 * with fewer bits.
 *
 * Aliasing. The output planes' extents must not meet the input's extent, and the written parts of the two planes must not share
 * a half; anything else is refused (TFFT_ERR_ARG). The window is copied into the plan.
 *
 * Life cycle. One kernel, stft256r::stft256r_kernel<R> with R = n / 256, per execution and no workspace. The tables, the window
 * buffer and the LDS opt-in are set up at creation, so an execution only launches: it is legal under stream capture, and
 * executions of one plan may overlap in time.
 */
#ifndef TFFT_STFTN_H_
#define TFFT_STFTN_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_STFTN_API __attribute__((visibility("default")))
#else
#define TFFT_STFTN_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_stftn_plan tfft_stftn_plan;

typedef struct tfft_stftn_opts {
  uint32_t struct_size;      /* sizeof(tfft_stftn_opts) as the caller was compiled (TFFT_STFTN_OPTS_INIT sets it); the struct grows
                                only by appending fields. Any other value is refused (TFFT_ERR_ARG) */
  uint32_t reserved_;        /* must be 0 */
  uint64_t in_sig_stride;    /* halves between consecutive signals of the input: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t out_frame_stride; /* halves between consecutive frames of an output plane: 0 (= 2 h) or a multiple of 8 that is >= n / 2 + 1 */
  uint32_t launch_iters;     /* launch shape, as tfft_stft_opts.launch_iters, over groups of 4096 / n transforms: 0 = the library's
                                default; k = 1 .. 65534: a wave takes about k groups and retires; TFFT_LAUNCH_PERSISTENT: one
                                workgroup per CU for all groups. Never changes results */
  int flags;                 /* no flag is defined yet: must be 0 */
} tfft_stftn_opts;
#define TFFT_STFTN_OPTS_INIT {(uint32_t)sizeof(tfft_stftn_opts)}

/* Host only: the frames per signal of a plan for `n`, `length`, `hop` and `pad`; the pointer may be NULL. TFFT_ERR_ARG for values
 * that tfft_stftn_plan_create refuses. */
TFFT_STFTN_API int tfft_stftn_geometry(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames);

/* opts: NULL (all defaults) or a tfft_stftn_opts. TFFT_ERR_ARG for anything outside the shapes above, checked before the device is
 * touched; TFFT_ERR_DEVICE / TFFT_ERR_HIP as tfft_plan_create. The first call compares tfft_abi_version() of the libtfft.so it
 * runs against with the TFFT_ABI_VERSION it was built with. */
TFFT_STFTN_API int tfft_stftn_plan_create(uint32_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id,
                                          const tfft_stftn_opts* opts, tfft_stftn_plan** out);
TFFT_STFTN_API void tfft_stftn_plan_destroy(tfft_stftn_plan* plan);

/* Copies the n binary16 window values at `window` (device memory) into a buffer the plan owns, ordered on `stream`; the caller's
 * buffer is not referenced once the copy has run. May be called again to replace the window: executions enqueued on `stream`
 * afterwards see the new one (executions on other streams are the caller's to order). The plan's device must be current.
 * tfft_stftn_exec before any set_window is TFFT_ERR_ARG. */
TFFT_STFTN_API int tfft_stftn_plan_set_window(tfft_stftn_plan* plan, const void* window, void* stream);

/* Enqueues all frames on `stream` (NULL = default stream); does not synchronise. The plan's device must be current. A refused call
 * launches nothing. */
TFFT_STFTN_API int tfft_stftn_exec(const tfft_stftn_plan* plan, const void* in, void* out_re, void* out_im, void* stream);

/* Kernel launches of one execution (1; 0 for NULL), and their names one per line in launch order
 * ("stft256r::stft256r_kernel<R>", R = 2, 4 or 8). _kernels returns the number of lines, or TFFT_ERR_ARG when `bytes` is too small. */
TFFT_STFTN_API int tfft_stftn_plan_num_launches(const tfft_stftn_plan* plan);
TFFT_STFTN_API int tfft_stftn_plan_kernels(const tfft_stftn_plan* plan, char* buf, size_t bytes);

/* Host only: what tfft_stftn_plan_create would build, as text: "stft256r<R>:n x F" with R = n / 256 and F the frames per signal,
 * "stft256r4:1024 x 13" for instance. Refuses what tfft_stftn_plan_create refuses on the same shape and flags. */
TFFT_STFTN_API int tfft_stftn_describe(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes);

/* Message of the last failure of a tfft_stftn_* call on this thread ("" if none). */
TFFT_STFTN_API const char* tfft_stftn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_STFTN_H_ */
