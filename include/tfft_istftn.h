/* tfft_istftn.h — C ABI of the short-frame inverse STFT add-on (libtfft_istftn.so) of the MI355X (gfx950) tensor-core FFT library:
 * the plans of tfft_istft.h at the frame lengths n = 512, 1024 and 2048: half spectra of hopped frames of n samples back to real
 * signals, by a one-pass C2R of every frame and a windowed overlap-add in a fixed order. It is the way back from
 * include/tfft_stftn.h. The frame length n is the leading argument of every call that has a shape.
 *
 * Geometry, as tfft_stftn.h: `rows` R real signals of `length` L samples, a frame length n, a `hop` and a `pad`;
 *
 *     F = 1 + floor((L + 2 pad - n) / hop)           frames per signal (tfft_istftn_geometry reports it),
 *
 * and frame g = r * F + f covers samples f * hop - pad .. + n - 1 of signal r.
 *
 * Shapes. n one of 512, 1024, 2048 (4096 is tfft_istft.h's, and is refused here with a pointer to tfft_istft_plan_create); L a
 * multiple of 8, 8 .. 2^26; hop a multiple of 8 and >= 8 (it may exceed n: the samples between frames come out as +0); pad a
 * multiple of 8, 0 <= pad < n, with L + 2 pad >= n; R >= 1 and R F below 2^32.
 *
 * Input. Two planes of half spectra in binary16, frame g at in_re / in_im + g * in_frame_stride halves, the values DFT(u) / n that
 * tfft_stftn_exec writes. A stride of 0 means 2 h with h = tfft_rplan_spectrum_pitch(n) (264, 520, 1032), which is exactly what
 * tfft_stftn_exec writes by default: stft(n) -> istft(n) needs no repacking. Otherwise the stride is a multiple of 8 that is at
 * least n / 2 + 1. Bins 0 .. n / 2 are read; the IM of bins 0 and n / 2 is ignored; halves beyond bin n / 2 of a frame are never
 * read. The two planes may interleave ([RE h | IM h] blocks). The inputs are never written.
 *
 * Arithmetic, which is the contract (tests hold it bit for bit):
 *
 *   1. merge with gain. Transform b takes frames 2b (A) and 2b + 1 (B) of the flat order g, the pairing of tfft_stftn.h; an odd total
 *      pairs its last frame with itself (B = A, the second result is discarded). Z' = merge(A, B) by the formulas of tfft_exec_c2r
 *      with one exact factor in front of the single rounding: Z'[k] = fp16(float(n) * (fp32 add)), on the edge bins 0 and n / 2
 *      fp16(float(n) * fp32(A.re)) and fp16(float(n) * fp32(B.re)). The gain undoes the 1 / n of the forward transform BEFORE the
 *      inverse stages, not after them: a frame kept at x / n would pass those stages near binary16's subnormals.
 *      INPUT CONDITION: |n (A[k] + i B[k])| <= 64512 for every bin, the TFFT_SCALE_SEQUENTIAL bound of include/tfft.h. Beyond it
 *      the result may hold inf / nan. Nothing is refused: the condition is on the data. Spectra of tfft_stftn_exec of signals and
 *      windows with |w x| <= 1 satisfy it unless they were amplified afterwards: A[k] + i B[k] = DFT(u_2b + i u_2b+1)[k] / n, so
 *      |A[k] + i B[k]| <= mean_j |u_2b[j] + i u_2b+1[j]|, and a pair is safe when that mean is <= 64512 / n (126, 63, 31.5). On the
 *      lower side nothing overflows, but spectra DFT(u) / n below 2^-14 are subnormal binary16 numbers with fewer bits. Subnormals are
 *      kept everywhere: in the loads, in the conversions around the gain and in the output.
 *   2. inverse transform. tfft_exec_inverse of the default plan of n (sequential scaling) on Z'. The RE result is frame 2b, the IM
 *      result frame 2b + 1; each is rounded once to binary16 and stored in the workspace at g * n halves.
 *   3. overlap-add. For sample t of signal r, f ascending over the frames that cover t, j = t + pad - f * hop, both sums from +0:
 *          num = sum fp32(w[j]) * fp32(v_g[j])      den = sum fp32(w[j]) * fp32(w[j])        (every product exact in fp32)
 *      y = fp16(num / den) where den > 0, the fp32 division correctly rounded; y = +0 where den = 0: samples no frame covers (the gaps
 *      of hop > n, a tail the last frame does not reach) and samples that lie only under zeros of the window. den = 0 is defined, not
 *      refused. With TFFT_ISTFTN_RAW_SUM, y = fp16(num) everywhere.
 *
 * Output. Real binary16, signal r at out + r * out_sig_stride halves; a stride of 0 means L, otherwise it is a multiple of 8 that is
 * at least L. Every sample of [0, L) of every signal is written exactly once, and nothing else is written. Pointers are 16-byte
 * aligned. The extents (R F - 1) * in_frame_stride + n / 2 + 1 and (R - 1) * out_sig_stride + L must stay below 2^62 halves.
 *
 * Workspace: R F * n halves for the time-domain frames, by the rules of tfft_conv.h / tfft_bconv.h: _workspace_bytes,
 * _set_workspace (256-byte aligned), _prepare, or a lazy hipMalloc on the first execution. Once it is settled an execution only
 * launches: it is legal under stream capture. Executions of one plan share the workspace and must not overlap in time.
 *
 * Aliasing. The output's extent must not meet the inputs' extents or the workspace, and the workspace must not meet the inputs;
 * anything else is refused (TFFT_ERR_ARG) and nothing is launched. The window is copied into the plan.
 *
 * The add-on is layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): it links against both and uses
 * their status codes (TFFT_OK, TFFT_ERR_*) and conventions. Only plain pointers and sizes cross this boundary: device pointers
 * are raw HIP device addresses, `stream` is a hipStream_t passed as void*.
 */
#ifndef TFFT_ISTFTN_H_
#define TFFT_ISTFTN_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_ISTFTN_API __attribute__((visibility("default")))
#else
#define TFFT_ISTFTN_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_istftn_plan tfft_istftn_plan;

/* tfft_istftn_opts.flags */
enum { TFFT_ISTFTN_RAW_SUM = 1 }; /* y = fp16(num): no division by the window envelope */

typedef struct tfft_istftn_opts {
  uint32_t struct_size;     /* sizeof(tfft_istftn_opts) as the caller was compiled (TFFT_ISTFTN_OPTS_INIT sets it); the struct grows only
                               by appending fields. Any other value is refused (TFFT_ERR_ARG) */
  uint32_t reserved_;       /* must be 0 */
  uint64_t in_frame_stride; /* halves between consecutive frames of an input plane: 0 (= 2 h) or a multiple of 8 that is >= n / 2 + 1 */
  uint64_t out_sig_stride;  /* halves between consecutive signals of the output: 0 (= L) or a multiple of 8 that is >= L */
  uint32_t launch_iters;    /* launch shape of the frames kernel, as tfft_stftn_opts.launch_iters, over groups of 4096 / n transforms:
                               0 = the library's default; k = 1 .. 65534: a wave takes about k groups and retires;
                               TFFT_LAUNCH_PERSISTENT: one workgroup per CU for all groups. Never changes results */
  int flags;                /* 0 or TFFT_ISTFTN_RAW_SUM */
} tfft_istftn_opts;
#define TFFT_ISTFTN_OPTS_INIT {(uint32_t)sizeof(tfft_istftn_opts)}

/* Host only: the frames per signal of a plan for `n`, `length`, `hop` and `pad`; the pointer may be NULL. TFFT_ERR_ARG for values
 * that tfft_istftn_plan_create refuses. */
TFFT_ISTFTN_API int tfft_istftn_geometry(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames);

/* opts: NULL (all defaults) or a tfft_istftn_opts. TFFT_ERR_ARG for anything outside the shapes above, checked before the device is
 * touched; TFFT_ERR_DEVICE / TFFT_ERR_HIP as tfft_plan_create. The first call compares tfft_abi_version() of the libtfft.so it
 * runs against with the TFFT_ABI_VERSION it was built with. */
TFFT_ISTFTN_API int tfft_istftn_plan_create(uint32_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id,
                                            const tfft_istftn_opts* opts, tfft_istftn_plan** out);
TFFT_ISTFTN_API void tfft_istftn_plan_destroy(tfft_istftn_plan* plan);

/* Copies the n binary16 window values at `window` (device memory) into a buffer the plan owns, ordered on `stream`, exactly as
 * tfft_stftn_plan_set_window does. May be called again to replace the window. The plan's device must be current. tfft_istftn_exec
 * before any set_window is TFFT_ERR_ARG. */
TFFT_ISTFTN_API int tfft_istftn_plan_set_window(tfft_istftn_plan* plan, const void* window, void* stream);

/* Bytes of workspace one execution needs (R F * n halves; 0 for NULL). */
TFFT_ISTFTN_API size_t tfft_istftn_plan_workspace_bytes(const tfft_istftn_plan* plan);
/* Hands in a caller-owned workspace of at least that many bytes, 256-byte aligned (TFFT_ERR_WORKSPACE when too small); NULL returns to
 * a workspace of the plan's own. Not while an execution is in flight. */
TFFT_ISTFTN_API int tfft_istftn_plan_set_workspace(tfft_istftn_plan* plan, void* device_ptr, size_t bytes);
/* Allocates the plan's own workspace now unless one is settled: every later execution only launches. */
TFFT_ISTFTN_API int tfft_istftn_plan_prepare(tfft_istftn_plan* plan);

/* Enqueues both kernels on `stream` (NULL = default stream); does not synchronise. The plan's device must be current. A refused call
 * launches nothing. */
TFFT_ISTFTN_API int tfft_istftn_exec(const tfft_istftn_plan* plan, const void* in_re, const void* in_im, void* out, void* stream);

/* Kernel launches of one execution (2; 0 for NULL), and their names one per line in launch order ("istft256r::frames_kernel<R>",
 * R = 2, 4 or 8, and "olan::ola_kernel"). _kernels returns the number of lines, or TFFT_ERR_ARG when `bytes` is too small. */
TFFT_ISTFTN_API int tfft_istftn_plan_num_launches(const tfft_istftn_plan* plan);
TFFT_ISTFTN_API int tfft_istftn_plan_kernels(const tfft_istftn_plan* plan, char* buf, size_t bytes);

/* Host only: what tfft_istftn_plan_create would build, as text: "istft256r<R>:n x F + ola" with R = n / 256 and F the frames per
 * signal, "istft256r4:1024 x 13 + ola" for instance. Refuses what tfft_istftn_plan_create refuses on the same shape and flags. */
TFFT_ISTFTN_API int tfft_istftn_describe(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes);

/* Message of the last failure of a tfft_istftn_* call on this thread ("" if none). */
TFFT_ISTFTN_API const char* tfft_istftn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_ISTFTN_H_ */
