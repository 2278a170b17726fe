/* tfft_istft.h — C ABI of the inverse short-time Fourier transform add-on (libtfft_istft.so) of the MI355X (gfx950) tensor-core FFT
 * library: half spectra of hopped frames of 4096 samples back to real signals, by a one-pass C2R of every frame and a windowed
 * overlap-add in a fixed order. It is the way back from include/tfft_stft.h.
 *
 * Geometry, as tfft_stft.h: `rows` R real signals of `length` L samples, frame length n = 4096 (TFFT_ISTFT_N), a `hop` and a `pad`;
 *
 *     F = 1 + floor((L + 2 pad - 4096) / hop)        frames per signal (tfft_istft_geometry reports it),
 *
 * and frame g = r * F + f covers samples f * hop - pad .. + 4095 of signal r.
 *
 * Shapes. L a multiple of 8, 8 .. 2^26; hop a multiple of 8 and >= 8 (it may exceed 4096: the samples between frames come out as
 * +0); pad a multiple of 8, 0 <= pad < 4096, with L + 2 pad >= 4096; R >= 1 and R F below 2^32.
 *
 * Input. Two planes of half spectra in binary16, frame g at in_re / in_im + g * in_frame_stride halves, the values DFT(u) / 4096 that
 * tfft_stft_exec writes. A stride of 0 means 2 * 2056, which is exactly what tfft_stft_exec writes by default: stft -> istft needs no
 * repacking. Otherwise the stride is a multiple of 8 that is at least 2049. Bins 0 .. 2048 are read; the IM of bins 0 and 2048 is
 * ignored; halves beyond bin 2048 of a frame are never read. The two planes may interleave ([RE h | IM h] blocks). The inputs are
 * never written.
 *
 * Arithmetic, which is the contract (tests hold it bit for bit):
 *
 *   1. merge with gain. Item i takes frames 2i (A) and 2i + 1 (B) of the flat order g, the pairing of tfft_stft.h; an odd total pairs
 *      its last frame with itself (B = A, the second result is discarded). Z' = merge(A, B) by the formulas of tfft_exec_c2r with one
 *      exact factor in front of the single rounding: Z'[k] = fp16(4096.0f * (fp32 add)), on the edge bins 0 and 2048
 *      fp16(4096.0f * fp32(A.re)) and fp16(4096.0f * fp32(B.re)). The gain undoes the 1 / 4096 of the forward transform BEFORE the
 *      inverse stages, not after them.
 *      INPUT CONDITION: |4096 (A[k] + i B[k])| <= 64512 for every bin, the TFFT_SCALE_SEQUENTIAL bound of include/tfft.h. Beyond it
 *      the result may hold inf / nan. Nothing is refused: the condition is on the data. Spectra of tfft_stft_exec of signals and
 *      windows with |w x| <= 1 satisfy it unless they were amplified afterwards.
 *      A condition a caller of stft -> istft can check on the products u = w x: A[k] + i B[k] = DFT(u_2i + i u_2i+1)[k] / 4096, so
 *      |A[k] + i B[k]| <= mean_j |u_2i[j] + i u_2i+1[j]|, and a pair is safe when that mean is <= 64512 / 4096 = 15.75: in particular
 *      when both frames have rms(u) <= 15.75 / sqrt 2 = 11.1, or mean |u| <= 7.875. (mean |u| <= 11.1 alone is NOT enough: a cosine and
 *      a sine of the same bin with mean |u| = 11.1 give |4096 (A + i B)| = 71400.) The limit binds far below the forward plan's: under
 *      a rectangular window with hop 4096 a tone c cos(2 pi k0 t / 4096) passes up to c = 22.27 (A[k0] = B[k0] = c / 2, |4096 (A + i B)| =
 *      4096 c / sqrt 2), a constant only up to c = 11.13 (A[0] = B[0] = c): a constant of 22 ends in inf. uniform(-1, 1) noise under a
 *      Hann window passes up to a factor 2^8. On the lower side nothing overflows, but the round trip loses accuracy: below about
 *      |x| = 2^-6 the spectra DFT(u) / 4096 enter binary16's subnormals (99 % of the halves at |x| = 2^-10), and istft(stft(x)) against
 *      x degrades from 4.3e-4 to 3.3e-3 at |x| = 2^-10 and 5.2e-2 at 2^-14 (rel-L2, Hann, hop 1024). Subnormals are kept everywhere:
 *      in the loads, in the conversions around the gain and in the output.
 *   2. inverse transform. tfft_exec_inverse of the default N = 4096 plan (sequential scaling) on Z'. The RE result is frame 2i, the IM
 *      result frame 2i + 1; each is rounded once to binary16 and stored in the workspace at g * 4096 halves.
 *   3. overlap-add. For sample t of signal r, f ascending over the frames that cover t, j = t + pad - f * hop, both sums from +0:
 *          num = sum fp32(w[j]) * fp32(v_g[j])      den = sum fp32(w[j]) * fp32(w[j])        (every product exact in fp32)
 *      y = fp16(num / den) where den > 0, the fp32 division correctly rounded; y = +0 where den = 0: samples no frame covers (the gaps
 *      of hop > 4096, a tail the last frame does not reach) and samples that lie only under zeros of the window. Whether the window
 *      and the hop satisfy a non-zero overlap-add condition is the caller's to choose; den = 0 is defined, not refused. With
 *      TFFT_ISTFT_RAW_SUM, y = fp16(num) everywhere.
 *
 * Output. Real binary16, signal r at out + r * out_sig_stride halves; a stride of 0 means L, otherwise it is a multiple of 8 that is
 * at least L. Every sample of [0, L) of every signal is written exactly once, and nothing else is written. Pointers are 16-byte
 * aligned. The extents (R F - 1) * in_frame_stride + 2049 and (R - 1) * out_sig_stride + L must stay below 2^62 halves.
 *
 * Workspace: R F * 4096 halves for the time-domain frames, by the rules of tfft_conv.h / tfft_bconv.h: _workspace_bytes,
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
#ifndef TFFT_ISTFT_H_
#define TFFT_ISTFT_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_ISTFT_API __attribute__((visibility("default")))
#else
#define TFFT_ISTFT_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_istft_plan tfft_istft_plan;

enum { TFFT_ISTFT_N = 4096, TFFT_ISTFT_BINS = 2049, TFFT_ISTFT_PITCH = 2056 };

/* tfft_istft_opts.flags */
enum { TFFT_ISTFT_RAW_SUM = 1 }; /* y = fp16(num): no division by the window envelope */

typedef struct tfft_istft_opts {
  uint32_t struct_size;     /* sizeof(tfft_istft_opts) as the caller was compiled (TFFT_ISTFT_OPTS_INIT sets it); the struct grows only
                               by appending fields. Any other value is refused (TFFT_ERR_ARG) */
  uint32_t reserved_;       /* must be 0 */
  uint64_t in_frame_stride; /* halves between consecutive frames of an input plane: 0 (= 2 * 2056) or a multiple of 8 that is >= 2049 */
  uint64_t out_sig_stride;  /* halves between consecutive signals of the output: 0 (= L) or a multiple of 8 that is >= L */
  uint32_t launch_iters;    /* launch shape of the frames kernel, as tfft_stft_opts.launch_iters: 0 = the library's default; k = 1 ..
                               65534: a wave takes about k items and retires; TFFT_LAUNCH_PERSISTENT: one workgroup per CU for all
                               items. Never changes results */
  int flags;                /* 0 or TFFT_ISTFT_RAW_SUM */
} tfft_istft_opts;
#define TFFT_ISTFT_OPTS_INIT {(uint32_t)sizeof(tfft_istft_opts)}

/* Host only: the frames per signal of a plan for `length`, `hop` and `pad`; the pointer may be NULL. TFFT_ERR_ARG for values that
 * tfft_istft_plan_create refuses. */
TFFT_ISTFT_API int tfft_istft_geometry(uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames);

/* opts: NULL (all defaults) or a tfft_istft_opts. TFFT_ERR_ARG for anything outside the shapes above, checked before the device is
 * touched; TFFT_ERR_DEVICE / TFFT_ERR_HIP as tfft_plan_create. The first call compares tfft_abi_version() of the libtfft.so it
 * runs against with the TFFT_ABI_VERSION it was built with. */
TFFT_ISTFT_API int tfft_istft_plan_create(uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id, const tfft_istft_opts* opts,
                                          tfft_istft_plan** out);
TFFT_ISTFT_API void tfft_istft_plan_destroy(tfft_istft_plan* plan);

/* Copies the 4096 binary16 window values at `window` (device memory) into a buffer the plan owns, ordered on `stream`, exactly as
 * tfft_stft_plan_set_window does. May be called again to replace the window. The plan's device must be current. tfft_istft_exec
 * before any set_window is TFFT_ERR_ARG. */
TFFT_ISTFT_API int tfft_istft_plan_set_window(tfft_istft_plan* plan, const void* window, void* stream);

/* Bytes of workspace one execution needs (R F * 4096 halves; 0 for NULL). */
TFFT_ISTFT_API size_t tfft_istft_plan_workspace_bytes(const tfft_istft_plan* plan);
/* Hands in a caller-owned workspace of at least that many bytes, 256-byte aligned (TFFT_ERR_WORKSPACE when too small); NULL returns to
 * a workspace of the plan's own. Not while an execution is in flight. */
TFFT_ISTFT_API int tfft_istft_plan_set_workspace(tfft_istft_plan* plan, void* device_ptr, size_t bytes);
/* Allocates the plan's own workspace now unless one is settled: every later execution only launches. */
TFFT_ISTFT_API int tfft_istft_plan_prepare(tfft_istft_plan* plan);

/* Enqueues both kernels on `stream` (NULL = default stream); does not synchronise. The plan's device must be current. A refused call
 * launches nothing. */
TFFT_ISTFT_API int tfft_istft_exec(const tfft_istft_plan* plan, const void* in_re, const void* in_im, void* out, void* stream);

/* Kernel launches of one execution (2; 0 for NULL), and their names one per line in launch order ("istft4096::frames_kernel",
 * "istft4096::ola_kernel"). _kernels returns the number of lines, or TFFT_ERR_ARG when `bytes` is too small. */
TFFT_ISTFT_API int tfft_istft_plan_num_launches(const tfft_istft_plan* plan);
TFFT_ISTFT_API int tfft_istft_plan_kernels(const tfft_istft_plan* plan, char* buf, size_t bytes);

/* Host only: what tfft_istft_plan_create would build, as text: "istft4096:4096 x F + ola", F the frames per signal. Refuses what
 * tfft_istft_plan_create refuses on the same shape and flags. */
TFFT_ISTFT_API int tfft_istft_describe(uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes);

/* Message of the last failure of a tfft_istft_* call on this thread ("" if none). */
TFFT_ISTFT_API const char* tfft_istft_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_ISTFT_H_ */
