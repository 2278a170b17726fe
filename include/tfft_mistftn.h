/* tfft_mistftn.h — C ABI of the masked short-frame inverse STFT add-on (libtfft_mistftn.so) of the MI355X (gfx950) tensor-core FFT
 * library: the plans of tfft_istftn.h (frame lengths n = 512, 1024 and 2048) with a real binary16 mask on the half spectra, applied
 * inside the merge, in front of its single rounding: a ratio mask of an enhancement or separation network, an equaliser curve, a
 * gate. The same kernel is the adjoint of the short-frame STFT (a raw-sum plan with a fixed per-bin weight) and the gradient of the
 * power spectrogram (a raw-sum plan with a per-frame weight); tensor-fft_amd/stft_autograd.py builds both on it.
 *
 * Everything this header does not restate is word for word tfft_istftn.h's: the geometry (F = 1 + floor((L + 2 pad - n) / hop)
 * frames per signal, frame g = r * F + f), the shapes (n one of 512, 1024, 2048; 4096 is refused with a pointer to
 * tfft_istft_plan_create; L a multiple of 8, 8 .. 2^26; hop a multiple of 8 and >= 8; pad a multiple of 8 below n with L + 2 pad >= n;
 * R >= 1 and R F below 2^32), the input planes (frame g at in_re / in_im + g * in_frame_stride halves, 0 = 2 h with
 * h = tfft_rplan_spectrum_pitch(n) = 264, 520, 1032; bins 0 .. n / 2 read, the IM of bins 0 and n / 2 ignored, halves beyond bin
 * n / 2 never read), the pairing of frames 2b (A) and 2b + 1 (B) with a self-paired last frame of an odd total, the output (signal r
 * at out + r * out_sig_stride halves, every sample of [0, L) written exactly once and nothing else), the workspace (R F * n halves,
 * _workspace_bytes / _set_workspace (256-byte aligned) / _prepare or a lazy hipMalloc on the first execution), the legality of an
 * execution under stream capture once the workspace is settled, the 16-byte alignment of every data pointer and the rule that the
 * extents stay below 2^62 halves.
 *
 * The mask. Real binary16, 16-byte aligned. Per frame (the default): the mask of frame g at mask + g * mask_frame_stride halves;
 * a stride of 0 means h (264, 520, 1032), otherwise it is a multiple of 8 that is >= n / 2 + 1, and the extent
 * (R F - 1) * mask_frame_stride + n / 2 + 1 stays below 2^62 halves. With TFFT_MISTFTN_MASK_PER_BIN one mask of n / 2 + 1 halves
 * serves every frame, and mask_frame_stride must be 0. Bins 0 .. n / 2 of a mask frame are read; halves beyond bin n / 2 are never
 * read; the mask is never written.
 *
 * Arithmetic, which is the contract (tests hold it bit for bit). It is step 1 of tfft_istftn.h with the mask inside the fp32 sum. For
 * transform b with A = frame 2b, B = frame 2b + 1 and their masks mA, mB (per-bin mode: mA = mB; a self-paired last frame uses its own
 * mask for both):
 *
 *   1. masked merge with gain. For the low bins 0 < k < n / 2
 *          Z'r[k] = fp16(n * fp32(fp32(mA[k]) * fp32(A.re[k]) - fp32(mB[k]) * fp32(B.im[k])))
 *          Z'i[k] = fp16(n * fp32(fp32(mA[k]) * fp32(A.im[k]) + fp32(mB[k]) * fp32(B.re[k])))
 *      the high bins n / 2 < k < n follow from bin n - k with the signs of the unmasked merge,
 *          Z'r[k] = fp16(n * fp32(mA A.re + mB B.im))          Z'i[k] = fp16(n * fp32(mB B.re - mA A.im))      (all at bin n - k)
 *      and the edges, bins 0 and n / 2, are Z'r = fp16(n * mA A.re) and Z'i = fp16(n * mB B.re). A product of two binary16 values is
 *      exact in fp32 (22 significant bits, exponents far inside the range), so every sum above has ONE fp32 rounding whether or not a
 *      compiler contracts it into a fused multiply-add, and n is a power of two: the results do not depend on contraction.
 *      INPUT CONDITION: |n (mA A[k] + i mB B[k])| <= 64512 for every bin, tfft_istftn.h's condition on the masked spectra. Beyond it
 *      the result may hold inf / nan; nothing is refused. Subnormals are kept everywhere, in the mask too.
 *   2. inverse transform and 3. overlap-add: tfft_istftn.h's, unchanged (tfft_exec_inverse of the default plan of n on Z'; the
 *      fixed-order overlap-add with y = fp16(num / den), +0 where den = 0, and y = fp16(num) with TFFT_MISTFTN_RAW_SUM).
 *
 * Consequences (tests hold them): a mask of all 1.0 gives the bits of libtfft_istftn.so; a mask of +-1, +-2 or 0 gives the bits of
 * libtfft_istftn.so on the planes multiplied by it beforehand, where the doubling does not overflow binary16.
 *
 * Aliasing. The output's extent and the workspace must not meet the inputs' extents, the mask's extent or each other; anything
 * else is refused (TFFT_ERR_ARG) and nothing is launched. The mask may alias the spectra: all three are only read. The window is
 * copied into the plan.
 *
 * The add-on is layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): it links against both, never
 * against a sibling add-on, and uses their status codes (TFFT_OK, TFFT_ERR_*) and conventions. Only plain pointers and sizes cross
 * this boundary: device pointers are raw HIP device addresses, `stream` is a hipStream_t passed as void*.
 */
#ifndef TFFT_MISTFTN_H_
#define TFFT_MISTFTN_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_MISTFTN_API __attribute__((visibility("default")))
#else
#define TFFT_MISTFTN_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_mistftn_plan tfft_mistftn_plan;

/* tfft_mistftn_opts.flags */
enum {
  TFFT_MISTFTN_RAW_SUM = 1,     /* y = fp16(num): no division by the window envelope */
  TFFT_MISTFTN_MASK_PER_BIN = 2 /* one mask of n / 2 + 1 halves for every frame; mask_frame_stride must be 0 */
};

typedef struct tfft_mistftn_opts {
  uint32_t struct_size;       /* sizeof(tfft_mistftn_opts) as the caller was compiled (TFFT_MISTFTN_OPTS_INIT sets it); the struct grows
                                 only by appending fields. Any other value is refused (TFFT_ERR_ARG) */
  uint32_t reserved_;         /* must be 0 */
  uint64_t in_frame_stride;   /* halves between consecutive frames of an input plane: 0 (= 2 h) or a multiple of 8 that is >= n / 2 + 1 */
  uint64_t out_sig_stride;    /* halves between consecutive signals of the output: 0 (= L) or a multiple of 8 that is >= L */
  uint32_t launch_iters;      /* launch shape of the frames kernel, as tfft_istftn_opts.launch_iters. Never changes results */
  int flags;                  /* 0 or a combination of TFFT_MISTFTN_RAW_SUM and TFFT_MISTFTN_MASK_PER_BIN */
  uint64_t mask_frame_stride; /* halves between consecutive frames of the mask: 0 (= h) or a multiple of 8 that is >= n / 2 + 1; 0 with
                                 TFFT_MISTFTN_MASK_PER_BIN */
} tfft_mistftn_opts;
#define TFFT_MISTFTN_OPTS_INIT {(uint32_t)sizeof(tfft_mistftn_opts)}

/* Host only: the frames per signal of a plan for `n`, `length`, `hop` and `pad`; the pointer may be NULL. TFFT_ERR_ARG for values
 * that tfft_mistftn_plan_create refuses. */
TFFT_MISTFTN_API int tfft_mistftn_geometry(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t* frames);

/* opts: NULL (all defaults: a per-frame mask at stride h) or a tfft_mistftn_opts. TFFT_ERR_ARG for anything outside the shapes above,
 * checked before the device is touched; TFFT_ERR_DEVICE / TFFT_ERR_HIP as tfft_plan_create. The first call compares
 * tfft_abi_version() of the libtfft.so it runs against with the TFFT_ABI_VERSION it was built with. */
TFFT_MISTFTN_API int tfft_mistftn_plan_create(uint32_t n, uint64_t rows, uint64_t length, uint64_t hop, uint64_t pad, int device_id,
                                              const tfft_mistftn_opts* opts, tfft_mistftn_plan** out);
TFFT_MISTFTN_API void tfft_mistftn_plan_destroy(tfft_mistftn_plan* plan);

/* Copies the n binary16 window values at `window` (device memory) into a buffer the plan owns, ordered on `stream`, exactly as
 * tfft_istftn_plan_set_window does. May be called again to replace the window. The plan's device must be current.
 * tfft_mistftn_exec before any set_window is TFFT_ERR_ARG. */
TFFT_MISTFTN_API int tfft_mistftn_plan_set_window(tfft_mistftn_plan* plan, const void* window, void* stream);

/* Bytes of workspace one execution needs (R F * n halves; 0 for NULL). */
TFFT_MISTFTN_API size_t tfft_mistftn_plan_workspace_bytes(const tfft_mistftn_plan* plan);
/* Hands in a caller-owned workspace of at least that many bytes, 256-byte aligned (TFFT_ERR_WORKSPACE when too small); NULL returns to
 * a workspace of the plan's own. Not while an execution is in flight. */
TFFT_MISTFTN_API int tfft_mistftn_plan_set_workspace(tfft_mistftn_plan* plan, void* device_ptr, size_t bytes);
/* Allocates the plan's own workspace now unless one is settled: every later execution only launches. */
TFFT_MISTFTN_API int tfft_mistftn_plan_prepare(tfft_mistftn_plan* plan);

/* Enqueues both kernels on `stream` (NULL = default stream); does not synchronise. The plan's device must be current. A refused call
 * launches nothing. */
TFFT_MISTFTN_API int tfft_mistftn_exec(const tfft_mistftn_plan* plan, const void* in_re, const void* in_im, const void* mask, void* out,
                                       void* stream);

/* Kernel launches of one execution (2; 0 for NULL), and their names one per line in launch order ("mistft256r::frames_kernel<R>",
 * R = 2, 4 or 8, and "olan::ola_kernel"). _kernels returns the number of lines, or TFFT_ERR_ARG when `bytes` is too small. */
TFFT_MISTFTN_API int tfft_mistftn_plan_num_launches(const tfft_mistftn_plan* plan);
TFFT_MISTFTN_API int tfft_mistftn_plan_kernels(const tfft_mistftn_plan* plan, char* buf, size_t bytes);

/* Host only: what tfft_mistftn_plan_create would build, as text: "mistft256r<R>:n x F + ola" with R = n / 256 and F the frames per
 * signal, "mistft256r4:1024 x 13 + ola" for instance. Refuses what tfft_mistftn_plan_create refuses on the same shape and flags. */
TFFT_MISTFTN_API int tfft_mistftn_describe(uint32_t n, uint64_t length, uint64_t hop, uint64_t pad, uint64_t rows, int flags, char* buf, size_t bytes);

/* Message of the last failure of a tfft_mistftn_* call on this thread ("" if none). */
TFFT_MISTFTN_API const char* tfft_mistftn_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_MISTFTN_H_ */
