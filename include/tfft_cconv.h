/* tfft_cconv.h — C ABI of the carried convolution add-on (libtfft_cconv.so) of the MI355X (gfx950) tensor-core FFT library: the
 * overlap-save causal convolution of tfft_sconv.h and its two gradients of tfft_bconv.h on a CHUNK of a longer sequence, with the
 * context a chunk needs from its neighbours read in place: no [history | x] copy, no slice of the result.
 *
 * A chunk is `rows` x `channels` REAL sequences of `length` L samples. Let xe be the input extended by its history of Hn samples
 * and ge the gradient g = d loss / d y extended by its future of Fn samples (Hn, Fn multiples of 8, 0 .. halo):
 *
 *     xe[t] = x[t]          0 <= t < L              ge[t] = g[t]          0 <= t < L
 *     xe[t] = hist[Hn + t]  -Hn <= t < 0            ge[t] = fut[t - L]    L <= t < L + Fn
 *     xe[t] = 0             elsewhere               ge[t] = 0             elsewhere
 *
 *     y[b][c][t]  = sum over j < K of  h[c][j] * xe[b][c][t - j]                     t = 0 .. L - 1    (forward plan)
 *     dx[b][c][t] = sum over j < K of  h[c][j] * ge[b][c][t + j]                     t = 0 .. L - 1    (gradient plan)
 *     dh[c][j]    = sum over b, 0 <= t < L of  g[b][c][t] * xe[b][c][t - j]          j = 0 .. K - 1, fp32
 *
 * The three uses: streaming or chunked inference (the history is the end of the previous chunk), chunked training, and sequence
 * parallel training (a rank receives K - 1 samples of x from the rank before it and K - 1 samples of g from the rank after it).
 * A context shorter than K - 1 is legal: it describes a stream that began Hn samples ago. A NULL context reads as zeros.
 *
 * Everything else is tfft_sconv.h and tfft_bconv.h, entry for entry: the shapes (L a multiple of 8, 8 .. 2^26; 1 <= K <= 2049),
 * the geometry (halo = K - 1 rounded up to a multiple of 64, hop = 4096 - halo, S = ceil(L / hop) segments; the context does not
 * change it), the pairing of rows 2p and 2p + 1, the item order, the spectrum (tfft_lconv_spectrum_host at n = 4096, rounded
 * once), the range contract per window, strides and alignment, the workspace and the summation order of the tap gradient. Only
 * segment 0 of the forward and tap-gradient windows can reach in front of sample 0, and only the last windows of the input
 * gradient reach behind sample L; the kernels (cconv4096::cconv4096_kernel, dgrad_kernel, wgrad_kernel, wreduce_kernel) are the
 * shipped ones with those load ends re-indexed. The add-on links libtfft_conv.so and libtfft.so only.
 *
 * carry_min = K - 1 rounded up to a multiple of 8 is the smallest context that loses nothing (tfft_cconv_geometry reports it).
 *   - With Hn = halo (and Fn = halo), a chunk that starts at a multiple of hop of the whole sequence transforms exactly the windows
 *     the whole-sequence plan transforms: y and dx have the BITS of tfft_sconv_exec and tfft_bconv_exec_input_grad on the whole
 *     sequence.
 *   - With a shorter context (carry_min <= Hn < halo), or a chunk that starts elsewhere, the windows differ from the whole-sequence
 *     plan's, so the results are the same values only within the accuracy bound of those plans, not bit for bit.
 *
 * Context layout. The history of sequence (b, c) is at hist + (b * channels + c) * hist_seq_stride halves, Hn samples; a stride
 * of 0 means Hn, otherwise it is a multiple of 8 and >= Hn. The same for the future with fut_seq_stride and Fn. Pointers are
 * 16-byte aligned. Nothing outside [0, L) of a sequence and [0, Hn) or [0, Fn) of a context is ever read; contexts are never
 * written.
 *
 * Aliasing. An output (out, dx, dh, the workspace) must not share a half with any input or context (TFFT_ERR_ARG, nothing is
 * launched). Inputs and contexts may alias each other freely: the normal zero-copy call passes hist = in - Hn with
 * hist_seq_stride = in_seq_stride, a view into the previous chunk of one long buffer, and fut = g + L likewise.
 */
#ifndef TFFT_CCONV_H_
#define TFFT_CCONV_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_CCONV_API __attribute__((visibility("default")))
#else
#define TFFT_CCONV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_cconv_plan tfft_cconv_plan;
typedef struct tfft_cconv_grad tfft_cconv_grad;

enum { TFFT_CCONV_MAX_TAPS = 2049 };

/* tfft_sconv_opts with the history appended */
typedef struct tfft_cconv_opts {
  uint32_t struct_size;     /* sizeof(tfft_cconv_opts) as the caller was compiled (TFFT_CCONV_OPTS_INIT sets it); the struct grows only
                               by appending fields. Any other value is refused (TFFT_ERR_ARG) */
  uint32_t reserved_;       /* must be 0 */
  uint64_t in_seq_stride;   /* halves between consecutive sequences of the input: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t out_seq_stride;  /* the same for the output */
  uint32_t launch_iters;    /* launch shape, as tfft_sconv_opts.launch_iters. Never changes results */
  int flags;                /* no flag is defined yet: must be 0 */
  uint64_t history;         /* Hn, the samples of history per sequence: a multiple of 8, 0 .. halo */
  uint64_t hist_seq_stride; /* halves between consecutive histories: 0 (= Hn) or a multiple of 8 that is >= Hn */
} tfft_cconv_opts;
#define TFFT_CCONV_OPTS_INIT {(uint32_t)sizeof(tfft_cconv_opts)}

/* tfft_bconv_opts with the history (of x, for the tap gradient) and the future (of g, for the input gradient) appended */
typedef struct tfft_cconv_grad_opts {
  uint32_t struct_size;     /* sizeof(tfft_cconv_grad_opts) (TFFT_CCONV_GRAD_OPTS_INIT sets it); any other value is refused */
  uint32_t reserved_;       /* must be 0 */
  uint64_t x_seq_stride;    /* halves between consecutive sequences of x: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t g_seq_stride;    /* the same for g */
  uint64_t dx_seq_stride;   /* the same for dx */
  uint32_t launch_iters;    /* launch shape of the input gradient, as tfft_sconv_opts.launch_iters. Never changes results */
  uint32_t partials;        /* cap on P, the partial sums per channel of the tap gradient; 0 = the default (tfft_bconv.h) */
  int flags;                /* no flag is defined yet: must be 0 */
  uint64_t history;         /* Hn of the x of the tap gradient: a multiple of 8, 0 .. halo */
  uint64_t hist_seq_stride; /* 0 (= Hn) or a multiple of 8 that is >= Hn */
  uint64_t future;          /* Fn of the g of the input gradient: a multiple of 8, 0 .. halo */
  uint64_t fut_seq_stride;  /* 0 (= Fn) or a multiple of 8 that is >= Fn */
} tfft_cconv_grad_opts;
#define TFFT_CCONV_GRAD_OPTS_INIT {(uint32_t)sizeof(tfft_cconv_grad_opts)}

/* ---- the forward plan: tfft_sconv.h entry for entry ---- */

/* Host only: halo, hop and segments of tfft_sconv_geometry, and *carry_min = K - 1 rounded up to a multiple of 8. Each pointer
 * may be NULL. TFFT_ERR_ARG for a length or a number of taps that tfft_cconv_plan_create refuses. */
TFFT_CCONV_API int tfft_cconv_geometry(uint64_t length, uint64_t taps, uint64_t* halo, uint64_t* hop, uint64_t* segments,
                                       uint64_t* carry_min);

/* The shapes, refusals and messages of tfft_sconv_plan_create; besides, TFFT_ERR_ARG for a history that is not a multiple of 8 or
 * exceeds halo, and for a hist_seq_stride that is neither 0 nor a multiple of 8 that is >= history. All checked before the device
 * is touched. */
TFFT_CCONV_API int tfft_cconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                          const tfft_cconv_opts* opts, tfft_cconv_plan** out);
TFFT_CCONV_API void tfft_cconv_plan_destroy(tfft_cconv_plan* plan);

/* tfft_sconv_plan_set_taps and tfft_sconv_plan_spectrum. */
TFFT_CCONV_API int tfft_cconv_plan_set_taps(tfft_cconv_plan* plan, const void* taps, void* stream);
TFFT_CCONV_API int tfft_cconv_plan_spectrum(const tfft_cconv_plan* plan, void* h_re, void* h_im);

/* tfft_sconv_exec with the history. hist = NULL reads as zeros (the first chunk of a stream) and is always legal; a plan created
 * with history = 0 takes only NULL. The output must not share a half with the input or the history; the input and the history may
 * overlap (hist = in - Hn). A refused call launches nothing. */
TFFT_CCONV_API int tfft_cconv_exec(const tfft_cconv_plan* plan, const void* in, const void* hist, void* out, void* stream);

/* Kernel launches of one execution (1; 0 for NULL), and their names one per line ("cconv4096::cconv4096_kernel"). */
TFFT_CCONV_API int tfft_cconv_plan_num_launches(const tfft_cconv_plan* plan);
TFFT_CCONV_API int tfft_cconv_plan_kernels(const tfft_cconv_plan* plan, char* buf, size_t bytes);

/* Host only: "cconv4096:4096 x S", S the segments per sequence. Refuses what tfft_cconv_plan_create refuses on the same shape. */
TFFT_CCONV_API int tfft_cconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes);

/* ---- the gradient plan: tfft_bconv.h entry for entry ---- */

/* Host only: tfft_bconv_geometry, and *carry_min as above. Each of the five pointers may be NULL. */
TFFT_CCONV_API int tfft_cconv_grad_geometry(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials,
                                            uint64_t* halo, uint64_t* hop, uint64_t* segments, uint64_t* partials_out, uint64_t* carry_min);

/* The shapes, refusals and messages of tfft_bconv_plan_create, and those of tfft_cconv_plan_create for history / hist_seq_stride
 * and future / fut_seq_stride. */
TFFT_CCONV_API int tfft_cconv_grad_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                          const tfft_cconv_grad_opts* opts, tfft_cconv_grad** out);
TFFT_CCONV_API void tfft_cconv_grad_destroy(tfft_cconv_grad* plan);

/* tfft_bconv_plan_set_taps (only the input gradient needs taps) and tfft_bconv_plan_spectrum (H, not conjugated). */
TFFT_CCONV_API int tfft_cconv_grad_set_taps(tfft_cconv_grad* plan, const void* taps, void* stream);
TFFT_CCONV_API int tfft_cconv_grad_spectrum(const tfft_cconv_grad* plan, void* h_re, void* h_im);

/* The workspace of the tap gradient, channels * P * Kpad * 4 bytes, under the rules of tfft_bconv.h. */
TFFT_CCONV_API size_t tfft_cconv_grad_workspace_bytes(const tfft_cconv_grad* plan);
TFFT_CCONV_API int tfft_cconv_grad_set_workspace(tfft_cconv_grad* plan, void* device_ptr, size_t bytes);
TFFT_CCONV_API int tfft_cconv_grad_prepare(tfft_cconv_grad* plan);

/* dx from g and the Fn samples behind it. g_future = NULL reads as zeros (the last chunk) and is always legal; a plan created with
 * future = 0 takes only NULL. dx must not share a half with g or the future. */
TFFT_CCONV_API int tfft_cconv_grad_exec_input_grad(const tfft_cconv_grad* plan, const void* g, const void* g_future, void* dx, void* stream);

/* dh ([channels][taps] fp32) from x, the Hn samples in front of it, and g: cconv4096::wgrad_kernel, then cconv4096::wreduce_kernel.
 * x_hist = NULL reads as zeros; a plan created with history = 0 takes only NULL. dh and the workspace must not overlap x, x_hist,
 * g or each other. */
TFFT_CCONV_API int tfft_cconv_grad_exec_tap_grad(const tfft_cconv_grad* plan, const void* x, const void* x_hist, const void* g, void* dh,
                                                 void* stream);

/* Kernel launches of the plan (3; 0 for NULL) and their names one per line: "cconv4096::dgrad_kernel", "cconv4096::wgrad_kernel",
 * "cconv4096::wreduce_kernel". */
TFFT_CCONV_API int tfft_cconv_grad_num_launches(const tfft_cconv_grad* plan);
TFFT_CCONV_API int tfft_cconv_grad_kernels(const tfft_cconv_grad* plan, char* buf, size_t bytes);

/* Host only: "cconv4096:4096 x S | partials P". Refuses what tfft_cconv_grad_create refuses on the same shape and flags. */
TFFT_CCONV_API int tfft_cconv_grad_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, int flags,
                                            char* buf, size_t bytes);

/* Message of the last failure of a tfft_cconv_* call on this thread ("" if none). */
TFFT_CCONV_API const char* tfft_cconv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_CCONV_H_ */
