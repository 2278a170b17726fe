/* tfft_gcconv.h — C ABI of the gated carried convolution add-on (libtfft_gcconv.so) of the MI355X (gfx950) tensor-core FFT library:
 * the GATED overlap-save causal convolution of tfft_gsconv.h and its gradients of tfft_gbconv.h on a CHUNK of a longer sequence,
 * with the context a chunk needs from its neighbours read in place, as tfft_cconv.h reads it for the ungated operator: gates and
 * context in one pass, no [history | x] copy, no product in a separate pass, no slice of the result.
 *
 * A chunk is `rows` x `channels` REAL sequences of `length` L samples, with `taps` K real taps h[c] and an optional skip weight d[c]
 * per channel (h' = h with d[c] added to tap 0) and the optional gates pre and post. Let
 *
 *     xe  = x    extended by Hn samples of `history`          pe = pre  extended by Hn samples of `pre_history`
 *     gye = gy   extended by Fn samples of `future`           qe = post extended by Fn samples of `post_future`
 *
 * each extension zero outside its stated range (Hn, Fn multiples of 8, 0 .. halo), as tfft_cconv.h defines xe and ge, and
 * ue = pe * xe, gze = qe * gye, gz = post * gy (a plan without a gate takes that gate as 1). For t = 0 .. L - 1:
 *
 *     y[b][c][t]    = post[b][c][t] * sum over j < K of  h'[c][j] * ue[b][c][t - j]                  (forward plan)
 *     du[b][c][t]   = sum over j < K of  h'[c][j] * gze[b][c][t + j]                                 (gradient plan)
 *     dx[b][c][t]   = pre[b][c][t] * du[b][c][t]           dpre[b][c][t] = x[b][c][t] * du[b][c][t]  (dpre only with a pre gate)
 *     dh[c][j]      = sum over b, 0 <= t < L of  gz[b][c][t] * ue[b][c][t - j]                       j = 0 .. K - 1, fp32
 *     dskip[c]      = dh[c][0]
 *
 * The gradient of the post gate, dpost = gy * z, is the FORWARD plan executed with gy handed in as its post gate, as in
 * tfft_gbconv.h; it needs no entry point of its own.
 *
 * Everything else is tfft_gsconv.h, tfft_gbconv.h and tfft_cconv.h, entry for entry: the shapes (L a multiple of 8, 8 .. 2^26;
 * 1 <= K <= 2049), the geometry (halo = K - 1 rounded up to a multiple of 64, hop = 4096 - halo, S = ceil(L / hop) segments),
 * carry_min = K - 1 rounded up to a multiple of 8, the pairing of rows 2p and 2p + 1, the item order, the spectrum H' (the skip folded
 * into tap 0 in fp64, rounded once), the partial sums P and the summation order of the tap gradient, the workspace rules and the range
 * contract per window. The context changes none of them. Every gate product is ONE IEEE binary16 multiply. The kernels
 * (gcconv4096::fwd_kernel<Pre, Post>, dgrad_kernel<Pre, Post>, wgrad_kernel<Pre, Post>, wreduce_kernel) are the shipped gated ones
 * with their load ends re-indexed: every window of a carried plan is a window of a shipped gated plan on the concatenated sequence,
 * so with Hn = halo (Fn = halo) on hop-aligned chunks y, dx and dpre have the BITS of tfft_gsconv_exec and
 * tfft_gbconv_exec_input_grad on the whole sequence, and a plan without gates and skip has the bits of tfft_cconv.h's plans.
 *
 * Contexts. One Hn serves x and the pre gate, one Fn serves gy and the post gate. Each context has its own pointer and its own
 * sequence stride (0 means Hn or Fn, otherwise a multiple of 8 that is >= Hn or Fn). A gate's context pointer is non-NULL exactly
 * when the sequence's context pointer is non-NULL and the plan has that gate; anything else is TFFT_ERR_ARG and nothing is launched.
 * NULL contexts read as zeros. A context shorter than K - 1 is legal. Pointers are 16-byte aligned. Nothing outside [0, L) of a
 * sequence or gate and [0, Hn) or [0, Fn) of a context is ever read; contexts are never written.
 *
 * Gates are fixed per plan by TFFT_GCCONV_PRE_GATE / TFFT_GCCONV_POST_GATE; which gate pointers are NULL follows tfft_gsconv.h and
 * tfft_gbconv.h.
 *
 * Aliasing: as in tfft_cconv.h. An output (out, dx, dpre, dh, dskip, the workspace) must not share a half with any input, gate or
 * context, or with another output (TFFT_ERR_ARG, nothing is launched). Inputs, gates and contexts may alias each other freely:
 * hist = in - Hn and pre_hist = pre - Hn with the buffers' own strides is the normal zero-copy call.
 *
 * The add-on links libtfft_conv.so and libtfft.so only.
 */
#ifndef TFFT_GCCONV_H_
#define TFFT_GCCONV_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_GCCONV_API __attribute__((visibility("default")))
#else
#define TFFT_GCCONV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_gcconv_plan tfft_gcconv_plan;
typedef struct tfft_gcconv_grad tfft_gcconv_grad;

enum { TFFT_GCCONV_MAX_TAPS = 2049 };

/* flags of the option structs and of the _describe calls; any other bit is refused */
enum {
  TFFT_GCCONV_PRE_GATE = 1,  /* the operator multiplies the input by a gate before the convolution */
  TFFT_GCCONV_POST_GATE = 2  /* the operator multiplies the result by a gate */
};

/* tfft_gsconv_opts with the context fields appended */
typedef struct tfft_gcconv_opts {
  uint32_t struct_size;         /* sizeof(tfft_gcconv_opts) as the caller was compiled (TFFT_GCCONV_OPTS_INIT sets it); the struct
                                   grows only by appending fields. Any other value is refused (TFFT_ERR_ARG) */
  uint32_t reserved_;           /* must be 0 */
  uint64_t in_seq_stride;       /* halves between consecutive sequences of the input: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t out_seq_stride;      /* the same for the output */
  uint64_t pre_seq_stride;      /* the same for the pre gate (checked whether or not the plan has that gate) */
  uint64_t post_seq_stride;     /* the same for the post gate */
  uint32_t launch_iters;        /* launch shape, as tfft_sconv_opts.launch_iters. Never changes results */
  int flags;                    /* TFFT_GCCONV_* */
  uint64_t history;             /* Hn, the samples of context per sequence in front of x AND of the pre gate: a multiple of 8, 0 .. halo */
  uint64_t hist_seq_stride;     /* halves between consecutive histories of x: 0 (= Hn) or a multiple of 8 that is >= Hn */
  uint64_t pre_hist_seq_stride; /* the same for the histories of the pre gate */
} tfft_gcconv_opts;             /* 72 bytes */
#define TFFT_GCCONV_OPTS_INIT {(uint32_t)sizeof(tfft_gcconv_opts)}

/* tfft_gbconv_opts with the context fields appended */
typedef struct tfft_gcconv_grad_opts {
  uint32_t struct_size;         /* sizeof(tfft_gcconv_grad_opts) (TFFT_GCCONV_GRAD_OPTS_INIT sets it); any other value is refused */
  uint32_t reserved_;           /* must be 0 */
  uint64_t x_seq_stride;        /* halves between consecutive sequences of x: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t pre_seq_stride;      /* the same for the pre gate (checked whether or not the plan has that gate) */
  uint64_t gy_seq_stride;       /* the same for gy */
  uint64_t post_seq_stride;     /* the same for the post gate */
  uint64_t dx_seq_stride;       /* the same for dx */
  uint64_t dpre_seq_stride;     /* the same for dpre */
  uint32_t launch_iters;        /* launch shape of the input gradient, as tfft_sconv_opts.launch_iters. Never changes results */
  uint32_t partials;            /* cap on P, the partial sums per channel of the tap gradient; 0 = the default (tfft_gbconv.h) */
  int flags;                    /* TFFT_GCCONV_* */
  uint64_t history;             /* Hn of x and the pre gate in the tap gradient: a multiple of 8, 0 .. halo */
  uint64_t hist_seq_stride;     /* 0 (= Hn) or a multiple of 8 that is >= Hn */
  uint64_t pre_hist_seq_stride; /* the same for the histories of the pre gate */
  uint64_t future;              /* Fn of gy and the post gate in the input gradient: a multiple of 8, 0 .. halo */
  uint64_t fut_seq_stride;      /* 0 (= Fn) or a multiple of 8 that is >= Fn */
  uint64_t post_fut_seq_stride; /* the same for the futures of the post gate */
} tfft_gcconv_grad_opts;        /* 120 bytes */
#define TFFT_GCCONV_GRAD_OPTS_INIT {(uint32_t)sizeof(tfft_gcconv_grad_opts)}

/* ---- the forward plan: tfft_gsconv.h entry for entry ---- */

/* Host only: halo, hop and segments of tfft_sconv_geometry, and *carry_min = K - 1 rounded up to a multiple of 8. Each pointer
 * may be NULL. TFFT_ERR_ARG for a length or a number of taps that tfft_gcconv_plan_create refuses. */
TFFT_GCCONV_API int tfft_gcconv_geometry(uint64_t length, uint64_t taps, uint64_t* halo, uint64_t* hop, uint64_t* segments,
                                         uint64_t* carry_min);

/* The shapes, refusals and messages of tfft_gsconv_plan_create; besides, TFFT_ERR_ARG for a history that is not a multiple of 8 or
 * exceeds halo, and for a hist_seq_stride / pre_hist_seq_stride that is neither 0 nor a multiple of 8 that is >= history. All
 * checked before the device is touched. */
TFFT_GCCONV_API int tfft_gcconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                            const tfft_gcconv_opts* opts, tfft_gcconv_plan** out);
TFFT_GCCONV_API void tfft_gcconv_plan_destroy(tfft_gcconv_plan* plan);

/* tfft_gsconv_plan_set_taps and tfft_gsconv_plan_spectrum. */
TFFT_GCCONV_API int tfft_gcconv_plan_set_taps(tfft_gcconv_plan* plan, const void* taps, const void* skip, void* stream);
TFFT_GCCONV_API int tfft_gcconv_plan_spectrum(const tfft_gcconv_plan* plan, void* h_re, void* h_im);

/* tfft_gsconv_exec with the contexts. hist = NULL reads as zeros (the first chunk of a stream) and is always legal; a plan created
 * with history = 0 takes only NULL. pre_hist is non-NULL exactly when hist is non-NULL and the plan has a pre gate. The output must
 * not share a half with the input, a gate or a context; those may overlap each other (hist = in - Hn, pre_hist = pre - Hn). A
 * refused call launches nothing. */
TFFT_GCCONV_API int tfft_gcconv_exec(const tfft_gcconv_plan* plan, const void* in, const void* pre, const void* post, const void* hist,
                                     const void* pre_hist, void* out, void* stream);

/* Kernel launches of one execution (1; 0 for NULL), and their names one per line: "gcconv4096::fwd_kernel<P, Q>" with P = "true"
 * for a plan with a pre gate and Q = "true" for one with a post gate, else "false". */
TFFT_GCCONV_API int tfft_gcconv_plan_num_launches(const tfft_gcconv_plan* plan);
TFFT_GCCONV_API int tfft_gcconv_plan_kernels(const tfft_gcconv_plan* plan, char* buf, size_t bytes);

/* Host only: "gcconv4096:4096 x S", "gcconv4096:4096:pre x S", "gcconv4096:4096:post x S" or "gcconv4096:4096:pre+post x S", S the
 * segments per sequence. Refuses what tfft_gcconv_plan_create refuses on the same shape and flags. */
TFFT_GCCONV_API int tfft_gcconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes);

/* ---- the gradient plan: tfft_gbconv.h entry for entry ---- */

/* Host only: tfft_gbconv_geometry, and *carry_min as above. Each of the five pointers may be NULL. */
TFFT_GCCONV_API int tfft_gcconv_grad_geometry(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials,
                                              uint64_t* halo, uint64_t* hop, uint64_t* segments, uint64_t* partials_out, uint64_t* carry_min);

/* The shapes, refusals and messages of tfft_gbconv_plan_create, and those of tfft_gcconv_plan_create for history and future and
 * their four strides. */
TFFT_GCCONV_API int tfft_gcconv_grad_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                            const tfft_gcconv_grad_opts* opts, tfft_gcconv_grad** out);
TFFT_GCCONV_API void tfft_gcconv_grad_destroy(tfft_gcconv_grad* plan);

/* tfft_gbconv_plan_set_taps (only the input gradient needs taps) and tfft_gbconv_plan_spectrum (H', not conjugated). */
TFFT_GCCONV_API int tfft_gcconv_grad_set_taps(tfft_gcconv_grad* plan, const void* taps, const void* skip, void* stream);
TFFT_GCCONV_API int tfft_gcconv_grad_spectrum(const tfft_gcconv_grad* plan, void* h_re, void* h_im);

/* The workspace of the tap gradient, channels * P * Kpad * 4 bytes, under the rules of tfft_gbconv.h. */
TFFT_GCCONV_API size_t tfft_gcconv_grad_workspace_bytes(const tfft_gcconv_grad* plan);
TFFT_GCCONV_API int tfft_gcconv_grad_set_workspace(tfft_gcconv_grad* plan, void* device_ptr, size_t bytes);
TFFT_GCCONV_API int tfft_gcconv_grad_prepare(tfft_gcconv_grad* plan);

/* tfft_gbconv_exec_input_grad with the Fn samples behind gy and behind the post gate. gy_future = NULL reads as zeros (the last
 * chunk) and is always legal; a plan created with future = 0 takes only NULL. post_future is non-NULL exactly when gy_future is
 * non-NULL and the plan has a post gate. dx and dpre must not share a half with an input, a gate, a context or each other. */
TFFT_GCCONV_API int tfft_gcconv_grad_exec_input_grad(const tfft_gcconv_grad* plan, const void* gy, const void* post, const void* gy_future,
                                                     const void* post_future, const void* x, const void* pre, void* dx, void* dpre,
                                                     void* stream);

/* tfft_gbconv_exec_tap_grad with the Hn samples in front of x and in front of the pre gate: gcconv4096::wgrad_kernel<Pre, Post>,
 * then gcconv4096::wreduce_kernel. x_hist = NULL reads as zeros; a plan created with history = 0 takes only NULL. pre_hist is
 * non-NULL exactly when x_hist is non-NULL and the plan has a pre gate. */
TFFT_GCCONV_API int tfft_gcconv_grad_exec_tap_grad(const tfft_gcconv_grad* plan, const void* x, const void* pre, const void* x_hist,
                                                   const void* pre_hist, const void* gy, const void* post, void* dh, void* dskip,
                                                   void* stream);

/* Kernel launches of the plan (3; 0 for NULL) and their names one per line: "gcconv4096::dgrad_kernel<P, Q>",
 * "gcconv4096::wgrad_kernel<P, Q>", "gcconv4096::wreduce_kernel". */
TFFT_GCCONV_API int tfft_gcconv_grad_num_launches(const tfft_gcconv_grad* plan);
TFFT_GCCONV_API int tfft_gcconv_grad_kernels(const tfft_gcconv_grad* plan, char* buf, size_t bytes);

/* Host only: "gcconv4096:4096[:gates] x S | partials P". Refuses what tfft_gcconv_grad_create refuses on the same shape and flags. */
TFFT_GCCONV_API int tfft_gcconv_grad_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, int flags,
                                              char* buf, size_t bytes);

/* Message of the last failure of a tfft_gcconv_* call on this thread ("" if none). */
TFFT_GCCONV_API const char* tfft_gcconv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_GCCONV_H_ */
