/* tfft_gbconv.h — C ABI of the gated gradient add-on (libtfft_gbconv.so) of the MI355X (gfx950) tensor-core FFT library: the
 * gradients of the gated overlap-save causal convolution of tfft_gsconv.h, so that the operator can be trained through.
 *
 * The forward pass takes `rows` x `channels` REAL sequences of `length` L samples, `taps` K real taps h[c] and an optional skip
 * weight d[c] per channel, and the optional gates pre and post:
 *
 *     u[b][c][t] = pre[b][c][t] * x[b][c][t]                                         (u = x without a pre gate)
 *     z[b][c][t] = sum over j <= t, j < K of  h'[c][j] * u[b][c][t - j]              h' = h with d[c] added to tap 0
 *     y[b][c][t] = post[b][c][t] * z[b][c][t]                                        (y = z without a post gate)
 *
 * With gy = d loss / d y, a gated gradient plan computes
 *
 *     gz[b][c][t]   = post[b][c][t] * gy[b][c][t]                                    (gz = gy without a post gate)
 *     du[b][c][t]   = sum over j < K, t + j < L  of  h'[c][j] * gz[b][c][t + j]
 *     dx[b][c][t]   = pre[b][c][t] * du[b][c][t]                                     (dx = du without a pre gate)
 *     dpre[b][c][t] = x[b][c][t] * du[b][c][t]                                       (only with a pre gate)
 *     dh[c][j]      = sum over b, t >= j, t < L  of  gz[b][c][t] * u[b][c][t - j]    (j = 0 .. K - 1, fp32)
 *     dskip[c]      = dh[c][0]                                                       (h'[0] = h[0] + d)
 *
 * The gradient of the post gate, dpost = gy * z, is the FORWARD plan of tfft_gsconv.h executed with gy handed in as its post gate;
 * it needs no plan of this add-on.
 *
 * The add-on is layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): it links against both and uses
 * their status codes (TFFT_OK, TFFT_ERR_*) and conventions. It uses none of the other add-ons. Only plain pointers and sizes cross
 * this boundary: device pointers are raw HIP device addresses, `stream` is a hipStream_t passed as void*.
 *
 * Shapes: those of tfft_gsconv_plan_create. L a multiple of 8 and >= 8, at most 2^26; rows B >= 1, channels C >= 1, B C and the
 * item count below 2^32; 1 <= K <= 2049 (a longer filter is refused with the message of tfft_gsconv_plan_create).
 *
 * Method: overlap-save at transform length 4096 on the geometry of tfft_sconv_geometry (halo = K - 1 rounded up to a multiple of
 * 64, hop = 4096 - halo, segments S = ceil(L / hop)). Nothing outside [0, L) of any sequence or gate is ever read.
 *
 *   input gradient  Segment s is the 4096-sample window of gz that starts at sample s * hop (no front halo), zero at or beyond
 *                   sample L. The post gate is applied on the way into the window, indexed by the SOURCE sample: a segment
 *                   re-reads the gate beyond its hop just as it re-reads gy. The window is multiplied by conj(H'), H' the
 *                   skip-carrying filter spectrum of tfft_gsconv.h, by the arithmetic of sconv4096_kernel; window samples
 *                   [0, min(hop, L - s * hop)) are du[s * hop ...], are multiplied by the pre gate (and by x, for dpre) at the
 *                   OUTPUT sample and written there. One kernel, gbconv4096::dgrad_kernel<Pre, Post>, no workspace.
 *   tap gradient    Item (p, s) of channel c: Zu is the complex window of the u pair as the forward plan loads it (it starts at
 *                   s * hop - halo; the pre gate indexed by the source sample), Zg the same window of the gz pair (the post gate
 *                   indexed by the source sample) with its first `halo` samples forced to zero (they belong to segment s - 1). The
 *                   rest is tfft_bconv.h's: gbconv4096::wgrad_kernel<Pre, Post> keeps conj(fft(Zu) / 4096), rounded to binary16, in
 *                   registers as the filter of sconv4096_kernel's two passes over Zg and adds lags 0 .. K - 1 of the RE plane in
 *                   fp32; gbconv4096::wreduce_kernel sums the partial sums, multiplies by 4096 (exact) and writes dh and dskip.
 *
 * Arithmetic. gz = post * gy and u = pre * x are ONE IEEE binary16 multiply per sample (round to nearest even, subnormals kept),
 * and so are dx = pre * du and dpre = x * du. Between them the statements are those of bconv4096's kernels: a plan without gates
 * gives tfft_bconv_exec_input_grad's and tfft_bconv_exec_tap_grad's bits (with a skip: for the skip-carrying spectrum).
 *
 * Summation order of the tap gradient: that of tfft_bconv.h. The items of a channel, i = p * S + s, are dealt to P partial sums:
 * partial q adds the items i = q, q + P, q + 2 P ... in increasing i, and dh is partial 0 + partial 1 + ... in increasing q, all in
 * fp32. P = min(items per channel, ceil(2048 / C)), capped by tfft_gbconv_opts.partials where that is not 0; tfft_gbconv_geometry
 * reports it. The order is fixed by P alone, never by the launch: no atomics, two executions give the same bits.
 *
 * Data contract: that of tfft_gsconv.h for x, pre, gy, post, dx and dpre, each with its own sequence stride (0 means L, otherwise a
 * multiple of 8 that is >= L); halves between sequences are never written. Pointers are 16-byte aligned. dh is [channels][taps]
 * fp32, dense, 4-byte aligned; dskip is [channels] fp32, 4-byte aligned, or NULL. Taps are [channels][taps] binary16 and the skip
 * weights [channels] binary16 on the device, or NULL (tfft_gbconv_plan_set_taps; the input gradient needs them, the tap gradient
 * does not). The spectrum is tfft_gsconv_plan_spectrum's, bit for bit, and the input gradient multiplies by its conjugate: the sign
 * bit of every non-zero imaginary part flipped, which is exact and keeps the planes exactly Hermitian.
 *
 * Gates are fixed per plan by TFFT_GBCONV_PRE_GATE / TFFT_GBCONV_POST_GATE. `post` is non-NULL exactly when the plan has a post
 * gate. For the input gradient `x` and `pre` are non-NULL exactly when the plan has a pre gate; `dpre` may be NULL on such a plan
 * (then only dx is written) and must be NULL on a plan without one. For the tap gradient `pre` is non-NULL exactly when the plan
 * has a pre gate. Anything else is refused (TFFT_ERR_ARG).
 *
 * Aliasing. Every output (dx, dpre, dh, dskip, the workspace) must be disjoint from every input of its call and from every other
 * output; ANY overlap is refused (TFFT_ERR_ARG), exact in-place execution included: segment s reads, beyond its hop, the first
 * samples of the stretch that segment s + 1 writes, and segments run in no defined order. Inputs may alias each other (x may be
 * pre, gy may be post). A refused call launches nothing.
 *
 * Pairing. Rows 2p and 2p + 1 of a channel are the RE and the IM plane of ONE complex transform, as in tfft_sconv.h. An odd number
 * of rows pairs its last row with zeros; that partner is neither loaded nor stored, and neither are its gates. Work item
 * (p * S + s) * channels + c of the input gradient is what a tfft_conv_plan with batch = items and filters = channels expects.
 *
 * Life cycle: that of tfft_bconv.h. The input gradient needs no workspace and only launches: it is legal under stream capture, and
 * executions may overlap in time. The tap gradient needs channels * P * Kpad * 4 bytes (Kpad = K rounded up to a multiple of 8)
 * for its partial sums, under the rules of tfft_conv.h: hand it in (tfft_gbconv_plan_set_workspace), let tfft_gbconv_plan_prepare
 * allocate it, or let the first execution do so; an execution never reallocates, and an execution of a prepared plan only launches
 * (legal under capture). Executions of ONE plan's tap gradient must not overlap in time: they share the partial sums.
 *
 * Range contract: that of tfft_bconv.h, per window, applied to the windows of gz and u and to H'. Input gradient: with G the
 * unscaled spectrum of a window of the gz pair, max_k |G_k| |H'_k| <= 32752, max |window's circular correlation| <= 65504, and
 * max |pre du|, max |x du| <= 65504. Tap gradient: max_k |G_k| |U_k| / 4096 <= 32752 and max |item's circular correlation| / 4096
 * <= 65504. Every pair that is transformed (gz in the input gradient, u and gz in the tap gradient: the gated values) has to meet
 * |v_2p + i v_2p+1| <= 64512 sample by sample (tfft_bconv.h; a row without partner: any finite value).
 */
#ifndef TFFT_GBCONV_H_
#define TFFT_GBCONV_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_GBCONV_API __attribute__((visibility("default")))
#else
#define TFFT_GBCONV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_gbconv_plan tfft_gbconv_plan;

enum { TFFT_GBCONV_MAX_TAPS = 2049 };

/* flags of tfft_gbconv_opts / tfft_gbconv_describe; any other bit is refused */
enum {
  TFFT_GBCONV_PRE_GATE = 1,  /* the forward operator multiplies the input by a gate before the convolution */
  TFFT_GBCONV_POST_GATE = 2  /* the forward operator multiplies the result by a gate */
};

typedef struct tfft_gbconv_opts {
  uint32_t struct_size;     /* sizeof(tfft_gbconv_opts) as the caller was compiled (TFFT_GBCONV_OPTS_INIT sets it); the struct grows
                               only by appending fields. Any other value is refused (TFFT_ERR_ARG), as tfft_gsconv_opts.struct_size is */
  uint32_t reserved_;       /* must be 0 */
  uint64_t x_seq_stride;    /* halves between consecutive sequences of x: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t pre_seq_stride;  /* the same for the pre gate (checked whether or not the plan has that gate) */
  uint64_t gy_seq_stride;   /* the same for gy */
  uint64_t post_seq_stride; /* the same for the post gate */
  uint64_t dx_seq_stride;   /* the same for dx */
  uint64_t dpre_seq_stride; /* the same for dpre */
  uint32_t launch_iters;    /* launch shape of the input gradient, as tfft_sconv_opts.launch_iters. Never changes results */
  uint32_t partials;        /* cap on P, the partial sums per channel of the tap gradient; 0 = the default (see Summation order) */
  int flags;                /* TFFT_GBCONV_* */
} tfft_gbconv_opts;         /* 72 bytes */
#define TFFT_GBCONV_OPTS_INIT {(uint32_t)sizeof(tfft_gbconv_opts)}

/* Host only: the geometry of a plan; halo, hop and segments are those of tfft_sconv_geometry, *partials_out is P for the cap
 * `partials` (0 = none). Each of the four pointers may be NULL. TFFT_ERR_ARG for a shape that tfft_gbconv_plan_create refuses. */
TFFT_GBCONV_API int tfft_gbconv_geometry(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, uint64_t* halo,
                                         uint64_t* hop, uint64_t* segments, uint64_t* partials_out);

/* The shapes, refusals and messages of tfft_gsconv_plan_create. opts: NULL (no gates, all defaults) or a tfft_gbconv_opts. */
TFFT_GBCONV_API int tfft_gbconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                            const tfft_gbconv_opts* opts, tfft_gbconv_plan** out);
TFFT_GBCONV_API void tfft_gbconv_plan_destroy(tfft_gbconv_plan* plan);

/* Builds the filter spectra from `taps` ([channels][taps] binary16 on the device) and `skip` ([channels] binary16 on the device, or
 * NULL for no skip) under the rules of tfft_gsconv_plan_set_taps (through the host, waits for `stream`, not under capture; may be
 * called again). Only the input gradient needs it: tfft_gbconv_exec_input_grad before any set_taps is TFFT_ERR_ARG,
 * tfft_gbconv_exec_tap_grad works without. */
TFFT_GBCONV_API int tfft_gbconv_plan_set_taps(tfft_gbconv_plan* plan, const void* taps, const void* skip, void* stream);

/* Copies the binary16 filter spectrum H' the plan built (NOT conjugated: bit for bit what tfft_gsconv_plan_spectrum hands out for
 * the same taps and skip) into caller device memory: two planes of channels * 4096 halves, natural bin order. Synchronous.
 * TFFT_ERR_ARG before set_taps. */
TFFT_GBCONV_API int tfft_gbconv_plan_spectrum(const tfft_gbconv_plan* plan, void* h_re, void* h_im);

/* The workspace of the tap gradient, under the rules of tfft_conv.h: _workspace_bytes is channels * P * Kpad * 4; _set_workspace
 * hands in caller memory (256-byte aligned, at least that large; TFFT_ERR_WORKSPACE when too small; NULL gives it back);
 * _prepare allocates the plan's own now, so that later executions only launch. */
TFFT_GBCONV_API size_t tfft_gbconv_plan_workspace_bytes(const tfft_gbconv_plan* plan);
TFFT_GBCONV_API int tfft_gbconv_plan_set_workspace(tfft_gbconv_plan* plan, void* device_ptr, size_t bytes);
TFFT_GBCONV_API int tfft_gbconv_plan_prepare(tfft_gbconv_plan* plan);

/* dx (and dpre, where it is not NULL) from gy, all sequences, enqueued on `stream` (NULL = default stream); does not synchronise.
 * Which pointers are NULL: see Gates. No output shares a half with an input or the other output (see Aliasing); a refused call
 * launches nothing. */
TFFT_GBCONV_API int tfft_gbconv_exec_input_grad(const tfft_gbconv_plan* plan, const void* gy, const void* post, const void* x, const void* pre,
                                                void* dx, void* dpre, void* stream);

/* dh ([channels][taps] fp32) and, where it is not NULL, dskip ([channels] fp32, the bits of dh[c][0]) from x, pre, gy and post:
 * gbconv4096::wgrad_kernel<Pre, Post>, then gbconv4096::wreduce_kernel, on `stream`. */
TFFT_GBCONV_API int tfft_gbconv_exec_tap_grad(const tfft_gbconv_plan* plan, const void* x, const void* pre, const void* gy, const void* post,
                                              void* dh, void* dskip, void* stream);

/* Kernel launches of the plan (3: one for the input gradient, two for the tap gradient; 0 for NULL), and their names one per line
 * as c++filt prints them: "gbconv4096::dgrad_kernel<P, Q>", "gbconv4096::wgrad_kernel<P, Q>" with P = "true" for a plan with a pre
 * gate and Q = "true" for one with a post gate, else "false", and "gbconv4096::wreduce_kernel". _kernels returns the number of
 * lines, or TFFT_ERR_ARG when `bytes` is too small. */
TFFT_GBCONV_API int tfft_gbconv_plan_num_launches(const tfft_gbconv_plan* plan);
TFFT_GBCONV_API int tfft_gbconv_plan_kernels(const tfft_gbconv_plan* plan, char* buf, size_t bytes);

/* Host only: what tfft_gbconv_plan_create would build, as text: "gbconv4096:4096 x S | partials P" without gates,
 * "gbconv4096:4096:pre x S | partials P", "gbconv4096:4096:post x S | partials P" or "gbconv4096:4096:pre+post x S | partials P".
 * Refuses what tfft_gbconv_plan_create refuses on the same shape and flags. */
TFFT_GBCONV_API int tfft_gbconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, int flags,
                                         char* buf, size_t bytes);

/* Message of the last failure of a tfft_gbconv_* call on this thread ("" if none). */
TFFT_GBCONV_API const char* tfft_gbconv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_GBCONV_H_ */
