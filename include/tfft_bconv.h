/* tfft_bconv.h — C ABI of the gradient add-on (libtfft_bconv.so) of the MI355X (gfx950) tensor-core FFT library: the two gradients
 * of the overlap-save causal convolution of tfft_sconv.h, so that the operator can be trained through.
 *
 * The forward pass takes `rows` x `channels` REAL sequences of `length` L samples and `taps` K real taps per channel:
 *
 *     y[b][c][t]  = sum over j <= t, j < K      of  h[c][j] * x[b][c][t - j]          t = 0 .. L - 1
 *
 * With g = d loss / d y, a gradient plan computes
 *
 *     dx[b][c][t] = sum over j < K, t + j < L   of  h[c][j] * g[b][c][t + j]          (input gradient: an anticausal correlation)
 *     dh[c][j]    = sum over b, t >= j, t < L   of  g[b][c][t] * x[b][c][t - j]       (tap gradient, j = 0 .. K - 1, fp32)
 *
 * The add-on is layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): it links against both and uses
 * their status codes (TFFT_OK, TFFT_ERR_*) and conventions. Only plain pointers and sizes cross this boundary: device pointers
 * are raw HIP device addresses, `stream` is a hipStream_t passed as void*.
 *
 * Shapes: those of tfft_sconv_plan_create. L a multiple of 8 and >= 8, at most 2^26; rows B >= 1, channels C >= 1, B C and the item
 * count below 2^32; 1 <= K <= 2049 (a longer filter is refused with the message of tfft_sconv_plan_create).
 *
 * Method: overlap-save at transform length 4096 on the geometry of tfft_sconv_geometry (halo = K - 1 rounded up to a multiple of
 * 64, hop = 4096 - halo, segments S = ceil(L / hop)). Nothing outside [0, L) of any sequence is ever read.
 *
 *   input gradient  Segment s is the 4096-sample window of g that starts at sample s * hop (no front halo), zero at or beyond
 *                   sample L. It is multiplied by conj(H), H the filter spectrum of tfft_sconv.h, by the arithmetic of
 *                   sconv4096_kernel; window samples [0, min(hop, L - s * hop)) are written to dx[s * hop ...]: sample t < hop needs
 *                   window samples up to t + K - 1 < 4096 because halo >= K - 1. One kernel, bconv4096::dgrad_kernel, no workspace.
 *   tap gradient    Item (p, s) of channel c: Zx is the complex window of the x pair as the forward plan loads it (it starts at
 *                   s * hop - halo), Zg the same window of the g pair with its first `halo` samples forced to zero (they belong
 *                   to segment s - 1). The RE plane of ifft(conj(fft(Zx)) fft(Zg)) holds, at lags 0 .. K - 1, the sum of the two
 *                   rows' correlations restricted to this segment; the cross terms land in the IM plane, which is discarded.
 *                   dh[c] is the sum of those RE planes over all items of the channel. bconv4096::wgrad_kernel keeps
 *                   conj(fft(Zx) / 4096), rounded to binary16, in registers as the filter of sconv4096_kernel's two passes over
 *                   Zg, so an item's result is its correlation DIVIDED BY 4096, a binary16 image of which lags 0 .. K - 1 are added
 *                   in fp32. bconv4096::wreduce_kernel sums the partial sums, multiplies by 4096 (exact) and writes dh.
 *
 * Summation order of the tap gradient. The items of a channel, i = p * S + s (p the pair of rows, s the segment), are dealt to P
 * partial sums: partial q adds the items i = q, q + P, q + 2 P ... in increasing i, and dh is partial 0 + partial 1 + ... in
 * increasing q, all in fp32. P = min(items per channel, ceil(2048 / C)) (2048 = 256 CUs x 8 waves), capped by
 * tfft_bconv_opts.partials where that is not 0; tfft_bconv_geometry reports it. The order is fixed by P alone, never by the launch:
 * there are no atomics, two executions give the same bits, and the result depends on P only through the order of fp32 additions.
 *
 * Data contract: that of tfft_sconv.h for x, g and dx, each with its own sequence stride (0 means L, otherwise a multiple of 8 that
 * is >= L); halves between sequences are never written. Pointers are 16-byte aligned. dh is [channels][taps] fp32, dense, 4-byte
 * aligned. Taps are [channels][taps] binary16 on the device (tfft_bconv_plan_set_taps; the input gradient needs them, the tap
 * gradient does not); the spectrum is tfft_lconv_spectrum_host's at n = 4096, and the input gradient multiplies by its conjugate:
 * the sign bit of every non-zero imaginary part flipped, which is exact and keeps the planes exactly Hermitian.
 *
 * Aliasing. ANY overlap of g and dx is refused (TFFT_ERR_ARG), exact in-place execution included: segment s reads, beyond its hop,
 * the first samples of the stretch that segment s + 1 writes, and segments run in no defined order. For the tap gradient, dh and
 * the workspace must not overlap x, g or each other; x and g may be the same memory.
 *
 * Pairing. Rows 2p and 2p + 1 of a channel are the RE and the IM plane of ONE complex transform, as in tfft_sconv.h. An odd number
 * of rows pairs its last row with zeros; that partner is neither loaded nor stored. Work item (p * S + s) * channels + c of the input
 * gradient is what a tfft_conv_plan with batch = items and filters = channels expects.
 *
 * Life cycle. The input gradient needs no workspace and only launches: it is legal under stream capture, and executions may
 * overlap in time. The tap gradient needs channels * P * Kpad * 4 bytes (Kpad = K rounded up to a multiple of 8) for its partial
 * sums, under the rules of tfft_conv.h: hand it in (tfft_bconv_plan_set_workspace), let tfft_bconv_plan_prepare allocate it, or
 * let the first execution do so; an execution never reallocates, and an execution of a prepared plan only launches (legal under
 * capture). Executions of ONE plan's tap gradient must not overlap in time: they share the partial sums.
 *
 * Range contract: that of tfft_sconv.h, per window. Input gradient: with G the unscaled spectrum of a window of the g pair,
 * max_k |G_k| |H_k| <= 32752 and max |window's circular correlation| <= 65504. Tap gradient: the "filter" is Zx's spectrum / 4096,
 * so max_k |G_k| |X_k| / 4096 <= 32752 and max |item's circular correlation| / 4096 <= 65504; for samples in (-1, 1) |X_k| / 4096
 * is about 0.03 and nothing comes near either bound. Every pair that is transformed (g in the input gradient, x and g in the tap
 * gradient) has to meet |v_2p + i v_2p+1| <= 64512 sample by sample (tfft_sconv.h; a row without partner: any finite value).
 */
#ifndef TFFT_BCONV_H_
#define TFFT_BCONV_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_BCONV_API __attribute__((visibility("default")))
#else
#define TFFT_BCONV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_bconv_plan tfft_bconv_plan;

enum { TFFT_BCONV_MAX_TAPS = 2049 };

typedef struct tfft_bconv_opts {
  uint32_t struct_size;    /* sizeof(tfft_bconv_opts) as the caller was compiled (TFFT_BCONV_OPTS_INIT sets it); the struct grows only
                              by appending fields. Any other value is refused (TFFT_ERR_ARG), as tfft_sconv_opts.struct_size is */
  uint32_t reserved_;      /* must be 0 */
  uint64_t x_seq_stride;   /* halves between consecutive sequences of x: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t g_seq_stride;   /* the same for g */
  uint64_t dx_seq_stride;  /* the same for dx */
  uint32_t launch_iters;   /* launch shape of the input gradient, as tfft_sconv_opts.launch_iters. Never changes results */
  uint32_t partials;       /* cap on P, the partial sums per channel of the tap gradient; 0 = the default (see Summation order) */
  int flags;               /* no flag is defined yet: must be 0 */
} tfft_bconv_opts;
#define TFFT_BCONV_OPTS_INIT {(uint32_t)sizeof(tfft_bconv_opts)}

/* Host only: the geometry of a plan; halo, hop and segments are those of tfft_sconv_geometry, *partials_out is P for the cap
 * `partials` (0 = none). Each of the four pointers may be NULL. TFFT_ERR_ARG for a shape that tfft_bconv_plan_create refuses. */
TFFT_BCONV_API int tfft_bconv_geometry(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, uint64_t* halo,
                                       uint64_t* hop, uint64_t* segments, uint64_t* partials_out);

/* The shapes, refusals and messages of tfft_sconv_plan_create. opts: NULL (all defaults) or a tfft_bconv_opts. */
TFFT_BCONV_API int tfft_bconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                          const tfft_bconv_opts* opts, tfft_bconv_plan** out);
TFFT_BCONV_API void tfft_bconv_plan_destroy(tfft_bconv_plan* plan);

/* Builds the filter spectra from `taps` ([channels][taps] binary16 on the device) under the rules of tfft_sconv_plan_set_taps (through
 * the host, waits for `stream`, not under capture; may be called again). Only the input gradient needs it:
 * tfft_bconv_exec_input_grad before any set_taps is TFFT_ERR_ARG, tfft_bconv_exec_tap_grad works without. */
TFFT_BCONV_API int tfft_bconv_plan_set_taps(tfft_bconv_plan* plan, const void* taps, void* stream);

/* Copies the binary16 filter spectrum H the plan built (NOT conjugated: what tfft_sconv_plan_spectrum hands out for the same taps)
 * into caller device memory: two planes of channels * 4096 halves, natural bin order. Synchronous. TFFT_ERR_ARG before set_taps. */
TFFT_BCONV_API int tfft_bconv_plan_spectrum(const tfft_bconv_plan* plan, void* h_re, void* h_im);

/* The workspace of the tap gradient, under the rules of tfft_conv.h: _workspace_bytes is channels * P * Kpad * 4; _set_workspace
 * hands in caller memory (256-byte aligned, at least that large; TFFT_ERR_WORKSPACE when too small; NULL gives it back);
 * _prepare allocates the plan's own now, so that later executions only launch. */
TFFT_BCONV_API size_t tfft_bconv_plan_workspace_bytes(const tfft_bconv_plan* plan);
TFFT_BCONV_API int tfft_bconv_plan_set_workspace(tfft_bconv_plan* plan, void* device_ptr, size_t bytes);
TFFT_BCONV_API int tfft_bconv_plan_prepare(tfft_bconv_plan* plan);

/* dx from g, all sequences, enqueued on `stream` (NULL = default stream); does not synchronise. g and dx must not share a half (see
 * Aliasing); a refused call launches nothing. */
TFFT_BCONV_API int tfft_bconv_exec_input_grad(const tfft_bconv_plan* plan, const void* g, void* dx, void* stream);

/* dh ([channels][taps] fp32) from x and g: bconv4096::wgrad_kernel, then bconv4096::wreduce_kernel, on `stream`. */
TFFT_BCONV_API int tfft_bconv_exec_tap_grad(const tfft_bconv_plan* plan, const void* x, const void* g, void* dh, void* stream);

/* Kernel launches of the plan (3: one for the input gradient, two for the tap gradient; 0 for NULL), and their names one per line:
 * "bconv4096::dgrad_kernel", "bconv4096::wgrad_kernel", "bconv4096::wreduce_kernel". _kernels returns the number of lines, or
 * TFFT_ERR_ARG when `bytes` is too small. */
TFFT_BCONV_API int tfft_bconv_plan_num_launches(const tfft_bconv_plan* plan);
TFFT_BCONV_API int tfft_bconv_plan_kernels(const tfft_bconv_plan* plan, char* buf, size_t bytes);

/* Host only: what tfft_bconv_plan_create would build, as text: "bconv4096:4096 x S | partials P". Refuses what
 * tfft_bconv_plan_create refuses on the same shape and flags. */
TFFT_BCONV_API int tfft_bconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, uint32_t partials, int flags,
                                       char* buf, size_t bytes);

/* Message of the last failure of a tfft_bconv_* call on this thread ("" if none). */
TFFT_BCONV_API const char* tfft_bconv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_BCONV_H_ */
