/* tfft_gconv.h — C ABI of the gated causal convolution add-on (libtfft_gconv.so) of the MI355X (gfx950) tensor-core FFT library.
 *
 * A gated plan computes, for `rows` x `channels` REAL sequences of `length` L samples, what the long-convolution operators of
 * sequence models (H3, Hyena and their relatives) wrap around the causal convolution of tfft_lconv.h:
 *
 *     u[b][c][t] = p[b][c][t] * x[b][c][t]                                           (pre gate; u = x without one)
 *     z[b][c][t] = sum over j <= t, j < K of  h[c][j] * u[b][c][t - j]  +  d[c] * u[b][c][t]
 *     y[b][c][t] = g[b][c][t] * z[b][c][t]                                           (post gate; y = z without one)
 *
 * in ONE pass over the data: x, p and g are read once and y is written once, 4 sequences of L halves through HBM where a caller
 * of tfft_lconv_exec with elementwise kernels around it moves 8 and more.
 *
 * The add-on is layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): it links against both, runs the
 * composed path through a tfft_conv_plan, and uses their status codes (TFFT_OK, TFFT_ERR_*) and conventions. It does not use
 * libtfft_lconv.so. Only plain pointers and sizes cross this boundary: device pointers are raw HIP device addresses, `stream` is a
 * hipStream_t passed as void*.
 *
 * Data contract. Real binary16. Sequence (b, c) of the input sits at in + (b * channels + c) * in_seq_stride halves and holds L
 * samples; a stride of 0 means L, otherwise it is a multiple of 8 and >= L. The gates and the output have the same layout, each
 * with its own stride (pre_seq_stride, post_seq_stride, out_seq_stride). Halves between output sequences are never written, and
 * nothing beyond sample L of an input or gate sequence is ever read. Pointers are 16-byte aligned.
 *
 * Gates are fixed per plan by TFFT_GCONV_PRE_GATE / TFFT_GCONV_POST_GATE: tfft_gconv_exec refuses (TFFT_ERR_ARG) a NULL pointer
 * for a gate the plan has and a non-NULL pointer for one it does not have. With an odd number of rows the gate sequences of the
 * row that does not exist are neither read nor used.
 *
 * Aliasing. Exact in-place execution (out == in, equal strides) is allowed. A gate may alias the input or the other gate: both
 * are only read. Any overlap of a gate with the output, and any overlap of input and output other than exact in-place, is refused
 * (TFFT_ERR_ARG).
 *
 * Taps are [channels][taps] binary16 on the device and the skip weights d are [channels] binary16 on the device or NULL (= 0),
 * handed over once per plan (tfft_gconv_plan_set_taps); sequence (b, c) takes filter c and skip c.
 *
 * Method: that of tfft_lconv.h. The transform length n is 4096 for every shape the fused kernel takes (below), else
 * tfft_gconv_fft_length(L, K), the smallest power of two >= max(L + K - 1, 256). Rows 2p and 2p + 1 of a channel are the RE and
 * the IM plane of ONE complex transform. An odd number of rows pairs its last row with zeros. Work items are ordered
 * p * channels + c, ceil(rows / 2) * channels of them.
 *
 * Filter spectrum and skip. h * u + d u is the convolution of u with the taps whose tap 0 is h[0] + d. So the skip costs nothing
 * on the device: H' = the fp64 FFT of the zero-padded taps with skip[c] added to tap 0 IN FP64 (no 1/n, as in tfft_conv.h),
 * rounded ONCE to binary16; the imaginary parts of bins 0 and n / 2 are exactly 0 and the planes are exactly Hermitian. With
 * skip == NULL or a skip of zero the spectrum is bit for bit tfft_lconv_spectrum_host's. tfft_gconv_spectrum_host is that
 * computation for one filter; tfft_gconv_plan_spectrum hands out what the plan built.
 *
 * Arithmetic. u = p * x is ONE IEEE binary16 multiply per sample (round to nearest even, subnormals kept). z is what the shipped
 * arithmetic gives for the input u with the spectrum H': the statements of lconv4096::lconv4096_kernel on the fused path, pack ->
 * tfft_conv_plan -> crop on the composed path. y = g * z is one more binary16 multiply. tests/test_gpu_gconv.py holds all three
 * bit for bit.
 *
 * Paths.
 *   L <= 2048 with L + K - 1 <= 4096 (default): ONE kernel at n = 4096, gconv4096::gconv4096_kernel<Pre, Post>, lconv4096_kernel
 *       with the gates at its two ends: the pre gate is multiplied in on the way into LDS, the post gate on the way out of it.
 *       4 L halves in and 2 L halves out per pair with both gates. No workspace; executions of one plan may overlap in time.
 *   every other shape, and TFFT_GCONV_COMPOSED (n = tfft_gconv_fft_length(L, K)): gate_copy::pack_kernel<Pre> writes the gated
 *       pairs into zero-padded [RE n | IM n] blocks in the workspace, a tfft_conv_plan (batch = items, filters = channels, whatever
 *       path that plan chooses) runs in place on them, gate_copy::crop_kernel<Post> writes the L kept samples per sequence, gated,
 *       into the output; one stream. Needs tfft_gconv_plan_workspace_bytes() of device memory (the blocks and the sub-plan's
 *       scratch): hand it in (256-byte aligned), call tfft_gconv_plan_prepare() once, or let the first execution hipMalloc it.
 *       After either of the first two an execution only launches kernels. Executions of one such plan must not overlap in time.
 *
 * Range contract: that of tfft_lconv.h, applied to u and H'. Results are finite whenever
 *     max_k |U_k| |H'_k| <= 32752  (U = the unscaled n-point spectrum of the zero-padded pair u_2p + i u_2p+1)
 *     and max |z| <= 65504         (z = the full linear convolution of the pair with the skip-carrying taps, discarded samples
 *                                   included)
 *     and max |g z| <= 65504
 *     and |u_2p + i u_2p+1| <= 64512 for every sample of a pair of rows (tfft_lconv.h: the condition is on the gated input).
 */
#ifndef TFFT_GCONV_H_
#define TFFT_GCONV_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_GCONV_API __attribute__((visibility("default")))
#else
#define TFFT_GCONV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_gconv_plan tfft_gconv_plan;

/* flags of tfft_gconv_opts / tfft_gconv_describe */
enum {
  TFFT_GCONV_PRE_GATE = 1,   /* the plan multiplies the input by a gate before the convolution */
  TFFT_GCONV_POST_GATE = 2,  /* the plan multiplies the result by a gate */
  TFFT_GCONV_COMPOSED = 4    /* the generic path for every shape, at the shortest transform length, for A/B and tests */
};

typedef struct tfft_gconv_opts {
  uint32_t struct_size;     /* sizeof(tfft_gconv_opts) as the caller was compiled (TFFT_GCONV_OPTS_INIT sets it); the struct grows only
                               by appending fields. Any other value is refused (TFFT_ERR_ARG), as tfft_lconv_opts.struct_size is */
  uint32_t reserved_;       /* must be 0 */
  uint64_t in_seq_stride;   /* halves between consecutive sequences of the input: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t out_seq_stride;  /* the same for the output */
  uint64_t pre_seq_stride;  /* the same for the pre gate (checked whether or not the plan has that gate) */
  uint64_t post_seq_stride; /* the same for the post gate */
  uint32_t launch_iters;    /* launch shape of the fused kernel, as tfft_lconv_opts.launch_iters: 0 = the library's default; k = 1 ..
                               65534: a wave takes about k items and retires (grid = ceil(workgroups / k)); TFFT_LAUNCH_PERSISTENT: one
                               workgroup per CU for all items. Never changes results. Handed to no sub-plan of the composed path */
  int flags;                /* TFFT_GCONV_* */
} tfft_gconv_opts;          /* 48 bytes */
#define TFFT_GCONV_OPTS_INIT {(uint32_t)sizeof(tfft_gconv_opts)}

/* Host only: the smallest power of two >= max(length + taps - 1, 256), the transform length of the composed path; 0 when length or
 * taps is 0 or the result would exceed 2^26. (tfft_lconv_fft_length.) */
TFFT_GCONV_API uint64_t tfft_gconv_fft_length(uint64_t length, uint64_t taps);

/* rows B >= 1, channels C >= 1 (B C and the item count below 2^32), length L a multiple of 8 and >= 8, taps K >= 1, transform
 * length <= 2^26: the shapes, refusals and messages of tfft_lconv_plan_create. opts: NULL (no gates, all defaults) or a
 * tfft_gconv_opts. TFFT_ERR_ARG for anything else, checked before the device is touched; TFFT_ERR_DEVICE / TFFT_ERR_HIP as
 * tfft_plan_create; errors of the sub-plan are passed through. The first call compares tfft_abi_version() of the libtfft.so it runs
 * against with the TFFT_ABI_VERSION it was built with. */
TFFT_GCONV_API int tfft_gconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                          const tfft_gconv_opts* opts, tfft_gconv_plan** out);
TFFT_GCONV_API void tfft_gconv_plan_destroy(tfft_gconv_plan* plan);

/* Builds the filter spectra from `taps` ([channels][taps] binary16 on the device) and `skip` ([channels] binary16 on the device, or
 * NULL for no skip); may be called again to replace both. Not on the hot path: it goes through the host and waits for `stream`
 * (not under stream capture), and when the plan already had taps the device is drained before they are replaced, as
 * tfft_lconv_plan_set_taps does. Executions enqueued later, on any stream, see the new taps; the caller's arrays are not referenced
 * after the call returns. The plan's device must be current. tfft_gconv_exec before any set_taps is TFFT_ERR_ARG. */
TFFT_GCONV_API int tfft_gconv_plan_set_taps(tfft_gconv_plan* plan, const void* taps, const void* skip, void* stream);

/* Copies the binary16 filter spectrum H' the plan built into caller device memory: two planes of channels * n halves, bin k of
 * channel c at [c * n + k], natural bin order (what tfft_conv_plan_set_filter takes). Synchronous. TFFT_ERR_ARG before set_taps. */
TFFT_GCONV_API int tfft_gconv_plan_spectrum(const tfft_gconv_plan* plan, void* h_re, void* h_im);

/* Host only: the same computation for one filter. taps: K binary16 values on the host; skip: one binary16 value on the host or
 * NULL; n: a power of two >= K, 2 .. 2^26; out_re / out_im: n binary16 values each. */
TFFT_GCONV_API int tfft_gconv_spectrum_host(const uint16_t* taps, uint64_t num_taps, const uint16_t* skip, uint64_t n, uint16_t* out_re,
                                            uint16_t* out_im);

TFFT_GCONV_API uint64_t tfft_gconv_plan_fft_length(const tfft_gconv_plan* plan);     /* the plan's transform length n; 0 for NULL */

TFFT_GCONV_API size_t tfft_gconv_plan_workspace_bytes(const tfft_gconv_plan* plan);    /* 0 for the fused plan */
TFFT_GCONV_API int tfft_gconv_plan_set_workspace(tfft_gconv_plan* plan, void* device_ptr, size_t bytes);
TFFT_GCONV_API int tfft_gconv_plan_prepare(tfft_gconv_plan* plan);

/* Enqueues all sequences on `stream` (NULL = default stream); does not synchronise. pre / post: the gates, each non-NULL exactly
 * when the plan has that gate. The plan's device must be current. */
TFFT_GCONV_API int tfft_gconv_exec(const tfft_gconv_plan* plan, const void* in, const void* pre, const void* post, void* out, void* stream);

/* Kernel launches of one execution, and their names one per line in launch order. The kernels of this library are named by their
 * instantiation, as c++filt prints it: "gconv4096::gconv4096_kernel<P, Q>", "gate_copy::pack_kernel<P>" and
 * "gate_copy::crop_kernel<Q>" with P = "true" for a plan with a pre gate and Q = "true" for one with a post gate, else "false"; the
 * sub-plan's as tfft_conv_plan_kernels names them. _kernels returns the number of lines, or TFFT_ERR_ARG when `bytes` is too
 * small. */
TFFT_GCONV_API int tfft_gconv_plan_num_launches(const tfft_gconv_plan* plan);
TFFT_GCONV_API int tfft_gconv_plan_kernels(const tfft_gconv_plan* plan, char* buf, size_t bytes);

/* Host only: the decomposition tfft_gconv_plan_create would choose, as text. Fused: "gconv4096:4096" without gates,
 * "gconv4096:4096:pre", "gconv4096:4096:post" or "gconv4096:4096:pre+post". Composed: "pack | <tfft_conv_describe of the
 * sub-plan> | crop", with "pack:pre" in place of "pack" for a plan with a pre gate and "crop:post" in place of "crop" for one with a
 * post gate. Refuses what tfft_gconv_plan_create refuses on the same shape and flags. */
TFFT_GCONV_API int tfft_gconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes);

/* Message of the last failure of a tfft_gconv_* call on this thread ("" if none); a failing sub-plan's text is copied into it. */
TFFT_GCONV_API const char* tfft_gconv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_GCONV_H_ */
