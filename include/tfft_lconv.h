/* tfft_lconv.h — C ABI of the causal real convolution add-on (libtfft_lconv.so) of the MI355X (gfx950) tensor-core FFT library.
 *
 * A causal convolution plan takes `rows` x `channels` REAL sequences of `length` L samples and convolves each with the `taps` K
 * real taps of its channel, linearly and causally (the depthwise long convolution of sequence models):
 *
 *     y[b][c][t] = sum over j <= t, j < K of  h[c][j] * x[b][c][t - j]          t = 0 .. L - 1
 *
 * The caller pads nothing, builds no spectrum, interleaves nothing and slices nothing: the plan does all of that.
 *
 * The add-on is layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): it links against both, runs the
 * composed path through a tfft_conv_plan, and uses their status codes (TFFT_OK, TFFT_ERR_*) and conventions. Only plain pointers
 * and sizes cross this boundary: device pointers are raw HIP device addresses, `stream` is a hipStream_t passed as void*.
 *
 * Data contract. Real binary16. Sequence (b, c) sits at in + (b * channels + c) * in_seq_stride halves and holds L samples; a
 * stride of 0 means L, otherwise it is a multiple of 8 and >= L. The output has the same layout with out_seq_stride and holds
 * L samples per sequence; halves between sequences are never written, and nothing beyond sample L of an input sequence is
 * ever read. Pointers are 16-byte aligned. Exact in-place execution (out == in, equal strides) is allowed; any other overlap of
 * input and output is refused (TFFT_ERR_ARG).
 *
 * Taps are [channels][taps] binary16 on the device, handed over once per plan (tfft_lconv_plan_set_taps); sequence (b, c) takes
 * filter c.
 *
 * Method. The transform length n is 4096 for every shape the fused kernel takes (below), else tfft_lconv_fft_length(L, K), the
 * smallest power of two >= max(L + K - 1, 256); either way n >= L + K - 1, so nothing wraps around.
 * tfft_lconv_plan_fft_length tells a plan's. Rows 2p and 2p + 1 of a channel are the RE and the IM plane of ONE complex
 * transform: they share a real filter, whose spectrum is Hermitian, so the two planes are convolved independently (the real-filter
 * argument of tfft_conv.h, exactly). An odd number of rows pairs its last row with zeros; that partner is neither loaded nor
 * stored. Work items are ordered p * channels + c, ceil(rows / 2) * channels of them.
 *
 * Filter spectrum. H = the fp64 FFT of the zero-padded taps (no 1/n, as in tfft_conv.h), rounded ONCE to binary16; the imaginary
 * parts of bins 0 and n / 2 are exactly 0 and the planes are exactly Hermitian. tfft_lconv_spectrum_host is that computation for
 * one filter; tfft_lconv_plan_spectrum hands out what the plan built.
 *
 * Paths.
 *   L <= 2048 with L + K - 1 <= 4096 (default): ONE kernel at n = 4096, lconv4096::lconv4096_kernel, the arithmetic of
 *       conv4096_kernel. The zero padding is written into LDS instead of being read from HBM and the discarded half is never
 *       stored: 2 L halves in and 2 L halves out per pair. No workspace; executions of one plan may overlap in time.
 *   every other shape, and TFFT_LCONV_COMPOSED (n = tfft_lconv_fft_length(L, K)): lconv_copy::pack_kernel writes the pairs into zero-padded [RE n | IM n] blocks in the
 *       workspace, a tfft_conv_plan (batch = items, filters = channels, whatever path that plan chooses) runs in place on them,
 *       lconv_copy::crop_kernel writes the L kept samples per sequence into the output; one stream. Needs
 *       tfft_lconv_plan_workspace_bytes() of device memory (the blocks and the sub-plan's scratch): hand it in (256-byte
 *       aligned), call tfft_lconv_plan_prepare() once, or let the first execution hipMalloc it. After either of the first two an
 *       execution only launches kernels. Executions of one such plan must not overlap in time.
 *
 * Range contract: that of tfft_conv.h. The forward transform is sequentially scaled, which bounds the complex magnitude of its
 * intermediates, not each component: rows 2p and 2p + 1 of a channel travel as one complex signal, so the PAIR has to meet
 *     |x_2p + i x_2p+1| <= 64512 for every sample (both rows up to 45600 at once); the last row of an odd count, whose partner is
 *     zero, may take any finite value.
 * The missing factor n is applied as an exact power of two to the fp32 filter value, the product with H is formed in fp32 and
 * rounded ONCE to binary16, and the inverse transform is sequentially scaled again. Results are finite whenever
 *     max_k |X_k| |H_k| <= 32752   (X = the unscaled n-point spectrum of the zero-padded pair x_2p + i x_2p+1)
 *     and max |y| <= 65504         (y = the full linear convolution of the pair, discarded samples included).
 */
#ifndef TFFT_LCONV_H_
#define TFFT_LCONV_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_LCONV_API __attribute__((visibility("default")))
#else
#define TFFT_LCONV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_lconv_plan tfft_lconv_plan;

/* flags of tfft_lconv_opts / tfft_lconv_describe */
enum { TFFT_LCONV_COMPOSED = 1 };   /* the generic path for every shape, at the shortest transform length, for A/B and tests */

typedef struct tfft_lconv_opts {
  uint32_t struct_size;    /* sizeof(tfft_lconv_opts) as the caller was compiled (TFFT_LCONV_OPTS_INIT sets it); the struct grows only
                              by appending fields. Any other value is refused (TFFT_ERR_ARG), as tfft_plan_opts.struct_size is */
  uint32_t reserved_;      /* must be 0 */
  uint64_t in_seq_stride;  /* halves between consecutive sequences of the input: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t out_seq_stride; /* the same for the output */
  uint32_t launch_iters;   /* launch shape of the fused kernel, as tfft_plan_opts.launch_iters: 0 = the library's default (the shape
                              of conv4096_kernel applied to the item count); k = 1 .. 65534: a wave takes about k items and
                              retires, at small item counts too (grid = ceil(workgroups / k)); TFFT_LAUNCH_PERSISTENT: one workgroup
                              per CU for all items. Never changes results. Handed to no sub-plan of the composed path */
  int flags;               /* TFFT_LCONV_* */
} tfft_lconv_opts;
#define TFFT_LCONV_OPTS_INIT {(uint32_t)sizeof(tfft_lconv_opts)}

/* Host only: the smallest power of two >= max(length + taps - 1, 256), the transform length of the composed path; 0 when length or
 * taps is 0 or the result would exceed 2^26. */
TFFT_LCONV_API uint64_t tfft_lconv_fft_length(uint64_t length, uint64_t taps);

/* rows B >= 1, channels C >= 1 (B C and the item count below 2^32), length L a multiple of 8 and >= 8, taps K >= 1, transform
 * length <= 2^26. opts: NULL (all defaults) or a tfft_lconv_opts. TFFT_ERR_ARG for anything else, checked before the device is
 * touched; TFFT_ERR_DEVICE / TFFT_ERR_HIP as tfft_plan_create; errors of the sub-plan are passed through. The first call compares
 * tfft_abi_version() of the libtfft.so it runs against with the TFFT_ABI_VERSION it was built with. */
TFFT_LCONV_API int tfft_lconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                          const tfft_lconv_opts* opts, tfft_lconv_plan** out);
TFFT_LCONV_API void tfft_lconv_plan_destroy(tfft_lconv_plan* plan);

/* Builds the filter spectra from `taps` ([channels][taps] binary16 on the device); may be called again to replace the taps. Not on
 * the hot path: it goes through the host and waits for `stream` (not under stream capture), and when the plan already had taps the
 * device is drained before they are replaced, as tfft_conv_plan_set_filter does. Executions enqueued later, on any stream, see the
 * new taps; the caller's array is not referenced after the call returns. The plan's device must be current. tfft_lconv_exec
 * before any set_taps is TFFT_ERR_ARG. */
TFFT_LCONV_API int tfft_lconv_plan_set_taps(tfft_lconv_plan* plan, const void* taps, void* stream);

/* Copies the binary16 filter spectrum the plan built into caller device memory: two planes of channels * n halves, bin k of
 * channel c at [c * n + k], natural bin order (what tfft_conv_plan_set_filter takes). Synchronous. TFFT_ERR_ARG before set_taps. */
TFFT_LCONV_API int tfft_lconv_plan_spectrum(const tfft_lconv_plan* plan, void* h_re, void* h_im);

/* Host only: the same computation for one filter. taps: K binary16 values on the host; n: a power of two >= K, 2 .. 2^26;
 * out_re / out_im: n binary16 values each. */
TFFT_LCONV_API int tfft_lconv_spectrum_host(const uint16_t* taps, uint64_t num_taps, uint64_t n, uint16_t* out_re, uint16_t* out_im);

TFFT_LCONV_API uint64_t tfft_lconv_plan_fft_length(const tfft_lconv_plan* plan);     /* the plan's transform length n; 0 for NULL */

TFFT_LCONV_API size_t tfft_lconv_plan_workspace_bytes(const tfft_lconv_plan* plan);    /* 0 for the fused plan */
TFFT_LCONV_API int tfft_lconv_plan_set_workspace(tfft_lconv_plan* plan, void* device_ptr, size_t bytes);
TFFT_LCONV_API int tfft_lconv_plan_prepare(tfft_lconv_plan* plan);

/* Enqueues all sequences on `stream` (NULL = default stream); does not synchronise. The plan's device must be current. */
TFFT_LCONV_API int tfft_lconv_exec(const tfft_lconv_plan* plan, const void* in, void* out, void* stream);

/* Kernel launches of one execution, and their names one per line in launch order (the kernels of this library are
 * "lconv4096::lconv4096_kernel", "lconv_copy::pack_kernel" and "lconv_copy::crop_kernel"; the sub-plan's as tfft_conv_plan_kernels names
 * them). _kernels returns the number of lines, or TFFT_ERR_ARG when `bytes` is too small. */
TFFT_LCONV_API int tfft_lconv_plan_num_launches(const tfft_lconv_plan* plan);
TFFT_LCONV_API int tfft_lconv_plan_kernels(const tfft_lconv_plan* plan, char* buf, size_t bytes);

/* Host only: the decomposition tfft_lconv_plan_create would choose, as text: "lconv4096:4096" (fused) or
 * "pack | <tfft_conv_describe of the sub-plan> | crop". Refuses what tfft_lconv_plan_create refuses on the same shape and flags. */
TFFT_LCONV_API int tfft_lconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes);

/* Message of the last failure of a tfft_lconv_* call on this thread ("" if none); a failing sub-plan's text is copied into it. */
TFFT_LCONV_API const char* tfft_lconv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_LCONV_H_ */
