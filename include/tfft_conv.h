/* tfft_conv.h — C ABI of the FFT convolution add-on (libtfft_conv.so) of the MI355X (gfx950) tensor-core FFT library.
 *
 * A convolution plan takes `batch` complex signals of length n and multiplies each, in the frequency domain, by one of
 * `filters` filter spectra:
 *
 *     y_b = ifft( fft(x_b) * H_(b mod filters) )        numpy conventions: fft unscaled, ifft carries the 1/n
 *
 * With H = fft(h) this is the circular convolution of x_b with h; no power of n is left for the caller to track. `b mod filters`
 * is the depthwise layout [batch][channel] with one filter per channel; filters = 1 is one filter for all signals.
 *
 * The add-on is layered on the public ABI of libtfft.so (include/tfft.h): it links against that library, uses its plans for the
 * composed path, its status codes (TFFT_OK, TFFT_ERR_*) and its conventions. Only plain pointers and sizes cross this boundary:
 * device pointers are raw HIP device addresses, `stream` is a hipStream_t passed as void*.
 *
 * Data contract (that of tfft_exec): planar binary16, signal b at plane + b * batch_stride halves (0 selects 2 n, the [RE | IM]
 * block), four independent plane pointers, 16-byte aligned. Exact in-place execution (out == in for both planes, equal strides)
 * is allowed; any other overlap of the planes is refused (TFFT_ERR_ARG), by the checks tfft_exec uses.
 *
 * The filter is handed over once per plan (tfft_conv_plan_set_filter) as two binary16 planes of filters * n halves on the device,
 * bin k of filter f at [f * n + k], natural bin order, unscaled (H = numpy.fft.fft(h)). The plan converts it into a device image of
 * its own (tfft_conv_filter_slot tells where a bin goes); the caller's planes are not referenced after the call returns.
 *
 * Real filters. The transform is linear, so with a REAL filter h (Hermitian H) the RE plane and the IM plane of a signal are
 * convolved independently: y_re = x_re (*) h, y_im = x_im (*) h. A plane pair therefore carries two real signals per complex
 * transform, 4 bytes per real sample through HBM.
 *
 * Paths.
 *   n = 4096 (default): ONE kernel, one pass over HBM (conv4096_kernel: forward transform, filter multiply and inverse
 *       transform without the spectrum leaving the compute unit; 16 KiB in, 16 KiB out per signal). No workspace; executions
 *       of one plan may overlap in time.
 *   every other n, and n = 4096 with TFFT_CONV_COMPOSED: a forward tfft_plan into the workspace, the pointwise kernel
 *       cmul_kernel in the workspace, tfft_exec_inverse into the caller's output. For 2^16 <= n <= 2^24
 *       (tfft_plan_transposed_n2(n) != 0) the spectrum stays in the transposed order between the two plans (2 + 1 + 2 passes;
 *       the filter image is permuted once instead). Needs tfft_conv_plan_workspace_bytes() of device memory: hand it in
 *       (256-byte aligned), call tfft_conv_plan_prepare() once, or let the first execution hipMalloc it. After either of the
 *       first two an execution only launches kernels. Executions of one such plan must not overlap in time.
 *
 * Range contract. The forward transform is sequentially scaled (1/R per radix-R stage). That bounds the complex magnitude of its
 * binary16 intermediates by that of the input, not each component (tfft.h, TFFT_SCALE_SEQUENTIAL), so the signal has to meet
 *     |x_re + i x_im| <= 64512 for every sample (both components up to 45600 at once; any finite value where one plane is all zero).
 * The missing factor n is applied as an exact power of two to the fp32 filter value, the product with H is formed in fp32 and rounded
 * ONCE to binary16, and the inverse transform is sequentially scaled again. Results are finite whenever
 *     max_k |X_k| |H_k| <= 32752   (X = the unscaled spectrum of the signal; half of 65504, so that either component fits)
 *     and max |y| <= 65504
 * for such a signal. (Measured on the MI355X: x_t = 65504 (sgn cos + i sgn sin)(2 pi k t / 4096) with H = 2^-14 at every bin meets the
 * last two conditions, max |X H| = 20 863 and max |y| = 5.7, and comes back as NaN in every sample for k = 1 and k = 16; k = 256 stays
 * finite in the fused kernel, whose third stage is not rounded. At 45600 all three are finite and within 2 ulp of the exact answer.)
 * Fused path: the spectrum is never rounded to binary16 before the multiply (fp32 accumulators times H * 4096); composed path: the
 * forward plan's output X / n is binary16, the multiply is (X / n) * (H * n) in fp32.
 */
#ifndef TFFT_CONV_H_
#define TFFT_CONV_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft.h"

#if defined(__GNUC__)
#define TFFT_CONV_API __attribute__((visibility("default")))
#else
#define TFFT_CONV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_conv_plan tfft_conv_plan;

/* flags of tfft_conv_plan_create / _describe / _filter_slot */
enum { TFFT_CONV_COMPOSED = 1 };   /* the generic three-step path at every n (n = 4096 too), for A/B and tests */

/* n: a power of two, 256 <= n <= 2^26. 1 <= filters <= batch < 2^32. in/out_batch_stride: halves between consecutive signals
 * of a plane, a multiple of 8 and >= 2 n, or 0 (= 2 n). TFFT_ERR_ARG for anything else (checked before the device is
 * touched); TFFT_ERR_DEVICE / TFFT_ERR_HIP as tfft_plan_create; errors of the sub-plans are passed through. The first call
 * compares tfft_abi_version() of the libtfft.so it runs against with the TFFT_ABI_VERSION it was built with. */
TFFT_CONV_API int tfft_conv_plan_create(uint64_t n, uint64_t batch, uint64_t filters, int device_id, uint64_t in_batch_stride,
                                        uint64_t out_batch_stride, int flags, tfft_conv_plan** out);
TFFT_CONV_API void tfft_conv_plan_destroy(tfft_conv_plan* plan);

/* Converts the caller's filter planes (see above) into the plan's own image; may be called again to replace the filter. The
 * conversion is not on the hot path: it goes through the host and waits for `stream` (not under stream capture). Executions
 * enqueued later, on any stream, see the new filter. The plan's device must be current (TFFT_ERR_ARG otherwise, as tfft_conv_exec).
 * tfft_conv_exec before any set_filter is TFFT_ERR_ARG. */
TFFT_CONV_API int tfft_conv_plan_set_filter(tfft_conv_plan* plan, const void* h_re, const void* h_im, void* stream);

TFFT_CONV_API size_t tfft_conv_plan_workspace_bytes(const tfft_conv_plan* plan);    /* 0 for the fused plan */
TFFT_CONV_API int tfft_conv_plan_set_workspace(tfft_conv_plan* plan, void* device_ptr, size_t bytes);
TFFT_CONV_API int tfft_conv_plan_prepare(tfft_conv_plan* plan);

/* Enqueues the whole batch on `stream` (NULL = default stream); does not synchronise. The plan's device must be current. */
TFFT_CONV_API int tfft_conv_exec(const tfft_conv_plan* plan, const void* in_re, const void* in_im, void* out_re, void* out_im, void* stream);

/* Kernel launches of one execution, and their names one per line in launch order (as tfft_plan_kernels names them; the kernels of
 * this library are "conv4096::conv4096_kernel" and "cmul::cmul_kernel"). _kernels returns the number of lines, or TFFT_ERR_ARG
 * when `bytes` is too small. */
TFFT_CONV_API int tfft_conv_plan_num_launches(const tfft_conv_plan* plan);
TFFT_CONV_API int tfft_conv_plan_kernels(const tfft_conv_plan* plan, char* buf, size_t bytes);

/* Host only: the decomposition tfft_conv_plan_create would choose, as text: "conv4096:4096" (fused) or
 * "<forward chain> | cmul | <inverse chain>" in the words of tfft_plan_describe. Refuses what tfft_conv_plan_create refuses on
 * the same n, batch, filters, flags. */
TFFT_CONV_API int tfft_conv_describe(uint64_t n, uint64_t batch, uint64_t filters, int flags, char* buf, size_t bytes);

/* Host only: the slot (in halves, inside one plane of one filter's image) where bin k < n sits in the image of a plan created
 * with (n, flags); UINT64_MAX for arguments no plan accepts. A bijection of 0 .. n - 1. Fused n = 4096, k = k0 + 16 k1 + 256 k2:
 * (((k0 >> 3) * 4 + (k2 & 3)) * 64 + 16 (k2 >> 2) + k1) * 8 + (k0 & 7), the fragment a lane of the kernel owns. Composed,
 * n = n1 n2 with n2 = tfft_plan_transposed_n2(n) != 0: slot k1 n2 + k2 holds bin k1 + n1 k2. Composed, other n: slot k. */
TFFT_CONV_API uint64_t tfft_conv_filter_slot(uint64_t n, int flags, uint64_t k);

/* Message of the last failure of a tfft_conv_* call on this thread ("" if none); a failing sub-plan's tfft_last_error() text is
 * copied into it. */
TFFT_CONV_API const char* tfft_conv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_CONV_H_ */
