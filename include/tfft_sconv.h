/* tfft_sconv.h — C ABI of the overlap-save causal convolution add-on (libtfft_sconv.so) of the MI355X (gfx950) tensor-core FFT
 * library: the causal real convolution of tfft_lconv.h for sequences of ANY length, in one kernel, for filters of up to 2049 taps.
 *
 * A long convolution plan takes `rows` x `channels` REAL sequences of `length` L samples and convolves each with the `taps` K real
 * taps of its channel, linearly and causally:
 *
 *     y[b][c][t] = sum over j <= t, j < K of  h[c][j] * x[b][c][t - j]          t = 0 .. L - 1
 *
 * The add-on is layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): it links against both and uses
 * their status codes (TFFT_OK, TFFT_ERR_*) and conventions. Only plain pointers and sizes cross this boundary: device pointers
 * are raw HIP device addresses, `stream` is a hipStream_t passed as void*.
 *
 * Shapes. L a multiple of 8 and >= 8, at most 2^26; rows B >= 1, channels C >= 1, B C below 2^32; 1 <= K <= 2049. A longer filter
 * is refused with a message that names tfft_lconv_plan_create, whose composed path takes it (partitioned filters are not built).
 *
 * Method: overlap-save at transform length 4096. The geometry depends on K alone (tfft_sconv_geometry reports it):
 *
 *     halo     = K - 1 rounded up to a multiple of 64 samples    (0 .. 2048; the multiple of 64 puts every segment boundary on a
 *                                                                  128-byte line whenever the sequence starts on one)
 *     hop      = 4096 - halo                                      (2048 .. 4096)
 *     segments = ceil(L / hop) = S
 *
 * Segment s of a sequence is the 4096-sample window that starts at sample s * hop - halo; it reads as zero wherever it lies before
 * sample 0 or at or after sample L, and nothing outside [0, L) of any sequence is ever read. The window is convolved circularly
 * with the filter by the arithmetic of conv4096_kernel. A circular product wraps only into the first K - 1 <= halo samples of the
 * window, so window samples [halo, halo + min(hop, L - s * hop)) are the linear convolution and are written to y[s * hop ...].
 * Every output sample is written once; every input sample is read (hop + halo) / hop times (1.02 for K <= 65, 2 at K = 2049).
 *
 * Data contract: that of tfft_lconv.h. Real binary16; sequence (b, c) at in + (b * channels + c) * in_seq_stride halves, L
 * samples; a stride of 0 means L, otherwise it is a multiple of 8 and >= L. The output has the same layout with out_seq_stride;
 * halves between sequences are never written. Pointers are 16-byte aligned.
 *
 * Aliasing. ANY overlap of input and output is refused (TFFT_ERR_ARG), exact in-place execution included, unlike tfft_lconv_exec:
 * segment s reads, as its halo, the last samples of the stretch that segment s - 1 writes, and the segments of a sequence are
 * work items of different waves that run in no defined order. In place, a segment could find its halo already convolved.
 *
 * Pairing. Rows 2p and 2p + 1 of a channel are the RE and the IM plane of ONE complex transform, as in tfft_lconv.h (a real filter
 * has a Hermitian spectrum, so the two planes are convolved independently). An odd number of rows pairs its last row with zeros;
 * that partner is neither loaded nor stored. Work item (p * S + s) * channels + c is segment s of pair p of channel c,
 * ceil(rows / 2) * S * channels items (below 2^32): the item index modulo `channels` is the filter, the layout a tfft_conv_plan
 * with batch = items and filters = channels expects.
 *
 * Taps are [channels][taps] binary16 on the device, handed over once per plan (tfft_sconv_plan_set_taps). The filter spectrum is
 * the n = 4096 spectrum of tfft_lconv_spectrum_host: H = the fp64 FFT of the zero-padded taps (no 1/n), rounded ONCE to binary16;
 * the imaginary parts of bins 0 and 2048 are exactly 0 and the planes are exactly Hermitian. tfft_sconv_plan_spectrum hands out
 * what the plan built.
 *
 * Life cycle. One kernel, sconv4096::sconv4096_kernel, per execution and no workspace. The tables, the LDS opt-in and the device
 * memory of the spectrum are set up at creation, so an execution only launches: it is legal under stream capture, and executions
 * of one plan may overlap in time.
 *
 * Range contract: that of tfft_lconv.h, per window. With X = the unscaled 4096-point spectrum of one window of the pair
 * x_2p + i x_2p+1, results are finite whenever
 *     max_k |X_k| |H_k| <= 32752
 *     and max |y| <= 65504     (y = the window's full 4096-point circular convolution, the discarded halo included)
 *     and |x_2p + i x_2p+1| <= 64512 for every sample of a pair of rows (both up to 45600 at once; a row without partner: any finite value).
 */
#ifndef TFFT_SCONV_H_
#define TFFT_SCONV_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_SCONV_API __attribute__((visibility("default")))
#else
#define TFFT_SCONV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_sconv_plan tfft_sconv_plan;

enum { TFFT_SCONV_MAX_TAPS = 2049 };

typedef struct tfft_sconv_opts {
  uint32_t struct_size;    /* sizeof(tfft_sconv_opts) as the caller was compiled (TFFT_SCONV_OPTS_INIT sets it); the struct grows only
                              by appending fields. Any other value is refused (TFFT_ERR_ARG), as tfft_lconv_opts.struct_size is */
  uint32_t reserved_;      /* must be 0 */
  uint64_t in_seq_stride;  /* halves between consecutive sequences of the input: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t out_seq_stride; /* the same for the output */
  uint32_t launch_iters;   /* launch shape, as tfft_lconv_opts.launch_iters: 0 = the library's default (the shape of conv4096_kernel
                              applied to the item count); k = 1 .. 65534: a wave takes about k items and retires (grid =
                              ceil(workgroups / k)); TFFT_LAUNCH_PERSISTENT: one workgroup per CU for all items. Never changes
                              results */
  int flags;               /* no flag is defined yet: must be 0 */
} tfft_sconv_opts;
#define TFFT_SCONV_OPTS_INIT {(uint32_t)sizeof(tfft_sconv_opts)}

/* Host only: the geometry of a plan for `length` and `taps`; each of the three pointers may be NULL. TFFT_ERR_ARG for a length or a
 * number of taps that tfft_sconv_plan_create refuses. */
TFFT_SCONV_API int tfft_sconv_geometry(uint64_t length, uint64_t taps, uint64_t* halo, uint64_t* hop, uint64_t* segments);

/* rows B >= 1, channels C >= 1 (B C and the item count below 2^32), length L a multiple of 8, 8 .. 2^26, taps 1 .. 2049. opts: NULL
 * (all defaults) or a tfft_sconv_opts. TFFT_ERR_ARG for anything else, checked before the device is touched; TFFT_ERR_DEVICE /
 * TFFT_ERR_HIP as tfft_plan_create. The first call compares tfft_abi_version() of the libtfft.so it runs against with the
 * TFFT_ABI_VERSION it was built with. */
TFFT_SCONV_API int tfft_sconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                          const tfft_sconv_opts* opts, tfft_sconv_plan** out);
TFFT_SCONV_API void tfft_sconv_plan_destroy(tfft_sconv_plan* plan);

/* Builds the filter spectra from `taps` ([channels][taps] binary16 on the device); may be called again to replace the taps. The
 * rules of tfft_lconv_plan_set_taps: not on the hot path, it goes through the host and waits for `stream` (not under stream
 * capture), and when the plan already had taps the device is drained before they are replaced. Executions enqueued later, on any
 * stream, see the new taps; the caller's array is not referenced after the call returns. The plan's device must be current.
 * tfft_sconv_exec before any set_taps is TFFT_ERR_ARG. */
TFFT_SCONV_API int tfft_sconv_plan_set_taps(tfft_sconv_plan* plan, const void* taps, void* stream);

/* Copies the binary16 filter spectrum the plan built into caller device memory: two planes of channels * 4096 halves, bin k of
 * channel c at [c * 4096 + k], natural bin order (what tfft_conv_plan_set_filter takes). Synchronous. TFFT_ERR_ARG before set_taps. */
TFFT_SCONV_API int tfft_sconv_plan_spectrum(const tfft_sconv_plan* plan, void* h_re, void* h_im);

/* Enqueues all sequences on `stream` (NULL = default stream); does not synchronise. The plan's device must be current. Input and
 * output must not share a half (see Aliasing); a refused call launches nothing. */
TFFT_SCONV_API int tfft_sconv_exec(const tfft_sconv_plan* plan, const void* in, void* out, void* stream);

/* Kernel launches of one execution (1; 0 for NULL), and their names one per line in launch order ("sconv4096::sconv4096_kernel").
 * _kernels returns the number of lines, or TFFT_ERR_ARG when `bytes` is too small. */
TFFT_SCONV_API int tfft_sconv_plan_num_launches(const tfft_sconv_plan* plan);
TFFT_SCONV_API int tfft_sconv_plan_kernels(const tfft_sconv_plan* plan, char* buf, size_t bytes);

/* Host only: what tfft_sconv_plan_create would build, as text: "sconv4096:4096 x S", S the segments per sequence. Refuses what
 * tfft_sconv_plan_create refuses on the same shape and flags. */
TFFT_SCONV_API int tfft_sconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes);

/* Message of the last failure of a tfft_sconv_* call on this thread ("" if none). */
TFFT_SCONV_API const char* tfft_sconv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_SCONV_H_ */
