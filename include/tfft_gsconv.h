/* tfft_gsconv.h — C ABI of the gated overlap-save causal convolution add-on (libtfft_gsconv.so) of the MI355X (gfx950) tensor-core
 * FFT library: the gated operator of tfft_gconv.h for sequences of ANY length, in one kernel, for filters of up to 2049 taps.
 *
 * A gated long convolution plan computes, for `rows` x `channels` REAL sequences of `length` L samples, `taps` K real taps h[c] and
 * an optional skip weight d[c] per channel:
 *
 *     u[b][c][t] = p[b][c][t] * x[b][c][t]                                           (pre gate; u = x without one)
 *     z[b][c][t] = sum over j <= t, j < K of  h[c][j] * u[b][c][t - j]  +  d[c] * u[b][c][t]
 *     y[b][c][t] = g[b][c][t] * z[b][c][t]                                           (post gate; y = z without one)
 *
 * in ONE pass over the data. With both gates x, p and g are read (1 + halo / hop times for x and p, once for g) and y is written
 * once, where a caller of tfft_sconv_exec with elementwise kernels around it moves 8 sequences of L halves and more.
 *
 * The add-on is layered on libtfft_conv.so (include/tfft_conv.h) and libtfft.so (include/tfft.h): it links against both and uses
 * their status codes (TFFT_OK, TFFT_ERR_*) and conventions. It uses neither libtfft_gconv.so nor libtfft_sconv.so. Only plain
 * pointers and sizes cross this boundary: device pointers are raw HIP device addresses, `stream` is a hipStream_t passed as void*.
 *
 * Shapes. Those of tfft_sconv.h: L a multiple of 8 and >= 8, at most 2^26; rows B >= 1, channels C >= 1, B C below 2^32;
 * 1 <= K <= 2049. A longer filter is refused with a message that names tfft_gconv_plan_create, whose composed path takes it.
 *
 * Method: overlap-save at transform length 4096, the geometry of tfft_sconv.h, fixed by K alone (tfft_gsconv_geometry reports it):
 *
 *     halo     = K - 1 rounded up to a multiple of 64 samples    (0 .. 2048)
 *     hop      = 4096 - halo                                      (2048 .. 4096)
 *     segments = ceil(L / hop) = S
 *
 * Segment s of a sequence is the 4096-sample window of u that starts at sample s * hop - halo; it reads as zero wherever it lies
 * before sample 0 or at or after sample L, and nothing outside [0, L) of any sequence or gate is ever read. The pre gate is applied
 * on the way into the window, indexed by the SOURCE sample: a segment re-reads the gate over its halo just as it re-reads x. The
 * window is convolved circularly with the filter by the arithmetic of conv4096_kernel; window samples
 * [halo, halo + min(hop, L - s * hop)) are the linear convolution, are multiplied by the post gate at the OUTPUT sample
 * s * hop + ... and written there. Every output sample is written once.
 *
 * Data contract: that of tfft_gconv.h. Real binary16; sequence (b, c) of the input at in + (b * channels + c) * in_seq_stride
 * halves, L samples; a stride of 0 means L, otherwise it is a multiple of 8 and >= L. The gates and the output have the same
 * layout, each with its own stride. Halves between output sequences are never written. Pointers are 16-byte aligned.
 *
 * Gates are fixed per plan by TFFT_GSCONV_PRE_GATE / TFFT_GSCONV_POST_GATE: tfft_gsconv_exec refuses (TFFT_ERR_ARG) a NULL pointer
 * for a gate the plan has and a non-NULL pointer for one it does not have.
 *
 * Aliasing. ANY overlap of input and output is refused (TFFT_ERR_ARG), exact in-place execution included, for the reason of
 * tfft_sconv.h: segment s reads, as its halo, the last samples of the stretch that segment s - 1 writes, and segments run in no
 * defined order. Any overlap of a gate with the output is refused. A gate may alias the input or the other gate: both are only
 * read. A refused call launches nothing.
 *
 * Pairing. Rows 2p and 2p + 1 of a channel are the RE and the IM plane of ONE complex transform. An odd number of rows pairs its
 * last row with zeros; neither that partner's sequence nor its gates are read or stored. Work item (p * S + s) * channels + c is
 * segment s of pair p of channel c, ceil(rows / 2) * S * channels items (below 2^32).
 *
 * Taps are [channels][taps] binary16 on the device and the skip weights d are [channels] binary16 on the device or NULL (= 0),
 * handed over once per plan (tfft_gsconv_plan_set_taps). The filter spectrum is H' = the n = 4096 fp64 FFT of the zero-padded taps
 * with skip[c] added to tap 0 IN FP64 (no 1/n), rounded ONCE to binary16; the imaginary parts of bins 0 and 2048 are exactly 0 and
 * the planes are exactly Hermitian. Bit for bit it is tfft_gconv_spectrum_host(taps, K, skip, 4096, ...); with no skip or a skip of
 * zero it is tfft_lconv_spectrum_host's. tfft_gsconv_plan_spectrum hands out what the plan built.
 *
 * Arithmetic. u = p * x is ONE IEEE binary16 multiply per sample (round to nearest even, subnormals kept). z is what
 * sconv4096::sconv4096_kernel's statements give for the input u with the spectrum H'. y = g * z is one more binary16 multiply. A
 * plan without gates gives tfft_sconv_exec's bits (with a skip: for the skip-carrying spectrum).
 *
 * Life cycle: that of tfft_sconv.h. One kernel, gsconv4096::gsconv4096_kernel<Pre, Post>, per execution and no workspace. The
 * tables, the LDS opt-in and the device memory of the spectrum are set up at creation, so an execution only launches: it is legal
 * under stream capture, and executions of one plan may overlap in time.
 *
 * Range contract: that of tfft_sconv.h per window, applied to the windows of u and to H'. With U = the unscaled 4096-point
 * spectrum of one window of the pair u_2p + i u_2p+1, results are finite whenever
 *     max_k |U_k| |H'_k| <= 32752
 *     and max |z| <= 65504     (z = the window's full 4096-point circular convolution, the discarded halo included)
 *     and max |g z| <= 65504
 *     and |u_2p + i u_2p+1| <= 64512 for every sample of a pair of rows (tfft_sconv.h: the condition is on the gated input).
 */
#ifndef TFFT_GSCONV_H_
#define TFFT_GSCONV_H_

#include <stddef.h>
#include <stdint.h>

#include "tfft_conv.h"

#if defined(__GNUC__)
#define TFFT_GSCONV_API __attribute__((visibility("default")))
#else
#define TFFT_GSCONV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tfft_gsconv_plan tfft_gsconv_plan;

enum { TFFT_GSCONV_MAX_TAPS = 2049 };

/* flags of tfft_gsconv_opts / tfft_gsconv_describe; any other bit is refused */
enum {
  TFFT_GSCONV_PRE_GATE = 1,  /* the plan multiplies the input by a gate before the convolution */
  TFFT_GSCONV_POST_GATE = 2  /* the plan multiplies the result by a gate */
};

typedef struct tfft_gsconv_opts {
  uint32_t struct_size;     /* sizeof(tfft_gsconv_opts) as the caller was compiled (TFFT_GSCONV_OPTS_INIT sets it); the struct grows
                               only by appending fields. Any other value is refused (TFFT_ERR_ARG), as tfft_gconv_opts.struct_size is */
  uint32_t reserved_;       /* must be 0 */
  uint64_t in_seq_stride;   /* halves between consecutive sequences of the input: 0 (= L) or a multiple of 8 that is >= L */
  uint64_t out_seq_stride;  /* the same for the output */
  uint64_t pre_seq_stride;  /* the same for the pre gate (checked whether or not the plan has that gate) */
  uint64_t post_seq_stride; /* the same for the post gate */
  uint32_t launch_iters;    /* launch shape, as tfft_sconv_opts.launch_iters: 0 = the library's default (the shape of conv4096_kernel
                               applied to the item count); k = 1 .. 65534: a wave takes about k items and retires (grid =
                               ceil(workgroups / k)); TFFT_LAUNCH_PERSISTENT: one workgroup per CU for all items. Never changes
                               results */
  int flags;                /* TFFT_GSCONV_* */
} tfft_gsconv_opts;         /* 48 bytes */
#define TFFT_GSCONV_OPTS_INIT {(uint32_t)sizeof(tfft_gsconv_opts)}

/* Host only: the geometry of a plan for `length` and `taps` (tfft_sconv_geometry's); each of the three pointers may be NULL.
 * TFFT_ERR_ARG for a length or a number of taps that tfft_gsconv_plan_create refuses. */
TFFT_GSCONV_API int tfft_gsconv_geometry(uint64_t length, uint64_t taps, uint64_t* halo, uint64_t* hop, uint64_t* segments);

/* rows B >= 1, channels C >= 1 (B C and the item count below 2^32), length L a multiple of 8, 8 .. 2^26, taps 1 .. 2049: the
 * shapes, refusals and messages of tfft_sconv_plan_create, but for the filter that is too long. opts: NULL (no gates, all
 * defaults) or a tfft_gsconv_opts. TFFT_ERR_ARG for anything else, checked before the device is touched; TFFT_ERR_DEVICE /
 * TFFT_ERR_HIP as tfft_plan_create. The first call compares tfft_abi_version() of the libtfft.so it runs against with the
 * TFFT_ABI_VERSION it was built with. */
TFFT_GSCONV_API int tfft_gsconv_plan_create(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, int device_id,
                                            const tfft_gsconv_opts* opts, tfft_gsconv_plan** out);
TFFT_GSCONV_API void tfft_gsconv_plan_destroy(tfft_gsconv_plan* plan);

/* Builds the filter spectra from `taps` ([channels][taps] binary16 on the device) and `skip` ([channels] binary16 on the device, or
 * NULL for no skip); may be called again to replace both. The rules of tfft_gconv_plan_set_taps: not on the hot path, it goes
 * through the host and waits for `stream` (not under stream capture), and when the plan already had taps the device is drained
 * before they are replaced. Executions enqueued later, on any stream, see the new taps; the caller's arrays are not referenced
 * after the call returns. The plan's device must be current. tfft_gsconv_exec before any set_taps is TFFT_ERR_ARG. */
TFFT_GSCONV_API int tfft_gsconv_plan_set_taps(tfft_gsconv_plan* plan, const void* taps, const void* skip, void* stream);

/* Copies the binary16 filter spectrum H' the plan built into caller device memory: two planes of channels * 4096 halves, bin k of
 * channel c at [c * 4096 + k], natural bin order (what tfft_conv_plan_set_filter takes). Synchronous. TFFT_ERR_ARG before set_taps. */
TFFT_GSCONV_API int tfft_gsconv_plan_spectrum(const tfft_gsconv_plan* plan, void* h_re, void* h_im);

/* Enqueues all sequences on `stream` (NULL = default stream); does not synchronise. pre / post: the gates, each non-NULL exactly
 * when the plan has that gate. The plan's device must be current. The output shares no half with the input or a gate (see
 * Aliasing); a refused call launches nothing. */
TFFT_GSCONV_API int tfft_gsconv_exec(const tfft_gsconv_plan* plan, const void* in, const void* pre, const void* post, void* out, void* stream);

/* Kernel launches of one execution (1; 0 for NULL), and their names one per line in launch order: the instantiation as c++filt
 * prints it, "gsconv4096::gsconv4096_kernel<P, Q>" with P = "true" for a plan with a pre gate and Q = "true" for one with a post
 * gate, else "false". _kernels returns the number of lines, or TFFT_ERR_ARG when `bytes` is too small. */
TFFT_GSCONV_API int tfft_gsconv_plan_num_launches(const tfft_gsconv_plan* plan);
TFFT_GSCONV_API int tfft_gsconv_plan_kernels(const tfft_gsconv_plan* plan, char* buf, size_t bytes);

/* Host only: what tfft_gsconv_plan_create would build, as text: "gsconv4096:4096 x S" without gates, "gsconv4096:4096:pre x S",
 * "gsconv4096:4096:post x S" or "gsconv4096:4096:pre+post x S", S the segments per sequence. Refuses what tfft_gsconv_plan_create
 * refuses on the same shape and flags. */
TFFT_GSCONV_API int tfft_gsconv_describe(uint64_t length, uint64_t taps, uint64_t rows, uint64_t channels, int flags, char* buf, size_t bytes);

/* Message of the last failure of a tfft_gsconv_* call on this thread ("" if none). */
TFFT_GSCONV_API const char* tfft_gsconv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* TFFT_GSCONV_H_ */
