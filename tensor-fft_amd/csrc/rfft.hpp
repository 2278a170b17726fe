// rfft.hpp — real-input transforms (include/tfft.h, tfft_rplan_*): two real signals per complex transform.
//
// Real signals 2p and 2p + 1 of a batch (stride s) are the RE and IM planes of complex block p with batch stride 2 s, so the
// library's complex plans transform them without a copy: Z = DFT(a + i b) / N. rsplit.hpp turns Z into the two half spectra and
// back. Paths:
//   R2C, N = 4096   one pass: the N = 4096 kernel with its fused split epilogue (k4096.hpp, RS = true)
//   R2C, other N    complex plan (input preserved) into the workspace, then split_kernel below
//   C2R             merge_kernel below into the workspace, then the inverse complex plan straight into the caller's real buffer
// An odd batch pairs its last signal with itself (its B half is never written / its IM output goes to a scratch plane): nothing
// reads or writes past the caller's `batch` signals. Included at the end of tfft.hip (uses its plan internals).
#pragma once

namespace rfft {

constexpr int kBlock = 256;
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ u4 ld(const uint16_t* p) {
  if (NT) return __builtin_nontemporal_load(reinterpret_cast<const u4*>(p));
  return *reinterpret_cast<const u4*>(p);
}
template <bool NT>
__device__ __forceinline__ void st(uint16_t* p, u4 v) {
  if (NT)
    __builtin_nontemporal_store(v, reinterpret_cast<u4*>(p));
  else
    *reinterpret_cast<u4*>(p) = v;
}
__device__ __forceinline__ uint16_t lane_elem(u4 v, int j) {
  return static_cast<uint16_t>(v[j >> 1] >> (16 * (j & 1)));
}
__device__ __forceinline__ u4 pack8(const uint16_t* h) {
  return u4{h[0] | (uint32_t{h[1]} << 16), h[2] | (uint32_t{h[3]} << 16), h[4] | (uint32_t{h[5]} << 16), h[6] | (uint32_t{h[7]} << 16)};
}
// 32-bit value of lane `src` of this wave (ds_bpermute); the caller guarantees that lane is active
__device__ __forceinline__ uint32_t from_lane(uint32_t v, int src) {
  return static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src * 4, static_cast<int>(v)));
}

struct SplitArgs {
  const uint16_t* z;          // pair p at z + 2 n p: [RE n | IM n], natural order
  uint16_t* out_re;           // half spectrum of signal s at out_* + s * ostride, bins 0 .. n/2
  uint16_t* out_im;
  uint64_t n, ostride;
  uint32_t pairs, self_pair;  // self_pair: index of the self-paired pair (odd batch), else 0xffffffff
};

// Thread (p, v), v < n/16: Z vector v (bins 8v .. 8v+7) and its mirror, vector n/8 - 1 - v (bins n - 8v - 8 .. n - 8v - 1). Bin
// 8v + j pairs with n - 8v - j: element 8 - j of the mirror for j = 1 .. 7; for j = 0, element 0 of vector n/8 - v, which is the
// mirror the neighbouring lane (v - 1) loaded. Lane 0 of a wave with v > 0 loads that vector itself; v = 0 pairs bin 0 with itself
// and also writes the Nyquist bin n/2 (element 0 of vector n/16) as one half.
template <bool NT>
__global__ __launch_bounds__(kBlock) void split_kernel(SplitArgs a) {
  const uint64_t half8 = a.n / 16, m8 = a.n / 8;
  const uint64_t total = static_cast<uint64_t>(a.pairs) * half8;
  const int lane = static_cast<int>(threadIdx.x & 63);
  for (uint64_t t = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x; t < total; t += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint32_t p = static_cast<uint32_t>(t / half8);
    const uint64_t v = t - p * half8;
    const uint16_t* const zr = a.z + 2 * a.n * p;
    const uint16_t* const zi = zr + a.n;
    const u4 xr = ld<false>(zr + 8 * v), xi = ld<false>(zi + 8 * v);
    const u4 yr = ld<false>(zr + 8 * (m8 - 1 - v)), yi = ld<false>(zi + 8 * (m8 - 1 - v));
    // element 0 of vector (n/8 - v) mod n/8, RE in the low half, IM in the high half
    const uint32_t mine = uint32_t{lane_elem(yr, 0)} | (uint32_t{lane_elem(yi, 0)} << 16);
    uint32_t e0 = from_lane(mine, lane > 0 ? lane - 1 : 0);
    if (v == 0) {
      e0 = uint32_t{lane_elem(xr, 0)} | (uint32_t{lane_elem(xi, 0)} << 16);
    } else if (lane == 0) {
      const u4 wr = ld<false>(zr + 8 * (m8 - v)), wi = ld<false>(zi + 8 * (m8 - v));
      e0 = uint32_t{lane_elem(wr, 0)} | (uint32_t{lane_elem(wi, 0)} << 16);
    }
    uint16_t ar[8], ai[8], br[8], bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint16_t mr = j ? lane_elem(yr, 8 - j) : static_cast<uint16_t>(e0);
      const uint16_t mi = j ? lane_elem(yi, 8 - j) : static_cast<uint16_t>(e0 >> 16);
      rsplit::split_bin(lane_elem(xr, j), lane_elem(xi, j), mr, mi, ar[j], ai[j], br[j], bi[j]);
    }
    uint16_t* const o_re = a.out_re + 2 * a.ostride * p;
    uint16_t* const o_im = a.out_im + 2 * a.ostride * p;
    const bool has_b = p != a.self_pair;
    st<NT>(o_re + 8 * v, pack8(ar));
    st<NT>(o_im + 8 * v, pack8(ai));
    if (has_b) {
      st<NT>(o_re + a.ostride + 8 * v, pack8(br));
      st<NT>(o_im + a.ostride + 8 * v, pack8(bi));
    }
    if (v == 0) {
      const uint16_t nr = zr[a.n / 2], ni = zi[a.n / 2];
      uint16_t qr, qi, sr, si;
      rsplit::split_bin(nr, ni, nr, ni, qr, qi, sr, si);
      o_re[a.n / 2] = qr;
      o_im[a.n / 2] = qi;
      if (has_b) {
        o_re[a.ostride + a.n / 2] = sr;
        o_im[a.ostride + a.n / 2] = si;
      }
    }
  }
}

struct MergeArgs {
  const uint16_t* in_re;      // half spectrum of signal s at in_* + s * istride, bins 0 .. n/2
  const uint16_t* in_im;
  uint16_t* z;                // pair p at z + 2 n p: [RE n | IM n]
  uint64_t n, istride;
  uint32_t pairs, self_pair;  // self_pair: its B half spectrum is its A half spectrum
};

// Thread (p, v), v < n/16: writes Z vector v (bins 8v + j, from bin 8v + j of A and B) and its mirror n/8 - 1 - v (bin
// n - 8v - 8 + j, from bin 8v + 8 - j): elements 7 .. 1 of the same input vector, and for j = 0 bin 8v + 8, element 0 of the next
// input vector, which the neighbouring lane (v + 1) loaded. Lane 63 loads it itself; for v = n/16 - 1 it is the Nyquist bin n/2,
// read as one half.
template <bool NT>
__global__ __launch_bounds__(kBlock) void merge_kernel(MergeArgs a) {
  const uint64_t half8 = a.n / 16, m8 = a.n / 8;
  const uint64_t total = static_cast<uint64_t>(a.pairs) * half8;
  const int lane = static_cast<int>(threadIdx.x & 63);
  for (uint64_t t = blockIdx.x * static_cast<uint64_t>(kBlock) + threadIdx.x; t < total; t += static_cast<uint64_t>(gridDim.x) * kBlock) {
    const uint32_t p = static_cast<uint32_t>(t / half8);
    const uint64_t v = t - p * half8;
    const uint16_t* const a_re = a.in_re + 2 * a.istride * p;
    const uint16_t* const a_im = a.in_im + 2 * a.istride * p;
    const uint64_t b_off = p == a.self_pair ? 0 : a.istride;
    const u4 ar = ld<NT>(a_re + 8 * v), ai = ld<NT>(a_im + 8 * v);
    const u4 br = ld<NT>(a_re + b_off + 8 * v), bi = ld<NT>(a_im + b_off + 8 * v);
    // bin 8v + 8 of A and B: (A.re | A.im << 16), (B.re | B.im << 16)
    uint32_t na = from_lane(uint32_t{lane_elem(ar, 0)} | (uint32_t{lane_elem(ai, 0)} << 16), lane < 63 ? lane + 1 : 63);
    uint32_t nb = from_lane(uint32_t{lane_elem(br, 0)} | (uint32_t{lane_elem(bi, 0)} << 16), lane < 63 ? lane + 1 : 63);
    const bool nyq = v + 1 == half8;
    if (nyq) {
      const uint64_t k = a.n / 2;
      na = uint32_t{a_re[k]} | (uint32_t{a_im[k]} << 16);
      nb = uint32_t{a_re[b_off + k]} | (uint32_t{a_im[b_off + k]} << 16);
    } else if (lane == 63) {
      const u4 war = ld<NT>(a_re + 8 * v + 8), wai = ld<NT>(a_im + 8 * v + 8);
      const u4 wbr = ld<NT>(a_re + b_off + 8 * v + 8), wbi = ld<NT>(a_im + b_off + 8 * v + 8);
      na = uint32_t{lane_elem(war, 0)} | (uint32_t{lane_elem(wai, 0)} << 16);
      nb = uint32_t{lane_elem(wbr, 0)} | (uint32_t{lane_elem(wbi, 0)} << 16);
    }
    uint16_t lr[8], li[8], hr[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      rsplit::merge_low(lane_elem(ar, j), lane_elem(ai, j), lane_elem(br, j), lane_elem(bi, j), v == 0 && j == 0, lr[j], li[j]);
      if (j)
        rsplit::merge_high(lane_elem(ar, 8 - j), lane_elem(ai, 8 - j), lane_elem(br, 8 - j), lane_elem(bi, 8 - j), false, hr[j], hi[j]);
      else
        rsplit::merge_high(static_cast<uint16_t>(na), static_cast<uint16_t>(na >> 16), static_cast<uint16_t>(nb),
                           static_cast<uint16_t>(nb >> 16), nyq, hr[0], hi[0]);
    }
    uint16_t* const zr = a.z + 2 * a.n * p;
    uint16_t* const zi = zr + a.n;
    st<false>(zr + 8 * v, pack8(lr));
    st<false>(zi + 8 * v, pack8(li));
    st<false>(zr + 8 * (m8 - 1 - v), pack8(hr));
    st<false>(zi + 8 * (m8 - 1 - v), pack8(hi));
  }
}

}  // namespace rfft

struct tfft_rplan {
  uint64_t n = 0, batch = 0, pairs = 0;
  int device = 0;
  uint64_t rstride = 0, sstride = 0;   // real-signal and half-spectrum batch strides (halves)
  bool fused = false;                  // R2C through the N = 4096 kernel's split epilogue
  bool plain_acc = false;              // split / merge with plain instead of non-temporal accesses on the caller's side
  int num_cus = 0;
  // complex plans: forward over the batch / 2 full pairs (fused: over all pairs) and over the self-paired last signal; inverse likewise
  tfft_plan* fwd = nullptr;
  tfft_plan* fwd_tail = nullptr;
  tfft_plan* inv = nullptr;
  tfft_plan* inv_tail = nullptr;
  // workspace: [Z: pairs x (RE n | IM n)] [scratch plane: n halves (odd batch)] [workspace of fwd / inv] [of fwd_tail / inv_tail]
  size_t off_scratch = 0, off_sub = 0, off_sub_tail = 0, ws_need = 0;
  mutable std::mutex ws_mutex;
  void* ws = nullptr;
  size_t ws_bytes = 0;
  bool ws_owned = false;
};

namespace {

inline size_t rpart(size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); }
inline uint64_t rpitch(uint64_t n) { return ((n / 2 + 1) + 7) & ~uint64_t{7}; }
inline bool rplan_fused(uint64_t n, int flags) { return n == 4096 && !(flags & TFFT_RPLAN_TWO_PASS); }
// Variant of the forward complex sub-plans. N = 4096: the default N = 4096 kernel (staged, non-temporal), named explicitly so that
// plan wisdom (tfft_tuning_*) cannot give the sub-plan another decomposition: the fused launch runs that kernel with the sub-plan's
// tables, and the two-pass path must compute the same spectra. Other n: 0, the library's default (wisdom included).
constexpr int kVarK4096Default = TFFT_VARIANT_K4096_STAGE_OUT | TFFT_VARIANT_K4096_NONTEMPORAL;
inline int rplan_fwd_variant(uint64_t n) { return n == 4096 ? kVarK4096Default : 0; }

// every argument of tfft_rplan_create that can be checked without a device; fills the strides
int rplan_check(uint64_t n, uint64_t batch, const tfft_plan_opts* caller_opts, int flags, tfft_plan_opts* o, uint64_t* rs, uint64_t* ss) {
  const int rc = normalise_opts(caller_opts, o);
  if (rc) return rc;
  if (!is_pow2(n)) return fail(TFFT_ERR_NOT_POW2, "Error! Input size has to be a power of 2!");
  if (n < 16) return fail(TFFT_ERR_TOO_SMALL, "real-input transforms need n >= 16");
  if (n > (uint64_t{1} << 30)) return fail(TFFT_ERR_ARG, "real-input transforms exist up to n = 2^30");
  if (batch == 0 || batch > 0xffffffffull) return fail(TFFT_ERR_ARG, "batch must be in [1, 2^32)");
  if (flags & ~TFFT_RPLAN_TWO_PASS) return fail(TFFT_ERR_ARG, "unknown tfft_rplan_create flags (" + std::to_string(flags) + ")");
  if (o->inner > 1) return fail(TFFT_ERR_ARG, "real-input transforms exist for a contiguous axis only (inner <= 1)");
  if (o->output_order != TFFT_ORDER_NATURAL || o->input_order != TFFT_ORDER_NATURAL)
    return fail(TFFT_ERR_ARG, "real-input transforms exist in natural order only");
  if (o->fourstep_n || o->fourstep_col0) return fail(TFFT_ERR_ARG, "fourstep_n is not available for real-input transforms");
  if (o->variant) return fail(TFFT_ERR_ARG, "tfft_plan_opts.variant must be 0 for real-input transforms (its bits are reserved)");
  if (o->preserve_input)
    return fail(TFFT_ERR_ARG, "tfft_plan_opts.preserve_input must be 0 for real-input transforms (their inputs are never written)");
  if (o->scale < TFFT_SCALE_SEQUENTIAL || o->scale > TFFT_SCALE_ONCE) return fail(TFFT_ERR_ARG, "unknown tfft_plan_opts.scale");
  if (o->launch_iters > TFFT_LAUNCH_PERSISTENT) return fail(TFFT_ERR_ARG, "launch_iters must be 0 .. 65535");
  *rs = o->in_batch_stride ? o->in_batch_stride : n;
  *ss = o->out_batch_stride ? o->out_batch_stride : 2 * rpitch(n);
  if (*rs < n || *rs % 8) return fail(TFFT_ERR_ARG, "real batch stride (in_batch_stride) must be a multiple of 8 and at least n");
  if (*ss < n / 2 + 1 || *ss % 8)
    return fail(TFFT_ERR_ARG, "spectrum batch stride (out_batch_stride) must be a multiple of 8 and at least n/2 + 1");
  if (*rs > (uint64_t{1} << 40) || *ss > (uint64_t{1} << 40)) return fail(TFFT_ERR_ARG, "batch stride too large");
  return TFFT_OK;
}

// hands every complex sub-plan its slice of the real plan's workspace
void rplan_distribute(tfft_rplan* r) {
  uint8_t* const w = static_cast<uint8_t*>(r->ws);
  auto give = [&](tfft_plan* p, size_t off) {
    if (p && tfft_plan_workspace_bytes(p)) tfft_plan_set_workspace(p, w ? w + off : nullptr, w ? tfft_plan_workspace_bytes(p) : 0);
  };
  give(r->fwd, r->off_sub);
  give(r->inv, r->off_sub);
  give(r->fwd_tail, r->off_sub_tail);
  give(r->inv_tail, r->off_sub_tail);
}

int rplan_ensure_workspace(tfft_rplan* r) {
  std::lock_guard<std::mutex> lock(r->ws_mutex);
  if (r->ws_need == 0 || r->ws) return TFFT_OK;       // (a caller's workspace was checked for size when it was handed in)
  TFFT_HIP(hipMalloc(&r->ws, r->ws_need));
  r->ws_bytes = r->ws_need;
  r->ws_owned = true;
  rplan_distribute(r);
  return TFFT_OK;
}

// [p, p + 2 ((batch - 1) stride + extent)) in bytes
inline bool ranges_meet(const void* a, uint64_t sa, uint64_t ea, const void* b, uint64_t sb, uint64_t eb, uint64_t batch) {
  const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
  const uintptr_t a_end = pa + 2 * ((batch - 1) * sa + ea), b_end = pb + 2 * ((batch - 1) * sb + eb);
  return !(a_end <= pb || b_end <= pa);
}

// pointer checks of both directions: real plane (rstride, n) and the two spectrum planes (sstride, n/2 + 1); all read-only inputs
// may share memory, every output must be disjoint from everything else
int rplan_check_ptrs(const tfft_rplan* r, const void* real, const void* s_re, const void* s_im, bool r2c) {
  if (!real || !s_re || !s_im) return fail(TFFT_ERR_ARG, "null data pointer");
  if ((reinterpret_cast<uintptr_t>(real) | reinterpret_cast<uintptr_t>(s_re) | reinterpret_cast<uintptr_t>(s_im)) & 15)
    return fail(TFFT_ERR_ARG, "data pointers must be 16-byte aligned");
  const uint64_t h = r->n / 2 + 1;
  if (ranges_meet(real, r->rstride, r->n, s_re, r->sstride, h, r->batch) || ranges_meet(real, r->rstride, r->n, s_im, r->sstride, h, r->batch))
    return fail(TFFT_ERR_ARG, "real and spectrum planes overlap (in-place real-input transforms are not supported)");
  if (r2c && planes_overlap(s_re, r->sstride, s_im, r->sstride, r->batch, h))
    return fail(TFFT_ERR_ARG, "the RE and IM spectrum planes overlap");
  int cur = 0;
  TFFT_HIP(hipGetDevice(&cur));
  if (cur != r->device) return fail(TFFT_ERR_ARG, "plan was created for another device than the current one");
  return TFFT_OK;
}

inline uint32_t rgrid(const tfft_rplan* r) {
  const uint64_t threads = r->pairs * (r->n / 16);
  return static_cast<uint32_t>(std::min<uint64_t>((threads + rfft::kBlock - 1) / rfft::kBlock, static_cast<uint64_t>(r->num_cus) * 16));
}

int launch_fused_r2c(const Launch& L, const tfft_rplan* r, const void* in, void* out_re, void* out_im) {
  const tfft_plan* const p = r->fwd;
  uint32_t live, grid;
  k4096_shape(p, live, grid);
  const k4096::RealOut ro{r->sstride, (r->batch & 1) ? static_cast<uint32_t>(r->pairs - 1) : 0xffffffffu};
  constexpr int V = k4096::kStageOut | k4096::kNonTemporal;
  return launch(L, p->device, k4096::fft4096_kernel<V, false, true>, kname("k4096::fft4096_kernel", V, false, true), dim3(grid), dim3(k4096::kThreads),
                k4096::kLdsBytes, static_cast<const uint16_t*>(in), static_cast<const uint16_t*>(in) + r->rstride, static_cast<uint16_t*>(out_re),
                static_cast<uint16_t*>(out_im), p->in_map, p->out_map, static_cast<uint32_t>(p->batch), live,
                static_cast<const uint8_t*>(p->d_tables), p->otw, ro);
}

// the split / merge pass of a real-input plan (non-temporal accesses unless the plan's cache policy says plain)
int launch_split(const Launch& L, const tfft_rplan* r, const rfft::SplitArgs& a) {
  if (r->plain_acc) return launch(L, r->device, rfft::split_kernel<false>, kname("rfft::split_kernel", false), dim3(rgrid(r)), dim3(rfft::kBlock), 0, a);
  return launch(L, r->device, rfft::split_kernel<true>, kname("rfft::split_kernel", true), dim3(rgrid(r)), dim3(rfft::kBlock), 0, a);
}

int launch_merge(const Launch& L, const tfft_rplan* r, const rfft::MergeArgs& a) {
  if (r->plain_acc) return launch(L, r->device, rfft::merge_kernel<false>, kname("rfft::merge_kernel", false), dim3(rgrid(r)), dim3(rfft::kBlock), 0, a);
  return launch(L, r->device, rfft::merge_kernel<true>, kname("rfft::merge_kernel", true), dim3(rgrid(r)), dim3(rfft::kBlock), 0, a);
}

void rplan_free(tfft_rplan* r) {
  tfft_plan_destroy(r->fwd);
  tfft_plan_destroy(r->fwd_tail);
  tfft_plan_destroy(r->inv);
  tfft_plan_destroy(r->inv_tail);
  if (r->ws && r->ws_owned) (void)hipFree(r->ws);
  delete r;
}

}  // namespace

extern "C" {

uint64_t tfft_rplan_spectrum_pitch(uint64_t n) { return (is_pow2(n) && n >= 16) ? rpitch(n) : 0; }

int tfft_rplan_create(uint64_t n, uint64_t batch, int device_id, const tfft_plan_opts* opts, int flags, tfft_rplan** out) {
  g_err.clear();
  if (!out) return fail(TFFT_ERR_ARG, "null plan pointer");
  *out = nullptr;
  tfft_plan_opts o;
  uint64_t rs = 0, ss = 0;
  int rc = rplan_check(n, batch, opts, flags, &o, &rs, &ss);
  if (rc) return rc;
  rc = tfft_device_check(device_id);
  if (rc) return rc;
  tfft_rplan* r = new tfft_rplan;
  r->n = n;
  r->batch = batch;
  r->pairs = (batch + 1) / 2;
  r->device = device_id;
  r->rstride = rs;
  r->sstride = ss;
  r->fused = rplan_fused(n, flags);
  r->plain_acc = cache_policy(n, 1, r->pairs);
  auto bail = [&](int code) {
    const std::string keep = g_err;
    rplan_free(r);
    g_err = keep;
    return code;
  };
  hipDeviceProp_t prop;
  r->num_cus = hipGetDeviceProperties(&prop, device_id) == hipSuccess ? prop.multiProcessorCount : 256;
  // forward sub-plans read the caller's signals (preserved); inverse ones read the merged spectrum in the workspace (scratch)
  auto sub = [&](uint64_t b, uint64_t in_stride, uint64_t out_stride, bool forward, tfft_plan** p) {
    tfft_plan_opts co = TFFT_PLAN_OPTS_INIT;
    co.in_batch_stride = in_stride;
    co.out_batch_stride = out_stride;
    co.preserve_input = forward ? 1 : 0;
    co.variant = forward ? rplan_fwd_variant(n) : 0;
    co.scale = o.scale;
    co.launch_iters = o.launch_iters;
    return tfft_plan_create(n, b, device_id, &co, p);
  };
  const uint64_t full = batch / 2;
  const bool odd = batch & 1;
  if (r->fused) {
    rc = sub(r->pairs, 2 * rs, 2 * ss, true, &r->fwd);       // the fused launch uses its tables, addressing and launch shape
    // (the launch assumes exactly this: one N = 4096 pass with its tables)
    if (rc == TFFT_OK && !(single_kernel(r->fwd) && r->fwd->passes[0].kind == PassKind::K4096 && r->fwd->d_tables))
      rc = fail(TFFT_ERR_ARG, "internal: the sub-plan of the fused R2C is not the N = 4096 kernel");
  } else {
    rc = full ? sub(full, 2 * rs, 2 * n, true, &r->fwd) : TFFT_OK;
    if (rc == TFFT_OK && odd) rc = sub(1, 0, 0, true, &r->fwd_tail);
  }
  if (rc == TFFT_OK && full) rc = sub(full, 2 * n, 2 * rs, false, &r->inv);
  if (rc == TFFT_OK && odd) rc = sub(1, 0, 0, false, &r->inv_tail);
  if (rc) return bail(rc);
  size_t off = rpart(static_cast<size_t>(r->pairs) * n * 4);
  r->off_scratch = off;
  if (odd) off += rpart(n * 2);
  r->off_sub = off;
  off += rpart(std::max(tfft_plan_workspace_bytes(r->fwd), tfft_plan_workspace_bytes(r->inv)));
  r->off_sub_tail = off;
  off += rpart(std::max(tfft_plan_workspace_bytes(r->fwd_tail), tfft_plan_workspace_bytes(r->inv_tail)));
  r->ws_need = off;
  if (r->fused) {   // LDS opt-in of the fused kernel now, so that an execution is launches only
    const WalkPtrs f = walk_ptrs(0);
    rc = launch_fused_r2c(Launch::opt_in(), r, f.in_re, f.out_re, f.out_im);
    if (rc) return bail(rc);
  }
  *out = r;
  return TFFT_OK;
}

void tfft_rplan_destroy(tfft_rplan* r) {
  if (r) rplan_free(r);
}

int tfft_rplan_describe(uint64_t n, uint64_t batch, int flags, char* buf, size_t bytes) {
  g_err.clear();
  if (!buf || bytes == 0) return fail(TFFT_ERR_ARG, "null buffer");
  tfft_plan_opts o;
  uint64_t rs = 0, ss = 0;
  int rc = rplan_check(n, batch, nullptr, flags, &o, &rs, &ss);
  if (rc) return rc;
  // the decompositions tfft_rplan_create gives its forward and inverse sub-plans (the full pairs; the odd tail is one more transform)
  char fchain[256], ichain[256];
  const uint64_t full = std::max<uint64_t>(batch / 2, 1);
  const uint64_t fwd_batch = rplan_fused(n, flags) ? (batch + 1) / 2 : full;
  const int fv = rplan_fwd_variant(n);
  rc = tfft_plan_describe(n, 1, fv ? fv : tfft_plan_default_variant(n, 1, fwd_batch), fchain, sizeof(fchain));
  if (rc == TFFT_OK) rc = tfft_plan_describe(n, 1, tfft_plan_default_variant(n, 1, full), ichain, sizeof(ichain));
  if (rc) return rc;
  const std::string text = std::string("r2c: ") + fchain + (rplan_fused(n, flags) ? "+split" : " split") + " | c2r: merge " + ichain;
  if (text.size() + 1 > bytes) return fail(TFFT_ERR_ARG, "buffer too small");
  std::memcpy(buf, text.c_str(), text.size() + 1);
  return TFFT_OK;
}

int tfft_rplan_kernels(const tfft_rplan* r, int c2r, char* buf, size_t bytes) {
  g_err.clear();
  if (!r) return fail(TFFT_ERR_ARG, "null plan");
  // the launch order of tfft_exec_r2c / tfft_exec_c2r; the sub-plans run out of place
  std::vector<std::string> names;
  int rc = TFFT_OK;
  if (!c2r && r->fused) {
    const WalkPtrs f = walk_ptrs(0);
    rc = record_walk(names, [&](const Launch& L) { return launch_fused_r2c(L, r, f.in_re, f.out_re, f.out_im); });
  } else if (!c2r) {
    for (const tfft_plan* sub : {r->fwd, r->fwd_tail})
      if (sub && rc == TFFT_OK) rc = record_kernels(sub, false, names);
    if (rc == TFFT_OK) rc = record_walk(names, [&](const Launch& L) { return launch_split(L, r, rfft::SplitArgs{}); });
  } else {
    rc = record_walk(names, [&](const Launch& L) { return launch_merge(L, r, rfft::MergeArgs{}); });
    for (const tfft_plan* sub : {r->inv, r->inv_tail})
      if (sub && rc == TFFT_OK) rc = record_kernels(sub, false, names);
  }
  return rc ? rc : put_kernel_lines(names, buf, bytes);
}

int tfft_rplan_num_launches(const tfft_rplan* r, int c2r) {
  if (!r) return 0;
  if (!c2r && r->fused) return 1;
  return 1 + tfft_plan_num_launches(c2r ? r->inv : r->fwd) + tfft_plan_num_launches(c2r ? r->inv_tail : r->fwd_tail);
}

size_t tfft_rplan_workspace_bytes(const tfft_rplan* r) { return r ? r->ws_need : 0; }

int tfft_rplan_set_workspace(tfft_rplan* r, void* device_ptr, size_t bytes) {
  g_err.clear();
  if (!r) return fail(TFFT_ERR_ARG, "null plan");
  if (device_ptr && bytes < r->ws_need)
    return fail(TFFT_ERR_WORKSPACE, "workspace of " + std::to_string(bytes) + " bytes is smaller than tfft_rplan_workspace_bytes() = " +
                                        std::to_string(r->ws_need));
  if (reinterpret_cast<uintptr_t>(device_ptr) & 255) return fail(TFFT_ERR_ARG, "workspace must be 256-byte aligned");
  std::lock_guard<std::mutex> lock(r->ws_mutex);
  if (r->ws && r->ws_owned) (void)hipFree(r->ws);
  r->ws = device_ptr;
  r->ws_bytes = device_ptr ? bytes : 0;
  r->ws_owned = false;
  rplan_distribute(r);
  return TFFT_OK;
}

int tfft_rplan_prepare(tfft_rplan* r) {
  g_err.clear();
  if (!r) return fail(TFFT_ERR_ARG, "null plan");
  int prev = 0;
  TFFT_HIP(hipGetDevice(&prev));
  TFFT_HIP(hipSetDevice(r->device));
  const DeviceRestore restore{prev};
  return rplan_ensure_workspace(r);
}

int tfft_exec_r2c(const tfft_rplan* rc_plan, const void* in, void* out_re, void* out_im, void* stream) {
  g_err.clear();
  if (!rc_plan) return fail(TFFT_ERR_ARG, "null plan");
  tfft_rplan* const r = const_cast<tfft_rplan*>(rc_plan);
  int rc = rplan_check_ptrs(r, in, out_re, out_im, true);
  if (rc) return rc;
  const Launch L = Launch::run(stream);
  if (r->fused) {
    rc = launch_fused_r2c(L, r, in, out_re, out_im);
    if (rc) return rc;
    TFFT_HIP(hipGetLastError());
    return TFFT_OK;
  }
  rc = rplan_ensure_workspace(r);
  if (rc) return rc;
  const uint16_t* const x = static_cast<const uint16_t*>(in);
  uint16_t* const z = static_cast<uint16_t*>(r->ws);
  const uint64_t n = r->n, full = r->batch / 2;
  if (r->fwd) {
    rc = tfft_exec(r->fwd, x, x + r->rstride, z, z + n, stream);
    if (rc) return rc;
  }
  if (r->fwd_tail) {
    const uint16_t* const xl = x + (r->batch - 1) * r->rstride;
    rc = tfft_exec(r->fwd_tail, xl, xl, z + 2 * n * full, z + 2 * n * full + n, stream);
    if (rc) return rc;
  }
  const rfft::SplitArgs a{z, static_cast<uint16_t*>(out_re), static_cast<uint16_t*>(out_im), n, r->sstride,
                          static_cast<uint32_t>(r->pairs), (r->batch & 1) ? static_cast<uint32_t>(r->pairs - 1) : 0xffffffffu};
  rc = launch_split(L, r, a);
  if (rc) return rc;
  TFFT_HIP(hipGetLastError());
  return TFFT_OK;
}

int tfft_exec_c2r(const tfft_rplan* rc_plan, const void* in_re, const void* in_im, void* out, void* stream) {
  g_err.clear();
  if (!rc_plan) return fail(TFFT_ERR_ARG, "null plan");
  tfft_rplan* const r = const_cast<tfft_rplan*>(rc_plan);
  int rc = rplan_check_ptrs(r, out, in_re, in_im, false);
  if (rc) return rc;
  rc = rplan_ensure_workspace(r);
  if (rc) return rc;
  const Launch L = Launch::run(stream);
  uint16_t* const z = static_cast<uint16_t*>(r->ws);
  const uint64_t n = r->n, full = r->batch / 2;
  const rfft::MergeArgs a{static_cast<const uint16_t*>(in_re), static_cast<const uint16_t*>(in_im), z, n, r->sstride,
                          static_cast<uint32_t>(r->pairs), (r->batch & 1) ? static_cast<uint32_t>(r->pairs - 1) : 0xffffffffu};
  rc = launch_merge(L, r, a);
  if (rc) return rc;
  TFFT_HIP(hipGetLastError());
  uint16_t* const y = static_cast<uint16_t*>(out);
  if (r->inv) {
    rc = tfft_exec_inverse(r->inv, z, z + n, y, y + r->rstride, stream);
    if (rc) return rc;
  }
  if (r->inv_tail) {
    uint16_t* const scratch = reinterpret_cast<uint16_t*>(static_cast<uint8_t*>(r->ws) + r->off_scratch);
    rc = tfft_exec_inverse(r->inv_tail, z + 2 * n * full, z + 2 * n * full + n, y + (r->batch - 1) * r->rstride, scratch, stream);
    if (rc) return rc;
  }
  return TFFT_OK;
}

}  // extern "C"
