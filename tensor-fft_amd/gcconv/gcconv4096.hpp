// gcconv4096.hpp — the GATED overlap-save causal convolution (gsconv/gsconv4096.hpp) and its two gradients (gbconv/gbconv4096.hpp)
// for gfx950 with CONTEXT carried across chunks of a longer sequence (cconv/cconv4096.hpp): gates and context in one pass.
//
//     forward   ue = pe (.) xe,   z = h' * ue,   y = post (.) z         xe / pe: x / pre extended by Hn samples of history / pre_history
//     gze = qe (.) gye                                                  gye / qe: gy / post extended by Fn samples of future / post_future
//     du[t] = sum_j h'[j] gze[t + j]      dx = pre (.) du      dpre = x (.) du
//     dh[j] = sum_b sum_{0 <= t < L} gz[t] ue[t - j]                    dskip = dh[:, 0]
//
// The middles are the shipped kernels', statement by statement (same tables, same three MFMA stages twice, same fp32 filter
// multiply with its one rounding, same filter image in conv4096::filter_slot order, same exchanged-plane write-back and stage-out
// swizzle, same launch shapes, item order and summation order); the store ends are the gated kernels'. Only the load ends are
// re-indexed, and a context is only a second base the per-lane address is selected from:
//
//   fwd_kernel<Pre, Post>    gsconv4096_kernel with a signed source chunk: window chunk j of item (p, s, c) is source chunk
//                            ch = s * hop / 8 - halo / 8 + j. Pre: chunk ch of x AND of the pre gate come in through registers, each
//                            from its sequence for ch in [0, L / 8) and from its context for ch in [-Hn / 8, 0); every other slot is
//                            zero. Without Pre the load is cconv4096::load_window<kHistory> (one LDS-DMA per plane and block).
//   dgrad_kernel<Pre, Post>  gbconv4096::dgrad_kernel with gy and the post gate selected from `future` / `post_future` for
//                            ch in [L / 8, (L + Fn) / 8). Without Post the load is cconv4096::load_window<kFuture>. The output end is
//                            unchanged: pre, x, dx and dpre are indexed by the output chunk.
//   wgrad_kernel<Pre, Post>  the u window as fwd_kernel loads it, the gz window as gbconv4096::wgrad_kernel loads it (no context:
//                            the tap gradient sums over the gz of this chunk only).
//   wreduce_kernel           gbconv4096::wreduce_kernel.
//
// Every context base is handed in shifted, so that source chunk ch of either buffer is base + 16 ch (cconv4096.hpp). The loads through
// registers keep the rule of gsconv4096::load_item: a plane's 16 loads are issued before its first product is formed and none sits
// under a per-lane branch; a lane without a source chunk loads a spare chunk of the SEQUENCE that the item reads anyway, and a
// select writes the product or zero. Hn / 8 and Fn / 8 arrive as 0 when the caller passed no context: nothing outside [0, L) of a
// sequence or gate and [0, Hn) or [0, Fn) of a context is ever read. lo and hi are per-item scalars and every test is on the chunk
// (DESIGN.md 3.12). Only segment 0 reaches in front of sample 0 (hop >= halo), and only the last windows reach behind sample L: whether
// an item's window reaches a context at all is wave-uniform, and an item whose window does not takes the shipped load (one scalar
// base and a 32-bit offset per lane).
//
// The stage code is restated on the k4096 helpers, as the other add-ons restate it and for their reason: including one of them
// would emit its kernels into this code object, and the code generation of the shipped kernels stays untouched.
#pragma once

#include "../csrc/k4096.hpp"

namespace gcconv4096 {

using k4096::f4;
using k4096::h8;
using k4096::s4;
using k4096::u2;
using k4096::u4;

// eight binary16 products, each rounded once (v_pk_mul_f16 x 4): gsconv4096::mul8
__device__ __forceinline__ u4 mul8(u4 a, u4 b) { return __builtin_bit_cast(u4, __builtin_bit_cast(h8, a) * __builtin_bit_cast(h8, b)); }

// one plane's share of a 1-KiB block by LDS-DMA, nt: sconv4096::dma_chunk (lane l's 16 bytes land at dst + 16 l, from the
// address lane l holds: the lanes of one instruction may read from two different buffers)
__device__ __forceinline__ void dma_chunk(const uint8_t* src, uint32_t dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off nt\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(src), "s"(dst)
      : "memory");
}

// sconv4096::geometry: L / 8, halo / 8, hop / 8 in 16-byte chunks, and the segments per sequence; all below 2^23
struct geometry {
  int32_t chunks, halo, hop, segments;
};

// where a window's chunks outside the sequence come from
enum : int { kNoContext = 0, kHistory = 1, kFuture = 2 };

// cconv4096::load_window, statement by statement: window chunk j is source chunk ch = first + j; it comes in by LDS-DMA where ch lies
// in [lo, hi), every other slot is written with zeros. Inside [0, L / 8) the lane reads the sequence; outside, the context: kHistory
// for ch < 0, kFuture for ch >= L / 8 (ctx is the shifted base). The caller's [lo, hi) keeps a lane off a context that is not there.
template <int Ctx>
__device__ __forceinline__ void load_window(const uint16_t* in, uint64_t in_seq, const uint16_t* ctx, uint64_t ctx_seq, uint32_t rows,
                                            uint32_t channels, const geometry& geo, uint32_t p, uint32_t c, int32_t first, int32_t lo,
                                            int32_t hi, uint8_t* wl, uint32_t wl_off, int lane) {
  const bool has_im = 2 * p + 1 < rows;                  // wave-uniform
  const uint64_t seq = static_cast<uint64_t>(2 * p) * channels + c;
  const uint8_t* const src_re = reinterpret_cast<const uint8_t*>(in + seq * in_seq);
  const uint8_t* const src_im = src_re + 2 * static_cast<uint64_t>(channels) * in_seq;
  const uint8_t* const ctx_re = reinterpret_cast<const uint8_t*>(ctx + seq * ctx_seq);
  const uint8_t* const ctx_im = ctx_re + 2 * static_cast<uint64_t>(channels) * ctx_seq;
  const u4 zero = {0, 0, 0, 0};
#pragma unroll
  for (int mm = 0; mm < 8; ++mm) {
    const int32_t j = mm * 64 + (lane ^ (2 * mm));       // the window chunk slot `lane` of block mm holds
    const int32_t chunk = first + j;
    uint8_t* const slot = wl + mm * 1024 + lane * 16;
    if (chunk >= lo && chunk < hi) {
      const int64_t byte = static_cast<int64_t>(chunk) * 16;
      const bool outside = Ctx == kHistory ? chunk < 0 : Ctx == kFuture ? chunk >= geo.chunks : false;
      dma_chunk((outside ? ctx_re : src_re) + byte, wl_off + mm * 1024);
      if (has_im)
        dma_chunk((outside ? ctx_im : src_im) + byte, wl_off + 8192 + mm * 1024);
      else
        *reinterpret_cast<u4*>(slot + 8192) = zero;
    } else {
      *reinterpret_cast<u4*>(slot) = zero;
      *reinterpret_cast<u4*>(slot + 8192) = zero;
    }
  }
}

// One plane of a gated window through registers: gbconv4096::gated_plane with a signed range and a second pair of bases. Window
// chunk j is source chunk ch = first + j of the data AND of the gate, valid in [lo, hi): from `src` / `gate` for ch in [0, L / 8), from
// `csrc` / `cgate` (shifted bases) outside. A lane without a valid chunk loads chunk `spare` of the sequence (in [0, L / 8), read by
// the item anyway) and writes zero. issue() puts the 16 loads in flight, under no per-lane branch; finish() forms the products and
// writes them where the DMA would have written.
struct gated_plane {
  u4 xv[8], gv[8];

  // all ones where chunk lies in [lo, hi), else zero. Sign arithmetic on purpose: a comparison would be kept as a lane mask in an
  // SGPR pair per block between issue() and finish(), which the kernels do not have (gbconv4096::gated_plane::valid)
  static __device__ __forceinline__ uint32_t valid(int32_t chunk, int32_t lo, int32_t hi) {
    return static_cast<uint32_t>(~((chunk - lo) >> 31) & ((chunk - hi) >> 31));
  }

  template <int Ctx>
  __device__ __forceinline__ void issue(const uint8_t* src, const uint8_t* gate, const uint8_t* csrc, const uint8_t* cgate, const geometry& geo,
                                        int32_t first, int32_t lo, int32_t hi, int32_t spare, int lane) {
#pragma unroll
    for (int mm = 0; mm < 8; ++mm) {
      const int32_t chunk = first + (mm * 64 + (lane ^ (2 * mm)));     // the source chunk slot `lane` of block mm holds
      // the chunk this lane loads: its own where that is valid, else the spare one (inside the sequence)
      const int32_t ch = spare + static_cast<int32_t>(static_cast<uint32_t>(chunk - spare) & valid(chunk, lo, hi));
      if constexpr (Ctx == kNoContext) {
        const uint32_t off = static_cast<uint32_t>(ch) * 16u;          // below 2^27
        xv[mm] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(src + off));
        gv[mm] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(gate + off));
      } else {
        const bool outside = Ctx == kHistory ? ch < 0 : ch >= geo.chunks;
        const int64_t byte = static_cast<int64_t>(ch) * 16;
        xv[mm] = __builtin_nontemporal_load(reinterpret_cast<const u4*>((outside ? csrc : src) + byte));
        gv[mm] = __builtin_nontemporal_load(reinterpret_cast<const u4*>((outside ? cgate : gate) + byte));
      }
    }
  }
  __device__ __forceinline__ void finish(int32_t first, int32_t lo, int32_t hi, uint8_t* dst, int lane) const {
#pragma unroll
    for (int mm = 0; mm < 8; ++mm) {
      const int32_t chunk = first + (mm * 64 + (lane ^ (2 * mm)));
      const uint32_t keep = valid(chunk, lo, hi);
      const u4 prod = mul8(xv[mm], gv[mm]);
      *reinterpret_cast<u4*>(dst + mm * 1024 + lane * 16) = u4{prod.x & keep, prod.y & keep, prod.z & keep, prod.w & keep};   // the product or zero
    }
  }
};

__device__ __forceinline__ void zero_plane(uint8_t* dst, int lane) {
  const u4 zero = {0, 0, 0, 0};
#pragma unroll
  for (int mm = 0; mm < 8; ++mm) *reinterpret_cast<u4*>(dst + mm * 1024 + lane * 16) = zero;
}

// The gated window of pair p, channel c, whole: both planes one after the other, as gsconv4096::load_item<true> builds them. `in`
// and `gate` are indexed alike, each with its own sequence stride, and so are their contexts `ctx` and `cgate` (shifted bases);
// spare must lie in [0, L / 8).
template <int Ctx>
__device__ __forceinline__ void load_gated(const uint16_t* in, const uint16_t* gate, const uint16_t* ctx, const uint16_t* cgate, uint64_t in_seq,
                                           uint64_t gate_seq, uint64_t ctx_seq, uint64_t cgate_seq, uint32_t rows, uint32_t channels,
                                           const geometry& geo, uint32_t p, uint32_t c, int32_t first, int32_t lo, int32_t hi, int32_t spare,
                                           uint8_t* wl, int lane) {
  const bool has_im = 2 * p + 1 < rows;                  // wave-uniform
  const uint64_t seq = static_cast<uint64_t>(2 * p) * channels + c, im = 2 * static_cast<uint64_t>(channels);
  const uint8_t* const src_re = reinterpret_cast<const uint8_t*>(in + seq * in_seq);
  const uint8_t* const gate_re = reinterpret_cast<const uint8_t*>(gate + seq * gate_seq);
  const uint8_t* const ctx_re = reinterpret_cast<const uint8_t*>(ctx + seq * ctx_seq);
  const uint8_t* const cgate_re = reinterpret_cast<const uint8_t*>(cgate + seq * cgate_seq);
  // Whether this window reaches into the context at all is wave-uniform (only segment 0 reaches in front of sample 0, only the
  // last windows behind sample L): every other item takes the shipped load, one base and a 32-bit offset per lane, and pays nothing
  // for the second base. The branch is on the item, not on the lane: no load sits under a per-lane branch on either side.
  const bool reaches = Ctx == kHistory ? lo < 0 : Ctx == kFuture ? (hi > geo.chunks && first + 512 > geo.chunks) : false;
  if (reaches) {
    {
      gated_plane pl;
      pl.issue<Ctx>(src_re, gate_re, ctx_re, cgate_re, geo, first, lo, hi, spare, lane);
      pl.finish(first, lo, hi, wl, lane);
    }
    if (has_im) {
      gated_plane pl;
      pl.issue<Ctx>(src_re + im * in_seq, gate_re + im * gate_seq, ctx_re + im * ctx_seq, cgate_re + im * cgate_seq, geo, first, lo, hi, spare, lane);
      pl.finish(first, lo, hi, wl + 8192, lane);
    } else {
      zero_plane(wl + 8192, lane);
    }
  } else {
    {
      gated_plane pl;
      pl.issue<kNoContext>(src_re, gate_re, src_re, gate_re, geo, first, lo, hi, spare, lane);
      pl.finish(first, lo, hi, wl, lane);
    }
    if (has_im) {
      gated_plane pl;
      pl.issue<kNoContext>(src_re + im * in_seq, gate_re + im * gate_seq, src_re, gate_re, geo, first, lo, hi, spare, lane);
      pl.finish(first, lo, hi, wl + 8192, lane);
    } else {
      zero_plane(wl + 8192, lane);
    }
  }
}

// what the kernels share: the wave's constants and the stage code of sconv4096_kernel (gbconv4096::stages, statement by statement)
struct stages {
  h8 f_re, f_im;
  f4 tw_re, tw_im;
  const uint8_t *g_tab, *h_tab;
  uint8_t* tr_base;
  int m;

  __device__ __forceinline__ void init(const uint8_t* __restrict__ tables, const uint8_t* lds, uint8_t* wl, int lane) {
    using namespace k4096;
    f_re = *reinterpret_cast<const h8*>(tables + kOffF1 + lane * 32);
    f_im = *reinterpret_cast<const h8*>(tables + kOffF1 + lane * 32 + 16);
    tw_re = *reinterpret_cast<const f4*>(tables + kOffTw + lane * 32);
    tw_im = *reinterpret_cast<const f4*>(tables + kOffTw + lane * 32 + 16);
    g_tab = lds + lane * 16;
    h_tab = lds + 16384 + lane * 16;
    // transposed-read geometry of stage 1 (k4096.hpp)
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    m = q + 4 * (g & 1);
    const int bb = g >> 1;
    tr_base = wl + m * 1024 + bb * 512 + 8 * p;
  }

  // stage 1 on the wave's LDS image: conv4096_kernel's, statement by statement
  __device__ __forceinline__ void stage1(uint32_t (&pr)[8][4], uint32_t (&pi)[8][4]) const {
    using namespace k4096;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      f4 dre[2], dim[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int n1 = 2 * t + e;
        uint8_t* a = tr_base + 32 * (n1 ^ m);
        const s4 xr = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(a));
        const s4 xi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(a + 8192));
        const u4 raw = {__builtin_bit_cast(u2, xr).x, __builtin_bit_cast(u2, xr).y, __builtin_bit_cast(u2, xi).x, __builtin_bit_cast(u2, xi).y};
        const h8 x = __builtin_bit_cast(h8, raw);
        dre[e] = mfma(f_re, x);
        dim[e] = mfma(f_im, x);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pr[t][r] = pk(dre[0][r], dre[1][r]);
        pi[t][r] = pk(dim[0][r], dim[1][r]);
      }
    }
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        transpose4(pr[0 + pp][r], pr[2 + pp][r], pr[4 + pp][r], pr[6 + pp][r]);
        transpose4(pi[0 + pp][r], pi[2 + pp][r], pi[4 + pp][r], pi[6 + pp][r]);
      }
  }

  // stages 2 and 3: conv4096_kernel's, statement by statement
  template <class Mul, class Sink>
  __device__ __forceinline__ void stage23(uint32_t (&pr)[8][4], uint32_t (&pi)[8][4], Mul&& mul, Sink&& sink) const {
    using namespace k4096;
    auto tile23 = [&](int k0, f4& o_re, f4& o_im) {
      const int a = k0 >> 2, r = k0 & 3;
      const u4 araw = {pr[2 * a][r], pr[2 * a + 1][r], pi[2 * a][r], pi[2 * a + 1][r]};
      const h8 aop = __builtin_bit_cast(h8, araw);
      const u4 graw = *reinterpret_cast<const u4*>(g_tab + k0 * 1024);
      const f4 e_re = mfma(aop, __builtin_bit_cast(h8, graw));
      const f4 e_im = mfma(aop, im_form(graw));
      // scalar fp32 on purpose, see tile23 of k4096.hpp
      f4 t_re, t_im;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        t_re[r4] = __builtin_fmaf(e_re[r4], tw_re[r4], -(e_im[r4] * tw_im[r4]));
        t_im[r4] = __builtin_fmaf(e_re[r4], tw_im[r4], e_im[r4] * tw_re[r4]);
      }
      const u4 braw = {pk(t_re[0], t_re[1]), pk(t_re[2], t_re[3]), pk(t_im[0], t_im[1]), pk(t_im[2], t_im[3])};
      const h8 bop = __builtin_bit_cast(h8, braw);
      const u4 hraw = *reinterpret_cast<const u4*>(h_tab + k0 * 1024);
      o_re = mfma(__builtin_bit_cast(h8, hraw), bop);   // o[r2] = X[k0 + 16 k1 + 256 (4g + r2)]
      o_im = mfma(im_form(hraw), bop);
      mul(k0, o_re, o_im);
    };
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      uint32_t ore[4][4], oim[4][4];   // [r2][k0 pair within this half]
#pragma unroll
      for (int kp = 0; kp < 4; ++kp) {
        f4 e_re, e_im, o_re, o_im;
        tile23(8 * half + 2 * kp, e_re, e_im);
        tile23(8 * half + 2 * kp + 1, o_re, o_im);
#pragma unroll
        for (int r2 = 0; r2 < 4; ++r2) {
          ore[r2][kp] = pk(e_re[r2], o_re[r2]);
          oim[r2][kp] = pk(e_im[r2], o_im[r2]);
        }
      }
#pragma unroll
      for (int r2 = 0; r2 < 4; ++r2) {
        const u4 vr = {ore[r2][0], ore[r2][1], ore[r2][2], ore[r2][3]};
        const u4 vi = {oim[r2][0], oim[r2][1], oim[r2][2], oim[r2][3]};
        sink(half, r2, vr, vi);
      }
    }
  }

  // pass 0 of sconv4096_kernel on the image in LDS, with hre / him ([half][r2] vectors of 8 bins) as the filter: the spectrum / 4096
  // in fp32 times the filter * 4096, one rounding, back into the image with the planes exchanged
  __device__ __forceinline__ void pass0(const u4 (&hre)[2][4], const u4 (&him)[2][4], uint8_t* wl, int lane) const {
    const int g = lane >> 4;
    uint32_t pr[8][4], pi[8][4];
    stage1(pr, pi);
    stage23(
        pr, pi,
        [&](int k0, f4& o_re, f4& o_im) {
#pragma unroll
          for (int r2 = 0; r2 < 4; ++r2) {
            const float fr = static_cast<float>(__builtin_bit_cast(h8, hre[k0 >> 3][r2])[k0 & 7]) * 4096.f;
            const float fi = static_cast<float>(__builtin_bit_cast(h8, him[k0 >> 3][r2])[k0 & 7]) * 4096.f;
            const float zr = __builtin_fmaf(o_re[r2], fr, -(o_im[r2] * fi));
            o_im[r2] = __builtin_fmaf(o_re[r2], fi, o_im[r2] * fr);
            o_re[r2] = zr;
          }
        },
        [&](int half, int r2, u4 vr, u4 vi) {
          // chunk c = 2 k1 + half + 32 k2 of a plane: block mm = c >> 6 = 2 g + (r2 >> 1), slot (c & 63) ^ 2 mm
          const uint32_t mm = 2u * g + (r2 >> 1);
          const uint32_t cl = 2u * (lane & 15) + half + 32u * (r2 & 1);
          const uint32_t off = 1024u * mm + 16u * (cl ^ (2u * mm));
          *reinterpret_cast<u4*>(wl + 8192 + off) = vr;
          *reinterpret_cast<u4*>(wl + off) = vi;
        });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }

  // pass 1: the inverse transform, staged through the image (slot swizzle of kStageOut), planes exchanged back
  __device__ __forceinline__ void pass1(uint8_t* wl, int lane) const {
    const int g = lane >> 4;
    uint32_t pr[8][4], pi[8][4];
    stage1(pr, pi);
    stage23(pr, pi, [](int, f4&, f4&) {},
            [&](int half, int r2, u4 vr, u4 vi) {
              const uint32_t slot = 2u * (lane & 15) + half;
              const uint32_t off = 16u * (slot ^ ((slot >> 3) & 1)) + 512u * (4 * g + r2);
              *reinterpret_cast<u4*>(wl + 8192 + off) = vr;
              *reinterpret_cast<u4*>(wl + off) = vi;
            });
  }
};

// item -> (pair p, segment s, channel c): item = (p * segments + s) * channels + c, wave-uniform (sconv4096::split_item)
__device__ __forceinline__ void split_item(uint32_t it, uint32_t channels, const geometry& geo, uint32_t& p, int32_t& s, uint32_t& c) {
  const uint32_t q = it / channels;
  c = it - q * channels;
  p = q / static_cast<uint32_t>(geo.segments);
  s = static_cast<int32_t>(q - p * static_cast<uint32_t>(geo.segments));
}

// A kernel's arguments, read through the kernarg segment and opaque at every call: what is read through it is loaded (s_load) where
// it is used, per item, instead of being held in SGPRs across the whole loop. The kernels take up to eight SGPR pairs
// more than their shipped originals (two context bases, two context strides, and the bases they are selected against), which the
// instantiations with both gates do not have: held across the loop they push scalars into VGPRs, and the middle then spills at two
// waves per SIMD. T is the kernel's ONLY parameter, so it sits at offset 0 of the segment.
template <class T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* kernarg() {
  auto p = (const __attribute__((address_space(4))) T*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}

// the sequence strides of fwd_kernel, in halves
struct fwd_strides {
  uint64_t in, pre, hist, pre_hist, post, out;
};

// fwd_kernel's arguments. in / pre / post / out: as gsconv4096_kernel's. hist / pre_hist: the samples in front of in's / pre's, each
// with its own sequence stride, 8 * hist_chunks samples per sequence (hist_chunks = 0: never read); pre_hist is read only when Pre.
// items, item order, launch shape: gsconv4096_kernel's. The inputs, gates and contexts may alias each other.
struct fwd_params {
  const uint16_t *in, *pre, *hist, *pre_hist, *post;
  uint16_t* out;
  fwd_strides seq_of;
  uint32_t rows, channels;
  geometry geo;
  int32_t hist_chunks;
  uint32_t items, live;
  const uint8_t* tables;
  const uint16_t* filt;
};

// The order of events is gsconv4096_kernel's.
template <bool Pre, bool Post>
__global__ __launch_bounds__(k4096::kThreads, 2) void fwd_kernel(fwd_params P) {
  const uint32_t rows = P.rows, channels = P.channels, items = P.items, live = P.live;
  const geometry geo = P.geo;
  const uint8_t* __restrict__ const tables = P.tables;
  const uint16_t* __restrict__ const filt = P.filt;
  using namespace k4096;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  uint8_t* const wl = lds + kLdsTableBytes + wave * kLdsWaveBytes;
  const uint32_t wl_off = __builtin_amdgcn_readfirstlane(
      static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)wl)));

  // live waves and the stride over the items: as conv4096_kernel
  const uint32_t stride_b = gridDim.x * live;
  uint32_t b = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave) < live ? blockIdx.x * live + wave : items);

  for (int i = tid; i < kLdsTableBytes / 16; i += kThreads)
    reinterpret_cast<u4*>(lds)[i] = reinterpret_cast<const u4*>(tables + kOffG)[i];

  stages st8;
  st8.init(tables, lds, wl, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // table loads retired: vmcnt below counts only loop traffic
  __syncthreads();
  if (b >= items) return;

  // The order of events of gsconv4096_kernel: an item's image is built at the top of the loop, once the previous item's image has
  // been read out (the lgkmcnt(0) at the bottom), and the waits follow in straight-line code, so every path from an LDS-DMA to the
  // end of the program passes an s_waitcnt vmcnt(0) whatever shape the compiler gives the loop's latch.
  do {
    uint32_t pb, cb;
    int32_t sb;
    split_item(b, channels, geo, pb, sb, cb);
    const int32_t first = sb * geo.hop - geo.halo;       // source (and output) chunk of window chunk 0: negative in front of sample 0
    {
      const auto* const ka = kernarg<fwd_params>();      // the load end's arguments: live until the loads are issued
      const int32_t hist_chunks = ka->hist_chunks;
      // the contexts' bases, shifted so that source chunk ch of either buffer is base + 16 ch: the history's chunk Hn / 8 (ch = -1
      // is its last chunk). Never dereferenced outside [lo, hi) below.
      const uint16_t* const hist0 = ka->hist + 8 * static_cast<int64_t>(hist_chunks);
      // only segment 0 can reach in front of sample 0 (hop >= halo): every other item's lower end is the sequence's
      const int32_t lo = sb == 0 ? -hist_chunks : 0;
      if constexpr (Pre)
        load_gated<kHistory>(ka->in, ka->pre, hist0, ka->pre_hist + 8 * static_cast<int64_t>(hist_chunks), ka->seq_of.in, ka->seq_of.pre,
                             ka->seq_of.hist, ka->seq_of.pre_hist, rows, channels, geo, pb, cb, first, lo, geo.chunks, first > 0 ? first : 0, wl,
                             lane);
      else
        load_window<kHistory>(ka->in, ka->seq_of.in, hist0, ka->seq_of.hist, rows, channels, geo, pb, cb, first, lo, geo.chunks, wl, wl_off, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the item's DMA has landed (Pre: its loads are the compiler's to count) ...
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and so have its zero fill and products, before stage 1 reads them

    // this item's filter values: [half][r2] vectors of 8 bins, RE and IM (plain cached loads; they fly under stage 1)
    const uint16_t* const fimg = filt + static_cast<uint64_t>(cb) * 8192u + 8u * lane;
    u4 hre[2][4], him[2][4];
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int r2 = 0; r2 < 4; ++r2) {
        hre[half][r2] = *reinterpret_cast<const u4*>(fimg + (half * 4 + r2) * 512);
        him[half][r2] = *reinterpret_cast<const u4*>(fimg + 4096 + (half * 4 + r2) * 512);
      }

    // ---- pass 0: U / 4096 in fp32, times H' * 4096, one rounding, back into the image with the planes exchanged
    st8.pass0(hre, him, wl, lane);

    // the kept samples: window chunk j = 64 i + lane behind the halo, as long as its place in the sequence lies below L / 8
    const bool has_im = 2 * pb + 1 < rows;
    const uint64_t seq = static_cast<uint64_t>(2 * pb) * channels + cb;

    // Post: gsconv4096_kernel's store end, statement by statement. The RE plane's gate chunks are issued here so that they fly under
    // pass 1 (32 registers); the IM plane's are all issued behind pass 1, ahead of the RE plane's stores. No load sits under a
    // per-lane branch: a lane that stores nothing reads output chunk s * hop / 8 of the same gate sequence, which this item always
    // stores. The gate chunk is the OUTPUT chunk, not the window chunk.
    const auto* const kb = kernarg<fwd_params>();        // the store end's arguments
    const uint64_t post_seq = kb->seq_of.post, out_seq = kb->seq_of.out;
    const uint16_t* const g_re = kb->post + seq * post_seq;                                               // Post only
    const uint16_t* const g_im = g_re + static_cast<uint64_t>(channels) * post_seq;
    auto gate_off = [&](int i) {                                                                         // in halves, below 2^26
      const int32_t j = 64 * i + lane;
      const int32_t chunk = first + j;
      return static_cast<uint32_t>(j >= geo.halo && chunk < geo.chunks ? chunk : sb * geo.hop) * 8u;
    };
    u4 gate[8], gate_im[8];
    if constexpr (Post) {
#pragma unroll
      for (int i = 0; i < 8; ++i) gate[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(g_re + gate_off(i)));
    }

    // ---- pass 1: the inverse transform; staged through the image (slot swizzle of kStageOut), planes exchanged back
    st8.pass1(wl, lane);
    uint16_t* const y_re = kb->out + seq * out_seq;
    uint16_t* const y_im = y_re + static_cast<uint64_t>(channels) * out_seq;
    const uint32_t rd = 16u * (lane ^ ((lane >> 3) & 1));
    if constexpr (Post) {
      if (has_im) {
#pragma unroll
        for (int i = 0; i < 8; ++i) gate_im[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(g_im + gate_off(i)));
      } else {
        // never read; defined on this path too, so that the registers are not carried around the loop as the last item's
#pragma unroll
        for (int i = 0; i < 8; ++i) gate_im[i] = u4{0, 0, 0, 0};
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int32_t j = 64 * i + lane;
        const int32_t chunk = first + j;
        if (j >= geo.halo && chunk < geo.chunks) {
          const u4 vr = mul8(*reinterpret_cast<const u4*>(wl + 1024 * i + rd), gate[i]);
          st<kNonTemporal>(y_re + static_cast<int64_t>(chunk) * 8, vr);
        }
      }
      if (has_im) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int32_t j = 64 * i + lane;
          const int32_t chunk = first + j;
          if (j >= geo.halo && chunk < geo.chunks) {
            const u4 vi = mul8(*reinterpret_cast<const u4*>(wl + 8192 + 1024 * i + rd), gate_im[i]);
            st<kNonTemporal>(y_im + static_cast<int64_t>(chunk) * 8, vi);
          }
        }
      }
    } else {
      // sconv4096_kernel's store, statement by statement
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int32_t j = 64 * i + lane;
        const int32_t chunk = first + j;
        if (j >= geo.halo && chunk < geo.chunks) {
          const int64_t half_off = static_cast<int64_t>(chunk) * 8;
          const u4 vr = *reinterpret_cast<const u4*>(wl + 1024 * i + rd);
          st<kNonTemporal>(y_re + half_off, vr);
          if (has_im) {
            const u4 vi = *reinterpret_cast<const u4*>(wl + 8192 + 1024 * i + rd);
            st<kNonTemporal>(y_im + half_off, vi);
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next item's image is built
    b += stride_b;
  } while (b < items);
}

// the sequence strides of dgrad_kernel, in halves
struct dgrad_strides {
  uint64_t gy, post, fut, post_fut, x, pre, dx, dpre;
};

// dgrad_kernel's arguments. gy / post / x / pre / dx / dpre: as gbconv4096::dgrad_kernel's. fut / post_fut: the samples behind gy's /
// post's, each with its own sequence stride, 8 * fut_chunks samples per sequence (0: never read); post_fut is read only when Post.
// filt: conj(H').
struct dgrad_params {
  const uint16_t *gy, *post, *fut, *post_fut, *x, *pre;
  uint16_t *dx, *dpre;
  dgrad_strides seq_of;
  uint32_t rows, channels;
  geometry geo;
  int32_t fut_chunks;
  uint32_t items, live;
  const uint8_t* tables;
  const uint16_t* filt;
};

// The order of events is gbconv4096::dgrad_kernel's.
template <bool Pre, bool Post>
__global__ __launch_bounds__(k4096::kThreads, 2) void dgrad_kernel(dgrad_params P) {
  const uint32_t rows = P.rows, channels = P.channels, items = P.items, live = P.live;
  const geometry geo = P.geo;
  const uint8_t* __restrict__ const tables = P.tables;
  const uint16_t* __restrict__ const filt = P.filt;
  using namespace k4096;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  uint8_t* const wl = lds + kLdsTableBytes + wave * kLdsWaveBytes;
  const uint32_t wl_off = __builtin_amdgcn_readfirstlane(
      static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)wl)));

  const uint32_t stride_b = gridDim.x * live;
  uint32_t b = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave) < live ? blockIdx.x * live + wave : items);

  for (int i = tid; i < kLdsTableBytes / 16; i += kThreads)
    reinterpret_cast<u4*>(lds)[i] = reinterpret_cast<const u4*>(tables + kOffG)[i];

  stages st8;
  st8.init(tables, lds, wl, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // table loads retired: vmcnt below counts only loop traffic
  __syncthreads();
  if (b >= items) return;

  do {
    uint32_t pb, cb;
    int32_t sb;
    split_item(b, channels, geo, pb, sb, cb);
    const int32_t first = sb * geo.hop;                  // source (and output) chunk of window chunk 0: no front halo; below L / 8
    {
      const auto* const ka = kernarg<dgrad_params>();    // the load end's arguments: live until the loads are issued
      // the contexts' bases, shifted so that source chunk ch of either buffer is base + 16 ch: the future's chunk -L / 8 (ch = L / 8
      // is its first chunk). Never dereferenced outside [0, hi) below.
      const uint16_t* const fut0 = ka->fut - 8 * static_cast<int64_t>(geo.chunks);
      const int32_t hi = geo.chunks + ka->fut_chunks;
      if constexpr (Post)
        load_gated<kFuture>(ka->gy, ka->post, fut0, ka->post_fut - 8 * static_cast<int64_t>(geo.chunks), ka->seq_of.gy, ka->seq_of.post,
                            ka->seq_of.fut, ka->seq_of.post_fut, rows, channels, geo, pb, cb, first, 0, hi, first, wl, lane);
      else
        load_window<kFuture>(ka->gy, ka->seq_of.gy, fut0, ka->seq_of.fut, rows, channels, geo, pb, cb, first, 0, hi, wl, wl_off, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the item's DMA has landed (Post: its loads are the compiler's to count) ...
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and so have its zero fill and products, before stage 1 reads them

    // this item's filter values: [half][r2] vectors of 8 bins, RE and IM (plain cached loads; they fly under stage 1)
    const uint16_t* const fimg = filt + static_cast<uint64_t>(cb) * 8192u + 8u * lane;
    u4 hre[2][4], him[2][4];
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int r2 = 0; r2 < 4; ++r2) {
        hre[half][r2] = *reinterpret_cast<const u4*>(fimg + (half * 4 + r2) * 512);
        him[half][r2] = *reinterpret_cast<const u4*>(fimg + 4096 + (half * 4 + r2) * 512);
      }
    st8.pass0(hre, him, wl, lane);

    // the kept samples: window chunk j = 64 i + lane below hop / 8, as long as its place in the sequence lies below L / 8
    const bool has_im = 2 * pb + 1 < rows;
    const uint64_t seq = static_cast<uint64_t>(2 * pb) * channels + cb;
    const uint32_t rd = 16u * (lane ^ ((lane >> 3) & 1));
    const auto* const kb = kernarg<dgrad_params>();      // the store end's arguments
    const uint16_t *const x = kb->x, *const pre = kb->pre;
    uint16_t *const dx = kb->dx, *const dpre = kb->dpre;
    const struct { uint64_t x, pre, dx, dpre; } seq_of = {kb->seq_of.x, kb->seq_of.pre, kb->seq_of.dx, kb->seq_of.dpre};

    if constexpr (Pre) {
      // gbconv4096::dgrad_kernel's store end, statement by statement. The gate chunk is the OUTPUT chunk. A lane that stores nothing
      // reads output chunk s * hop / 8, which this item always stores. kept: the staged chunks this item stores, in one per-item scalar
      const int32_t kept = geo.hop < geo.chunks - first ? geo.hop : geo.chunks - first;                  // >= 1
      auto gate_off = [&](int i) {                                                                       // in halves, below 2^26
        const int32_t j = 64 * i + lane;
        return static_cast<uint32_t>(first + (j < kept ? j : 0)) * 8u;
      };
      const uint16_t* const p_re = pre + seq * seq_of.pre;
      const uint16_t* const p_im = p_re + static_cast<uint64_t>(channels) * seq_of.pre;
      const uint16_t* const x_re = x + seq * seq_of.x;                                                   // read only when dpre
      const uint16_t* const x_im = x_re + static_cast<uint64_t>(channels) * seq_of.x;
      uint16_t* const dx_re = dx + seq * seq_of.dx;
      uint16_t* const dx_im = dx_re + static_cast<uint64_t>(channels) * seq_of.dx;
      // dpre's two sequences as offsets in halves: the pointers are formed only where dpre is not null
      const uint64_t dp_re = seq * seq_of.dpre, dp_im = dp_re + static_cast<uint64_t>(channels) * seq_of.dpre;
      const bool want_dpre = dpre != nullptr;            // wave-uniform: a kernel argument

      st8.pass1(wl, lane);
      asm volatile("" ::: "memory");                     // nothing below is hoisted into pass 1

      // Everything the stores need comes in behind pass 1, a plane at a time: the chunks of pre and of x, 64 registers, ahead of
      // the plane's stores. The middle leaves no room for more at two waves per SIMD.
      u4 gate[8], xg[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) gate[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(p_re + gate_off(i)));
      if (want_dpre) {
#pragma unroll
        for (int i = 0; i < 8; ++i) xg[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(x_re + gate_off(i)));
      } else {
        // never read; defined on this path too, so that the registers are not carried around the loop as the last item's
#pragma unroll
        for (int i = 0; i < 8; ++i) xg[i] = u4{0, 0, 0, 0};
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int32_t j = 64 * i + lane;
        if (j < kept) {
          const u4 vr = *reinterpret_cast<const u4*>(wl + 1024 * i + rd);
          st<kNonTemporal>(dx_re + static_cast<int64_t>(first + j) * 8, mul8(vr, gate[i]));
          if (want_dpre) st<kNonTemporal>(dpre + dp_re + static_cast<int64_t>(first + j) * 8, mul8(vr, xg[i]));
        }
      }
      if (has_im) {
        asm volatile("" ::: "memory");                   // the IM plane's loads stay behind the RE plane's stores
#pragma unroll
        for (int i = 0; i < 8; ++i) gate[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(p_im + gate_off(i)));
        if (want_dpre) {
#pragma unroll
          for (int i = 0; i < 8; ++i) xg[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(x_im + gate_off(i)));
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const int32_t j = 64 * i + lane;
          if (j < kept) {
            const u4 vi = *reinterpret_cast<const u4*>(wl + 8192 + 1024 * i + rd);
            st<kNonTemporal>(dx_im + static_cast<int64_t>(first + j) * 8, mul8(vi, gate[i]));
            if (want_dpre) st<kNonTemporal>(dpre + dp_im + static_cast<int64_t>(first + j) * 8, mul8(vi, xg[i]));
          }
        }
      }
    } else {
      st8.pass1(wl, lane);
      // bconv4096::dgrad_kernel's store, statement by statement
      uint16_t* const y_re = dx + seq * seq_of.dx;
      uint16_t* const y_im = y_re + static_cast<uint64_t>(channels) * seq_of.dx;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int32_t j = 64 * i + lane;
        const int32_t chunk = first + j;
        if (j < geo.hop && chunk < geo.chunks) {
          const int64_t half_off = static_cast<int64_t>(chunk) * 8;
          const u4 vr = *reinterpret_cast<const u4*>(wl + 1024 * i + rd);
          st<kNonTemporal>(y_re + half_off, vr);
          if (has_im) {
            const u4 vi = *reinterpret_cast<const u4*>(wl + 8192 + 1024 * i + rd);
            st<kNonTemporal>(y_im + half_off, vi);
          }
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next item's image is built
    b += stride_b;
  } while (b < items);
}

// wgrad_kernel runs in workgroups of FOUR waves, one per SIMD, as bconv4096::wgrad_kernel does and for its reason.
constexpr int kWgradWaves = 4;
constexpr int kWgradThreads = 64 * kWgradWaves;
constexpr int kWgradLdsBytes = k4096::kLdsTableBytes + kWgradWaves * k4096::kLdsWaveBytes;

// the sequence strides of wgrad_kernel, in halves
struct wgrad_strides {
  uint64_t x, pre, hist, pre_hist, gy, post;
};

// wgrad_kernel's arguments. x / pre / gy / post / units / per_channel / kchunks / ws: as gbconv4096::wgrad_kernel's. hist / pre_hist:
// the samples in front of x's / pre's, 8 * hist_chunks each (0: never read); pre_hist is read only when Pre. The gz window has no
// context.
struct wgrad_params {
  const uint16_t *x, *pre, *hist, *pre_hist, *gy, *post;
  wgrad_strides seq_of;
  uint32_t rows, channels;
  geometry geo;
  int32_t hist_chunks;
  uint32_t partials, per_channel, units, live;
  int32_t kchunks;
  uint32_t kpad;
  const uint8_t* tables;
  float* ws;
};

template <bool Pre, bool Post>
__global__ __launch_bounds__(kWgradThreads, 1) void wgrad_kernel(wgrad_params P) {
  const uint32_t rows = P.rows, channels = P.channels, partials = P.partials, per_channel = P.per_channel, units = P.units, live = P.live;
  const uint32_t kpad = P.kpad;
  const int32_t kchunks = P.kchunks;
  const geometry geo = P.geo;
  const uint8_t* __restrict__ const tables = P.tables;
  float* __restrict__ const ws = P.ws;
  using namespace k4096;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  uint8_t* const wl = lds + kLdsTableBytes + wave * kLdsWaveBytes;
  const uint32_t wl_off = __builtin_amdgcn_readfirstlane(
      static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)wl)));

  const uint32_t u = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave) < live ? blockIdx.x * live + wave : units);

  for (int i = tid; i < kLdsTableBytes / 16; i += kWgradThreads)
    reinterpret_cast<u4*>(lds)[i] = reinterpret_cast<const u4*>(tables + kOffG)[i];

  stages st8;
  st8.init(tables, lds, wl, lane);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // table loads retired: vmcnt below counts only loop traffic
  __syncthreads();
  if (u >= units) return;

  const uint32_t q = u / channels, c = u - q * channels;
  const uint32_t rd = 16u * (lane ^ ((lane >> 3) & 1));
  float acc[4][8], last = 0.f;     // taps 8 (64 i + lane) .. + 7, and tap 2048 (chunk 256, the same value in every lane)
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;

  uint32_t it = q;                 // q < partials <= per_channel: every unit has a first item
  do {
    const uint32_t p = it / static_cast<uint32_t>(geo.segments);
    const int32_t s = static_cast<int32_t>(it - p * static_cast<uint32_t>(geo.segments));
    const int32_t first = s * geo.hop - geo.halo;        // source chunk of window chunk 0: negative in front of sample 0
    const int32_t own = s * geo.hop;                     // the first source chunk that belongs to this segment; below L / 8
    const bool has_im = 2 * p + 1 < rows;                // wave-uniform
    // the image's LDS address, opaque per item: as a loop invariant the compiler keeps wl_off + 1024 mm, the 16 DMA destinations,
    // in SGPRs across the whole loop, which the gated instantiations do not have
    uint32_t wl_item = wl_off;
    if constexpr (!Pre || !Post) asm volatile("" : "+s"(wl_item));      // with both gates no window comes in by DMA

    // ---- (a) the ue = pe (.) xe window through stages 1 - 3; what the sink receives is kept as the filter registers of (c):
    // conj(fp16(Zu / 4096))
    {
      const auto* const ka = kernarg<wgrad_params>();    // this window's arguments: live until its loads are issued
      const int32_t hist_chunks = ka->hist_chunks;
      const int32_t lo = s == 0 ? -hist_chunks : 0;      // only segment 0 can reach into the history
      // source chunk 0 of the histories: one behind their last
      const uint16_t* const hist0 = ka->hist + 8 * static_cast<int64_t>(hist_chunks);
      if constexpr (Pre)
        load_gated<kHistory>(ka->x, ka->pre, hist0, ka->pre_hist + 8 * static_cast<int64_t>(hist_chunks), ka->seq_of.x, ka->seq_of.pre,
                             ka->seq_of.hist, ka->seq_of.pre_hist, rows, channels, geo, p, c, first, lo, geo.chunks, first > 0 ? first : 0, wl,
                             lane);
      else
        load_window<kHistory>(ka->x, ka->seq_of.x, hist0, ka->seq_of.hist, rows, channels, geo, p, c, first, lo, geo.chunks, wl, wl_item, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    u4 hre[2][4], him[2][4];
    {
      uint32_t pr[8][4], pi[8][4];
      st8.stage1(pr, pi);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // stage 1 has read the image out ...
      // ---- (b) ... so the gz window may come in under stages 2 and 3, which read the tables only. Its first halo samples belong
      // to segment s - 1 (or, in segment 0, to the chunk before this one): zero below source chunk first + halo = s * hop. Post:
      // the loads of both planes fly under the stages in registers, and the products are written behind them
      auto keep = [&](int half, int r2, u4 vr, u4 vi) {
        hre[half][r2] = vr;
        him[half][r2] = u4{vi.x ^ 0x80008000u, vi.y ^ 0x80008000u, vi.z ^ 0x80008000u, vi.w ^ 0x80008000u};
      };
      const auto* const kb = kernarg<wgrad_params>();    // the gz window's arguments
      const uint16_t* const gy = kb->gy;
      const struct { uint64_t gy, post; } seq_of = {kb->seq_of.gy, kb->seq_of.post};
      if constexpr (Post) {
        const uint64_t seq = static_cast<uint64_t>(2 * p) * channels + c;
        const uint8_t* const src_re = reinterpret_cast<const uint8_t*>(gy + seq * seq_of.gy);
        const uint8_t* const gate_re = reinterpret_cast<const uint8_t*>(kb->post + seq * seq_of.post);
        gated_plane re_pl, im_pl;
        re_pl.issue<kNoContext>(src_re, gate_re, src_re, gate_re, geo, first, own, geo.chunks, own, lane);
        if (has_im) {
          const uint8_t* const src_im = src_re + 2 * static_cast<uint64_t>(channels) * seq_of.gy;
          const uint8_t* const gate_im = gate_re + 2 * static_cast<uint64_t>(channels) * seq_of.post;
          im_pl.issue<kNoContext>(src_im, gate_im, src_im, gate_im, geo, first, own, geo.chunks, own, lane);
        }
        st8.stage23(pr, pi, [](int, f4&, f4&) {}, keep);
        re_pl.finish(first, own, geo.chunks, wl, lane);
        if (has_im)
          im_pl.finish(first, own, geo.chunks, wl + 8192, lane);
        else
          zero_plane(wl + 8192, lane);
      } else {
        load_window<kNoContext>(gy, seq_of.gy, gy, seq_of.gy, rows, channels, geo, p, c, first, own, geo.chunks, wl, wl_item, lane);
        st8.stage23(pr, pi, [](int, f4&, f4&) {}, keep);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- (c) (d) sconv's two passes on the gz window
    st8.pass0(hre, him, wl, lane);
    st8.pass1(wl, lane);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the staged result is in the image

    // ---- (e) lags 0 .. K - 1 of the RE plane, chunk 64 i + lane, added in fp32. The test is on the block of 64 chunks, which is
    // wave-uniform: the lanes behind chunk ceil(K / 8) - 1 of the last block add lags >= K, sums that are never written out
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (64 * i < kchunks) {
        const h8 v = __builtin_bit_cast(h8, *reinterpret_cast<const u4*>(wl + 1024 * i + rd));
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] += static_cast<float>(v[e]);
      }
    }
    if (kchunks > 256) last += static_cast<float>(*reinterpret_cast<const _Float16*>(wl + 4096));   // chunk 256: block 4, slot 0
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next item's image is built
    it += partials;
  } while (it < per_channel);

  float* const part = ws + (static_cast<uint64_t>(c) * partials + q) * kpad;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int32_t j = 64 * i + lane;
    if (j < kchunks) {
      *reinterpret_cast<f4*>(part + 8 * j) = f4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
      *reinterpret_cast<f4*>(part + 8 * j + 4) = f4{acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
    }
  }
  if (kchunks > 256 && lane == 0) part[2048] = last;
}

// gbconv4096::wreduce_kernel: dh[c][j] = 4096 * (sum of the partials of tap j of channel c in increasing q), one thread per (c, j);
// the thread of tap 0 also writes dskip[c], the same bits, when dskip is not null.
__global__ __launch_bounds__(256) void wreduce_kernel(const float* __restrict__ ws, float* __restrict__ dh, float* __restrict__ dskip,
                                                       uint32_t channels, uint32_t taps, uint32_t partials, uint32_t kpad) {
  const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= static_cast<uint64_t>(channels) * taps) return;
  const uint32_t c = static_cast<uint32_t>(idx / taps), j = static_cast<uint32_t>(idx - static_cast<uint64_t>(c) * taps);
  const float* src = ws + static_cast<uint64_t>(c) * partials * kpad + j;
  float sum = src[0];
  for (uint32_t q = 1; q < partials; ++q) sum += src[static_cast<uint64_t>(q) * kpad];
  sum *= 4096.f;
  dh[idx] = sum;
  if (dskip && j == 0) dskip[c] = sum;
}

}  // namespace gcconv4096
