// cconv4096.hpp — the overlap-save causal convolution (sconv/sconv4096.hpp) and its two gradients (bconv/bconv4096.hpp) for gfx950
// with CONTEXT carried across chunks of a longer sequence: the forward and the tap-gradient windows may reach up to Hn samples in
// front of sample 0 into a `history`, the input-gradient windows up to Fn samples behind sample L into a `future`. The middle is
// those kernels', statement by statement (same tables, same three MFMA stages twice, same fp32 filter multiply with its one
// rounding, same filter image in conv4096::filter_slot order, same exchanged-plane write-back and stage-out swizzle, same launch
// shapes and order of events); only the load ends are re-indexed:
//
//   cconv4096_kernel  window chunk j of item (p, s, c) is source chunk ch = s * hop / 8 - halo / 8 + j, SIGNED: ch in [0, L / 8) comes
//                     from the sequence, ch in [-Hn / 8, 0) from chunk ch + Hn / 8 of the history, every other slot is zero fill.
//   dgrad_kernel      window chunk j is source chunk ch = s * hop / 8 + j: ch in [0, L / 8) from g, ch in [L / 8, (L + Fn) / 8) from
//                     chunk ch - L / 8 of the future, zero fill at or behind that.
//   wgrad_kernel      the x window as cconv4096_kernel loads it; the g window as bconv4096::wgrad_kernel loads it (no context: the
//                     tap gradient sums over the g of this chunk only).
//   wreduce_kernel    bconv4096::wreduce_kernel.
//
// A block of 64 slots takes ONE LDS-DMA per plane as before: an LDS-DMA takes a per-lane source address, so "outside the sequence
// but inside the context" is a select on that address (the context's base is handed in shifted, so that both sources are
// base + 16 * ch), not a second load. Hn / 8 and Fn / 8 arrive as 0 when the caller passed no context: nothing outside [0, L) of a
// sequence and [0, Hn) or [0, Fn) of a context is ever read. Only segment 0 has ch < 0 (hop >= halo), and only windows that reach
// sample L have ch >= L / 8; every other item takes the sequence's address in every lane. Stores are those of the originals.
//
// The stage code is restated on the k4096 helpers, as sconv4096.hpp and bconv4096.hpp restate it and for their reason: the code
// generation of the shipped kernels is untouched.
#pragma once

#include "../csrc/k4096.hpp"

namespace cconv4096 {

using k4096::f4;
using k4096::h8;
using k4096::s4;
using k4096::u2;
using k4096::u4;

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

// Builds a window of pair p, channel c in the wave's LDS region: bconv4096::load_window with a second source. Window chunk j is
// source chunk ch = first + j; it comes in by LDS-DMA where ch lies in [lo, hi), every other slot is written with zeros. Inside
// [0, L / 8) the lane reads the sequence; outside, the context: kHistory for ch < 0 (ctx is the history's chunk Hn / 8, so that
// ch = -1 is its last chunk), kFuture for ch >= L / 8 (ctx is the future's chunk -L / 8). The caller's [lo, hi) is what keeps a
// lane off a context that is not there: [0, L / 8) without one. lo and hi are per-item scalars and the tests are on the chunk
// (the slots are swizzled), as in load_window and for its reason. A zero partner's plane is all fill.
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

// what the kernels share: the wave's constants and the stage code of sconv4096_kernel, cut behind stage 1 so that wgrad_kernel can
// issue its second window's loads between the two halves (bconv4096::stages, statement by statement)
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

  // pass 0 and pass 1 of sconv4096_kernel on the image in LDS, with hre / him ([half][r2] vectors of 8 bins) as the filter: the
  // spectrum / 4096 in fp32 times the filter * 4096, one rounding, back into the image with the planes exchanged; then the inverse
  // transform, staged through the image (slot swizzle of kStageOut), planes exchanged back
  __device__ __forceinline__ void convolve(const u4 (&hre)[2][4], const u4 (&him)[2][4], uint8_t* wl, int lane) const {
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

// One kernel body for the forward pass and the input gradient, which differ in their two ends only (sconv4096_kernel and
// bconv4096::dgrad_kernel): Ctx = kHistory: the window starts at s * hop - halo, reaches into ctx in front of sample 0 and keeps the
// chunks j >= halo; Ctx = kFuture: the window starts at s * hop, reaches into ctx at and behind sample L and keeps the chunks
// j < hop. ctx_chunks = Hn / 8 or Fn / 8, 0 when there is no context (ctx is then never read).
template <int Ctx>
__device__ __forceinline__ void conv_body(const uint16_t* in, const uint16_t* ctx, uint16_t* out, uint64_t in_seq, uint64_t ctx_seq,
                                          uint64_t out_seq, uint32_t rows, uint32_t channels, const geometry& geo, int32_t ctx_chunks,
                                          uint32_t items, uint32_t live, const uint8_t* __restrict__ tables,
                                          const uint16_t* __restrict__ filt) {
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

  // the context's base, shifted so that source chunk ch of either buffer is base + 16 ch: the history's chunk Hn / 8 (ch = -1 is
  // its last chunk), the future's chunk -L / 8 (ch = L / 8 is its first). Never dereferenced outside [lo, hi) below.
  const uint16_t* const ctx0 = Ctx == kHistory ? ctx + 8 * static_cast<int64_t>(ctx_chunks) : ctx - 8 * static_cast<int64_t>(geo.chunks);

  // The order of events of sconv4096_kernel: an item's zero fill and DMA are issued once the previous item's image has been read
  // out (the lgkmcnt(0) at the bottom), they fly under that item's stores, and the waits follow in straight-line code, so every
  // path from an LDS-DMA to the end of the program passes an s_waitcnt vmcnt(0) whatever shape the compiler gives the loop's latch.
  do {
    uint32_t pb, cb;
    int32_t sb;
    split_item(b, channels, geo, pb, sb, cb);
    // source (and output) chunk of window chunk 0: negative in front of sample 0
    const int32_t first = Ctx == kHistory ? sb * geo.hop - geo.halo : sb * geo.hop;
    // only segment 0 can reach in front of sample 0 (hop >= halo): every other item's lower end is today's
    const int32_t lo = Ctx == kHistory && sb == 0 ? -ctx_chunks : 0;
    const int32_t hi = Ctx == kFuture ? geo.chunks + ctx_chunks : geo.chunks;
    load_window<Ctx>(in, in_seq, ctx0, ctx_seq, rows, channels, geo, pb, cb, first, lo, hi, wl, wl_off, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the item's DMA has landed ...
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and so has its zero fill, before stage 1 reads either

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
    st8.convolve(hre, him, wl, lane);

    // the kept samples: window chunk j = 64 i + lane behind the halo (forward) or below hop / 8 (input gradient), as long as its
    // place in the sequence lies below L / 8
    const bool has_im = 2 * pb + 1 < rows;
    uint16_t* const y_re = out + (static_cast<uint64_t>(2 * pb) * channels + cb) * out_seq;
    uint16_t* const y_im = y_re + static_cast<uint64_t>(channels) * out_seq;
    const uint32_t rd = 16u * (lane ^ ((lane >> 3) & 1));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int32_t j = 64 * i + lane;
      const int32_t chunk = first + j;
      if ((Ctx == kHistory ? j >= geo.halo : j < geo.hop) && chunk < geo.chunks) {
        const int64_t half_off = static_cast<int64_t>(chunk) * 8;
        const u4 vr = *reinterpret_cast<const u4*>(wl + 1024 * i + rd);
        st<kNonTemporal>(y_re + half_off, vr);
        if (has_im) {
          const u4 vi = *reinterpret_cast<const u4*>(wl + 8192 + 1024 * i + rd);
          st<kNonTemporal>(y_im + half_off, vi);
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next item's zero fill and DMA
    b += stride_b;
  } while (b < items);
}

// in / out: real binary16, sequence (b, c) at + (b * channels + c) * seq stride halves, 8 * geo.chunks samples each; hist: the
// same layout with hist_seq, 8 * hist_chunks samples each (hist_chunks = 0: never read). items, item order and launch shape:
// sconv4096_kernel's. filt: filter images as conv4096_kernel takes them, channel c at + c * 8192 halves.
__global__ __launch_bounds__(k4096::kThreads, 2) void cconv4096_kernel(
    const uint16_t* in, const uint16_t* hist, uint16_t* out, uint64_t in_seq, uint64_t hist_seq, uint64_t out_seq, uint32_t rows,
    uint32_t channels, geometry geo, int32_t hist_chunks, uint32_t items, uint32_t live, const uint8_t* __restrict__ tables,
    const uint16_t* __restrict__ filt) {
  conv_body<kHistory>(in, hist, out, in_seq, hist_seq, out_seq, rows, channels, geo, hist_chunks, items, live, tables, filt);
}

// g / dx as bconv4096::dgrad_kernel's; fut: the samples behind g's, fut_seq apart, 8 * fut_chunks each (0: never read). filt: conj(H).
__global__ __launch_bounds__(k4096::kThreads, 2) void dgrad_kernel(
    const uint16_t* in, const uint16_t* fut, uint16_t* out, uint64_t in_seq, uint64_t fut_seq, uint64_t out_seq, uint32_t rows,
    uint32_t channels, geometry geo, int32_t fut_chunks, uint32_t items, uint32_t live, const uint8_t* __restrict__ tables,
    const uint16_t* __restrict__ filt) {
  conv_body<kFuture>(in, fut, out, in_seq, fut_seq, out_seq, rows, channels, geo, fut_chunks, items, live, tables, filt);
}

// wgrad_kernel runs in workgroups of FOUR waves, one per SIMD, as bconv4096::wgrad_kernel and for its reason.
constexpr int kWgradWaves = 4;
constexpr int kWgradThreads = 64 * kWgradWaves;
constexpr int kWgradLdsBytes = k4096::kLdsTableBytes + kWgradWaves * k4096::kLdsWaveBytes;

// x / g / units / per_channel / kchunks / ws: as bconv4096::wgrad_kernel. hist: the samples in front of x's, hist_seq apart,
// 8 * hist_chunks each (0: never read); the g window has no context.
__global__ __launch_bounds__(kWgradThreads, 1) void wgrad_kernel(
    const uint16_t* x, const uint16_t* hist, const uint16_t* gr, uint64_t x_seq, uint64_t hist_seq, uint64_t g_seq, uint32_t rows,
    uint32_t channels, geometry geo, int32_t hist_chunks, uint32_t partials, uint32_t per_channel, uint32_t units, uint32_t live,
    int32_t kchunks, uint32_t kpad, const uint8_t* __restrict__ tables, float* __restrict__ ws) {
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
  const uint16_t* const hist0 = hist + 8 * static_cast<int64_t>(hist_chunks);      // source chunk 0 of the history: one behind its last

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

    // ---- (a) the x window through stages 1 - 3; what the sink receives is kept as the filter registers of (c): conj(fp16(Zx / 4096)).
    // Only segment 0 can reach into the history.
    load_window<kHistory>(x, x_seq, hist0, hist_seq, rows, channels, geo, p, c, first, s == 0 ? -hist_chunks : 0, geo.chunks, wl, wl_off,
                          lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    u4 hre[2][4], him[2][4];
    {
      uint32_t pr[8][4], pi[8][4];
      st8.stage1(pr, pi);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // stage 1 has read the image out ...
      // ---- (b) ... so the g window may come in under stages 2 and 3, which read the tables only. Its first halo samples belong
      // to segment s - 1 (or, in segment 0, to the chunk before this one): zero fill below source chunk first + halo = s * hop
      load_window<kNoContext>(gr, g_seq, gr, g_seq, rows, channels, geo, p, c, first, s * geo.hop, geo.chunks, wl, wl_off, lane);
      st8.stage23(pr, pi, [](int, f4&, f4&) {},
                  [&](int half, int r2, u4 vr, u4 vi) {
                    hre[half][r2] = vr;
                    him[half][r2] = u4{vi.x ^ 0x80008000u, vi.y ^ 0x80008000u, vi.z ^ 0x80008000u, vi.w ^ 0x80008000u};
                  });
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- (c) (d) sconv's two passes on the g window
    st8.convolve(hre, him, wl, lane);
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
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next item's zero fill and DMA
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

// dh[c][j] = 4096 * (sum of the partials of tap j of channel c in increasing q), one thread per (c, j): bconv4096::wreduce_kernel
__global__ __launch_bounds__(256) void wreduce_kernel(const float* __restrict__ ws, float* __restrict__ dh, uint32_t channels, uint32_t taps,
                                                       uint32_t partials, uint32_t kpad) {
  const uint64_t idx = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (idx >= static_cast<uint64_t>(channels) * taps) return;
  const uint32_t c = static_cast<uint32_t>(idx / taps), j = static_cast<uint32_t>(idx - static_cast<uint64_t>(c) * taps);
  const float* src = ws + static_cast<uint64_t>(c) * partials * kpad + j;
  float sum = src[0];
  for (uint32_t q = 1; q < partials; ++q) sum += src[static_cast<uint64_t>(q) * kpad];
  dh[idx] = sum * 4096.f;
}

}  // namespace cconv4096
