// lconv4096.hpp — fused causal convolution of REAL sequences at transform length 4096 for gfx950: the arithmetic of
// conv/conv4096.hpp (same tables, same three MFMA stages twice, same fp32 filter multiply with its one rounding, same filter image
// in conv4096::filter_slot order), with the two ends of the kernel made for zero-padded real data:
//
//   load    sequences (2p, c) and (2p + 1, c), L = 8 * chunks halves each, are the RE and the IM plane of one complex signal. The
//           wave builds the image k4096::dma_in<true> would leave for the zero-padded signal (slot l of 1-KiB block mm holds
//           16-byte chunk l ^ 2 mm of the plane): chunks below L / 8 come in by LDS-DMA, every other slot of both planes is
//           written with zeros (ds_write_b128). The padding never travels through HBM, and nothing beyond sample L of a
//           sequence is read. An odd number of rows pairs its last row with zeros: that plane is all zero fill.
//   store   of the staged result only the 16-byte chunks below L / 8 are written, RE plane to (2p, c), IM plane to (2p + 1, c)
//           where that row exists.
//
// The zero fill is per item: pass 0 and the output staging overwrite the whole image, so what the previous item left behind is
// never zero. The stage code is restated on the k4096 helpers, as conv4096.hpp restates it, so that the code generation of the
// shipped kernels is untouched.
#pragma once

#include "../csrc/k4096.hpp"

namespace lconv4096 {

using k4096::f4;
using k4096::h8;
using k4096::s4;
using k4096::u2;
using k4096::u4;

// one plane's share of 1-KiB block mm by LDS-DMA, nt (the statement of k4096::dma_in for a single plane; called under the
// lanes' own predicate: M0 is written by the scalar unit whatever the mask, the load obeys it, and lane l's 16 bytes land at
// dst + 16 l whichever other lanes are off)
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

// Builds the image of item `it` in the wave's LDS region. The zero writes and the DMA touch disjoint slots; both are retired by
// the s_waitcnt vmcnt(0) / lgkmcnt(0) that follow it in the kernel's loop, one phase before stage 1 reads the image.
__device__ __forceinline__ void load_item(const uint16_t* in, uint64_t in_seq, uint32_t rows, uint32_t channels, uint32_t chunks,
                                          uint32_t it, uint8_t* wl, uint32_t wl_off, int lane) {
  const uint32_t p = it / channels, c = it - p * channels;
  const bool has_im = 2 * p + 1 < rows;                  // wave-uniform
  const uint8_t* const src_re = reinterpret_cast<const uint8_t*>(in + (static_cast<uint64_t>(2 * p) * channels + c) * in_seq);
  const uint8_t* const src_im = src_re + 2 * static_cast<uint64_t>(channels) * in_seq;
  const u4 zero = {0, 0, 0, 0};
#pragma unroll
  for (int mm = 0; mm < 8; ++mm) {
    const uint32_t chunk = static_cast<uint32_t>(mm * 64 + (lane ^ (2 * mm)));     // the chunk slot `lane` of block mm holds
    uint8_t* const slot = wl + mm * 1024 + lane * 16;
    // The test is on the chunk, not the lane: the slots are swizzled. A block wholly beyond L has no lane left in the first
    // branch, which the wave then skips as a whole: no DMA is issued for it.
    if (chunk < chunks) {
      dma_chunk(src_re + chunk * 16u, wl_off + mm * 1024);
      if (has_im)
        dma_chunk(src_im + chunk * 16u, wl_off + 8192 + mm * 1024);
      else
        *reinterpret_cast<u4*>(slot + 8192) = zero;
    } else {
      *reinterpret_cast<u4*>(slot) = zero;
      *reinterpret_cast<u4*>(slot + 8192) = zero;
    }
  }
}

// in / out: real binary16, sequence (b, c) at + (b * channels + c) * seq stride halves, 8 * chunks samples each. items =
// ceil(rows / 2) * channels, item p * channels + c. tables: the first k4096::kOffF1n bytes of a k4096::build_tables() blob.
// filt: filter images as conv4096_kernel takes them, channel c at + c * 8192 halves.
__global__ __launch_bounds__(k4096::kThreads, 2) void lconv4096_kernel(
    const uint16_t* in, uint16_t* out, uint64_t in_seq, uint64_t out_seq, uint32_t rows, uint32_t channels, uint32_t chunks,
    uint32_t items, uint32_t live, const uint8_t* __restrict__ tables, const uint16_t* __restrict__ filt) {
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

  const h8 f_re = *reinterpret_cast<const h8*>(tables + kOffF1 + lane * 32);
  const h8 f_im = *reinterpret_cast<const h8*>(tables + kOffF1 + lane * 32 + 16);
  const f4 tw_re = *reinterpret_cast<const f4*>(tables + kOffTw + lane * 32);
  const f4 tw_im = *reinterpret_cast<const f4*>(tables + kOffTw + lane * 32 + 16);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // table loads retired: vmcnt below counts only loop traffic
  __syncthreads();
  if (b >= items) return;

  const uint8_t* const g_tab = lds + lane * 16;
  const uint8_t* const h_tab = lds + 16384 + lane * 16;

  // transposed-read geometry of stage 1 (k4096.hpp)
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int m = q + 4 * (g & 1), bb = g >> 1;
  uint8_t* const tr_base = wl + m * 1024 + bb * 512 + 8 * p;

  // stages 1 -> 3 on the wave's LDS image: conv4096_kernel's, statement by statement
  auto transform = [&](auto&& mul, auto&& sink) {
    uint32_t pr[8][4], pi[8][4];
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
  };

  // conv4096_kernel issues the next signal's copy at the bottom of its loop, behind the read-out, and waits for it at the top. The
  // same order of events is written here with the load at the top: an item's zero fill and DMA are issued once the previous
  // item's image has been read out (the lgkmcnt(0) at the bottom), they fly under that item's stores, and the waits follow
  // in straight-line code, so every path from an LDS-DMA to the end of the program passes an s_waitcnt vmcnt(0) whatever shape the
  // compiler gives the loop's latch.
  do {
    load_item(in, in_seq, rows, channels, chunks, b, wl, wl_off, lane);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the item's DMA has landed ...
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // ... and so has its zero fill, before stage 1 reads either

    // this item's filter values: [half][r2] vectors of 8 bins, RE and IM (plain cached loads; they fly under stage 1)
    const uint16_t* const fimg = filt + static_cast<uint64_t>(b % channels) * 8192u + 8u * lane;
    u4 hre[2][4], him[2][4];
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int r2 = 0; r2 < 4; ++r2) {
        hre[half][r2] = *reinterpret_cast<const u4*>(fimg + (half * 4 + r2) * 512);
        him[half][r2] = *reinterpret_cast<const u4*>(fimg + 4096 + (half * 4 + r2) * 512);
      }

    // ---- pass 0: X / 4096 in fp32, times H * 4096, one rounding, back into the image with the planes exchanged
    transform(
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

    // ---- pass 1: the inverse transform; staged through the image (slot swizzle of kStageOut), planes exchanged back
    transform([](int, f4&, f4&) {},
              [&](int half, int r2, u4 vr, u4 vi) {
                const uint32_t slot = 2u * (lane & 15) + half;
                const uint32_t off = 16u * (slot ^ ((slot >> 3) & 1)) + 512u * (4 * g + r2);
                *reinterpret_cast<u4*>(wl + 8192 + off) = vr;
                *reinterpret_cast<u4*>(wl + off) = vi;
              });
    // the kept samples: chunk 64 i + lane of a plane, as long as it lies below L / 8
    const uint32_t pb = b / channels, cb = b - pb * channels;
    const bool has_im = 2 * pb + 1 < rows;
    uint16_t* const y_re = out + (static_cast<uint64_t>(2 * pb) * channels + cb) * out_seq;
    uint16_t* const y_im = y_re + static_cast<uint64_t>(channels) * out_seq;
    const uint32_t rd = 16u * (lane ^ ((lane >> 3) & 1));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (static_cast<uint32_t>(64 * i + lane) < chunks) {
        const u4 vr = *reinterpret_cast<const u4*>(wl + 1024 * i + rd);
        st<kNonTemporal>(y_re + 512 * i + 8 * lane, vr);
        if (has_im) {
          const u4 vi = *reinterpret_cast<const u4*>(wl + 8192 + 1024 * i + rd);
          st<kNonTemporal>(y_im + 512 * i + 8 * lane, vi);
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next item's zero fill and DMA
    b += stride_b;
  } while (b < items);
}

}  // namespace lconv4096
