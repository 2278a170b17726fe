// conv4096.hpp — fused FFT convolution at N = 4096 for gfx950: forward transform, multiplication of the spectrum by a filter and
// inverse transform in ONE pass over HBM (16 KiB in, 16 KiB out per signal), one wave per signal.
//
// The three MFMA stages are those of csrc/k4096.hpp (fft4096_kernel, variant kStageOut | kNonTemporal), restated on top of
// its helpers so that the headline kernel's code generation is untouched. What is new sits between two runs of them:
//
//   pass 0   dma_in -> stage 1 -> 2 -> 3: the fp32 accumulators hold X / 4096 (1/16 per stage, sequential scaling: no finite
//            input overflows). Each lane multiplies the bins it owns, k = k0 + 16 k1 + 256 (4 g + r2), by H_k * 4096 in scalar
//            fp32 (the factor is an exact power of two on the fp32 filter value), rounds ONCE to binary16 and writes the
//            filtered spectrum Z = X H back into the wave's LDS region in the layout dma_in leaves there (slot l of 1-KiB block
//            mm holds 16-byte chunk l ^ 2 mm), RE into the IM half and IM into the RE half.
//   pass 1   stage 1 -> 2 -> 3 on that image: DFT(swap Z) / 4096 = swap(ifft(Z)). The result is staged through LDS as the
//            headline kernel stages its spectrum, planes exchanged back, and stored as full 1-KiB rows, non-temporally.
//
// Filter image (built once by tfft_conv_plan_set_filter, 16 KiB per filter as binary16, [RE 4096 | IM 4096]): bin k sits at
// slot ((half * 4 + r2) * 64 + lane) * 8 + j of its plane, k0 = 8 half + j, lane = 16 g + k1: a lane's eight values for one
// (half, r2) are one 16-byte vector, a wave's load of them one contiguous KiB. The image is shared by every signal of a channel and
// is read with plain cached loads (it lives in L2 / Infinity Cache); the signals themselves stream (nt).
#pragma once

#include "../csrc/k4096.hpp"

namespace conv4096 {

using k4096::f4;
using k4096::h8;
using k4096::s4;
using k4096::u2;
using k4096::u4;

// in_* / out_*: planar binary16, signal b at + b * stride halves. tables: the first k4096::kOffF1n bytes of a
// k4096::build_tables() blob (default scaling). filt: filter images, filter f at + f * 8192 halves; signal b takes b % filters.
__global__ __launch_bounds__(k4096::kThreads, 2) void conv4096_kernel(
    const uint16_t* in_re, const uint16_t* in_im, uint16_t* out_re, uint16_t* out_im, uint64_t in_stride, uint64_t out_stride,
    uint32_t batch, uint32_t live, uint32_t filters, const uint8_t* __restrict__ tables, const uint16_t* __restrict__ filt) {
  using namespace k4096;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  uint8_t* const wl = lds + kLdsTableBytes + wave * kLdsWaveBytes;
  const uint32_t wl_off = __builtin_amdgcn_readfirstlane(
      static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) uint8_t*)wl)));

  // live waves and the stride over the batch: as fft4096_kernel
  const uint32_t stride_b = gridDim.x * live;
  uint32_t b = static_cast<uint32_t>(wave) < live ? blockIdx.x * live + wave : batch;

  for (int i = tid; i < kLdsTableBytes / 16; i += kThreads)
    reinterpret_cast<u4*>(lds)[i] = reinterpret_cast<const u4*>(tables + kOffG)[i];

  const h8 f_re = *reinterpret_cast<const h8*>(tables + kOffF1 + lane * 32);
  const h8 f_im = *reinterpret_cast<const h8*>(tables + kOffF1 + lane * 32 + 16);
  const f4 tw_re = *reinterpret_cast<const f4*>(tables + kOffTw + lane * 32);
  const f4 tw_im = *reinterpret_cast<const f4*>(tables + kOffTw + lane * 32 + 16);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // table loads retired: vmcnt below counts only loop traffic
  __syncthreads();
  if (b >= batch) return;
  dma_in<true>(reinterpret_cast<const uint8_t*>(in_re + b * in_stride), reinterpret_cast<const uint8_t*>(in_im + b * in_stride), wl_off, lane);

  const uint8_t* const g_tab = lds + lane * 16;
  const uint8_t* const h_tab = lds + 16384 + lane * 16;

  // transposed-read geometry of stage 1 (k4096.hpp)
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int m = q + 4 * (g & 1), bb = g >> 1;
  uint8_t* const tr_base = wl + m * 1024 + bb * 512 + 8 * p;

  // stages 1 -> 3 on the wave's LDS image. sink(half, r2, vr, vi): the packed outputs k0 = 8 half .. 8 half + 7 of
  // k2 = 4 g + r2, k1 = lane & 15; mul(half, k0, o_re, o_im): the fp32 accumulators o[r2] of tile k0, before they are packed
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

  // Loop shape as fft4096_kernel: the only exit lies BEFORE an iteration's look-ahead copy is issued, so every path from an
  // LDS-DMA to the end of the program passes the s_waitcnt vmcnt(0) at the loop top.
  for (;;) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // this signal's filter values: [half][r2] vectors of 8 bins, RE and IM (plain cached loads; they fly under stage 1)
    const uint16_t* const fimg = filt + static_cast<uint64_t>(b % filters) * 8192u + 8u * lane;
    u4 hre[2][4], him[2][4];
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int r2 = 0; r2 < 4; ++r2) {
        hre[half][r2] = *reinterpret_cast<const u4*>(fimg + (half * 4 + r2) * 512);
        him[half][r2] = *reinterpret_cast<const u4*>(fimg + 4096 + (half * 4 + r2) * 512);
      }

    // ---- pass 0: X / 4096 in fp32, times H * 4096, one rounding, back into the image with the planes exchanged
    // (the compiler fuses the outer fma of the product with the conversion into v_fma_mixlo / mixhi_f16, as it does for the stage-2
    // twiddles: intended here, it is the one rounding of the contract. cmul.hpp suppresses the same fusion because its fp32
    // value is what the numpy restatement pins bit for bit.)
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
    uint16_t* const y_re = out_re + b * out_stride;
    uint16_t* const y_im = out_im + b * out_stride;
    const uint32_t rd = 16u * (lane ^ ((lane >> 3) & 1));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const u4 vr = *reinterpret_cast<const u4*>(wl + 1024 * i + rd);
      const u4 vi = *reinterpret_cast<const u4*>(wl + 8192 + 1024 * i + rd);
      st<kNonTemporal>(y_re + 512 * i + 8 * lane, vr);
      st<kNonTemporal>(y_im + 512 * i + 8 * lane, vi);
    }
    const uint32_t nb = b + stride_b;
    if (nb >= batch) break;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before reuse
    dma_in<true>(reinterpret_cast<const uint8_t*>(in_re + nb * in_stride), reinterpret_cast<const uint8_t*>(in_im + nb * in_stride), wl_off, lane);
    b = nb;
  }
}

}  // namespace conv4096
