// stft4096.hpp — short-time Fourier transform of REAL signals at frame length 4096 for gfx950: hopped, windowed frames of long
// signals, each transformed to its half spectrum (bins 0 .. 2048), in one pass over HBM. Three measured pieces in a row:
//
//   load    sconv/sconv4096.hpp's window indexing: frame f of a signal is the 4096 samples that start at sample f * hop - pad, a
//           SIGNED quantity; samples outside [0, L) read as zero and are never loaded.
//   times   gsconv/gsconv4096.hpp's multiplier on the way in (load_item<true>): the samples come in through registers, are
//           multiplied (one packed binary16 multiply per pair of samples: round to nearest even, subnormals kept) and written into
//           the slot an LDS-DMA would have filled (ds_write_b128). The multiplier is the WINDOW, indexed by the position in the
//           frame, not in the signal: a lane's eight window chunks are the same for every item, loaded once per wave and held in 32
//           registers. The loop carries no window traffic at all.
//   split   csrc/k4096.hpp's real-input epilogue (RS = true, csrc/rsplit.hpp): two frames travel as the RE and the IM plane of one
//           complex transform and leave as two half spectra.
//
// Frames are numbered g = r * F + f over all signals (F frames per signal); item i transforms frames 2i (RE plane) and 2i + 1 (IM
// plane), so a pair may straddle two signals. An odd total pairs its last frame with itself and writes only the first half
// spectrum. That is fft4096_kernel<kStageOut | kNonTemporal, false, true> on the frames laid out in the order g, and the middle is
// that kernel's, statement by statement (same tables, same three MFMA stages, same stage-out swizzle, same split, same LDS image
// and launch shape): the two agree in every bit.
//
//   slot l of 1-KiB block mm holds frame chunk j = 64 mm + (l ^ 2 mm), whose SOURCE chunk is (f * hop - pad) / 8 + j, signed. A
//   plane's eight loads are issued together and none sits under a per-lane branch: a lane whose source chunk lies outside
//   [0, L / 8) loads chunk max((f * hop - pad) / 8, 0) of the same signal instead, which this item reads anyway and which is always
//   below L / 8 (a frame starts at most at sample L + pad - 4096 < L), and a select then writes the product or zero.
//
// The stage code is restated on the k4096 helpers, as sconv4096.hpp restates it, so that the code generation of the shipped kernels
// is untouched.
#pragma once

#include "../csrc/k4096.hpp"

namespace stft4096 {

using k4096::f4;
using k4096::h8;
using k4096::s4;
using k4096::u2;
using k4096::u4;

// eight binary16 products, each rounded once (v_pk_mul_f16 x 4)
__device__ __forceinline__ u4 mul8(u4 a, u4 b) { return __builtin_bit_cast(u4, __builtin_bit_cast(h8, a) * __builtin_bit_cast(h8, b)); }

// what the kernel needs of a plan's geometry: L / 8, hop / 8 and pad / 8 in 16-byte chunks (8 samples), and the frames per signal.
// (frames - 1) * hop <= L + 2 pad - 4096 < 2^27 samples, so the signed 32-bit chunk arithmetic below cannot overflow; a plan with
// one frame per signal passes hop = 0 (f is always 0), so a hop of any size is carried.
struct geometry {
  int32_t chunks, hop, pad;
  uint32_t frames;
};

// in: real binary16, signal r at + r * in_sig halves, 8 * geo.chunks samples each. window: 4096 halves. out_re / out_im: frame g
// at + g * out_frame halves, bins 0 .. 2048. total = rows * geo.frames frames, items = ceil(total / 2). tables: the first
// k4096::kOffF1n bytes of a k4096::build_tables() blob.
__global__ __launch_bounds__(k4096::kThreads, 2) void stft4096_kernel(
    const uint16_t* in, const uint16_t* __restrict__ window, uint16_t* out_re, uint16_t* out_im, uint64_t in_sig, uint64_t out_frame,
    geometry geo, uint32_t total, uint32_t items, uint32_t live, const uint8_t* __restrict__ tables) {
  using namespace k4096;
  constexpr int V = kStageOut | kNonTemporal;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  uint8_t* const wl = lds + kLdsTableBytes + wave * kLdsWaveBytes;

  // live waves and the stride over the items: as conv4096_kernel
  const uint32_t stride_b = gridDim.x * live;
  uint32_t b = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave) < live ? blockIdx.x * live + wave : items);

  for (int i = tid; i < kLdsTableBytes / 16; i += kThreads)
    reinterpret_cast<u4*>(lds)[i] = reinterpret_cast<const u4*>(tables + kOffG)[i];

  const h8 f_re = *reinterpret_cast<const h8*>(tables + kOffF1 + lane * 32);
  const h8 f_im = *reinterpret_cast<const h8*>(tables + kOffF1 + lane * 32 + 16);
  const f4 tw_re = *reinterpret_cast<const f4*>(tables + kOffTw + lane * 32);
  const f4 tw_im = *reinterpret_cast<const f4*>(tables + kOffTw + lane * 32 + 16);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // table loads retired
  __syncthreads();
  if (b >= items) return;

  // the window, once per wave: chunk j = 64 mm + (lane ^ 2 mm) is what slot `lane` of block mm is multiplied with, whatever the item
  u4 wv[8];
#pragma unroll
  for (int mm = 0; mm < 8; ++mm) wv[mm] = *reinterpret_cast<const u4*>(window + 8 * (mm * 64 + (lane ^ (2 * mm))));

  const uint8_t* const g_tab = lds + lane * 16;
  const uint8_t* const h_tab = lds + 16384 + lane * 16;

  // transposed-read geometry of stage 1 (k4096.hpp)
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int m = q + 4 * (g & 1), bb = g >> 1;
  uint8_t* const tr_base = wl + m * 1024 + bb * 512 + 8 * p;

  const u4 zero = {0, 0, 0, 0};
  // One plane of an item's image: frame `fr` in the flat order, w (.) x in the slots whose source chunk lies in [0, L / 8), zeros
  // everywhere else. The eight loads are issued before the first product is formed, so a plane pays one HBM round trip. The test is
  // on the source chunk, not the lane or the frame chunk: the slots are swizzled and the frame is offset.
  auto plane = [&](uint32_t fr, uint8_t* dst) {
    const uint32_t r = fr / geo.frames;                                  // wave-uniform: one division per plane
    const int32_t f = static_cast<int32_t>(fr - r * geo.frames);
    const int32_t first = f * geo.hop - geo.pad;                         // source chunk of frame chunk 0: negative in front of sample 0
    const int32_t spare = first > 0 ? first : 0;
    const uint8_t* const src = reinterpret_cast<const uint8_t*>(in + static_cast<uint64_t>(r) * in_sig);
    u4 xv[8];
#pragma unroll
    for (int mm = 0; mm < 8; ++mm) {
      const int32_t chunk = first + (mm * 64 + (lane ^ (2 * mm)));       // the source chunk slot `lane` of block mm holds
      const uint32_t off = static_cast<uint32_t>(chunk >= 0 && chunk < geo.chunks ? chunk : spare) * 16u;        // below 2^27
      xv[mm] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(src + off));
    }
#pragma unroll
    for (int mm = 0; mm < 8; ++mm) {
      const int32_t chunk = first + (mm * 64 + (lane ^ (2 * mm)));
      const u4 prod = mul8(xv[mm], wv[mm]);
      *reinterpret_cast<u4*>(dst + mm * 1024 + lane * 16) = chunk >= 0 && chunk < geo.chunks ? prod : zero;
    }
  };

  // The order of events of sconv4096_kernel: an item's image is built at the top of the loop, once the previous item's image has
  // been read out (the lgkmcnt(0) at the bottom), and the waits follow in straight-line code.
  do {
    const uint32_t fr_a = 2 * b;
    const bool has_b = fr_a + 1 < total;                                 // wave-uniform; false: the last frame of an odd total, paired with itself
    plane(fr_a, wl);
    plane(has_b ? fr_a + 1 : fr_a, wl + 8192);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the loads are the compiler's to count: every product above waited for its own)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the image, products and zero fill, has landed before stage 1 reads it

    // ---- stage 1 (fft4096_kernel's, statement by statement)
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

    // ---- stages 2 and 3, tile by tile
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
        // the stage-out swizzle of kStageOut
        const uint32_t slot = 2u * (lane & 15) + half;
        const uint32_t off = 16u * (slot ^ ((slot >> 3) & 1)) + 512u * (4 * g + r2);
        *reinterpret_cast<u4*>(wl + off) = vr;
        *reinterpret_cast<u4*>(wl + 8192 + off) = vi;
      }
    }

    // ---- the RS epilogue of fft4096_kernel: the image split into the two half spectra (rsplit.hpp), b_off = out_frame
    auto img = [&](uint32_t v) { return wl + 16u * (v ^ ((v >> 3) & 1u)); };
    uint16_t* const a_re = out_re + static_cast<uint64_t>(fr_a) * out_frame;
    uint16_t* const a_im = out_im + static_cast<uint64_t>(fr_a) * out_frame;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t v = 64u * i + lane;
      const u4 xr = *reinterpret_cast<const u4*>(img(v));
      const u4 xi = *reinterpret_cast<const u4*>(img(v) + 8192);
      const u4 yr = *reinterpret_cast<const u4*>(img(511u - v));
      const u4 yi = *reinterpret_cast<const u4*>(img(511u - v) + 8192);
      const uint16_t y0r = *reinterpret_cast<const uint16_t*>(img((512u - v) & 511u));
      const uint16_t y0i = *reinterpret_cast<const uint16_t*>(img((512u - v) & 511u) + 8192);
      uint16_t zr[8], zi[8], mr[8], mi[8];
      __builtin_memcpy(zr, &xr, 16);
      __builtin_memcpy(zi, &xi, 16);
      __builtin_memcpy(mr, &yr, 16);
      __builtin_memcpy(mi, &yi, 16);
      uint16_t ar[8], ai[8], br[8], bi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        rsplit::split_bin(zr[j], zi[j], j ? mr[8 - j] : y0r, j ? mi[8 - j] : y0i, ar[j], ai[j], br[j], bi[j]);
      u4 var, vai, vbr, vbi;
      __builtin_memcpy(&var, ar, 16);
      __builtin_memcpy(&vai, ai, 16);
      __builtin_memcpy(&vbr, br, 16);
      __builtin_memcpy(&vbi, bi, 16);
      st<V>(a_re + 8 * v, var);
      st<V>(a_im + 8 * v, vai);
      if (has_b) {
        st<V>(a_re + out_frame + 8 * v, vbr);
        st<V>(a_im + out_frame + 8 * v, vbi);
      }
    }
    if (lane == 0) {
      const uint16_t nr = *reinterpret_cast<const uint16_t*>(img(256));
      const uint16_t ni = *reinterpret_cast<const uint16_t*>(img(256) + 8192);
      uint16_t ar, ai, br, bi;
      rsplit::split_bin(nr, ni, nr, ni, ar, ai, br, bi);
      a_re[2048] = ar;
      a_im[2048] = ai;
      if (has_b) {
        a_re[out_frame + 2048] = br;
        a_im[out_frame + 2048] = bi;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next item's image is built
    b += stride_b;
  } while (b < items);
}

}  // namespace stft4096
