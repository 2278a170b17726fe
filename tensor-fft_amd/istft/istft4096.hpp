// istft4096.hpp — the time-domain frames of an inverse short-time Fourier transform at frame length 4096 for gfx950: two half
// spectra (bins 0 .. 2048) in, two real frames of 4096 samples out, in one pass over HBM. It is the real-input epilogue of
// csrc/k4096.hpp (RS = true) run backwards in FRONT of stage 1:
//
//   merge   csrc/rsplit.hpp's merge_low / merge_high with one exact factor in front of the single rounding:
//           Z'[k] = fp16(4096.0f * (fp32 add)), on the edge bins 0 and 2048 fp16(4096.0f * fp32(A.re)) and fp16(4096.0f * fp32(B.re)).
//           The gain undoes the 1 / 4096 of the forward transform BEFORE the inverse stages, which scale by 1/16 each: a frame kept at
//           x / 4096 would cross them near the binary16 subnormals for |x| < 0.25. The half spectra come in through registers and Z'
//           is written into the slot an LDS-DMA would have filled (ds_write_b128), Zi' into the RE half and Zr' into the IM half:
//           DFT(swap Z') / 4096 = swap(ifft(Z')), as pass 1 of conv/conv4096.hpp.
//   stages  fft4096_kernel<kStageOut | kNonTemporal>'s three MFMA stages and stage-out swizzle, statement by statement (same tables,
//           same LDS image, same launch shape), planes exchanged back on the way out as conv4096.hpp's pass 1 does it.
//
// Frames are numbered g = r * F + f over all signals; item i takes the half spectra of frames 2i (A) and 2i + 1 (B) and leaves
// frame 2i from the RE result and frame 2i + 1 from the IM result, each rounded once, at g * 4096 of the workspace. An odd total
// pairs its last frame with itself (B = A) and stores only the first result. That is tfft_exec_inverse of the default N = 4096 plan
// on Z', and the two agree in every bit.
//
//   lane takes input chunks v = 64 i + lane, i < 4 (bins 8v .. 8v + 7 of A.re, A.im, B.re, B.im: four 16-byte loads), and bin 8v + 8
//   from the lane above it (lane 63: from chunk 64 (i + 1) of lane 0; the last one is bin 2048, read as ONE half by every lane: halves
//   beyond bin 2048 of a frame are never read). It writes Z' chunk v (bins 8v + e) and the mirror chunk 511 - v, whose element e is bin
//   4096 - (8v + 8 - e), made from bin 8v + 8 - e. Chunk j of a plane goes to slot (j & 63) ^ 2 (j >> 6) of 1-KiB block j >> 6. Every
//   one of the 512 slots of both planes is written for every item; all loads of an item are issued before the first merge and none
//   sits under a per-lane branch.
//
// The stage code is restated on the k4096 helpers, as stft4096.hpp restates it, so that the code generation of the shipped kernels is
// untouched.
#pragma once

#include "../csrc/k4096.hpp"

namespace istft4096 {

using k4096::f4;
using k4096::h8;
using k4096::s4;
using k4096::u2;
using k4096::u4;

constexpr float kGain = 4096.0f;

// rsplit::merge_low with the gain: Z'[k] for k <= 2048 from bin k of A and B (edge: k = 0 or 2048, whose IM is ignored)
__device__ __forceinline__ void merge_low_gain(uint16_t ar, uint16_t ai, uint16_t br, uint16_t bi, bool edge, uint16_t& zr, uint16_t& zi) {
  using rsplit::f2h;
  using rsplit::h2f;
  const uint16_t r = f2h(kGain * (h2f(ar) - h2f(bi))), i = f2h(kGain * (h2f(ai) + h2f(br)));
  zr = edge ? f2h(kGain * h2f(ar)) : r;
  zi = edge ? f2h(kGain * h2f(br)) : i;
}

// rsplit::merge_high with the gain: Z'[k] for k > 2048 from bin 4096 - k of A and B (edge: 4096 - k = 2048)
__device__ __forceinline__ void merge_high_gain(uint16_t ar, uint16_t ai, uint16_t br, uint16_t bi, bool edge, uint16_t& zr, uint16_t& zi) {
  using rsplit::f2h;
  using rsplit::h2f;
  const uint16_t r = f2h(kGain * (h2f(ar) + h2f(bi))), i = f2h(kGain * (h2f(br) - h2f(ai)));
  zr = edge ? f2h(kGain * h2f(ar)) : r;
  zi = edge ? f2h(kGain * h2f(br)) : i;
}

__device__ __forceinline__ uint16_t elem(u4 v, int j) { return static_cast<uint16_t>(v[j >> 1] >> (16 * (j & 1))); }
__device__ __forceinline__ u4 pack8(const uint16_t* h) {
  return u4{h[0] | (uint32_t{h[1]} << 16), h[2] | (uint32_t{h[3]} << 16), h[4] | (uint32_t{h[5]} << 16), h[6] | (uint32_t{h[7]} << 16)};
}
// 32-bit value of lane `src` of this wave (ds_bpermute): every lane of the wave is active where this is called
__device__ __forceinline__ uint32_t from_lane(uint32_t v, int src) {
  return static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src * 4, static_cast<int>(v)));
}

// in_re / in_im: half spectrum of frame g at + g * in_frame halves, bins 0 .. 2048. frames_out: frame g at + g * 4096 halves. total
// frames, items = ceil(total / 2). tables: the first k4096::kOffF1n bytes of a k4096::build_tables() blob.
__global__ __launch_bounds__(k4096::kThreads, 2) void frames_kernel(
    const uint16_t* in_re, const uint16_t* in_im, uint16_t* frames_out, uint64_t in_frame, uint32_t total, uint32_t items, uint32_t live,
    const uint8_t* __restrict__ tables) {
  using namespace k4096;
  constexpr int V = kStageOut | kNonTemporal;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  uint8_t* const wl = lds + kLdsTableBytes + wave * kLdsWaveBytes;

  // live waves and the stride over the items: as stft4096_kernel
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

  const uint8_t* const g_tab = lds + lane * 16;
  const uint8_t* const h_tab = lds + 16384 + lane * 16;

  // transposed-read geometry of stage 1 (k4096.hpp)
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int m = q + 4 * (g & 1), bb = g >> 1;
  uint8_t* const tr_base = wl + m * 1024 + bb * 512 + 8 * p;

  const int up = (lane + 1) & 63;      // the lane whose chunk starts with bin 8v + 8

  // The order of events of stft4096_kernel: an item's image is built at the top of the loop, once the previous item's image has
  // been read out (the lgkmcnt(0) at the bottom), and the waits follow in straight-line code.
  do {
    const uint32_t fr_a = 2 * b;
    const bool has_b = fr_a + 1 < total;                                 // wave-uniform; false: the last frame of an odd total, paired with itself
    const uint16_t* const a_re = in_re + static_cast<uint64_t>(fr_a) * in_frame;
    const uint16_t* const a_im = in_im + static_cast<uint64_t>(fr_a) * in_frame;
    const uint64_t b_off = has_b ? in_frame : 0;

    // ---- the merge of rfft::merge_kernel with the gain, straight into the image. All loads first: one HBM round trip per item
    u4 xar[4], xai[4], xbr[4], xbi[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t v = 64u * i + lane;
      xar[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_re + 8 * v));
      xai[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_im + 8 * v));
      xbr[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_re + b_off + 8 * v));
      xbi[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_im + b_off + 8 * v));
    }
    // bin 2048 as one half (its IM is ignored, so it is not read at all); the same address in every lane
    const uint16_t nyq_a = a_re[2048], nyq_b = a_re[b_off + 2048];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      // bin 8v + 8 of A and B, (RE | IM << 16): lane 0 hands up what lane 63 needs, element 0 of its NEXT chunk, or bin 2048
      const uint32_t own_a = uint32_t{elem(xar[i], 0)} | (uint32_t{elem(xai[i], 0)} << 16);
      const uint32_t own_b = uint32_t{elem(xbr[i], 0)} | (uint32_t{elem(xbi[i], 0)} << 16);
      const uint32_t next_a = i < 3 ? uint32_t{elem(xar[i < 3 ? i + 1 : 3], 0)} | (uint32_t{elem(xai[i < 3 ? i + 1 : 3], 0)} << 16) : uint32_t{nyq_a};
      const uint32_t next_b = i < 3 ? uint32_t{elem(xbr[i < 3 ? i + 1 : 3], 0)} | (uint32_t{elem(xbi[i < 3 ? i + 1 : 3], 0)} << 16) : uint32_t{nyq_b};
      const uint32_t na = from_lane(lane == 0 ? next_a : own_a, up);
      const uint32_t nb = from_lane(lane == 0 ? next_b : own_b, up);
      uint16_t lr[8], li[8], hr[8], hi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        merge_low_gain(elem(xar[i], j), elem(xai[i], j), elem(xbr[i], j), elem(xbi[i], j), i == 0 && j == 0 && lane == 0, lr[j], li[j]);
        if (j)
          merge_high_gain(elem(xar[i], 8 - j), elem(xai[i], 8 - j), elem(xbr[i], 8 - j), elem(xbi[i], 8 - j), false, hr[j], hi[j]);
        else
          merge_high_gain(static_cast<uint16_t>(na), static_cast<uint16_t>(na >> 16), static_cast<uint16_t>(nb), static_cast<uint16_t>(nb >> 16),
                          i == 3 && lane == 63, hr[0], hi[0]);
      }
      // chunk v = 64 i + lane: block i, slot lane ^ 2 i. Its mirror 511 - v = 64 (7 - i) + (63 - lane): block 7 - i, slot
      // (63 - lane) ^ 2 (7 - i). Each is a permutation of the 64 slots of its block: conflict free. Planes exchanged.
      const uint32_t lo = 1024u * i + 16u * (lane ^ (2 * i));
      const uint32_t hi_off = 1024u * (7 - i) + 16u * ((63 - lane) ^ (2 * (7 - i)));
      *reinterpret_cast<u4*>(wl + lo) = pack8(li);
      *reinterpret_cast<u4*>(wl + 8192 + lo) = pack8(lr);
      *reinterpret_cast<u4*>(wl + hi_off) = pack8(hi);
      *reinterpret_cast<u4*>(wl + 8192 + hi_off) = pack8(hr);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the loads are the compiler's to count: every merge above waited for its own)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the image has landed before stage 1 reads it

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
        // the stage-out swizzle of kStageOut, planes exchanged back (pass 1 of conv4096.hpp)
        const uint32_t slot = 2u * (lane & 15) + half;
        const uint32_t off = 16u * (slot ^ ((slot >> 3) & 1)) + 512u * (4 * g + r2);
        *reinterpret_cast<u4*>(wl + 8192 + off) = vr;
        *reinterpret_cast<u4*>(wl + off) = vi;
      }
    }

    // ---- the image read back row by row and stored coalesced: the RE half is frame 2i, the IM half frame 2i + 1
    uint16_t* const y = frames_out + static_cast<uint64_t>(fr_a) * 4096u;
    const uint32_t rd = 16u * (lane ^ ((lane >> 3) & 1));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const u4 vr = *reinterpret_cast<const u4*>(wl + 1024 * i + rd);
      const u4 vi = *reinterpret_cast<const u4*>(wl + 8192 + 1024 * i + rd);
      st<V>(y + 512 * i + 8 * lane, vr);
      if (has_b) st<V>(y + 4096 + 512 * i + 8 * lane, vi);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next item's image is built
    b += stride_b;
  } while (b < items);
}

}  // namespace istft4096
