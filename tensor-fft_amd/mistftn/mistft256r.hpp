// mistft256r.hpp — the time-domain frames of a MASKED inverse short-time Fourier transform at the frame lengths n = 256 R, R = 2, 4,
// 8 (512, 1024, 2048) for gfx950: two half spectra (bins 0 .. n / 2) and their two real masks in, two real frames of n samples out,
// in one pass over HBM. It is istftn/istft256r.hpp's frames_kernel<R> with the masks loaded beside the spectra and multiplied in
// inside the merge's fp32 sum, in front of its single rounding (include/tfft_mistftn.h states the arithmetic):
//
//   merge   Z'r[k] = fp16(n * fp32(mA A.re - mB B.im)), Z'i[k] = fp16(n * fp32(mA A.im + mB B.re)) on the low bins, the high bins
//           from bin n - k with merge_high_gain's signs, the edge bins 0 and n / 2 fp16(n * mA A.re) and fp16(n * mB B.re), whose IM is
//           never read. A product of two binary16 values is exact in fp32 (11 + 11 significant bits, exponents between 2^-48 and
//           2^32), so each sum has one fp32 rounding whether the compiler forms it as mul, mul, add or as mul, fma: no `fp contract`
//           pragma is needed, as olan.hpp says of its own sums. The gain n is a power of two. Z' is written with ds_write_b128 into
//           the slot the LDS-DMA of fft256r_kernel would have filled, Zi' into the RE plane and Zr' into the IM plane.
//   middle  istft256r::frames_kernel<R>'s, which is csrc/k256r.hpp's fft256r_kernel<R, true, false>, statement by statement.
//   store   the end of fft256r_kernel: every plane leaves as n contiguous halves with non-temporal 16-byte stores.
//
// Frames, pairing, the ragged last group, the task mapping (task = 64 i + lane, t = task / 16 R, v = task % 16 R), the LDS image
// (slot_of), its freedom from bank conflicts and the launch shape (launch_iters, live) are istft256r.hpp's; its header comment holds
// the derivations. What a task takes MORE than there:
//
//   two 16-byte non-temporal loads, chunk v of mA and of mB (bins 8v .. 8v + 7 of the masks of frames 2b and 2b + 1),
//   one half each for bin n / 2 of mA and mB, which every lane reads of its own transform, so that halves beyond bin n / 2 of a mask
//       frame are never read,
//   one ds_bpermute that carries mA[8v + 8] | mB[8v + 8] << 16 from the lane above; at R = 8 lane 0 hands up element 0 of its NEXT
//       chunk for lane 63 of an even i, as for the spectra.
//
// The mask of frame g lies at mask + g * mask_frame halves, formed in 64 bits. In per-bin mode the host passes mask_frame = 0 and
// every frame reads the one mask. Frame, B = A and per-bin are selects on the address; none sits under a per-lane branch, and all
// loads of a group, 24 chunk loads and 16 halves, are issued before the first merge.
//
// The stage code, the butterflies and the merge are restated here, as istft256r.hpp restates k256r.hpp, stockham.hpp and
// istft4096.hpp, so that the code generation of the shipped kernels is untouched and this library's code object holds the masked
// kernels (and olan::ola_kernel) alone. The host side (tfft_mistftn.hip) includes k256r.hpp for build_tables and holds the
// constants below to it.
#pragma once

#include "../csrc/k4096.hpp"

namespace mistft256r {

using k4096::f4;
using k4096::h8;
using k4096::s4;
using k4096::u2;
using k4096::u4;

// ---- k256r.hpp's: the constant blob, the LDS budget, the swizzle of the 32-byte blocks of row n1
constexpr int kDataBytes = k4096::kWavesPerBlock * k4096::kLdsWaveBytes;   // 128 KiB: 8 waves x 4096 points
constexpr int kOffFa = 0, kOffFb = 2048, kOffS = 4096;                     // stage-1 / stage-2 B operands, then S[R] and T[R - 1]
template <int R> constexpr int table_bytes() { return kOffS + 2048 * R + 2048 * (R - 1); }
template <int R> constexpr int lds_bytes() { return kDataBytes + 2048 * R + 2048 * (R - 1); }   // data + S + T
__host__ __device__ constexpr int swz(int R, int n1) { return (n1 >> (R == 2 ? 2 : (R == 4 ? 1 : 0))) & (R - 1); }
// the 16-byte slot of a plane that holds frame chunk j (and the frame chunk that slot j holds: an involution)
__host__ __device__ constexpr uint32_t slot_of(int R, uint32_t j) {
  return 2 * R * (j / (2 * R)) + 2 * (((j % (2 * R)) >> 1) ^ static_cast<uint32_t>(swz(R, static_cast<int>(j / (2 * R))))) + (j & 1);
}

// ---- stockham.hpp's: the radix-2, 4, 8 butterflies, forward, natural order in and out
struct cf {
  float re, im;
};
__device__ __forceinline__ cf cmul(cf a, cf b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cf cadd(cf a, cf b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cf csub(cf a, cf b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cf mul_mi(cf a) { return {a.im, -a.re}; }     // a * (-i)
__device__ __forceinline__ void dft4(cf& a, cf& b, cf& c, cf& d) {
  const cf s0 = cadd(a, c), s1 = csub(a, c), s2 = cadd(b, d), s3 = mul_mi(csub(b, d));
  a = cadd(s0, s2);
  b = cadd(s1, s3);
  c = csub(s0, s2);
  d = csub(s1, s3);
}
template <int R>
__device__ __forceinline__ void dft(cf (&v)[R]);
template <>
__device__ __forceinline__ void dft<2>(cf (&v)[2]) {
  const cf a = v[0], b = v[1];
  v[0] = cadd(a, b);
  v[1] = csub(a, b);
}
template <>
__device__ __forceinline__ void dft<4>(cf (&v)[4]) {
  dft4(v[0], v[1], v[2], v[3]);
}
// n = n0 + 4 n1 (n0<4, n1<2), k = k0 + 2 k1 (k0<2, k1<4)
template <>
__device__ __forceinline__ void dft<8>(cf (&v)[8]) {
  const float h = 0.70710678118654752f;
  cf y[4][2];
#pragma unroll
  for (int n0 = 0; n0 < 4; ++n0) {
    y[n0][0] = cadd(v[n0], v[n0 + 4]);
    y[n0][1] = csub(v[n0], v[n0 + 4]);
  }
  // y[n0][1] *= w8^n0
  y[1][1] = cmul(y[1][1], cf{h, -h});
  y[2][1] = mul_mi(y[2][1]);
  y[3][1] = cmul(y[3][1], cf{-h, -h});
#pragma unroll
  for (int k0 = 0; k0 < 2; ++k0) {
    cf a = y[0][k0], b = y[1][k0], c = y[2][k0], d = y[3][k0];
    dft4(a, b, c, d);
    v[k0] = a;
    v[k0 + 2] = b;
    v[k0 + 4] = c;
    v[k0 + 6] = d;
  }
}

// ---- istft256r.hpp's merge with the masks inside the sum. Every product below is exact in fp32, so each sum rounds once, with or
// without contraction into an fma
// Z'[k] for k <= n / 2 from bin k of A and B and of their masks (edge: k = 0 or n / 2, whose IM is ignored)
__device__ __forceinline__ void merge_low_masked(float gain, uint16_t ma, uint16_t mb, uint16_t ar, uint16_t ai, uint16_t br, uint16_t bi,
                                                 bool edge, uint16_t& zr, uint16_t& zi) {
  using rsplit::f2h;
  using rsplit::h2f;
  const float fa = h2f(ma), fb = h2f(mb);
  const uint16_t r = f2h(gain * (fa * h2f(ar) - fb * h2f(bi))), i = f2h(gain * (fa * h2f(ai) + fb * h2f(br)));
  zr = edge ? f2h(gain * (fa * h2f(ar))) : r;
  zi = edge ? f2h(gain * (fb * h2f(br))) : i;
}
// Z'[k] for k > n / 2 from bin n - k of A and B and of their masks (edge: n - k = n / 2)
__device__ __forceinline__ void merge_high_masked(float gain, uint16_t ma, uint16_t mb, uint16_t ar, uint16_t ai, uint16_t br, uint16_t bi,
                                                  bool edge, uint16_t& zr, uint16_t& zi) {
  using rsplit::f2h;
  using rsplit::h2f;
  const float fa = h2f(ma), fb = h2f(mb);
  const uint16_t r = f2h(gain * (fa * h2f(ar) + fb * h2f(bi))), i = f2h(gain * (fb * h2f(br) - fa * h2f(ai)));
  zr = edge ? f2h(gain * (fa * h2f(ar))) : r;
  zi = edge ? f2h(gain * (fb * h2f(br))) : i;
}
__device__ __forceinline__ uint16_t elem(u4 v, int j) { return static_cast<uint16_t>(v[j >> 1] >> (16 * (j & 1))); }
__device__ __forceinline__ u4 pack8(const uint16_t* h) {
  return u4{h[0] | (uint32_t{h[1]} << 16), h[2] | (uint32_t{h[3]} << 16), h[4] | (uint32_t{h[5]} << 16), h[6] | (uint32_t{h[7]} << 16)};
}
// 32-bit value of lane `src` of this wave (ds_bpermute): every lane of the wave is active where this is called
__device__ __forceinline__ uint32_t from_lane(uint32_t v, int src) {
  return static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(src * 4, static_cast<int>(v)));
}

// in_re / in_im: half spectrum of frame g at + g * in_frame halves, bins 0 .. n / 2. mask: the mask of frame g at + g * mask_frame
// halves, bins 0 .. n / 2 (mask_frame = 0: one mask for every frame). frames_out: frame g at + g * n halves. total frames, batch =
// ceil(total / 2) transforms. tables: a k256r::build_tables(R) blob.
template <int R>
__global__ __launch_bounds__(k4096::kThreads, 2) void frames_kernel(const uint16_t* in_re, const uint16_t* in_im, const uint16_t* mask,
                                                                    uint16_t* frames_out, uint64_t in_frame, uint64_t mask_frame,
                                                                    uint32_t total, uint32_t batch, uint32_t live,
                                                                    const uint8_t* __restrict__ tables) {
  using namespace k4096;
  constexpr int kPerWave = 16 / R;          // transforms per wave iteration
  constexpr int kPlane = 512 * R;           // bytes of one plane of one transform
  constexpr uint32_t kChunks = 32 * R;      // 16-byte chunks of one plane: n / 8
  constexpr uint32_t kTasks = 16 * R;       // merge tasks of one transform: the chunks below bin n / 2
  constexpr uint32_t kN = 256 * R;
  constexpr float kGain = static_cast<float>(kN);
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // S and T tables behind the data regions
  uint8_t* const tab = lds + kDataBytes;
  for (int i = tid; i < (2048 * R + 2048 * (R - 1)) / 16; i += kThreads)
    reinterpret_cast<u4*>(tab)[i] = reinterpret_cast<const u4*>(tables + kOffS)[i];
  const h8 fa_re = *reinterpret_cast<const h8*>(tables + kOffFa + lane * 32);
  const h8 fa_im = *reinterpret_cast<const h8*>(tables + kOffFa + lane * 32 + 16);
  const h8 fb_re = *reinterpret_cast<const h8*>(tables + kOffFb + lane * 32);
  const h8 fb_im = *reinterpret_cast<const h8*>(tables + kOffFb + lane * 32 + 16);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const uint8_t* const s_tab = tab + lane * 32;
  const uint8_t* const t_tab = tab + 2048 * R + lane * 32;

  uint8_t* const wl = lds + wave * kLdsWaveBytes;
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3, x = lane & 15;
  // transposed read of tile u: row n1 = 4 g + q, block u ^ swz(n1), bytes 8 p of it
  const int n1r = 4 * g + q;
  const uint8_t* const tr_row = wl + 32 * R * n1r + 8 * p;
  const int sw = swz(R, n1r);
  // staging position of a lane's 8-byte piece inside a segment's 512 bytes (k256r.hpp)
  const uint32_t stage_off = 32u * x + 16u * ((g >> 1) ^ ((x >> 2) & 1)) + 8u * ((g & 1) ^ ((x >> 3) & 1));
  const int up = (lane + 1) & 63;           // the lane whose chunk starts with bin 8v + 8

  const uint32_t groups = (batch + kPerWave - 1) / kPerWave;
  // live waves and the stride over the groups: as stft256r_kernel
  const uint32_t stride_g = gridDim.x * live;
  uint32_t grp = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave) < live ? blockIdx.x * live + wave : groups);
  if (grp >= groups) return;

  do {
    const uint32_t b0 = grp * kPerWave;
    const uint32_t nb = (batch - b0 < kPerWave) ? (batch - b0) : kPerWave;   // ragged last group

    // ---- the half spectra and the masks of the group. A transform the group lacks takes the last valid one again; the B of a
    // self-paired last transform is its A, and so is its mask. All are selects on the address. The 24 chunk loads and the 16 halves of
    // bin n / 2 are issued before the first merge, so a group pays one HBM round trip.
    u4 xar[4], xai[4], xbr[4], xbi[4], xma[4], xmb[4];
    uint16_t nqa[4], nqb[4], nqma[4], nqmb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t task = 64u * i + lane;
      const uint32_t t = task / kTasks, v = task % kTasks;
      const uint32_t fr_a = 2 * (b0 + (t < nb ? t : nb - 1));
      const bool paired = fr_a + 1 < total;                                // false: the last frame of an odd total, paired with itself
      const uint64_t b_off = paired ? in_frame : 0;
      const uint64_t mb_off = paired ? mask_frame : 0;                     // (0 in per-bin mode either way)
      const uint16_t* const a_re = in_re + static_cast<uint64_t>(fr_a) * in_frame;
      const uint16_t* const a_im = in_im + static_cast<uint64_t>(fr_a) * in_frame;
      const uint16_t* const a_m = mask + static_cast<uint64_t>(fr_a) * mask_frame;
      xar[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_re + 8 * v));
      xai[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_im + 8 * v));
      xbr[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_re + b_off + 8 * v));
      xbi[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_im + b_off + 8 * v));
      xma[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_m + 8 * v));
      xmb[i] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(a_m + mb_off + 8 * v));
      // bin n / 2 of the lane's own transform as one half (its IM is ignored, so it is not read at all), and of its masks
      nqa[i] = a_re[kN / 2];
      nqb[i] = a_re[b_off + kN / 2];
      nqma[i] = a_m[kN / 2];
      nqmb[i] = a_m[mb_off + kN / 2];
    }
    // ---- the merge of rfft::merge_kernel with the masks and the gain, straight into the image
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t task = 64u * i + lane;
      const uint32_t t = task / kTasks, v = task % kTasks;
      const bool last = v == kTasks - 1;                                   // bin 8v + 8 is bin n / 2
      // bin 8v + 8 of A and B, (RE | IM << 16), and of the masks, (mA | mB << 16), from the lane above
      uint32_t give_a = uint32_t{elem(xar[i], 0)} | (uint32_t{elem(xai[i], 0)} << 16);
      uint32_t give_b = uint32_t{elem(xbr[i], 0)} | (uint32_t{elem(xbi[i], 0)} << 16);
      uint32_t give_m = uint32_t{elem(xma[i], 0)} | (uint32_t{elem(xmb[i], 0)} << 16);
      if constexpr (R == 8) {
        if ((i & 1) == 0) {                                                // lane 0 hands up what lane 63 needs: element 0 of its NEXT chunk
          const int i1 = i < 3 ? i + 1 : 3;
          const uint32_t next_a = uint32_t{elem(xar[i1], 0)} | (uint32_t{elem(xai[i1], 0)} << 16);
          const uint32_t next_b = uint32_t{elem(xbr[i1], 0)} | (uint32_t{elem(xbi[i1], 0)} << 16);
          const uint32_t next_m = uint32_t{elem(xma[i1], 0)} | (uint32_t{elem(xmb[i1], 0)} << 16);
          give_a = lane == 0 ? next_a : give_a;
          give_b = lane == 0 ? next_b : give_b;
          give_m = lane == 0 ? next_m : give_m;
        }
      }
      const uint32_t got_a = from_lane(give_a, up), got_b = from_lane(give_b, up), got_m = from_lane(give_m, up);
      const uint32_t na = last ? uint32_t{nqa[i]} : got_a;
      const uint32_t nx = last ? uint32_t{nqb[i]} : got_b;
      const uint32_t nm = last ? (uint32_t{nqma[i]} | (uint32_t{nqmb[i]} << 16)) : got_m;
      uint16_t lr[8], li[8], hr[8], hi[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        merge_low_masked(kGain, elem(xma[i], j), elem(xmb[i], j), elem(xar[i], j), elem(xai[i], j), elem(xbr[i], j), elem(xbi[i], j),
                         j == 0 && v == 0, lr[j], li[j]);
        if (j)
          merge_high_masked(kGain, elem(xma[i], 8 - j), elem(xmb[i], 8 - j), elem(xar[i], 8 - j), elem(xai[i], 8 - j), elem(xbr[i], 8 - j),
                            elem(xbi[i], 8 - j), false, hr[j], hi[j]);
        else
          merge_high_masked(kGain, static_cast<uint16_t>(nm), static_cast<uint16_t>(nm >> 16), static_cast<uint16_t>(na),
                            static_cast<uint16_t>(na >> 16), static_cast<uint16_t>(nx), static_cast<uint16_t>(nx >> 16), last, hr[0], hi[0]);
      }
      // chunk v and its mirror n / 8 - 1 - v, each into the slot of the source-swizzled image (conflict free: istft256r.hpp's header
      // comment). Planes exchanged: Zi' into the RE plane, Zr' into the IM plane.
      uint8_t* const tb = wl + t * 2 * kPlane;
      const uint32_t lo = 16u * slot_of(R, v), hi_off = 16u * slot_of(R, kChunks - 1 - v);
      *reinterpret_cast<u4*>(tb + lo) = pack8(li);
      *reinterpret_cast<u4*>(tb + kPlane + lo) = pack8(lr);
      *reinterpret_cast<u4*>(tb + hi_off) = pack8(hi);
      *reinterpret_cast<u4*>(tb + kPlane + hi_off) = pack8(hr);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the loads are the compiler's to count: every merge above waited for its own)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the image has landed before stage 1 reads it

#pragma unroll
    for (int t = 0; t < kPerWave; ++t) {
      const uint8_t* const tb = tr_row + t * 2 * kPlane;
      // ---- stage 1 + twiddle, all R tiles of the transform (fft256r_kernel's, statement by statement)
      f4 t_re[R], t_im[R];
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const uint8_t* ad = tb + 32 * (u ^ sw);
        const s4 xr = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(ad));
        const s4 xi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4*)(ad + kPlane));
        const u4 raw = {__builtin_bit_cast(u2, xr).x, __builtin_bit_cast(u2, xr).y, __builtin_bit_cast(u2, xi).x,
                        __builtin_bit_cast(u2, xi).y};
        const h8 a1 = __builtin_bit_cast(h8, raw);
        const f4 d_re = mfma(a1, fa_re);
        const f4 d_im = mfma(a1, fa_im);
        const f4 s_re = *reinterpret_cast<const f4*>(s_tab + u * 2048);
        const f4 s_im = *reinterpret_cast<const f4*>(s_tab + u * 2048 + 16);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          t_re[u][r4] = __builtin_fmaf(d_re[r4], s_re[r4], -(d_im[r4] * s_im[r4]));
          t_im[u][r4] = __builtin_fmaf(d_re[r4], s_im[r4], d_im[r4] * s_re[r4]);
        }
      }
      // ---- stage-2 operands per decimated sequence
      u4 op[R];
      if constexpr (R == 2) {
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
          op[rr] = u4{pk(t_re[0][rr], t_re[0][rr + 2]), pk(t_re[1][rr], t_re[1][rr + 2]), pk(t_im[0][rr], t_im[0][rr + 2]),
                      pk(t_im[1][rr], t_im[1][rr + 2])};
      } else if constexpr (R == 4) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          op[rr] = u4{pk(t_re[0][rr], t_re[1][rr]), pk(t_re[2][rr], t_re[3][rr]), pk(t_im[0][rr], t_im[1][rr]),
                      pk(t_im[2][rr], t_im[3][rr])};
      } else {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          // lane groups 0, 2 hold sequence reg, groups 1, 3 sequence reg + 4; tiles (0,1),(2,3) <-> (4,5),(6,7)
          auto a_re = __builtin_amdgcn_permlane16_swap(pk(t_re[0][reg], t_re[1][reg]), pk(t_re[4][reg], t_re[5][reg]), false, false);
          auto b_re = __builtin_amdgcn_permlane16_swap(pk(t_re[2][reg], t_re[3][reg]), pk(t_re[6][reg], t_re[7][reg]), false, false);
          auto a_im = __builtin_amdgcn_permlane16_swap(pk(t_im[0][reg], t_im[1][reg]), pk(t_im[4][reg], t_im[5][reg]), false, false);
          auto b_im = __builtin_amdgcn_permlane16_swap(pk(t_im[2][reg], t_im[3][reg]), pk(t_im[6][reg], t_im[7][reg]), false, false);
          op[reg] = u4{a_re[0], b_re[0], a_im[0], b_im[0]};
          op[reg + 4] = u4{a_re[1], b_re[1], a_im[1], b_im[1]};
        }
      }
      // ---- stage 2, twiddle, radix-R butterfly, staged write
      f4 o_re[R], o_im[R];
#pragma unroll
      for (int rr = 0; rr < R; ++rr) {
        const h8 a2 = __builtin_bit_cast(h8, op[rr]);
        o_re[rr] = mfma(a2, fb_re);
        o_im[rr] = mfma(a2, fb_im);
      }
      uint32_t pk_re[R][2], pk_im[R][2];   // [s][register pair]
      float keep_re[R], keep_im[R];
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        cf v[R];
        v[0] = {o_re[0][reg], o_im[0][reg]};
#pragma unroll
        for (int rr = 1; rr < R; ++rr) {
          const f4 w_re = *reinterpret_cast<const f4*>(t_tab + (rr - 1) * 2048);
          const f4 w_im = *reinterpret_cast<const f4*>(t_tab + (rr - 1) * 2048 + 16);
          v[rr].re = __builtin_fmaf(o_re[rr][reg], w_re[reg], -(o_im[rr][reg] * w_im[reg]));
          v[rr].im = __builtin_fmaf(o_re[rr][reg], w_im[reg], o_im[rr][reg] * w_re[reg]);
        }
        dft<R>(v);
#pragma unroll
        for (int s = 0; s < R; ++s) {
          if ((reg & 1) == 0) {
            keep_re[s] = v[s].re;
            keep_im[s] = v[s].im;
          } else {
            pk_re[s][reg >> 1] = pk(keep_re[s], v[s].re);
            pk_im[s][reg >> 1] = pk(keep_im[s], v[s].im);
          }
        }
      }
      // the transposed reads of transform t have all returned (their data went through the MFMAs above). Planes exchanged back: the
      // IM result is the real part of ifft(Z'), frame 2 (b0 + t), and goes into plane 0
      uint8_t* const slot = wl + t * 2 * kPlane + stage_off;
#pragma unroll
      for (int s = 0; s < R; ++s) {
        *reinterpret_cast<u2*>(slot + 512 * s) = u2{pk_im[s][0], pk_im[s][1]};
        *reinterpret_cast<u2*>(slot + kPlane + 512 * s) = u2{pk_re[s][0], pk_re[s][1]};
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the staged frames have landed before they are read back

    // ---- the staged image read back in natural order (the end of fft256r_kernel): KiB i is piece pq of plane `plane` of transform
    // t; plane 0 is frame 2 (b0 + t), plane 1 the frame after it, when it exists
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = i / R, ii = i % R, plane = ii / (R / 2), pq = ii % (R / 2);
      u4 v = *reinterpret_cast<const u4*>(wl + i * 1024 + 16 * lane);
      const uint32_t chunk = lane ^ ((lane >> 3) & 1);          // (two 512-byte segments per piece; the swizzle is per segment)
      if ((lane >> 4) & 1) v = u4{v.z, v.w, v.x, v.y};
      const uint32_t fr = 2 * (b0 + t) + plane;
      if (static_cast<uint32_t>(t) < nb && fr < total) {         // wave-uniform
        uint16_t* const dst = frames_out + static_cast<uint64_t>(fr) * kN + 512 * pq + 8 * chunk;
        __builtin_nontemporal_store(v, reinterpret_cast<u4*>(dst));
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next group's image is built
    grp += stride_g;
  } while (grp < groups);
}

}  // namespace mistft256r
