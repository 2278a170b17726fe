// spec256r.hpp — power and band spectrograms of REAL signals at the frame lengths n = 256 R, R = 2, 4, 8 (512, 1024, 2048) for
// gfx950: stftn/stft256r.hpp's one-pass STFT with the binary16 half spectra kept in registers and an fp32 epilogue behind them.
//
//   load, middle   stft256r::stft256r_kernel<R>'s, statement by statement (its header describes the frames, the pairing of frames
//                  2b and 2b + 1 as the RE and IM plane of transform b, the LDS image and the staging).
//   split          stft256r's, up to the eight (ar, ai, br, bi) of a task, with its split_bin and the written-out +0 addend: the
//                  halves are the bits tfft_stftn_exec stores.
//   power          P = fp32(gain * fp32(fp32(re)^2 + fp32(im)^2)) per bin. The squares of binary16 values are exact in fp32, so the
//                  sum is one rounding and the gain a second one (none for a power of two short of overflow).
//
// kBands = false stores P: frame g at out + g * out_frame floats, bins 0 .. n / 2, eight bins of a task as two non-temporal
// 16-byte stores, bin n / 2 as a single float by task v = 0.
//
// kBands = true never stores P. The n / 2 + 1 powers of a transform's two frames are 4 n + 8 bytes, its two consumed planes 4 n:
// bins 0 .. n / 2 - 1 of frame A go where the RE plane was and those of frame B where the IM plane was, and the two bin-n / 2
// powers go to a region of 32 / R floats per wave behind the tables. The split of task v reads element 0 of the mirror chunk of
// task v - 1 and, at R = 8, a transform's tasks span two of the four rounds: so the powers of all four rounds are formed in
// registers first (64 VGPRs; the 64 of the loaded frames are dead by then), and only then is the image written. Everything is one
// wave's own LDS and a wave's LDS operations complete in order; the waits below say so anyway.
//
// The power image of a plane: bin k at dword k ^ (4 * ((k >> 5) & 1)), that is natural order with the two 16-byte halves of a
// task's 32 bytes exchanged for tasks 4 .. 7 of every eight. ds_write_b128 is served in groups of 8 consecutive lanes over 32
// banks: in natural order lanes l and l + 4 of a group, 128 bytes apart, meet on the same four banks (2-way, 16 array cycles where
// the instruction takes 13); with the exchange lanes 0 .. 3 take banks 8 l .. 8 l + 3 and lanes 4 .. 7 banks 8 l + 4 .. 8 l + 7:
// conflict free. The band tasks read single dwords at addresses their bands choose; the XOR is one instruction per read.
//
// Band tasks: task 64 i + lane is (frame of the group, band j) = (task / B, task % B) over the frames that exist, so consecutive
// lanes take consecutive bands of a frame and their stores coalesce. A task reads its band's descriptor {first bin, count, offset
// of its weights} and runs acc = w[0] * P[first], then acc = acc + w[i] * P[first + i] in ascending i, every product and every sum
// rounded on its own (mul_rn / add_rn below: no contraction). The weights come from memory (they stay in cache; the LDS is full).
// No atomics, and nothing depends on the launch shape.
//
// The helpers are restated from stftn/stft256r.hpp, as that file restates csrc/k256r.hpp and csrc/stockham.hpp: this library's
// code object holds the spectrogram kernels alone. The host side (tfft_spec.hip) holds the constants to csrc/k256r.hpp.
#pragma once

#include "../csrc/k4096.hpp"

namespace spec256r {

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

// the bin-n / 2 powers of a band kernel: 32 / R floats per wave, kept in a flat KiB behind the tables
constexpr int kNyquistBytes = 1024;
template <int R, bool kBands> constexpr int spec_lds_bytes() { return lds_bytes<R>() + (kBands ? kNyquistBytes : 0); }
static_assert(k4096::kWavesPerBlock * (32 / 2) * 4 <= kNyquistBytes, "the bin-n/2 powers of eight waves must fit their region");
static_assert(spec_lds_bytes<8, true>() <= 159 * 1024 && spec_lds_bytes<8, true>() <= 160 * 1024,
              "R = 8 with bands: 128 KiB of data, 30 KiB of tables and 1 KiB of bin-n/2 powers are 159 of the 160 KiB of a CU");

constexpr uint32_t kMaxBands = 1024;

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

// ---- stft256r.hpp's
// eight binary16 products, each rounded once (v_pk_mul_f16 x 4)
__device__ __forceinline__ u4 mul8(u4 a, u4 b) { return __builtin_bit_cast(u4, __builtin_bit_cast(h8, a) * __builtin_bit_cast(h8, b)); }

// L / 8, hop / 8 and pad / 8 in 16-byte chunks (8 samples), and the frames per signal; a plan with one frame per signal passes hop = 0
struct geometry {
  int32_t chunks, hop, pad;
  uint32_t frames;
};

// bin k of both half spectra from Z[k] = (xr, xi) and Z[n - k] = (yr, yi), to the sign of a zero as tfft_stftn_exec leaves it
__device__ __forceinline__ uint16_t half_of(float s) { return rsplit::f2h(__builtin_fmaf(s, 0.5f, 0.0f)); }
__device__ __forceinline__ void split_bin(uint16_t xr, uint16_t xi, uint16_t yr, uint16_t yi, uint16_t& ar, uint16_t& ai, uint16_t& br,
                                          uint16_t& bi) {
  const float zr = rsplit::h2f(xr), zi = rsplit::h2f(xi), mr = rsplit::h2f(yr), mi = rsplit::h2f(yi);
  ar = half_of(zr + mr);
  ai = half_of(zi - mi);
  br = half_of(zi + mi);
  bi = half_of(mr - zr);
}

// chunk w of a staged plane in natural order, and element 0 of it
__device__ __forceinline__ u4 staged_chunk(const uint8_t* plane, uint32_t w) {
  const u4 v = *reinterpret_cast<const u4*>(plane + 16u * (w ^ ((w >> 3) & 1u)));
  return ((w >> 4) & 1u) ? u4{v.z, v.w, v.x, v.y} : v;
}
__device__ __forceinline__ uint16_t staged_elem0(const uint8_t* plane, uint32_t w) {
  return *reinterpret_cast<const uint16_t*>(plane + 16u * (w ^ ((w >> 3) & 1u)) + 8u * ((w >> 4) & 1u));
}

// ---- the epilogue's own
// One float32 product and one float32 sum, each rounded on its own. Device code is compiled with contraction on, and this
// toolchain's __fmul_rn / __fadd_rn are a plain `x * y` and `x + y` that the compiler fuses like any other (with them, the first GPU
// run had every fourth band energy one ulp off the restatement): the pragma is what keeps them apart.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
// the power of one bin from its binary16 halves: two exact squares, one rounded sum, one rounded product with the gain
__device__ __forceinline__ float power_of(uint16_t re, uint16_t im, float gain) {
  const float a = rsplit::h2f(re), b = rsplit::h2f(im);
  return mul_rn(gain, add_rn(mul_rn(a, a), mul_rn(b, b)));
}
// dword of bin k < n / 2 in the power image of a plane
__device__ __forceinline__ uint32_t image_dword(uint32_t k) { return k ^ (((k >> 5) & 1u) << 2); }

// one band: its first bin, its bins, and where its weights start in the plan's weight array
struct band {
  uint32_t start, count, offset, reserved_;
};

// in: real binary16, signal r at + r * in_sig halves, 8 * geo.chunks samples each. window: n halves. out: fp32, frame g at
// + g * out_frame floats: bins 0 .. n / 2 (kBands = false) or nbands band energies (kBands = true, with `bands` the nbands
// descriptors and `weights` what they point into). total = rows * geo.frames frames, batch = ceil(total / 2) transforms. tables: a
// k256r::build_tables(R) blob.
template <int R, bool kBands>
__global__ __launch_bounds__(k4096::kThreads, 2) void spec_kernel(
    const uint16_t* in, const uint16_t* __restrict__ window, float* out, uint64_t in_sig, uint64_t out_frame, geometry geo, uint32_t total,
    uint32_t batch, uint32_t live, const uint8_t* __restrict__ tables, float gain, uint32_t nbands, const band* __restrict__ bands,
    const float* __restrict__ weights) {
  using namespace k4096;
  constexpr int kPerWave = 16 / R;          // transforms per wave iteration
  constexpr int kPlane = 512 * R;           // bytes of one plane of one transform
  constexpr uint32_t kChunks = 32 * R;      // 16-byte chunks of one plane: n / 8
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
  // the wave's bin-n / 2 powers, one per frame of a group (band kernels only)
  float* const nyq = reinterpret_cast<float*>(lds + lds_bytes<R>()) + wave * (2 * kPerWave);
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3, x = lane & 15;
  // transposed read of tile u: row n1 = 4 g + q, block u ^ swz(n1), bytes 8 p of it
  const int n1r = 4 * g + q;
  const uint8_t* const tr_row = wl + 32 * R * n1r + 8 * p;
  const int sw = swz(R, n1r);
  // the image: LDS chunk c = 64 pq + lane of a plane <- row n1 = c / 2R, block (c % 2R) / 2 ^ swz(n1), half c & 1 of the frame
  int32_t src_chunk[R / 2];   // the frame chunk slot `lane` of 1-KiB piece pq of a plane holds
#pragma unroll
  for (int pq = 0; pq < R / 2; ++pq) {
    const int c = 64 * pq + lane;
    const int n1 = c / (2 * R), cc = c % (2 * R);
    src_chunk[pq] = 2 * R * n1 + 2 * ((cc >> 1) ^ swz(R, n1)) + (cc & 1);
  }
  // staging position of a lane's 8-byte piece inside a segment's 512 bytes (k256r.hpp)
  const uint32_t stage_off = 32u * x + 16u * ((g >> 1) ^ ((x >> 2) & 1)) + 8u * ((g & 1) ^ ((x >> 3) & 1));

  const uint32_t groups = (batch + kPerWave - 1) / kPerWave;
  // live waves and the stride over the groups: as fft256r_kernel
  const uint32_t stride_g = gridDim.x * live;
  uint32_t grp = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(wave) < live ? blockIdx.x * live + wave : groups);
  if (grp >= groups) return;

  // the window, once per wave: chunk src_chunk[pq] is what slot `lane` of piece pq is multiplied with, whatever the transform
  u4 wv[R / 2];
#pragma unroll
  for (int pq = 0; pq < R / 2; ++pq) wv[pq] = *reinterpret_cast<const u4*>(window + 8 * src_chunk[pq]);

  const u4 zero = {0, 0, 0, 0};
  do {
    const uint32_t b0 = grp * kPerWave;
    const uint32_t nb = (batch - b0 < kPerWave) ? (batch - b0) : kPerWave;   // ragged last group

    // ---- the image of the group (stft256r_kernel's): w (.) x in the slots whose source chunk lies in [0, L / 8), zeros everywhere
    // else. A plane past the last frame takes the last frame again. All wave-uniform; the 16 loads are issued before the first
    // product is formed.
    uint32_t fr = 2 * b0;
    uint32_t r = fr / geo.frames;
    int32_t f = static_cast<int32_t>(fr - r * geo.frames);
    u4 xv[16];
    int32_t first_of[2 * kPerWave];
#pragma unroll
    for (int pl = 0; pl < 2 * kPerWave; ++pl) {
      const int32_t first = f * geo.hop - geo.pad;                         // source chunk of frame chunk 0: negative in front of sample 0
      const int32_t spare = first > 0 ? first : 0;                         // below L / 8: a frame starts before sample L + pad - n < L
      const uint8_t* const src = reinterpret_cast<const uint8_t*>(in + static_cast<uint64_t>(r) * in_sig);
      first_of[pl] = first;
#pragma unroll
      for (int pq = 0; pq < R / 2; ++pq) {
        const int32_t chunk = first + src_chunk[pq];
        const uint32_t off = static_cast<uint32_t>(chunk >= 0 && chunk < geo.chunks ? chunk : spare) * 16u;        // below 2^27
        xv[pl * (R / 2) + pq] = __builtin_nontemporal_load(reinterpret_cast<const u4*>(src + off));
      }
      if (fr + 1 < total) {                                                // the next frame exists: step to it
        ++fr;
        if (++f == static_cast<int32_t>(geo.frames)) {
          f = 0;
          ++r;
        }
      }
    }
    // every slot of the 16-KiB image is written: the staged spectra or the powers of the previous group lie there
#pragma unroll
    for (int pl = 0; pl < 2 * kPerWave; ++pl)
#pragma unroll
      for (int pq = 0; pq < R / 2; ++pq) {
        const int i = pl * (R / 2) + pq;
        const int32_t chunk = first_of[pl] + src_chunk[pq];
        const u4 prod = mul8(xv[i], wv[pq]);
        *reinterpret_cast<u4*>(wl + i * 1024 + lane * 16) = chunk >= 0 && chunk < geo.chunks ? prod : zero;
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the loads are the compiler's to count: every product above waited for its own)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the image, products and zero fill, has landed before stage 1 reads it

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
      // the transposed reads of transform t have all returned (their data went through the MFMAs above)
      uint8_t* const slot = wl + t * 2 * kPlane + stage_off;
#pragma unroll
      for (int s = 0; s < R; ++s) {
        *reinterpret_cast<u2*>(slot + 512 * s) = u2{pk_re[s][0], pk_re[s][1]};
        *reinterpret_cast<u2*>(slot + kPlane + 512 * s) = u2{pk_im[s][0], pk_im[s][1]};
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the staged spectra have landed before the split reads them

    // ---- the split (stft256r_kernel's) and the powers: task (t, v), v < n / 16, takes Z chunk v (bins 8 v .. 8 v + 7) and its
    // mirror, chunk n / 8 - 1 - v; bin 8 v pairs with element 0 of chunk (n / 8 - v) mod n / 8. v = 0 also takes bin n / 2.
    f4 pa[4][2], pb[4][2];     // the powers of frame A and frame B of the task of round i (kBands: all four rounds before any is written)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t task = 64u * i + lane;
      const uint32_t t = task / (kChunks / 2), v = task % (kChunks / 2);
      const uint8_t* const z_re = wl + t * 2 * kPlane;
      const uint8_t* const z_im = z_re + kPlane;
      const u4 xr = staged_chunk(z_re, v), xi = staged_chunk(z_im, v);
      const u4 yr = staged_chunk(z_re, kChunks - 1 - v), yi = staged_chunk(z_im, kChunks - 1 - v);
      const uint16_t y0r = staged_elem0(z_re, (kChunks - v) & (kChunks - 1));
      const uint16_t y0i = staged_elem0(z_im, (kChunks - v) & (kChunks - 1));
      uint16_t zr[8], zi[8], mr[8], mi[8];
      __builtin_memcpy(zr, &xr, 16);
      __builtin_memcpy(zi, &xi, 16);
      __builtin_memcpy(mr, &yr, 16);
      __builtin_memcpy(mi, &yi, 16);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        uint16_t ar, ai, br, bi;
        split_bin(zr[j], zi[j], j ? mr[8 - j] : y0r, j ? mi[8 - j] : y0i, ar, ai, br, bi);
        pa[i][j >> 2][j & 3] = power_of(ar, ai, gain);
        pb[i][j >> 2][j & 3] = power_of(br, bi, gain);
      }
      const uint32_t fr_a = 2 * (b0 + t);
      const bool has_b = fr_a + 1 < total;                                 // false: the last frame of an odd total, paired with itself
      float* const a = out + static_cast<uint64_t>(fr_a) * out_frame;      // (formed, not used, for a transform the group lacks)
      if constexpr (!kBands) {
        if (t < nb) {                                                      // a ragged group stores nothing for the transforms it lacks
          __builtin_nontemporal_store(pa[i][0], reinterpret_cast<f4*>(a + 8 * v));
          __builtin_nontemporal_store(pa[i][1], reinterpret_cast<f4*>(a + 8 * v + 4));
          if (has_b) {
            __builtin_nontemporal_store(pb[i][0], reinterpret_cast<f4*>(a + out_frame + 8 * v));
            __builtin_nontemporal_store(pb[i][1], reinterpret_cast<f4*>(a + out_frame + 8 * v + 4));
          }
        }
      }
      if (v == 0) {                                                        // bin n / 2
        const uint16_t nr = staged_elem0(z_re, kChunks / 2), ni = staged_elem0(z_im, kChunks / 2);
        uint16_t qr, qi, sr, si;
        split_bin(nr, ni, nr, ni, qr, qi, sr, si);
        const float na = power_of(qr, qi, gain), nbp = power_of(sr, si, gain);
        if constexpr (kBands) {
          // a region of its own, read by the band tasks alone, and the previous group's have been waited for
          nyq[2 * t] = na;
          nyq[2 * t + 1] = nbp;
        } else if (t < nb) {
          a[128 * R] = na;
          if (has_b) a[out_frame + 128 * R] = nbp;
        }
      }
    }
    if constexpr (kBands) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every task of the four rounds has read its halves: the planes are consumed
      // ---- the power image: frame A of transform t over the RE plane, frame B over the IM plane, a task's 32 bytes at 32 v
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t task = 64u * i + lane;
        const uint32_t t = task / (kChunks / 2), v = task % (kChunks / 2);
        uint8_t* const img = wl + t * 2 * kPlane + 32u * v;
        const uint32_t lo = 16u * ((v >> 2) & 1u);         // image_dword: the halves exchanged for tasks 4 .. 7 of every eight
        *reinterpret_cast<f4*>(img + lo) = pa[i][0];
        *reinterpret_cast<f4*>(img + (lo ^ 16u)) = pa[i][1];
        *reinterpret_cast<f4*>(img + kPlane + lo) = pb[i][0];
        *reinterpret_cast<f4*>(img + kPlane + (lo ^ 16u)) = pb[i][1];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the image and the bin-n / 2 powers have landed before a band task reads them

      // ---- the band tasks over the frames of the group that exist
      const uint32_t have = total - 2 * b0;
      const uint32_t nframes = have < 2 * nb ? have : 2 * nb;
      const uint32_t ntasks = nframes * nbands;             // at most 16 * 1024
      for (uint32_t task = lane; task < ntasks; task += 64) {
        const uint32_t fi = task / nbands, j = task - fi * nbands;
        const band bd = bands[j];
        const float* const w = weights + bd.offset;
        const float* const img = reinterpret_cast<const float*>(wl + fi * kPlane);   // frame fi: transform fi / 2, plane fi & 1
        float acc = 0.0f;
        for (uint32_t c = 0; c < bd.count; ++c) {
          const uint32_t k = bd.start + c;
          const float pw = k == 128u * R ? nyq[fi] : img[image_dword(k)];
          const float term = mul_rn(w[c], pw);
          acc = c ? add_rn(acc, term) : term;
        }
        out[static_cast<uint64_t>(2 * b0 + fi) * out_frame + j] = acc;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // image read out before the next group's image is built
    grp += stride_g;
  } while (grp < groups);
}

}  // namespace spec256r
