// host_math.hpp — the host arithmetic every convolution library (conv, lconv, gconv, sconv, gsconv, bconv, gbconv, cconv, gcconv)
// shares: binary16 conversion, the fp64 spectrum builder, the filter image, the overlap tests and the overlap-save geometry.
//
// Plain C++17: no HIP, no library header, no state. Each library includes it into its one translation unit; nothing here is
// exported, and including it links nothing. tests/cxx/conv_host_math.cpp checks it on the CPU.
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace host_math {

inline bool is_pow2(uint64_t v) { return v && !(v & (v - 1)); }
inline int ilog2(uint64_t v) {
  int l = 0;
  while (v >>= 1) ++l;
  return l;
}
inline size_t round256(size_t v) { return (v + 255) & ~size_t{255}; }

constexpr uint64_t kMinN = 256, kMaxN = uint64_t{1} << 26;        // the transform lengths of tfft_conv.h
constexpr uint64_t kN = 4096, kMaxLength = uint64_t{1} << 26;      // the window of the one-pass kernels; the longest sequence
constexpr uint64_t kMaxTaps = 2049;                                // the halo of a 4096-sample window, plus one
constexpr uint64_t kWaves = 2048;                                  // 256 CUs x 8 waves: the work units the default P aims at

// the transform length of a composed causal convolution: the power of two >= length + taps - 1, 0 when there is none in range
inline uint64_t fft_length(uint64_t length, uint64_t taps) {
  if (!length || !taps || length > kMaxN || taps > kMaxN) return 0;
  const uint64_t need = std::max(length + taps - 1, kMinN);
  uint64_t n = kMinN;
  while (n < need) n *= 2;
  return n > kMaxN ? 0 : n;
}

// ---- the overlap-save geometry, fixed by the number of taps alone (include/tfft_sconv.h); a context does not change it
inline uint64_t halo_of(uint64_t taps) { return (taps - 1 + 63) / 64 * 64; }
inline uint64_t hop_of(uint64_t taps) { return kN - halo_of(taps); }
inline uint64_t segments_of(uint64_t length, uint64_t taps) { return (length + hop_of(taps) - 1) / hop_of(taps); }
inline uint64_t carry_min_of(uint64_t taps) { return (taps - 1 + 7) / 8 * 8; }
// partial sums per channel of the tap gradient: one per item until the chip's waves are all busy, capped by the caller
inline uint64_t partials_of(uint64_t rows, uint64_t channels, uint64_t length, uint64_t taps, uint64_t cap) {
  const uint64_t per_channel = (rows + 1) / 2 * segments_of(length, taps);
  const uint64_t p = std::min(per_channel, (kWaves + channels - 1) / channels);
  return cap ? std::min(p, cap) : p;
}
inline uint64_t kpad_of(uint64_t taps) { return (taps + 7) / 8 * 8; }

// ---- overlap tests
// Element-exact test whether two sets of sequences share a half: `count` blocks of la halves, sa halves apart, at pa, against
// `count` blocks of lb halves, sb apart, at pb (a context has a length of its own). The test of tfft_exec.
inline bool seqs_overlap(const void* pa, uint64_t sa, uint64_t la, const void* pb, uint64_t sb, uint64_t lb, uint64_t count) {
  if (la == 0 || lb == 0) return false;
  const uintptr_t a = reinterpret_cast<uintptr_t>(pa), b = reinterpret_cast<uintptr_t>(pb);
  const uintptr_t a_end = a + 2 * ((count - 1) * sa + la), b_end = b + 2 * ((count - 1) * sb + lb);
  if (a_end <= b || b_end <= a) return false;
  if (count == 1 || sa != sb) return true;            // different strides: conservative
  // one period: a block of la halves starting d halves behind the start of a block of lb halves, both repeating every sa
  const uint64_t d = a >= b ? static_cast<uint64_t>(a - b) / 2 % sa : (sa - static_cast<uint64_t>(b - a) / 2 % sa) % sa;
  return d < lb || d + la > sa;
}
// a block of `bytes` against the whole extent of a set of sequences, gaps included (conservative); a null set or an empty one
// overlaps nothing
inline bool block_overlaps(const void* block, uint64_t bytes, const void* seqs, uint64_t stride, uint64_t count, uint64_t len) {
  if (!seqs || len == 0) return false;
  const uintptr_t a = reinterpret_cast<uintptr_t>(block), b = reinterpret_cast<uintptr_t>(seqs);
  return a < b + 2 * ((count - 1) * stride + len) && b < a + bytes;
}
// two blocks of bytes
inline bool blocks_overlap(const void* pa, uint64_t bytes_a, const void* pb, uint64_t bytes_b) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(pa), b = reinterpret_cast<uintptr_t>(pb);
  return a < b + bytes_b && b < a + bytes_a;
}

// ---- binary16 on the host, bit by bit (round to nearest even, one rounding from fp64)
inline double from_half(uint16_t h) {
  const int e = (h >> 10) & 31, m = h & 1023;
  double v;
  if (e == 0)
    v = std::ldexp(static_cast<double>(m), -24);
  else if (e == 31)
    v = m ? NAN : INFINITY;
  else
    v = std::ldexp(static_cast<double>(m + 1024), e - 25);
  return (h & 0x8000) ? -v : v;
}
inline uint16_t to_half(double v) {
  const uint16_t sign = std::signbit(v) ? 0x8000 : 0;
  if (v != v) return sign | 0x7e00;
  const double a = std::fabs(v);
  if (a >= 65520.0) return sign | 0x7c00;
  if (a == 0.0) return sign;
  int e2;
  (void)std::frexp(a, &e2);                                 // a = f * 2^e2, f in [0.5, 1)
  const int e = std::max(e2 - 1, -14);                      // the binade whose spacing applies (subnormals share the lowest)
  const long r = std::lrint(std::ldexp(a, 10 - e));         // exact scaling, then the one rounding (to nearest even)
  if (e == -14 && r < 1024) return sign | static_cast<uint16_t>(r);
  return sign | static_cast<uint16_t>(((e + 15) << 10) + (r - 1024));    // r = 2048 carries into the exponent
}

// in-place radix-2 fp64 FFT (forward, unscaled). Twiddles w^k = A[k >> s] B[k & mask] from two tables of about sqrt(n) entries
// (64 each at n = 4096), each entry from sin / cos directly: one product per twiddle, no error growth along a recurrence.
inline void fft64(std::vector<std::complex<double>>& a) {
  const uint64_t n = a.size();
  const int lg = ilog2(n);
  for (uint64_t i = 1, j = 0; i < n; ++i) {
    uint64_t bit = n >> 1;
    for (; j & bit; bit >>= 1) j ^= bit;
    j ^= bit;
    if (i < j) std::swap(a[i], a[j]);
  }
  const int s = lg / 2;
  const uint64_t lo_n = uint64_t{1} << s, hi_n = std::max<uint64_t>(n >> s, 1);
  std::vector<std::complex<double>> ta(hi_n), tb(lo_n);
  const double step = -2.0 * M_PI / static_cast<double>(n);
  for (uint64_t i = 0; i < hi_n; ++i) ta[i] = {std::cos(step * static_cast<double>(i << s)), std::sin(step * static_cast<double>(i << s))};
  for (uint64_t i = 0; i < lo_n; ++i) tb[i] = {std::cos(step * static_cast<double>(i)), std::sin(step * static_cast<double>(i))};
  for (uint64_t m = 2; m <= n; m *= 2) {
    const uint64_t half = m / 2, mul = n / m;
    for (uint64_t k = 0; k < n; k += m)
      for (uint64_t j = 0; j < half; ++j) {
        const uint64_t idx = j * mul;
        const std::complex<double> w = ta[idx >> s] * tb[idx & (lo_n - 1)];
        const std::complex<double> u = a[k + j], t = w * a[k + j + half];
        a[k + j] = u + t;
        a[k + j + half] = u - t;
      }
  }
}

// one filter: H' = FFT of the taps zero-padded to n, with the skip weight added to tap 0 in fp64, each component rounded once;
// exactly Hermitian, Im of bins 0 and n / 2 exactly 0. A skip of zero adds nothing, not even to the sign of a zero tap: an
// ungated library passes 0 and gets H.
inline void spectrum(const uint16_t* taps, uint64_t num_taps, uint16_t skip, uint64_t n, uint16_t* out_re, uint16_t* out_im) {
  std::vector<std::complex<double>> a(n);
  for (uint64_t j = 0; j < num_taps; ++j) a[j] = from_half(taps[j]);
  if (skip & 0x7fff) a[0] += from_half(skip);
  fft64(a);
  for (uint64_t k = 0; k <= n / 2; ++k) {
    const uint16_t re = to_half(a[k].real());
    const uint16_t im = (k == 0 || k == n / 2) ? 0 : to_half(a[k].imag());
    out_re[k] = re;
    out_im[k] = im;
    if (k && k < n / 2) {
      out_re[n - k] = re;
      out_im[n - k] = (im & 0x7fff) ? (im ^ 0x8000) : 0;        // conj; a zero stays +0
    }
  }
}

// ---- the filter image of the one-pass kernels (conv/conv4096.hpp): 16 KiB per filter as binary16, [RE 4096 | IM 4096]
// slot of bin k in a plane of the image: k = k0 + 16 k1 + 256 (4 g + r2), k0 = 8 half + j, sits at
// ((half * 4 + r2) * 64 + lane) * 8 + j with lane = 16 g + k1; a bijection of 0 .. 4095
constexpr uint32_t filter_slot(uint32_t k) {
  const uint32_t k0 = k & 15, k1 = (k >> 4) & 15, k2 = k >> 8;
  const uint32_t half = k0 >> 3, j = k0 & 7, g = k2 >> 2, r2 = k2 & 3;
  return ((half * 4 + r2) * 64 + 16 * g + k1) * 8 + j;
}
// one filter's spectrum, 4096 bins in natural order, into slot order: H, or conj(H) for a gradient plan (the sign bit flipped,
// exact; a zero stays +0, so the image is as exactly Hermitian as H is)
inline void filter_image(const uint16_t* re, const uint16_t* im, bool conjugate, uint16_t* img) {
  for (uint32_t k = 0; k < kN; ++k) {
    const uint32_t slot = filter_slot(k);
    img[slot] = re[k];
    img[kN + slot] = !conjugate ? im[k] : (im[k] & 0x7fff) ? (im[k] ^ 0x8000) : 0;
  }
}

}  // namespace host_math
