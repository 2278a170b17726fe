// olan.hpp — windowed overlap-add of the time-domain frames of an inverse STFT at the frame lengths 512, 1024 and 2048
// (include/tfft_istftn.h), in a fixed order: istft/ola.hpp with the frame length n in its geometry struct instead of the literals
// 4096 / 4088. One kernel for all three n.
//
// Sample t of signal r lies under the frames f with 0 <= j = t + pad - f * hop < n. With f ASCENDING and both sums starting from +0:
//
//   num = sum fp32(w[j]) * fp32(v_g[j])        den = sum fp32(w[j]) * fp32(w[j])        g = r * F + f
//
// A product of two binary16 values is exact in fp32 (22 significant bits, exponents far inside the range), so only the order of the
// adds matters, and fusing a product into its add changes no bit. y = fp16(num / den) where den > 0, the division correctly rounded;
// y = +0 where den = 0: samples no frame covers (the gaps of hop > n, a tail the last frame does not reach) and samples that lie
// only under zeros of the window. With raw, y = fp16(num) everywhere.
//
// One thread per 16-byte output chunk (8 samples). hop and pad are multiples of 8, so a chunk lies wholly inside or outside a frame:
// per frame one 16-byte load from the workspace and one from the window (at most 4 KiB, it stays in cache), eight num and eight den
// accumulators, one 16-byte store. No atomics: the order of the adds is the contract.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../csrc/rsplit.hpp"

namespace olan {

constexpr int kOlaBlock = 256;

// L / 8 chunks per signal; hop in samples, below 2^28: (F - 1) * hop <= L + 2 pad - n for F > 1, and the host passes L + 2 pad for a
// plan with one frame per signal, whatever its hop (ola_hop of conv/stft_host.hpp), so the signed 64-bit frame range below cannot overflow
struct ola_geometry {
  uint64_t rows, chunks, hop, out_stride;
  uint32_t pad, frames, n;
};

// frames_in: frame g at + g * geo.n halves. out: signal r at + r * geo.out_stride halves, 8 * geo.chunks samples each.
__global__ __launch_bounds__(kOlaBlock) void ola_kernel(const uint16_t* __restrict__ frames_in, const uint16_t* __restrict__ window, uint16_t* __restrict__ out,
                                                        ola_geometry geo, int raw) {
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const uint64_t total = geo.rows * geo.chunks;
  const int64_t reach = static_cast<int64_t>(geo.n) - 8;                   // the last chunk of a frame starts at sample n - 8
  for (uint64_t c = blockIdx.x * static_cast<uint64_t>(kOlaBlock) + threadIdx.x; c < total; c += static_cast<uint64_t>(gridDim.x) * kOlaBlock) {
    const uint64_t r = c / geo.chunks;
    const uint64_t t0 = (c - r * geo.chunks) * 8;
    const int64_t s = static_cast<int64_t>(t0 + geo.pad);                  // position of the chunk in the padded signal
    const int64_t hop = static_cast<int64_t>(geo.hop);
    const int64_t f_hi = min(static_cast<int64_t>(geo.frames) - 1, s / hop);
    const int64_t f_lo = s - reach > 0 ? (s - reach + hop - 1) / hop : 0;    // ceil((s - (n - 8)) / hop), not below 0
    float num[8], den[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) num[e] = den[e] = 0.f;
    for (int64_t f = f_lo; f <= f_hi; ++f) {
      const uint64_t j = static_cast<uint64_t>(s - f * hop);               // 0 .. n - 8, a multiple of 8
      const u4 vv = *reinterpret_cast<const u4*>(frames_in + (r * geo.frames + static_cast<uint64_t>(f)) * geo.n + j);
      const u4 wv = *reinterpret_cast<const u4*>(window + j);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float w = rsplit::h2f(static_cast<uint16_t>(wv[e >> 1] >> (16 * (e & 1))));
        const float v = rsplit::h2f(static_cast<uint16_t>(vv[e >> 1] >> (16 * (e & 1))));
        num[e] = num[e] + w * v;
        den[e] = den[e] + w * w;
      }
    }
    uint16_t y[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = raw ? rsplit::f2h(num[e]) : den[e] > 0.f ? rsplit::f2h(__fdiv_rn(num[e], den[e])) : uint16_t{0};
    const u4 yv = {y[0] | (uint32_t{y[1]} << 16), y[2] | (uint32_t{y[3]} << 16), y[4] | (uint32_t{y[5]} << 16), y[6] | (uint32_t{y[7]} << 16)};
    *reinterpret_cast<u4*>(out + r * geo.out_stride + t0) = yv;
  }
}

}  // namespace olan
