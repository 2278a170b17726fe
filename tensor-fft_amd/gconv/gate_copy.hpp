// gate_copy.hpp — the two ends of the composed gated causal convolution (include/tfft_gconv.h): lconv_copy's two kernels
// (lconv/pack.hpp) with the gate multiply added, at the same chunk granularity and under the same grid rule. One thread per 16-byte
// chunk, grid-stride. A product is one packed binary16 multiply: round to nearest even, subnormals kept. Like their models the
// kernels are not tuned (64-bit divisions by `channels` and `chunks` per chunk): the composed path is not the hot path.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gate_copy {

constexpr int kThreads = 256;
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ u4 mul8(u4 a, u4 b) { return __builtin_bit_cast(u4, __builtin_bit_cast(h8, a) * __builtin_bit_cast(h8, b)); }

// blocks: item it = p * channels + c at + it * 2 n halves, n = 8 << log_n8: plane 0 = p (.) x of sequence (2p, c), plane 1 = of
// (2p + 1, c), zeros from sample 8 * chunks on and for a row that does not exist (neither its sequence nor its gate is read).
// total = items * 2 * (n / 8) chunks. pre is read only when Pre; it may alias in. The blocks are read right back by the sub-plan:
// plain stores; the sequences are touched once: nt loads.
template <bool Pre>
__global__ __launch_bounds__(kThreads) void pack_kernel(const uint16_t* in, const uint16_t* pre, uint16_t* __restrict__ blocks, uint64_t in_seq,
                                                        uint64_t pre_seq, uint32_t rows, uint32_t channels, uint32_t chunks, uint32_t log_n8,
                                                        uint64_t total) {
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; t < total; t += step) {
    const uint64_t j = t & ((uint64_t{1} << log_n8) - 1);
    const uint64_t plane = t >> log_n8;                          // 2 it + (0: RE, 1: IM)
    const uint64_t it = plane >> 1, p = it / channels, c = it - p * channels;
    const uint64_t row = 2 * p + (plane & 1);
    u4 v = {0, 0, 0, 0};
    if (j < chunks && row < rows) {
      v = __builtin_nontemporal_load(reinterpret_cast<const u4*>(in + (row * channels + c) * in_seq) + j);
      if constexpr (Pre) v = mul8(v, __builtin_nontemporal_load(reinterpret_cast<const u4*>(pre + (row * channels + c) * pre_seq) + j));
    }
    reinterpret_cast<u4*>(blocks)[t] = v;
  }
}

// out: sequence s = b * channels + c at + s * out_seq halves takes the first 8 * chunks samples of plane b & 1 of item
// (b >> 1) * channels + c, times the same samples of the gate (Post). total = rows * channels * chunks.
template <bool Post>
__global__ __launch_bounds__(kThreads) void crop_kernel(const uint16_t* __restrict__ blocks, const uint16_t* post, uint16_t* out, uint64_t post_seq,
                                                        uint64_t out_seq, uint32_t channels, uint32_t chunks, uint32_t log_n8, uint64_t total) {
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kThreads;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; t < total; t += step) {
    const uint64_t s = t / chunks, j = t - s * chunks;
    const uint64_t b = s / channels, c = s - b * channels;
    const uint64_t plane = 2 * ((b >> 1) * channels + c) + (b & 1);
    u4 v = reinterpret_cast<const u4*>(blocks)[(plane << log_n8) + j];
    if constexpr (Post) v = mul8(v, __builtin_nontemporal_load(reinterpret_cast<const u4*>(post + s * post_seq) + j));
    __builtin_nontemporal_store(v, reinterpret_cast<u4*>(out + s * out_seq) + j);
  }
}

}  // namespace gate_copy
