// cmul.hpp — pointwise product of a batch of spectra with per-channel filter spectra, in place (the middle step of the composed
// convolution path, tfft_conv.hip). Memory bound: 16-byte vectors, grid-stride.
//
// spec: [batch][RE n | IM n] binary16 (the composed plan's workspace); filt: [filters][RE n | IM n] in the SAME bin order as the
// spectra (the plan's filter image, permuted at tfft_conv_plan_set_filter where the transforms leave the transposed order), so
// the kernel knows nothing about orders. Signal b takes filter b % filters. Arithmetic: binary16 -> fp32, H times `scale` (an
// exact power of two: the factor n that the sequentially scaled forward transform took out), complex product in scalar fp32
// with one fma per component, ONE rounding to binary16 (RNE). tests/conv_ref.py restates it in numpy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cmul {

constexpr int kThreads = 256;

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));

// lg_v = log2(n / 8): vectors per plane; total = batch * n / 8
__global__ __launch_bounds__(kThreads) void cmul_kernel(uint16_t* spec, const uint16_t* __restrict__ filt, uint32_t lg_v, uint64_t total,
                                                        uint32_t filters, float scale) {
  const uint64_t step = static_cast<uint64_t>(gridDim.x) * kThreads;
  const uint64_t n = uint64_t{8} << lg_v;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kThreads + threadIdx.x; i < total; i += step) {
    const uint64_t b = i >> lg_v, v = i & ((uint64_t{1} << lg_v) - 1);
    uint16_t* const x_re = spec + b * 2 * n + 8 * v;
    uint16_t* const x_im = x_re + n;
    const uint16_t* const f_re = filt + (b % filters) * 2 * n + 8 * v;
    const h8 xr = __builtin_bit_cast(h8, *reinterpret_cast<const u4*>(x_re));
    const h8 xi = __builtin_bit_cast(h8, *reinterpret_cast<const u4*>(x_im));
    const h8 hr = __builtin_bit_cast(h8, *reinterpret_cast<const u4*>(f_re));
    const h8 hi = __builtin_bit_cast(h8, *reinterpret_cast<const u4*>(f_re + n));
    h8 zr, zi;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float ar = static_cast<float>(xr[j]), ai = static_cast<float>(xi[j]);
      const float cr = static_cast<float>(hr[j]) * scale, ci = static_cast<float>(hi[j]) * scale;
      float pr = __builtin_fmaf(ar, cr, -(ai * ci)), pi = __builtin_fmaf(ar, ci, ai * cr);
      // the fp32 values are the contract (and what conv_ref.cmul restates): keep the compiler from folding the fma and the
      // conversion into one v_fma_mix*_f16, whose rounding is not that of the two steps
      asm volatile("" : "+v"(pr), "+v"(pi));
      zr[j] = static_cast<_Float16>(pr);
      zi[j] = static_cast<_Float16>(pi);
    }
    *reinterpret_cast<u4*>(x_re) = __builtin_bit_cast(u4, zr);
    *reinterpret_cast<u4*>(x_im) = __builtin_bit_cast(u4, zi);
  }
}

}  // namespace cmul
