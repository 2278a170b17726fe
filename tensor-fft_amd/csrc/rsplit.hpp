// rsplit.hpp — the split and merge arithmetic of the real-input transforms (include/tfft.h, tfft_rplan_*), shared by every path
// that computes it: the fused epilogue of the N = 4096 kernel (k4096.hpp) and the streaming split / merge passes (rfft.hpp).
//
// Two real signals a, b of length N travel as one complex signal z = a + i b. With Z = DFT(z) and Z[N] = Z[0], for k = 0 .. N/2:
//
//   A.re[k] = 0.5 (Zr[k] + Zr[N-k])    A.im[k] = 0.5 (Zi[k] - Zi[N-k])
//   B.re[k] = 0.5 (Zi[k] + Zi[N-k])    B.im[k] = 0.5 (Zr[N-k] - Zr[k])
//
// and back (merge), with the IM of bins 0 and N/2 ignored:
//
//   k <= N/2:  Zr[k] = A.re[k] - B.im[k],          Zi[k] = A.im[k] + B.re[k]
//   k >  N/2:  Zr[k] = A.re[N-k] + B.im[N-k],      Zi[k] = B.re[N-k] - A.im[N-k]
//   k = 0, N/2: Zr[k] = A.re[k],                   Zi[k] = B.re[k]
//
// fp16 operands widened to fp32, one IEEE add, an exact * 0.5 (split only), one round to nearest even to fp16. These exact
// operations in exactly this order are what tests/test_rfft_host.py restates with numpy float32, and what makes the fused and the
// two-pass R2C agree bit for bit. Scalar fp32 only (the library is built with -fno-slp-vectorize, see k4096.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsplit {

__device__ __forceinline__ float h2f(uint16_t h) { return static_cast<float>(__builtin_bit_cast(_Float16, h)); }
__device__ __forceinline__ uint16_t f2h(float f) { return __builtin_bit_cast(uint16_t, static_cast<_Float16>(f)); }

// bin k of both half spectra from Z[k] = (xr, xi) and Z[N-k] = (yr, yi)
__device__ __forceinline__ void split_bin(uint16_t xr, uint16_t xi, uint16_t yr, uint16_t yi, uint16_t& ar, uint16_t& ai,
                                          uint16_t& br, uint16_t& bi) {
  const float zr = h2f(xr), zi = h2f(xi), mr = h2f(yr), mi = h2f(yi);
  ar = f2h(0.5f * (zr + mr));
  ai = f2h(0.5f * (zi - mi));
  br = f2h(0.5f * (zi + mi));
  bi = f2h(0.5f * (mr - zr));
}

// Z[k] for k <= N/2 from bin k of A and B (edge: k = 0 or N/2, whose IM is ignored)
__device__ __forceinline__ void merge_low(uint16_t ar, uint16_t ai, uint16_t br, uint16_t bi, bool edge, uint16_t& zr,
                                          uint16_t& zi) {
  if (edge) {
    zr = ar;
    zi = br;
    return;
  }
  zr = f2h(h2f(ar) - h2f(bi));
  zi = f2h(h2f(ai) + h2f(br));
}

// Z[k] for k > N/2 from bin N-k of A and B (edge: N-k = N/2)
__device__ __forceinline__ void merge_high(uint16_t ar, uint16_t ai, uint16_t br, uint16_t bi, bool edge, uint16_t& zr,
                                           uint16_t& zi) {
  if (edge) {
    zr = ar;
    zi = br;
    return;
  }
  zr = f2h(h2f(ar) + h2f(bi));
  zi = f2h(h2f(br) - h2f(ai));
}

}  // namespace rsplit
