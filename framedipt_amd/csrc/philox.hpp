// philox.hpp — counter-based N(0,1) draws for the step kernels (noise="device"; contract in include/fdipt.h, "device noise").
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) restated from the paper: a draw is a
// pure function of (key, purpose, step k, residue i, component), never of where or when it is computed.  tests/noise_ref.py is the same
// text in NumPy; the two and the header's contract change together.
//   key     = the sample's 64-bit noise key (low word, high word)
//   counter = (i, k, purpose, j): j = 0 gives components x, y; j = 1 gives z (its second normal is discarded)
//   uniform = ((a >> 5) * 2^26 + (b >> 6) + 0.5) * 2^-53 in (0, 1) from two output words: words 0, 1 -> u0, words 2, 3 -> u1
//   normal  = Box-Muller in float64: r = sqrt(-2 log u0), z0 = r cos(2 pi u1), z1 = r sin(2 pi u1)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

enum : uint32_t { FD_NOISE_REV_ROT = 0, FD_NOISE_REV_TRANS = 1, FD_NOISE_FWD_ROT = 2, FD_NOISE_FWD_TRANS = 3, FD_NOISE_PURPOSES = 4 };

__device__ __forceinline__ void fd_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
__device__ __forceinline__ double fd_uniform53(uint32_t a, uint32_t b) {  // every step exact in float64
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 0.5) * 0x1p-53;
}
// the three N(0,1) components of residue i of the sample with `key` at step k, for one purpose
__device__ __forceinline__ void fd_noise3(uint64_t key, uint32_t i, uint32_t k, uint32_t purpose, double z[3]) {
#pragma clang fp contract(off)
  const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
  uint32_t c[4] = {i, k, purpose, 0u};
  fd_philox4x32_10(c, k0, k1);
  double r = sqrt(-2.0 * log(fd_uniform53(c[0], c[1])));
  double a = 6.283185307179586 * fd_uniform53(c[2], c[3]);
  z[0] = r * cos(a);
  z[1] = r * sin(a);
  uint32_t d[4] = {i, k, purpose, 1u};
  fd_philox4x32_10(d, k0, k1);
  r = sqrt(-2.0 * log(fd_uniform53(d[0], d[1])));
  a = 6.283185307179586 * fd_uniform53(d[2], d[3]);
  z[2] = r * cos(a);
}
