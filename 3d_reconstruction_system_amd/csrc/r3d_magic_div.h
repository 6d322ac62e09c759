// floor(x / d) by a host-made magic number: one 32 x 32 -> 64 bit multiply and a shift per lane instead of a hardware divide.
// Shared by the fused launches (r3d_fuse.hip) and the normals' view lookup (r3d_knn.hip).  Internal to libr3d_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace r3d_magic {

// Magic number for floor(x / d), exact for every x < 2^31 and d >= 1 (round-up method):
//   s = ceil(log2 d), m = floor(2^(31+s) / d) + 1 (< 2^32), x / d = (x * m) >> (31 + s).
// m*d - 2^(31+s) lies in (0, d] <= 2^s, which is the exactness condition for 31-bit x.
inline void make_magic(uint32_t d, uint32_t* magic, uint32_t* shift) {
  uint32_t s = 0;
  while (((uint64_t)1 << s) < d) ++s;
  *magic = (uint32_t)((((uint64_t)1 << (31 + s)) / d) + 1);
  *shift = 31 + s;
}

__device__ __forceinline__ uint32_t magic_div(uint32_t x, uint32_t magic, uint32_t shift) {
  return (uint32_t)(((uint64_t)x * magic) >> shift);
}

}  // namespace r3d_magic
