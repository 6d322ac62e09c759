// What the mesh kernels share (r3d_mesh_cc.hip, r3d_mesh_smooth.hip): the validity rule of a triangle, stated once.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace r3d_mesh {

__device__ __forceinline__ bool tri_valid(int32_t a, int32_t b, int32_t c, uint32_t nv) {
  return (uint32_t)a < nv && (uint32_t)b < nv && (uint32_t)c < nv;   // a negative index is >= 2^31 > nv as unsigned
}

}  // namespace r3d_mesh
