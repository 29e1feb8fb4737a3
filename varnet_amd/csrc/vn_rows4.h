// Four rows per thread: the 16-byte vector type of the 4-row kernels, its load and store, and the rule that picks them -- the
// 4-row kernel when the row count is a multiple of 4 and every stream the kernel touches is 16-byte aligned (nullptr counts),
// else the 1-row kernel.  (vn_gemm.hip, of the frozen layer-by-layer route, keeps its own.)
#pragma once
#include <cstdint>
#include <initializer_list>

#include <hip/hip_runtime.h>

typedef float f32x4t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4t load4(const float* p, long i) { return reinterpret_cast<const f32x4t*>(p)[i]; }
__device__ __forceinline__ void store4(float* p, long i, f32x4t v) { reinterpret_cast<f32x4t*>(p)[i] = v; }

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline bool rows4_ok(long n, std::initializer_list<const void*> ptrs) {
  bool four = n % 4 == 0;
  for (const void* p : ptrs) four = four && aligned16(p);
  return four;
}
