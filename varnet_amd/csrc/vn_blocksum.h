// The sum of one float per thread over a 256-thread block, in a fixed order: a shuffle tree per wave, then the four wave sums
// left to right.  Every per-block loss or gradient partial of the engine is formed by it, so two evaluations give the same bits.
// red: 4 floats of LDS; the leading barrier lets a caller reuse it for the next sum.  Every thread of the block must call.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float block_sum(float v, float* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
