// The chunk walk of the plane-streaming kernels (ops_bn.hip, ops_epilogue.hip): a block of CHUNK_BLOCK threads owns
// CHUNK_ELEMS consecutive elements of one (n, c) plane of HW elements, CHUNK_PER_THREAD per thread.  VEC (HW % 4 == 0, 16-byte
// aligned planes): two float4 per thread, the block's quads interleaved; otherwise eight scalars at stride CHUNK_BLOCK.
// Either way v[k] / ok[k] name the same element in load8 and store8, and a kernel that calls all its load8 before its first
// store8 has every load of a thread in flight at once, whatever its pointers may alias.  (ops_epilogue.hip takes the vector
// walk from here and keeps its scalar walk element at a time: see there.)
#pragma once
#include <hip/hip_runtime.h>

namespace dfe {

constexpr int CHUNK_BLOCK = 256;
constexpr int CHUNK_PER_THREAD = 8;                            // elements per thread (two float4)
constexpr int CHUNK_ELEMS = CHUNK_BLOCK * CHUNK_PER_THREAD;    // elements of one (n, c) plane per block

// the thread's elements of the chunk at `base`; past the plane's end: 0 and ok = false
template <bool VEC>
__device__ __forceinline__ void load8(const float* __restrict__ p, int base, int HW, float (&v)[CHUNK_PER_THREAD], bool (&ok)[CHUNK_PER_THREAD]) {
  if (VEC) {
#pragma unroll
    for (int k = 0; k < CHUNK_PER_THREAD / 4; ++k) {
      const int e = base + (k * CHUNK_BLOCK + threadIdx.x) * 4;
      const bool in = e < HW;
      float4 q = in ? *reinterpret_cast<const float4*>(p + e) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
      ok[4 * k] = ok[4 * k + 1] = ok[4 * k + 2] = ok[4 * k + 3] = in;
    }
  } else {
#pragma unroll
    for (int k = 0; k < CHUNK_PER_THREAD; ++k) {
      const int e = base + k * CHUNK_BLOCK + threadIdx.x;
      ok[k] = e < HW;
      v[k] = ok[k] ? p[e] : 0.0f;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void store8(float* __restrict__ p, int base, int HW, const float (&v)[CHUNK_PER_THREAD]) {
  if (VEC) {
#pragma unroll
    for (int k = 0; k < CHUNK_PER_THREAD / 4; ++k) {
      const int e = base + (k * CHUNK_BLOCK + threadIdx.x) * 4;
      if (e < HW) *reinterpret_cast<float4*>(p + e) = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < CHUNK_PER_THREAD; ++k) {
      const int e = base + k * CHUNK_BLOCK + threadIdx.x;
      if (e < HW) p[e] = v[k];
    }
  }
}

}  // namespace dfe
