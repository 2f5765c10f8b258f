// Operand staging of the fp32 matrix-core convolutions that read NCHW directly: the vector types and the packed quad (every
// matrix-core file), the 16 x 16 x 4 tile loop (ops_sconv.hip, ops_conv1x1s2.hip), the row-window slot loader, the LDS store
// forms and the filter-slab stage (ops_sconv.hip).  One copy each: a change of the staging (a deeper prefetch, direct-to-LDS
// loads) is made here.  k_wino_wgrad2 keeps a loader of its own (ops_wino_wgrad.hip: the workspace as its safe address, the edge
// patches per channel): on load_slots it measured 10 % slower on every layer (profiles/mfma_stage_refactor.txt).
#pragma once
#include <hip/hip_runtime.h>

namespace dfe {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
struct __attribute__((packed, aligned(4))) QuadU { float a, b, c, d; };     // dword-aligned 16 bytes

// The row-window slot loader.  A slot is 16 bytes of a row: the four columns col ... col + 3 at base + off0; a thread loads the
// slot of N channels `step` apart (plane stride `plane`), the first of them channel ch0 of its block.  Straight-line: a 16-byte
// load from the slot's address -- or from `base` itself, the loads' safe address (the caller's planner refuses tensors of fewer
// than four floats; the value is dropped), when the slot is outside the image (!full) or its channel is not below nch, the fewer
// of the block's and the layer's channels -- and a select; the slots the image's edge cuts (`cut`: two per row) are then patched
// word by word under one branch that whole waves skip.
template <int N>
__device__ __forceinline__ void load_slots(f32x4 (&v)[N], const float* base, int off0, int plane, int ch0, int step, int nch, int col,
                                           int width, bool full, bool cut) {
  QuadU u[N];
#pragma unroll
  for (int jj = 0; jj < N; ++jj) u[jj] = *reinterpret_cast<const QuadU*>(base + (full && ch0 + jj * step < nch ? off0 + jj * step * plane : 0));
  // sched_barrier: left alone, the scheduler puts each select (and the wait for its load) right behind the load: one load in flight
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int jj = 0; jj < N; ++jj) {
    const bool ok = full && ch0 + jj * step < nch;
    v[jj] = f32x4{ok ? u[jj].a : 0.0f, ok ? u[jj].b : 0.0f, ok ? u[jj].c : 0.0f, ok ? u[jj].d : 0.0f};
  }
  if (cut) {
#pragma unroll
    for (int jj = 0; jj < N; ++jj)
      if (ch0 + jj * step < nch) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (col + e >= 0 && col + e < width) v[jj][e] = base[off0 + jj * step * plane + e];
      }
  }
}

// A slot into LDS.  Stride 2: the even columns at d, the odd ones qw words on, so that the four pixels of a step are four
// consecutive words.  Contiguous: two 8-byte stores where the channel stride is even but no multiple of four (a multiple of
// four takes one 16-byte store of the f32x4).
__device__ __forceinline__ void store_slot_split(float* d, int qw, f32x4 v) {
  *reinterpret_cast<f32x2*>(d) = f32x2{v[0], v[2]};
  *reinterpret_cast<f32x2*>(d + qw) = f32x2{v[1], v[3]};
}
__device__ __forceinline__ void store_slot_pairs(float* d, f32x4 v) {
  *reinterpret_cast<f32x2*>(d) = f32x2{v[0], v[1]};
  *reinterpret_cast<f32x2*>(d + 2) = f32x2{v[2], v[3]};
}

// The filter slab of a channel chunk: rows of WQ 16-byte words (row stride srs floats in memory, lrs in LDS), wl4 words in all,
// word tid + 256 jj to thread tid: 16-byte copies, no index arithmetic in the multiply loop.
template <int WQ, int NWL>
__device__ __forceinline__ void load_slab(f32x4 (&w)[NWL], const float* src, int srs, int wl4, int tid) {
#pragma unroll
  for (int jj = 0; jj < NWL; ++jj) {
    const int e = tid + 256 * jj, row = e / WQ, q = e - row * WQ;
    w[jj] = e < wl4 ? *reinterpret_cast<const f32x4*>(src + static_cast<long>(row) * srs + 4 * q) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
}
template <int WQ, int NWL>
__device__ __forceinline__ void store_slab(float* dst, int lrs, const f32x4 (&w)[NWL], int wl4, int tid) {
#pragma unroll
  for (int jj = 0; jj < NWL; ++jj) {
    const int e = tid + 256 * jj, row = e / WQ, q = e - row * WQ;
    if (e < wl4) *reinterpret_cast<f32x4*>(dst + row * lrs + 4 * q) = w[jj];
  }
}

// One reduction step (4 deep) of a wave's MT x NT tiles of 16 x 16, in (mt, j) order
template <int MT, int NT>
__device__ __forceinline__ void mfma_tile(f32x4 (&acc)[MT][NT], const float (&a)[MT], const float (&b)[NT]) {
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[j], acc[mt][j], 0, 0, 0);
}

}  // namespace dfe
