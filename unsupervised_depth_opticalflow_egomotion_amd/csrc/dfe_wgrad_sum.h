// The split of a weight gradient's reduction over blocks and the fixed-order sum of the splits' partials (ops_wino_wgrad.hip,
// ops_sconv.hip, ops_conv1x1s2.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>

namespace dfe {

// gw[i] = sum over the splits of part[s][i]: SG groups of consecutive splits are summed side by side (each in split order) and
// the SG group sums are added in group order -- a fixed association, whatever the timing.  32 groups when there are many splits
// (64 x 64 filters: up to 768 splits of 36 k outputs -- 8 groups left every thread a chain of ~100 dependent loads).
template <int SG>
__global__ void __launch_bounds__(32 * SG) k_wgrad_sum(const float* __restrict__ part, float* __restrict__ gw, int S, long n) {
  __shared__ float sm[SG][32];
  const int o = threadIdx.x & 31, g = threadIdx.x >> 5;
  const long idx = static_cast<long>(blockIdx.x) * 32 + o;
  const int per = (S + SG - 1) / SG, s0 = g * per, s1 = min(S, s0 + per);
  float s = 0.0f;
  if (idx < n)
    for (int k = s0; k < s1; ++k) s += part[k * n + idx];
  sm[g][o] = s;
  __syncthreads();
  if (g == 0 && idx < n) {
    float t = sm[0][o];
#pragma unroll
    for (int j = 1; j < SG; ++j) t += sm[j][o];
    gw[idx] = t;
  }
}

inline void launch_wgrad_sum(const float* ws, float* gw, int nsplit, long n, hipStream_t st) {
  const unsigned blocks = static_cast<unsigned>((n + 31) / 32);
  if (nsplit > 64) k_wgrad_sum<32><<<blocks, 1024, 0, st>>>(ws, gw, nsplit, n);
  else k_wgrad_sum<8><<<blocks, 256, 0, st>>>(ws, gw, nsplit, n);
}

// The split of a reduction of nchunks chunks over blocks: one resident round of `target` blocks, ntb of them per split.  Returns
// the number of splits, *cps = chunks per split.
inline int split_round(int target, long ntb, int nchunks, int* cps) {
  long sp = (target + ntb / 2) / ntb;
  sp = std::max(1L, std::min<long>(sp, nchunks));
  *cps = static_cast<int>((nchunks + sp - 1) / sp);
  return (nchunks + *cps - 1) / *cps;
}

}  // namespace dfe
