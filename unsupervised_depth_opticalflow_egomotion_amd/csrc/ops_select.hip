// dfe_topk_select: the pixel indices of the k largest scores of every plane, in ascending pixel order (the top-ratio
// selection of sample_match, model_geometry.py:427-437, without topk's sort and without a host read).
//
// One workgroup per plane.  (1) Radix select over order-preserving 32-bit keys -- torch.topk's order: NaN above +inf,
// -0 equal to +0 -- four 8-bit digits from the top, one LDS histogram (integer atomics) each, finds the key T of the k-th
// largest score and how many scores equal to T belong to the set.  (2) One ordered pass: a score is kept when its key is
// above T, or equals T while fewer than that many equal scores precede it (ties go to the lower pixel index); a block-wide
// prefix count of both flags gives its output position.  No float atomics, nothing depends on the order the integer atomics
// retire in: same bits run after run.
#include "dfe_internal.h"

namespace dfe {
namespace {

constexpr int SEL_THREADS = 1024;
constexpr int SEL_WAVES = SEL_THREADS / 64;
constexpr int SEL_ITEMS = 4;                       // consecutive scores per thread in the ordered pass
constexpr int SEL_RECORD_WORDS = 4;                // per plane: threshold key, scores above it, ties taken, 0

__device__ __forceinline__ unsigned score_key(float v) {
  if (v != v) return 0xffffffffu;
  if (v == 0.0f) return 0x80000000u;               // -0 and +0 rank equal
  const unsigned bits = static_cast<unsigned>(__float_as_int(v));
  return (bits >> 31) ? ~bits : (bits | 0x80000000u);
}

__global__ void __launch_bounds__(SEL_THREADS) k_topk_select(const float* __restrict__ scores, int* __restrict__ idx,
                                                            unsigned* __restrict__ record, int n, int k) {
  __shared__ int hist[256];
  __shared__ unsigned picked[2];
  __shared__ unsigned wave_tot[2][SEL_WAVES];
  const float* p = scores + static_cast<long>(blockIdx.x) * n;
  int* out = idx + static_cast<long>(blockIdx.x) * k;
  const int tid = threadIdx.x;

  unsigned prefix = 0;
  int need = k;                                    // the need-th largest among the scores whose key starts with prefix
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned mask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
    // scores of one plane share their leading digits: a thread counts a run of equal digits privately and adds it once
    // (one bin would otherwise take every lane's atomic in turn)
    int run_bin = -1, run = 0;
#pragma unroll 4
    for (int i = tid; i < n; i += SEL_THREADS) {
      const unsigned key = score_key(p[i]);
      if ((key & mask) == prefix) {
        const int bin = static_cast<int>((key >> shift) & 255u);
        if (bin == run_bin) ++run;
        else {
          if (run > 0) atomicAdd(&hist[run_bin], run);
          run_bin = bin;
          run = 1;
        }
      }
    }
    if (run > 0) atomicAdd(&hist[run_bin], run);
    __syncthreads();
    if (tid < 256) {
      int above = 0;
      for (int i = 255; i > tid; --i) above += hist[i];
      if (above < need && above + hist[tid] >= need) {           // exactly one bin
        picked[0] = prefix | (static_cast<unsigned>(tid) << shift);
        picked[1] = static_cast<unsigned>(need - above);
      }
    }
    __syncthreads();
    prefix = picked[0];
    need = static_cast<int>(picked[1]);
    __syncthreads();
  }
  const unsigned T = prefix;
  const int ties = need;                           // scores equal to T that belong to the set: the first `ties` in pixel order
  if (tid == 0) {
    unsigned* r = record + static_cast<long>(blockIdx.x) * SEL_RECORD_WORDS;
    r[0] = T; r[1] = static_cast<unsigned>(k - ties); r[2] = static_cast<unsigned>(ties); r[3] = 0u;
  }

  // ordered compaction; counts packed as (above | equal << 16): a chunk holds 4096 scores, so neither half overflows
  const int lane = tid & 63, wave = tid >> 6;
  int base_gt = 0, base_eq = 0;
  int round = 0;
  for (long start = 0; start < n; start += SEL_THREADS * SEL_ITEMS, ++round) {
    const long first = start + static_cast<long>(tid) * SEL_ITEMS;
    unsigned flag[SEL_ITEMS], mine = 0;
#pragma unroll
    for (int e = 0; e < SEL_ITEMS; ++e) {
      flag[e] = 0;
      if (first + e < n) {
        const unsigned key = score_key(p[first + e]);
        flag[e] = key > T ? 1u : (key == T ? 0x10000u : 0u);
      }
      mine += flag[e];
    }
    unsigned incl = mine;                          // inclusive scan over the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = static_cast<unsigned>(__shfl_up(static_cast<int>(incl), o));
      if (lane >= o) incl += up;
    }
    unsigned* tot = wave_tot[round & 1];
    if (lane == 63) tot[wave] = incl;
    __syncthreads();
    unsigned before = incl - mine, all = 0;
    for (int wv = 0; wv < SEL_WAVES; ++wv) {
      const unsigned t = tot[wv];
      if (wv < wave) before += t;
      all += t;
    }
    int gt = base_gt + static_cast<int>(before & 0xffffu), eq = base_eq + static_cast<int>(before >> 16);
#pragma unroll
    for (int e = 0; e < SEL_ITEMS; ++e) {
      if (flag[e] == 1u) {
        const int pos = gt + min(eq, ties);
        if (pos < k) out[pos] = static_cast<int>(first + e);
        ++gt;
      } else if (flag[e] != 0u) {
        if (eq < ties) {
          const int pos = gt + eq;
          if (pos < k) out[pos] = static_cast<int>(first + e);
        }
        ++eq;
      }
    }
    base_gt += static_cast<int>(all & 0xffffu);
    base_eq += static_cast<int>(all >> 16);
  }
}

}  // namespace
}  // namespace dfe

using namespace dfe;

extern "C" long dfe_topk_ws_bytes(int planes, int n, int k) {
  if (planes <= 0 || n <= 0 || k <= 0 || k > n) return 0;
  return 4L * SEL_RECORD_WORDS * planes;
}

extern "C" int dfe_topk_select(const float* scores, int* idx, void* ws, int planes, int n, int k, void* stream) {
  if (!scores || !idx || !ws) return DFE_ERR_NULL;
  if (planes <= 0 || n <= 0 || k <= 0 || k > n) return DFE_ERR_DIMS;
  if (reinterpret_cast<uintptr_t>(ws) & 3) return DFE_ERR_DIMS;
  k_topk_select<<<static_cast<unsigned>(planes), SEL_THREADS, 0, static_cast<hipStream_t>(stream)>>>(
      scores, idx, static_cast<unsigned*>(ws), n, k);
  return launch_status();
}
