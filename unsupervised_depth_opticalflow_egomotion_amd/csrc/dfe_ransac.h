// What the RANSAC terms (ops_eight_point.hip, ops_pnp.hip) share, stated once: the clamped draw of a match (also the
// triangulation term's, ops_triangulate.hip), the workspace layout, the block reductions, the scoring kernel's body, the
// consensus kernel's skeleton, the entry points' common refusals and their launch sequence.  A term supplies a model:
//   struct Model {
//     static constexpr int PT, HP, MIN;     // doubles per match and per hypothesis; the smallest set a fit accepts
//     struct Ctx;                           // what the test needs per plane beside the hypothesis (a camera, or nothing)
//     static __device__ bool inlier(const Ctx&, const double* hyp, const double* match, double thr2);
//   };
// and each named kernel is a thin wrapper around a body here.  No float atomics: every float sum has an order fixed by thread
// index.
#pragma once
#include "dfe_internal.h"

namespace dfe {
namespace ransac {

constexpr int THREADS = 256;           // the block of the per-match kernels, of the consensus kernel and of the reductions
constexpr int MATCH_TILE = 256;        // matches per block of the scoring kernel, one per thread
constexpr int HYP_TILE = 64;           // hypotheses staged in LDS at a time
constexpr int MAX_NUM = 16384;         // the draw's limit of the triangulation term, kept here
constexpr int MAX_HYP = 4096;

// ---------------------------------------------------------------------------------------------- the draw
struct Match {
  int pix, x, y;      // the pixel and its column and row
  float u, v;         // the flow there
};

// Match j of a plane: the pixel idx[plane][pick[j]] of sample b, pick clamped to [0, k) and the pixel to [0, HW); flow: the
// plane's direction, [B, 2, H, W].
__device__ __forceinline__ Match load_match(const float* __restrict__ flow, const int* __restrict__ idx,
                                            const long long* __restrict__ pick, int plane, int b, int j, int k, int H, int W) {
  long long p = pick[j];
  p = p < 0 ? 0 : (p > k - 1 ? k - 1 : p);
  const int HW = H * W;
  int pix = idx[static_cast<long>(plane) * k + p];
  pix = pix < 0 ? 0 : (pix > HW - 1 ? HW - 1 : pix);
  const float* fl = flow + static_cast<long>(b) * 2 * HW;
  return Match{pix, pix - (pix / W) * W, pix / W, fl[pix], fl[HW + pix]};
}

// ---------------------------------------------------------------------------------------------- workspace
__host__ __device__ inline long round16(long v) { return (v + 15) & ~15L; }

// Sections, each starting on 16 bytes: matches [2B, num, pt] doubles; hypotheses [2B, hyp, hp] doubles; counts int [2B, hyp];
// the 0/1 weights of the first and of the second fit, int [2B, num] each.
struct WsOffsets { long hyps, counts, w1, w2, bytes; };
inline WsOffsets ws_offsets(int pt, int hp, int B, int num, int hyp) {
  WsOffsets o;
  o.hyps = 8L * pt * 2 * B * num;
  o.counts = o.hyps + round16(8L * hp * 2 * B * hyp);
  o.w1 = o.counts + round16(4L * 2 * B * hyp);
  o.w2 = o.w1 + round16(4L * 2 * B * num);
  o.bytes = o.w2 + round16(4L * 2 * B * num);
  return o;
}
struct Ws {
  double* m;
  double* hyps;
  int* counts;
  int* w1;
  int* w2;
};
inline Ws ws_sections(void* ws, const WsOffsets& o) {
  char* p = static_cast<char*>(ws);
  return Ws{reinterpret_cast<double*>(p), reinterpret_cast<double*>(p + o.hyps), reinterpret_cast<int*>(p + o.counts),
            reinterpret_cast<int*>(p + o.w1), reinterpret_cast<int*>(p + o.w2)};
}

// ---------------------------------------------------------------------------------------------- block reductions
// N sums side by side, each in a fixed order: every thread's strided partial, then a tree over the threads.  v <- the sums, in
// every thread.  red: N * THREADS doubles of LDS.
template <int N>
__device__ inline void block_sum(double* v, double* red) {
  for (int i = 0; i < N; ++i) red[i * THREADS + threadIdx.x] = v[i];
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s)
      for (int i = 0; i < N; ++i) red[i * THREADS + threadIdx.x] += red[i * THREADS + threadIdx.x + s];
    __syncthreads();
  }
  for (int i = 0; i < N; ++i) v[i] = red[i * THREADS];
  __syncthreads();
}

__device__ inline int block_sum_int(int v, int* ired) {
  ired[threadIdx.x] = v;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) ired[threadIdx.x] += ired[threadIdx.x + s];
    __syncthreads();
  }
  const int r = ired[0];
  __syncthreads();
  return r;
}

// the index of the largest of c[0 .. n), ties to the lowest index; *largest receives the value.  ired, ibest: THREADS ints each
__device__ inline int block_argmax(const int* __restrict__ c, int n, int* ired, int* ibest, int* largest) {
  int bc = -1, bh = 0;
  for (int h = threadIdx.x; h < n; h += THREADS)
    if (c[h] > bc) { bc = c[h]; bh = h; }
  ired[threadIdx.x] = bc;
  ibest[threadIdx.x] = bh;
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) {
      const int oc = ired[threadIdx.x + s], oh = ibest[threadIdx.x + s];
      if (oc > ired[threadIdx.x] || (oc == ired[threadIdx.x] && oh < ibest[threadIdx.x])) { ired[threadIdx.x] = oc; ibest[threadIdx.x] = oh; }
    }
    __syncthreads();
  }
  const int best = ibest[0];
  *largest = ired[0];
  __syncthreads();
  return best;
}

// ---------------------------------------------------------------------------------------------- scoring
// A tile of MATCH_TILE matches per block (one per thread), the plane's hypotheses in tiles of HYP_TILE through LDS: inlier
// counts by wave ballots, integer atomics.  Grid (tiles of matches, planes).
template <class M>
__device__ __forceinline__ void score_body(const typename M::Ctx& ctx, const double* __restrict__ m, const double* __restrict__ hyps,
                                           int* __restrict__ counts, int num, int hyp, double thr2) {
  __shared__ double sH[HYP_TILE * M::HP];
  __shared__ int sC[HYP_TILE];
  const int j = blockIdx.x * MATCH_TILE + threadIdx.x;
  const int plane = blockIdx.y;
  const bool live = j < num;
  double pt[M::PT];
  for (int i = 0; i < M::PT; ++i) pt[i] = 0.0;
  if (live)
    for (int i = 0; i < M::PT; ++i) pt[i] = m[(static_cast<long>(plane) * num + j) * M::PT + i];
  for (int h0 = 0; h0 < hyp; h0 += HYP_TILE) {
    const int nh = hyp - h0 < HYP_TILE ? hyp - h0 : HYP_TILE;
    for (int i = threadIdx.x; i < nh * M::HP; i += MATCH_TILE) sH[i] = hyps[(static_cast<long>(plane) * hyp + h0) * M::HP + i];
    if (threadIdx.x < HYP_TILE) sC[threadIdx.x] = 0;
    __syncthreads();
    for (int hh = 0; hh < nh; ++hh) {
      const bool in = live && M::inlier(ctx, sH + hh * M::HP, pt, thr2);
      const unsigned long long bal = __ballot(in);
      if ((threadIdx.x & 63) == 0 && bal != 0ull) atomicAdd(&sC[hh], __popcll(bal));
    }
    __syncthreads();
    if (static_cast<int>(threadIdx.x) < nh && sC[threadIdx.x] != 0)
      atomicAdd(&counts[static_cast<long>(plane) * hyp + h0 + threadIdx.x], sC[threadIdx.x]);
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------- consensus
// w[j] <- 1 where match j agrees with the hypothesis cur (LDS, read into registers first), 0 elsewhere; returns their number
template <class M>
__device__ __forceinline__ int inlier_set(const typename M::Ctx& ctx, const double* cur, const double* __restrict__ mp,
                                          int* __restrict__ w, int num, double thr2, int* ired) {
  double h[M::HP], pt[M::PT];
  for (int i = 0; i < M::HP; ++i) h[i] = cur[i];
  int c = 0;
  for (int j = threadIdx.x; j < num; j += THREADS) {
    for (int i = 0; i < M::PT; ++i) pt[i] = mp[static_cast<long>(j) * M::PT + i];
    const int in = M::inlier(ctx, h, pt, thr2) ? 1 : 0;
    w[j] = in;
    c += in;
  }
  return block_sum_int(c, ired);
}

// One block per plane: the hypothesis with the most inliers (ties: the lowest index) -> cur, its inlier set (fewer than MIN:
// all matches), fit(weights, 0), the inlier set of that fit (fewer than MIN: the previous set), fit(weights, 1), finish(), info.
// cur: M::HP doubles of LDS that fit reads the model from and leaves its result in, behind a barrier; fit and finish are called
// by every thread.  Both fall-backs are uniform over the block (their counts are block sums), so every barrier is reached by
// every thread.
template <class M, class Fit, class Finish>
__device__ __forceinline__ void consensus_body(const typename M::Ctx& ctx, const double* __restrict__ m, const double* __restrict__ hyps,
                                               const int* __restrict__ counts, int* __restrict__ w1, int* __restrict__ w2,
                                               int* __restrict__ info, int num, int hyp, double thr2, double* cur, Fit fit,
                                               Finish finish) {
  __shared__ int ired[THREADS], ibest[THREADS];
  const int plane = blockIdx.x;
  const double* mp = m + static_cast<long>(plane) * num * M::PT;
  int* w1p = w1 + static_cast<long>(plane) * num;
  int* w2p = w2 + static_cast<long>(plane) * num;
  int best_count;
  const int best = block_argmax(counts + static_cast<long>(plane) * hyp, hyp, ired, ibest, &best_count);
  if (threadIdx.x < M::HP) cur[threadIdx.x] = hyps[(static_cast<long>(plane) * hyp + best) * M::HP + threadIdx.x];
  __syncthreads();
  int n1 = inlier_set<M>(ctx, cur, mp, w1p, num, thr2, ired);
  if (n1 < M::MIN) {                      // no consensus: all matches
    for (int j = threadIdx.x; j < num; j += THREADS) w1p[j] = 1;
    n1 = num;
  }
  fit(w1p, 0);                            // every thread reads back only the weights it wrote
  int n2 = inlier_set<M>(ctx, cur, mp, w2p, num, thr2, ired);
  if (n2 < M::MIN) {                      // keep the previous set
    for (int j = threadIdx.x; j < num; j += THREADS) w2p[j] = w1p[j];
    n2 = n1;
  }
  fit(w2p, 1);
  finish();
  if (threadIdx.x == 0) {
    info[plane * 4] = best; info[plane * 4 + 1] = best_count; info[plane * 4 + 2] = n1; info[plane * 4 + 3] = n2;
  }
}

// ---------------------------------------------------------------------------------------------- entry points
// the refusals both entry points share, in their order; have_all: no pointer argument is NULL; out64: the double result
inline int check_args(bool have_all, int B, int H, int W, int k, int num, int hyp, int min_num, const void* ws, const void* out64) {
  if (!have_all) return DFE_ERR_NULL;
  if (B <= 0 || B > 16384 || H < 1 || W < 1 || k <= 0 || num < min_num || hyp < 1) return DFE_ERR_DIMS;
  if (static_cast<long>(H) * W >= (1L << 28) || k > H * W) return DFE_ERR_DIMS;
  if (num > MAX_NUM || hyp > MAX_HYP) return DFE_ERR_UNSUPPORTED;
  if (!aligned16(ws) || !aligned8(out64)) return DFE_ERR_DIMS;
  return DFE_OK;
}

// A memset of the counts (everything else in the workspace is written before it is read), then the four kernels; each argument
// launches its kernel on the grid it is given, the hypothesis kernel with hyp_threads threads per block.
template <class Matches, class Hyps, class Score, class Consensus>
inline int launch_all(int* counts, int B, int num, int hyp, int hyp_threads, hipStream_t st, Matches matches, Hyps hyps, Score score,
                      Consensus consensus) {
  if (hipMemsetAsync(counts, 0, static_cast<size_t>(4L * 2 * B * hyp), st) != hipSuccess) return DFE_ERR_LAUNCH;
  matches(dim3(static_cast<unsigned>((num + THREADS - 1) / THREADS), 2 * B));
  DFE_LAUNCH_CHECK();
  hyps(dim3(static_cast<unsigned>((hyp + hyp_threads - 1) / hyp_threads), 2 * B));
  DFE_LAUNCH_CHECK();
  score(dim3(static_cast<unsigned>((num + MATCH_TILE - 1) / MATCH_TILE), 2 * B));
  DFE_LAUNCH_CHECK();
  consensus(dim3(2 * B));
  return launch_status();
}

}  // namespace ransac
}  // namespace dfe
