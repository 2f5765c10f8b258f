// PWC cost volume (corr_naive, core/networks/structures/pwc_tf.py:97-106; d = 4, 81 displacements) and its two
// gradients, LDS-staged (round 4; replaces the per-displacement-row register kernels of rounds 1-3, which fetched f1
// nine times and every f2 window through L1: 3.4-4.9x the algorithmic bytes over the fabric, 0.03-0.20 of the HBM
// roofline -- VERDICT r03 weak #2).
//
//   out[b, i*9+j, y, x] = 1/C sum_c f1[b,c,y,x] * f2[b,c,y+i-4,x+j-4]          (zero outside the image)
//   g1[b,c,p] = 1/C sum_k g[b,k,p]       * f2[b,c,p+d_k]                        d_k = (i-4, j-4), k = i*9+j
//   g2[b,c,p] = 1/C sum_k g[b,k,p-d_k]   * f1[b,c,p-d_k]
//
// Forward: a block owns a TH x 4*TXQ tile of output pixels and ALL 81 displacements.  Per chunk of CC channels it
// stages the f1 tile and the f2 tile with its +-4 halo in LDS once (16-byte coalesced loads, zero-filled outside the
// image, double-buffered: the next chunk's loads are in flight while this one is multiplied), then every thread
// (displacement row dy, tile row, quad of 4 pixels) reads one f1 quad + its 12-wide f2 window (4 ds_read_b128) per
// channel and issues 36 FMAs.  Each input byte crosses the fabric ~once per tile (halo re-reads stay inside the XCD's
// L2: tiles are dealt in XCD order), 9 FMAs per LDS read keep the LDS array ~25 % busy.  No MFMA: a banded 16x16 Gram tile
// uses 28 % of the matrix pipe (9 of 32 diagonals) while a wave-wide fp32 FMA issues every ~2.5 cycles, and exact fp32
// sums in channel order are kept.  Measured (level 2, C = 32, B = 8: 61.8 MB in 21.0 us = 0.37 of the HBM peak, PMC /
// algorithmic 1.00; tools/corr_ablate.sh): the FMAs are free (20.5 us without them); the launch is one round of 512
// blocks in lockstep -- read burst, LDS pipeline, 34.5 MB write burst back to back.
// Coarse levels (16x52 ... 4x13: fewer pixels than the chip has lanes): the channel sum is split over KS threads per
// output and the partials meet in LDS in fixed order (deterministic).
//
// Backward: the same kernel for both gradients -- writing k' = 80 - k, g2[c,p] = 1/C sum_k' g[80-k', p+d_k'] f1[c, p+d_k'],
// i.e. g1's formula with the planes reversed and the gradient sampled at the window position instead of at p.  A block
// stages the halo tile of the OTHER feature for a range of channels once; a thread owns (8 channels, tile row, quad):
// per displacement row it loads the 9 gradient quads from global memory (its own pixel, or the shifted one: a
// dword-aligned 16-byte load) and re-uses them across its 8 channels: 3 LDS reads + 36 FMAs per channel and row.
// Displacement rows are split over IS threads per output where the level is small; partials meet in LDS in fixed order.
#include "dfe_device.h"
#include "dfe_internal.h"
#include "dfe_mfma_stage.h"
#include "loss_stack_exact.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>

// DFE_CORR_ABL (debug builds of tools/corr_ablate.sh only): 1 = no output stores, 2 = no FMAs, 4 = no staging loads
#ifndef DFE_CORR_ABL
#define DFE_CORR_ABL 0
#endif

namespace dfe {

namespace {

constexpr int CR_D = 4, CR_K = 2 * CR_D + 1, CR_NK = CR_K * CR_K;
constexpr int CF_PF1 = 2;          // staged f1 quads per thread and chunk (forward)
constexpr int CB_CK = 8;           // channels per thread (backward)
constexpr int CB_STAGE = 12;       // tile quads per thread and staging batch (backward)
constexpr int CORR_MAX_LDS = 160 * 1024;

struct MagicDiv { unsigned m, d; };   // q = e / d for e * d < 2^32
__device__ __forceinline__ unsigned mdiv(unsigned e, MagicDiv k) { return k.d == 1 ? e : __umulhi(e, k.m); }
inline MagicDiv make_magic(unsigned d) { return MagicDiv{d <= 1 ? 0u : static_cast<unsigned>(((1ull << 32) + d - 1) / d), d}; }

// A block stages a [channels][rows][quads] image with its threads striding through it: thread t takes elements t,
// t + NT, ...  One division decodes the first element, every further one is (channel, row, quad) += step with carries.
struct StageStep { int a, b, c; };    // NT = a * (rows * quads) + b * quads + c
inline StageStep make_step(int NT, int rows, int quads) { return StageStep{NT / (rows * quads), (NT % (rows * quads)) / quads, NT % quads}; }
struct StagePos { int cl, r, q; };
__device__ __forceinline__ StagePos stage_first(int tid, MagicDiv mP, MagicDiv mQ, int P, int Q) {
  StagePos s;
  s.cl = mdiv(tid, mP);
  const int rem = tid - s.cl * P;
  s.r = mdiv(rem, mQ);
  s.q = rem - s.r * Q;
  return s;
}
__device__ __forceinline__ void stage_next(StagePos& s, StageStep st, int rows, int quads) {
  s.q += st.c; if (s.q >= quads) { s.q -= quads; ++s.r; }
  s.r += st.b; if (s.r >= rows) { s.r -= rows; ++s.cl; }
  s.cl += st.a;
}

struct CorrFwdCfg {
  int TH, TXQ, KS, CC;             // tile rows, tile width in quads, channel split, channels per chunk
  int DYG, ndyg;                   // displacement rows per block (9 = all of them), groups of them (ceil(9 / DYG))
  int ntx, nty, NI;                // tiles across / down, work items per channel slot (TH * TXQ * DYG)
  int R2, Q2, P2, P1;              // f2 tile rows / quads per row, quads per channel of the f2 / f1 tile
  int n2, n1;                      // CC * P2, CC * P1
  MagicDiv mP2, mQ2, mP1, mTXQ;
  StageStep s2, s1;
};

struct CorrBwdCfg {
  int TH, TXQ, NCG, IS;            // tile rows, quads, channel groups (of CB_CK) per block, displacement-row split
  int ntx, nty, ncr, NI;           // tiles, channel ranges per sample, work items per row slot (NCG * TH * TXQ)
  int R2, Q2, P2;
  int tile_quads;                  // NCG * CB_CK * P2
  MagicDiv mP2, mQ2;
  StageStep st;
};

// one gradient of the backward launch: MODE 0 (g1: other = f2, addend optional) or MODE 1 (g2: other = f1)
struct CorrBwdSide { const float* other; float* gin; const float* addend; long abs_; unsigned* amax; };   // amax: word that receives max |gin| as a bit pattern (dfe_scatter.h header), or NULL

__device__ __forceinline__ float4 load_quad_checked(const float* __restrict__ p, int gx, int W) {
  // p points at column gx of a valid row; elements outside [0, W) read as zero
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (gx >= 0 && gx + 3 < W) { const QuadU q = *reinterpret_cast<const QuadU*>(p); v = make_float4(q.a, q.b, q.c, q.d); }
  else {
    if (gx >= 0 && gx < W) v.x = p[0];
    if (gx + 1 >= 0 && gx + 1 < W) v.y = p[1];
    if (gx + 2 >= 0 && gx + 2 < W) v.z = p[2];
    if (gx + 3 >= 0 && gx + 3 < W) v.w = p[3];
  }
  return v;
}

// The same for a quad that starts inside the row (0 <= gx < W) and may be cut by the right border only -- every staged
// quad is of that kind (tiles start at multiples of 4): four dword loads from clamped addresses, no branch.  (A
// dword-aligned 16-byte load shifted back into the row was measured and is slower: unaligned wide loads are split.)
__device__ __forceinline__ float4 load_quad_right(const float* __restrict__ p, int gx, int W) {
  const int n = W - gx;                                // >= 1 elements inside the row
  float4 v;
  v.x = p[0];
  const float y = p[n > 1 ? 1 : 0], z = p[n > 2 ? 2 : 0], w = p[n > 3 ? 3 : 0];
  v.y = n > 1 ? y : 0.0f; v.z = n > 2 ? z : 0.0f; v.w = n > 3 ? w : 0.0f;
  return v;
}

// max over the wave of a non-negative bit pattern, then one atomicMax per wave (none when the word already holds as much):
// max is associative and commutative, so the word does not depend on the order (dfe_scatter.h; a NaN's pattern wins)
__device__ __forceinline__ void wave_amax_to(unsigned* word, unsigned m) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, static_cast<unsigned>(__shfl_xor(static_cast<int>(m), o)));
  if ((threadIdx.x & 63) == 0 && m > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, m);
}
__device__ __forceinline__ unsigned abs_bits(float v) { return static_cast<unsigned>(__float_as_int(v)) & 0x7fffffffu; }

// ------------------------------------------------------------------------------------------------ forward
// PF2: staged f2 quads per thread and chunk (4: the fine levels, <= 128 VGPRs = two 512-thread blocks per CU;
// 10: the coarse levels, where few large chunks beat many small ones -- every chunk is a global-memory round trip
// that the little arithmetic of a small level cannot hide).
template <bool VEC, int PF2, int WPE>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(WPE, WPE)))
k_corr_fwd_lds(const float* __restrict__ f1, const float* __restrict__ f2, float* __restrict__ out, long obs, float* __restrict__ tail,
               const float* __restrict__ flow, int C, int H, int W, float fC, float rC, CorrFwdCfg g) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, NT = blockDim.x;
  const unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int dyg = bid % g.ndyg, tile = bid / g.ndyg;
  const int tx = tile % g.ntx, ty = (tile / g.ntx) % g.nty, b = tile / (g.ntx * g.nty);
  const int tx0 = tx * 4 * g.TXQ, ty0 = ty * g.TH, dy0 = dyg * g.DYG;
  const long HW = static_cast<long>(H) * W;
  const float* f1b = f1 + static_cast<long>(b) * C * HW;
  const float* f2b = f2 + static_cast<long>(b) * C * HW;

  // ---- what this thread stages per chunk: quads tid, tid + NT, ... of the f2 image [CC][R2][Q2] and of the f1 image [CC][TH][TXQ]
  int off2[PF2], cl2[PF2], gx2[PF2], off1[CF_PF1], cl1[CF_PF1], gx1[CF_PF1];    // offset from channel 0 of the chunk (-1: zero), channel in the chunk, column (only read where W % 4 != 0)
  {
    StagePos s = stage_first(tid, g.mP2, g.mQ2, g.P2, g.Q2);
#pragma unroll
    for (int q = 0; q < PF2; ++q) {
      const int gy = ty0 - CR_D + dy0 + s.r, gx = tx0 - CR_D + 4 * s.q;
      const bool ok = (tid + q * NT < g.n2) && gy >= 0 && gy < H && gx >= 0 && gx < W;
      off2[q] = ok ? static_cast<int>(s.cl * HW + static_cast<long>(gy) * W + gx) : -1;
      cl2[q] = s.cl; gx2[q] = gx;
      stage_next(s, g.s2, g.R2, g.Q2);
    }
    s = stage_first(tid, g.mP1, g.mTXQ, g.P1, g.TXQ);
#pragma unroll
    for (int q = 0; q < CF_PF1; ++q) {
      const int gy = ty0 + s.r, gx = tx0 + 4 * s.q;
      const bool ok = (tid + q * NT < g.n1) && gy < H && gx < W;
      off1[q] = ok ? static_cast<int>(s.cl * HW + static_cast<long>(gy) * W + gx) : -1;
      cl1[q] = s.cl; gx1[q] = gx;
      stage_next(s, g.s1, g.TH, g.TXQ);
    }
  }
  float4 pf2[PF2], pf1[CF_PF1];
  // unconditional loads from clamped addresses, zero selected afterwards: no branch around a load, all of them in flight
  auto fetch = [&](const float* base, int off, int cl, int gx, int c0) {
    const bool ok = off >= 0 && cl < C - c0;
    const float* p = base + (ok ? static_cast<long>(c0) * HW + off : 0);
    float4 v;
    if (DFE_CORR_ABL & 4) return make_float4(1.f, 2.f, 3.f, static_cast<float>(off));
    if (VEC) v = *reinterpret_cast<const float4*>(p);           // W % 4 == 0: a quad is inside or outside as a whole
    else v = load_quad_right(p, ok ? gx : 0, W);
    return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto prefetch = [&](int c0) {
#pragma unroll
    for (int q = 0; q < PF2; ++q) pf2[q] = fetch(f2b, off2[q], cl2[q], gx2[q], c0);
#pragma unroll
    for (int q = 0; q < CF_PF1; ++q) pf1[q] = fetch(f1b, off1[q], cl1[q], gx1[q], c0);
  };
  // One PWC level's input is x = cat(cost volume, c1, flow) (pwc_tf.py:119-121): when `tail` is given (planes 81 ... of x, same
  // batch stride as the cost volume) the f1 quads this block stages anyway are also stored there, and the flow planes copied
  // below -- round 3 ran a copy kernel of its own for that.  Only the block of the first displacement-row group writes.
  float* tail_b = (tail && dyg == 0) ? tail + static_cast<long>(b) * obs : nullptr;
  auto commit = [&](float* buf, int c0) {
#pragma unroll
    for (int q = 0; q < PF2; ++q) { const int e = tid + q * NT; if (e < g.n2) *reinterpret_cast<float4*>(buf + 4 * e) = pf2[q]; }
#pragma unroll
    for (int q = 0; q < CF_PF1; ++q) {
      const int e = tid + q * NT;
      if (e < g.n1) *reinterpret_cast<float4*>(buf + 4 * (g.n2 + e)) = pf1[q];
      if (tail_b && off1[q] >= 0 && cl1[q] < C - c0) {
        float* t = tail_b + static_cast<long>(c0) * HW + off1[q];
        if (VEC) *reinterpret_cast<float4*>(t) = pf1[q];
        else {
          t[0] = pf1[q].x;
          if (gx1[q] + 1 < W) t[1] = pf1[q].y;
          if (gx1[q] + 2 < W) t[2] = pf1[q].z;
          if (gx1[q] + 3 < W) t[3] = pf1[q].w;
        }
      }
    }
  };
  if (tail_b) {       // the two flow planes of this tile
    const float* fb = flow + static_cast<long>(b) * 2 * HW;
    float* tb = tail_b + static_cast<long>(C) * HW;
    for (int e = tid; e < 2 * g.P1; e += NT) {
      const int pl = e / g.P1, rem = e - pl * g.P1, r = rem / g.TXQ, y = ty0 + r, x = tx0 + 4 * (rem - r * g.TXQ);
      if (y < H && x < W) {
        const long o = static_cast<long>(pl) * HW + static_cast<long>(y) * W + x;
        if (VEC) *reinterpret_cast<float4*>(tb + o) = *reinterpret_cast<const float4*>(fb + o);
        else for (int u = 0; u < 4 && x + u < W; ++u) tb[o + u] = fb[o + u];
      }
    }
  }

  // ---- this thread's outputs: displacement row dy, tile row yl, quad xq, channel slot ks
  const int ks = tid / g.NI, item = tid - ks * g.NI;
  const int xq = item % g.TXQ, t2 = item / g.TXQ, yl = t2 % g.TH, dyl = t2 / g.TH, dy = dy0 + dyl;    // dyl: row inside the block's group
  const bool worker = tid < g.NI * g.KS && dy < CR_K;
  const int S2 = 4 * g.Q2, S1 = 4 * g.TXQ;
  const int o2 = (ks * g.R2 + yl + dyl) * S2 + 4 * xq, o1 = 4 * g.n2 + (ks * g.TH + yl) * S1 + 4 * xq;
  const int st2 = g.KS * g.R2 * S2, st1 = g.KS * g.TH * S1, nm = g.CC / g.KS;
  const int buf_floats = 4 * (g.n2 + g.n1);

  float acc[4][CR_K];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int j = 0; j < CR_K; ++j) acc[u][j] = 0.0f;

  const int nchunk = (C + g.CC - 1) / g.CC;
  prefetch(0);
  commit(smem, 0);
  __syncthreads();
  for (int k = 0; k < nchunk; ++k) {
    const float* buf = smem + (k & 1) * buf_floats;
    if (k + 1 < nchunk) prefetch((k + 1) * g.CC);
    if (worker) {
      const float* s2 = buf + o2;
      const float* s1 = buf + o1;
      // the next channel's operands are read from LDS while this one's 36 FMAs issue
      float4 a4 = *reinterpret_cast<const float4*>(s1), w0 = *reinterpret_cast<const float4*>(s2);
      float4 w1 = *reinterpret_cast<const float4*>(s2 + 4), w2 = *reinterpret_cast<const float4*>(s2 + 8);
#pragma unroll 2
      for (int m = 0; m < nm; ++m) {
        const float a[4] = {a4.x, a4.y, a4.z, a4.w};
        const float w[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
        const int mn = (m + 1 < nm) ? m + 1 : m;
        a4 = *reinterpret_cast<const float4*>(s1 + mn * st1);
        w0 = *reinterpret_cast<const float4*>(s2 + mn * st2);
        w1 = *reinterpret_cast<const float4*>(s2 + mn * st2 + 4);
        w2 = *reinterpret_cast<const float4*>(s2 + mn * st2 + 8);
        if (DFE_CORR_ABL & 2) { acc[0][0] += a[0] + a[1] + a[2] + a[3] + w[0] + w[4] + w[8] + w[11]; continue; }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < CR_K; ++j) acc[u][j] = __fmaf_rn(a[u], w[u + j], acc[u][j]);
      }
    }
    if (k + 1 < nchunk) commit(smem + ((k + 1) & 1) * buf_floats, (k + 1) * g.CC);
    __syncthreads();
  }

  const int y = ty0 + yl, x0 = tx0 + 4 * xq;
  float* o = out + static_cast<long>(b) * obs + static_cast<long>(dy * CR_K) * HW + static_cast<long>(y) * W + x0;   // obs: batch stride of out (the 81 planes may be a slice of a wider tensor)
  const bool live = worker && y < H && x0 < W;
  if (g.KS == 1) {
    if ((DFE_CORR_ABL & 1) && acc[0][0] != 12345.678f) return;
    if (live) {
#pragma unroll
      for (int j = 0; j < CR_K; ++j) {
        const float v0 = div_cr(acc[0][j], fC, rC), v1 = div_cr(acc[1][j], fC, rC), v2 = div_cr(acc[2][j], fC, rC), v3 = div_cr(acc[3][j], fC, rC);
        if (VEC) *reinterpret_cast<float4*>(o + j * HW) = make_float4(v0, v1, v2, v3);
        else {
          o[j * HW] = v0;
          if (x0 + 1 < W) o[j * HW + 1] = v1;
          if (x0 + 2 < W) o[j * HW + 2] = v2;
          if (x0 + 3 < W) o[j * HW + 3] = v3;
        }
      }
    }
    return;
  }
  // channel-split partial sums meet in LDS (the staging buffers are free: the loop ended with a barrier) and are added
  // in slot order: red[(ks * 36 + a) * NI + item], a = u * 9 + j; slot ks finishes the components a = ks, ks + KS, ...
  float* red = smem;
  if (worker) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < CR_K; ++j) red[(ks * 36 + u * CR_K + j) * g.NI + item] = acc[u][j];
  }
  __syncthreads();
  if (live) {
    const int nout = 36 * g.NI;
    for (int a = ks; a < 36; a += g.KS) {
      float s = red[a * g.NI + item];
      for (int k2 = 1; k2 < g.KS; ++k2) s += red[k2 * nout + a * g.NI + item];
      const int u = a / CR_K, j = a - u * CR_K;
      if (x0 + u < W) o[j * HW + u] = div_cr(s, fC, rC);
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward
// MODE 0: gin = g1 (other = f2);  MODE 1: gin = g2 (other = f1), planes reversed, gradient sampled at the window position
template <int MODE, bool VEC>
__device__ __forceinline__ void corr_bwd_body(float* smem, const CorrBwdSide sd, const float* __restrict__ gout, long gbs,
                                              int C, int H, int W, float fC, float rC, const CorrBwdCfg& g) {
  const int tid = threadIdx.x, NT = blockDim.x;
  const unsigned bid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int cr = bid % g.ncr, tx = (bid / g.ncr) % g.ntx, ty = (bid / (g.ncr * g.ntx)) % g.nty, b = bid / (g.ncr * g.ntx * g.nty);
  const int tx0 = tx * 4 * g.TXQ, ty0 = ty * g.TH, cbase = cr * g.NCG * CB_CK;
  const long HW = static_cast<long>(H) * W;
  const float* __restrict__ ob = sd.other + static_cast<long>(b) * C * HW;

  // ---- stage the halo tile of `other` for this block's channels: [NCG * 8][R2][Q2] quads, zero outside image / beyond C.
  // Batches of CB_STAGE quads per thread, all loads of a batch in flight at once (nothing else is live yet: the
  // registers are free) -- a block's arithmetic is only a few microseconds, every serial round trip here shows.
  {
    StagePos s = stage_first(tid, g.mP2, g.mQ2, g.P2, g.Q2);
    for (int e0 = 0; e0 < g.tile_quads; e0 += CB_STAGE * NT) {
      float4 v[CB_STAGE];
#pragma unroll
      for (int q = 0; q < CB_STAGE; ++q) {
        const int gy = ty0 - CR_D + s.r, gx = tx0 - CR_D + 4 * s.q, c = cbase + s.cl;
        const bool ok = (e0 + q * NT + tid < g.tile_quads) && c < C && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const float* p = ob + (ok ? static_cast<long>(c) * HW + static_cast<long>(gy) * W + gx : 0);
        float4 t;
        if (VEC) t = *reinterpret_cast<const float4*>(p);
        else t = load_quad_right(p, ok ? gx : 0, W);
        v[q] = ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
        stage_next(s, g.st, g.R2, g.Q2);
      }
#pragma unroll
      for (int q = 0; q < CB_STAGE; ++q) {
        const int e = e0 + q * NT + tid;
        if (e < g.tile_quads) *reinterpret_cast<float4*>(smem + 4 * e) = v[q];
      }
    }
  }
  __syncthreads();

  const bool worker = tid < g.NI * g.IS;
  const int is = tid / g.NI, item = tid - is * g.NI;
  const int xq = item % g.TXQ, t2 = item / g.TXQ, yl = t2 % g.TH, cg = t2 / g.TH;
  const int S2 = 4 * g.Q2, PF = g.R2 * S2;          // floats per tile row / per channel
  const int y = ty0 + yl, x0 = tx0 + 4 * xq;
  const bool live = worker && y < H && x0 < W;
  const float* __restrict__ gb = gout + static_cast<long>(b) * gbs;

  float acc[CB_CK][4];
#pragma unroll
  for (int c = 0; c < CB_CK; ++c)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[c][u] = 0.0f;

  // the 9 gradient quads of displacement row i (zero where the sampled pixel is outside the image)
  auto load_g = [&](int i, float (&gq)[CR_K][4]) {
    if (MODE == 0) {
      const float* gp = gb + static_cast<long>(i * CR_K) * HW + static_cast<long>(y) * W + x0;
#pragma unroll
      for (int j = 0; j < CR_K; ++j) {
        float4 v;
        if (VEC) v = *reinterpret_cast<const float4*>(gp + j * HW);
        else v = load_quad_checked(gp + j * HW, x0, W);
        gq[j][0] = v.x; gq[j][1] = v.y; gq[j][2] = v.z; gq[j][3] = v.w;
      }
    } else {
      const int yy = y + i - CR_D;
      const bool row_ok = yy >= 0 && yy < H;
      const float* gp = gb + static_cast<long>(CR_NK - 1 - i * CR_K) * HW + static_cast<long>(row_ok ? yy : 0) * W + x0 - CR_D;
#pragma unroll
      for (int j = 0; j < CR_K; ++j) {
        const int gx = x0 - CR_D + j;
        float4 v;
        if (VEC && j == CR_D) v = *reinterpret_cast<const float4*>(gp - static_cast<long>(j) * HW + j);   // the centre column is the thread's own aligned quad
        else if (gx >= 0 && gx + 3 < W) { const QuadU qv = *reinterpret_cast<const QuadU*>(gp - static_cast<long>(j) * HW + j); v = make_float4(qv.a, qv.b, qv.c, qv.d); }
        else v = load_quad_checked(gp - static_cast<long>(j) * HW + j, gx, W);
        gq[j][0] = row_ok ? v.x : 0.0f; gq[j][1] = row_ok ? v.y : 0.0f; gq[j][2] = row_ok ? v.z : 0.0f; gq[j][3] = row_ok ? v.w : 0.0f;
      }
    }
  };

  if (live) {
    const float* tl = smem + (cg * CB_CK) * PF + yl * S2 + 4 * xq;
    float gn[CR_K][4];
    load_g(is, gn);
#pragma unroll 1
    for (int i = is; i < CR_K; i += g.IS) {
      float gq[CR_K][4];
#pragma unroll
      for (int j = 0; j < CR_K; ++j)
#pragma unroll
        for (int u = 0; u < 4; ++u) gq[j][u] = gn[j][u];
      if (i + g.IS < CR_K) load_g(i + g.IS, gn);     // the next row's gradients are in flight while this row is multiplied
      const float* tr = tl + i * S2;
#pragma unroll
      for (int c = 0; c < CB_CK; ++c) {
        const float4 w0 = *reinterpret_cast<const float4*>(tr + c * PF);
        const float4 w1 = *reinterpret_cast<const float4*>(tr + c * PF + 4);
        const float4 w2 = *reinterpret_cast<const float4*>(tr + c * PF + 8);
        const float w[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
#pragma unroll
        for (int j = 0; j < CR_K; ++j)
#pragma unroll
          for (int u = 0; u < 4; ++u) acc[c][u] = __fmaf_rn(gq[j][u], w[u + j], acc[c][u]);
      }
    }
  }

  const int c0 = cbase + cg * CB_CK;
  float* gi = sd.gin + static_cast<long>(b) * C * HW + static_cast<long>(c0) * HW + static_cast<long>(y) * W + x0;
  const float* ad = sd.addend ? sd.addend + static_cast<long>(b) * sd.abs_ + static_cast<long>(c0) * HW + static_cast<long>(y) * W + x0 : nullptr;
  if (g.IS == 1) {
    unsigned am = 0u;
    if (live) {
#pragma unroll
      for (int c = 0; c < CB_CK; ++c) {
        if (c0 + c >= C) break;
        float v0 = div_cr(acc[c][0], fC, rC), v1 = div_cr(acc[c][1], fC, rC), v2 = div_cr(acc[c][2], fC, rC), v3 = div_cr(acc[c][3], fC, rC);
        if (VEC) {
          if (ad) { const float4 a4 = *reinterpret_cast<const float4*>(ad + c * HW); v0 += a4.x; v1 += a4.y; v2 += a4.z; v3 += a4.w; }
          *reinterpret_cast<float4*>(gi + c * HW) = make_float4(v0, v1, v2, v3);
          am = max(max(am, abs_bits(v0)), max(abs_bits(v1), max(abs_bits(v2), abs_bits(v3))));
        } else {
          const float vv[4] = {v0, v1, v2, v3};
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (x0 + u < W) { const float r = ad ? vv[u] + ad[c * HW + u] : vv[u]; gi[c * HW + u] = r; am = max(am, abs_bits(r)); }
        }
      }
    }
    if (sd.amax) wave_amax_to(sd.amax, am);        // every lane of every wave arrives here
    return;
  }
  // displacement-row partials meet in LDS in row-slot order: red[(is * 32 + a) * NI + item], a = c * 4 + u; row slot `is`
  // finishes the components a = is, is + IS, ...
  __syncthreads();                                   // every thread is done with the tile
  float* red = smem;
  if (worker) {
#pragma unroll
    for (int c = 0; c < CB_CK; ++c)
#pragma unroll
      for (int u = 0; u < 4; ++u) red[(is * 32 + c * 4 + u) * g.NI + item] = acc[c][u];
  }
  __syncthreads();
  unsigned am = 0u;
  if (live) {
    const int nout = 32 * g.NI;
    for (int a = is; a < 32; a += g.IS) {
      float s = red[a * g.NI + item];
      for (int k2 = 1; k2 < g.IS; ++k2) s += red[k2 * nout + a * g.NI + item];
      const int c = a >> 2, u = a & 3;
      if (c0 + c < C && x0 + u < W) {
        float v = div_cr(s, fC, rC);
        if (ad) v += ad[c * HW + u];
        gi[c * HW + u] = v;
        am = max(am, abs_bits(v));
      }
    }
  }
  if (sd.amax) wave_amax_to(sd.amax, am);
}

// both gradients in one launch: blockIdx.y picks the side (mode0: the first side's MODE)
template <bool VEC>
__global__ void __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_corr_bwd_lds(CorrBwdSide s0, CorrBwdSide s1, int mode0, const float* __restrict__ gout, long gbs, int C, int H, int W,
               float fC, float rC, CorrBwdCfg g) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  if (static_cast<int>(blockIdx.y) + mode0 == 0) corr_bwd_body<0, VEC>(smem, s0, gout, gbs, C, H, W, fC, rC, g);
  else corr_bwd_body<1, VEC>(smem, blockIdx.y == 0 ? s0 : s1, gout, gbs, C, H, W, fC, rC, g);
}

// ------------------------------------------------------------------------------------------------ host side
inline bool al16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// DFE_CORR_FWD="TH,KS,CC" / DFE_CORR_BWD="TH,NCG,IS": tuning override (tools/corr_bench.py); 0 keeps the heuristic's value
inline void env_triple(const char* name, int& a, int& b, int& c) {
  const char* s = std::getenv(name);
  if (!s) return;
  int x = 0, y = 0, z = 0;
  if (std::sscanf(s, "%d,%d,%d", &x, &y, &z) >= 1) { if (x > 0) a = x; if (y > 0) b = y; if (z > 0) c = z; }
}

inline void tile_width(int W, int& TXQ, int& ntx) {
  const int WQ = (W + 3) / 4;
  ntx = (WQ + 15) / 16;                  // at most 16 quads (one 256-byte LDS row segment) per tile row
  TXQ = (WQ + ntx - 1) / ntx;
}

bool corr_fwd_config(int B, int C, int H, int W, CorrFwdCfg& g, int& NT, size_t& lds, int& pf2, bool* is_coarse = nullptr) {
  int TXQ, ntx;
  tile_width(W, TXQ, ntx);
  // rows per tile: 4 where that still gives every CU a block, fewer on the small levels (measured per PWC level:
  // tools/corr_bench.py --sweep, profiles/r04_corr_sweep.txt)
  int TH = 4;
  while (TH > 1 && (TH > H || static_cast<long>(B) * ((H + TH - 1) / TH) * ntx < 256)) TH >>= 1;
  // displacement rows per block: all 9 where the tiles alone fill the chip; 3 on the coarse levels (three times the
  // blocks, a 3-row instead of a 9-row f2 tile each: 13.8 / 19.7 / 17.2 -> 11.4 / 11.0 / 12.1 us at levels 4 / 5 / 6)
  int KS = 0, CC = 0, DYG = static_cast<long>(B) * ((H + TH - 1) / TH) * ntx >= 256 ? CR_K : 3;
  env_triple("DFE_CORR_FWD", TH, KS, CC);
  if (const int v = env_int("DFE_CORR_DYG", 0); v >= 1 && v <= CR_K) DYG = v;
  const int ndyg = (CR_K + DYG - 1) / DYG;
  int NI = TH * TXQ * DYG;
  while (NI > 512 && TH > 1) { TH >>= 1; NI = TH * TXQ * DYG; }
  if (NI > 512) return false;
  if (KS <= 0) KS = static_cast<long>(B) * ((H + TH - 1) / TH) * ntx >= 256 ? 1 : 512 / NI;   // the channel sum is split only where the grid cannot fill the chip
  if (KS > C) KS = C;
  if (KS < 1) KS = 1;
  while (NI * KS > 512) --KS;
  NT = ((NI * KS + 63) / 64) * 64;
  const int R2 = TH + DYG - 1, Q2 = TXQ + 2, P2 = R2 * Q2, P1 = TH * TXQ;      // rows y + dy - 4 for the block's dy group
  const long blocks = static_cast<long>(B) * ((H + TH - 1) / TH) * ntx * ndyg;
  // fine levels (every CU has two 512-thread blocks): chunks of ~8 channels, 4 staged quads per thread (<= 128 VGPRs),
  // 2 x 36 KB of LDS; coarse levels: as few chunks as 10 staged quads per thread and 2 x 72 KB of LDS allow -- every
  // chunk is a global-memory round trip that the little arithmetic of a small level cannot hide
  const bool coarse = blocks * NT < 256l * 1024;
  if (is_coarse) *is_coarse = coarse;
  auto fits = [&](int cc, int pf, long cap) {
    return static_cast<long>(cc) * P2 <= static_cast<long>(pf) * NT && static_cast<long>(cc) * P1 <= static_cast<long>(CF_PF1) * NT &&
           static_cast<long>(cc) * (P2 + P1) * 16 <= cap;
  };
  const int Cr = ((C + KS - 1) / KS) * KS;
  if (CC <= 0) {
    CC = KS;
    if (coarse) while (CC + KS <= Cr && fits(CC + KS, 10, 72 * 1024) && 3 * (CC + KS) <= Cr + 3 * KS - 1) CC += KS;   // about three chunks
    else while (CC + KS <= Cr && fits(CC + KS, 4, 36 * 1024) && (KS > 1 || CC < 8)) CC += KS;
    const int nch = (C + CC - 1) / CC;      // the same number of chunks with the smallest chunk size
    while (CC - KS >= KS && (C + (CC - KS) - 1) / (CC - KS) == nch) CC -= KS;
  }
  CC = ((CC + KS - 1) / KS) * KS;
  if (CC > Cr) CC = Cr;
  while (CC > KS && !fits(CC, 10, 72 * 1024)) CC -= KS;
  if (!fits(CC, 10, 72 * 1024)) return false;
  pf2 = fits(CC, 4, 36 * 1024) ? 4 : 10;
  g.TH = TH; g.TXQ = TXQ; g.KS = KS; g.CC = CC; g.DYG = DYG; g.ndyg = ndyg; g.ntx = ntx; g.nty = (H + TH - 1) / TH; g.NI = NI;
  g.R2 = R2; g.Q2 = Q2; g.P2 = P2; g.P1 = P1; g.n2 = CC * P2; g.n1 = CC * P1;
  g.mP2 = make_magic(P2); g.mQ2 = make_magic(Q2); g.mP1 = make_magic(P1); g.mTXQ = make_magic(TXQ);
  g.s2 = make_step(NT, R2, Q2); g.s1 = make_step(NT, TH, TXQ);
  lds = 2ul * (g.n2 + g.n1) * 16;
  if (KS > 1 && static_cast<size_t>(KS) * 36 * NI * 4 > lds) lds = static_cast<size_t>(KS) * 36 * NI * 4;
  return lds <= CORR_MAX_LDS && static_cast<long>(C) * H * W < (1l << 30);
}

bool corr_bwd_config(int B, int C, int H, int W, int sides, CorrBwdCfg& g, int& NT, size_t& lds) {
  int TXQ, ntx;
  tile_width(W, TXQ, ntx);
  const int ngroups = (C + CB_CK - 1) / CB_CK;
  auto nblocks = [&](int th, int ncg) { return static_cast<long>(B) * ((H + th - 1) / th) * ntx * ((ngroups + ncg - 1) / ncg); };
  auto tile_bytes = [&](int th, int ncg) { return static_cast<long>(ncg) * CB_CK * (th + 2 * CR_D) * (TXQ + 2) * 16; };
  // The largest tile (rows first, then channel groups: the gradient planes are read once per channel range) that
  // keeps >= 512 blocks in the launch (both gradients go out together), <= 128 KB of LDS and <= 512 work items
  // (measured per PWC level: tools/corr_bench.py --sweep, profiles/r04_corr_sweep.txt)
  int TH = 1, NCG = 1, IS = 0;
  {
    bool found = false;
    for (int th = 8; th >= 1 && !found; th >>= 1) {
      if (th > H && th > 1) continue;
      for (int ncg = ngroups; ncg >= 1; --ncg) {
        if (tile_bytes(th, ncg) > 128 * 1024 || ncg * th * TXQ > 512) continue;
        if (nblocks(th, ncg) * sides < 512 && !(th == 1 && ncg == 1)) continue;
        TH = th; NCG = ncg; found = true;
        break;
      }
    }
  }
  {
    int th = 0, ncg = 0;
    env_triple("DFE_CORR_BWD", th, ncg, IS);
    if (th > 0) TH = th;
    if (ncg > 0) NCG = ncg;
  }
  const int R2 = TH + 2 * CR_D, Q2 = TXQ + 2, P2 = R2 * Q2;
  if (NCG > ngroups) NCG = ngroups;
  const int NI = NCG * TH * TXQ;
  if (NI > 512) return false;
  if (IS <= 0) IS = NI * 9 <= 256 ? 9 : (NI * 3 <= 256 ? 3 : 1);
  while (NI * IS > 512) --IS;
  NT = ((NI * IS + 63) / 64) * 64;
  g.TH = TH; g.TXQ = TXQ; g.NCG = NCG; g.IS = IS; g.ntx = ntx; g.nty = (H + TH - 1) / TH; g.ncr = (ngroups + NCG - 1) / NCG; g.NI = NI;
  g.R2 = R2; g.Q2 = Q2; g.P2 = P2; g.mP2 = make_magic(P2); g.mQ2 = make_magic(Q2);
  g.tile_quads = NCG * CB_CK * P2;
  g.st = make_step(NT, R2, Q2);
  lds = static_cast<size_t>(g.tile_quads) * 16;
  if (IS > 1 && static_cast<size_t>(IS) * 32 * NI * 4 > lds) lds = static_cast<size_t>(IS) * 32 * NI * 4;
  return lds <= CORR_MAX_LDS;
}

// more than 64 KB of dynamic LDS has to be allowed per kernel, once per process (one device per process).
// KERNEL is the kernel itself, not its type: every instantiation of a kernel template has the same function type, and a
// flag per type would be set by whichever instantiation asked first and skip the call for the others.
template <auto KERNEL>
inline bool allow_lds(size_t lds) {
  if (lds <= 64 * 1024) return true;
  static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, CORR_MAX_LDS) == hipSuccess;
  return ok;
}

template <bool VEC, int PF2, int WPE>
inline int run_corr_fwd(const float* f1, const float* f2, float* out, long obs, float* tail, const float* flow, int B, int C, int H, int W,
                        const CorrFwdCfg& g, int NT, size_t lds, hipStream_t st) {
  if (!allow_lds<k_corr_fwd_lds<VEC, PF2, WPE>>(lds)) return DFE_ERR_LAUNCH;
  const float fC = static_cast<float>(C), rC = 1.0f / fC;
  k_corr_fwd_lds<VEC, PF2, WPE><<<static_cast<unsigned>(B) * g.nty * g.ntx * g.ndyg, NT, lds, st>>>(f1, f2, out, obs, tail, flow, C, H, W, fC, rC, g);
  return DFE_OK;
}

}  // namespace

int launch_corr_fwd(const float* f1, const float* f2, float* out, long obs, float* tail, const float* flow, int B, int C, int H, int W,
                    hipStream_t st) {
  CorrFwdCfg g;
  int NT, pf2;
  size_t lds;
  if (!corr_fwd_config(B, C, H, W, g, NT, lds, pf2)) return DFE_ERR_UNSUPPORTED;
  const bool vec = (W % 4 == 0) && al16(f1) && al16(f2) && al16(out) && obs % 4 == 0 && al16(tail) && al16(flow);
  if (tail && !flow) return DFE_ERR_NULL;
  if (pf2 == 4) return vec ? run_corr_fwd<true, 4, 4>(f1, f2, out, obs, tail, flow, B, C, H, W, g, NT, lds, st)
                           : run_corr_fwd<false, 4, 3>(f1, f2, out, obs, tail, flow, B, C, H, W, g, NT, lds, st);
  return vec ? run_corr_fwd<true, 10, 2>(f1, f2, out, obs, tail, flow, B, C, H, W, g, NT, lds, st)
             : run_corr_fwd<false, 10, 2>(f1, f2, out, obs, tail, flow, B, C, H, W, g, NT, lds, st);
}

// gout: 81 planes per sample with batch stride gbs; add1 (batch stride abs1) is added to g1 when given.  Both gradients
// go out in ONE launch (grid.y = 2).  amax2 (optional): a zeroed word that receives max |g2| as a bit pattern -- the bound
// of the feature-warp scatter that follows in a PWC level (dfe_scatter.h), saving that pass its own max-reduction launch.
int launch_corr_bwd(const float* f1, const float* f2, const float* gout, long gbs, const float* add1, long abs1,
                    float* g1, float* g2, unsigned* amax2, int B, int C, int H, int W, hipStream_t st) {
  CorrBwdCfg g;
  int NT;
  size_t lds;
  if (!corr_bwd_config(B, C, H, W, (g1 && g2) ? 2 : 1, g, NT, lds)) return DFE_ERR_UNSUPPORTED;
  const bool vec = (W % 4 == 0) && al16(f1) && al16(f2) && al16(gout) && al16(g1) && al16(g2) && al16(add1) && gbs % 4 == 0 && abs1 % 4 == 0;
  const float fC = static_cast<float>(C), rC = 1.0f / fC;
  const CorrBwdSide side1{f2, g1, add1, abs1, nullptr}, side2{f1, g2, nullptr, 0, g2 ? amax2 : nullptr};
  const CorrBwdSide s0 = g1 ? side1 : side2, s1 = side2;
  const int mode0 = g1 ? 0 : 1;
  const dim3 grid(static_cast<unsigned>(B) * g.nty * g.ntx * g.ncr, (g1 && g2) ? 2 : 1);
  if (vec) {
    if (!allow_lds<k_corr_bwd_lds<true>>(lds)) return DFE_ERR_LAUNCH;
    k_corr_bwd_lds<true><<<grid, NT, lds, st>>>(s0, s1, mode0, gout, gbs, C, H, W, fC, rC, g);
  } else {
    if (!allow_lds<k_corr_bwd_lds<false>>(lds)) return DFE_ERR_LAUNCH;
    k_corr_bwd_lds<false><<<grid, NT, lds, st>>>(s0, s1, mode0, gout, gbs, C, H, W, fC, rC, g);
  }
  return DFE_OK;
}

}  // namespace dfe

// ------------------------------------------------------------------------------------------------ plan queries (host only)
// What launch_corr_fwd / launch_corr_bwd decide for a shape, from the same two functions and the same environment overrides;
// nothing is launched and no device is touched.  `vec`: whether every pointer and batch stride of the call is 16-byte aligned
// (the launchers' al16 / % 4 tests); the kernels are the VEC ones only when W % 4 == 0 as well, which the last field reports.
extern "C" int dfe_corr_fwd_plan(int B, int C, int H, int W, int vec, int* plan) {
  if (!plan) return DFE_ERR_NULL;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return DFE_ERR_DIMS;
  dfe::CorrFwdCfg g;
  int NT, pf2;
  size_t lds;
  bool coarse;
  if (!dfe::corr_fwd_config(B, C, H, W, g, NT, lds, pf2, &coarse)) return DFE_ERR_UNSUPPORTED;
  const int v[12] = {g.TH, g.TXQ, g.ntx, g.KS, g.CC, g.DYG, pf2, NT, static_cast<int>(lds), (C + g.CC - 1) / g.CC, coarse ? 1 : 0,
                     (vec && W % 4 == 0) ? 1 : 0};
  for (int i = 0; i < 12; ++i) plan[i] = v[i];
  return DFE_OK;
}

extern "C" int dfe_corr_bwd_plan(int B, int C, int H, int W, int sides, int vec, int* plan) {
  if (!plan) return DFE_ERR_NULL;
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || sides < 1 || sides > 2) return DFE_ERR_DIMS;
  dfe::CorrBwdCfg g;
  int NT;
  size_t lds;
  if (!dfe::corr_bwd_config(B, C, H, W, sides, g, NT, lds)) return DFE_ERR_UNSUPPORTED;
  const int per = dfe::CB_STAGE * NT;
  const int v[10] = {g.TH, g.TXQ, g.ntx, g.NCG, g.ncr, g.IS, NT, static_cast<int>(lds), (g.tile_quads + per - 1) / per, (vec && W % 4 == 0) ? 1 : 0};
  for (int i = 0; i < 10; ++i) plan[i] = v[i];
  return DFE_OK;
}
