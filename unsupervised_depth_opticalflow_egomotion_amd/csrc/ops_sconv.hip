// Weight gradients of the networks' STRIDED convolutions on the fp32 matrix cores, straight from NCHW (reference layers: the ResNet18
// encoder's 7x7/2 stem depth_model.py:60-95, FeaturePyramid's first 3x3/2 layers feature_pyramid.py:7-36, PoseCNN's 7x7/2 and 5x5/2
// layers pose_cnn.py:14-36).  MIOpen ran them as NHWC implicit GEMMs wrapped in three layout transposes and a zero fill and reached
// 6 - 40 TFLOP/s on the 3-, 9- and 16-channel inputs (profiles/r05_sconv_bench_all.md); here ONE launch (+ a fixed-order sum of the
// split partials) stages raw NCHW rows in LDS and reads the matrix-core operands from there:
//     dW[co][ci][ky][kx] = sum_pixels gy[co][oy][ox] x[ci][S oy + D ky - P][S ox + D kx - P]
// is a GEMM (co) x (ci, ky, kx) whose reduction runs over the output pixels.  v_mfma_f32_16x16x4_f32 takes "one row / column per
// lane & 15, one of four reduction slots per lane >> 4": the A operand is gy[co = lane & 15][pixel 4 g + (lane >> 4)], the B
// operand x at the lane's OWN (ci, ky, kx) column for the same pixel -- a per-lane LDS offset fixed for the whole kernel plus
// the step's uniform pixel offset.  For stride 2 the staged x rows are split into even and odd columns so that the four
// pixels of a step are four consecutive words.  Columns are either "one filter tap per 16-lane tile, 16 input channels
// across the lanes" (Ci >= 16) or the flattened (ci, ky, kx) index (the 3- and 9-channel stems, 5x5).  The pixel range is
// split over blocks; partials [split][co][ci][ky][kx] are added in split order by k_wgrad_sum: no atomics, bit-reproducible.
// Bound: MFMA (157 TFLOP/s fp32 dense) for the wide layers, HBM for the 3-channel stems.
// The forward pass (k_sconv_fwd) and the data gradient (k_sconv_dgrad) in the same style -- filter slab packed [ci / 4][tap][ci % 4][Co],
// the data gradient as four phase correlations -- are on a par with MIOpen's whole call per layer but lose 0.05 - 0.15 ms in the step
// (EXPERIMENT_LOG.md "strided convolutions"): only the deterministic mode (convs.set_deterministic) routes layers to them, because
// their sums have one fixed order.  The 1x1 stride-2 layers of the same mode: ops_conv1x1s2.hip.
#include "dfe_internal.h"
#include "dfe_device.h"
#include "dfe_mfma_stage.h"
#include "dfe_wgrad_sum.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>

namespace dfe {

struct ScWg {
  long xbs, gbs;
  int Ci, Co, H, W, Ho, Wo, KH, KW, S, D, P, flat;
  int TH, TW;              // a chunk: TH output rows x TW output columns (TW % 4 == 0)
  int RI, NSLOT, QW;       // staged input rows, 16-byte slots per staged row, words per column phase (stride 2)
  int XRS, XCS, GCS;       // LDS strides: x row, x channel, gy channel (a gy row is TW words)
  int DX;                  // columns the staged window starts left of the first tap's: the window starts on a multiple of 4
  int CIB, COB;            // channels of a block: input (the column slab) / output
  int XCH, GCH;            // ... rounded up to whole thread groups: the channels the LDS regions hold
  int cpr, rpi, nchunks, cps, ncit, ntb;
};

// MT x NT tiles of 16 x 16 per wave, WM x WN waves per block: COB = 16 MT WM output channels x 16 NT WN columns.  Staging: a thread
// group of 2^XSH threads covers the (row, 16-byte slot) positions of the x window and each thread loads NXL channels 256 >> XSH
// apart (2^GSH, NGL for gy): the counts are compile-time so that the prefetch is straight-line code in registers.
template <int MT, int NT, int WM, int WN, int XSH, int NXL, int GSH, int NGL>
__global__ void __launch_bounds__(256, (NT <= 7 && NXL <= 9) ? 3 : 2)
k_sconv_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ part, const ScWg g) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, kq = lane >> 4;
  const int wm = wv / WN, wn = wv % WN;
  const unsigned lid = xcd_swizzle(blockIdx.x, gridDim.x);
  const int tb = static_cast<int>(lid % static_cast<unsigned>(g.ntb)), split = static_cast<int>(lid / static_cast<unsigned>(g.ntb));
  const int cob0 = (tb / g.ncit) * g.COB, cib0 = (tb % g.ncit) * g.CIB;
  const int c_beg = split * g.cps, c_end = min(g.nchunks, c_beg + g.cps);
  const int KK = g.KH * g.KW, HW = g.H * g.W, gHW = g.Ho * g.Wo;
  const int XTOT = g.XCH * g.XCS;

  // ---- the lane's operand offsets
  int boff[NT], oidx[NT], aoff[MT];
  bool any_col = false;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int tile = wn * NT + j;
    int ci_l, t;
    bool ok;
    if (g.flat) { const int col = tile * 16 + i; ci_l = col / KK; t = col - ci_l * KK; ok = ci_l < g.CIB; }
    else { t = tile % KK; ci_l = (tile / KK) * 16 + i; ok = ci_l < g.CIB; }
    ok = ok && cib0 + ci_l < g.Ci;
    const int ky = t / g.KW, kx = t - ky * g.KW, dk = g.D * kx + g.DX;
    const int o = ci_l * g.XCS + g.D * ky * g.XRS + (g.S == 2 ? (dk & 1) * g.QW + (dk >> 1) : dk) + kq;
    boff[j] = ok ? o : kq;
    oidx[j] = ok ? (cib0 + ci_l) * KK + t : -1;
    any_col = any_col || ok;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) aoff[mt] = XTOT + ((wm * MT + mt) * 16 + i) * g.GCS + kq;
  const bool wave_on = __any(any_col) && cob0 + wm * MT * 16 < g.Co;

  // ---- staging: thread = (position = (row, slot) of the window, channel group)
  constexpr int xncg = 256 >> XSH, gncg = 256 >> GSH;
  const int xpos = tid & ((1 << XSH) - 1), xcg = tid >> XSH;
  const int xr_ = xpos / g.NSLOT, xs_ = xpos - xr_ * g.NSLOT;
  const bool xact = xpos < g.RI * g.NSLOT;
  const int xl0 = xcg * g.XCS + xr_ * g.XRS + (g.S == 2 ? 2 : 4) * xs_;
  const int GSL = g.TW >> 2;
  const int gpos = tid & ((1 << GSH) - 1), gcg = tid >> GSH;
  const int gr_ = gpos / GSL, gs_ = gpos - gr_ * GSL;
  const bool gact = gpos < g.TH * GSL;
  const int gl0 = XTOT + gcg * g.GCS + gr_ * g.TW + 4 * gs_;
  f32x4 xr[NXL], gr[NGL];

  // the loads' safe address: the sample's first words (sc_wg_plan: no tensor of fewer than four)
  const int xnch = min(g.CIB, g.Ci - cib0), gnch = min(g.COB, g.Co - cob0);
  auto load_chunk = [&](int c) {
    const int cx = c % g.cpr, ry = (c / g.cpr) % g.rpi, img = c / g.cpr / g.rpi;
    {
      const int iy = g.S * ry * g.TH - g.P + xr_, ix = g.S * cx * g.TW - g.P - g.DX + 4 * xs_;
      const bool rowok = xact && iy >= 0 && iy < g.H;
      const bool full = rowok && ix >= 0 && ix + 3 < g.W;
      const bool cut = rowok && !full && ix + 3 >= 0 && ix < g.W;
      const float* xb = x + img * g.xbs;
      load_slots(xr, xb, (cib0 + xcg) * HW + iy * g.W + ix, HW, xcg, xncg, xnch, ix, g.W, full, cut);
    }
    {
      const int oy = ry * g.TH + gr_, ox = cx * g.TW + 4 * gs_;
      const bool rowok = gact && oy < g.Ho;
      const bool full = rowok && ox + 3 < g.Wo;
      const bool cut = rowok && !full && ox < g.Wo;
      const float* gb = gy + img * g.gbs;
      load_slots(gr, gb, (cob0 + gcg) * gHW + oy * g.Wo + ox, gHW, gcg, gncg, gnch, ox, g.Wo, full, cut);
    }
  };
  // the LDS regions hold whole thread groups of channels (XCH / GCH >= CIB / COB): every active thread stores
  auto store_chunk = [&]() {
    if (xact) {
#pragma unroll
      for (int jj = 0; jj < NXL; ++jj) {
        float* d = lds + xl0 + jj * xncg * g.XCS;
        if (g.S == 2) store_slot_split(d, g.QW, xr[jj]);
        else store_slot_pairs(d, xr[jj]);
      }
    }
    if (gact) {
#pragma unroll
      for (int jj = 0; jj < NGL; ++jj) store_slot_pairs(lds + gl0 + jj * gncg * g.GCS, gr[jj]);      // the channel stride is even, not a multiple of four
    }
  };

  f32x4 acc[MT][NT] = {};

  if (c_beg < c_end) {
    load_chunk(c_beg);
    store_chunk();
  }
  __syncthreads();
  const int xstep_row = g.S * g.XRS;
  for (int c = c_beg; c < c_end; ++c) {
    const bool more = c + 1 < c_end;
    if (more) load_chunk(c + 1);
    if (wave_on) {
      // two steps per trip, the operands of the next step read while this step's MFMAs run (the compiler, left alone, waits for
      // every LDS word right before the MFMA that takes it: a third of the pipe)
      const int n4 = g.TW >> 2;
      for (int oyl = 0; oyl < g.TH; ++oyl) {
        int pa[MT], pb[NT];      // word offsets (pointers would lose the LDS address space: flat loads)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) pa[mt] = aoff[mt] + oyl * g.TW;
#pragma unroll
        for (int j = 0; j < NT; ++j) pb[j] = boff[j] + oyl * xstep_row;
        float a0[MT], b0[NT], a1[MT], b1[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) a0[mt] = lds[pa[mt]];
#pragma unroll
        for (int j = 0; j < NT; ++j) b0[j] = lds[pb[j]];
        int s4 = 0;
        // sched_barrier: left alone, the scheduler merges the reads of the two steps into ds_read2 or sinks them to right before
        // their first use (no prefetch left)
        for (; s4 + 2 <= n4; s4 += 2) {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) a1[mt] = lds[pa[mt] + 4];
#pragma unroll
          for (int j = 0; j < NT; ++j) b1[j] = lds[pb[j] + 4];
          __builtin_amdgcn_sched_barrier(0);
          mfma_tile(acc, a0, b0);
          __builtin_amdgcn_sched_barrier(0);
          // unconditional (past the row's end in the last trip: words nobody uses, inside the allocation + its 16-word tail): a
          // branch here makes the compiler wait for ALL outstanding LDS words at the loop's head
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) a0[mt] = lds[pa[mt] + 8];
#pragma unroll
          for (int j = 0; j < NT; ++j) b0[j] = lds[pb[j] + 8];
          __builtin_amdgcn_sched_barrier(0);
          mfma_tile(acc, a1, b1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) pa[mt] += 8;
#pragma unroll
          for (int j = 0; j < NT; ++j) pb[j] += 8;
        }
        if (s4 < n4) mfma_tile(acc, a0, b0);
      }
    }
    __syncthreads();
    if (more) {
      store_chunk();
      __syncthreads();
    }
  }

  // ---- partial sums of this split: [co][ci][ky][kx]
  float* po = part + static_cast<long>(split) * g.Co * g.Ci * KK;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = cob0 + (wm * MT + mt) * 16 + 4 * kq + r;
      if (co >= g.Co) continue;
#pragma unroll
      for (int j = 0; j < NT; ++j)
        if (oidx[j] >= 0) po[static_cast<long>(co) * g.Ci * KK + oidx[j]] = acc[mt][j][r];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Forward: y[co][oy][ox] = act(bias[co] + sum_(ci, ky, kx) w[co][ci][ky][kx] x[ci][2 oy + ky - P][2 ox + kx - P]), K x K, stride 2,
// P = K / 2.  A GEMM (co) x (pixels) whose reduction runs over (ci, ky, kx): a step of v_mfma_f32_16x16x4_f32 takes four INPUT
// CHANNELS at one tap.  The A operand is the filter w[co = lane & 15][ci = 4 c4 + (lane >> 4)][tap] from a slab that k_sconv_pack laid
// out as rows [ci / 4][tap][ci % 4][Co] (16-byte copies into LDS, no index arithmetic in the loop), the B operand the staged x at the
// lane's own output pixel (a per-lane LDS offset) plus the tap's uniform offset; x rows are split into even and odd columns as in the
// weight gradient.  A block = COB output channels x a tile of TH x TW output pixels (16 NT WN pixels, numbered row-major inside the
// tile), the input channels in chunks of CB; thin layers split the chunks over blocks and k_sconv_sum adds the partials in order.

// The geometry of the forward and of the data gradient (below): "staged" is the tensor whose windows go through LDS (x / gy),
// "written" the one the block's accumulators go to (y / gx).
struct ScGeo {
  long sbs, obs;                 // batch strides of the staged and of the written tensor
  int Ci, Co, H, W, Ho, Wo;      // x and gx are [Ci][H][W], y and gy [Co][Ho][Wo]
  int TH, TW, RI, NSLOT, QW, XRS, XCS;
  int CB, nck, cps, nsplit;      // staged channels per chunk, chunks, chunks per split
  int cpr, rpi, ntile, ncb;      // tiles per row, tile rows per image, tiles, blocks over the written channels
  int Mp, WRS;                   // padded written channels of the packed filter; LDS row stride of the filter slab
  int wl4;                       // 16-byte words of a chunk's filter slab
  float slope;                   // forward: the activation
};

// block = (written-channel block fastest: the blocks that share a staged window are neighbours, pixel tile, split)
struct ScBlock { int cb, cx, ry, img, split, c_beg, c_end; };
__device__ __forceinline__ ScBlock sc_block(const ScGeo& g) {
  const unsigned lid = xcd_swizzle(blockIdx.x, gridDim.x), ncb = static_cast<unsigned>(g.ncb), ntile = static_cast<unsigned>(g.ntile);
  const int tile = static_cast<int>((lid / ncb) % ntile), split = static_cast<int>(lid / (ncb * ntile));
  return ScBlock{static_cast<int>(lid % ncb), tile % g.cpr, (tile / g.cpr) % g.rpi, tile / g.cpr / g.rpi, split, split * g.cps,
                 min(g.nck, split * g.cps + g.cps)};
}

// wp[g4][t][k][Cop] = w[co][4 g4 + k][t] (zero past Ci / Co); TRANSPOSED (data gradient): wp[g4][t][k][Cip] = w[4 g4 + k][ci][t]
template <bool TRANSPOSED>
__global__ void k_sconv_pack(const float* __restrict__ w, float* __restrict__ wp, int Co, int Ci, int KK, int Mp, int rows) {
  const long idx = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<long>(rows) * Mp) return;
  const int m = static_cast<int>(idx % Mp), row = static_cast<int>(idx / Mp);
  const int k = row & 3, t = (row >> 2) % KK, g4 = (row >> 2) / KK, r = 4 * g4 + k;
  float v = 0.0f;
  if (!TRANSPOSED) { if (m < Co && r < Ci) v = w[(static_cast<long>(m) * Ci + r) * KK + t]; }
  else { if (m < Ci && r < Co) v = w[(static_cast<long>(r) * Ci + m) * KK + t]; }
  wp[idx] = v;
}

__global__ void k_sconv_sum(const float* __restrict__ part, float* __restrict__ y, long ybs, long per_img, long n, int S, int HWo,
                            const float* __restrict__ bias, float slope) {
  const long idx = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  float s = 0.0f;
  for (int k = 0; k < S; ++k) s += part[k * n + idx];
  const long b = idx / per_img, r = idx - b * per_img;
  if (bias) s += bias[r / HWo];
  if (slope != 1.0f) s = s > 0.0f ? s : s * slope;
  y[b * ybs + r] = s;
}

template <int K, int MT, int NT, int WM, int WN, int XSH, int NXL, int NWL>
__global__ void __launch_bounds__(256, 2)
k_sconv_fwd(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ bias, float* __restrict__ y,
            float* __restrict__ part, const ScGeo g) {
  constexpr int KK = K * K, P = K / 2, DX = (4 - P % 4) % 4, COB = 16 * MT * WM;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, kq = lane >> 4;
  const int wm = wv / WN, wn = wv % WN;
  const ScBlock bk = sc_block(g);
  const int cob0 = bk.cb * COB, img = bk.img, split = bk.split, c_beg = bk.c_beg, c_end = bk.c_end;
  const int oy0 = bk.ry * g.TH, ox0 = bk.cx * g.TW;
  const int HW = g.H * g.W, HWo = g.Ho * g.Wo;
  const int XTOT = g.CB * g.XCS;

  // ---- the lane's output pixels and operand offsets
  int boff[NT], opix[NT], aoff[MT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int p = (wn * NT + j) * 16 + i, oyl = p / g.TW, oxl = p - oyl * g.TW;
    const bool ok = oyl < g.TH && oy0 + oyl < g.Ho && ox0 + oxl < g.Wo;
    boff[j] = kq * g.XCS + (ok ? 2 * oyl * g.XRS + oxl : 0);
    opix[j] = ok ? (oy0 + oyl) * g.Wo + ox0 + oxl : -1;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) aoff[mt] = XTOT + kq * g.WRS + (wm * MT + mt) * 16 + i;

  // ---- staging: x as in the weight gradient (thread = (row, slot) position, channels 256 >> XSH apart), the filter slab by 16-byte words
  constexpr int xncg = 256 >> XSH;
  const int xpos = tid & ((1 << XSH) - 1), xcg = tid >> XSH;
  const int xr_ = xpos / g.NSLOT, xs_ = xpos - xr_ * g.NSLOT;
  const bool xact = xpos < g.RI * g.NSLOT;
  const int xl0 = xcg * g.XCS + xr_ * g.XRS + 2 * xs_;
  const int iy = 2 * oy0 - P + xr_, ix = 2 * ox0 - P - DX + 4 * xs_;
  const bool rowok = xact && iy >= 0 && iy < g.H;
  const bool full = rowok && ix >= 0 && ix + 3 < g.W;
  const bool cut = rowok && !full && ix + 3 >= 0 && ix < g.W;
  const float* xb = x + img * g.sbs;      // the loads' safe address: the sample's first words (sc_fw_plan: no x of fewer than four)
  constexpr int WQ = COB / 4;      // 16-byte words per filter row of this block
  f32x4 xr[NXL], wr[NWL];
  auto load_chunk = [&](int c) {
    load_slots(xr, xb, (c * g.CB + xcg) * HW + iy * g.W + ix, HW, xcg, xncg, min(g.CB, g.Ci - c * g.CB), ix, g.W, full, cut);
    load_slab<WQ>(wr, wp + static_cast<long>(c) * g.CB * KK * g.Mp + cob0, g.Mp, g.wl4, tid);
  };
  auto store_chunk = [&]() {
    if (xact) {
#pragma unroll
      for (int jj = 0; jj < NXL; ++jj)
        if (xcg + jj * xncg < g.CB) store_slot_split(lds + xl0 + jj * xncg * g.XCS, g.QW, xr[jj]);
    }
    store_slab<WQ>(lds + XTOT, g.WRS, wr, g.wl4, tid);
  };

  f32x4 acc[MT][NT] = {};

  if (c_beg < c_end) {
    load_chunk(c_beg);
    store_chunk();
  }
  __syncthreads();
  const int nc4 = g.CB >> 2;
  for (int c = c_beg; c < c_end; ++c) {
    const bool more = c + 1 < c_end;
    if (more) load_chunk(c + 1);
    for (int c4 = 0; c4 < nc4; ++c4)
      for (int ky = 0; ky < K; ++ky) {
        // one filter row: the operands of its K taps are all requested before the first MFMA (7 taps: four, then three -- with all
        // seven in flight the 64-channel block needs more than its 256 registers)
        const int ab = (c4 * KK + ky * K) * 4 * g.WRS, bb = c4 * 4 * g.XCS + ky * g.XRS;
        constexpr int KG = K == 7 ? 4 : K;
#pragma unroll
        for (int k0 = 0; k0 < K; k0 += KG) {
          float a[KG][MT], b[KG][NT];
#pragma unroll
          for (int kk = 0; kk < KG; ++kk) {
            const int kx = k0 + kk;
            if (kx >= K) continue;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) a[kk][mt] = lds[aoff[mt] + ab + kx * 4 * g.WRS];
#pragma unroll
            for (int j = 0; j < NT; ++j) b[kk][j] = lds[boff[j] + bb + ((kx + DX) & 1) * g.QW + ((kx + DX) >> 1)];
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int kk = 0; kk < KG; ++kk) {
            if (k0 + kk >= K) continue;
            mfma_tile(acc, a[kk], b[kk]);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    __syncthreads();
    if (more) {
      store_chunk();
      __syncthreads();
    }
  }

  // ---- epilogue: bias + activation and y, or this split's partial sums
  const bool direct = g.nsplit == 1;
  const int nimg = g.ntile / (g.cpr * g.rpi);
  float* ob = direct ? y + img * g.obs : part + (static_cast<long>(split) * nimg + img) * g.Co * HWo;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = cob0 + (wm * MT + mt) * 16 + 4 * kq + r;
      if (co >= g.Co) continue;
      const float bv = (direct && bias) ? bias[co] : 0.0f;
#pragma unroll
      for (int j = 0; j < NT; ++j)
        if (opix[j] >= 0) {
          float v = acc[mt][j][r];
          if (direct) { v += bv; v = v > 0.0f ? v : v * g.slope; }
          ob[static_cast<long>(co) * HWo + opix[j]] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Data gradient of the stride-2 convolution: gx[ci][iy][ix] = sum_(co, ky, kx) w[co][ci][ky][kx] gy[co][(iy + P - ky) / 2][(ix + P - kx) / 2]
// over the taps that divide evenly.  Input pixel (2u + py, 2v + px) only meets the taps with ky = (py + P) mod 2, kx = (px + P) mod 2:
// four stride-1 correlations of gy with sub-filters, one per PHASE (py, px).  A block owns COB input channels x a tile of (u, v)
// positions and keeps the four phases' accumulators; per group of four OUTPUT channels it reads the (2 x 2 for 3x3, 3 x 3 for 5x5)
// shifted gy operands once and every tap's filter operand once: MFMA count = the forward's, no zero-stuffed work.  The filter slab
// is k_sconv_pack<true>'s [co / 4][tap][co % 4][Ci]; gy is staged unsplit (stride 1).  1x1 (the ResNet down-sampling shortcuts,
// depth_model.py:31-36): phase (0, 0) gets w^T gy, the three others zeros.
template <int K, int MT, int NT, int WM, int WN, int XSH, int NXL, int NWL>
__global__ void __launch_bounds__(256, 2)
k_sconv_dgrad(const float* __restrict__ gy, const float* __restrict__ wp, float* __restrict__ gx, float* __restrict__ part, const ScGeo g) {
  constexpr int KK = K * K, P = K / 2, CIB = 16 * MT * WM;
  // row shift of tap ky: gy row = u + (py + P - ky) / 2 with py = (ky + P) & 1; DMIN / ND: the smallest shift, the number of shifts
  constexpr int DMIN = K == 5 ? -1 : 0, ND = K == 1 ? 1 : (K == 3 ? 2 : 3), DXA = ((DMIN % 4) + 4) % 4;
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, kq = lane >> 4;
  const int wm = wv / WN, wn = wv % WN;
  const ScBlock bk = sc_block(g);
  const int cib0 = bk.cb * CIB, img = bk.img, split = bk.split, c_beg = bk.c_beg, c_end = bk.c_end;
  const int u0 = bk.ry * g.TH, v0 = bk.cx * g.TW;
  const int gHW = g.Ho * g.Wo, HW = g.H * g.W;
  const int XTOT = g.CB * g.XCS;

  int boff[NT], pu[NT], pv[NT], aoff[MT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int p = (wn * NT + j) * 16 + i, ul = p / g.TW, vl = p - ul * g.TW;
    const bool ok = ul < g.TH;
    boff[j] = kq * g.XCS + (ok ? ul * g.XRS + vl : 0) + DXA;
    pu[j] = ok ? u0 + ul : -1; pv[j] = v0 + vl;
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) aoff[mt] = XTOT + kq * g.WRS + (wm * MT + mt) * 16 + i;

  constexpr int xncg = 256 >> XSH;
  const int xpos = tid & ((1 << XSH) - 1), xcg = tid >> XSH;
  const int xr_ = xpos / g.NSLOT, xs_ = xpos - xr_ * g.NSLOT;
  const bool xact = xpos < g.RI * g.NSLOT;
  const int xl0 = xcg * g.XCS + xr_ * g.XRS + 4 * xs_;
  const int oy = u0 + DMIN + xr_, ox = v0 + DMIN - DXA + 4 * xs_;
  const bool rowok = xact && oy >= 0 && oy < g.Ho;
  const bool full = rowok && ox >= 0 && ox + 3 < g.Wo;
  const bool cut = rowok && !full && ox + 3 >= 0 && ox < g.Wo;
  const float* gb = gy + img * g.sbs;      // the loads' safe address: the sample's first words (sc_dg_plan: no gy of fewer than four)
  constexpr int WQ = CIB / 4;
  f32x4 xr[NXL], wr[NWL];
  auto load_chunk = [&](int c) {
    load_slots(xr, gb, (c * g.CB + xcg) * gHW + oy * g.Wo + ox, gHW, xcg, xncg, min(g.CB, g.Co - c * g.CB), ox, g.Wo, full, cut);
    load_slab<WQ>(wr, wp + static_cast<long>(c) * g.CB * KK * g.Mp + cib0, g.Mp, g.wl4, tid);
  };
  auto store_chunk = [&]() {
    if (xact) {
#pragma unroll
      for (int jj = 0; jj < NXL; ++jj)
        if (xcg + jj * xncg < g.CB) *reinterpret_cast<f32x4*>(lds + xl0 + jj * xncg * g.XCS) = xr[jj];
    }
    store_slab<WQ>(lds + XTOT, g.WRS, wr, g.wl4, tid);
  };

  f32x4 acc[2][2][MT][NT] = {};

  if (c_beg < c_end) {
    load_chunk(c_beg);
    store_chunk();
  }
  __syncthreads();
  const int nc4 = g.CB >> 2;
  for (int c = c_beg; c < c_end; ++c) {
    const bool more = c + 1 < c_end;
    if (more) load_chunk(c + 1);
    for (int c4 = 0; c4 < nc4; ++c4) {
      // the shifted gy operands of this channel group, then filter row by filter row
      float b[ND][ND][NT];
      const int bb = c4 * 4 * g.XCS;
#pragma unroll
      for (int dy = 0; dy < ND; ++dy)
#pragma unroll
        for (int dx = 0; dx < ND; ++dx)
#pragma unroll
          for (int j = 0; j < NT; ++j) b[dy][dx][j] = lds[boff[j] + bb + dy * g.XRS + dx];
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int py = (ky + P) & 1, dy = (py + P - ky) / 2 - DMIN;
        float a[K][MT];
        const int ab = (c4 * KK + ky * K) * 4 * g.WRS;
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) a[kx][mt] = lds[aoff[mt] + ab + kx * 4 * g.WRS];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
          const int px = (kx + P) & 1, dx = (px + P - kx) / 2 - DMIN;
          mfma_tile(acc[py][px], a[kx], b[dy][dx]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
    if (more) {
      store_chunk();
      __syncthreads();
    }
  }

  // ---- gx (or this split's partial sums): the two column phases of a position are neighbours
  const int nimg = g.ntile / (g.cpr * g.rpi);
  float* ob = g.nsplit == 1 ? gx + img * g.obs : part + (static_cast<long>(split) * nimg + img) * g.Ci * HW;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ci = cib0 + (wm * MT + mt) * 16 + 4 * kq + r;
      if (ci >= g.Ci) continue;
      float* oc = ob + static_cast<long>(ci) * HW;
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        if (pu[j] < 0) continue;
#pragma unroll
        for (int py = 0; py < 2; ++py) {
          const int iy = 2 * pu[j] + py, ix = 2 * pv[j];
          if (iy >= g.H || ix >= g.W) continue;
          float* o = oc + iy * g.W + ix;
          o[0] = acc[py][0][mt][j][r];
          if (ix + 1 < g.W) o[1] = acc[py][1][mt][j][r];
        }
      }
    }
}

}  // namespace dfe

using namespace dfe;

namespace {
int g_sc_blocks = env_int("DFE_SCONV_BLOCKS", 0), g_sc_th = env_int("DFE_SCONV_TH", 0);

int sc_log2_ceil(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }
int sc_pad_stride(int v) { return v + ((34 - (v & 31)) & 31); }      // the next stride with stride % 32 == 2 (see the bank note below)

// the kernels by layer.  mt, nt, wm, wn: the wave tiling; flat: columns = the flattened (ci, ky, kx) index instead of one tap per
// tile; xsh / nxl, gsh / ngl: the staging shape (k_sconv_wgrad):
//   0: 3x3, Ci >= 16: one tap per tile, 16 input x 64 output channels      1: flat, 160 columns x 64 output channels (7x7 x 3)
//   2: flat, 448 columns x 16 output channels (7x7 x 9, 3x3 x 3)           3: flat, 448 columns x 32 output channels (5x5 x 16)
struct ScTile { int mt, nt, wm, wn, flat, xsh, nxl, gsh, ngl; };
const ScTile SC_TILES[4] = {{1, 9, 4, 1, 0, 7, 8, 4, 4}, {2, 5, 2, 2, 1, 8, 3, 4, 4}, {1, 7, 1, 4, 1, 8, 9, 4, 1}, {2, 7, 1, 4, 1, 8, 16, 4, 2}};

bool sc_wg_plan(int B, int Ci, int Co, int H, int W, int K, int S, int P, ScWg* out, int* cfg, int* nsplit) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0 || (S != 1 && S != 2) || P < 0 || K < 1 || K > 7) return false;
  if (static_cast<long>(Ci) * H * W < 4) return false;      // the loads' safe address: the tensors' first four words
  ScWg g = {};
  g.Ci = Ci; g.Co = Co; g.H = H; g.W = W; g.KH = K; g.KW = K; g.S = S; g.D = 1; g.P = P;
  g.Ho = (H + 2 * P - K) / S + 1; g.Wo = (W + 2 * P - K) / S + 1;
  if (g.Ho < 1 || g.Wo < 1 || static_cast<long>(Co) * g.Ho * g.Wo < 4) return false;
  const int KK = K * K;
  int c = -1;
  if (K == 3 && Ci >= 16) c = 0;      // (a 128-output-channel block, 18 accumulators per wave, measured no faster: 124 / 118 / 125 us against 108 / 103 / 118)
  else if (Ci * KK <= 160 && Co > 32) c = 1;
  else if (Ci * KK <= 448 && Co <= 16 && Ci <= 9) c = 2;
  else if (Ci * KK <= 448 && Co <= 32 && Ci <= 16) c = 3;
  else if (Ci * KK <= 160) c = 1;
  if (c < 0) return false;
  const ScTile t = SC_TILES[c];
  g.flat = t.flat;
  g.COB = 16 * t.mt * t.wm;
  const int cols = 16 * t.nt * t.wn;
  g.CIB = t.flat ? std::min(Ci, cols / KK) : 16 * (t.nt * t.wn / KK);
  const int xncg = 256 >> t.xsh, gncg = 256 >> t.gsh;
  if (g.CIB < 1 || g.CIB > t.nxl * xncg || g.COB > t.ngl * gncg) return false;
  g.XCH = t.nxl * xncg; g.GCH = t.ngl * gncg;
  // the staged window starts on a multiple of four columns (16-byte loads that the image's edge never cuts when W % 4 == 0):
  // DX columns left of the first tap's.  A chunk's first output column is a multiple of TW, TW of 4: DX is the same for all.
  g.DX = ((-P) % 4 + 4) % 4;
  // the chunk: TW output columns (a multiple of 4, at most 64, the row cut into equal parts), TH rows: the most the thread
  // groups' positions hold
  const int wo4 = (g.Wo + 3) / 4 * 4, parts = (wo4 + 63) / 64;
  g.TW = ((g.Wo + parts - 1) / parts + 3) / 4 * 4;
  bool found = false;
  for (int th = 8; th >= 1 && !found; th >>= 1) {
    if (th > 1 && (th * g.TW > 128 || th > g.Ho)) continue;
    if (g_sc_th > 0 && th > g_sc_th) continue;
    g.TH = th;
    g.RI = S * (th - 1) + (K - 1) + 1;
    const int ciw = S * (g.TW - 1) + (K - 1) + 1 + g.DX;
    g.NSLOT = (ciw + 3) / 4;
    if (g.RI * g.NSLOT > (1 << t.xsh) || th * (g.TW / 4) > (1 << t.gsh)) continue;
    g.QW = 2 * g.NSLOT;
    g.XRS = S == 2 ? 2 * g.QW : 4 * g.NSLOT;
    // channel strides % 32 == 2: the lanes of a 16-lane tile differ in the channel (and the four lane groups by one word each):
    // a 32-lane pass of a dword read covers 32 different banks
    g.XCS = sc_pad_stride(g.RI * g.XRS);
    g.GCS = sc_pad_stride(th * g.TW);
    if (sizeof(float) * (static_cast<size_t>(g.XCH) * g.XCS + static_cast<size_t>(g.GCH) * g.GCS + 16) > 76 * 1024) continue;
    found = true;
  }
  if (!found) return false;
  g.cpr = (g.Wo + g.TW - 1) / g.TW; g.rpi = (g.Ho + g.TH - 1) / g.TH;
  const long nch = static_cast<long>(B) * g.cpr * g.rpi;
  if (nch >= (1L << 30)) return false;
  g.nchunks = static_cast<int>(nch);
  const int ncot = (Co + g.COB - 1) / g.COB;
  g.ncit = (Ci + g.CIB - 1) / g.CIB;
  g.ntb = ncot * g.ncit;
  // one resident round of blocks: three per CU for the kernels that fit three waves per SIMD (configurations 1 and 2), else two
  *nsplit = split_round(g_sc_blocks > 0 ? g_sc_blocks : ((c == 1 || c == 2) ? 768 : 512), g.ntb, g.nchunks, &g.cps);
  *out = g; *cfg = c;
  return true;
}
}  // namespace

extern "C" int dfe_sconv_tune(int blocks, int rows) {
  if (blocks >= 0) g_sc_blocks = blocks;
  if (rows >= 0) g_sc_th = rows;
  return DFE_OK;
}

extern "C" long dfe_sconv_wgrad_floats(int B, int Ci, int Co, int H, int W, int K, int stride, int P) {
  ScWg g; int cfg, ns;
  if (!sc_wg_plan(B, Ci, Co, H, W, K, stride, P, &g, &cfg, &ns)) return 0;
  return static_cast<long>(ns) * Co * Ci * K * K;
}

extern "C" int dfe_sconv_wgrad(const float* x, long x_batch_stride, const float* gy, long gy_batch_stride, float* gweight, float* ws, int B,
                               int Ci, int Co, int H, int W, int K, int stride, int P, void* stream) {
  if (!x || !gy || !gweight || !ws) return DFE_ERR_NULL;
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return DFE_ERR_DIMS;
  ScWg g; int cfg, ns;
  if (!sc_wg_plan(B, Ci, Co, H, W, K, stride, P, &g, &cfg, &ns)) return DFE_ERR_UNSUPPORTED;
  const long n = static_cast<long>(Co) * Ci * K * K;
  if (!sample_ok(x_batch_stride, static_cast<long>(Ci) * H * W) || !sample_ok(gy_batch_stride, static_cast<long>(Co) * g.Ho * g.Wo) || n >= (1L << 30)) return DFE_ERR_DIMS;
  g.xbs = x_batch_stride; g.gbs = gy_batch_stride;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned grid = static_cast<unsigned>(g.ntb) * ns;
  const size_t lds_bytes = sizeof(float) * (static_cast<size_t>(g.XCH) * g.XCS + static_cast<size_t>(g.GCH) * g.GCS + 16);
#define SC_WG(...) launch_dyn_lds<k_sconv_wgrad<__VA_ARGS__>>(grid, lds_bytes, 80 * 1024, st, x, gy, ws, g)
  switch (cfg) {
    case 0: SC_WG(1, 9, 4, 1, 7, 8, 4, 4); break;
    case 1: SC_WG(2, 5, 2, 2, 8, 3, 4, 4); break;
    case 2: SC_WG(1, 7, 1, 4, 8, 9, 4, 1); break;
    default: SC_WG(2, 7, 1, 4, 8, 16, 4, 2); break;
  }
#undef SC_WG
  DFE_LAUNCH_CHECK();
  launch_wgrad_sum(ws, gweight, ns, n, st);
  DFE_LAUNCH_CHECK();
  return DFE_OK;
}

// ---- forward and data gradient, host side
namespace {
int sc_pad16(int v) { return v + ((48 - (v & 31)) & 31); }      // the next stride with stride % 32 == 16

// The pixel tile and the channel split of the forward and of the data gradient.  The block's tile is TH x TW of the rows x cols
// grid it walks (TW a multiple of 4 / S: the staged window starts on a multiple of four columns), at most npix positions, whose
// staged window -- S (TH - 1) + ext rows, S (TW - 1) + ext + dx columns -- fits maxpos staging positions and lds_kb of LDS with
// the filter slab; the most useful positions per tile.  Before: Ci ... Wo, CB, WRS and ncb of *g.
bool sc_tile_plan(ScGeo* g, int B, int KK, int rows, int cols, int npix, int S, int ext, int dx, int maxpos, int lds_kb) {
  const int step = 4 / S;
  double best = 0.0;
  for (int tw = std::min(64, (cols + step - 1) / step * step); tw >= step; tw -= step) {
    const int th = std::min(npix / tw, rows);
    if (th < 1) continue;
    const int ri = S * (th - 1) + ext, nslot = (S * (tw - 1) + ext + dx + 3) / 4;
    if (ri * nslot > maxpos) continue;
    const int xrs = 4 * nslot, xcs = sc_pad16(ri * xrs);
    if (sizeof(float) * (static_cast<size_t>(g->CB) * xcs + static_cast<size_t>(g->CB) * KK * g->WRS + 64) > static_cast<size_t>(lds_kb) * 1024) continue;
    const int cpr = (cols + tw - 1) / tw, rpi = (rows + th - 1) / th;
    const double eff = static_cast<double>(rows) * cols / (static_cast<double>(cpr) * rpi * npix);
    if (eff > best + 1e-9) { best = eff; g->TW = tw; g->TH = th; g->RI = ri; g->NSLOT = nslot; g->QW = 2 * nslot; g->XRS = xrs; g->XCS = xcs; g->cpr = cpr; g->rpi = rpi; }
  }
  if (best == 0.0) return false;
  const long nt = static_cast<long>(B) * g->cpr * g->rpi, blocks = nt * g->ncb;
  if (blocks >= (1L << 24)) return false;
  g->ntile = static_cast<int>(nt);
  // thin layers: the channel chunks are split over blocks until there are two blocks per CU
  const long sp = blocks >= 384 ? 1 : std::min<long>(g->nck, (512 + blocks - 1) / blocks);
  g->cps = static_cast<int>((g->nck + sp - 1) / sp);
  g->nsplit = (g->nck + g->cps - 1) / g->cps;
  return true;
}

// what both passes derive from the layer alone; *t32: the written tensor gets 32-channel blocks (else 64)
bool sc_geo_init(ScGeo* g, int B, int Ci, int Co, int H, int W, int K, bool dgrad, int* t32) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return false;
  const int P = K / 2;
  *g = ScGeo{};
  g->Ci = Ci; g->Co = Co; g->H = H; g->W = W;
  g->Ho = (H + 2 * P - K) / 2 + 1; g->Wo = (W + 2 * P - K) / 2 + 1;
  // the loads' safe address: the staged tensor's first four words
  if (g->Ho < 1 || g->Wo < 1 || (dgrad ? static_cast<long>(Co) * g->Ho * g->Wo : static_cast<long>(Ci) * H * W) < 4) return false;
  const int staged = dgrad ? Co : Ci, written = dgrad ? Ci : Co, sp4 = (staged + 3) / 4 * 4;
  *t32 = written <= 32;
  const int blk = *t32 ? 32 : 64;
  g->CB = dgrad ? std::min(K == 5 ? 8 : 16, sp4) : (K == 3 ? std::min(8, sp4) : 4);
  g->nck = (sp4 + g->CB - 1) / g->CB;
  g->Mp = (written + 63) / 64 * 64;
  g->WRS = blk + 16;
  g->wl4 = g->CB * K * K * blk / 4;
  g->ncb = (written + blk - 1) / blk;
  return true;
}

bool sc_fw_plan(int B, int Ci, int Co, int H, int W, int K, ScGeo* g, int* t32) {
  if ((K != 3 && K != 5 && K != 7) || !sc_geo_init(g, B, Ci, Co, H, W, K, false, t32)) return false;
  const int P = K / 2;
  return sc_tile_plan(g, B, K * K, g->Ho, g->Wo, 128, 2, K, (4 - P % 4) % 4, 256, 80);
}

// the data gradient walks the positions (u, v) of the half-resolution grid whose phases the block writes: ceil(H / 2) x ceil(W / 2)
bool sc_dg_plan(int B, int Ci, int Co, int H, int W, int K, ScGeo* g, int* t32) {
  if ((K != 1 && K != 3 && K != 5) || !sc_geo_init(g, B, Ci, Co, H, W, K, true, t32)) return false;
  const int dmin = K == 5 ? -1 : 0, nd = K == 1 ? 1 : (K == 3 ? 2 : 3), dxa = ((dmin % 4) + 4) % 4;
  return sc_tile_plan(g, B, K * K, (H + 1) / 2, (W + 1) / 2, *t32 ? 128 : 64, 1, nd, dxa, 64, 76);
}

long sc_packed_floats(const ScGeo& g, int K) { return static_cast<long>(g.nck) * g.CB * K * K * g.Mp + 64; }
size_t sc_lds_bytes(const ScGeo& g, int K) { return sizeof(float) * (static_cast<size_t>(g.CB) * g.XCS + static_cast<size_t>(g.CB) * K * K * g.WRS + 64); }
}  // namespace

extern "C" long dfe_sconv_fwd_floats(int B, int Ci, int Co, int H, int W, int K) {
  ScGeo g; int t32;
  if (!sc_fw_plan(B, Ci, Co, H, W, K, &g, &t32)) return 0;
  return sc_packed_floats(g, K) + (g.nsplit > 1 ? static_cast<long>(g.nsplit) * B * Co * g.Ho * g.Wo : 0);
}

extern "C" int dfe_sconv_fwd(const float* x, long x_batch_stride, const float* weight, const float* bias, float slope, float* y,
                             long y_batch_stride, float* ws, int B, int Ci, int Co, int H, int W, int K, void* stream) {
  if (!x || !weight || !y || !ws) return DFE_ERR_NULL;
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return DFE_ERR_DIMS;
  ScGeo g; int t32;
  if (!sc_fw_plan(B, Ci, Co, H, W, K, &g, &t32)) return DFE_ERR_UNSUPPORTED;
  const long oplane = static_cast<long>(g.Ho) * g.Wo;
  if (!sample_ok(x_batch_stride, static_cast<long>(Ci) * H * W) || !sample_ok(y_batch_stride, Co * oplane)) return DFE_ERR_DIMS;
  if (!aligned16(ws)) return DFE_ERR_UNSUPPORTED;      // the packed filter is read with 16-byte loads
  g.sbs = x_batch_stride; g.obs = y_batch_stride; g.slope = slope;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rows = g.nck * g.CB * K * K;
  const long npk = static_cast<long>(rows) * g.Mp;
  k_sconv_pack<false><<<static_cast<unsigned>((npk + 255) / 256), 256, 0, st>>>(weight, ws, Co, Ci, K * K, g.Mp, rows);
  DFE_LAUNCH_CHECK();
  float* part = ws + sc_packed_floats(g, K);
  const unsigned grid = static_cast<unsigned>(g.ntile) * g.ncb * g.nsplit;
#define SC_FW(...) launch_dyn_lds<k_sconv_fwd<__VA_ARGS__>>(grid, sc_lds_bytes(g, K), 80 * 1024, st, x, ws, bias, y, part, g)
  if (K == 3 && !t32) SC_FW(3, 2, 4, 2, 2, 8, 8, 5);
  else if (K == 3) SC_FW(3, 2, 2, 1, 4, 8, 8, 3);
  else if (K == 5 && !t32) SC_FW(5, 2, 4, 2, 2, 8, 4, 7);
  else if (K == 5) SC_FW(5, 2, 2, 1, 4, 8, 4, 4);
  else if (!t32) SC_FW(7, 2, 4, 2, 2, 8, 4, 13);
  else SC_FW(7, 2, 2, 1, 4, 8, 4, 7);
#undef SC_FW
  DFE_LAUNCH_CHECK();
  if (g.nsplit > 1) {
    const long per_img = Co * oplane, n = per_img * B;
    k_sconv_sum<<<static_cast<unsigned>((n + 255) / 256), 256, 0, st>>>(part, y, y_batch_stride, per_img, n, g.nsplit, static_cast<int>(oplane), bias, slope);
    DFE_LAUNCH_CHECK();
  }
  return DFE_OK;
}

extern "C" long dfe_sconv_dgrad_floats(int B, int Ci, int Co, int H, int W, int K) {
  ScGeo g; int t32;
  if (!sc_dg_plan(B, Ci, Co, H, W, K, &g, &t32)) return 0;
  return sc_packed_floats(g, K) + (g.nsplit > 1 ? static_cast<long>(g.nsplit) * B * Ci * H * W : 0);
}

extern "C" int dfe_sconv_dgrad(const float* gy, long gy_batch_stride, const float* weight, float* gx, long gx_batch_stride, float* ws, int B,
                               int Ci, int Co, int H, int W, int K, void* stream) {
  if (!gy || !weight || !gx || !ws) return DFE_ERR_NULL;
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return DFE_ERR_DIMS;
  ScGeo g; int t32;
  if (!sc_dg_plan(B, Ci, Co, H, W, K, &g, &t32)) return DFE_ERR_UNSUPPORTED;
  const long oplane = static_cast<long>(g.Ho) * g.Wo, iplane = static_cast<long>(H) * W;
  if (!sample_ok(gx_batch_stride, Ci * iplane) || !sample_ok(gy_batch_stride, Co * oplane)) return DFE_ERR_DIMS;
  if (!aligned16(ws)) return DFE_ERR_UNSUPPORTED;      // the packed filter is read with 16-byte loads
  g.sbs = gy_batch_stride; g.obs = gx_batch_stride;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rows = g.nck * g.CB * K * K;
  const long npk = static_cast<long>(rows) * g.Mp;
  k_sconv_pack<true><<<static_cast<unsigned>((npk + 255) / 256), 256, 0, st>>>(weight, ws, Co, Ci, K * K, g.Mp, rows);
  DFE_LAUNCH_CHECK();
  float* part = ws + sc_packed_floats(g, K);
  const unsigned grid = static_cast<unsigned>(g.ntile) * g.ncb * g.nsplit;
#define SC_DG(...) launch_dyn_lds<k_sconv_dgrad<__VA_ARGS__>>(grid, sc_lds_bytes(g, K), 80 * 1024, st, gy, ws, gx, part, g)
  if (K == 3 && !t32) SC_DG(3, 2, 2, 2, 2, 6, 4, 9);
  else if (K == 3) SC_DG(3, 2, 2, 1, 4, 6, 4, 5);
  else if (K == 5 && !t32) SC_DG(5, 2, 2, 2, 2, 6, 2, 13);
  else if (K == 5) SC_DG(5, 2, 2, 1, 4, 6, 2, 7);
  else if (!t32) SC_DG(1, 2, 2, 2, 2, 6, 4, 1);
  else SC_DG(1, 2, 2, 1, 4, 6, 4, 1);
#undef SC_DG
  DFE_LAUNCH_CHECK();
  if (g.nsplit > 1) {
    const long per_img = Ci * iplane, n = per_img * B;
    k_sconv_sum<<<static_cast<unsigned>((n + 255) / 256), 256, 0, st>>>(part, gx, gx_batch_stride, per_img, n, g.nsplit, static_cast<int>(iplane), nullptr, 1.0f);
    DFE_LAUNCH_CHECK();
  }
  return DFE_OK;
}
