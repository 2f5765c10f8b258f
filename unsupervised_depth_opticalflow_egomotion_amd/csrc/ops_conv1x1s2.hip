// The 1x1 STRIDE-2 convolutions (the ResNet18 encoder's down-sampling shortcuts depth_model.py:31-36: 64 -> 128, 128 -> 256,
// 256 -> 512, no bias, a BatchNorm follows) on the fp32 matrix cores, straight from NCHW, for the deterministic mode
// (convs.set_deterministic): every sum below has one fixed order, whatever the allocator or the timing does.
//   forward  y[b][co][oy][ox] = sum_ci w[co][ci] x[b][ci][2 oy][2 ox]: a GEMM (co) x (pixels of the whole batch) reduced over ci;
//   weight gradient  gW[co][ci] = sum_(b, oy, ox) gy[b][co][oy][ox] x[b][ci][2 oy][2 ox]: a GEMM (co) x (ci) reduced over the pixels,
//            the pixel range split over one resident round of blocks, the partials [split][co][ci] added in split order by
//            k_wgrad_sum (no atomics).
// (The data gradient is dfe_sconv_dgrad with K = 1.)  v_mfma_f32_16x16x4_f32: A[row = lane & 15][k = lane >> 4], B[k = lane >> 4]
// [col = lane & 15], D[row = 4 (lane >> 4) + r][col = lane & 15].  Only the even rows and columns of x are ever addressed: a
// quarter of its lines.  Every global access is predicated on its own index: no safe addresses, views of any size.
// Bound: the stride-2 reads of x (half of every 64-byte line fetched is used), not the matrix pipe (<= 0.7 GFLOP per layer).
#include "dfe_internal.h"
#include "dfe_device.h"
#include "dfe_mfma_stage.h"
#include "dfe_wgrad_sum.h"
#include <hip/hip_runtime.h>
#include <algorithm>

namespace dfe {

constexpr int C1_T = 64;        // a block's output channels, and its pixels (forward) / input channels (weight gradient): 2 x 2 waves of 2 x 2 tiles
constexpr int C1_KC = 16;       // forward: input channels per staged chunk
constexpr int C1_XS = 80;       // forward: LDS stride of a staged channel of x, % 32 == 16: lanes = 16 pixels x 2 channels per pass, 32 banks
constexpr int C1_WS = 18;       // forward: LDS stride of a filter row [co][ci], % 32 == 2: lanes = 16 rows x 2 channels per pass
constexpr int C1_PK = 32;       // weight gradient: pixels per staged chunk
constexpr int C1_PS = 34;       // weight gradient: LDS stride of a staged channel [channel][pixel], % 32 == 2

struct C1Geo {
  long xbs, obs;                // batch strides of x and of y / gy, in floats
  int Ci, Co, H, W, Wo, HWo, N; // N = B Ho Wo: the pixels of the whole batch, numbered (b, oy, ox)
  int ncot, ncit, ntb;          // blocks over the output / input channels
  int nchunks, cps;             // weight gradient: pixel chunks, chunks per split
};

// amdgpu_waves_per_eu(2), here and below: with no blocks per CU named the compiler plans for one wave per SIMD and keeps the MFMA
// accumulators in AGPRs (76 + 24 registers here, 104 + 20 in the weight gradient); held to the 256 VGPRs of two waves it needs 53 / 86
// and no AGPR (tests/test_api_cpu.py holds both to that)
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
k_conv1x1s2_fwd(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, const C1Geo g) {
  __shared__ float xs[C1_KC * C1_XS];
  __shared__ float wl[C1_T * C1_WS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, kq = lane >> 4;
  const int wm = wv >> 1, wn = wv & 1;
  // the output-channel block fastest: the blocks that read the same pixels of x are neighbours
  const int co0 = static_cast<int>(blockIdx.x % static_cast<unsigned>(g.ncot)) * C1_T;
  const int n0 = static_cast<int>(blockIdx.x / static_cast<unsigned>(g.ncot)) * C1_T;
  const int HW = g.H * g.W;

  // staging: x by (pixel, channel group of 4 channels 4 apart), the filter by (channel, row group of 4 rows 16 apart)
  const int px = tid & 63, cg = tid >> 6;
  const int n = n0 + px;
  const bool pok = n < g.N;
  const int b = pok ? n / g.HWo : 0, p = pok ? n - b * g.HWo : 0, oy = p / g.Wo, ox = p - oy * g.Wo;
  const float* xp = x + b * g.xbs + 2 * oy * g.W + 2 * ox;
  const int wci = tid & 15, wro = tid >> 4;
  float xr[4], wr[4];
  auto load_chunk = [&](int c0) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int ci = c0 + cg + 4 * jj;
      xr[jj] = (pok && ci < g.Ci) ? xp[static_cast<long>(ci) * HW] : 0.0f;
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int co = co0 + wro + 16 * jj, ci = c0 + wci;
      wr[jj] = (co < g.Co && ci < g.Ci) ? w[static_cast<long>(co) * g.Ci + ci] : 0.0f;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) xs[(cg + 4 * jj) * C1_XS + px] = xr[jj];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) wl[(wro + 16 * jj) * C1_WS + wci] = wr[jj];
  };

  f32x4 acc[2][2] = {};

  load_chunk(0);
  store_chunk();
  __syncthreads();
  for (int c0 = 0; c0 < g.Ci; c0 += C1_KC) {
    const bool more = c0 + C1_KC < g.Ci;
    if (more) load_chunk(c0 + C1_KC);
#pragma unroll
    for (int k4 = 0; k4 < C1_KC / 4; ++k4) {
      float a[2], bv[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) a[mt] = wl[((wm * 2 + mt) * 16 + i) * C1_WS + 4 * k4 + kq];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) bv[nt] = xs[(4 * k4 + kq) * C1_XS + (wn * 2 + nt) * 16 + i];
      mfma_tile(acc, a, bv);
    }
    __syncthreads();
    if (more) {
      store_chunk();
      __syncthreads();
    }
  }

#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int no = n0 + (wn * 2 + nt) * 16 + i;
    if (no >= g.N) continue;
    const int bo = no / g.HWo, po = no - bo * g.HWo;
    float* yo = y + bo * g.obs + po;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + (wm * 2 + mt) * 16 + 4 * kq + r;
        if (co < g.Co) yo[static_cast<long>(co) * g.HWo] = acc[mt][nt][r];
      }
  }
}

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
k_conv1x1s2_wgrad(const float* __restrict__ x, const float* __restrict__ gy, float* __restrict__ part, const C1Geo g) {
  __shared__ float gs[C1_T * C1_PS];
  __shared__ float xs[C1_T * C1_PS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 15, kq = lane >> 4;
  const int wm = wv >> 1, wn = wv & 1;
  const int tb = static_cast<int>(blockIdx.x % static_cast<unsigned>(g.ntb)), split = static_cast<int>(blockIdx.x / static_cast<unsigned>(g.ntb));
  const int co0 = (tb / g.ncit) * C1_T, ci0 = (tb % g.ncit) * C1_T;
  const int c_beg = split * g.cps, c_end = min(g.nchunks, c_beg + g.cps);
  const int HW = g.H * g.W;

  // staging: thread = (pixel of the chunk, channel group: 8 channels 8 apart), gy and x alike
  const int pl = tid & 31, ch = tid >> 5;
  float gr[8], xr[8];
  auto load_chunk = [&](int c) {
    const int n = c * C1_PK + pl;
    const bool pok = n < g.N;
    const int b = pok ? n / g.HWo : 0, p = pok ? n - b * g.HWo : 0, oy = p / g.Wo, ox = p - oy * g.Wo;
    const float* gp = gy + b * g.obs + p;
    const float* xp = x + b * g.xbs + 2 * oy * g.W + 2 * ox;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int co = co0 + ch + 8 * jj, ci = ci0 + ch + 8 * jj;
      gr[jj] = (pok && co < g.Co) ? gp[static_cast<long>(co) * g.HWo] : 0.0f;
      xr[jj] = (pok && ci < g.Ci) ? xp[static_cast<long>(ci) * HW] : 0.0f;
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      gs[(ch + 8 * jj) * C1_PS + pl] = gr[jj];
      xs[(ch + 8 * jj) * C1_PS + pl] = xr[jj];
    }
  };

  f32x4 acc[2][2] = {};

  if (c_beg < c_end) {
    load_chunk(c_beg);
    store_chunk();
  }
  __syncthreads();
  for (int c = c_beg; c < c_end; ++c) {
    const bool more = c + 1 < c_end;
    if (more) load_chunk(c + 1);
#pragma unroll
    for (int k4 = 0; k4 < C1_PK / 4; ++k4) {
      float a[2], bv[2];
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) a[mt] = gs[((wm * 2 + mt) * 16 + i) * C1_PS + 4 * k4 + kq];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) bv[nt] = xs[((wn * 2 + nt) * 16 + i) * C1_PS + 4 * k4 + kq];
      mfma_tile(acc, a, bv);
    }
    __syncthreads();
    if (more) {
      store_chunk();
      __syncthreads();
    }
  }

  // this split's partial sums [co][ci]
  float* po = part + static_cast<long>(split) * g.Co * g.Ci;
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int ci = ci0 + (wn * 2 + nt) * 16 + i;
    if (ci >= g.Ci) continue;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = co0 + (wm * 2 + mt) * 16 + 4 * kq + r;
        if (co < g.Co) po[static_cast<long>(co) * g.Ci + ci] = acc[mt][nt][r];
      }
  }
}

}  // namespace dfe

using namespace dfe;

namespace {
// shape logic only (no device): the layers both kernels take, and the weight gradient's split of the pixel range
bool c1_plan(int B, int Ci, int Co, int H, int W, C1Geo* out, int* nsplit) {
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return false;
  C1Geo g = {};
  g.Ci = Ci; g.Co = Co; g.H = H; g.W = W;
  const int Ho = (H - 1) / 2 + 1;
  g.Wo = (W - 1) / 2 + 1;
  const long hwo = static_cast<long>(Ho) * g.Wo, n = hwo * B;
  // 32-bit pixel and element numbers inside a sample, and a grid that fits
  if (n >= (1L << 30) || static_cast<long>(Ci) * H * W >= (1L << 30) || Co * hwo >= (1L << 30) || static_cast<long>(Co) * Ci >= (1L << 30)) return false;
  g.HWo = static_cast<int>(hwo); g.N = static_cast<int>(n);
  g.ncot = (Co + C1_T - 1) / C1_T; g.ncit = (Ci + C1_T - 1) / C1_T;
  g.ntb = g.ncot * g.ncit;
  if (static_cast<long>(g.ncot) * ((n + C1_T - 1) / C1_T) >= (1L << 30) || g.ntb >= (1 << 20)) return false;
  g.nchunks = (g.N + C1_PK - 1) / C1_PK;
  *nsplit = split_round(512, g.ntb, g.nchunks, &g.cps);      // one resident round of blocks (two per CU)
  *out = g;
  return true;
}
}  // namespace

extern "C" int dfe_conv1x1s2_supported(int B, int Ci, int Co, int H, int W) {
  C1Geo g; int ns;
  return c1_plan(B, Ci, Co, H, W, &g, &ns) ? 1 : 0;
}

extern "C" int dfe_conv1x1s2_fwd(const float* x, long x_batch_stride, const float* weight, float* y, long y_batch_stride, int B, int Ci,
                                 int Co, int H, int W, void* stream) {
  if (!x || !weight || !y) return DFE_ERR_NULL;
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return DFE_ERR_DIMS;
  C1Geo g; int ns;
  if (!c1_plan(B, Ci, Co, H, W, &g, &ns)) return DFE_ERR_UNSUPPORTED;
  if (!sample_ok(x_batch_stride, static_cast<long>(Ci) * H * W) || !sample_ok(y_batch_stride, static_cast<long>(Co) * g.HWo)) return DFE_ERR_DIMS;
  g.xbs = x_batch_stride; g.obs = y_batch_stride;
  const unsigned blocks = static_cast<unsigned>(g.ncot) * static_cast<unsigned>((g.N + C1_T - 1) / C1_T);
  k_conv1x1s2_fwd<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(x, weight, y, g);
  DFE_LAUNCH_CHECK();
  return DFE_OK;
}

extern "C" long dfe_conv1x1s2_wgrad_floats(int B, int Ci, int Co, int H, int W) {
  C1Geo g; int ns;
  if (!c1_plan(B, Ci, Co, H, W, &g, &ns)) return 0;
  return static_cast<long>(ns) * Co * Ci;
}

extern "C" int dfe_conv1x1s2_wgrad(const float* x, long x_batch_stride, const float* gy, long gy_batch_stride, float* gweight, float* ws,
                                   int B, int Ci, int Co, int H, int W, void* stream) {
  if (!x || !gy || !gweight || !ws) return DFE_ERR_NULL;
  if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return DFE_ERR_DIMS;
  C1Geo g; int ns;
  if (!c1_plan(B, Ci, Co, H, W, &g, &ns)) return DFE_ERR_UNSUPPORTED;
  if (!sample_ok(x_batch_stride, static_cast<long>(Ci) * H * W) || !sample_ok(gy_batch_stride, static_cast<long>(Co) * g.HWo)) return DFE_ERR_DIMS;
  g.xbs = x_batch_stride; g.obs = gy_batch_stride;
  hipStream_t st = static_cast<hipStream_t>(stream);
  k_conv1x1s2_wgrad<<<static_cast<unsigned>(g.ntb) * ns, 256, 0, st>>>(x, gy, ws, g);
  DFE_LAUNCH_CHECK();
  launch_wgrad_sum(ws, gweight, ns, static_cast<long>(Co) * Ci, st);
  DFE_LAUNCH_CHECK();
  return DFE_OK;
}
