// The eight-point epipolar map (model_geometry.py:318-353, call site :831-835): the dense distance of every pixel's match
// (x + u, y + v) to its epipolar line under a GIVEN fundamental matrix -- the robust F of the step's sampled matches
// (dfe_fundamental_ransac), not the pose's K^-T [t]x R K^-1 --, its plain mean over a plane (compute_epipolar_loss, :413-418)
// and that mean's gradient to the flow.  Plane p = d*B + b (d = 0: target -> left from flow_bwd, 1: target -> right from
// flow_fwd), the order F32 of dfe_fundamental_ransac has.  F is a constant (the reference builds it from numpy).
//
//   k_epi_map        dist of every pixel of a plane
//   k_epi_loss_part  per block the double sum of its pixels' dist -> ws[plane][block]
//   k_epi_loss_fin   one block per sample: the partials of its two planes in block order -> loss[b]
//   k_epi_bwd        gloss[b] / (H*W) * sgn(s) * (l0, l1) / div to both flow planes, l, s and div recomputed
// Grid (blocks per plane, planes).  A thread owns EPI_ITERS quads of four consecutive pixels.  Where the plane size is a
// multiple of four and every pointer is on 16 bytes a quad moves as one 16-byte access per flow plane (VEC); otherwise as up
// to four element accesses.  The pixel -> thread assignment and the arithmetic are the same on both paths, so are the bits.
// The pass is bound by memory (two flow planes in, one or two planes out), hence the correctly rounded sqrtf and division:
// the map feeds mask decisions (get_rigid_mask).
// No float atomics, no arrival ticket: every sum is in double in an order fixed by plane, block and thread index; the same
// bits run after run.  Every loop is bounded by the shape; a non-finite F or flow only makes that plane's values non-finite.
#include "dfe_internal.h"

namespace dfe {
namespace {

constexpr int EPI_THREADS = 256;
constexpr int EPI_ITERS = 2;                                    // quads per thread
constexpr int EPI_BLOCK_PIX = EPI_THREADS * EPI_ITERS * 4;      // pixels per block
constexpr int EPI_WAVES = EPI_THREADS / 64;

inline int epi_blocks(long HW) { return static_cast<int>((HW + EPI_BLOCK_PIX - 1) / EPI_BLOCK_PIX); }

// The one statement of the expression.  l = F (x, y, 1)^T in the large-bmm order the fused stack uses for its own epipolar
// term (loss_stack_fwd.hip:444-447: fma(F1, y, F0 * x) + F2), s = p2 . l summed left to right, div as the reference writes it.
struct EpiPoint {
  float l0, l1, s, div;
  __device__ __forceinline__ float dist() const { return fabsf(s) / div; }
};

__device__ __forceinline__ EpiPoint epi_point(const float* F, float x, float y, float u, float v) {
  EpiPoint p;
  p.l0 = __fmaf_rn(F[1], y, F[0] * x) + F[2];
  p.l1 = __fmaf_rn(F[4], y, F[3] * x) + F[5];
  const float l2 = __fmaf_rn(F[7], y, F[6] * x) + F[8];
  p.s = ((x + u) * p.l0 + (y + v) * p.l1) + l2;
  p.div = sqrtf(p.l0 * p.l0 + p.l1 * p.l1) + 1e-6f;
  return p;
}

// four consecutive pixels i0 .. i0 + n - 1 of a plane: flows and integer coordinates
struct EpiQuad {
  float u[4], v[4], x[4], y[4];
  int i0, n;       // n = 0: the quad lies beyond the plane
};

template <bool VEC>
__device__ __forceinline__ EpiQuad epi_load(const float* __restrict__ pu, const float* __restrict__ pv, int HW, int W, int it) {
  EpiQuad q = {};
  const long i0 = (static_cast<long>(blockIdx.x) * EPI_ITERS + it) * (EPI_THREADS * 4) + threadIdx.x * 4;
  q.n = i0 >= HW ? 0 : (HW - i0 < 4 ? static_cast<int>(HW - i0) : 4);
  q.i0 = q.n ? static_cast<int>(i0) : 0;
  if (VEC) {               // HW % 4 == 0: a quad inside the plane is whole
    if (q.n) {
      const float4 a = *reinterpret_cast<const float4*>(pu + q.i0), b = *reinterpret_cast<const float4*>(pv + q.i0);
      q.u[0] = a.x; q.u[1] = a.y; q.u[2] = a.z; q.u[3] = a.w;
      q.v[0] = b.x; q.v[1] = b.y; q.v[2] = b.z; q.v[3] = b.w;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < q.n) { q.u[e] = pu[q.i0 + e]; q.v[e] = pv[q.i0 + e]; }
  }
  int yi = q.i0 / W, xi = q.i0 - yi * W;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    q.x[e] = static_cast<float>(xi); q.y[e] = static_cast<float>(yi);
    if (++xi == W) { xi = 0; ++yi; }
  }
  return q;
}

template <bool VEC>
__device__ __forceinline__ void epi_store(float* __restrict__ p, const EpiQuad& q, const float* o) {
  if (VEC) {
    if (q.n) *reinterpret_cast<float4*>(p + q.i0) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < q.n) p[q.i0 + e] = o[e];
  }
}

// the flow planes of plane p: planes below `split` come from fa (sample p), the others from fb (sample p - split)
__device__ __forceinline__ const float* epi_flow(const float* fa, const float* fb, int split, int p, long HW) {
  return p < split ? fa + 2 * HW * p : fb + 2 * HW * (p - split);
}

__device__ __forceinline__ void epi_F(const float* __restrict__ F32, int p, float* F) {
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = F32[static_cast<long>(p) * 9 + i];
}

// sum over the block in a fixed order: lanes by a shuffle tree, waves in index order; valid in thread 0
__device__ __forceinline__ double epi_block_sum(double v, double* sW) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) sW[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < EPI_WAVES; ++w) t += sW[w];
  }
  __syncthreads();
  return t;
}

template <bool VEC>
__global__ void __launch_bounds__(EPI_THREADS) k_epi_map(const float* __restrict__ flow, const float* __restrict__ F32,
                                                          float* __restrict__ dist, int HW, int W) {
  const int p = blockIdx.y;
  const float* pu = flow + 2L * HW * p;
  float* po = dist + static_cast<long>(HW) * p;
  float F[9];
  epi_F(F32, p, F);
#pragma unroll
  for (int it = 0; it < EPI_ITERS; ++it) {
    const EpiQuad q = epi_load<VEC>(pu, pu + HW, HW, W, it);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = e < q.n ? epi_point(F, q.x[e], q.y[e], q.u[e], q.v[e]).dist() : 0.f;
    epi_store<VEC>(po, q, o);
  }
}

template <bool VEC>
__global__ void __launch_bounds__(EPI_THREADS) k_epi_loss_part(const float* __restrict__ flow_bwd, const float* __restrict__ flow_fwd,
                                                                const float* __restrict__ F32, double* __restrict__ part, int B,
                                                                int HW, int W) {
  __shared__ double sW[EPI_WAVES];
  const int p = blockIdx.y;
  const float* pu = epi_flow(flow_bwd, flow_fwd, B, p, HW);
  float F[9];
  epi_F(F32, p, F);
  double acc = 0.0;
#pragma unroll
  for (int it = 0; it < EPI_ITERS; ++it) {
    const EpiQuad q = epi_load<VEC>(pu, pu + HW, HW, W, it);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < q.n) acc += static_cast<double>(epi_point(F, q.x[e], q.y[e], q.u[e], q.v[e]).dist());
  }
  const double t = epi_block_sum(acc, sW);
  if (threadIdx.x == 0) part[static_cast<long>(p) * gridDim.x + blockIdx.x] = t;
}

// loss[b] = mean(plane b) + mean(plane B + b): thread t takes partials t, t + 256, ... of each plane, then the block sum
__global__ void __launch_bounds__(EPI_THREADS) k_epi_loss_fin(const double* __restrict__ part, float* __restrict__ loss, int B, int nb,
                                                               int HW) {
  __shared__ double sW[EPI_WAVES];
  const int b = blockIdx.x;
  double a0 = 0.0, a1 = 0.0;
  for (int k = threadIdx.x; k < nb; k += EPI_THREADS) {
    a0 += part[static_cast<long>(b) * nb + k];
    a1 += part[static_cast<long>(B + b) * nb + k];
  }
  const double s0 = epi_block_sum(a0, sW), s1 = epi_block_sum(a1, sW);
  if (threadIdx.x == 0) loss[b] = static_cast<float>(s0 / HW + s1 / HW);
}

template <bool VEC>
__global__ void __launch_bounds__(EPI_THREADS) k_epi_bwd(const float* __restrict__ flow_bwd, const float* __restrict__ flow_fwd,
                                                          const float* __restrict__ F32, const float* __restrict__ gloss,
                                                          float* __restrict__ gflow_bwd, float* __restrict__ gflow_fwd, int B, int HW,
                                                          int W) {
  const int p = blockIdx.y, b = p < B ? p : p - B;
  const float* pu = epi_flow(flow_bwd, flow_fwd, B, p, HW);
  float* gu = (p < B ? gflow_bwd : gflow_fwd) + 2L * HW * b;
  float F[9];
  epi_F(F32, p, F);
  const float c = gloss[b] / static_cast<float>(HW);
#pragma unroll
  for (int it = 0; it < EPI_ITERS; ++it) {
    const EpiQuad q = epi_load<VEC>(pu, pu + HW, HW, W, it);
    float ou[4], ov[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ou[e] = ov[e] = 0.f;
      if (e < q.n) {
        const EpiPoint pt = epi_point(F, q.x[e], q.y[e], q.u[e], q.v[e]);
        // torch.abs's derivative: sgn(0) = 0; a NaN s passes through the product
        const float sg = pt.s > 0.f ? 1.f : (pt.s < 0.f ? -1.f : (pt.s == 0.f ? 0.f : pt.s));
        const float cs = c * sg;
        ou[e] = cs * pt.l0 / pt.div;
        ov[e] = cs * pt.l1 / pt.div;
      }
    }
    epi_store<VEC>(gu, q, ou);
    epi_store<VEC>(gu + HW, q, ov);
  }
}

int epi_check(int planes, int H, int W) {
  if (planes <= 0 || planes > 32768 || H < 1 || W < 1) return DFE_ERR_DIMS;
  if (static_cast<long>(H) * W >= (1L << 28)) return DFE_ERR_DIMS;
  return DFE_OK;
}

}  // namespace
}  // namespace dfe

using namespace dfe;

extern "C" long dfe_epipolar_ws_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return 8L * 2 * B * epi_blocks(static_cast<long>(H) * W);
}

extern "C" int dfe_epipolar_map(const float* flow, const float* F32, float* dist, int P, int H, int W, void* stream) {
  if (!flow || !F32 || !dist) return DFE_ERR_NULL;
  const int rc = epi_check(P, H, W);
  if (rc != DFE_OK) return rc;
  const int HW = H * W;
  const dim3 grid(epi_blocks(HW), P);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (HW % 4 == 0 && aligned16(flow) && aligned16(dist)) k_epi_map<true><<<grid, EPI_THREADS, 0, st>>>(flow, F32, dist, HW, W);
  else k_epi_map<false><<<grid, EPI_THREADS, 0, st>>>(flow, F32, dist, HW, W);
  return launch_status();
}

extern "C" int dfe_epipolar_loss_fwd(const float* flow_bwd, const float* flow_fwd, const float* F32, float* loss, void* ws, int B,
                                     int H, int W, void* stream) {
  if (!flow_bwd || !flow_fwd || !F32 || !loss || !ws) return DFE_ERR_NULL;
  if (B > 16384) return DFE_ERR_DIMS;
  const int rc = epi_check(2 * B, H, W);
  if (rc != DFE_OK) return rc;
  if (!aligned8(ws)) return DFE_ERR_DIMS;
  const int HW = H * W, nb = epi_blocks(HW);
  const dim3 grid(nb, 2 * B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(ws);
  if (HW % 4 == 0 && aligned16(flow_bwd) && aligned16(flow_fwd))
    k_epi_loss_part<true><<<grid, EPI_THREADS, 0, st>>>(flow_bwd, flow_fwd, F32, part, B, HW, W);
  else
    k_epi_loss_part<false><<<grid, EPI_THREADS, 0, st>>>(flow_bwd, flow_fwd, F32, part, B, HW, W);
  DFE_LAUNCH_CHECK();
  k_epi_loss_fin<<<B, EPI_THREADS, 0, st>>>(part, loss, B, nb, HW);
  return launch_status();
}

extern "C" int dfe_epipolar_loss_bwd(const float* flow_bwd, const float* flow_fwd, const float* F32, const float* gloss,
                                     float* gflow_bwd, float* gflow_fwd, int B, int H, int W, void* stream) {
  if (!flow_bwd || !flow_fwd || !F32 || !gloss || !gflow_bwd || !gflow_fwd) return DFE_ERR_NULL;
  if (B > 16384) return DFE_ERR_DIMS;
  const int rc = epi_check(2 * B, H, W);
  if (rc != DFE_OK) return rc;
  const int HW = H * W;
  const dim3 grid(epi_blocks(HW), 2 * B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (HW % 4 == 0 && aligned16(flow_bwd) && aligned16(flow_fwd) && aligned16(gflow_bwd) && aligned16(gflow_fwd))
    k_epi_bwd<true><<<grid, EPI_THREADS, 0, st>>>(flow_bwd, flow_fwd, F32, gloss, gflow_bwd, gflow_fwd, B, HW, W);
  else
    k_epi_bwd<false><<<grid, EPI_THREADS, 0, st>>>(flow_bwd, flow_fwd, F32, gloss, gflow_bwd, gflow_fwd, B, HW, W);
  return launch_status();
}
