// Convolution epilogue of the flow nets (reference net_utils.py conv(): Conv2d(bias=True) + LeakyReLU(0.1), used by
// FeaturePyramid and PWC_tf).  PyTorch-ROCm runs "conv, broadcast bias add, activation" as three passes forward and
// "activation backward, bias-gradient reduction" as two more; here the convolution is called without its bias and
//   dfe_bias_act_fwd   y = act(z + bias[c])            in place, one read + one write
//   dfe_bias_act_bwd   gz = gy * act'(y);  gbias[c] = sum_{b,h,w} gz     one pass + a fixed-order final sum
// act(v) = v > 0 ? v : slope * v  (slope 0.1 = LeakyReLU, 0 = ReLU, 1 = bias only); act' is taken from the sign of
// the output (same decision as ATen's, which tests the input: slope >= 0 preserves the sign).
// Bound: HBM.  The bias gradient is reduced per block and finished in a fixed order (no atomics: reproducible).
//
// The same epilogue serves a DenseNet-style block (PWC_tf's decoder, pwc_tf.py:113-117: every layer output is consumed
// through torch.cat by the next two layers): dfe_bias_act_fwd2 / _bwd2.  Forward: read the bias-free convolution output z
// once and write act(z + bias) straight into the channel slices of the (up to two) concatenated buffers that consume it
// -- dst1 may be z itself (in place).  Backward: the output's gradient is the sum of the matching channel slices of the
// consumers' input gradients (g2 optional); y is read from the slice it was written to.  All slices are given by a base
// pointer and a batch stride (channel planes are contiguous inside a sample).  The single-tensor entry points are the
// case d1 = z, no d2 / dense y, no g2 of the same two kernels.
#include "dfe_internal.h"
#include "dfe_device.h"
#include "dfe_chunk.h"
#include <hip/hip_runtime.h>

namespace dfe {

constexpr int EP_BLOCK = CHUNK_BLOCK;
constexpr int EP_PER_THREAD = CHUNK_PER_THREAD;
constexpr int EP_CHUNK = CHUNK_ELEMS;                  // elements of one (b, c) plane per block

// grid: x = chunk of the plane, y = c, z = b
// z, d1 and d2 may alias (d1 == z in place; d1 / d2 slices of one buffer): no __restrict__ on them.  A thread stores only
// the elements it loaded.  The vector walk (hw % 4 == 0: every large plane of the nets) goes through load8 / store8 with all
// its loads issued before the first store.  The scalar walk stays element at a time: its planes are the pose net's few
// hundred elements, those launches take 5 us from a cold instruction cache, and their time follows their code size -- through
// load8 / store8 the scalar forward took 5.4 -> 7.6 us per launch (profiles/glue_epilogue_refactor.txt, D1).
// TWO (a second destination) is a template argument, not a test of d2, for the same reason: with the second destination's
// stores compiled in, the in-place vector launches of a training step took 6.6 -> 7.1 us (same file).
template <bool VEC, bool TWO>
__global__ void __launch_bounds__(EP_BLOCK) k_bias_act_fwd(const float* z, const float* __restrict__ bias,
                                                           float* d1, long d1_bs, float* d2,
                                                           long d2_bs, int C, int HW, float slope) {
  const int b = plane_id() / C, c = plane_id() - b * C;
  const float bv = bias ? bias[c] : 0.0f;
  const long co = static_cast<long>(c) * HW;
  const float* p = z + static_cast<long>(plane_id()) * HW;
  float* o1 = d1 + b * d1_bs + co;
  float* o2 = TWO ? d2 + b * d2_bs + co : nullptr;
  const int base = blockIdx.x * EP_CHUNK;
  if (VEC) {
    float v[EP_PER_THREAD]; bool ok[EP_PER_THREAD];
    load8<true>(p, base, HW, v, ok);
#pragma unroll
    for (int k = 0; k < EP_PER_THREAD; ++k) { const float t = v[k] + bv; v[k] = t > 0.0f ? t : t * slope; }
    store8<true>(o1, base, HW, v);
    if (TWO) store8<true>(o2, base, HW, v);
  } else {
#pragma unroll
    for (int k = 0; k < EP_PER_THREAD; ++k) {
      const int e = base + k * EP_BLOCK + threadIdx.x;
      if (e < HW) { float v = p[e] + bv; v = v > 0.0f ? v : v * slope; o1[e] = v; if (TWO) o2[e] = v; }
    }
  }
}

// y, g1, g2 and gz may be slices of shared buffers: no __restrict__ on them; the two walks as above.  The association of a
// thread's share of the block's bias-gradient partial is part of the result: the vector walk adds (g0 + g1) + (g2 + g3)
// per quad into the accumulator, the scalar walk element by element; elements past the plane's end are left out (not added
// as zeros: an accumulator of -0.0 stays -0.0).
template <bool VEC>
__global__ void __launch_bounds__(EP_BLOCK) k_bias_act_bwd(const float* y, long y_bs, const float* g1,
                                                           long g1_bs, const float* g2, long g2_bs,
                                                           float* gz, float* __restrict__ part, int C, int HW,
                                                           float slope) {
  __shared__ float red[4 * (EP_BLOCK / 64)];
  const int b = plane_id() / C, c = plane_id() - b * C;
  const long co = static_cast<long>(c) * HW;
  const float* py = y + b * y_bs + co;
  const float* pa = g1 + b * g1_bs + co;
  const float* pb = g2 ? g2 + b * g2_bs + co : nullptr;
  float* pz = gz + static_cast<long>(plane_id()) * HW;
  const int base = blockIdx.x * EP_CHUNK;
  float acc[1] = {0.0f};
  if (VEC) {
    float yv[EP_PER_THREAD], g[EP_PER_THREAD], h[EP_PER_THREAD]; bool ok[EP_PER_THREAD];
    load8<true>(py, base, HW, yv, ok);
    load8<true>(pa, base, HW, g, ok);
    if (pb) load8<true>(pb, base, HW, h, ok);
#pragma unroll
    for (int k = 0; k < EP_PER_THREAD; ++k) {
      const float t = pb ? g[k] + h[k] : g[k];
      g[k] = yv[k] > 0.0f ? t : t * slope;
    }
    store8<true>(pz, base, HW, g);
#pragma unroll
    for (int k = 0; k < EP_PER_THREAD; k += 4)
      if (ok[k]) acc[0] += (g[k] + g[k + 1]) + (g[k + 2] + g[k + 3]);
  } else {
#pragma unroll
    for (int k = 0; k < EP_PER_THREAD; ++k) {
      const int e = base + k * EP_BLOCK + threadIdx.x;
      if (e < HW) {
        float g = pa[e];
        if (pb) g += pb[e];
        g = py[e] > 0.0f ? g : g * slope;
        pz[e] = g; acc[0] += g;
      }
    }
  }
  if (part) block_sum<1>(acc, red, part + static_cast<long>(plane_id()) * gridDim.x + blockIdx.x);
}

// The bias-gradient finisher of the epilogues above and of the decoder glue (ops_decoder.hip), the one statement of its
// summation order (a reproducibility contract: deterministic mode, bench.py --dump-outputs):
//   gbias[c] = sum over b, k of part[(b*C + c)*n + k]: one wave per channel; lane l adds its k = l, l + 64, ... of sample 0,
//   then of sample 1, ...; four DPP steps leave each row of 16 lanes with its sum; (r0 + r1) + (r2 + r3) of the four rows.
// n is the number of partials per plane: as many as the producing launch had blocks per plane.
__device__ __forceinline__ void bias_final_sum(const float* __restrict__ part, float* __restrict__ gbias, int B, int C, int n, int c) {
  const int lane = threadIdx.x;
  float s = 0.0f;
  for (int b = 0; b < B; ++b) {
    const float* p = part + (static_cast<long>(b) * C + c) * n;
    for (int k = lane; k < n; k += 64) s += p[k];
  }
  s = dpp_add<0xB1>(s); s = dpp_add<0x4E>(s); s = dpp_add<0x141>(s); s = dpp_add<0x140>(s);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s), 48));
  if (lane == 0) gbias[c] = (r0 + r1) + (r2 + r3);
}

// one layer: grid.x = C, block = one wave
__global__ void __launch_bounds__(64) k_bias_grad_final(const float* __restrict__ part, float* __restrict__ gbias,
                                                        int B, int C, int n) {
  bias_final_sum(part, gbias, B, C, n, blockIdx.x);
}

// Up to EP_MAXL layers in ONE launch (a PWC decoder level's five epilogues used to finish their bias gradients with five
// one-wave-per-channel launches of ~4.5 us each, serialised in the flow stream's backward chain).
// grid.x = sum of the layers' channel counts; block = one wave.  A single job does not go through this kernel: finding its
// layer and fetching the job from the struct put +0.5 us on each of the decoder glue's 6 us finishes
// (profiles/glue_epilogue_refactor.txt, D1).
constexpr int EP_MAXL = 8;
struct BiasFinalJobs { const float* part[EP_MAXL]; float* gbias[EP_MAXL]; int C[EP_MAXL]; int nchunk[EP_MAXL]; int first[EP_MAXL + 1]; int n; };

__global__ void __launch_bounds__(64) k_bias_grad_final_multi(BiasFinalJobs j, int B) {
  int l = 0;
  while (l + 1 < j.n && static_cast<int>(blockIdx.x) >= j.first[l + 1]) ++l;
  bias_final_sum(j.part[l], j.gbias[l], B, j.C[l], j.nchunk[l], blockIdx.x - j.first[l]);
}

int launch_bias_final(const float* part, float* gbias, int B, int C, int n, hipStream_t st) {
  k_bias_grad_final<<<C, 64, 0, st>>>(part, gbias, B, C, n);
  return launch_status();
}

}  // namespace dfe

using namespace dfe;

static inline int ep_nchunk(long hw) { return static_cast<int>((hw + EP_CHUNK - 1) / EP_CHUNK); }

// a plane the chunk walk can index: hw = H * W below 2^31
static bool ep_plane(int H, int W, long& hw) {
  hw = static_cast<long>(H) * W;
  return H > 0 && W > 0 && hw < (1L << 31);
}

// dimensions of a (nchunk, C, B) launch
static int ep_dims(int B, int C, int H, int W, long& hw) {
  return B > 0 && C > 0 && ep_plane(H, W, hw) && C <= 65535 && B <= 65535 ? DFE_OK : DFE_ERR_DIMS;
}

// batch stride of a dense [B, C, H, W] tensor.  Unsigned: it is formed before ep_dims has looked at the dimensions, and
// wraps on those that ep_dims then refuses.
static inline long dense_bs(int C, int H, int W) {
  return static_cast<long>(static_cast<unsigned long>(C) * static_cast<unsigned long>(H) * static_cast<unsigned long>(W));
}

extern "C" long dfe_bias_act_partials_floats(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return static_cast<long>(B) * C * ep_nchunk(static_cast<long>(H) * W);
}

static int ep_fwd(const float* z, const float* bias, float* d1, long d1_bs, float* d2, long d2_bs, int B, int C, int H, int W,
                  float slope, void* stream) {
  if (!z || !d1) return DFE_ERR_NULL;
  long hw;
  if (ep_dims(B, C, H, W, hw) != DFE_OK) return DFE_ERR_DIMS;
  if (d1_bs < C * hw || (d2 && d2_bs < C * hw)) return DFE_ERR_DIMS;
  const dim3 g(ep_nchunk(hw), C, B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool vec = hw % 4 == 0 && aligned16(z) && aligned16(d1) && d1_bs % 4 == 0 && (!d2 || (aligned16(d2) && d2_bs % 4 == 0));
  auto kern = vec ? (d2 ? k_bias_act_fwd<true, true> : k_bias_act_fwd<true, false>)
                  : (d2 ? k_bias_act_fwd<false, true> : k_bias_act_fwd<false, false>);
  kern<<<g, EP_BLOCK, 0, st>>>(z, bias, d1, d1_bs, d2, d2_bs, C, static_cast<int>(hw), slope);
  DFE_LAUNCH_CHECK();
  return DFE_OK;
}

static int ep_bwd(const float* y, long y_bs, const float* g1, long g1_bs, const float* g2, long g2_bs, float* gz, float* gbias,
                  float* partials, int B, int C, int H, int W, float slope, void* stream) {
  if (!y || !g1 || !gz || (gbias && !partials)) return DFE_ERR_NULL;
  long hw;
  if (ep_dims(B, C, H, W, hw) != DFE_OK) return DFE_ERR_DIMS;
  if (y_bs < C * hw || g1_bs < C * hw || (g2 && g2_bs < C * hw)) return DFE_ERR_DIMS;
  const int nchunk = ep_nchunk(hw);
  const dim3 g(nchunk, C, B);
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* part = partials;      // written whenever given: gbias == NULL leaves the finish to dfe_bias_grad_final_multi
  const bool vec = hw % 4 == 0 && aligned16(y) && aligned16(g1) && aligned16(gz) && y_bs % 4 == 0 && g1_bs % 4 == 0 &&
                   (!g2 || (aligned16(g2) && g2_bs % 4 == 0));
  if (vec) k_bias_act_bwd<true><<<g, EP_BLOCK, 0, st>>>(y, y_bs, g1, g1_bs, g2, g2_bs, gz, part, C, static_cast<int>(hw), slope);
  else k_bias_act_bwd<false><<<g, EP_BLOCK, 0, st>>>(y, y_bs, g1, g1_bs, g2, g2_bs, gz, part, C, static_cast<int>(hw), slope);
  DFE_LAUNCH_CHECK();
  return gbias ? launch_bias_final(partials, gbias, B, C, nchunk, st) : DFE_OK;
}

// the single-tensor forms: d1 = z with the dense stride C * hw, which is a multiple of 4 whenever hw is -- the vector
// predicate reduces to "hw % 4 == 0 and the pointers 16-byte aligned"
extern "C" int dfe_bias_act_fwd(float* z, const float* bias, int B, int C, int H, int W, float slope, void* stream) {
  return ep_fwd(z, bias, z, dense_bs(C, H, W), nullptr, 0, B, C, H, W, slope, stream);
}

extern "C" int dfe_bias_act_bwd(const float* y, const float* gy, long gy_batch_stride, float* gz, float* gbias,
                                float* partials, int B, int C, int H, int W, float slope, void* stream) {
  return ep_bwd(y, dense_bs(C, H, W), gy, gy_batch_stride, nullptr, 0, gz, gbias, partials, B, C, H, W, slope, stream);
}

extern "C" int dfe_bias_act_fwd2(const float* z, const float* bias, float* dst1, long dst1_batch_stride, float* dst2,
                                 long dst2_batch_stride, int B, int C, int H, int W, float slope, void* stream) {
  return ep_fwd(z, bias, dst1, dst1_batch_stride, dst2, dst2_batch_stride, B, C, H, W, slope, stream);
}

extern "C" int dfe_bias_act_bwd2(const float* y, long y_batch_stride, const float* g1, long g1_batch_stride, const float* g2,
                                 long g2_batch_stride, float* gz, float* gbias, float* partials, int B, int C, int H, int W,
                                 float slope, void* stream) {
  return ep_bwd(y, y_batch_stride, g1, g1_batch_stride, g2, g2_batch_stride, gz, gbias, partials, B, C, H, W, slope, stream);
}

extern "C" int dfe_bias_grad_final_multi(const float* const* partials, float* const* gbias, const int* C, int n, int B, int H, int W,
                                         void* stream) {
  if (!partials || !gbias || !C) return DFE_ERR_NULL;
  long hw;
  if (n <= 0 || n > EP_MAXL || B <= 0 || !ep_plane(H, W, hw)) return DFE_ERR_DIMS;
  BiasFinalJobs j;
  j.n = n; j.first[0] = 0;
  for (int l = 0; l < n; ++l) {
    if (!partials[l] || !gbias[l]) return DFE_ERR_NULL;
    if (C[l] <= 0 || C[l] > 65535) return DFE_ERR_DIMS;
    j.part[l] = partials[l]; j.gbias[l] = gbias[l]; j.C[l] = C[l];
    j.nchunk[l] = ep_nchunk(hw);
    j.first[l + 1] = j.first[l] + C[l];
  }
  k_bias_grad_final_multi<<<j.first[n], 64, 0, static_cast<hipStream_t>(stream)>>>(j, B);
  DFE_LAUNCH_CHECK();
  return DFE_OK;
}
