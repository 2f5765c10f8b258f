// Adam update of all parameters in ONE launch (reference train.py:85-87: torch.optim.Adam(model.parameters(), lr);
// default betas / eps, no weight decay, no amsgrad).  The optimiser step is the serial tail of the training step:
// nothing else runs while it does.  ATen's fused multi-tensor Adam passes its pointer tables as kernel arguments, which
// limits one launch to 36 tensors and 320 blocks of 64 Ki elements: six launches of ~48 us at 21.6 M parameters in ~250
// tensors (2 TB/s of the 7 fp32 streams it moves).  Here the tables live in device memory, one block owns
// DFE_ADAM_CHUNK elements of one tensor, and one launch covers everything.  Bound: HBM (4 reads + 3 writes per element).
//   m = m + (1 - b1) (g - m);  v = b2 v + (1 - b2) g g;  p = p - (lr / c1) m / (sqrt(v) / sqrt(c2) + eps)
// (sqrtf here is the compiler's correctly rounded one: oclc_correctly_rounded_sqrt)
// with the bias corrections c1 = 1 - b1^t, c2 = 1 - b2^t of the step count t (the arithmetic of ATen's fused kernel).
#include "dfe_internal.h"
#include <hip/hip_runtime.h>
#include <cstdint>

namespace dfe {

constexpr int ADAM_CHUNK = 4096;       // elements per block: 256 threads x 4 float4

struct AdamRec { float* p; const float* g; float* m; float* v; long long n; };   // 5 x 8 bytes per tensor

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float b1c, float b2, float b2c, float step_size,
                                      float c2s, float eps) {
  m = m + b1c * (g - m);
  v = b2 * v + b2c * g * g;
  const float denom = sqrtf(v) / c2s + eps;
  p = p - step_size * m / denom;
}

// The step count on the DEVICE (a training step replayed from a hipGraph cannot take its bias corrections as kernel arguments:
// they would stay those of the captured step).  One thread: t = ++count; coef = {lr / (1 - b1^t), sqrt(1 - b2^t)}, formed in double.
__global__ void k_adam_tick(double* __restrict__ count, float* __restrict__ coef, double lr, double b1, double b2) {
  const double t = count[0] + 1.0;
  count[0] = t;
  coef[0] = static_cast<float>(lr / (1.0 - pow(b1, t)));
  coef[1] = static_cast<float>(sqrt(1.0 - pow(b2, t)));
}

// One block's update.  GUARDED: the gradient that enters adam1 is fl32(g * gc) (one fp32 product: the build has no implicit FMA),
// which is g itself when gc == 1; the unguarded instantiation is the update as it always was.
template <bool GUARDED>
__device__ __forceinline__ void adam_block(const AdamRec* __restrict__ table, const int* __restrict__ blockmap, float b1c, float b2,
                                           float b2c, float step_size, float c2s, float eps, float gc) {
  const int t = blockmap[2 * blockIdx.x], c = blockmap[2 * blockIdx.x + 1];
  const AdamRec r = table[t];
  const long long base = static_cast<long long>(c) * ADAM_CHUNK;
  const long long left = r.n - base;
  const bool vec = ((reinterpret_cast<uintptr_t>(r.p) | reinterpret_cast<uintptr_t>(r.g) | reinterpret_cast<uintptr_t>(r.m) |
                     reinterpret_cast<uintptr_t>(r.v)) & 15) == 0;
  if (vec && left >= ADAM_CHUNK) {
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / (256 * 4); ++k) {
      const long long e = base + (static_cast<long long>(k) * 256 + threadIdx.x) * 4;
      float4 p = *reinterpret_cast<const float4*>(r.p + e), m = *reinterpret_cast<const float4*>(r.m + e);
      float4 v = *reinterpret_cast<const float4*>(r.v + e);
      float4 g = *reinterpret_cast<const float4*>(r.g + e);
      if (GUARDED) { g.x = g.x * gc; g.y = g.y * gc; g.z = g.z * gc; g.w = g.w * gc; }
      adam1(p.x, g.x, m.x, v.x, b1c, b2, b2c, step_size, c2s, eps);
      adam1(p.y, g.y, m.y, v.y, b1c, b2, b2c, step_size, c2s, eps);
      adam1(p.z, g.z, m.z, v.z, b1c, b2, b2c, step_size, c2s, eps);
      adam1(p.w, g.w, m.w, v.w, b1c, b2, b2c, step_size, c2s, eps);
      *reinterpret_cast<float4*>(r.p + e) = p; *reinterpret_cast<float4*>(r.m + e) = m; *reinterpret_cast<float4*>(r.v + e) = v;
    }
  } else {
    const long long end = left < ADAM_CHUNK ? r.n : base + ADAM_CHUNK;
    for (long long e = base + threadIdx.x; e < end; e += 256) {
      float p = r.p[e], m = r.m[e], v = r.v[e];
      const float g = GUARDED ? r.g[e] * gc : r.g[e];
      adam1(p, g, m, v, b1c, b2, b2c, step_size, c2s, eps);
      r.p[e] = p; r.m[e] = m; r.v[e] = v;
    }
  }
}

// grid: x = block of the block map; blockmap[2k] = tensor, blockmap[2k+1] = chunk.  coef != nullptr: step_size and c2s come from
// device memory (k_adam_tick), the arguments of those names are ignored.
__global__ void __launch_bounds__(256) k_adam_step(const AdamRec* __restrict__ table, const int* __restrict__ blockmap,
                                                   float b1c, float b2, float b2c, float step_size, float c2s, float eps,
                                                   const float* __restrict__ coef) {
  if (coef) { step_size = coef[0]; c2s = coef[1]; }
  adam_block<false>(table, blockmap, b1c, b2, b2c, step_size, c2s, eps, 1.0f);
}

// ---- gradient guard: global-norm clipping (torch.nn.utils.clip_grad_norm_) and the skip of a step whose gradients are not
// finite (GradScaler's, without the scaling), decided on the device.  One more READ of the gradients (4 bytes per element, HBM
// bound), nothing written back: the update multiplies by the coefficient as it loads.  No atomics; every order of addition is
// fixed by thread and block index, so the norm, the coefficient and the decision repeat bit for bit.
struct GuardRec { double norm; double skipped; float c; int finite; int skip; int zero; };   // 32 bytes, see include/dfe_hip.h

__device__ __forceinline__ void sq_acc(double& s, unsigned& bad, float x) {
  const double d = static_cast<double>(x);
  s = s + d * d;                                                     // a 24 x 24 bit product: exact in double
  bad |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;          // NaN or +-inf: all exponent bits set
}

// The sum of ``s`` and the OR of ``bad`` over the block, valid in thread 0: lanes by shuffle (a fixed tree), then the four
// waves in index order through LDS -- never in the order the waves arrive.
__device__ __forceinline__ void block_sum_or(double& s, unsigned& bad) {
  __shared__ double wave_s[4];
  __shared__ unsigned wave_bad[4];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s = s + __shfl_down(s, off);
  bad = __ballot(bad != 0) != 0;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { wave_s[wave] = s; wave_bad[wave] = bad; }
  __syncthreads();
  s = ((wave_s[0] + wave_s[1]) + wave_s[2]) + wave_s[3];
  bad = wave_bad[0] | wave_bad[1] | wave_bad[2] | wave_bad[3];
}

// grid: as k_adam_step's.  Only g is read, so only g's alignment decides between the float4 and the scalar path.
__global__ void __launch_bounds__(256) k_grad_sumsq(const AdamRec* __restrict__ table, const int* __restrict__ blockmap,
                                                    double* __restrict__ partial, int* __restrict__ flags) {
  const int t = blockmap[2 * blockIdx.x], c = blockmap[2 * blockIdx.x + 1];
  const float* __restrict__ g = table[t].g;
  const long long n = table[t].n;
  const long long base = static_cast<long long>(c) * ADAM_CHUNK;
  const long long left = n - base;
  double s = 0.0;
  unsigned bad = 0;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0 && left >= ADAM_CHUNK) {
    float4 x[ADAM_CHUNK / (256 * 4)];
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / (256 * 4); ++k)
      x[k] = *reinterpret_cast<const float4*>(g + base + (static_cast<long long>(k) * 256 + threadIdx.x) * 4);
#pragma unroll
    for (int k = 0; k < ADAM_CHUNK / (256 * 4); ++k) {
      sq_acc(s, bad, x[k].x); sq_acc(s, bad, x[k].y); sq_acc(s, bad, x[k].z); sq_acc(s, bad, x[k].w);
    }
  } else {
    const long long end = left < ADAM_CHUNK ? n : base + ADAM_CHUNK;
    for (long long e = base + threadIdx.x; e < end; e += 256) sq_acc(s, bad, g[e]);
  }
  block_sum_or(s, bad);
  if (threadIdx.x == 0) { partial[blockIdx.x] = s; flags[blockIdx.x] = static_cast<int>(bad); }
}

__device__ __forceinline__ void adam_tick(double* __restrict__ count, float* __restrict__ coef, double lr, double b1, double b2) {
  const double t = count[0] + 1.0;
  count[0] = t;
  coef[0] = static_cast<float>(lr / (1.0 - pow(b1, t)));
  coef[1] = static_cast<float>(sqrt(1.0 - pow(b2, t)));
}

// One block of 256: thread i adds partials i, i + 256, ... in that order, then block_sum_or; thread 0 takes the decisions.
// It stands where k_adam_tick stands on the unguarded path.
__global__ void __launch_bounds__(256) k_grad_guard_finish(const double* __restrict__ partial, const int* __restrict__ flags, int nblocks,
                                                           double max_norm, int skip_nonfinite, double* __restrict__ count,
                                                           float* __restrict__ coef, double lr, double b1, double b2,
                                                           GuardRec* __restrict__ rec) {
  double s = 0.0;
  unsigned bad = 0;
  for (int i = threadIdx.x; i < nblocks; i += 256) { s = s + partial[i]; bad |= static_cast<unsigned>(flags[i]); }
  block_sum_or(s, bad);
  if (threadIdx.x != 0) return;
  const double norm = sqrt(s);
  double c = 1.0;
  if (max_norm > 0.0) {                      // torch: clamp(max_norm / (norm + 1e-6), max = 1); a NaN stays a NaN, inf gives 0
    c = max_norm / (norm + 1e-6);
    c = c > 1.0 ? 1.0 : c;
  }
  const int skip = (skip_nonfinite && bad) ? 1 : 0;
  rec->norm = norm;
  rec->c = static_cast<float>(c);
  rec->finite = bad ? 0 : 1;
  rec->skip = skip;
  rec->zero = 0;
  if (skip) rec->skipped = rec->skipped + 1.0;
  else adam_tick(count, coef, lr, b1, b2);
}

__global__ void k_adam_tick_guarded(double* __restrict__ count, float* __restrict__ coef, double lr, double b1, double b2,
                                    const GuardRec* __restrict__ rec) {
  if (!rec->skip) adam_tick(count, coef, lr, b1, b2);
}

// k_adam_step behind the guard: a skipped step returns before its first load of p, m or v.
__global__ void __launch_bounds__(256) k_adam_step_guarded(const AdamRec* __restrict__ table, const int* __restrict__ blockmap,
                                                           float b1c, float b2, float b2c, float eps, const float* __restrict__ coef,
                                                           const GuardRec* __restrict__ rec) {
  if (rec->skip) return;
  adam_block<true>(table, blockmap, b1c, b2, b2c, coef[0], coef[1], eps, rec->c);
}

}  // namespace dfe

extern "C" int dfe_adam_chunk(void) { return dfe::ADAM_CHUNK; }

extern "C" int dfe_adam_step(const void* table, const int* blockmap, int nblocks, double lr, double beta1, double beta2, double eps,
                             double bias_correction1, double bias_correction2, void* stream) {
  if (!table || !blockmap) return DFE_ERR_NULL;
  if (nblocks <= 0 || !(bias_correction1 > 0.0) || !(bias_correction2 > 0.0)) return DFE_ERR_DIMS;
  // the coefficients are formed in double and rounded once (1 - 0.999f is 4.7e-5 away from 0.001)
  const float step_size = static_cast<float>(lr / bias_correction1);
  const float c2s = static_cast<float>(sqrt(bias_correction2));
  dfe::k_adam_step<<<nblocks, 256, 0, static_cast<hipStream_t>(stream)>>>(static_cast<const dfe::AdamRec*>(table), blockmap,
                                                                        static_cast<float>(1.0 - beta1), static_cast<float>(beta2),
                                                                        static_cast<float>(1.0 - beta2), step_size, c2s, static_cast<float>(eps), nullptr);
  return dfe::launch_status();
}

extern "C" int dfe_adam_step_dev(const void* table, const int* blockmap, int nblocks, double lr, double beta1, double beta2, double eps,
                                 double* step_count, float* coef, void* stream) {
  if (!table || !blockmap || !step_count || !coef) return DFE_ERR_NULL;
  if (nblocks <= 0) return DFE_ERR_DIMS;
  hipStream_t st = static_cast<hipStream_t>(stream);
  dfe::k_adam_tick<<<1, 1, 0, st>>>(step_count, coef, lr, beta1, beta2);
  DFE_LAUNCH_CHECK();
  dfe::k_adam_step<<<nblocks, 256, 0, st>>>(static_cast<const dfe::AdamRec*>(table), blockmap, static_cast<float>(1.0 - beta1),
                                            static_cast<float>(beta2), static_cast<float>(1.0 - beta2), 0.0f, 1.0f, static_cast<float>(eps), coef);
  return dfe::launch_status();
}

extern "C" int dfe_grad_guard_ws_bytes(int nblocks) { return nblocks > 0 ? nblocks * 12 : 0; }     // a double and an int32 per block

extern "C" int dfe_grad_guard_record_bytes(void) { return static_cast<int>(sizeof(dfe::GuardRec)); }

extern "C" int dfe_grad_guard(const void* table, const int* blockmap, int nblocks, double max_norm, int skip_nonfinite, double lr,
                              double beta1, double beta2, void* ws, double* step_count, float* coef, void* record, void* stream) {
  if (!table || !blockmap || !ws || !step_count || !coef || !record) return DFE_ERR_NULL;
  if (nblocks <= 0 || nblocks > (1 << 27)) return DFE_ERR_DIMS;
  if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(record)) & 7) return DFE_ERR_DIMS;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* partial = static_cast<double*>(ws);
  int* flags = reinterpret_cast<int*>(partial + nblocks);
  dfe::k_grad_sumsq<<<nblocks, 256, 0, st>>>(static_cast<const dfe::AdamRec*>(table), blockmap, partial, flags);
  DFE_LAUNCH_CHECK();
  dfe::k_grad_guard_finish<<<1, 256, 0, st>>>(partial, flags, nblocks, max_norm, skip_nonfinite, step_count, coef, lr, beta1, beta2,
                                              static_cast<dfe::GuardRec*>(record));
  return dfe::launch_status();
}

extern "C" int dfe_adam_tick_guarded(double lr, double beta1, double beta2, double* step_count, float* coef, const void* record,
                                     void* stream) {
  if (!step_count || !coef || !record) return DFE_ERR_NULL;
  dfe::k_adam_tick_guarded<<<1, 1, 0, static_cast<hipStream_t>(stream)>>>(step_count, coef, lr, beta1, beta2,
                                                                          static_cast<const dfe::GuardRec*>(record));
  return dfe::launch_status();
}

extern "C" int dfe_adam_step_guarded(const void* table, const int* blockmap, int nblocks, double beta1, double beta2, double eps,
                                     const float* coef, const void* record, void* stream) {
  if (!table || !blockmap || !coef || !record) return DFE_ERR_NULL;
  if (nblocks <= 0) return DFE_ERR_DIMS;
  dfe::k_adam_step_guarded<<<nblocks, 256, 0, static_cast<hipStream_t>(stream)>>>(
      static_cast<const dfe::AdamRec*>(table), blockmap, static_cast<float>(1.0 - beta1), static_cast<float>(beta2),
      static_cast<float>(1.0 - beta2), static_cast<float>(eps), coef, static_cast<const dfe::GuardRec*>(record));
  return dfe::launch_status();
}
