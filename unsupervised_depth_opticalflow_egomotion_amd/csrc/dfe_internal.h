// Internal (non-ABI) declarations shared by the translation units of libdfe_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include "../../include/dfe_hip.h"

// after a kernel launch inside an entry point: a failed launch ends the call with DFE_ERR_LAUNCH
#define DFE_LAUNCH_CHECK() do { if (hipGetLastError() != hipSuccess) return DFE_ERR_LAUNCH; } while (0)

namespace dfe {
struct ScaleList { float v[DFE_MAX_SCALES]; };
struct IntList { int v[DFE_MAX_SCALES]; };

// host helpers of the launchers
inline int launch_status() { return hipGetLastError() == hipSuccess ? DFE_OK : DFE_ERR_LAUNCH; }   // the value an entry point returns after its last launch
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }   // an integer tuning switch; dflt when unset
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// a tensor of `per` floats per sample at batch stride bs: the stride holds a sample, and 32-bit offsets hold inside one
inline bool sample_ok(long bs, long per) { return bs >= per && per < (1L << 30); }
// a 256-thread launch with lds_bytes of dynamic LDS; more than 64 KB needs the opt-in attribute (attr_bytes) once per kernel:
// the kernel is a template argument so that every instantiation has its own flag
template <auto Kern, class... Args>
inline void launch_dyn_lds(unsigned grid, size_t lds_bytes, int attr_bytes, hipStream_t st, Args... args) {
  static bool attr_set = false;
  if (!attr_set) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, attr_bytes); attr_set = true; }
  Kern<<<grid, 256, lds_bytes, st>>>(args...);
}

// ops_corr.hip: the PWC cost volume and its gradients (LDS-staged).  out / gout: 81 planes per sample with batch stride
// obs / gbs (the planes may be a slice of a wider tensor); add1 (batch stride abs1) is added to g1 when given.
// tail / flow (optional): planes 81 ... of the same tensor as `out` (a PWC level's x) receive f1 and the two flow planes
int launch_corr_fwd(const float* f1, const float* f2, float* out, long obs, float* tail, const float* flow, int B, int C, int H, int W,
                    hipStream_t st);
int launch_corr_bwd(const float* f1, const float* f2, const float* gout, long gbs, const float* add1, long abs1, float* g1,
                    float* g2, unsigned* amax2, int B, int C, int H, int W, hipStream_t st);

// ops_epilogue.hip: the bias-gradient finisher of the epilogue and decoder-glue passes, in its one fixed order:
// gbias[c] = sum over b < B, k < n of part[(b*C + c)*n + k] (n partials per plane, as many as the producing launch had blocks)
int launch_bias_final(const float* part, float* gbias, int B, int C, int n, hipStream_t st);
}  // namespace dfe
