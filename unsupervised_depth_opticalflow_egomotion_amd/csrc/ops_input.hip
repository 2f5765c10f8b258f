// Device-side input pipeline: what KITTI_Prepared.__getitem__ does per sample on CPU workers
// (core/dataset/kitti_prepared.py:63-90,132-152) -- split the stacked triplet, resize each frame to the training
// size, optional horizontal flip, / 255, HWC -> CHW -- as one launch over the whole batch, fed with the raw uint8
// triplets (one H2D copy of 1/4 of the float bytes instead of a blocking float copy, train.py:171).
//   in  : uint8 [B][3*H0][W0][3]  (frames stacked along H, channel order as stored -- cv2.imread's BGR is kept)
//   out : fp32  [B][3][3*H][W]    in [0,1]
// Resize = bilinear with half-pixel centres and edge replication (cv2.INTER_LINEAR's geometry) evaluated in fp32;
// cv2's 8-bit path rounds through 11-bit fixed-point coefficients, which is not reproduced (differences <= 1/255).
// One thread per output pixel, three channels each: 12 source bytes gathered, 12 bytes written -> HBM-bound streaming.
#include "dfe_device.h"
#include "dfe_internal.h"

namespace dfe {

__global__ void __launch_bounds__(256) k_prepare_triplets(const unsigned char* __restrict__ in, const unsigned char* __restrict__ flip,
                                                          float* __restrict__ out, int B, int H0, int W0, int H, int W) {
  const long n = static_cast<long>(B) * 3 * H * W;
  const long i = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = static_cast<int>(i % W), y = static_cast<int>((i / W) % H);
  const int f = static_cast<int>((i / (static_cast<long>(W) * H)) % 3), b = static_cast<int>(i / (static_cast<long>(W) * H * 3));
  const int xs = (flip && flip[b]) ? W - 1 - x : x;           // cv2.flip(img, 1) after the resize
  const float sy = static_cast<float>(H0) / H, sx = static_cast<float>(W0) / W;
  float fy = (y + 0.5f) * sy - 0.5f, fx = (xs + 0.5f) * sx - 0.5f;
  fy = fminf(fmaxf(fy, 0.0f), static_cast<float>(H0 - 1)); fx = fminf(fmaxf(fx, 0.0f), static_cast<float>(W0 - 1));
  const int y0 = static_cast<int>(fy), x0 = static_cast<int>(fx);
  const int y1 = min(y0 + 1, H0 - 1), x1 = min(x0 + 1, W0 - 1);
  const float wy = fy - y0, wx = fx - x0;
  const unsigned char* src = in + (static_cast<long>(b) * 3 + f) * H0 * W0 * 3;
  const unsigned char* p00 = src + (static_cast<long>(y0) * W0 + x0) * 3;
  const unsigned char* p01 = src + (static_cast<long>(y0) * W0 + x1) * 3;
  const unsigned char* p10 = src + (static_cast<long>(y1) * W0 + x0) * 3;
  const unsigned char* p11 = src + (static_cast<long>(y1) * W0 + x1) * 3;
  float* o = out + (static_cast<long>(b) * 3 * 3 * H + static_cast<long>(f) * H + y) * W + x;   // [b][c][f*H + y][x]
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float top = p00[c] + (static_cast<float>(p01[c]) - p00[c]) * wx;
    const float bot = p10[c] + (static_cast<float>(p11[c]) - p10[c]) * wx;
    o[static_cast<long>(c) * 3 * H * W] = (top + (bot - top) * wy) * (1.0f / 255.0f);
  }
}

}  // namespace dfe

extern "C" int dfe_prepare_triplets(const unsigned char* in_u8, const unsigned char* flip, float* out, int B, int H0, int W0,
                                    int H, int W, void* stream) {
  if (!in_u8 || !out) return DFE_ERR_NULL;
  if (B <= 0 || H0 <= 0 || W0 <= 0 || H <= 0 || W <= 0) return DFE_ERR_DIMS;
  const long n = static_cast<long>(B) * 3 * H * W;
  dfe::k_prepare_triplets<<<static_cast<unsigned>((n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(in_u8, flip, out, B, H0, W0, H, W);
  return dfe::launch_status();
}

// ---------------------------------------------------------------------------------------------------------------------
// The reference's own 8-bit arithmetic (kitti_prepared.py:63-90,132-152: cv2.imread -> per-frame cv2.resize INTER_LINEAR on
// uint8 -> cv2.flip(img, 1) -> / 255.0), for a batch whose samples each have their own raw size (H0, W0).  The host
// (ops.prepare_triplets_u8) restates OpenCV 4.1.1's resize.cpp coefficient set-up (cv::resize / cv::hal::resize,
// resizeGeneric_'s xofs / ialpha / yofs / ibeta, the INTER_AREA switch at an exact 1/2) into per-size tables; the kernel is
// integer-only:
//   horizontal (HResizeLinear, fixed point 2^11):  h = S[y][x0]*a0 + S[y][x0+1]*a1                        (int32)
//   vertical, vector rule (VResizeLinearVec_32s8u): u = sat_u8((((b0*(h0>>4))>>16) + ((b1*(h1>>4))>>16) + 2) >> 2)
//   vertical, scalar rule (VResizeLinear + FixedPtCast<int,uchar,22>): u = sat_u8((h0*b0 + h1*b1 + (1<<21)) >> 22)
// with the scalar rule on the row's bytes at and beyond `nvec` (the tail OpenCV's vector loop leaves; host-computed).
// A same-size frame (cv::resize copies) is the table x0 = dx, a = (2048, 0), y0 = dy, b = (2048, 0): both rules return S.
// The exact 1/2 (INTER_AREA, resizeAreaFast_: (a + b + c + d + 2) >> 2) is the table x0 = 2dx, a = (1024, 1024),
// y0 = 2dy, y1 = 2dy + 1, b = (1024, 1024): both rules reduce to that sum exactly.  u -> lut[u] = float32(u / 255.0)
// (256 entries made in double on the host; not u * (1/255.f)).
// One thread per output (sample, frame, row, column): three gathered pixels' bytes per channel, three coalesced fp32
// stores (one per channel plane).

namespace dfe {

// The one statement of the 8-bit arithmetic above: byte `c` (0..2 = B, G, R) of column xs, row y of frame f of the sample d
// describes, resized.  k_prepare_triplets_u8 looks the byte up in the table; k_resize_strips_u8 stores it.
__device__ __forceinline__ void resized_bgr_u8(const unsigned char* __restrict__ in, const dfe_u8_desc& d, const int2* __restrict__ xtab,
                                               const int4* __restrict__ ytab, int f, int y, int xs, int nvec, int rgb, int (&u)[3]) {
  const int2 xt = xtab[d.xtab + xs];
  const int4 yt = ytab[d.ytab + y];
  const int x0 = xt.x, x1 = min(x0 + 1, d.w0 - 1);
  const int a0 = xt.y & 0xffff, a1 = xt.y >> 16, b0 = yt.z & 0xffff, b1 = yt.z >> 16;
  const unsigned char* src = in + d.offset + static_cast<long>(f) * d.h0 * d.w0 * 3;
  const unsigned char* r0 = src + static_cast<long>(yt.x) * d.w0 * 3;
  const unsigned char* r1 = src + static_cast<long>(yt.y) * d.w0 * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int ci = rgb ? 2 - c : c;                // cv2.imread's B, G, R from R, G, B bytes
    const int h0 = r0[x0 * 3 + ci] * a0 + r0[x1 * 3 + ci] * a1;
    const int h1 = r1[x0 * 3 + ci] * a0 + r1[x1 * 3 + ci] * a1;
    const int v = (3 * xs + c < nvec) ? ((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2)
                                      : ((h0 * b0 + h1 * b1 + (1 << 21)) >> 22);
    u[c] = min(max(v, 0), 255);
  }
}

__global__ void __launch_bounds__(256) k_prepare_triplets_u8(const unsigned char* __restrict__ in, const dfe_u8_desc* __restrict__ desc,
                                                             const int2* __restrict__ xtab, const int4* __restrict__ ytab,
                                                             const float* __restrict__ lut, float* __restrict__ out, int B, int H,
                                                             int W, int nvec, int rgb) {
  __shared__ float s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];          // blockDim.x == 256
  __syncthreads();
  const long n = static_cast<long>(B) * 3 * H * W;
  const long i = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = static_cast<int>(i % W), y = static_cast<int>((i / W) % H);
  const int f = static_cast<int>((i / (static_cast<long>(W) * H)) % 3), b = static_cast<int>(i / (static_cast<long>(W) * H * 3));
  const dfe_u8_desc d = desc[b];
  const int xs = d.flip ? W - 1 - x : x;          // cv2.flip(img, 1) of the resized strip: column xs of the resize
  int u[3];
  resized_bgr_u8(in, d, xtab, ytab, f, y, xs, nvec, rgb, u);
  float* o = out + (static_cast<long>(b) * 3 * 3 * H + static_cast<long>(f) * H + y) * W + x;   // [b][c][f*H + y][x]
#pragma unroll
  for (int c = 0; c < 3; ++c) o[static_cast<long>(c) * 3 * H * W] = s_lut[u[c]];
}

// The same bytes kept instead of looked up: frame f of sample b goes to store[slot[b*3 + f]] as [3 (B,G,R)][H][W] (slot < 0: the
// frame is stored already, nothing is written).  One thread per (sample, frame, row, column), three byte stores, one per plane.
__global__ void __launch_bounds__(256) k_resize_strips_u8(const unsigned char* __restrict__ in, const dfe_u8_desc* __restrict__ desc,
                                                          const int2* __restrict__ xtab, const int4* __restrict__ ytab,
                                                          const long long* __restrict__ slot, unsigned char* __restrict__ store,
                                                          long F, int B, int H, int W, int nvec, int rgb) {
  const long n = static_cast<long>(B) * 3 * H * W;
  const long i = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int x = static_cast<int>(i % W), y = static_cast<int>((i / W) % H);
  const int f = static_cast<int>((i / (static_cast<long>(W) * H)) % 3), b = static_cast<int>(i / (static_cast<long>(W) * H * 3));
  const long long s = slot[b * 3 + f];
  if (s < 0 || s >= F) return;                    // the store is never written outside its F frames, whatever slot holds
  int u[3];
  resized_bgr_u8(in, desc[b], xtab, ytab, f, y, x, nvec, rgb, u);
  unsigned char* o = store + (static_cast<long>(s) * 3 * H + y) * W + x;                        // [s][c][y][x]
#pragma unroll
  for (int c = 0; c < 3; ++c) o[static_cast<long>(c) * H * W] = static_cast<unsigned char>(u[c]);
}

// ---------------------------------------------------------------------------------------------------------------------
// One training batch out of the resident store: out[b][c][f*H + y][x] = lut[store[tri[idx[b]][f]][c][y][flip ? W-1-x : x]] and
// the two intrinsics blocks of triplet idx[b].  The batch's triplet indices and flips are kernel ARGUMENTS (GatherBatch, by
// value): no staging buffer, no copy for the stream to wait on.  Pure streaming: 1 byte in, 4 bytes out per element.
// The table stays a table (lut[u] = float32(u / 255.0) made in double on the host, see above: u * (1/255.f) differs in the
// last bit for some u), kept in LDS.
constexpr int GATHER_MAX = 64;                     // samples per launch
struct GatherBatch {
  int idx[GATHER_MAX];
  unsigned long long flip;                         // bit b: sample b is flipped
};

// the frame's first byte, or nullptr when the slot is not one of the store's (the row is then written as lut[0])
__device__ __forceinline__ const unsigned char* gather_frame(const unsigned char* __restrict__ store, long F, const int* __restrict__ tri,
                                                             int t, int f, long frame_bytes) {
  const int s = tri[static_cast<long>(t) * 3 + f];
  return (s >= 0 && s < F) ? store + s * frame_bytes : nullptr;
}

__device__ __forceinline__ void gather_intrinsics(const GatherBatch& gb, const float* __restrict__ ktab, float* __restrict__ K_ms,
                                                  float* __restrict__ K_inv_ms, long i, int nb, int S) {
  const int per = S * 9;
  if (i >= static_cast<long>(nb) * 2 * per) return;
  const int e = static_cast<int>(i % per), which = static_cast<int>((i / per) % 2), b = static_cast<int>(i / (2 * per));
  (which ? K_inv_ms : K_ms)[b * per + e] = ktab[(static_cast<long>(gb.idx[b]) * 2 + which) * per + e];
}

// Vector path (W % 16 == 0, store and out on 16 bytes): a lane owns 16 bytes of one row -- one 16-byte load (from W - 16 - x
// with the bytes reversed in registers when flipped), 16 look-ups, four 16-byte stores.  Lanes run along (b, c, f, y, x / 16):
// the output is written front to back.
__global__ void __launch_bounds__(256) k_gather_triplets_u8_vec(const unsigned char* __restrict__ store, long F, const int* __restrict__ tri,
                                                                const float* __restrict__ ktab, const float* __restrict__ lut,
                                                                float* __restrict__ out, float* __restrict__ K_ms,
                                                                float* __restrict__ K_inv_ms, GatherBatch gb, int nb, int S, int H, int W) {
  __shared__ float s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];          // blockDim.x == 256
  __syncthreads();
  const long i = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  gather_intrinsics(gb, ktab, K_ms, K_inv_ms, i, nb, S);
  const int W16 = W >> 4;
  if (i >= static_cast<long>(nb) * 9 * H * W16) return;
  const int g = static_cast<int>(i % W16), y = static_cast<int>((i / W16) % H);
  const int p = static_cast<int>(i / (static_cast<long>(W16) * H));      // (b * 3 + c) * 3 + f
  const int f = p % 3, c = (p / 3) % 3, b = p / 9;
  const bool flip = (gb.flip >> b) & 1ull;
  const unsigned char* fr = gather_frame(store, F, tri, gb.idx[b], f, static_cast<long>(3) * H * W);
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (fr) v = *reinterpret_cast<const uint4*>(fr + (static_cast<long>(c) * H + y) * W + (flip ? W - 16 - 16 * g : 16 * g));
  if (flip) {                                      // reverse the 16 bytes
    const uint4 t = v;
    v.x = __builtin_bswap32(t.w); v.y = __builtin_bswap32(t.z); v.z = __builtin_bswap32(t.y); v.w = __builtin_bswap32(t.x);
  }
  float4* o = reinterpret_cast<float4*>(out + ((static_cast<long>(b) * 3 + c) * 3 * H + static_cast<long>(f) * H + y) * W + 16 * g);
  const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int q = 0; q < 4; ++q)
    o[q] = make_float4(s_lut[w[q] & 0xffu], s_lut[(w[q] >> 8) & 0xffu], s_lut[(w[q] >> 16) & 0xffu], s_lut[w[q] >> 24]);
}

// Element path (any W, any alignment): one output element per thread, the same bits.
__global__ void __launch_bounds__(256) k_gather_triplets_u8_elem(const unsigned char* __restrict__ store, long F, const int* __restrict__ tri,
                                                                 const float* __restrict__ ktab, const float* __restrict__ lut,
                                                                 float* __restrict__ out, float* __restrict__ K_ms,
                                                                 float* __restrict__ K_inv_ms, GatherBatch gb, int nb, int S, int H, int W) {
  __shared__ float s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];          // blockDim.x == 256
  __syncthreads();
  const long i = static_cast<long>(blockIdx.x) * blockDim.x + threadIdx.x;
  gather_intrinsics(gb, ktab, K_ms, K_inv_ms, i, nb, S);
  if (i >= static_cast<long>(nb) * 9 * H * W) return;
  const int x = static_cast<int>(i % W), y = static_cast<int>((i / W) % H);
  const int p = static_cast<int>(i / (static_cast<long>(W) * H));        // (b * 3 + c) * 3 + f
  const int f = p % 3, c = (p / 3) % 3, b = p / 9;
  const bool flip = (gb.flip >> b) & 1ull;
  const unsigned char* fr = gather_frame(store, F, tri, gb.idx[b], f, static_cast<long>(3) * H * W);
  const unsigned u = fr ? fr[(static_cast<long>(c) * H + y) * W + (flip ? W - 1 - x : x)] : 0u;
  out[i] = s_lut[u];                               // i IS the offset of [b][c][f*H + y][x]
}

}  // namespace dfe

extern "C" int dfe_prepare_triplets_u8(const unsigned char* in_u8, const dfe_u8_desc* desc, const int* xtab, const int* ytab,
                                       const float* lut, float* out, int B, int H, int W, int nvec, int rgb, void* stream) {
  if (!in_u8 || !desc || !xtab || !ytab || !lut || !out) return DFE_ERR_NULL;
  if (B <= 0 || H <= 0 || W <= 0 || nvec < 0 || nvec > 3 * W) return DFE_ERR_DIMS;
  const long n = static_cast<long>(B) * 3 * H * W;
  dfe::k_prepare_triplets_u8<<<static_cast<unsigned>((n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      in_u8, desc, reinterpret_cast<const int2*>(xtab), reinterpret_cast<const int4*>(ytab), lut, out, B, H, W, nvec, rgb);
  return dfe::launch_status();
}

extern "C" int dfe_resize_strips_u8(const unsigned char* in_u8, const dfe_u8_desc* desc, const int* xtab, const int* ytab,
                                    const long long* slot, unsigned char* store, long F, int B, int H, int W, int nvec, int rgb,
                                    void* stream) {
  if (!in_u8 || !desc || !xtab || !ytab || !slot || !store) return DFE_ERR_NULL;
  if (F <= 0 || B <= 0 || H <= 0 || W <= 0 || nvec < 0 || nvec > 3 * W) return DFE_ERR_DIMS;
  const long n = static_cast<long>(B) * 3 * H * W;
  if ((n + 255) / 256 > 0x7fffffffL) return DFE_ERR_DIMS;
  dfe::k_resize_strips_u8<<<static_cast<unsigned>((n + 255) / 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      in_u8, desc, reinterpret_cast<const int2*>(xtab), reinterpret_cast<const int4*>(ytab), slot, store, F, B, H, W, nvec, rgb);
  return dfe::launch_status();
}

extern "C" int dfe_gather_triplets_u8(const unsigned char* store, long F, const int* tri, const float* ktab, int N, const float* lut,
                                      const int* idx_host, const unsigned char* flip_host, float* out, float* K_ms, float* K_inv_ms,
                                      int B, int S, int H, int W, void* stream) {
  if (!store || !tri || !ktab || !lut || !idx_host || !out || !K_ms || !K_inv_ms) return DFE_ERR_NULL;
  if (F <= 0 || N <= 0 || B <= 0 || S <= 0 || S > DFE_MAX_SCALES || H <= 0 || W <= 0) return DFE_ERR_DIMS;
  const long per = static_cast<long>(9) * H * W;                           // output elements per sample
  if (per >= (1L << 31) / dfe::GATHER_MAX) return DFE_ERR_DIMS;            // p * H * W and the grid stay inside 32 bits
  for (int b = 0; b < B; ++b)
    if (idx_host[b] < 0 || idx_host[b] >= N) return DFE_ERR_DIMS;          // before any launch
  const bool vec = W % 16 == 0 && dfe::aligned16(store) && dfe::aligned16(out);
  for (int b0 = 0; b0 < B; b0 += dfe::GATHER_MAX) {
    const int nb = B - b0 < dfe::GATHER_MAX ? B - b0 : dfe::GATHER_MAX;
    dfe::GatherBatch gb;
    gb.flip = 0;
    for (int b = 0; b < dfe::GATHER_MAX; ++b) gb.idx[b] = b < nb ? idx_host[b0 + b] : 0;
    if (flip_host)
      for (int b = 0; b < nb; ++b) gb.flip |= static_cast<unsigned long long>(flip_host[b0 + b] != 0) << b;
    const long nimg = vec ? nb * per / 16 : nb * per, nk = static_cast<long>(nb) * 2 * S * 9;
    const long n = nimg > nk ? nimg : nk;
    const unsigned grid = static_cast<unsigned>((n + 255) / 256);
    float* o = out + b0 * per;
    float* k = K_ms + static_cast<long>(b0) * S * 9;
    float* ki = K_inv_ms + static_cast<long>(b0) * S * 9;
    if (vec)
      dfe::k_gather_triplets_u8_vec<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(store, F, tri, ktab, lut, o, k, ki, gb, nb, S, H, W);
    else
      dfe::k_gather_triplets_u8_elem<<<grid, 256, 0, static_cast<hipStream_t>(stream)>>>(store, F, tri, ktab, lut, o, k, ki, gb, nb, S, H, W);
    DFE_LAUNCH_CHECK();
  }
  return DFE_OK;
}
