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
  const int2 xt = xtab[d.xtab + xs];
  const int4 yt = ytab[d.ytab + y];
  const int x0 = xt.x, x1 = min(x0 + 1, d.w0 - 1);
  const int a0 = xt.y & 0xffff, a1 = xt.y >> 16, b0 = yt.z & 0xffff, b1 = yt.z >> 16;
  const unsigned char* src = in + d.offset + static_cast<long>(f) * d.h0 * d.w0 * 3;
  const unsigned char* r0 = src + static_cast<long>(yt.x) * d.w0 * 3;
  const unsigned char* r1 = src + static_cast<long>(yt.y) * d.w0 * 3;
  float* o = out + (static_cast<long>(b) * 3 * 3 * H + static_cast<long>(f) * H + y) * W + x;   // [b][c][f*H + y][x]
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int ci = rgb ? 2 - c : c;                // cv2.imread's B, G, R from R, G, B bytes
    const int h0 = r0[x0 * 3 + ci] * a0 + r0[x1 * 3 + ci] * a1;
    const int h1 = r1[x0 * 3 + ci] * a0 + r1[x1 * 3 + ci] * a1;
    int u = (3 * xs + c < nvec) ? ((((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2)
                                : ((h0 * b0 + h1 * b1 + (1 << 21)) >> 22);
    u = min(max(u, 0), 255);
    o[static_cast<long>(c) * 3 * H * W] = s_lut[u];
  }
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
