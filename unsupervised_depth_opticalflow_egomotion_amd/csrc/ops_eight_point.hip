// The eight-point term (model_geometry.py:532-566, call site :949-950): the robust fundamental matrix of the sampled matches --
// GeometrySolvers.compute_fundmental_mat's FM_RANSAC branch, step for step, in double -- and the smooth-L1 loss against the
// pose's K^-T ([t]x R) K^-1.  Plane p = d*B + b (d = 0: target -> left, 1: target -> right); match j of a plane is the pixel
// idx[p][pick[j]] as in ops_triangulate.hip; both directions of sample b vote with the minimal sets sets[b].
//
//   k_ep_matches    one thread per match: (x, y, x + u, y + v), the sums in fp32, widened -> ws
//   k_ep_hyp        one thread per (plane, hypothesis): normalised eight-point on its 8 matches, its 9x9 matrices in LDS -> ws
//   k_ep_score      a tile of MATCH_TILE matches per block (one per thread), hypotheses in tiles of HYP_TILE through LDS:
//                   inlier counts by wave ballots, integer atomics
//   k_ep_consensus  one block per plane: best hypothesis (ties: lowest index), its inlier set, two weighted refits, F / F[2][2]
//   k_ep_loss_fwd / k_ep_loss_bwd   one thread per sample / per (sample, direction)
// The draw, the workspace, scoring, the consensus skeleton and the launch sequence are dfe_ransac.h's, shared with ops_pnp.hip;
// here: the model, the hypothesis kernel, the refit, the loss.
// No float atomics: every float sum has an order fixed by thread index; same bits run after run.
#include "dfe_internal.h"
#include "dfe_eight_point.h"
#include "dfe_ransac.h"

namespace dfe {
namespace {

using ransac::THREADS;
constexpr int EP_HYP_THREADS = 32;     // k_ep_hyp: 2 x 81 doubles of LDS per thread, 40.5 KiB per block
constexpr int EP_RED = 15;             // sums reduced side by side (the 45 entries of the normal matrix in three rounds)

struct EpModel {
  static constexpr int PT = 4, HP = 9, MIN = 8;     // (x1, y1, x2, y2); F row-major; the eight-point algorithm's set
  struct Ctx {};
  static __device__ __forceinline__ bool inlier(const Ctx&, const double* F, const double* m, double thr2) {
    return ep::inlier(F, m[0], m[1], m[2], m[3], thr2);
  }
};

__global__ void __launch_bounds__(THREADS) k_ep_matches(const float* __restrict__ flow_bwd, const float* __restrict__ flow_fwd,
                                                         const int* __restrict__ idx, const long long* __restrict__ pick,
                                                         double* __restrict__ m, int B, int H, int W, int k, int num) {
  const int j = blockIdx.x * THREADS + threadIdx.x;
  const int plane = blockIdx.y, d = plane / B, b = plane - d * B;
  if (j >= num) return;
  const ransac::Match mt = ransac::load_match(d ? flow_fwd : flow_bwd, idx, pick, plane, b, j, k, H, W);
  const float y = static_cast<float>(mt.y), x = static_cast<float>(mt.x);
  const float x2 = x + mt.u, y2 = y + mt.v;
  double* o = m + (static_cast<long>(plane) * num + j) * 4;
  o[0] = x; o[1] = y; o[2] = x2; o[3] = y2;
}

__global__ void __launch_bounds__(EP_HYP_THREADS) k_ep_hyp(const double* __restrict__ m, const int* __restrict__ sets,
                                                            double* __restrict__ Fh, int B, int num, int hyp) {
  __shared__ double sMV[2 * 81 * EP_HYP_THREADS];
  const int h = blockIdx.x * EP_HYP_THREADS + threadIdx.x;
  const int plane = blockIdx.y, b = plane % B;
  if (h >= hyp) return;             // no barrier below: every thread works on its own slice of sMV
  const double* mp = m + static_cast<long>(plane) * num * 4;
  double pt[8][4];
  double sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int s = sets[(static_cast<long>(b) * hyp + h) * 8 + i];
    s = s < 0 ? 0 : (s > num - 1 ? num - 1 : s);
    for (int c = 0; c < 4; ++c) pt[i][c] = mp[static_cast<long>(s) * 4 + c];
    sx1 += pt[i][0]; sy1 += pt[i][1]; sx2 += pt[i][2]; sy2 += pt[i][3];
  }
  const double cx1 = sx1 / 8.0, cy1 = sy1 / 8.0, cx2 = sx2 / 8.0, cy2 = sy2 / 8.0;
  double d1 = 0.0, d2 = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    d1 += sqrt((pt[i][0] - cx1) * (pt[i][0] - cx1) + (pt[i][1] - cy1) * (pt[i][1] - cy1));
    d2 += sqrt((pt[i][2] - cx2) * (pt[i][2] - cx2) + (pt[i][3] - cy2) * (pt[i][3] - cy2));
  }
  const ep::Norm n1 = ep::make_norm(cx1, cy1, d1 / 8.0), n2 = ep::make_norm(cx2, cy2, d2 / 8.0);
  // the thread's two 9x9 matrices in LDS, element i at [i * EP_HYP_THREADS + thread]: Jacobi indexes them at run time
  double* M = sMV + threadIdx.x;
  double* V = sMV + 81 * EP_HYP_THREADS + threadIdx.x;
  double a[9], F[9];
  for (int i = 0; i < 81; ++i) M[i * EP_HYP_THREADS] = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    ep::row9(n1, n2, pt[i][0], pt[i][1], pt[i][2], pt[i][3], a);
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
      for (int c = 0; c < 9; ++c) M[(9 * r + c) * EP_HYP_THREADS] += a[r] * a[c];
  }
  ep::solve_normal(M, V, EP_HYP_THREADS, n1, n2, F);
  double* o = Fh + (static_cast<long>(plane) * hyp + h) * 9;
  for (int i = 0; i < 9; ++i) o[i] = F[i];
}

__global__ void __launch_bounds__(ransac::MATCH_TILE) k_ep_score(const double* __restrict__ m, const double* __restrict__ Fh,
                                                                  int* __restrict__ counts, int num, int hyp, double thr2) {
  ransac::score_body<EpModel>(EpModel::Ctx{}, m, Fh, counts, num, hyp, thr2);
}

// _eight_point(m, w) of one plane by the whole block: weighted Hartley sums, the normal matrix, thread 0 solves -> sF (LDS)
__device__ void refit(const double* __restrict__ mp, const int* __restrict__ w, int num, double* red, double* sM, double* sV, double* sF) {
  double v[EP_RED];
  for (int i = 0; i < EP_RED; ++i) v[i] = 0.0;
  for (int j = threadIdx.x; j < num; j += THREADS) {
    const double wj = w[j];
    v[0] += mp[4 * j] * wj; v[1] += mp[4 * j + 1] * wj; v[2] += mp[4 * j + 2] * wj; v[3] += mp[4 * j + 3] * wj;
    v[4] += wj;
  }
  ransac::block_sum<EP_RED>(v, red);
  const double cnt = v[4] < 1.0 ? 1.0 : v[4];
  const double cx1 = v[0] / cnt, cy1 = v[1] / cnt, cx2 = v[2] / cnt, cy2 = v[3] / cnt;
  for (int i = 0; i < EP_RED; ++i) v[i] = 0.0;
  for (int j = threadIdx.x; j < num; j += THREADS) {
    const double wj = w[j];
    const double ax = mp[4 * j] - cx1, ay = mp[4 * j + 1] - cy1, bx = mp[4 * j + 2] - cx2, by = mp[4 * j + 3] - cy2;
    v[0] += sqrt(ax * ax + ay * ay) * wj;
    v[1] += sqrt(bx * bx + by * by) * wj;
  }
  ransac::block_sum<EP_RED>(v, red);
  const ep::Norm n1 = ep::make_norm(cx1, cy1, v[0] / cnt), n2 = ep::make_norm(cx2, cy2, v[1] / cnt);
  double acc[45];
  for (int i = 0; i < 45; ++i) acc[i] = 0.0;
  for (int j = threadIdx.x; j < num; j += THREADS) {
    const double wj = w[j];
    double a[9];
    ep::row9(n1, n2, mp[4 * j], mp[4 * j + 1], mp[4 * j + 2], mp[4 * j + 3], a);
    int e = 0;
    for (int r = 0; r < 9; ++r)
      for (int c = r; c < 9; ++c) acc[e++] += a[r] * wj * a[c];
  }
  ransac::block_sum<EP_RED>(acc, red);
  ransac::block_sum<EP_RED>(acc + EP_RED, red);
  ransac::block_sum<EP_RED>(acc + 2 * EP_RED, red);
  if (threadIdx.x == 0) {
    int e = 0;
    for (int r = 0; r < 9; ++r)
      for (int c = r; c < 9; ++c) { sM[9 * r + c] = acc[e]; sM[9 * c + r] = acc[e]; ++e; }
    ep::solve_normal(sM, sV, 1, n1, n2, sF);
  }
  __syncthreads();
}

__global__ void __launch_bounds__(THREADS) k_ep_consensus(const double* __restrict__ m, const double* __restrict__ Fh,
                                                           const int* __restrict__ counts, int* __restrict__ w1,
                                                           int* __restrict__ w2, double* __restrict__ F64, float* __restrict__ F32,
                                                           int* __restrict__ info, int num, int hyp, double thr2) {
  __shared__ double red[EP_RED * THREADS];
  __shared__ double sM[81], sV[81], sF[9];
  const int plane = blockIdx.x;
  const double* mp = m + static_cast<long>(plane) * num * 4;
  ransac::consensus_body<EpModel>(
      EpModel::Ctx{}, m, Fh, counts, w1, w2, info, num, hyp, thr2, sF,
      [&](const int* w, int) { refit(mp, w, num, red, sM, sV, sF); },
      [&]() {
        if (threadIdx.x < 9) {
          const double f = sF[threadIdx.x] / sF[8];
          F64[plane * 9 + threadIdx.x] = f;
          F32[plane * 9 + threadIdx.x] = static_cast<float>(f);
        }
      });
}

// ---------------------------------------------------------------------------------------------- loss
__device__ __forceinline__ void mat3(const float* a, const float* b, float* o) {     // o = a b, the sum in index order
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

// F_pred - F of (b, d): E rows are sample-major (b*2 + d), F planes direction-major (d*B + b)
__device__ __forceinline__ void ep_diff(const float* E, const float* Kt_inv, const float* K_inv, const float* F32, int B, int b, int d,
                                        float* diff) {
  float meta[9], pred[9];
  mat3(E + (b * 2 + d) * 9, K_inv + b * 9, meta);
  mat3(Kt_inv + b * 9, meta, pred);
  for (int i = 0; i < 9; ++i) diff[i] = pred[i] - F32[(d * B + b) * 9 + i];
}

__global__ void k_ep_loss_fwd(const float* __restrict__ E, const float* __restrict__ Kt_inv, const float* __restrict__ K_inv,
                              const float* __restrict__ F32, float* __restrict__ loss, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float term[2];
  for (int d = 0; d < 2; ++d) {
    float diff[9], s = 0.f;
    ep_diff(E, Kt_inv, K_inv, F32, B, b, d, diff);
    for (int i = 0; i < 9; ++i) {
      const float a = fabsf(diff[i]);
      s += a < 1.f ? 0.5f * diff[i] * diff[i] : a - 0.5f;
    }
    term[d] = s / 9.f;
  }
  loss[b] = term[0] + term[1];
}

__global__ void k_ep_loss_bwd(const float* __restrict__ E, const float* __restrict__ Kt_inv, const float* __restrict__ K_inv,
                              const float* __restrict__ F32, const float* __restrict__ gloss, float* __restrict__ gE, int B) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * B) return;
  const int b = t >> 1, d = t & 1;
  float diff[9], G[9], tmp[9];
  ep_diff(E, Kt_inv, K_inv, F32, B, b, d, diff);
  const float g = gloss[b] / 9.f;
  for (int i = 0; i < 9; ++i) G[i] = g * (fabsf(diff[i]) < 1.f ? diff[i] : (diff[i] > 0.f ? 1.f : -1.f));
  // F_pred = A E C, A = Kt_inv, C = K_inv: gE = A^T G C^T
  const float* A = Kt_inv + b * 9;
  const float* C = K_inv + b * 9;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) tmp[3 * i + j] = (A[i] * G[j] + A[3 + i] * G[3 + j]) + A[6 + i] * G[6 + j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) gE[t * 9 + 3 * i + j] = (tmp[3 * i] * C[3 * j] + tmp[3 * i + 1] * C[3 * j + 1]) + tmp[3 * i + 2] * C[3 * j + 2];
}

}  // namespace
}  // namespace dfe

using namespace dfe;

extern "C" long dfe_eight_point_ws_bytes(int B, int num, int hyp) {
  if (B <= 0 || num <= 0 || hyp <= 0) return 0;
  return ransac::ws_offsets(EpModel::PT, EpModel::HP, B, num, hyp).bytes;
}

extern "C" int dfe_fundamental_ransac(const float* flow_bwd, const float* flow_fwd, const int* idx, const long long* pick,
                                      const int* sets, double* F64, float* F32, int* info, void* ws, int B, int H, int W, int k,
                                      int num, int hyp, double thresh, void* stream) {
  const bool have_all = flow_bwd && flow_fwd && idx && pick && sets && F64 && F32 && info && ws;
  const int rc = ransac::check_args(have_all, B, H, W, k, num, hyp, EpModel::MIN, ws, F64);
  if (rc != DFE_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ransac::Ws w = ransac::ws_sections(ws, ransac::ws_offsets(EpModel::PT, EpModel::HP, B, num, hyp));
  const double thr2 = thresh * thresh;
  return ransac::launch_all(
      w.counts, B, num, hyp, EP_HYP_THREADS, st,
      [&](dim3 g) { k_ep_matches<<<g, THREADS, 0, st>>>(flow_bwd, flow_fwd, idx, pick, w.m, B, H, W, k, num); },
      [&](dim3 g) { k_ep_hyp<<<g, EP_HYP_THREADS, 0, st>>>(w.m, sets, w.hyps, B, num, hyp); },
      [&](dim3 g) { k_ep_score<<<g, ransac::MATCH_TILE, 0, st>>>(w.m, w.hyps, w.counts, num, hyp, thr2); },
      [&](dim3 g) { k_ep_consensus<<<g, THREADS, 0, st>>>(w.m, w.hyps, w.counts, w.w1, w.w2, F64, F32, info, num, hyp, thr2); });
}

extern "C" int dfe_eight_point_loss_fwd(const float* E, const float* Kt_inv, const float* K_inv, const float* F32, float* loss,
                                        int B, void* stream) {
  if (!E || !Kt_inv || !K_inv || !F32 || !loss) return DFE_ERR_NULL;
  if (B <= 0 || B > 16384) return DFE_ERR_DIMS;
  k_ep_loss_fwd<<<(B + 63) / 64, 64, 0, static_cast<hipStream_t>(stream)>>>(E, Kt_inv, K_inv, F32, loss, B);
  return launch_status();
}

extern "C" int dfe_eight_point_loss_bwd(const float* E, const float* Kt_inv, const float* K_inv, const float* F32, const float* gloss,
                                        float* gE, int B, void* stream) {
  if (!E || !Kt_inv || !K_inv || !F32 || !gloss || !gE) return DFE_ERR_NULL;
  if (B <= 0 || B > 16384) return DFE_ERR_DIMS;
  k_ep_loss_bwd<<<(2 * B + 63) / 64, 64, 0, static_cast<hipStream_t>(stream)>>>(E, Kt_inv, K_inv, F32, gloss, gE, B);
  return launch_status();
}
