// The PnP term (model_geometry.py:473-530, call site :944-945): the robust pose that reprojects the target frame's back-projected
// matches onto their matched pixels -- GeometrySolvers.pnp's robust branch, step for step, in double -- and the L1 loss between
// that (T, axis-angle) and the pose vector.  Plane p = d*B + b (d = 0: target -> left, 1: target -> right); match j of a plane is
// the pixel idx[p][pick[j]] as in ops_eight_point.hip; both directions of sample b vote with the minimal sets sets[b].
//
//   k_pnp_points     one thread per match: the point K_inv (x, y, 1) disp_t formed in double, (x + u, y + v) in fp32, widened -> ws
//   k_pnp_hyp        one thread per (plane, hypothesis): six-point DLT on its 6 matches, its two 12x12 matrices in LDS -> ws
//   k_pnp_score      a tile of MATCH_TILE matches per block (one per thread), hypotheses in tiles of HYP_TILE through LDS:
//                    inlier counts by wave ballots, integer atomics
//   k_pnp_consensus  one block per plane: best hypothesis (ties: lowest index), its inlier set, Levenberg-Marquardt on SE(3),
//                    the re-scored set, Levenberg-Marquardt again, so3 log
//   k_pnp_loss_fwd / k_pnp_loss_bwd   one thread per sample / per (sample, direction)
// The draw, the workspace, scoring, the consensus skeleton and the launch sequence are dfe_ransac.h's, shared with
// ops_eight_point.hip; here: the model, the hypothesis kernel, the refinement, the loss.
// No float atomics: every float sum has an order fixed by thread index; same bits run after run.
#include "dfe_internal.h"
#include "dfe_pnp.h"
#include "dfe_ransac.h"

namespace dfe {
namespace {

using ransac::THREADS;
constexpr int PNP_WAVES = THREADS / 64;
constexpr int PNP_HYP_THREADS = 32;    // k_pnp_hyp: 2 x 144 doubles of LDS per thread, 72 KiB per block

struct PnpModel {
  static constexpr int PT = 5, HP = 12, MIN = 6;    // X, Y, Z, x2, y2; R row-major, T; the six-point DLT's set
  using Ctx = pnp::Cam;
  static __device__ __forceinline__ bool inlier(const Ctx& cam, const double* P, const double* m, double thr2) {
    return pnp::inlier(cam, P, P + 9, m, thr2);
  }
};

__device__ __forceinline__ pnp::Cam load_cam(const float* __restrict__ K, int b) {
  return pnp::Cam{static_cast<double>(K[b * 9]), static_cast<double>(K[b * 9 + 4]), static_cast<double>(K[b * 9 + 2]),
                  static_cast<double>(K[b * 9 + 5])};
}

__global__ void __launch_bounds__(THREADS) k_pnp_points(const float* __restrict__ flow_bwd, const float* __restrict__ flow_fwd,
                                                         const float* __restrict__ disp_t, const int* __restrict__ idx,
                                                         const long long* __restrict__ pick, const float* __restrict__ K_inv,
                                                         double* __restrict__ m, int B, int H, int W, int k, int num) {
  const int j = blockIdx.x * THREADS + threadIdx.x;
  const int plane = blockIdx.y, d = plane / B, b = plane - d * B;
  if (j >= num) return;
  const ransac::Match mt = ransac::load_match(d ? flow_fwd : flow_bwd, idx, pick, plane, b, j, k, H, W);
  const int pix = mt.pix, HW = H * W;
  const float y = static_cast<float>(mt.y), x = static_cast<float>(mt.x);
  const float x2 = x + mt.u, y2 = y + mt.v;
  const double depth = disp_t[static_cast<long>(b) * HW + pix];
  const float* Ki = K_inv + b * 9;
  const double xd = x, yd = y;
  double* o = m + (static_cast<long>(plane) * num + j) * PnpModel::PT;
  for (int i = 0; i < 3; ++i)
    o[i] = ((static_cast<double>(Ki[3 * i]) * xd + static_cast<double>(Ki[3 * i + 1]) * yd) + static_cast<double>(Ki[3 * i + 2])) * depth;
  o[3] = x2; o[4] = y2;
}

__global__ void __launch_bounds__(PNP_HYP_THREADS) k_pnp_hyp(const double* __restrict__ m, const int* __restrict__ sets,
                                                              const float* __restrict__ K, double* __restrict__ Ph, int B, int num,
                                                              int hyp) {
  __shared__ double sMV[2 * 144 * PNP_HYP_THREADS];
  const int h = blockIdx.x * PNP_HYP_THREADS + threadIdx.x;
  const int plane = blockIdx.y, b = plane % B;
  if (h >= hyp) return;             // no barrier below: every thread works on its own slice of sMV
  const double* mp = m + static_cast<long>(plane) * num * PnpModel::PT;
  double Kd[9], Kinv[9];
  for (int i = 0; i < 9; ++i) Kd[i] = K[b * 9 + i];
  pnp::inverse3(Kd, Kinv);
  double S[10], Su[10], Sv[10], Sq[10];
#pragma unroll
  for (int e = 0; e < 10; ++e) S[e] = Su[e] = Sv[e] = Sq[e] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    int s = sets[(static_cast<long>(b) * hyp + h) * 6 + i];
    s = s < 0 ? 0 : (s > num - 1 ? num - 1 : s);
    const double* q = mp + static_cast<long>(s) * PnpModel::PT;
    const double Xh[4] = {q[0], q[1], q[2], 1.0};
    const double u = (Kinv[0] * q[3] + Kinv[1] * q[4]) + Kinv[2], v = (Kinv[3] * q[3] + Kinv[4] * q[4]) + Kinv[5];
    const double uv2 = u * u + v * v;
    int e = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = r; c < 4; ++c) {
        const double pr = Xh[r] * Xh[c];
        S[e] += pr; Su[e] += u * pr; Sv[e] += v * pr; Sq[e] += uv2 * pr;
        ++e;
      }
  }
  // the thread's two 12x12 matrices in LDS, element i at [i * PNP_HYP_THREADS + thread]: Jacobi indexes them at run time
  double* M = sMV + threadIdx.x;
  double* V = sMV + 144 * PNP_HYP_THREADS + threadIdx.x;
  pnp::dlt_normal(S, Su, Sv, Sq, M, PNP_HYP_THREADS);
  const int col = jacobi_sym<12>(M, V, PNP_HYP_THREADS, pnp::JACOBI12_SWEEPS);
  double P[12], R[9], T[3];
  for (int i = 0; i < 12; ++i) P[i] = V[(12 * i + col) * PNP_HYP_THREADS];
  pnp::pose_from_dlt(P, R, T);
  double* o = Ph + (static_cast<long>(plane) * hyp + h) * PnpModel::HP;
  for (int i = 0; i < 9; ++i) o[i] = R[i];
  for (int i = 0; i < 3; ++i) o[9 + i] = T[i];
}

__global__ void __launch_bounds__(ransac::MATCH_TILE) k_pnp_score(const double* __restrict__ m, const double* __restrict__ Ph,
                                                                   const float* __restrict__ K, int* __restrict__ counts, int B, int num,
                                                                   int hyp, double thr2) {
  ransac::score_body<PnpModel>(load_cam(K, blockIdx.y % B), m, Ph, counts, num, hyp, thr2);
}

// v[0..LM_SUMS) summed over the block in an order fixed by thread index: lanes of a wave by shuffles (a tree over the lane
// index), the waves' partials through LDS; thread 0 then holds the totals in v.  red: LM_SUMS * PNP_WAVES doubles.
__device__ void block_sum_lm(double* v, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < pnp::LM_SUMS; ++i) {
    double x = v[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    if (lane == 0) red[i * PNP_WAVES + wave] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < pnp::LM_SUMS; ++i)
      v[i] = (red[i * PNP_WAVES] + red[i * PNP_WAVES + 1]) + (red[i * PNP_WAVES + 2] + red[i * PNP_WAVES + 3]);
  }
}

// the state of one refinement, kept by thread 0 in LDS: the pose, the candidate every thread evaluates, the sums at the pose
struct LmState {
  double pose[12];          // R row-major, T
  double cand[12];
  double sums[pnp::LM_SUMS];
  double lam;
  double A[42];
};

// every thread: its matches' share of the LM sums at st.cand; thread 0 receives the totals in acc
__device__ void lm_sums_at_candidate(const pnp::Cam& cam, const LmState& st, const double* __restrict__ mp, const int* __restrict__ w,
                                     int num, double* acc, double* red) {
  double R[9], T[3];
  for (int i = 0; i < 9; ++i) R[i] = st.cand[i];
  for (int i = 0; i < 3; ++i) T[i] = st.cand[9 + i];
#pragma unroll
  for (int i = 0; i < pnp::LM_SUMS; ++i) acc[i] = 0.0;
  for (int j = threadIdx.x; j < num; j += THREADS) {
    double pt[PnpModel::PT];
    for (int i = 0; i < PnpModel::PT; ++i) pt[i] = mp[static_cast<long>(j) * PnpModel::PT + i];
    pnp::lm_accumulate(cam, R, T, pt, static_cast<double>(w[j]), acc);
  }
  block_sum_lm(acc, red);
}

// _pnp_refine over the matches of weight 1 from the pose in st.pose, iters iterations; st.pose receives the result.
// Each iteration reduces the LM_SUMS sums at the candidate pose once: its cost decides the accept test, its H and g serve the
// next iteration if it is accepted.
__device__ void refine(const pnp::Cam& cam, LmState& st, const double* __restrict__ mp, const int* __restrict__ w, int num, int iters,
                       double* red) {
  double acc[pnp::LM_SUMS];
  if (threadIdx.x == 0) {
    for (int i = 0; i < 12; ++i) st.cand[i] = st.pose[i];
    st.lam = 1e-3;
  }
  __syncthreads();
  lm_sums_at_candidate(cam, st, mp, w, num, acc, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < pnp::LM_SUMS; ++i) st.sums[i] = acc[i];
  }
  for (int it = 0; it < iters; ++it) {
    if (threadIdx.x == 0) {
      double step[6];
      pnp::lm_solve(st.sums, st.lam, st.A, step);
      pnp::apply_step(step, st.pose, st.pose + 9, st.cand, st.cand + 9);
    }
    __syncthreads();          // the candidate is published; red is free again (thread 0 read it before this barrier)
    lm_sums_at_candidate(cam, st, mp, w, num, acc, red);
    if (threadIdx.x == 0) {
      const bool ok = acc[27] < st.sums[27];          // cn < cost: false for NaN
      if (ok) {
        for (int i = 0; i < 12; ++i) st.pose[i] = st.cand[i];
#pragma unroll
        for (int i = 0; i < pnp::LM_SUMS; ++i) st.sums[i] = acc[i];
      }
      double lam = ok ? st.lam * 0.3 : st.lam * 5.0;
      lam = lam < 1e-9 ? 1e-9 : (lam > 1e6 ? 1e6 : lam);
      st.lam = lam;
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(THREADS) k_pnp_consensus(const double* __restrict__ m, const double* __restrict__ Ph,
                                                            const int* __restrict__ counts, const float* __restrict__ K,
                                                            int* __restrict__ w1, int* __restrict__ w2, double* __restrict__ P64,
                                                            float* __restrict__ P32, int* __restrict__ info, int B, int num, int hyp,
                                                            int iters, double thr2) {
  __shared__ LmState st;
  __shared__ double red[pnp::LM_SUMS * PNP_WAVES];
  const int plane = blockIdx.x;
  const pnp::Cam cam = load_cam(K, plane % B);
  const double* mp = m + static_cast<long>(plane) * num * PnpModel::PT;
  // iters iterations over the first set, max(iters / 2, 1) over the second; then (T, log R)
  ransac::consensus_body<PnpModel>(
      cam, m, Ph, counts, w1, w2, info, num, hyp, thr2, st.pose,
      [&](const int* w, int fit) { refine(cam, st, mp, w, num, fit == 0 ? iters : (iters / 2 > 1 ? iters / 2 : 1), red); },
      [&]() {
        if (threadIdx.x == 0) {
          double R[9], v[3];
          for (int i = 0; i < 9; ++i) R[i] = st.pose[i];
          pnp::so3_log(R, v);
          for (int i = 0; i < 3; ++i) {
            P64[plane * 6 + i] = st.pose[9 + i];
            P32[plane * 6 + i] = static_cast<float>(st.pose[9 + i]);
            P64[plane * 6 + 3 + i] = v[i];
            P32[plane * 6 + 3 + i] = static_cast<float>(v[i]);
          }
        }
      });
}

// ---------------------------------------------------------------------------------------------- loss
// pose rows are sample-major (b*2 + d), P32 planes direction-major (d*B + b)
__global__ void k_pnp_loss_fwd(const float* __restrict__ pose, const float* __restrict__ P32, float* __restrict__ loss, int B, float beta) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float term[2];
  for (int d = 0; d < 2; ++d) {
    const float* p = pose + (b * 2 + d) * 6;
    const float* q = P32 + (d * B + b) * 6;
    float s = 0.f;
    for (int i = 0; i < 3; ++i) s += fabsf(q[i] - p[i]) + beta * fabsf(q[3 + i] - p[3 + i]);
    term[d] = s / 3.f;
  }
  loss[b] = term[0] + term[1];
}

__global__ void k_pnp_loss_bwd(const float* __restrict__ pose, const float* __restrict__ P32, const float* __restrict__ gloss,
                               float* __restrict__ gpose, int B, float beta) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * B) return;
  const int b = t >> 1, d = t & 1;
  const float* p = pose + t * 6;
  const float* q = P32 + (d * B + b) * 6;
  const float g = gloss[b] / 3.f;
  for (int i = 0; i < 6; ++i) {
    const float df = p[i] - q[i];
    const float sg = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);      // sign(0) = 0, as F.l1_loss has it
    gpose[t * 6 + i] = g * sg * (i < 3 ? 1.f : beta);
  }
}

}  // namespace
}  // namespace dfe

using namespace dfe;

extern "C" long dfe_pnp_ws_bytes(int B, int num, int hyp) {
  if (B <= 0 || num <= 0 || hyp <= 0) return 0;
  return ransac::ws_offsets(PnpModel::PT, PnpModel::HP, B, num, hyp).bytes;
}

extern "C" int dfe_pnp_ransac(const float* flow_bwd, const float* flow_fwd, const float* disp_t, const int* idx, const long long* pick,
                              const int* sets, const float* K, const float* K_inv, double* P64, float* P32, int* info, void* ws,
                              int B, int H, int W, int k, int num, int hyp, int iters, double thresh, void* stream) {
  const bool have_all = flow_bwd && flow_fwd && disp_t && idx && pick && sets && K && K_inv && P64 && P32 && info && ws;
  if (have_all && iters < 1) return DFE_ERR_DIMS;
  const int rc = ransac::check_args(have_all, B, H, W, k, num, hyp, PnpModel::MIN, ws, P64);
  if (rc != DFE_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const ransac::Ws w = ransac::ws_sections(ws, ransac::ws_offsets(PnpModel::PT, PnpModel::HP, B, num, hyp));
  const double thr2 = thresh * thresh;
  return ransac::launch_all(
      w.counts, B, num, hyp, PNP_HYP_THREADS, st,
      [&](dim3 g) { k_pnp_points<<<g, THREADS, 0, st>>>(flow_bwd, flow_fwd, disp_t, idx, pick, K_inv, w.m, B, H, W, k, num); },
      [&](dim3 g) { k_pnp_hyp<<<g, PNP_HYP_THREADS, 0, st>>>(w.m, sets, K, w.hyps, B, num, hyp); },
      [&](dim3 g) { k_pnp_score<<<g, ransac::MATCH_TILE, 0, st>>>(w.m, w.hyps, K, w.counts, B, num, hyp, thr2); },
      [&](dim3 g) {
        k_pnp_consensus<<<g, THREADS, 0, st>>>(w.m, w.hyps, w.counts, K, w.w1, w.w2, P64, P32, info, B, num, hyp, iters, thr2);
      });
}

extern "C" int dfe_pnp_loss_fwd(const float* pose, const float* P32, float* loss, int B, float beta, void* stream) {
  if (!pose || !P32 || !loss) return DFE_ERR_NULL;
  if (B <= 0 || B > 16384) return DFE_ERR_DIMS;
  k_pnp_loss_fwd<<<(B + 63) / 64, 64, 0, static_cast<hipStream_t>(stream)>>>(pose, P32, loss, B, beta);
  return launch_status();
}

extern "C" int dfe_pnp_loss_bwd(const float* pose, const float* P32, const float* gloss, float* gpose, int B, float beta, void* stream) {
  if (!pose || !P32 || !gloss || !gpose) return DFE_ERR_NULL;
  if (B <= 0 || B > 16384) return DFE_ERR_DIMS;
  k_pnp_loss_bwd<<<(2 * B + 63) / 64, 64, 0, static_cast<hipStream_t>(stream)>>>(pose, P32, gloss, gpose, B, beta);
  return launch_status();
}
