// Per-plane arithmetic of the PnP term (ops_pnp.hip): the back-projected point, the six-point DLT's 12x12 normal matrix and its
// null direction (dfe_jacobi.h's cyclic Jacobi), the projection onto SO(3) (its one-sided Jacobi on the 3x3, as ep::rank2 uses
// it), the reprojection test, one match's share of the
// Levenberg-Marquardt sums, the 6x6 solve, exp and log on SO(3).  All in double, as GeometrySolvers.pnp evaluates it; host and
// device compile the same text.  Every loop has a fixed upper bound: with NaN or inf the sweeps run out and the result is
// non-finite.
#pragma once
#include <hip/hip_runtime.h>
#include "dfe_jacobi.h"

namespace dfe {
namespace pnp {

constexpr int JACOBI12_SWEEPS = 24;    // cyclic sweeps over the 66 pairs; 8-11 in practice
constexpr int LM_SUMS = 28;            // 21 of H (upper triangle, row-major), 6 of g, the cost

struct Cam { double fx, fy, cx, cy; };     // K[0][0], K[1][1], K[0][2], K[1][2] as GeometrySolvers.pnp reads them

// inverse of a row-major 3x3 (adjugate over the determinant): the hypotheses' normalised image coordinates
__host__ __device__ inline void inverse3(const double* K, double* Ki) {
  const double c0 = K[4] * K[8] - K[5] * K[7], c1 = K[5] * K[6] - K[3] * K[8], c2 = K[3] * K[7] - K[4] * K[6];
  const double det = K[0] * c0 + K[1] * c1 + K[2] * c2;
  Ki[0] = c0 / det; Ki[1] = (K[2] * K[7] - K[1] * K[8]) / det; Ki[2] = (K[1] * K[5] - K[2] * K[4]) / det;
  Ki[3] = c1 / det; Ki[4] = (K[0] * K[8] - K[2] * K[6]) / det; Ki[5] = (K[2] * K[3] - K[0] * K[5]) / det;
  Ki[6] = c2 / det; Ki[7] = (K[1] * K[6] - K[0] * K[7]) / det; Ki[8] = (K[0] * K[4] - K[1] * K[3]) / det;
}

// entry (r, c) of a symmetric 4x4 kept as its 10 upper-triangle entries, row-major
__host__ __device__ constexpr int sym4(int r, int c) { return r <= c ? (r * (7 - r)) / 2 + c : (c * (7 - c)) / 2 + r; }

// A^T A of the DLT system [Xh, 0, -u Xh; 0, Xh, -v Xh] over the set's points from its four 4x4 blocks: S = sum Xh Xh^T,
// Su = sum u Xh Xh^T, Sv = sum v Xh Xh^T, Sq = sum (u^2 + v^2) Xh Xh^T.  M: 144 elements with stride S_.
__host__ __device__ inline void dlt_normal(const double* S, const double* Su, const double* Sv, const double* Sq, double* M, int S_) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int e = sym4(r, c);
      M[(12 * r + c) * S_] = S[e];
      M[(12 * r + 4 + c) * S_] = 0.0;
      M[(12 * r + 8 + c) * S_] = -Su[e];
      M[(12 * (4 + r) + c) * S_] = 0.0;
      M[(12 * (4 + r) + 4 + c) * S_] = S[e];
      M[(12 * (4 + r) + 8 + c) * S_] = -Sv[e];
      M[(12 * (8 + r) + c) * S_] = -Su[e];
      M[(12 * (8 + r) + 4 + c) * S_] = -Sv[e];
      M[(12 * (8 + r) + 8 + c) * S_] = Sq[e];
    }
}

// _pnp_hypotheses after the null direction P [3,4]: R = U W^T sign(det), T = P[:, 3] sign / mean(singular values), from the SVD of
// P[:, :3] by a one-sided Jacobi: the columns of G = A W are made orthogonal, their norms are the singular values.
__host__ __device__ inline void pose_from_dlt(const double* P, double* R, double* T) {
  double G[9], W[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) G[3 * i + j] = P[4 * i + j];
  orthogonalize3(G, W);
  double sv[3];
  for (int j = 0; j < 3; ++j) sv[j] = sqrt(G[j] * G[j] + G[3 + j] * G[3 + j] + G[6 + j] * G[6 + j]);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      R[3 * i + j] = (G[3 * i] / sv[0] * W[3 * j] + G[3 * i + 1] / sv[1] * W[3 * j + 1]) + G[3 * i + 2] / sv[2] * W[3 * j + 2];
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  const double sign = det < 0.0 ? -1.0 : 1.0;
  double mean = (sv[0] + sv[1] + sv[2]) / 3.0;
  mean = mean < 1e-300 ? 1e-300 : mean;          // clamp_min: NaN stays NaN
  for (int i = 0; i < 9; ++i) R[i] *= sign;
  for (int i = 0; i < 3; ++i) T[i] = P[4 * i + 3] * (sign / mean);
}

// Y = R X + T, the sums in index order
__host__ __device__ inline void transform(const double* R, const double* T, const double* X, double* Y) {
  for (int i = 0; i < 3; ++i) Y[i] = ((X[0] * R[3 * i] + X[1] * R[3 * i + 1]) + X[2] * R[3 * i + 2]) + T[i];
}

// the reprojection residual (eu, ev) with pnp's clamp_min(1e-9) on z; zc receives the clamped depth
__host__ __device__ inline void residual(const Cam& cam, const double* Y, double x2, double y2, double* eu, double* ev, double* zc) {
  const double z = Y[2] < 1e-9 ? 1e-9 : Y[2];    // NaN stays NaN, as torch.clamp_min keeps it
  *zc = z;
  *eu = cam.fx * Y[0] / z + cam.cx - x2;
  *ev = cam.fy * Y[1] / z + cam.cy - y2;
}

// eu^2 + ev^2 <= thr2 and z > 0; a non-finite residual is an outlier (both comparisons are false for NaN)
__host__ __device__ inline bool inlier(const Cam& cam, const double* R, const double* T, const double* m, double thr2) {
  double Y[3], eu, ev, zc;
  transform(R, T, m, Y);
  residual(cam, Y, m[3], m[4], &eu, &ev, &zc);
  return (eu * eu + ev * ev) <= thr2 && Y[2] > 0.0;
}

// One match's share of _pnp_refine's sums at the pose (R, T) with weight w (0 or 1): acc[0..20] += the upper triangle of
// J^T J, acc[21..26] += J^T r, acc[27] += r.r, with J = d(u, v) / d(omega, T) under R <- exp([omega]x) R.
__host__ __device__ inline void lm_accumulate(const Cam& cam, const double* R, const double* T, const double* m, double w, double* acc) {
  double Y[3], ru, rv, z;
  transform(R, T, m, Y);
  residual(cam, Y, m[3], m[4], &ru, &rv, &z);
  ru *= w; rv *= w;
  const double zi = 1.0 / z;
  const double du0 = cam.fx * zi, du2 = -cam.fx * Y[0] * zi * zi;
  const double dv1 = cam.fy * zi, dv2 = -cam.fy * Y[1] * zi * zi;
  const double P0 = Y[0] - T[0], P1 = Y[1] - T[1], P2 = Y[2] - T[2];
  // -(du [P]x), du and -(dv [P]x), dv
  const double Ju[6] = {-(-du2 * P1) * w, -(-du0 * P2 + du2 * P0) * w, -(du0 * P1) * w, du0 * w, 0.0 * w, du2 * w};
  const double Jv[6] = {-(dv1 * P2 - dv2 * P1) * w, -(dv2 * P0) * w, -(-dv1 * P0) * w, 0.0 * w, dv1 * w, dv2 * w};
  int e = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) acc[e++] += Ju[r] * Ju[c] + Jv[r] * Jv[c];
#pragma unroll
  for (int r = 0; r < 6; ++r) acc[21 + r] += Ju[r] * ru + Jv[r] * rv;
  acc[27] += ru * ru + rv * rv;
}

// (H + lam diag(max(diag H, 1e-12))) step = -g by Gaussian elimination with partial pivoting.  A: 42 doubles of LDS (6 rows of 7),
// indexed at run time.  sums: the LM_SUMS of lm_accumulate.  A singular system gives a non-finite step, which the accept test rejects.
__host__ __device__ inline void lm_solve(const double* sums, double lam, double* A, double* step) {
  int e = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c) { A[7 * r + c] = sums[e]; A[7 * c + r] = sums[e]; ++e; }
  for (int r = 0; r < 6; ++r) {
    const double d = A[8 * r];
    A[8 * r] = d + lam * (d < 1e-12 ? 1e-12 : d);
    A[7 * r + 6] = -sums[21 + r];
  }
  for (int c = 0; c < 6; ++c) {
    int piv = c;
    for (int r = c + 1; r < 6; ++r)
      if (fabs(A[7 * r + c]) > fabs(A[7 * piv + c])) piv = r;
    if (piv != c)
      for (int k = 0; k < 7; ++k) { const double t = A[7 * c + k]; A[7 * c + k] = A[7 * piv + k]; A[7 * piv + k] = t; }
    const double inv = 1.0 / A[8 * c];
    for (int r = c + 1; r < 6; ++r) {
      const double f = A[7 * r + c] * inv;
      for (int k = c; k < 7; ++k) A[7 * r + k] -= f * A[7 * c + k];
    }
  }
  for (int r = 5; r >= 0; --r) {
    double s = A[7 * r + 6];
    for (int k = r + 1; k < 6; ++k) s -= A[7 * r + k] * A[7 * k + 6];
    A[7 * r + 6] = s / A[8 * r];
  }
  for (int r = 0; r < 6; ++r) step[r] = A[7 * r + 6];
}

// Rn = exp([w]x) R (_so3_exp: Rodrigues, the series below 1e-6), Tn = T + dT
__host__ __device__ inline void apply_step(const double* step, const double* R, const double* T, double* Rn, double* Tn) {
  const double w0 = step[0], w1 = step[1], w2 = step[2];
  const double th = sqrt(((w0 * w0 + w1 * w1) + w2 * w2) + 1e-30);
  const double a = th > 1e-6 ? sin(th) / th : 1.0 - th * th / 6.0;
  const double b = th > 1e-6 ? (1.0 - cos(th)) / (th * th) : 0.5 - th * th / 24.0;
  const double Kx[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
  double E[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double k2 = (Kx[3 * i] * Kx[j] + Kx[3 * i + 1] * Kx[3 + j]) + Kx[3 * i + 2] * Kx[6 + j];
      E[3 * i + j] = ((i == j ? 1.0 : 0.0) + a * Kx[3 * i + j]) + b * k2;
    }
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
    Tn[i] = T[i] + step[3 + i];
  }
}

// _so3_log: rotation -> axis-angle (angles below pi)
__host__ __device__ inline void so3_log(const double* R, double* v) {
  double c = (R[0] + R[4] + R[8] - 1.0) / 2.0;
  c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
  const double th = acos(c);
  double sn = sin(th);
  sn = sn < 1e-30 ? 1e-30 : sn;
  const double k = th > 1e-6 ? th / sn : 1.0 + th * th / 6.0;
  v[0] = (R[7] - R[5]) / 2.0 * k;
  v[1] = (R[2] - R[6]) / 2.0 * k;
  v[2] = (R[3] - R[1]) / 2.0 * k;
}

}  // namespace pnp
}  // namespace dfe
