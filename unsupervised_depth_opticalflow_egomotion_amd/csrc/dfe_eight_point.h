// Per-plane arithmetic of the eight-point term (ops_eight_point.hip): Hartley normalisation, a row of the 9-column system, the
// null direction of the 9x9 normal matrix and rank 2 (the two iterations of dfe_jacobi.h), un-normalisation, OpenCV's
// residual.  All in double, as GeometrySolvers.compute_fundmental_mat evaluates it; host and device compile the same text.
// Every loop has a fixed upper bound: with NaN or inf in the matrix the sweeps run out and the result is non-finite.
#pragma once
#include <hip/hip_runtime.h>
#include "dfe_jacobi.h"

namespace dfe {
namespace ep {

constexpr int JACOBI9_SWEEPS = 20;     // cyclic sweeps over the 36 pairs; convergence is quadratic, 6-9 sweeps in practice
constexpr double SQRT2 = 1.4142135623730951;    // 2.0 ** 0.5

struct Norm { double s, tx, ty; };     // T = [[s, 0, tx], [0, s, ty], [0, 0, 1]], tx = -s cx, ty = -s cy

// _weighted_hartley after its sums: centroid (cx, cy), mean distance to it
__host__ __device__ inline Norm make_norm(double cx, double cy, double dmean) {
  const double s = SQRT2 / (dmean + 1e-12);
  return Norm{s, -s * cx, -s * cy};
}

// row (i, j) = p2_i * p1_j of the match (x1, y1, x2, y2) under the two normalisations
__host__ __device__ inline void row9(const Norm& n1, const Norm& n2, double x1, double y1, double x2, double y2, double* a) {
  const double p1[3] = {n1.s * x1 + n1.tx, n1.s * y1 + n1.ty, 1.0};
  const double p2[3] = {n2.s * x2 + n2.tx, n2.s * y2 + n2.ty, 1.0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) a[3 * i + j] = p2[i] * p1[j];
}

// F <- F with its smallest singular value set to zero: with the columns of G = F W orthogonal (F = G W^T), the column of the
// smallest norm is sigma_3 u_3 and that column of W is v_3.
__host__ __device__ inline void rank2(double* F) {
  double G[9], W[9];
  for (int i = 0; i < 9; ++i) G[i] = F[i];
  orthogonalize3(G, W);
  double nrm[3];
  for (int j = 0; j < 3; ++j) nrm[j] = G[j] * G[j] + G[3 + j] * G[3 + j] + G[6 + j] * G[6 + j];
  // the column of the smallest norm, picked by comparisons (a run-time column index would put G and W into private memory)
  const bool m1 = nrm[1] < nrm[0], m2 = nrm[2] < (m1 ? nrm[1] : nrm[0]);
  for (int i = 0; i < 3; ++i) {
    const double g = m2 ? G[3 * i + 2] : (m1 ? G[3 * i + 1] : G[3 * i]);
    for (int j = 0; j < 3; ++j) F[3 * i + j] -= g * (m2 ? W[3 * j + 2] : (m1 ? W[3 * j + 1] : W[3 * j]));
  }
}

// _eight_point after its normal matrix M (destroyed; V: 81 more doubles; both with element stride S): null direction, rank 2,
// F = T2^T Fn T1
__host__ __device__ inline void solve_normal(double* M, double* V, int S, const Norm& n1, const Norm& n2, double* F) {
  const int col = jacobi_sym<9>(M, V, S, JACOBI9_SWEEPS);
  double Fn[9], X[9];
  for (int i = 0; i < 9; ++i) Fn[i] = V[(9 * i + col) * S];
  rank2(Fn);
  for (int j = 0; j < 3; ++j) {
    X[j] = n2.s * Fn[j];
    X[3 + j] = n2.s * Fn[3 + j];
    X[6 + j] = n2.tx * Fn[j] + n2.ty * Fn[3 + j] + Fn[6 + j];
  }
  for (int i = 0; i < 3; ++i) {
    F[3 * i] = n1.s * X[3 * i];
    F[3 * i + 1] = n1.s * X[3 * i + 1];
    F[3 * i + 2] = n1.tx * X[3 * i] + n1.ty * X[3 * i + 1] + X[3 * i + 2];
  }
}

// _epipolar_residual <= thr2: the larger of the squared distances of x2 to F x1 and of x1 to F^T x2 (OpenCV's computeError, the
// 1e-300 guards).  A non-finite residual is an outlier: both comparisons are false for NaN.
__host__ __device__ inline bool inlier(const double* F, double x1, double y1, double x2, double y2, double thr2) {
  const double a2 = F[0] * x1 + F[1] * y1 + F[2], b2 = F[3] * x1 + F[4] * y1 + F[5], c2 = F[6] * x1 + F[7] * y1 + F[8];
  const double a1 = F[0] * x2 + F[3] * y2 + F[6], b1 = F[1] * x2 + F[4] * y2 + F[7];
  const double n = x2 * a2 + y2 * b2 + c2;
  const double d2 = n * n / (a2 * a2 + b2 * b2 + 1e-300);
  const double d1 = n * n / (a1 * a1 + b1 * b1 + 1e-300);
  return d1 <= thr2 && d2 <= thr2;
}

}  // namespace ep
}  // namespace dfe
