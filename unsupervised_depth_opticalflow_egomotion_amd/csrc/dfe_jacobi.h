// The two Jacobi iterations of the eight-point and PnP terms (dfe_eight_point.h, dfe_pnp.h): the eigenvectors of a symmetric
// N x N matrix by cyclic rotations, and the one-sided iteration that makes the columns of a 3x3 orthogonal.  All in double; host
// and device compile the same text.  Every loop has a fixed upper bound: with NaN or inf in the matrix the sweeps run out and the
// result is non-finite.
#pragma once
#include <hip/hip_runtime.h>

namespace dfe {

constexpr int JACOBI3_SWEEPS = 12;

// Eigenvectors of the symmetric N x N matrix A (row-major, both halves stored; destroyed) by at most `sweeps` cyclic sweeps of
// Jacobi rotations; V receives them as columns.  Element i of either matrix lives at [i * S]: the kernels keep them in LDS,
// interleaved over the threads of a block (S = threads) or dense (S = 1) -- never in private memory, which would index them
// dynamically through scratch.  Returns the column of the smallest eigenvalue.
template <int N>
__host__ __device__ inline int jacobi_sym(double* A, double* V, int S, int sweeps) {
  for (int i = 0; i < N * N; ++i) V[i * S] = (i % (N + 1) == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < sweeps; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (int i = 0; i < N * N; ++i) {
      const double v = A[i * S] * A[i * S];
      tot += v;
      if (i % (N + 1) != 0) off += v;
    }
    if (off <= 1e-32 * tot) break;          // false for NaN: the sweeps run out
    for (int p = 0; p < N - 1; ++p)
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[(N * p + q) * S];
        if (apq == 0.0) continue;
        const double theta = (A[(N + 1) * q * S] - A[(N + 1) * p * S]) / (2.0 * apq);
        const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        A[(N + 1) * p * S] -= t * apq;
        A[(N + 1) * q * S] += t * apq;
        A[(N * p + q) * S] = 0.0;
        A[(N * q + p) * S] = 0.0;
        for (int k = 0; k < N; ++k) {
          if (k != p && k != q) {
            const double akp = A[(N * k + p) * S], akq = A[(N * k + q) * S];
            const double np = c * akp - s * akq, nq = s * akp + c * akq;
            A[(N * k + p) * S] = np; A[(N * p + k) * S] = np;
            A[(N * k + q) * S] = nq; A[(N * q + k) * S] = nq;
          }
          const double vkp = V[(N * k + p) * S], vkq = V[(N * k + q) * S];
          V[(N * k + p) * S] = c * vkp - s * vkq;
          V[(N * k + q) * S] = s * vkp + c * vkq;
        }
      }
  }
  int best = 0;
  for (int i = 1; i < N; ++i)
    if (A[(N + 1) * i * S] < A[(N + 1) * best * S]) best = i;
  return best;
}

// One-sided Jacobi on a row-major 3x3: G <- G W with W orthogonal (W starts as the identity here) and the columns of G
// orthogonal, so that the input is G W^T, the columns' norms are its singular values and the columns of W its right singular
// vectors.  Indexed by constants only once unrolled: G and W stay in registers.
__host__ __device__ inline void orthogonalize3(double* G, double* W) {
  for (int i = 0; i < 9; ++i) W[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < JACOBI3_SWEEPS; ++sweep) {
    int rotated = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int k = 0; k < 3; ++k) {
          alpha += G[3 * k + p] * G[3 * k + p];
          beta += G[3 * k + q] * G[3 * k + q];
          gamma += G[3 * k + p] * G[3 * k + q];
        }
        if (!(fabs(gamma) > 1e-17 * sqrt(alpha * beta))) continue;       // orthogonal already (or NaN)
        ++rotated;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int k = 0; k < 3; ++k) {
          const double gp = G[3 * k + p], gq = G[3 * k + q];
          G[3 * k + p] = c * gp - s * gq;
          G[3 * k + q] = s * gp + c * gq;
          const double wp = W[3 * k + p], wq = W[3 * k + q];
          W[3 * k + p] = c * wp - s * wq;
          W[3 * k + q] = s * wp + c * wq;
        }
      }
    if (!rotated) break;
  }
}

}  // namespace dfe
