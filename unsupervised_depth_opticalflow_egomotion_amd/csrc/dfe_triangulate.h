// Per-point arithmetic of the triangulation term (geometry_solvers.GeometrySolvers.midpoint_triangulate, reproject and
// register_depth's grid_sample; the reference: model_geometry.py:569-651), shared by the forward and backward kernels of
// ops_triangulate.hip.  The expressions are the reference's, with its epsilons, evaluated in double: the mid-point of two
// nearly parallel rays loses most of fp32's digits, and there are only 2 * B * num points, so the wider format costs nothing.
//
// tri_point is a template over the scalar: double for values, Dual for one forward-mode tangent (the backward kernel runs
// it once per tangent direction -- u, v and the twelve entries of T34 -- instead of a hand-derived mid-point Jacobian).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>

namespace dfe {
namespace tri {

constexpr double EPS = 1e-12;

struct Dual { double v, d; };
__host__ __device__ __forceinline__ Dual operator+(Dual a, Dual b) { return Dual{a.v + b.v, a.d + b.d}; }
__host__ __device__ __forceinline__ Dual operator-(Dual a, Dual b) { return Dual{a.v - b.v, a.d - b.d}; }
__host__ __device__ __forceinline__ Dual operator*(Dual a, Dual b) { return Dual{a.v * b.v, a.d * b.v + a.v * b.d}; }
__host__ __device__ __forceinline__ Dual operator/(Dual a, Dual b) {
  const double q = a.v / b.v;
  return Dual{q, (a.d - q * b.d) / b.v};
}
__host__ __device__ __forceinline__ Dual operator-(Dual a) { return Dual{-a.v, -a.d}; }
__host__ __device__ __forceinline__ Dual root(Dual a) {
  const double r = sqrt(a.v);
  return Dual{r, r > 0.0 ? a.d / (2.0 * r) : 0.0};
}
__host__ __device__ __forceinline__ double root(double a) { return sqrt(a); }
__host__ __device__ __forceinline__ void lift(double c, double& out) { out = c; }
__host__ __device__ __forceinline__ void lift(double c, Dual& out) { out = Dual{c, 0.0}; }
template <class S> __host__ __device__ __forceinline__ S cst(double c) { S s; lift(c, s); return s; }

template <class S> __host__ __device__ __forceinline__ void cross3(const S* a, const S* b, S* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
template <class S> __host__ __device__ __forceinline__ S dot3(const S* a, const S* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// unit ray and origin of one view: RT = K^-1 P, Rt = RT[:, :3]^T, d = Rt K^-1 (x, y, 1), ray = d / (|d| + eps), origin = -Rt RT[:, 3]
template <class S>
__host__ __device__ __forceinline__ void view_ray(const double* Kinv, const S* P, S x, S y, S* ray, S* org) {
  S RT[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c)
      RT[r * 4 + c] = (cst<S>(Kinv[r * 3 + 0]) * P[0 * 4 + c] + cst<S>(Kinv[r * 3 + 1]) * P[1 * 4 + c]) + cst<S>(Kinv[r * 3 + 2]) * P[2 * 4 + c];
  S q[3];
  for (int r = 0; r < 3; ++r) q[r] = (cst<S>(Kinv[r * 3 + 0]) * x + cst<S>(Kinv[r * 3 + 1]) * y) + cst<S>(Kinv[r * 3 + 2]);
  S d[3];
  for (int r = 0; r < 3; ++r) {
    d[r] = (RT[0 * 4 + r] * q[0] + RT[1 * 4 + r] * q[1]) + RT[2 * 4 + r] * q[2];
    org[r] = -((RT[0 * 4 + r] * RT[0 * 4 + 3] + RT[1 * 4 + r] * RT[1 * 4 + 3]) + RT[2 * 4 + r] * RT[2 * 4 + 3]);
  }
  const S nrm = root(dot3(d, d)) + cst<S>(EPS);
  for (int r = 0; r < 3; ++r) ray[r] = d[r] / nrm;
}

// p = P (X, 1): pixel (p0, p1) / (p2 + eps) and depth p2
template <class S> __host__ __device__ __forceinline__ void reproject(const S* P, const S* X, S* out) {
  S p[3];
  for (int r = 0; r < 3; ++r) p[r] = ((P[r * 4 + 0] * X[0] + P[r * 4 + 1] * X[1]) + P[r * 4 + 2] * X[2]) + P[r * 4 + 3];
  const S zz = p[2] + cst<S>(EPS);
  out[0] = p[0] / zz;
  out[1] = p[1] / zz;
  out[2] = p[2];
}

// The match (x, y, x + u, y + v) under P1 = K [I | 0] and P2 = K T (T row-major 3 x 4) ->
// out = (c1x, c1y, z1, c2x, c2y, z2): the mid-point's reprojection into both views and its two depths.
template <class S>
__host__ __device__ __forceinline__ void tri_point(const double* K, const double* Kinv, const S* T, double x, double y, S u, S v, S* out) {
  S P1[12], P2[12];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      P1[r * 4 + c] = cst<S>(c < 3 ? K[r * 3 + c] : 0.0);
      P2[r * 4 + c] = (cst<S>(K[r * 3 + 0]) * T[0 * 4 + c] + cst<S>(K[r * 3 + 1]) * T[1 * 4 + c]) + cst<S>(K[r * 3 + 2]) * T[2 * 4 + c];
    }
  S r0[3], o0[3], r1[3], o1[3];
  view_ray(Kinv, P1, cst<S>(x), cst<S>(y), r0, o0);
  view_ray(Kinv, P2, cst<S>(x) + u, cst<S>(y) + v, r1, o1);
  S cr[3], base[3], t1[3], t2[3];
  cross3(r0, r1, cr);
  const S denom = cst<S>(1.0) / (dot3(cr, cr) + cst<S>(EPS));
  for (int r = 0; r < 3; ++r) base[r] = o1[r] - o0[r];
  cross3(base, r1, t1);
  cross3(base, r0, t2);
  const S a1 = dot3(t1, cr) * denom, a2 = dot3(t2, cr) * denom;
  S X[3];
  for (int r = 0; r < 3; ++r) X[r] = ((o0[r] + a1 * r0[r]) + (o1[r] + a2 * r1[r])) / cst<S>(2.0);
  reproject(P1, X, out);
  reproject(P2, X, out + 3);
}

// One axis of grid_sample(padding_mode="reflection") for the pixel coordinate c that register_depth normalises with
// g = 2 c / (size - 1) - 1: the un-normalised, reflected and clipped coordinate and its derivative with respect to c.
__host__ __device__ __forceinline__ void reflect_axis(double c, int size, int ac, double& r, double& drdc) {
  const double g = 2.0 * c / (size - 1.0) - 1.0;
  double ix, slope, lo, span;
  if (ac) { ix = (g + 1.0) / 2.0 * (size - 1.0); slope = 1.0; lo = 0.0; span = size - 1.0; }
  else { ix = ((g + 1.0) * size - 1.0) / 2.0; slope = size / (size - 1.0); lo = -0.5; span = size; }
  if (!(span > 0.0) || !(fabs(ix) < 1e15)) { r = 0.0; drdc = 0.0; return; }   // a one-pixel axis, or a NaN / huge coordinate
  double t = ix - lo, sgn = 1.0;
  if (t < 0.0) { t = -t; sgn = -1.0; }
  const double flips = floor(t / span), extra = t - flips * span;
  if (fmod(flips, 2.0) == 0.0) r = extra + lo;
  else { r = span - extra + lo; sgn = -sgn; }
  if (r < 0.0) { r = 0.0; sgn = 0.0; }
  if (r > size - 1.0) { r = size - 1.0; sgn = 0.0; }
  drdc = sgn * slope;
}

struct Sample {
  double val, dcx, dcy;   // the interpolated value and its derivatives with respect to the pixel coordinate (cx, cy)
  int off[4];             // plane offsets of the taps nw, ne, sw, se (always inside the plane)
  double w[4];            // their weights; 0 where the tap is outside
};

__host__ __device__ __forceinline__ Sample sample_reflect(const float* __restrict__ plane, double cx, double cy, int H, int W, int ac) {
  double rx, ry, sx, sy;
  reflect_axis(cx, W, ac, rx, sx);
  reflect_axis(cy, H, ac, ry, sy);
  const double fx = floor(rx), fy = floor(ry);
  const double wx = rx - fx, wy = ry - fy;
  int x0 = static_cast<int>(fx), y0 = static_cast<int>(fy);
  x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);
  y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0);
  const bool xin = x0 + 1 <= W - 1, yin = y0 + 1 <= H - 1;
  const int x1 = xin ? x0 + 1 : x0, y1 = yin ? y0 + 1 : y0;
  Sample s;
  s.off[0] = y0 * W + x0; s.off[1] = y0 * W + x1; s.off[2] = y1 * W + x0; s.off[3] = y1 * W + x1;
  s.w[0] = (1.0 - wx) * (1.0 - wy);
  s.w[1] = xin ? wx * (1.0 - wy) : 0.0;
  s.w[2] = yin ? (1.0 - wx) * wy : 0.0;
  s.w[3] = (xin && yin) ? wx * wy : 0.0;
  const double nw = plane[s.off[0]], ne = xin ? plane[s.off[1]] : 0.0, sw = yin ? plane[s.off[2]] : 0.0,
               se = (xin && yin) ? plane[s.off[3]] : 0.0;
  s.val = ((nw * s.w[0] + ne * s.w[1]) + sw * s.w[2]) + se * s.w[3];
  s.dcx = ((ne - nw) * (1.0 - wy) + (se - sw) * wy) * sx;
  s.dcy = ((sw - nw) * (1.0 - wx) + (se - ne) * wx) * sy;
  return s;
}

}  // namespace tri
}  // namespace dfe
