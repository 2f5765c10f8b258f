// The triangulation term (model_geometry.py:569-683, call site :939-940) as point kernels: both directions and all samples in
// one launch each.  Point (d, b, j) -- direction d (0: target -> left, 1: target -> right), sample b, draw j < num -- is the
// pixel idx[d*B + b][pick[j]] of the pixel-ordered top-k set (ops_select.hip).  Per-point arithmetic: dfe_triangulate.h.
//
//   dfe_triangulate_fwd    one thread per point: match, mid-point, reprojection, the two reflection-padded bilinear samples
//                          -> rec[(d*B + b)*num + j] = (inter1, z1, inter2, z2), doubles
//   dfe_triangulate_stats  one block per (b, d, view): the two lower medians (radix select over order-preserving 64-bit keys
//                          staged in LDS), scale, scale_adapt's a, the loss of that view; then loss[b] = (L00 + L01) + (L10 + L11)
//   dfe_triangulate_bwd    per-point gradients by forward-mode duals (14 tangents), scattered through dfe_scatter.h's 64-bit
//                          fixed-point accumulators (points repeat); T34's gradient from per-block partial sums added in block order
// Every sum has an order fixed by thread and block index; the only atomics are integer ones: same bits run after run.
#include "dfe_internal.h"
#include "dfe_ransac.h"
#include "dfe_scatter.h"
#include "dfe_triangulate.h"

namespace dfe {
namespace {

constexpr int TRI_THREADS = ransac::THREADS;     // the shared block sum is over a block of this size
constexpr int STATS_DOUBLES = 4;     // per (b, d, view): scale, a, a / (scale + eps), loss

struct TriIn {
  const float* flow[2];     // scale-0 flow of each direction [B,2,H,W]
  const float* disp_t;      // target disparity [B,1,H,W]
  const float* disp_s[2];   // source disparity of each direction [B,1,H,W]
  const float* T34;         // [B,2,12]
  const float* K;           // [B,9]
  const float* Kinv;        // [B,9]
  const int* idx;           // [2*B, k]
  const long long* pick;    // [num]
  int B, H, W, k, num, ac;
};

struct PointCtx {
  double K[9], Kinv[9], T[12];
  double x, y, u, v;
  int pix;
};

__device__ __forceinline__ PointCtx load_point(const TriIn& a, int d, int b, int j) {
  PointCtx c;
  for (int i = 0; i < 9; ++i) { c.K[i] = a.K[b * 9 + i]; c.Kinv[i] = a.Kinv[b * 9 + i]; }
  for (int i = 0; i < 12; ++i) c.T[i] = a.T34[(b * 2 + d) * 12 + i];
  const ransac::Match mt = ransac::load_match(a.flow[d], a.idx, a.pick, d * a.B + b, b, j, a.k, a.H, a.W);
  c.pix = mt.pix;
  c.y = mt.y;
  c.x = mt.x;
  c.u = mt.u;
  c.v = mt.v;
  return c;
}

__global__ void __launch_bounds__(TRI_THREADS) k_tri_fwd(TriIn a, double* __restrict__ rec) {
  const int j = blockIdx.x * TRI_THREADS + threadIdx.x;
  const int plane = blockIdx.y, d = plane / a.B, b = plane - d * a.B;
  if (j >= a.num) return;
  const PointCtx c = load_point(a, d, b, j);
  double o[6];
  tri::tri_point<double>(c.K, c.Kinv, c.T, c.x, c.y, c.u, c.v, o);
  const long HW = static_cast<long>(a.H) * a.W;
  const tri::Sample s1 = tri::sample_reflect(a.disp_t + b * HW, o[0], o[1], a.H, a.W, a.ac);
  const tri::Sample s2 = tri::sample_reflect(a.disp_s[d] + b * HW, o[3], o[4], a.H, a.W, a.ac);
  double* r = rec + (static_cast<long>(plane) * a.num + j) * 4;
  r[0] = s1.val; r[1] = o[2]; r[2] = s2.val; r[3] = o[5];
}

// ---------------------------------------------------------------------------------------------- statistics
// order-preserving key of a double: larger value <=> larger key (NaN above +inf, as torch sorts it)
__device__ __forceinline__ unsigned long long order_key(double v) {
  if (v != v) return ~0ull;
  const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(v));
  return (bits >> 63) ? ~bits : (bits | (1ull << 63));
}
__device__ __forceinline__ double key_value(unsigned long long key) {
  if (key == ~0ull) return __longlong_as_double(0x7ff8000000000000ll);
  const unsigned long long bits = (key >> 63) ? (key & ~(1ull << 63)) : ~key;
  return __longlong_as_double(static_cast<long long>(bits));
}

// The element of ascending rank `rank` among keys[0 .. n) (LDS): eight 8-bit digits from the top, an LDS histogram each.
__device__ unsigned long long select_rank(const unsigned long long* keys, int n, int rank, int* hist, unsigned long long* pick_out) {
  unsigned long long prefix = 0;
  int need = n - rank;            // the need-th largest
  for (int shift = 56; shift >= 0; shift -= 8) {
    for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
    __syncthreads();
    const unsigned long long mask = shift == 56 ? 0ull : (~0ull << (shift + 8));
    int run_bin = -1, run = 0;      // a run of equal digits is counted privately and added once (the leading digits are shared)
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const unsigned long long key = keys[i];
      if ((key & mask) == prefix) {
        const int bin = static_cast<int>((key >> shift) & 255ull);
        if (bin == run_bin) ++run;
        else {
          if (run > 0) atomicAdd(&hist[run_bin], run);
          run_bin = bin;
          run = 1;
        }
      }
    }
    if (run > 0) atomicAdd(&hist[run_bin], run);
    __syncthreads();
    if (threadIdx.x < 256) {
      int above = 0;
      for (int i = 255; i > static_cast<int>(threadIdx.x); --i) above += hist[i];
      if (above < need && above + hist[threadIdx.x] >= need) {     // exactly one bin
        pick_out[0] = prefix | (static_cast<unsigned long long>(threadIdx.x) << shift);
        pick_out[1] = static_cast<unsigned long long>(need - above);
      }
    }
    __syncthreads();
    prefix = pick_out[0];
    need = static_cast<int>(pick_out[1]);
    __syncthreads();
  }
  return prefix;
}

__global__ void __launch_bounds__(TRI_THREADS) k_tri_stats(const double* __restrict__ rec, double* __restrict__ stats, int B, int num) {
  extern __shared__ unsigned long long tri_keys[];     // num keys
  __shared__ int hist[256];
  __shared__ unsigned long long picked[2];
  __shared__ double red[TRI_THREADS];
  const int view = blockIdx.x & 1, d = (blockIdx.x >> 1) & 1, b = blockIdx.x >> 2;
  const double* r = rec + static_cast<long>(d * B + b) * num * 4 + view * 2;    // (inter, z) of this view at stride 4
  const int rank = (num - 1) / 2;
  double med[2];
  for (int which = 0; which < 2; ++which) {
    for (int i = threadIdx.x; i < num; i += TRI_THREADS) tri_keys[i] = order_key(r[static_cast<long>(i) * 4 + which]);
    __syncthreads();
    med[which] = key_value(select_rank(tri_keys, num, rank, hist, picked));
    __syncthreads();
  }
  const double scale = med[0] / (med[1] + tri::EPS);
  double A = 0.0, C = 0.0;
  for (int i = threadIdx.x; i < num; i += TRI_THREADS) {
    const double is = r[static_cast<long>(i) * 4] / (scale + tri::EPS), z = r[static_cast<long>(i) * 4 + 1];
    A += (is * is) / (z * z + tri::EPS);
    C += is / (z + tri::EPS);
  }
  ransac::block_sum<1>(&A, red);     // a fixed order: every thread's strided partial, then a tree over the threads
  ransac::block_sum<1>(&C, red);
  const double aa = C / (A + tri::EPS);
  double L = 0.0;
  for (int i = threadIdx.x; i < num; i += TRI_THREADS) {
    const double is = r[static_cast<long>(i) * 4] / (scale + tri::EPS), z = r[static_cast<long>(i) * 4 + 1];
    const double e = 1.0 - aa * is / (z + tri::EPS);
    L += e * e;
  }
  ransac::block_sum<1>(&L, red);
  L = L / num;
  if (threadIdx.x == 0) {
    double* s = stats + static_cast<long>(blockIdx.x) * STATS_DOUBLES;
    s[0] = scale; s[1] = aa; s[2] = aa / (scale + tri::EPS); s[3] = L;
  }
}

__global__ void k_tri_loss(const double* __restrict__ stats, float* __restrict__ loss, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* s = stats + static_cast<long>(b) * 4 * STATS_DOUBLES;
  loss[b] = static_cast<float>((s[3] + s[STATS_DOUBLES + 3]) + (s[2 * STATS_DOUBLES + 3] + s[3 * STATS_DOUBLES + 3]));
}

// ---------------------------------------------------------------------------------------------- backward
// workspace: [64-byte header: word 0 = bound of the flow contributions, word 1 = bound of the disparity contributions]
//            [int64 accumulators: flow of direction 0, of direction 1 (B*2*HW each), disp_t, disp_l, disp_r (B*HW each)]
//            [per point: float gu, gv, gI1, gI2] [per (plane, block): 12 doubles of T34 partial sums]
struct TriWs {
  unsigned* header;
  long long* acc;
  float* pg;
  double* part;
};
__host__ __device__ inline long tri_blocks(int num) { return (num + TRI_THREADS - 1) / TRI_THREADS; }
__host__ __device__ inline long tri_acc_count(int B, int H, int W) { return 7L * B * H * W; }
inline long tri_ws_bytes(int B, int H, int W, int num) {
  return SCATTER_HEADER_BYTES + 8 * tri_acc_count(B, H, W) + 16L * 2 * B * num + 96L * 2 * B * tri_blocks(num);
}
inline TriWs tri_ws(void* ws, int B, int H, int W, int num) {
  TriWs w;
  char* p = static_cast<char*>(ws);
  w.header = reinterpret_cast<unsigned*>(p);
  w.acc = reinterpret_cast<long long*>(p + SCATTER_HEADER_BYTES);
  w.pg = reinterpret_cast<float*>(p + SCATTER_HEADER_BYTES + 8 * tri_acc_count(B, H, W));
  w.part = reinterpret_cast<double*>(p + SCATTER_HEADER_BYTES + 8 * tri_acc_count(B, H, W) + 16L * 2 * B * num);
  return w;
}

__device__ __forceinline__ unsigned abs_bits(float v) { return static_cast<unsigned>(__float_as_int(v)) & 0x7fffffffu; }

__global__ void __launch_bounds__(TRI_THREADS) k_tri_bwd_points(TriIn a, const double* __restrict__ stats,
                                                                 const float* __restrict__ gloss, TriWs w) {
  __shared__ double red[TRI_THREADS];
  __shared__ unsigned bmax[2];
  const int j = blockIdx.x * TRI_THREADS + threadIdx.x;
  const int plane = blockIdx.y, d = plane / a.B, b = plane - d * a.B;
  if (threadIdx.x < 2) bmax[threadIdx.x] = 0u;
  __syncthreads();
  double gT[12];
  for (int i = 0; i < 12; ++i) gT[i] = 0.0;
  if (j < a.num) {
    const PointCtx c = load_point(a, d, b, j);
    double o[6];
    tri::tri_point<double>(c.K, c.Kinv, c.T, c.x, c.y, c.u, c.v, o);
    const long HW = static_cast<long>(a.H) * a.W;
    const tri::Sample s1 = tri::sample_reflect(a.disp_t + b * HW, o[0], o[1], a.H, a.W, a.ac);
    const tri::Sample s2 = tri::sample_reflect(a.disp_s[d] + b * HW, o[3], o[4], a.H, a.W, a.ac);
    const double g = static_cast<double>(gloss[b]) * 2.0 / a.num;
    const double* st = stats + static_cast<long>((b * 2 + d) * 2) * STATS_DOUBLES;
    // L = mean((1 - c I / (z + eps))^2), c = a / (scale + eps) a constant: dL/dI and dL/dz of both views
    const double c1 = st[2], c2 = st[STATS_DOUBLES + 2];
    const double z1 = o[2] + tri::EPS, z2 = o[5] + tri::EPS;
    const double e1 = 1.0 - c1 * s1.val / z1, e2 = 1.0 - c2 * s2.val / z2;
    const double gI1 = g * e1 * (-c1 / z1), gI2 = g * e2 * (-c2 / z2);
    const double gZ1 = g * e1 * (c1 * s1.val / (z1 * z1)), gZ2 = g * e2 * (c2 * s2.val / (z2 * z2));
    // weights of the six outputs of tri_point in the loss
    const double wo[6] = {gI1 * s1.dcx, gI1 * s1.dcy, gZ1, gI2 * s2.dcx, gI2 * s2.dcy, gZ2};
    double guv[2];
    for (int t = 0; t < 14; ++t) {       // one forward-mode pass per tangent direction: u, v, T34[0 .. 12)
      tri::Dual T[12], od[6];
      for (int i = 0; i < 12; ++i) T[i] = tri::Dual{c.T[i], (t - 2 == i) ? 1.0 : 0.0};
      tri::tri_point<tri::Dual>(c.K, c.Kinv, T, c.x, c.y, tri::Dual{c.u, t == 0 ? 1.0 : 0.0}, tri::Dual{c.v, t == 1 ? 1.0 : 0.0}, od);
      double s = 0.0;
      for (int i = 0; i < 6; ++i) s += wo[i] * od[i].d;
      if (t < 2) guv[t] = s; else gT[t - 2] = s;
    }
    float* pg = w.pg + (static_cast<long>(plane) * a.num + j) * 4;
    pg[0] = static_cast<float>(guv[0]); pg[1] = static_cast<float>(guv[1]);
    pg[2] = static_cast<float>(gI1); pg[3] = static_cast<float>(gI2);
    // bounds of the fixed-point scatter: max is order-independent (NaN / inf bit patterns win and poison the result)
    atomicMax(&bmax[0], max(abs_bits(pg[0]), abs_bits(pg[1])));
    atomicMax(&bmax[1], max(abs_bits(pg[2]), abs_bits(pg[3])));
  }
  __syncthreads();
  if (threadIdx.x < 2 && bmax[threadIdx.x] != 0u) atomicMax(w.header + threadIdx.x, bmax[threadIdx.x]);
  double* part = w.part + (static_cast<long>(plane) * gridDim.x + blockIdx.x) * 12;
  for (int i = 0; i < 12; ++i) {
    double s = gT[i];
    ransac::block_sum<1>(&s, red);
    if (threadIdx.x == 0) part[i] = s;
  }
}

__global__ void __launch_bounds__(TRI_THREADS) k_tri_bwd_scatter(TriIn a, TriWs w) {
  const int j = blockIdx.x * TRI_THREADS + threadIdx.x;
  const int plane = blockIdx.y, d = plane / a.B, b = plane - d * a.B;
  if (j >= a.num) return;
  const ScatterScale sf = scatter_scale(w.header[0]), sd = scatter_scale(w.header[1]);
  const PointCtx c = load_point(a, d, b, j);
  double o[6];
  tri::tri_point<double>(c.K, c.Kinv, c.T, c.x, c.y, c.u, c.v, o);
  const long HW = static_cast<long>(a.H) * a.W;
  const tri::Sample s1 = tri::sample_reflect(a.disp_t + b * HW, o[0], o[1], a.H, a.W, a.ac);
  const tri::Sample s2 = tri::sample_reflect(a.disp_s[d] + b * HW, o[3], o[4], a.H, a.W, a.ac);
  const float* pg = w.pg + (static_cast<long>(plane) * a.num + j) * 4;
  long long* aflow = w.acc + (static_cast<long>(d) * a.B + b) * 2 * HW;
  fixed_add(aflow + c.pix, to_fixed(pg[0], sf.to_fixed));
  fixed_add(aflow + HW + c.pix, to_fixed(pg[1], sf.to_fixed));
  long long* at = w.acc + 4L * a.B * HW + b * HW;
  long long* as = w.acc + (5L + d) * a.B * HW + b * HW;
  for (int t = 0; t < 4; ++t) {
    fixed_add(at + s1.off[t], to_fixed(static_cast<float>(pg[2] * s1.w[t]), sd.to_fixed));
    fixed_add(as + s2.off[t], to_fixed(static_cast<float>(pg[3] * s2.w[t]), sd.to_fixed));
  }
}

// grads[i] = float(acc[i]) for the 7*B*HW accumulators (the first 4*B*HW are the flows'); block 0 also adds T34's partials
__global__ void __launch_bounds__(TRI_THREADS) k_tri_bwd_finish(TriWs w, float* __restrict__ grads, float* __restrict__ gT34, int B, long HW,
                                                                 int nblk) {
  const ScatterScale sf = scatter_scale(w.header[0]), sd = scatter_scale(w.header[1]);
  const long n = 7L * B * HW, nflow = 4L * B * HW;
  for (long i = static_cast<long>(blockIdx.x) * TRI_THREADS + threadIdx.x; i < n; i += static_cast<long>(gridDim.x) * TRI_THREADS)
    grads[i] = from_fixed(w.acc[i], i < nflow ? sf : sd);
  if (blockIdx.x == 0) {
    for (int e = threadIdx.x; e < 2 * B * 12; e += TRI_THREADS) {
      const int plane = e / 12, i = e - plane * 12, d = plane / B, b = plane - d * B;
      double s = 0.0;
      for (int k = 0; k < nblk; ++k) s += w.part[(static_cast<long>(plane) * nblk + k) * 12 + i];
      gT34[(b * 2 + d) * 12 + i] = static_cast<float>(s);
    }
  }
}

int check_in(const TriIn& a) {
  if (!a.flow[0] || !a.flow[1] || !a.disp_t || !a.disp_s[0] || !a.disp_s[1] || !a.T34 || !a.K || !a.Kinv || !a.idx || !a.pick)
    return DFE_ERR_NULL;
  if (a.B <= 0 || a.B > 16384 || a.H < 2 || a.W < 2 || a.k <= 0 || a.num <= 0) return DFE_ERR_DIMS;
  if (static_cast<long>(a.H) * a.W >= (1L << 28) || a.k > a.H * a.W) return DFE_ERR_DIMS;
  return DFE_OK;
}

constexpr int TRI_MAX_NUM = 16384;     // the medians stage num 8-byte keys in LDS (128 KB of the CU's 160 KB)

}  // namespace
}  // namespace dfe

using namespace dfe;

extern "C" long dfe_triangulate_ws_bytes(int B, int H, int W, int num) {
  if (B <= 0 || H <= 0 || W <= 0 || num <= 0) return 0;
  return tri_ws_bytes(B, H, W, num);
}

extern "C" int dfe_triangulate_fwd(const float* flow_bwd, const float* flow_fwd, const float* disp_t, const float* disp_l,
                                   const float* disp_r, const float* T34, const float* K, const float* K_inv, const int* idx,
                                   const long long* pick, double* rec, int B, int H, int W, int k, int num, int align_corners,
                                   void* stream) {
  const TriIn a{{flow_bwd, flow_fwd}, disp_t, {disp_l, disp_r}, T34, K, K_inv, idx, pick, B, H, W, k, num, align_corners ? 1 : 0};
  const int rc = check_in(a);
  if (rc != DFE_OK) return rc;
  if (!rec) return DFE_ERR_NULL;
  if (!aligned8(rec)) return DFE_ERR_DIMS;
  k_tri_fwd<<<dim3(static_cast<unsigned>(tri_blocks(num)), 2 * B), TRI_THREADS, 0, static_cast<hipStream_t>(stream)>>>(a, rec);
  return launch_status();
}

extern "C" int dfe_triangulate_stats(const double* rec, double* stats, float* loss, int B, int num, void* stream) {
  if (!rec || !stats || !loss) return DFE_ERR_NULL;
  if (B <= 0 || B > 16384 || num <= 0) return DFE_ERR_DIMS;
  if (num > TRI_MAX_NUM) return DFE_ERR_UNSUPPORTED;
  if (!aligned8(rec) || !aligned8(stats)) return DFE_ERR_DIMS;
  hipStream_t st = static_cast<hipStream_t>(stream);
  launch_dyn_lds<k_tri_stats>(4u * B, static_cast<size_t>(num) * 8, TRI_MAX_NUM * 8, st, rec, stats, B, num);
  DFE_LAUNCH_CHECK();
  k_tri_loss<<<(B + 63) / 64, 64, 0, st>>>(stats, loss, B);
  return launch_status();
}

extern "C" int dfe_triangulate_bwd(const float* flow_bwd, const float* flow_fwd, const float* disp_t, const float* disp_l,
                                   const float* disp_r, const float* T34, const float* K, const float* K_inv, const int* idx,
                                   const long long* pick, const double* stats, const float* gloss, float* grads,
                                   float* gT34, void* ws, int B, int H, int W, int k, int num, int align_corners, void* stream) {
  const TriIn a{{flow_bwd, flow_fwd}, disp_t, {disp_l, disp_r}, T34, K, K_inv, idx, pick, B, H, W, k, num, align_corners ? 1 : 0};
  const int rc = check_in(a);
  if (rc != DFE_OK) return rc;
  if (!stats || !gloss || !grads || !gT34 || !ws) return DFE_ERR_NULL;
  if (!aligned16(ws) || !aligned8(stats)) return DFE_ERR_DIMS;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const TriWs w = tri_ws(ws, B, H, W, num);
  const long HW = static_cast<long>(H) * W;
  // header and accumulators start at zero; the per-point records and the partial sums are written before they are read
  if (hipMemsetAsync(ws, 0, static_cast<size_t>(SCATTER_HEADER_BYTES + 8 * tri_acc_count(B, H, W)), st) != hipSuccess) return DFE_ERR_LAUNCH;
  const dim3 grid(static_cast<unsigned>(tri_blocks(num)), 2 * B);
  k_tri_bwd_points<<<grid, TRI_THREADS, 0, st>>>(a, stats, gloss, w);
  DFE_LAUNCH_CHECK();
  k_tri_bwd_scatter<<<grid, TRI_THREADS, 0, st>>>(a, w);
  DFE_LAUNCH_CHECK();
  const long n = 7L * B * HW;
  const long blocks = (n + TRI_THREADS * 4 - 1) / (TRI_THREADS * 4);
  k_tri_bwd_finish<<<static_cast<unsigned>(blocks > 4096 ? 4096 : blocks), TRI_THREADS, 0, st>>>(w, grads, gT34, B, HW,
                                                                                                static_cast<int>(tri_blocks(num)));
  return launch_status();
}
