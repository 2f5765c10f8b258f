// KITTI evaluation metrics on a device-resident set (include/dfe_hip.h "evaluation metrics"): a batch of predictions at the
// training size -> the reference's per-sample numbers (core/evaluation/evaluate_flow.py:85-174, evaluate_depth.py:13-52,
// evaluation_utils.py:11-32) with no host read.
//
// Order of every sum: a thread adds its pixels in increasing index, a block its threads with the DPP butterfly and the row sums
// in index order, a fold launch the blocks of a sample in index order -- all in double, so a record depends on its sample alone
// (not on the batch it ran in).  Where one block's result feeds another the kernel boundary is the hand-off (as dfe_grad_guard
// and the split sums do); the only atomics are integer adds on histogram bins, which do not depend on order.
#include "dfe_device.h"
#include "dfe_internal.h"

namespace dfe {
namespace {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_ROWS = EVAL_THREADS / 16;   // DPP rows of 16 lanes per block
constexpr int FLOW_BPS = 64;                   // blocks per sample: fixed, so that a record does not depend on the batch
constexpr int FLOW_SUMS = 13;
constexpr int FLOW_REC = 16;
constexpr int DEPTH_BPS = 32;
constexpr int DEPTH_SUMS = 7;
constexpr int DEPTH_PART = 8;
constexpr int DEPTH_REC = 10;
constexpr int SEL = 4;                         // selections carried through the radix passes: gt lower / upper middle, pred lower / upper
constexpr int BINS = 256;
constexpr int STATE_WORDS = 16;                // per sample: prefix[4], rank[4], count, padding

// ---------------------------------------------------------------- the resize of kitti_io.resize_bilinear_u8 / eval_oracle.resize_linear
// half-pixel centres, edge replication; the source coordinate in double as numpy evaluates it, the weight rounded to fp32
struct Axis { int i0, i1; float w1; };
__device__ __forceinline__ Axis resize_axis(int dst, int in_size, int out_size) {
  double s = (static_cast<double>(dst) + 0.5) * (static_cast<double>(in_size) / static_cast<double>(out_size)) - 0.5;
  s = fmin(fmax(s, 0.0), static_cast<double>(in_size - 1));
  Axis a;
  a.i0 = static_cast<int>(s);
  a.i1 = min(a.i0 + 1, in_size - 1);
  a.w1 = static_cast<float>(s - static_cast<double>(a.i0));
  return a;
}
// top = a (1 - wx) + b wx, bot likewise, top (1 - wy) + bot wy; every tap times `scale` first
__device__ __forceinline__ float resize_at(const float* __restrict__ plane, int w, const Axis ay, const Axis ax, float scale) {
  const float* r0 = plane + static_cast<long>(ay.i0) * w;
  const float* r1 = plane + static_cast<long>(ay.i1) * w;
  const float a = r0[ax.i0] * scale, b = r0[ax.i1] * scale, c = r1[ax.i0] * scale, d = r1[ax.i1] * scale;
  const float top = a * (1.0f - ax.w1) + b * ax.w1;
  const float bot = c * (1.0f - ax.w1) + d * ax.w1;
  return top * (1.0f - ay.w1) + bot * ay.w1;
}

// ---------------------------------------------------------------- block sums in double (dfe_device.h's block_sum on 64-bit values)
template <int CTRL>
__device__ __forceinline__ double dpp_add_f64(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, static_cast<int>(b & 0xffffffffLL), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, static_cast<int>(b >> 32), CTRL, 0xF, 0xF, false);
  return v + __longlong_as_double((static_cast<long long>(hi) << 32) | static_cast<long long>(static_cast<unsigned>(lo)));
}
// out[0..N) written by threads 0..N-1; every thread of the 256 calls it; smem: N * EVAL_ROWS doubles
template <int N>
__device__ __forceinline__ void block_sum_f64(double (&vals)[N], double* smem, double* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) vals[i] = dpp_add_f64<0xB1>(vals[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) vals[i] = dpp_add_f64<0x4E>(vals[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) vals[i] = dpp_add_f64<0x141>(vals[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) vals[i] = dpp_add_f64<0x140>(vals[i]);
  if ((lane & 15) == 0) {
    const int slot = wave * 4 + (lane >> 4);
#pragma unroll
    for (int i = 0; i < N; ++i) smem[slot * N + i] = vals[i];
  }
  __syncthreads();
  if (threadIdx.x < N) {
    double s = 0.0;
    for (int r = 0; r < EVAL_ROWS; ++r) s += smem[r * N + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// the size table's entries, clamped so that no index derived from them leaves the padded planes
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---------------------------------------------------------------- flow
// grid (FLOW_BPS, n).  Quads of four ground-truth pixels of one row: 16-byte loads of u and v, one dword of flags.
// part: [n][FLOW_BPS][FLOW_REC] doubles, the first FLOW_SUMS of every entry written by every block.
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_flow(const float* __restrict__ pred, int h, int w, const float* __restrict__ gu,
                                                           const float* __restrict__ gv, const unsigned char* __restrict__ flags,
                                                           const int* __restrict__ dims, int Hmax, int Wmax, int first,
                                                           double* __restrict__ part) {
  __shared__ double smem[FLOW_SUMS * EVAL_ROWS];
  const int i = blockIdx.y;
  const long row = static_cast<long>(first) + i;
  const int H = clampi(dims[row * 2], 0, Hmax), W = clampi(dims[row * 2 + 1], 0, Wmax);
  const long plane = row * Hmax * Wmax;
  const float* pu = pred + static_cast<long>(i) * 2 * h * w;
  const float* pv = pu + static_cast<long>(h) * w;
  const float sx = static_cast<float>(W) / static_cast<float>(w), sy = static_cast<float>(H) / static_cast<float>(h);
  const int Wq = (W + 3) >> 2, Q = H * Wq;
  const int per = (Q + FLOW_BPS - 1) / FLOW_BPS;
  const int q0 = min(static_cast<int>(blockIdx.x) * per, Q), q1 = min(q0 + per, Q);
  double s_val = 0.0, s_noc = 0.0, s_occ = 0.0, s_mv = 0.0, s_st = 0.0;
  int c_val = 0, c_noc = 0, c_occ = 0, b_val = 0, b_mv = 0, b_st = 0, c_mv = 0, c_st = 0;
  for (int q = q0 + threadIdx.x; q < q1; q += EVAL_THREADS) {
    const int y = q / Wq, x4 = (q - y * Wq) * 4;
    const long o = plane + static_cast<long>(y) * Wmax + x4;     // Wmax % 4 == 0: the quad lies inside the padded row
    const float4 u4 = *reinterpret_cast<const float4*>(gu + o);
    const float4 v4 = *reinterpret_cast<const float4*>(gv + o);
    const uchar4 f4 = *reinterpret_cast<const uchar4*>(flags + o);
    const float us[4] = {u4.x, u4.y, u4.z, u4.w}, vs[4] = {v4.x, v4.y, v4.z, v4.w};
    const unsigned fs[4] = {f4.x, f4.y, f4.z, f4.w};
    const Axis ay = resize_axis(y, h, H);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (x4 + k < W) {                                          // the padding of the row is loaded and never used
        const Axis ax = resize_axis(x4 + k, w, W);
        const float du = resize_at(pu, w, ay, ax, sx) - us[k], dv = resize_at(pv, w, ay, ax, sy) - vs[k];
        const float epe = sqrtf(du * du + dv * dv);
        const float mag = fmaxf(sqrtf(us[k] * us[k] + vs[k] * vs[k]), 1e-10f);
        const int valid = fs[k] & 1, noc = (fs[k] >> 1) & 1, mv = (fs[k] >> 2) & 1;
        const int bad = (epe > 3.0f) && (epe / mag > 0.05f);
        const double e = static_cast<double>(epe);
        const int occ = valid - noc;                             // the arithmetic form: noc = 1, valid = 0 counts -1
        if (valid) s_val += e;
        if (noc) s_noc += e;
        if (occ != 0) s_occ += e * static_cast<double>(occ);
        if (valid & mv) s_mv += e;
        if (valid & (mv ^ 1)) s_st += e;
        c_val += valid; c_noc += noc; c_occ += occ;
        c_mv += valid & mv; c_st += valid & (mv ^ 1);
        b_val += valid & bad; b_mv += valid & mv & bad; b_st += valid & (mv ^ 1) & bad;
      }
    }
  }
  double vals[FLOW_SUMS] = {s_val, s_noc, s_occ, s_mv, s_st, static_cast<double>(c_val), static_cast<double>(c_noc),
                            static_cast<double>(c_occ), static_cast<double>(b_val), static_cast<double>(b_mv),
                            static_cast<double>(b_st), static_cast<double>(c_mv), static_cast<double>(c_st)};
  block_sum_f64<FLOW_SUMS>(vals, smem, part + (static_cast<long>(i) * FLOW_BPS + blockIdx.x) * FLOW_REC);
}

// grid n, 64 threads: the blocks of a sample in index order -> its record
__global__ void k_eval_flow_fold(const double* __restrict__ part, double* __restrict__ records) {
  const int i = blockIdx.x, t = threadIdx.x;
  if (t >= FLOW_REC) return;
  double s = 0.0;
  if (t < FLOW_SUMS)
    for (int b = 0; b < FLOW_BPS; ++b) s += part[(static_cast<long>(i) * FLOW_BPS + b) * FLOW_REC + t];
  records[static_cast<long>(i) * FLOW_REC + t] = s;
}

// one block, 8 threads: table value t = the mean over the samples, in index order, of the sample's ratio
__global__ void k_eval_flow_finish(const double* __restrict__ records, int N, int has_moving, double* __restrict__ table) {
  const int t = threadIdx.x;
  if (t >= 8) return;
  // numerator and denominator of the eight values: epe, epe_noc, epe_occ, err_rate, epe_move, epe_static, move_rate, static_rate
  const int num[8] = {0, 1, 2, 8, 3, 4, 9, 10}, den[8] = {5, 6, 7, 5, 11, 12, 11, 12};
  double acc = 0.0;
  if (t < 4 || has_moving) {
    for (int i = 0; i < N; ++i) {
      const double* r = records + static_cast<long>(i) * FLOW_REC;
      double d = r[den[t]];
      if (t == 2) d = fmax(d, 1.0);
      acc += r[num[t]] / d;
    }
    acc = acc / static_cast<double>(N);
  }
  table[t] = acc;
}

// ---------------------------------------------------------------- depth
struct DepthBox { int H, W, y0, y1, xq0, cq, x0, x1; };
__device__ __forceinline__ DepthBox depth_box(const int* __restrict__ dims, long row, int Hmax, int Wmax) {
  DepthBox b;
  b.H = clampi(dims[row * 6], 0, Hmax); b.W = clampi(dims[row * 6 + 1], 0, Wmax);
  b.y0 = clampi(dims[row * 6 + 2], 0, b.H); b.y1 = clampi(dims[row * 6 + 3], b.y0, b.H);
  b.x0 = clampi(dims[row * 6 + 4], 0, b.W); b.x1 = clampi(dims[row * 6 + 5], b.x0, b.W);
  b.xq0 = b.x0 >> 2;
  b.cq = ((b.x1 + 3) >> 2) - b.xq0;                 // quads that cover the crop's columns (>= 0)
  return b;
}

// One radix digit.  grid (DEPTH_BPS, n).  FIRST: the resize, pred = 1 / (disp + 1e-4) into the workspace for the masked pixels
// (and only those), and the histogram of the top digit; later passes histogram digit `d` of the keys that match the prefix of
// their selection.  Unmasked and padded pixels reach neither a histogram nor the workspace.
template <bool FIRST>
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_depth_hist(const float* __restrict__ disp, int h, int w, const float* __restrict__ gt,
                                                                 const int* __restrict__ dims, int Hmax, int Wmax, int first,
                                                                 float min_depth, float max_depth, float* __restrict__ pred,
                                                                 int* __restrict__ ghist, const unsigned* __restrict__ state, int d) {
  __shared__ int hist[SEL * BINS];
  const int i = blockIdx.y;
  const long row = static_cast<long>(first) + i;
  const DepthBox bx = depth_box(dims, row, Hmax, Wmax);
  const long plane = row * Hmax * Wmax, wplane = static_cast<long>(i) * Hmax * Wmax;
  const float* dp = disp + static_cast<long>(i) * h * w;
  for (int t = threadIdx.x; t < SEL * BINS; t += EVAL_THREADS) hist[t] = 0;
  unsigned prefix[SEL] = {0u, 0u, 0u, 0u};
  if (!FIRST) {
#pragma unroll
    for (int s = 0; s < SEL; ++s) prefix[s] = state[i * STATE_WORDS + s];
  }
  __syncthreads();
  const int shift = 24 - 8 * d;                      // the digit's position; the prefix is everything above it
  const int Q = (bx.y1 - bx.y0) * bx.cq;
  const int per = (Q + DEPTH_BPS - 1) / DEPTH_BPS;
  const int q0 = min(static_cast<int>(blockIdx.x) * per, Q), q1 = min(q0 + per, Q);
  for (int q = q0 + threadIdx.x; q < q1; q += EVAL_THREADS) {
    const int yr = q / bx.cq, y = bx.y0 + yr, x4 = (bx.xq0 + (q - yr * bx.cq)) * 4;
    const long o = static_cast<long>(y) * Wmax + x4;
    const float4 g4 = *reinterpret_cast<const float4*>(gt + plane + o);
    const float gs[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = x4 + k;
      if (x >= bx.x0 && x < bx.x1 && gs[k] > min_depth && gs[k] < max_depth) {
        float p;
        if (FIRST) {
          const float r = resize_at(dp, w, resize_axis(y, h, bx.H), resize_axis(x, w, bx.W), 1.0f);
          p = 1.0f / (r + 1e-4f);
          pred[wplane + o + k] = p;
        } else {
          p = pred[wplane + o + k];
        }
        const unsigned kg = __float_as_uint(gs[k]), kp = __float_as_uint(p);
#pragma unroll
        for (int s = 0; s < SEL; ++s) {
          const unsigned key = s < 2 ? kg : kp;
          if (FIRST || ((key >> (shift + 8)) == prefix[s])) atomicAdd(&hist[s * BINS + ((key >> shift) & 255u)], 1);
        }
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < SEL * BINS; t += EVAL_THREADS)
    if (hist[t] != 0) atomicAdd(&ghist[static_cast<long>(i) * SEL * BINS + t], hist[t]);
}

// grid n, 256 threads: the bin that holds each selection's rank -> prefix and rank inside the bin; the histogram is left zeroed
// for the next digit.  d == 0 also derives the count and the two middle ranks from it.
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_depth_pick(int* __restrict__ ghist, unsigned* __restrict__ state, int d) {
  __shared__ int hist[SEL * BINS];
  const int i = blockIdx.x;
  int* g = ghist + static_cast<long>(i) * SEL * BINS;
  for (int t = threadIdx.x; t < SEL * BINS; t += EVAL_THREADS) { hist[t] = g[t]; g[t] = 0; }
  __syncthreads();
  const int s = threadIdx.x;
  if (s >= SEL) return;
  unsigned* st = state + i * STATE_WORDS;
  const int* hs = hist + s * BINS;
  unsigned prefix = 0u, rank = 0u;
  if (d == 0) {
    unsigned count = 0u;
    for (int b = 0; b < BINS; ++b) count += static_cast<unsigned>(hs[b]);
    rank = count == 0u ? 0u : ((s & 1) ? count / 2u : (count - 1u) / 2u);
    if (s == 0) st[2 * SEL] = count;
  } else {
    prefix = st[s]; rank = st[SEL + s];
  }
  unsigned cum = 0u;
  int bin = 0;
  for (int b = 0; b < BINS; ++b) {
    const unsigned n = static_cast<unsigned>(hs[b]);
    if (rank < cum + n) { bin = b; break; }
    cum += n;
    if (b == BINS - 1) { bin = 0; cum = rank; }     // an empty mask: nothing to select (the medians are then meaningless)
  }
  st[s] = (prefix << 8) | static_cast<unsigned>(bin);
  st[SEL + s] = rank - cum;
}

__device__ __forceinline__ void depth_medians(const unsigned* __restrict__ st, float& med_gt, float& med_pred) {
  // numpy.median: the mean of the two middle values (the value itself when they are the same element)
  med_gt = 0.5f * (__uint_as_float(st[0]) + __uint_as_float(st[1]));
  med_pred = 0.5f * (__uint_as_float(st[2]) + __uint_as_float(st[3]));
}

// grid (DEPTH_BPS, n): the seven sums of compute_errors over the masked pixels; part [n][DEPTH_BPS][DEPTH_PART] doubles
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_depth_sums(const float* __restrict__ gt, const int* __restrict__ dims, int Hmax, int Wmax,
                                                                 int first, float min_depth, float max_depth, const float* __restrict__ pred,
                                                                 const unsigned* __restrict__ state, double* __restrict__ part) {
  __shared__ double smem[DEPTH_SUMS * EVAL_ROWS];
  const int i = blockIdx.y;
  const long row = static_cast<long>(first) + i;
  const DepthBox bx = depth_box(dims, row, Hmax, Wmax);
  const long plane = row * Hmax * Wmax, wplane = static_cast<long>(i) * Hmax * Wmax;
  float med_gt, med_pred;
  depth_medians(state + i * STATE_WORDS, med_gt, med_pred);
  const float ratio = med_gt / med_pred;
  double s_abs = 0.0, s_sq = 0.0, s_mse = 0.0, s_log = 0.0;
  int a1 = 0, a2 = 0, a3 = 0;
  const int Q = (bx.y1 - bx.y0) * bx.cq;
  const int per = (Q + DEPTH_BPS - 1) / DEPTH_BPS;
  const int q0 = min(static_cast<int>(blockIdx.x) * per, Q), q1 = min(q0 + per, Q);
  for (int q = q0 + threadIdx.x; q < q1; q += EVAL_THREADS) {
    const int yr = q / bx.cq, y = bx.y0 + yr, x4 = (bx.xq0 + (q - yr * bx.cq)) * 4;
    const long o = static_cast<long>(y) * Wmax + x4;
    const float4 g4 = *reinterpret_cast<const float4*>(gt + plane + o);
    const float gs[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = x4 + k;
      if (x >= bx.x0 && x < bx.x1 && gs[k] > min_depth && gs[k] < max_depth) {
        const float p = fminf(fmaxf(pred[wplane + o + k] * ratio, min_depth), max_depth);
        const float g = fminf(fmaxf(gs[k], min_depth), max_depth);
        const float th = fmaxf(g / p, p / g);
        a1 += th < 1.25f; a2 += th < 1.5625f; a3 += th < 1.953125f;
        const float df = g - p, sq = df * df, lg = logf(g) - logf(p);
        s_abs += static_cast<double>(fabsf(df) / g);
        s_sq += static_cast<double>(sq / g);
        s_mse += static_cast<double>(sq);
        s_log += static_cast<double>(lg * lg);
      }
    }
  }
  double vals[DEPTH_SUMS] = {s_abs, s_sq, s_mse, s_log, static_cast<double>(a1), static_cast<double>(a2), static_cast<double>(a3)};
  block_sum_f64<DEPTH_SUMS>(vals, smem, part + (static_cast<long>(i) * DEPTH_BPS + blockIdx.x) * DEPTH_PART);
}

// grid n, 64 threads: record = abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, median(gt), median(pred), count
__global__ void k_eval_depth_fold(const double* __restrict__ part, const unsigned* __restrict__ state, double* __restrict__ records) {
  const int i = blockIdx.x, t = threadIdx.x;
  if (t >= DEPTH_REC) return;
  const unsigned* st = state + i * STATE_WORDS;
  const double count = static_cast<double>(st[2 * SEL]);
  double v;
  if (t < DEPTH_SUMS) {
    double s = 0.0;
    for (int b = 0; b < DEPTH_BPS; ++b) s += part[(static_cast<long>(i) * DEPTH_BPS + b) * DEPTH_PART + t];
    v = s / count;
    if (t == 2 || t == 3) v = sqrt(v);
  } else if (t == DEPTH_REC - 1) {
    v = count;
  } else {
    float med_gt, med_pred;
    depth_medians(st, med_gt, med_pred);
    v = static_cast<double>(t == DEPTH_SUMS ? med_gt : med_pred);
  }
  records[static_cast<long>(i) * DEPTH_REC + t] = v;
}

inline long align16(long v) { return (v + 15) / 16 * 16; }
inline bool batch_ok(int n, int h, int w, int N, int Hmax, int Wmax, int first) {
  return n >= 1 && n <= 1024 && h >= 1 && w >= 1 && static_cast<long>(n) * 2 * h * w < (1L << 31) && N >= 1 && Hmax >= 1 && Wmax >= 4 &&
         Wmax % 4 == 0 && static_cast<long>(Hmax) * Wmax < (1L << 28) && first >= 0 && static_cast<long>(first) + n <= N;
}
struct DepthWs { long pred, part, hist, state, total; };
inline DepthWs depth_ws(int n, int Hmax, int Wmax) {
  DepthWs l;
  l.pred = 0;
  l.part = align16(static_cast<long>(n) * Hmax * Wmax * 4);
  l.hist = l.part + align16(static_cast<long>(n) * DEPTH_BPS * DEPTH_PART * 8);
  l.state = l.hist + align16(static_cast<long>(n) * SEL * BINS * 4);
  l.total = l.state + align16(static_cast<long>(n) * STATE_WORDS * 4);
  return l;
}

}  // namespace
}  // namespace dfe

using namespace dfe;

extern "C" {

int dfe_eval_flow_record_doubles(void) { return FLOW_REC; }
int dfe_eval_depth_record_doubles(void) { return DEPTH_REC; }

long dfe_eval_flow_ws_bytes(int n) { return n >= 1 && n <= 1024 ? static_cast<long>(n) * FLOW_BPS * FLOW_REC * 8 : 0; }

long dfe_eval_depth_ws_bytes(int n, int Hmax, int Wmax) {
  if (n < 1 || n > 1024 || Hmax < 1 || Wmax < 4 || Wmax % 4 != 0 || static_cast<long>(Hmax) * Wmax >= (1L << 28)) return 0;
  return depth_ws(n, Hmax, Wmax).total;
}

int dfe_eval_flow(const float* pred, int n, int h, int w, const float* gt_u, const float* gt_v, const unsigned char* flags,
                  const int* dims, int N, int Hmax, int Wmax, int first, void* ws, long ws_bytes, double* records, void* stream) {
  if (!pred || !gt_u || !gt_v || !flags || !dims || !ws || !records) return DFE_ERR_NULL;
  if (!batch_ok(n, h, w, N, Hmax, Wmax, first)) return DFE_ERR_DIMS;
  if (!aligned16(gt_u) || !aligned16(gt_v) || (reinterpret_cast<uintptr_t>(flags) & 3) != 0 || !aligned8(ws) || !aligned8(records))
    return DFE_ERR_DIMS;
  if (ws_bytes < dfe_eval_flow_ws_bytes(n)) return DFE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(ws);
  k_eval_flow<<<dim3(FLOW_BPS, n), EVAL_THREADS, 0, st>>>(pred, h, w, gt_u, gt_v, flags, dims, Hmax, Wmax, first, part);
  DFE_LAUNCH_CHECK();
  k_eval_flow_fold<<<n, 64, 0, st>>>(part, records);
  return launch_status();
}

int dfe_eval_flow_finish(const double* records, int N, int has_moving, double* table, void* stream) {
  if (!records || !table) return DFE_ERR_NULL;
  if (N < 1 || !aligned8(records) || !aligned8(table)) return DFE_ERR_DIMS;
  k_eval_flow_finish<<<1, 64, 0, static_cast<hipStream_t>(stream)>>>(records, N, has_moving != 0, table);
  return launch_status();
}

int dfe_eval_depth(const float* disp, int n, int h, int w, const float* gt, const int* dims, int N, int Hmax, int Wmax, int first,
                   float min_depth, float max_depth, void* ws, long ws_bytes, double* records, void* stream) {
  if (!disp || !gt || !dims || !ws || !records) return DFE_ERR_NULL;
  if (!batch_ok(n, h, w, N, Hmax, Wmax, first)) return DFE_ERR_DIMS;
  if (!aligned16(gt) || !aligned16(ws) || !aligned8(records)) return DFE_ERR_DIMS;
  const DepthWs l = depth_ws(n, Hmax, Wmax);
  if (ws_bytes < l.total) return DFE_ERR_WORKSPACE;
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* base = static_cast<char*>(ws);
  float* pred = reinterpret_cast<float*>(base + l.pred);
  double* part = reinterpret_cast<double*>(base + l.part);
  int* hist = reinterpret_cast<int*>(base + l.hist);
  unsigned* state = reinterpret_cast<unsigned*>(base + l.state);
  if (hipMemsetAsync(hist, 0, static_cast<size_t>(n) * SEL * BINS * 4, st) != hipSuccess) return DFE_ERR_LAUNCH;
  const dim3 grid(DEPTH_BPS, n);
  k_eval_depth_hist<true><<<grid, EVAL_THREADS, 0, st>>>(disp, h, w, gt, dims, Hmax, Wmax, first, min_depth, max_depth, pred, hist, state, 0);
  DFE_LAUNCH_CHECK();
  k_eval_depth_pick<<<n, EVAL_THREADS, 0, st>>>(hist, state, 0);
  DFE_LAUNCH_CHECK();
  for (int d = 1; d < 4; ++d) {
    k_eval_depth_hist<false><<<grid, EVAL_THREADS, 0, st>>>(disp, h, w, gt, dims, Hmax, Wmax, first, min_depth, max_depth, pred, hist, state, d);
    DFE_LAUNCH_CHECK();
    k_eval_depth_pick<<<n, EVAL_THREADS, 0, st>>>(hist, state, d);
    DFE_LAUNCH_CHECK();
  }
  k_eval_depth_sums<<<grid, EVAL_THREADS, 0, st>>>(gt, dims, Hmax, Wmax, first, min_depth, max_depth, pred, state, part);
  DFE_LAUNCH_CHECK();
  k_eval_depth_fold<<<n, 64, 0, st>>>(part, state, records);
  return launch_status();
}

}  // extern "C"
