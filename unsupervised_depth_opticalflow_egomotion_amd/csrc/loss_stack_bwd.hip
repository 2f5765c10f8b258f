// Fused loss stack, backward: dfe_geom_loss_bwd (include/dfe_hip.h).
//
// Recompute-in-backward: only the 1-byte mask pack, the masked warped images and the
// per-(sample,scale) normalisers survive from the forward.  Launches:
//   k_geom_ssim_bwd_roll    dL/d(warped) of the SSIM term: rolling 60-column strips, DPP row sums, register windows
//   k_geom_point_bwd        per pixel, both directions: bilinear-warp and projection chain rule,
//                           writes grad_flow / grad_disp(target), block sums for the pose
//   k_geom_flow_smooth_bwd  adds the 2nd-order smoothness gradient into grad_flow
//   k_geom_disp_smooth_bwd1 dL/d(up-sampled disp) per full-res pixel (writes scale 0 directly)
//   k_geom_disp_smooth_bwd2 adjoint of the bilinear up-sampling as a gather per low-res pixel (register path for
//                           ratios >= 1/4, k_geom_disp_smooth_bwd2_coarse = one wave per pixel below that)
//   k_geom_pose_finalize    fixed-order reduction + closed-form 3x3 chains -> grad_pose
// No float atomics anywhere (the one scatter, of the optional depth-consistency term, adds 64-bit fixed-point
// integers): gradients are bitwise reproducible run to run.
// The three point kernels (k_geom_ / k_depth_ / k_flow_point_bwd) share the gradient pieces stated once above
// k_geom_point_bwd: flow_warp_grad, flow_consis_grad, depth_consis_grad.  k_depth_ and k_flow_point_bwd find their pixel
// with locate_pixel (loss_stack_exact.h); k_geom_point_bwd keeps its own prologue and its own reconstruction-gradient
// loop (see the note above it).  Argument check, event timing and the scale-count dispatch come from loss_stack.h.
#include "loss_stack_exact.h"
#include "dfe_scatter.h"
#include <cstdlib>

// wave footprint of the pointwise kernels: DFE_PB_TILE x (64 / DFE_PB_TILE) pixels (tile_pixel, loss_stack_exact.h); 0 = a row segment
#ifndef DFE_PB_TILE
#define DFE_PB_TILE 16
#endif
// 1: the SSIM backward takes value and partials from one refined reciprocal (dfe_device.h: ssim_value_partials_y); 0: two divisions
#ifndef DFE_SSIM_BWD_RCP
#define DFE_SSIM_BWD_RCP 1
#endif

namespace dfe {

struct GeomBwd {
  const float* gl;      // [DFE_NUM_LOSSES][B]
  const float* coef;    // [B][S][CF_COUNT]
  float* gw[DFE_MAX_SCALES];     // [2][B][3][N_s]
  float* gup;           // [3][S-1][B][N_0]
  float* gdisp[3][DFE_MAX_SCALES];
  float* gflow[2][DFE_MAX_SCALES];
  float* bpart;         // [B][nblk_total][PB_COUNT]
  float* gyr[DFE_MAX_SCALES];    // depth-SSIM term: dL/d(masked rigid reconstruction) [2][B][3][N_s]
  int rmw_all;          // depth-consistency term: grad_disp of the SOURCE frames already holds the projected-depth
                        // scatter when the smoothness kernels run -> they add instead of store
  float* adjp;          // coarse levels: per-segment column sums of the up-sampled gradients (GeomLayout::o_adjp)
  int adj_all, adj_s0, adj_nseg, adj_L[DFE_MAX_SCALES];   // adj_all: every pixel of the levels >= adj_s0 (no register-path pixels)
  const unsigned* scq_header;                  // ... and that scatter's fixed-point accumulators (dfe_scatter.h)
  long long* gdq[2][DFE_MAX_SCALES];           // [source frame 0 / 2][scale] -> [B][N_s]
};

// Bound of every value the depth-consistency term scatters: d q / d pd = gq (-a - b q), |.| <= gq (1 + q) / |cd + pd|
// <= gq * 2 / 2e-3 (q <= 1 inside the clamp; both depths are clamped at 1e-3).  gq is uniform per (sample, scale,
// direction).  <<<1, 64>>>; writes the workspace header.
__global__ void __launch_bounds__(64) k_geom_scatter_bound(GeomDev D, GeomBwd G, unsigned* __restrict__ header) {
  unsigned m = 0u;
  for (int i = threadIdx.x; i < D.B * D.S * 2; i += 64) {
    const int d = i & 1, s = (i >> 1) % D.S, b = (i >> 1) / D.S;
    const float gl = G.gl[DFE_LOSS_DEPTH_CONSIS * D.B + b];
    const float gq = D.mode == 1 ? gl / static_cast<float>(D.N[s])
                                 : gl * 3.0f * G.coef[(static_cast<long>(b) * D.S + s) * CF_COUNT + d * CF_PER_DIR + CF_DEPTH];
    m = max(m, static_cast<unsigned>(__float_as_int(gq * 1000.0f)) & 0x7fffffffu);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, static_cast<unsigned>(__shfl_xor(static_cast<int>(m), o)));
  if (threadIdx.x == 0) *header = m;
}

__device__ __forceinline__ float sgn(float v) { return static_cast<float>(v > 0.0f) - static_cast<float>(v < 0.0f); }

// ---------------------------------------------------------------------- SSIM backward, rolling window
// Same structure as k_geom_ssim_fwd_roll with a 2-lane / 2-row halo: raw rows -> DPP row sums -> SSIM
// partial-derivative coefficients of the row above -> DPP row sums of the coefficients -> 3-row sum ->
// dL/d(warped) of the row two above.  Lanes 2..61 are valid (60 columns per wave).  The centre values needed
// at gradient time are re-loaded (prefetched) instead of kept, so every rolling window has period 3 and the
// 3-way unrolled loop needs no register shuffling.
struct CoefH { float v[9]; };

__device__ __forceinline__ CoefH ssim_coef_hsum(const RowSums& r0, const RowSums& r1, const RowSums& r2, float gscale, bool in) {
  CoefH o;
  const float r9 = 1.0f / 9.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float c_my = 0.0f, c_eyy = 0.0f, c_exy = 0.0f;
    const float mx = ((r0.v[c * 5] + r1.v[c * 5]) + r2.v[c * 5]) * r9, my = ((r0.v[c * 5 + 1] + r1.v[c * 5 + 1]) + r2.v[c * 5 + 1]) * r9;
    const float exx = ((r0.v[c * 5 + 2] + r1.v[c * 5 + 2]) + r2.v[c * 5 + 2]) * r9, eyy = ((r0.v[c * 5 + 3] + r1.v[c * 5 + 3]) + r2.v[c * 5 + 3]) * r9;
    const float exy = ((r0.v[c * 5 + 4] + r1.v[c * 5 + 4]) + r2.v[c * 5 + 4]) * r9;
#if DFE_SSIM_BWD_RCP
    float d_my, d_eyy, d_exy;
    const float v = (1.0f - ssim_value_partials_y(mx, my, exx, eyy, exy, d_my, d_eyy, d_exy)) * 0.5f;
    if (in && v >= 0.0f && v <= 1.0f) {   // coefficients exist only at real pixels; clamp passes gradient on [0,1]
      c_my = d_my * gscale; c_eyy = d_eyy * gscale; c_exy = d_exy * gscale;
    }
#else
    const float v = (1.0f - ssim_from_means(mx, my, exx, eyy, exy)) / 2.0f;
    if (in && v >= 0.0f && v <= 1.0f) {   // coefficients exist only at real pixels; clamp passes gradient on [0,1]
      float d_mx, d_my, d_exx, d_eyy, d_exy;
      ssim_partials(mx, my, exx, eyy, exy, d_mx, d_my, d_exx, d_eyy, d_exy);
      c_my = d_my * gscale; c_eyy = d_eyy * gscale; c_exy = d_exy * gscale;
    }
#endif
    o.v[c * 3 + 0] = wave_nbr_sum(c_my); o.v[c * 3 + 1] = wave_nbr_sum(c_eyy); o.v[c * 3 + 2] = wave_nbr_sum(c_exy);
  }
  return o;
}

// gw: the three gradient planes as a buffer (wave-uniform base), voff = the lane's column as a byte offset, rowoff = row * W * 4 (scalar)
__device__ __forceinline__ void ssim_grad_store(const CoefH& a, const CoefH& bq, const CoefH& cq, const RowRaw& ctr,
                                                __amdgpu_buffer_rsrc_t gw, unsigned voff, unsigned rowoff, unsigned N4) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float s0 = (a.v[c * 3] + bq.v[c * 3]) + cq.v[c * 3], s1 = (a.v[c * 3 + 1] + bq.v[c * 3 + 1]) + cq.v[c * 3 + 1];
    const float s2 = (a.v[c * 3 + 2] + bq.v[c * 3 + 2]) + cq.v[c * 3 + 2];
    const float g = ((s0 + 2.0f * ctr.b[c] * s1 + ctr.a[c] * s2) * (1.0f / 9.0f)) * ctr.vo;
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, g), gw, voff, rowoff + c * N4, 0);
  }
}

#ifndef DFE_SSIM_BWD_WAVES
#define DFE_SSIM_BWD_WAVES 5     // waves per SIMD the register allocation must leave room for (<= 96 VGPRs): at B = 4 the launch has 4 736 waves
#endif                           // and the chip holds 4 096 at 4 per SIMD (101 VGPRs as compiled freely) -- a second, 16 %-full round
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(DFE_SSIM_BWD_WAVES)))
k_geom_ssim_bwd_roll(GeomDev D, GeomBwd G, int rigid) {
  const unsigned nunit_total = D.rollb_start[D.S];
  const unsigned unit = xcd_swizzle(blockIdx.x, nunit_total);
  const int b = blockIdx.y >> 1, d = blockIdx.y & 1;
  const int s = find_scale(D.rollb_start, D.S, unit);
  const int H = D.H[s], W = D.W[s], N = D.N[s];
  const int u = unit - D.rollb_start[s];
  const int strip = u % D.rollb_strips[s], rb = u / D.rollb_strips[s];
  const int x = strip * RSB_COLS + static_cast<int>(threadIdx.x) - 2, y0 = rb * RSB_ROWS, yend = min(y0 + RSB_ROWS, H);
  const float* it = D.pyr[1][s] + static_cast<long>(b) * 3 * N;
  const float* yw = (rigid ? D.yr[s] : D.yw[s]) + (static_cast<long>(d) * D.B + b) * 3 * N;
  const unsigned char* mk = D.mode == 2 ? reinterpret_cast<const unsigned char*>(D.wgt[s] + (static_cast<long>(d) * D.B + b) * N)
                                        : D.mask[s] + static_cast<long>(b) * N;
  const unsigned need = D.mode == 2 ? 0u : (rigid ? rigid_ssim_mask(D.mode) : DFE_MASK_VALID_BWD | DFE_MASK_OCC_BWD) << d;
  float* gw = (rigid ? G.gyr[s] : G.gw[s]) + (static_cast<long>(d) * D.B + b) * 3 * N;
  const float gscale = -0.5f * G.gl[(rigid ? DFE_LOSS_DEPTH_SSIM : DFE_LOSS_FLOW_SSIM) * D.B + b] *
                       G.coef[(static_cast<long>(b) * D.S + s) * CF_COUNT + d * CF_PER_DIR + (rigid ? CF_DEPTH : CF_VO)];
  const bool col_in = x >= 0 && x < W;
  const bool lane_ok = threadIdx.x >= 2 && threadIdx.x <= RSB_COLS + 1 && col_in;
  const auto SB = SSIM_SOURCE(it, yw, mk, need, x, H, W, N);
  const __amdgpu_buffer_rsrc_t gwb = __builtin_amdgcn_make_buffer_rsrc(gw, 0, 12 * N, 0x00020000);
#if DFE_SSIM_BUF
  const unsigned gcol = SB.colf;                                  // stores are made by the lanes with lane_ok only: inside the image
#else
  const unsigned gcol = 4u * static_cast<unsigned>(x);
#endif
  const unsigned N4 = 4u * N, W4 = 4u * W;
  // prologue: row sums of rows y0-2, y0-1, y0; coefficient sums of rows y0-1 (and y0 inside the loop)
  RowRaw w0 = ssim_load(SB, y0 - 2), w1 = ssim_load(SB, y0 - 1);
  RowRaw w2 = ssim_load(SB, y0), w3 = ssim_load(SB, y0 + 1);
  RowSums ha = ssim_hsum(w0), hb = ssim_hsum(w1), hc = ssim_hsum(w2);
  CoefH ca = ssim_coef_hsum(ha, hb, hc, gscale, col_in && y0 - 1 >= 0 && y0 - 1 < H);   // coefficients of row y0-1
  RowSums hd = ssim_hsum(w3);
  CoefH cb = ssim_coef_hsum(hb, hc, hd, gscale, col_in && y0 < H);                        // row y0
  // invariant at the top of each third of the loop body for gradient row g:
  //   h?,h?: row sums of rows g, g+1 ; c?,c?: coefficient sums of rows g-1, g
  RowRaw nx = ssim_load(SB, y0 + 2);
  for (int g = y0; g < yend; g += 3) {
    // ---- gradient row g: needs row sums g+2 -> coefficients g+1
    {
      const RowRaw pf = ssim_load(SB, g + 3);
      const RowRaw ctr = ssim_load(SB, g);
      ha = ssim_hsum(nx);                                                                   // rows: hc=g, hd=g+1, ha=g+2
      CoefH cc = ssim_coef_hsum(hc, hd, ha, gscale, col_in && g + 1 < H);                   // row g+1
      if (lane_ok && g < yend) ssim_grad_store(ca, cb, cc, ctr, gwb, gcol, static_cast<unsigned>(g) * W4, N4);
      ca = cc; nx = pf;   // now: cb = row g, ca = row g+1
    }
    // ---- gradient row g+1
    {
      const RowRaw pf = ssim_load(SB, g + 4);
      const RowRaw ctr = ssim_load(SB, g + 1);
      hb = ssim_hsum(nx);                                                                   // rows: hd=g+1, ha=g+2, hb=g+3
      CoefH cc = ssim_coef_hsum(hd, ha, hb, gscale, col_in && g + 2 < H);                   // row g+2
      if (lane_ok && g + 1 < yend) ssim_grad_store(cb, ca, cc, ctr, gwb, gcol, static_cast<unsigned>(g + 1) * W4, N4);
      cb = cc; nx = pf;   // now: ca = row g+1, cb = row g+2
    }
    // ---- gradient row g+2
    {
      const RowRaw pf = ssim_load(SB, g + 5);
      const RowRaw ctr = ssim_load(SB, g + 2);
      hc = ssim_hsum(nx);                                                                   // rows: ha=g+2, hb=g+3, hc=g+4
      CoefH cc = ssim_coef_hsum(ha, hb, hc, gscale, col_in && g + 3 < H);                   // row g+3
      if (lane_ok && g + 2 < yend) ssim_grad_store(ca, cb, cc, ctr, gwb, gcol, static_cast<unsigned>(g + 2) * W4, N4);
      // rotate for the next iteration (gradient row g+3): row sums hc=g+3?? -> rename below
      ca = cb; cb = cc; nx = pf;    // ca = row g+2, cb = row g+3
      const RowSums t0 = hb, t1 = hc;   // rows g+3, g+4
      hc = t0; hd = t1;                 // loop invariant: hc = row g', hd = row g'+1 with g' = g+3
    }
  }
}

// ---------------------------------------------------------------------- pointwise backward
// DT: + the two optional depth terms (dfe_geom_args.depth_terms): dL/d(rigid reconstruction) of the SSIM launch over
// the rigid warps (G.gyr), and the depth-consistency term's gradient wrt the computed depth (the projection's Z), the
// rigid coordinate (through the sampled source disparity) and the source disparity itself (bilinear scatter in 64-bit
// fixed point, dfe_scatter.h: order-independent).
//
// The gradient pieces that more than one of the three kernels needs, each stated once.  What the kernels deliberately do
// differently stays with them: the projection and grid variants (project_fast / rigid_grid_d / flow_coords_d and rcp_nr
// in the geom kernel, the IEEE forms in the depth and flow kernels) and the weights l1c, gq and k they pass in.
// The area-pyramid reconstruction loop stays written out in k_geom_point_bwd and k_depth_point_bwd: see below.

// Flow warp of one direction at the tap (ix, iy): dL/d(flow) of the L1 term (weight l1c) and of the SSIM term (gw: its
// gradient wrt the warped image at this pixel, plane stride N); zero where the warp is not kept.
__device__ __forceinline__ void flow_warp_grad(const float* __restrict__ src, const float* __restrict__ gw, float ix, float iy,
                                               int H, int W, int N, int ac, const float (&im)[3], float l1c, float& gfu, float& gfv) {
  const Tap t = make_tap(ix, iy, H, W);
  if (tap_cover(t) < 0.9999f) return;
  float gix = 0.0f, giy = 0.0f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const Corners q = load_corners(src + static_cast<long>(c) * N, t, W, H);
    float dx, dy;
    interp_grad(q, t, dx, dy);
    const float g = gw[static_cast<long>(c) * N] + sgn(interp(q, t) - im[c]) * l1c;
    gix += g * dx; giy += g * dy;
  }
  gfu = gix * flow_coord_scale(W, ac);
  gfv = giy * flow_coord_scale(H, ac);
}

// Flow consistency: only the forward flow carries gradient (bwd is detached).  k = (1 - occlusion weight) x normaliser x
// dL/d(loss), formed by the caller.
__device__ __forceinline__ void flow_consis_grad(const float (&fu)[2], const float (&fv)[2], float k, float& gfu, float& gfv) {
  if (k == 0.0f) return;
  const float rf = sqrtf(fu[1] * fu[1] + fv[1] * fv[1]), nf = rf + 1e-12f;
  const float nb = l2norm2(fu[0], fv[0]);
  const float uu = fu[1] / nf, uv = fv[1] / nf;
  const float au = sgn(uu + fu[0] / nb) * k, av = sgn(uv + fv[0] / nb) * k;
  const float ir = (rf > 0.0f) ? 1.0f / (rf * nf * nf) : 0.0f, inf_ = rcp_nr(nf);     // nf >= 1e-12
  gfu += au * (inf_ - fu[1] * fu[1] * ir) + av * (-fv[1] * fu[1] * ir);
  gfv += au * (-fu[1] * fv[1] * ir) + av * (inf_ - fv[1] * fv[1] * ir);
}

// Depth consistency q = |cd - pd| / |cd + pd| clamped to [0,1] (gradient passes on the closed interval, like
// torch.clamp), weight gq: gZ = d/d(cd), the rigid coordinate's share through the sampled source disparity `dsrc` into
// (gix, giy), and d/d(that disparity) as a four-tap scatter in 64-bit fixed point into `gdq` (null: not wanted).
__device__ __forceinline__ void depth_consis_grad(const float* __restrict__ dsrc, long long* gdq, const unsigned* scq_header,
                                                  const Tap& t, int H, int W, float cd, float gq, float& gZ, float& gix, float& giy) {
  const Corners qd = load_corners(dsrc, t, W, H);
  const float v = interp(qd, t);
  const float pd = (v >= 1e-3f || v != v) ? v : 1e-3f;
  const float num = cd - pd, den = cd + pd, qv = fabsf(num) / fabsf(den);
  if (!(qv >= 0.0f && qv <= 1.0f)) return;
  const float a = sgn(num) / fabsf(den), bq = qv * sgn(den) / fabsf(den);
  gZ = gq * (a - bq);                       // d q / d cd
  const float gp = (v >= 1e-3f) ? gq * (-a - bq) : 0.0f;   // d q / d pd, cut by the clamp(min=1e-3)
  float dx, dy;
  interp_grad(qd, t, dx, dy);
  gix += gp * dx; giy += gp * dy;
  if (gdq && gp != 0.0f) {
    long long* base = gdq + static_cast<long>(t.y0) * W + t.x0;
    const float gs = gp * scatter_scale(*scq_header).to_fixed;
    if (t.in_nw) fixed_add(base, to_fixed(gs, t.nw));
    if (t.in_ne) fixed_add(base + 1, to_fixed(gs, t.ne));
    if (t.in_sw) fixed_add(base + W, to_fixed(gs, t.sw));
    if (t.in_se) fixed_add(base + W + 1, to_fixed(gs, t.se));
  }
}

#ifndef DFE_PB_WPE
#define DFE_PB_WPE 0             // 0: the compiler's own register budget (90 VGPRs = 5 waves per SIMD)
#endif
#if DFE_PB_WPE
#define DFE_PB_ATTR __attribute__((amdgpu_waves_per_eu(DFE_PB_WPE, DFE_PB_WPE)))
#else
#define DFE_PB_ATTR
#endif
// k_geom_point_bwd<true> compiles at the scalar-register ceiling (106 SGPRs), where the number of scalar registers the
// compiler spills to vector lanes moves with the kernel's text.  With locate_pixel in place of the prologue below it
// spills 4 to 6 whatever else is folded, with the reconstruction loop behind a shared function 3, as written here 1
// (profiles/loss_stack_point_refactor.txt, A2).  So the prologue and that loop stay written out in this kernel.
template <bool DT>
__global__ void __launch_bounds__(GS_BLOCK) DFE_PB_ATTR k_geom_point_bwd(GeomDev D, GeomT T, GeomBwd G) {
  __shared__ float red[PB_COUNT * 4 * (GS_BLOCK / 64)];
  const unsigned nblk_total = D.blk_start[D.S];
  const unsigned blk = xcd_swizzle(blockIdx.x, nblk_total);
  const int b = blockIdx.y, B = D.B;
  const int s = find_scale(D.blk_start, D.S, blk);
  const int H = D.H[s], W = D.W[s], N = D.N[s];
  const int pl = (blk - D.blk_start[s]) * GS_BLOCK + threadIdx.x;
  float acc[PB_COUNT];
#pragma unroll
  for (int i = 0; i < PB_COUNT; ++i) acc[i] = 0.0f;
  if (pl < N) {
    unsigned upx, upy;
    tile_pixel<DFE_PB_TILE>(static_cast<unsigned>(pl), W, H, T.rW[s], upx, upy);     // wave footprint: loss_stack_exact.h
    const int px = static_cast<int>(upx), py = static_cast<int>(upy), p = py * W + px;
    const Divisor dw = T.dw[s], dh = T.dh[s];
    const long o3 = static_cast<long>(b) * 3 * N + p, o2 = static_cast<long>(b) * 2 * N + p, o1 = static_cast<long>(b) * N + p;
    const float* it = D.pyr[1][s];
    const float im[3] = {it[o3], it[o3 + N], it[o3 + 2 * N]};
    const unsigned bits = D.mask[s][o1];
    const float dsp = D.disp[1][s][o1];
    const float* cf = G.coef + (static_cast<long>(b) * D.S + s) * CF_COUNT;
    const float g_dp = G.gl[DFE_LOSS_DEPTH_PIXEL * B + b], g_fp = G.gl[DFE_LOSS_FLOW_PIXEL * B + b];
    const float g_fc = G.gl[DFE_LOSS_FLOW_CONSIS * B + b], g_dfc = G.gl[DFE_LOSS_DEPTH_FLOW_CONSIS * B + b];
    const float g_epi = G.gl[DFE_LOSS_EPIPOLAR * B + b];
    float fu[2], fv[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) { fu[d] = D.flow[d][s][o2]; fv[d] = D.flow[d][s][o2 + N]; }
    float gdisp = 0.0f;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const bool valid = bits & (DFE_MASK_VALID_BWD << d), occ = bits & (DFE_MASK_OCC_BWD << d);
      const bool dyna = bits & (DFE_MASK_DYNA_BWD << d), tex = bits & (DFE_MASK_TEX_BWD << d);
      const float vo = (valid && occ) ? 1.0f : 0.0f;
      const float m_rig = dyna ? vo : 0.0f, m_dyn = dyna ? 0.0f : vo, m_tex = tex ? m_rig : 0.0f;
      float gfu = 0.0f, gfv = 0.0f;
      // ---- flow warp: L1 (rigid + 2x dynamic masks) and SSIM gradients wrt the warped image
      {
        float ix, iy;
        flow_coords_d(px, py, fu[d], fv[d], H, W, D.ac, dw, dh, ix, iy);
        const float l1c = g_fp * (m_rig * cf[d * CF_PER_DIR + CF_RIG] + m_dyn * cf[d * CF_PER_DIR + CF_DYN]);
        flow_warp_grad(D.pyr[d == 0 ? 0 : 2][s] + static_cast<long>(b) * 3 * N, G.gw[s] + (static_cast<long>(d) * B + b) * 3 * N + p,
                       ix, iy, H, W, N, D.ac, im, l1c, gfu, gfv);
      }
      // ---- rigid branch
      const Camera& cam = D.cams[(b * 2 + d) * D.S + s];
      Proj pr = project_fast(cam, px, py, dsp);
      float gU = 0.0f, gV = 0.0f, gZ = 0.0f;
      if (m_tex != 0.0f) {
        float xn, yn; bool lx, ly;
        rigid_grid_d(pr, dw, dh, xn, yn, lx, ly);
        Tap t = make_tap(unnormalize(xn, W, D.ac), unnormalize(yn, H, D.ac), H, W);
        const float* ar = D.area[d][s] + static_cast<long>(b) * 3 * N;
        const float gc = g_dp * cf[d * CF_PER_DIR + CF_DEPTH];
        float gix = 0.0f, giy = 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          Corners q = load_corners(ar + static_cast<long>(c) * N, t, W, H);
          float dx, dy;
          interp_grad(q, t, dx, dy);
          float g = sgn(interp(q, t) - im[c]) * gc;
          if (DT && (D.dt & DFE_DEPTH_TERM_SSIM)) g += G.gyr[s][(static_cast<long>(d) * B + b) * 3 * N + static_cast<long>(c) * N + p];
          gix += g * dx; giy += g * dy;
        }
        if (DT && (D.dt & DFE_DEPTH_TERM_CONSIS)) {
          const float gq = G.gl[DFE_LOSS_DEPTH_CONSIS * B + b] * 3.0f * cf[d * CF_PER_DIR + CF_DEPTH];   // 1 / (N n_tex)
          depth_consis_grad(D.disp[2 * d][s] + static_cast<long>(b) * N, G.gdisp[2 * d][s] ? G.gdq[d][s] + static_cast<long>(b) * N : nullptr,
                            G.scq_header, t, H, W, pr.Z, gq, gZ, gix, giy);
        }
        const float sx = D.ac ? static_cast<float>(W - 1) / 2.0f : static_cast<float>(W) / 2.0f;
        const float sy = D.ac ? static_cast<float>(H - 1) / 2.0f : static_cast<float>(H) / 2.0f;
        if (lx) gU = gix * sx * (2.0f * rcp_nr(static_cast<float>(W - 1)));
        if (ly) gV = giy * sy * (2.0f * rcp_nr(static_cast<float>(H - 1)));
      }
      if (s == 0) {
        // depth-flow consistency |rigid - flow| on valid*occ*dyna (model_geometry.py:716-732, scale 0 only)
        const float ru = pr.U - static_cast<float>(px), rv = pr.V - static_cast<float>(py);
        const float g = g_dfc * cf[d * CF_PER_DIR + CF_FD] * m_rig;
        const float su = sgn(ru - fu[d]) * g, sv = sgn(rv - fv[d]) * g;
        gU += su; gV += sv; gfu -= su; gfv -= sv;
        // epipolar distance (plain mean; model_geometry.py:413-418)
        const Epi& e = D.epi[b * 2 + d];
        const float x1 = static_cast<float>(px), y1 = static_cast<float>(py);
        const float l0 = __fmaf_rn(e.F[1], y1, e.F[0] * x1) + e.F[2];
        const float l1 = __fmaf_rn(e.F[4], y1, e.F[3] * x1) + e.F[5];
        const float l2 = __fmaf_rn(e.F[7], y1, e.F[6] * x1) + e.F[8];
        const float r = sqrtf(l0 * l0 + l1 * l1), div = r + 1e-6f;
        const float x2 = x1 + fu[d], y2 = y1 + fv[d];
        const float n = (x2 * l0 + y2 * l1) + l2;
        const float ge = g_epi * rcp_nr(static_cast<float>(N)), sg = sgn(n), idiv = rcp_nr(div);     // div >= 1e-6
        gfu += ge * sg * l0 * idiv; gfv += ge * sg * l1 * idiv;
        const float tail = (r > 0.0f) ? fabsf(n) * idiv * idiv * rcp_nr(r > 0.0f ? r : 1.0f) : 0.0f;
        const float dl0 = ge * (sg * x2 * idiv - tail * l0), dl1 = ge * (sg * y2 * idiv - tail * l1), dl2 = ge * sg * idiv;
        float* aF = acc + d * PB_PER_DIR + 12;
        aF[0] = dl0 * x1; aF[1] = dl0 * y1; aF[2] = dl0;
        aF[3] = dl1 * x1; aF[4] = dl1 * y1; aF[5] = dl1;
        aF[6] = dl2 * x1; aF[7] = dl2 * y1; aF[8] = dl2;
      }
      float gd;
      project_backward(cam, pr, dsp, gU, gV, gZ, gd, acc + d * PB_PER_DIR);
      gdisp += gd;
      if (d == 1) flow_consis_grad(fu, fv, (occ ? 0.0f : 1.0f) * cf[CF_CONSIS] * g_fc, gfu, gfv);
      if (G.gflow[d][s]) { G.gflow[d][s][o2] = gfu; G.gflow[d][s][o2 + N] = gfv; }
    }
    if (G.gdisp[1][s]) G.gdisp[1][s][o1] = gdisp;
  }
  block_sum<PB_COUNT>(acc, red, G.bpart + (static_cast<long>(b) * nblk_total + blk) * PB_COUNT);
}

// ---------------------------------------------------------------------- flow-only pointwise backward
// Model_flow: gradient wrt the flows of the weighted L1 (1-channel mean diff), the SSIM term (gw) and the flow
// consistency (forward flow only); the soft weights are detached (model_flow.py:124).
__global__ void __launch_bounds__(GS_BLOCK) k_flow_point_bwd(GeomDev D, GeomBwd G) {
  const PixelAt at = locate_pixel<DFE_PB_TILE>(D);
  if (!at.live) return;                                // no block sum in this kernel: the early return is legal here only
  const int b = at.b, B = D.B, s = at.s, H = at.H, W = at.W, N = at.N;
  const int px = static_cast<int>(at.px), py = static_cast<int>(at.py), p = static_cast<int>(at.pm);
  const long o3 = static_cast<long>(b) * 3 * N + p, o2 = static_cast<long>(b) * 2 * N + p;
  const float* it = D.pyr[1][s];
  const float im[3] = {it[o3], it[o3 + N], it[o3 + 2 * N]};
  const float* cf = G.coef + (static_cast<long>(b) * D.S + s) * CF_COUNT;
  const float g_fp = G.gl[DFE_LOSS_FLOW_PIXEL * B + b], g_fc = G.gl[DFE_LOSS_FLOW_CONSIS * B + b];
  float fu[2], fv[2];
#pragma unroll
  for (int d = 0; d < 2; ++d) { fu[d] = D.flow[d][s][o2]; fv[d] = D.flow[d][s][o2 + N]; }
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const float wgt = (D.wgt[s] + (static_cast<long>(d) * B + b) * N)[p];
    float gfu = 0.0f, gfv = 0.0f;
    float ix, iy;
    flow_coords(px, py, fu[d], fv[d], H, W, D.ac, ix, iy);
    flow_warp_grad(D.pyr[d == 0 ? 0 : 2][s] + static_cast<long>(b) * 3 * N, G.gw[s] + (static_cast<long>(d) * B + b) * 3 * N + p,
                   ix, iy, H, W, N, D.ac, im, g_fp * wgt * cf[d * CF_PER_DIR + CF_RIG], gfu, gfv);
    if (d == 1) flow_consis_grad(fu, fv, (1.0f - wgt) * cf[CF_CONSIS] * g_fc, gfu, gfv);
    if (G.gflow[d][s]) { G.gflow[d][s][o2] = gfu; G.gflow[d][s][o2 + N] = gfv; }
  }
}

// ---------------------------------------------------------------------- depth-only pointwise backward
// Model_depth: gradient of the masked L1 on the rigid recon wrt the target disparity and the camera sums.
template <bool DT>
__global__ void __launch_bounds__(GS_BLOCK) k_depth_point_bwd(GeomDev D, GeomBwd G) {
  __shared__ float red[PB_COUNT * 4 * (GS_BLOCK / 64)];
  const PixelAt at = locate_pixel<DFE_PB_TILE>(D);
  const int b = at.b, B = D.B, s = at.s, H = at.H, W = at.W, N = at.N;
  float acc[PB_COUNT];
#pragma unroll
  for (int i = 0; i < PB_COUNT; ++i) acc[i] = 0.0f;
  if (at.live) {
    const int px = static_cast<int>(at.px), py = static_cast<int>(at.py), p = static_cast<int>(at.pm);
    const long o3 = static_cast<long>(b) * 3 * N + p, o1 = static_cast<long>(b) * N + p;
    const float* it = D.pyr[1][s];
    const float im[3] = {it[o3], it[o3 + N], it[o3 + 2 * N]};
    const unsigned bits = D.mask[s][o1];
    const float dsp = D.disp[1][s][o1];
    const float* cf = G.coef + (static_cast<long>(b) * D.S + s) * CF_COUNT;
    const float g_dp = G.gl[DFE_LOSS_DEPTH_PIXEL * B + b];
    float gdisp = 0.0f;
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const bool m = (bits & (DFE_MASK_VALID_BWD << d)) && (bits & (DFE_MASK_TEX_BWD << d));
      const Camera& cam = D.cams[(b * 2 + d) * D.S + s];
      Proj pr = project(cam, px, py, dsp);
      float gU = 0.0f, gV = 0.0f, gZ = 0.0f;
      const bool consis = DT && (D.dt & DFE_DEPTH_TERM_CONSIS);      // unmasked in Model_depth: every pixel
      if (m || consis) {
        float xn, yn; bool lx, ly;
        rigid_grid(pr, H, W, xn, yn, lx, ly);
        Tap t = make_tap(unnormalize(xn, W, D.ac), unnormalize(yn, H, D.ac), H, W);
        float gix = 0.0f, giy = 0.0f;
        if (m) {
          const float* ar = D.area[d][s] + static_cast<long>(b) * 3 * N;
          const float gc = g_dp * cf[d * CF_PER_DIR + CF_DEPTH];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            Corners q = load_corners(ar + static_cast<long>(c) * N, t, W, H);
            float dx, dy;
            interp_grad(q, t, dx, dy);
            float g = sgn(interp(q, t) - im[c]) * gc;
            if (DT && (D.dt & DFE_DEPTH_TERM_SSIM)) g += G.gyr[s][(static_cast<long>(d) * B + b) * 3 * N + static_cast<long>(c) * N + p];
            gix += g * dx; giy += g * dy;
          }
        }
        if (consis) depth_consis_grad(D.disp[2 * d][s] + static_cast<long>(b) * N, G.gdisp[2 * d][s] ? G.gdq[d][s] + static_cast<long>(b) * N : nullptr,
                                      G.scq_header, t, H, W, pr.Z, G.gl[DFE_LOSS_DEPTH_CONSIS * B + b] / static_cast<float>(N), gZ, gix, giy);
        const float sx = D.ac ? static_cast<float>(W - 1) / 2.0f : static_cast<float>(W) / 2.0f;
        const float sy = D.ac ? static_cast<float>(H - 1) / 2.0f : static_cast<float>(H) / 2.0f;
        if (lx) gU = gix * sx * (2.0f / static_cast<float>(W - 1));
        if (ly) gV = giy * sy * (2.0f / static_cast<float>(H - 1));
      }
      float gd;
      project_backward(cam, pr, dsp, gU, gV, gZ, gd, acc + d * PB_PER_DIR);
      gdisp += gd;
    }
    if (G.gdisp[1][s]) G.gdisp[1][s][o1] = gdisp;
  }
  block_sum<PB_COUNT>(acc, red, G.bpart + at.slot * PB_COUNT);
}

// ---------------------------------------------------------------------- flow smoothness backward
// Rolling wave kernel (see k_geom_flow_smooth_fwd): per row and lane the signed, weighted second
// differences S (x stencil starting at this lane) and T (y stencil starting at this row) are formed once;
// the gradient of pixel (g, x) is cx (S(x) - 2 S(x-1) + S(x-2)) + cy (T(g) - 2 T(g-1) + T(g-2)), with the x
// neighbours from DPP wave shifts and the y neighbours from a register window.  Lanes 2..61 are valid (60
// columns per wave).  Adds into grad_flow (after k_geom_point_bwd wrote it), both directions per pass.
struct FT { float v[4]; };

__device__ __forceinline__ FT fs_S(const FRow& r, bool ok) {
  FT o;
  float i1[3], i2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { i1[c] = wave_shl1(r.i[c]); i2[c] = wave_shl1(i1[c]); }
  const float w = expf(-10.0f * mean3_abs_diff(i2[0], i2[1], i2[2], i1[0], i1[1], i1[2]));
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float a1 = wave_shl1(r.f[k]), a2 = wave_shl1(a1);
    o.v[k] = ok ? w * sgn((a2 - a1) - (a1 - r.f[k])) : 0.0f;
  }
  return o;
}

__device__ __forceinline__ FT fs_T(const FRow& r0, const FRow& r1, const FRow& r2, bool ok) {
  FT o;
  const float w = expf(-10.0f * mean3_abs_diff(r2.i[0], r2.i[1], r2.i[2], r1.i[0], r1.i[1], r1.i[2]));
#pragma unroll
  for (int k = 0; k < 4; ++k) o.v[k] = ok ? w * sgn((r2.f[k] - r1.f[k]) - (r1.f[k] - r0.f[k])) : 0.0f;
  return o;
}

__device__ __forceinline__ void fs_grad(const FRow& r, const FT& t0, const FT& t1, const FT& t2, bool s_ok, bool out_ok,
                                        float cx, float cy, float* __restrict__ gb, float* __restrict__ gf, int q, int N) {
  const FT s0 = fs_S(r, s_ok);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float s1 = wave_shr1(s0.v[k]), s2 = wave_shr1(s1);
    const float g = cx * ((s0.v[k] - 2.0f * s1) + s2) + cy * ((t0.v[k] - 2.0f * t1.v[k]) + t2.v[k]);
    if (out_ok) {
      float* dst = (k < 2 ? gb : gf) + (k & 1) * N + q;
      if (k < 2 ? gb != nullptr : gf != nullptr) *dst += g;
    }
  }
}

__global__ void __launch_bounds__(64) k_geom_flow_smooth_bwd(GeomDev D, GeomBwd G) {
  const unsigned unit = xcd_swizzle(blockIdx.x, D.rollb_start[D.S]);    // halo-sharing neighbours on one XCD (see k_geom_flow_smooth_fwd)
  const int b = blockIdx.y;
  const int s = find_scale(D.rollb_start, D.S, unit);
  const int H = D.H[s], W = D.W[s], N = D.N[s];
  const int u = unit - D.rollb_start[s];
  const int strip = u % D.rollb_strips[s], rb = u / D.rollb_strips[s];
  const int x = strip * RSB_COLS + static_cast<int>(threadIdx.x) - 2, y0 = rb * RSB_ROWS, yend = min(y0 + RSB_ROWS, H);
  const float* it = D.pyr[1][s] + static_cast<long>(b) * 3 * N;
  const float* fb = D.flow[0][s] + static_cast<long>(b) * 2 * N;
  const float* ff = D.flow[1][s] + static_cast<long>(b) * 2 * N;
  float* gb = G.gflow[0][s] ? G.gflow[0][s] + static_cast<long>(b) * 2 * N : nullptr;
  float* gf = G.gflow[1][s] ? G.gflow[1][s] + static_cast<long>(b) * 2 * N : nullptr;
  const float g = G.gl[DFE_LOSS_FLOW_SMOOTH * D.B + b];
  const float cx = g / (2.0f * H * (W - 2.0f)) / 2.0f / 20.0f, cy = g / (2.0f * (H - 2.0f) * W) / 2.0f / 20.0f;
  const bool col_in = x >= 0 && x < W;
  const bool lane_ok = threadIdx.x >= 2 && threadIdx.x <= RSB_COLS + 1 && col_in;
  const bool s_ok = x >= 0 && x + 2 < W;     // an x stencil starts at this lane
  // raw rows y0-2 .. ; T(r) uses rows r, r+1, r+2 and exists for 0 <= r, r+2 < H
  FRow ra = fs_load(it, fb, ff, y0 - 2, x, H, W, N), rb1 = fs_load(it, fb, ff, y0 - 1, x, H, W, N);
  FRow rc = fs_load(it, fb, ff, y0, x, H, W, N), rd = fs_load(it, fb, ff, y0 + 1, x, H, W, N);
  FRow nx = fs_load(it, fb, ff, y0 + 2, x, H, W, N);
  FT ta = fs_T(ra, rb1, rc, col_in && y0 - 2 >= 0 && y0 < H);          // T(y0-2)
  FT tb = fs_T(rb1, rc, rd, col_in && y0 - 1 >= 0 && y0 + 1 < H);      // T(y0-1)
  // invariant for gradient row gy: rc = row gy, rd = row gy+1, nx = row gy+2; ta = T(gy-2), tb = T(gy-1)
  for (int gy = y0; gy < yend; gy += 3) {
    {
      const FT tc = fs_T(rc, rd, nx, col_in && gy + 2 < H);                                   // T(gy)
      fs_grad(rc, tc, tb, ta, s_ok, lane_ok && gy < yend, cx, cy, gb, gf, gy * W + x, N);
      ta = tc;                                                                                // ta = T(gy), tb = T(gy-1)
      ra = nx; nx = fs_load(it, fb, ff, gy + 3, x, H, W, N);                                  // rows: rd = gy+1, ra = gy+2, nx = gy+3
    }
    {
      const FT tc = fs_T(rd, ra, nx, col_in && gy + 3 < H);                                   // T(gy+1)
      fs_grad(rd, tc, ta, tb, s_ok, lane_ok && gy + 1 < yend, cx, cy, gb, gf, (gy + 1) * W + x, N);
      tb = tc;                                                                                // tb = T(gy+1), ta = T(gy)
      rb1 = nx; nx = fs_load(it, fb, ff, gy + 4, x, H, W, N);                                 // rows: ra = gy+2, rb1 = gy+3, nx = gy+4
    }
    {
      const FT tc = fs_T(ra, rb1, nx, col_in && gy + 4 < H);                                  // T(gy+2)
      fs_grad(ra, tc, tb, ta, s_ok, lane_ok && gy + 2 < yend, cx, cy, gb, gf, (gy + 2) * W + x, N);
      ta = tb; tb = tc;                                                                       // next gy' = gy+3: ta = T(gy'-2), tb = T(gy'-1)
      rc = rb1; rd = nx; nx = fs_load(it, fb, ff, gy + 5, x, H, W, N);                        // rc = row gy', rd = gy'+1, nx = gy'+2
    }
  }
}

// ---------------------------------------------------------------------- disparity smoothness backward
// stage 1: per full-resolution pixel, dL/d(up_s(p)) for every scale.  Rolling wave kernel like
// k_geom_disp_smooth_fwd (lanes 1..62 valid: x-1 and x+1 come from DPP wave shifts).  With
//   A_s(y,x) = sgn(u(y,x) - u(y,x+1)) wx(y,x)   and   B_s(y,x) = sgn(u(y,x) - u(y+1,x)) wy(y,x)
// the gradient is cx (A(y,x) - A(y,x-1)) + cy (B(y,x) - B(y-1,x)); B of the previous row stays in a register,
// the march starts one row early to seed it.  grid: x = units (strip x row block), y = f*B + b.
template <int NS>
__global__ void __launch_bounds__(64) k_geom_disp_smooth_bwd1(GeomDev D, GeomBwd G, int strips) {
  const int f = blockIdx.y / D.B, b = blockIdx.y - f * D.B;
  const int H = D.H[0], W = D.W[0], N = D.N[0];
  const unsigned unit = xcd_swizzle(blockIdx.x, gridDim.x);
  const int strip = unit % strips, rb = unit / strips;
  const int x = strip * RS_COLS + static_cast<int>(threadIdx.x) - 1, xc = min(max(x, 0), W - 1);
  const int y0 = rb * DSM_ROWS, yend = min(y0 + DSM_ROWS, H), ys = max(y0 - 1, 0);
  const float* im = D.pyr[f][0] + static_cast<long>(b) * 3 * N;
  const float* d0 = D.disp[f][0] + static_cast<long>(b) * N;
  const bool col_in = x >= 0 && x < W;
  const bool lane_ok = threadIdx.x >= 1 && threadIdx.x <= RS_COLS && col_in;
  const bool hxp = col_in && x + 1 < W, hxm = x > 0;
  const float g = G.gl[DFE_LOSS_DEPTH_SMOOTH * D.B + b];
  const float cx = g / (static_cast<float>(H) * (W - 1.0f)), cy = g / ((H - 1.0f) * static_cast<float>(W));
  UpMap mp[NS > 1 ? NS - 1 : 1];
  UpCache ch[NS > 1 ? NS - 1 : 1];
  const bool small_out = aten_small_resize(H, W);   // tiny full-resolution images only (see up_row)
  const float* dps[NS > 1 ? NS - 1 : 1];
  float rhs[NS > 1 ? NS - 1 : 1];
#pragma unroll
  for (int s = 1; s < NS; ++s) {
    bilinear_src(xc, static_cast<float>(D.W[s]) / W, D.W[s], mp[s - 1].x0, mp[s - 1].x1, mp[s - 1].l0, mp[s - 1].l1);
    ch[s - 1].r0 = -1; ch[s - 1].r1 = -1; ch[s - 1].h0 = 0.0f; ch[s - 1].h1 = 0.0f;
    dps[s - 1] = D.disp[f][s] + static_cast<long>(b) * D.N[s];
    rhs[s - 1] = static_cast<float>(D.H[s]) / H;
  }
  int q = ys * W + xc;
  float c0 = im[q], c1 = im[q + N], c2 = im[q + 2 * N];
  float u[NS], bprev[NS];
  u[0] = d0[q];
#pragma unroll
  for (int s = 1; s < NS; ++s) u[s] = up_row(dps[s - 1], D.H[s], D.W[s], rhs[s - 1], ys, mp[s - 1], ch[s - 1], small_out);
#pragma unroll
  for (int s = 0; s < NS; ++s) bprev[s] = 0.0f;
  int qn = min(ys + 1, H - 1) * W + xc;
  float n0 = im[qn], n1 = im[qn + N], n2 = im[qn + 2 * N], nd = d0[qn];
  for (int y = ys; y < yend; ++y) {
    const float e0 = n0, e1 = n1, e2 = n2, ed = nd;          // row y+1
    const int qf = min(y + 2, H - 1) * W + xc;                // issue the loads of row y+2
    n0 = im[qf]; n1 = im[qf + N]; n2 = im[qf + 2 * N]; nd = d0[qf];
    const bool hyp = col_in && y + 1 < H;
    const float wx = expf(-mean3_abs_diff(c0, c1, c2, wave_shl1(c0), wave_shl1(c1), wave_shl1(c2)));
    const float wy = expf(-mean3_abs_diff(c0, c1, c2, e0, e1, e2));
    float un[NS];
    un[0] = ed;
#pragma unroll
    for (int s = 1; s < NS; ++s) un[s] = up_row(dps[s - 1], D.H[s], D.W[s], rhs[s - 1], min(y + 1, H - 1), mp[s - 1], ch[s - 1], small_out);
    const bool store = lane_ok && y >= y0;
    const long p = static_cast<long>(y) * W + x;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      // DPP shifts must run with every lane enabled: a lane reading a neighbour that EXEC disabled gets 0
      const float ur = wave_shl1(u[s]);
      const float A = hxp ? sgn(u[s] - ur) * wx : 0.0f;
      const float Am = wave_shr1(A);
      const float Bv = hyp ? sgn(u[s] - un[s]) * wy : 0.0f;
      const float gsum = cx * (A - (hxm ? Am : 0.0f)) + cy * (Bv - bprev[s]);
      if (store) {
        if (s == 0) {
          float* o = G.gdisp[f][0];
          if (o) { if (f == 1 || G.rmw_all) o[static_cast<long>(b) * N + p] += gsum; else o[static_cast<long>(b) * N + p] = gsum; }
        } else {
          G.gup[((static_cast<long>(f) * (D.S - 1) + (s - 1)) * D.B + b) * N + p] = gsum;
        }
      }
      bprev[s] = Bv;
      u[s] = un[s];
    }
    c0 = e0; c1 = e1; c2 = e2;
  }
}

// stage 2: adjoint of the bilinear up-sampling as a gather, one thread per low-res pixel of scales >= 1
// (deterministic: no scatter atomics).  The adjoint is separable: the weight of full-res pixel (y, x) on low-res
// pixel (i, j) is wy(y) * wx(x), so the (at most G2_MAX) candidate rows / columns and their weights are formed
// once per thread and the double loop only touches the non-zero taps (16 at ratio 1/2, 64 at 1/4).
// grid.x covers blocks [blk_start[1], blk_start[S]); grid.y = f*B + b.
// exact 1/2 and 1/4 pyramids (every power-of-two image size), interior low-res pixels: the footprint is the dense
// 2n x 2n block starting at (n i - n/2, n j - n/2) with the tent weights (2k + 1) / 2n mirrored -- the same non-zero
// taps, weights and summation order as the general path below, without forming 24 candidate weights and issuing 144
// mostly-masked loads per pixel (36 us -> see profiles; bit-identical results).
template <int NR>   // n = NR: 2 or 4
__device__ __forceinline__ float adj_pow2(const float* __restrict__ gu, int W, int y0, int x0) {
  constexpr int NT = 2 * NR;
  float w[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) w[k] = (k < NR) ? (2.0f * k + 1.0f) / (2.0f * NR) : (2.0f * (NT - 1 - k) + 1.0f) / (2.0f * NR);
  float total = 0.0f;
#pragma unroll
  for (int ky = 0; ky < NT; ++ky) {
    const float* row = gu + static_cast<long>(y0 + ky) * W + x0;
    float v[NT];
    // pairs of horizontally adjacent taps as one dword-aligned 8-byte load (x0 = 4 j - 2 is 8-byte aligned, x0 = 2 j - 1
    // only dword aligned: the load is still one instruction; round 3: 16 -> 8 loads per pixel at the 1/2 level)
#pragma unroll
    for (int k = 0; k < NT; k += 2) { const PairF q = *reinterpret_cast<const PairF*>(row + k); v[k] = q.a; v[k + 1] = q.b; }
    float acc = 0.0f;
#pragma unroll
    for (int kx = 0; kx < NT; ++kx) acc += w[kx] * v[kx];
    total += w[ky] * acc;
  }
  return total;
}

// Measured and rejected in round 3: a rolling form of this adjoint for the interior of exact 1/2 and 1/4 levels (a wave
// marches down 64 full-resolution columns, every up-sampled gradient read once with a coalesced dword per lane, tent sums
// by DPP shifts and two rolling accumulators; bit-identical results) plus this kernel for the border ring: 36-38 us
// against 23.8 us here -- three launches instead of one, 18 / 36 dependent rows per wave and only every 2nd / 4th lane
// producing an output, against 16-32 independent loads per thread below.
__global__ void __launch_bounds__(GS_BLOCK) k_geom_disp_smooth_bwd2(GeomDev D, GeomBwd G) {
  const unsigned blk = blockIdx.x + D.blk_start[1];
  const int f = blockIdx.y / D.B, b = blockIdx.y - f * D.B;
  const int s = find_scale(D.blk_start, D.S, blk);
  const int Hs = D.H[s], Ws = D.W[s], Ns = D.N[s];
  const int q = (blk - D.blk_start[s]) * GS_BLOCK + threadIdx.x;
  if (q >= Ns || !G.gdisp[f][s]) return;
  const int H = D.H[0], W = D.W[0], N = D.N[0];
  // thread -> pixel: the (Hs-2) x (Ws-2) interior pixels first, then the border ring, so that a wave runs either the
  // dense fast path or the general one (a row-major map puts two border pixels into almost every wave)
  int i, j;
  {
    const int wi = Ws - 2, nint = (Hs - 2) * wi;
    if (q < nint) { i = 1 + q / wi; j = 1 + q - (i - 1) * wi; }
    else {
      const int e = q - nint;
      if (e < Ws) { i = 0; j = e; }
      else if (e < 2 * Ws) { i = Hs - 1; j = e - Ws; }
      else if (e < 2 * Ws + (Hs - 2)) { i = 1 + (e - 2 * Ws); j = 0; }
      else { i = 1 + (e - 2 * Ws - (Hs - 2)); j = Ws - 1; }
    }
  }
  const float rh = static_cast<float>(Hs) / H, rw = static_cast<float>(Ws) / W;
  const float* gu = G.gup + ((static_cast<long>(f) * (D.S - 1) + (s - 1)) * D.B + b) * N;
  float* o = G.gdisp[f][s] + static_cast<long>(b) * Ns + static_cast<long>(i) * Ws + j;
  const int nr = H / Hs;
  if ((nr == 2 || nr == 4) && Hs * nr == H && Ws * nr == W && i >= 1 && i < Hs - 1 && j >= 1 && j < Ws - 1) {
    const float t = nr == 2 ? adj_pow2<2>(gu, W, 2 * i - 1, 2 * j - 1) : adj_pow2<4>(gu, W, 4 * i - 2, 4 * j - 2);
    if (f == 1 || G.rmw_all) *o += t; else *o = t;
    return;
  }
  float total = 0.0f;
  int ylo, ny, xlo, nx;
  float wy[G2_MAX], wx[G2_MAX];
  adj_weights(i, rh, Hs, H, ylo, ny, wy);
  adj_weights(j, rw, Ws, W, xlo, nx, wx);
  if (ny > G2_MAX || nx > G2_MAX) return;      // large footprint: k_geom_disp_smooth_bwd2_coarse owns this pixel
#pragma unroll
  for (int ky = 0; ky < G2_MAX; ++ky) {
    if (wy[ky] == 0.0f) continue;
    const float* row = gu + static_cast<long>(ylo + ky) * W + xlo;
    float acc = 0.0f;
#pragma unroll
    for (int kx = 0; kx < G2_MAX; ++kx)
      if (wx[kx] != 0.0f) acc += wx[kx] * row[kx];
    total += wy[ky] * acc;
  }
  if (f == 1 || G.rmw_all) *o += total; else *o = total;
}

// Coarse scales (ratio < 1/4, footprints of up to (2^(s+1)+4)^2 full-res pixels per low-res pixel): a group of
// g = 16 / 32 / 64 lanes per low-res pixel (g = the scale's widest footprint rounded up, so 4 / 2 / 1 pixels share a
// wave).  Lanes stride over the footprint columns (a lane's horizontal weight is fixed for its whole march) and walk
// the rows four at a time (four independent loads in flight); a fixed-order DPP tree adds the lane sums of a group.
// Pixels whose clamped footprint fits the register path above are skipped here (same predicate on both sides).
// grid.x = sum_{s >= s0} ceil(N_s * g_s / 64) wave units, 4 per block; grid.y = f*B + b.
__device__ __forceinline__ void adj_range(int i, float r, int fullN, int& lo, int& cnt) {
  lo = max(static_cast<int>(floorf((i - 0.5f) / r - 0.5f)) - 1, 0);
  const int hi = min(static_cast<int>(ceilf((i + 1.5f) / r - 0.5f)) + 1, fullN - 1);
  cnt = hi - lo + 1;
}

__host__ __device__ __forceinline__ int coarse_group(int W, int Ws) {
  const int nxmax = (2 * W + Ws - 1) / Ws + 4;
  return nxmax <= 16 ? 16 : nxmax <= 32 ? 32 : 64;
}

struct AdjMarch {
  const float* gu; float rh, rw; int Hs, Ws, W, i, j, ylo, ny, xlo, nx, g, lx, gbase; float wrow; bool mine, tall;
};

template <int U>
__device__ __forceinline__ float adj_march(const AdjMarch& m) {
  float total = 0.0f;
  const int yend = m.ylo + m.ny;
  for (int x = m.xlo + m.lx; __any(x < m.xlo + m.nx); x += m.g) {
    const bool on = m.mine && x < m.xlo + m.nx;
    const int xc = min(x, m.W - 1);
    int c0, c1; float m0, m1;
    bilinear_src(xc, m.rw, m.Ws, c0, c1, m0, m1);
    const float wxx = on ? ((c0 == m.j ? m0 : 0.0f) + (c1 == m.j ? m1 : 0.0f)) : 0.0f;
    float col = 0.0f;
    for (int y = 0; __any(y < m.ny); y += U) {
      float wy[U], v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = y + u;
        const int yy = min(m.ylo + k, yend - 1);
        if (m.tall) {
          int a0, a1; float l0, l1;
          bilinear_src(yy, m.rh, m.Hs, a0, a1, l0, l1);
          wy[u] = (k < m.ny) ? ((a0 == m.i ? l0 : 0.0f) + (a1 == m.i ? l1 : 0.0f)) : 0.0f;
        } else {
          const float w = __shfl(m.wrow, m.gbase + min(k, m.g - 1));     // executed by every lane of the wave
          wy[u] = (k < m.ny) ? w : 0.0f;
        }
        v[u] = (wxx != 0.0f) ? m.gu[static_cast<long>(yy) * m.W + xc] : 0.0f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) col += wy[u] * v[u];
    }
    total += wxx * col;
  }
  return total;
}

__global__ void __launch_bounds__(GS_BLOCK) k_geom_disp_smooth_bwd2_coarse(GeomDev D, GeomBwd G, int s0) {
  const int f = blockIdx.y / D.B, b = blockIdx.y - f * D.B;
  const int lane = threadIdx.x & 63;
  int unit = blockIdx.x * (GS_BLOCK / 64) + (threadIdx.x >> 6);
  int s = s0, g = 64;
  for (; s < D.S; ++s) {
    g = coarse_group(D.W[0], D.W[s]);
    const int units = (D.N[s] * (g / 16) + 3) / 4;      // ceil(N_s / (64 / g))
    if (unit < units) break;
    unit -= units;
  }
  if (s >= D.S || !G.gdisp[f][s]) return;
  const int Hs = D.H[s], Ws = D.W[s], Ns = D.N[s];
  const int H = D.H[0], W = D.W[0], N = D.N[0];
  const int lx = lane & (g - 1);
  const int q = unit * (64 / g) + lane / g;
  const bool live = q < Ns;
  const int qq = live ? q : Ns - 1;
  const int i = qq / Ws, j = qq - i * Ws;
  const float rh = static_cast<float>(Hs) / H, rw = static_cast<float>(Ws) / W;
  int ylo, ny, xlo, nx;
  adj_range(i, rh, H, ylo, ny);
  adj_range(j, rw, W, xlo, nx);
  const bool mine = live && (ny > G2_MAX || nx > G2_MAX);
  const float* gu = G.gup + ((static_cast<long>(f) * (D.S - 1) + (s - 1)) * D.B + b) * N;
  float total = 0.0f;
  // vertical weights: lane lx of the group forms the weight of footprint row ylo + lx once; the march below
  // fetches it from that lane (ds_bpermute).  Footprints taller than the group recompute (tiny odd-shaped inputs).
  float wrow = 0.0f;
  {
    int a0, a1; float l0, l1;
    bilinear_src(min(ylo + lx, H - 1), rh, Hs, a0, a1, l0, l1);
    wrow = (lx < ny) ? ((a0 == i ? l0 : 0.0f) + (a1 == i ? l1 : 0.0f)) : 0.0f;
  }
  const bool tall = __any(ny > g);
  const int gbase = lane & ~(g - 1);
  AdjMarch m{gu, rh, rw, Hs, Ws, W, i, j, ylo, ny, xlo, nx, g, lx, gbase, wrow, mine, tall};
  // widest footprints (g = 64: up to 2^(s+1)+4 rows) keep 16 row loads in flight, the others 4
  total = (g == 64) ? adj_march<16>(m) : adj_march<4>(m);
  // re-converged: butterfly inside each 16-lane row, then the rows of a group in a fixed order
  total = dpp_add<0xB1>(total);
  total = dpp_add<0x4E>(total);
  total = dpp_add<0x141>(total);
  total = dpp_add<0x140>(total);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(total), 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(total), 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(total), 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(total), 48));
  float t;
  if (g == 16) t = total;                                   // each row is one pixel
  else if (g == 32) t = lane < 32 ? r0 + r1 : r2 + r3;
  else t = (r0 + r1) + (r2 + r3);
  if (mine && lx == 0) {
    float* o = G.gdisp[f][s] + static_cast<long>(b) * Ns + q;
    if (f == 1 || G.rmw_all) *o += t; else *o = t;
  }
}

// ---------------------------------------------------------------------- coarse levels: the adjoint in two passes
// Round 4 (VERDICT r03 missing #6): the up-sampling is separable, U = U_y (x) U_x, so is its adjoint.  The wave-per-pixel
// gather above read every up-sampled gradient ~4x and marched footprints of up to 68 x 68 pixels per coarse pixel
// (91 us at B = 2, 583 us at B = 16 on the 375 x 1242 six-scale pyramid: the most expensive launch there).
//   k_geom_adj_rows: lanes along x (coalesced 256-byte rows), a wave owns 64 columns x one segment of L <= 32 rows and
//                    all L loads are in flight at once; the rows' vertical weights are wave-uniform; the <= 8 low-res
//                    rows the segment touches are 8 register accumulators -> P[f][s][b][segment][slot][x].
//                    Every up-sampled gradient is read exactly once, at streaming rate.
//   k_geom_adj_cols: one thread per coarse pixel: the horizontal weights over its (<= 68 wide) footprint of the few
//                    segment sums that hold its row.  P is W_0 * 8 * H_0 / L floats per (frame, level, sample): L2-sized.
// Fixed summation order (segments in order, columns in order): bitwise reproducible.  Pixels whose clamped footprint
// fits the register path of k_geom_disp_smooth_bwd2 stay there (same predicate on both sides).
__device__ __forceinline__ long adj_plane(const GeomDev& D, const GeomBwd& G, int f, int s, int b) {
  return ((static_cast<long>(f) * (D.S - G.adj_s0) + (s - G.adj_s0)) * D.B + b) * G.adj_nseg * ADJ_SLOTS * D.W[0];
}

// grid: x = ceil(strips / 4) * adj_nseg, y = f*B + b, z = s - adj_s0; block = 4 waves = 4 strips of 64 columns
__global__ void __launch_bounds__(256) k_geom_adj_rows(GeomDev D, GeomBwd G) {
  const int f = blockIdx.y / D.B, b = blockIdx.y - f * D.B, s = G.adj_s0 + blockIdx.z;
  if (!G.gdisp[f][s]) return;
  const int H = D.H[0], W = D.W[0], N = D.N[0], Hs = D.H[s], L = G.adj_L[s];
  const int sgroups = ((W + 63) / 64 + 3) / 4;
  const int seg = blockIdx.x / sgroups, x = ((blockIdx.x - seg * sgroups) * 4 + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
  const int y0 = seg * L;
  if (y0 >= H || x >= W) return;
  const int nrows = min(L, H - y0);
  const float rh = static_cast<float>(Hs) / H;
  const float* gu = G.gup + ((static_cast<long>(f) * (D.S - 1) + (s - 1)) * D.B + b) * N + static_cast<long>(y0) * W + x;
  float v[ADJ_LMAX];
#pragma unroll
  for (int r = 0; r < ADJ_LMAX; ++r) v[r] = (r < nrows) ? gu[static_cast<long>(r) * W] : 0.0f;
  int cur, t1; float u0, u1;
  bilinear_src(y0, rh, Hs, cur, t1, u0, u1);
  // The vertical taps of a row are wave-uniform (scalar control flow): `a` collects low-res row `cur`, `nx` the row below
  // it; when the first tap moves on (by one row: the ratio is below 1/2) `a` is stored as the next slot.  (A first
  // version added every row into 8 select-masked accumulators: 1 500 vector instructions per wave, 3x this.)
  float* P = G.adjp + adj_plane(D, G, f, s, b) + static_cast<long>(seg) * ADJ_SLOTS * W + x;
  float* const Pend = P + static_cast<long>(ADJ_SLOTS) * W;
  float a = 0.0f, nx = 0.0f;
#pragma unroll
  for (int r = 0; r < ADJ_LMAX; ++r) {
    if (r < nrows) {                              // wave-uniform
      int a0, a1; float l0, l1;
      bilinear_src(y0 + r, rh, Hs, a0, a1, l0, l1);
      if (a0 != cur) { *P = a; P += W; a = nx; nx = 0.0f; cur = a0; }
      a = __fmaf_rn(l0, v[r], a);
      if (a1 != a0) nx = __fmaf_rn(l1, v[r], nx); else a = __fmaf_rn(l1, v[r], a);
    }
  }
  *P = a; P += W;
  if (P < Pend) { *P = nx; P += W; }
  for (; P < Pend; P += W) *P = 0.0f;
}

// grid: x = sum_{s >= adj_s0} ceil(N_s / 256) blocks, y = f*B + b
__global__ void __launch_bounds__(GS_BLOCK) k_geom_adj_cols(GeomDev D, GeomBwd G) {
  const int f = blockIdx.y / D.B, b = blockIdx.y - f * D.B;
  int blk = blockIdx.x, s = G.adj_s0;
  for (; s < D.S; ++s) {
    const int nb = (D.N[s] + GS_BLOCK - 1) / GS_BLOCK;
    if (blk < nb) break;
    blk -= nb;
  }
  if (s >= D.S || !G.gdisp[f][s]) return;
  const int Hs = D.H[s], Ws = D.W[s], Ns = D.N[s], H = D.H[0], W = D.W[0], L = G.adj_L[s];
  const int q = blk * GS_BLOCK + threadIdx.x;
  if (q >= Ns) return;
  const int i = q / Ws, j = q - i * Ws;
  const float rh = static_cast<float>(Hs) / H, rw = static_cast<float>(Ws) / W;
  int ylo, ny, xlo, nx;
  adj_range(i, rh, H, ylo, ny);
  adj_range(j, rw, W, xlo, nx);
  if (!G.adj_all && !(ny > G2_MAX || nx > G2_MAX)) return;      // "mixed" mode: small clamped footprint, k_geom_disp_smooth_bwd2 owns this pixel
  // the segments whose rows can touch low-res row i, and the slot row i has in each
  const int klo = ylo / L, khi = min((ylo + ny - 1) / L, G.adj_nseg - 1);
  const float* P = G.adjp + adj_plane(D, G, f, s, b);
  float total = 0.0f;
  for (int k = klo; k <= khi; ++k) {
    int ibase, t1; float u0, u1;
    bilinear_src(k * L, rh, Hs, ibase, t1, u0, u1);
    const int slot = i - ibase;
    if (slot < 0 || slot >= ADJ_SLOTS) continue;
    const float* row = P + (static_cast<long>(k) * ADJ_SLOTS + slot) * W;
    float part = 0.0f;
#pragma unroll 4
    for (int x = xlo; x < xlo + nx; ++x) {
      int c0, c1; float m0, m1;
      bilinear_src(x, rw, Ws, c0, c1, m0, m1);
      const float wxx = (c0 == j ? m0 : 0.0f) + (c1 == j ? m1 : 0.0f);
      part = __fmaf_rn(wxx, row[x], part);
    }
    total += part;
  }
  float* o = G.gdisp[f][s] + static_cast<long>(b) * Ns + q;
  if (f == 1 || G.rmw_all) *o += total; else *o = total;
}

// ---------------------------------------------------------------------- pose finalize
// (Measured and rejected in round 3: one wave per camera with a shuffle butterfly instead of the LDS pass -- 16.7 us against
// 15.0; and running it as an extra block row of k_geom_disp_smooth_bwd1 -- its 21 double accumulators lift that kernel from
// 58 to 145 VGPRs.)
// One 256-thread block per (b, d).  Per scale, thread t accumulates rows k = t (mod 256) of the 21
// columns (12 camera sums + 9 dF sums, the latter only at scale 0) in double; the 256 per-thread sums of a column
// are then added in two fixed-order stages (32 at a time, then the 8 parts: reproducible).
__global__ void __launch_bounds__(256) k_geom_pose_finalize(GeomDev D, GeomBwd G, float* __restrict__ gpose) {
  __shared__ double lds[256][PB_PER_DIR + 1];
  __shared__ double parts[8][PB_PER_DIR + 1];
  __shared__ double sm[DFE_MAX_SCALES * 12 + 9];
  const int cam = blockIdx.x, b = cam >> 1, d = cam & 1, S = D.S, t = threadIdx.x;
  const unsigned nblk_total = D.blk_start[S];
  for (int s = 0; s < S; ++s) {
    double a[PB_PER_DIR];
#pragma unroll
    for (int i = 0; i < PB_PER_DIR; ++i) a[i] = 0.0;
    // four rows' loads in flight at once, added in row order (the same sums as one row at a time)
    const float* base = G.bpart + static_cast<long>(b) * nblk_total * PB_COUNT + d * PB_PER_DIR;
    const int kend = D.blk_start[s + 1];
    int k = D.blk_start[s] + t;
    for (; k + 3 * 256 < kend; k += 4 * 256) {
      float v[4][PB_PER_DIR];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < PB_PER_DIR; ++i) v[u][i] = base[static_cast<long>(k + u * 256) * PB_COUNT + i];
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < PB_PER_DIR; ++i) a[i] += v[u][i];
    }
    for (; k < kend; k += 256) {
      const float* r = base + static_cast<long>(k) * PB_COUNT;
#pragma unroll
      for (int i = 0; i < PB_PER_DIR; ++i) a[i] += r[i];
    }
#pragma unroll
    for (int i = 0; i < PB_PER_DIR; ++i) lds[t][i] = a[i];
    __syncthreads();
    // column sums in two fixed-order stages: 8 x 21 threads add 32 per-thread sums each, then 21 threads add the 8 parts
    if (t < 8 * PB_PER_DIR) {
      const int c = t % PB_PER_DIR, part = t / PB_PER_DIR;
      double v = 0.0;
      for (int k = part * 32; k < part * 32 + 32; ++k) v += lds[k][c];
      parts[part][c] = v;
    }
    __syncthreads();
    if (t < PB_PER_DIR) {
      double v = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) v += parts[k][t];
      if (t < 12) sm[s * 12 + t] = v;
      else if (s == 0) sm[S * 12 + (t - 12)] = v;
    }
    __syncthreads();
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double g[6] = {0, 0, 0, 0, 0, 0}, gR[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int s = 0; s < S; ++s) {
    const double* acc = sm + s * 12;
    const Camera& c = D.cams[cam * S + s];
    for (int j = 0; j < 3; ++j) g[j] += c.K[j] * acc[0] + c.K[3 + j] * acc[1] + c.K[6 + j] * acc[2];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) gR[i * 3 + j] += c.K[i] * acc[3 + j] + c.K[3 + i] * acc[6 + j] + c.K[6 + i] * acc[9 + j];
  }
  const Camera& c0 = D.cams[cam * S];
  if (D.mode == 0) {
  // epipolar: F = Ki^T E Ki, E = S R
  const Epi& e = D.epi[cam];
  const double* gF = sm + S * 12;
  double T[9], gE[9];
  for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) T[r * 3 + q] = e.Kinv[r * 3] * gF[q] + e.Kinv[r * 3 + 1] * gF[3 + q] + e.Kinv[r * 3 + 2] * gF[6 + q];
  for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) gE[r * 3 + q] = T[r * 3] * e.Kinv[q * 3] + T[r * 3 + 1] * e.Kinv[q * 3 + 1] + T[r * 3 + 2] * e.Kinv[q * 3 + 2];
  double gS[9];
  for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) {
    double a = 0, bq = 0;
    for (int k = 0; k < 3; ++k) { a += e.S[k * 3 + r] * gE[k * 3 + q]; bq += gE[r * 3 + k] * c0.R[q * 3 + k]; }
    gR[r * 3 + q] += a; gS[r * 3 + q] = bq;
  }
  g[0] += gS[7] - gS[5]; g[1] += gS[2] - gS[6]; g[2] += gS[3] - gS[1];
  }
  for (int k = 0; k < 3; ++k) { double t = 0; for (int i = 0; i < 9; ++i) t += gR[i] * c0.dR[k * 9 + i]; g[3 + k] += t; }
  for (int i = 0; i < 6; ++i) gpose[cam * 6 + i] = static_cast<float>(g[i]);
}

}  // namespace dfe

using namespace dfe;


static int geom_bwd_impl(const dfe_geom_args* a, void* stream, hipEvent_t* ev) {
  GeomLayout L;
  int rc = geom_layout(a, &L);
  if (rc != DFE_OK) return rc;
  rc = check_args(a, L, true);
  if (rc != DFE_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* ws = a->workspace;
  GeomDev D;
  geom_dev(a, L, &D);
  GeomT T{};
  tile_dev(L, &T);
  GeomBwd G;
  G.gl = a->grad_losses; G.coef = ws + L.o_coef; G.gup = ws + L.o_gup; G.bpart = ws + L.o_bpart;
  for (int s = 0; s < DFE_MAX_SCALES; ++s) {
    G.gw[s] = (s < L.S) ? ws + L.o_gw + 6L * L.B * L.off_px[s] : nullptr;
    for (int f = 0; f < 3; ++f) G.gdisp[f][s] = (s < L.S) ? a->grad_disp[f][s] : nullptr;
    for (int d = 0; d < 2; ++d) G.gflow[d][s] = (s < L.S) ? a->grad_flow[d][s] : nullptr;
  }
  for (int s = 0; s < DFE_MAX_SCALES; ++s) G.gyr[s] = (s < L.S) ? ws + L.o_gyr + 6L * L.B * L.off_px[s] : nullptr;
  G.adjp = ws + L.o_adjp; G.adj_s0 = L.adj_s0; G.adj_nseg = L.adj_nseg; G.adj_all = L.adj_mode == 0;
  for (int s = 0; s < DFE_MAX_SCALES; ++s) G.adj_L[s] = L.adj_L[s];
  G.rmw_all = (L.dt & DFE_DEPTH_TERM_CONSIS) ? 1 : 0;
  G.scq_header = reinterpret_cast<const unsigned*>(ws + L.o_scq);
  for (int fi = 0; fi < 2; ++fi)
    for (int s = 0; s < DFE_MAX_SCALES; ++s)
      G.gdq[fi][s] = (G.rmw_all && s < L.S) ? scatter_acc(ws + L.o_scq) + (static_cast<long>(fi) * L.off_px[L.S] + L.off_px[s]) * L.B : nullptr;
  const unsigned nblk_total = L.blk_start[L.S];
  int seg = 0;
  if (ev) (void)hipEventRecord(ev[0], st);
  if (G.rmw_all) {   // the projected-depth scatter: zero accumulators + the analytic bound of what is added to them
    const int rc = scatter_begin_bound(ws + L.o_scq, 2L * L.B * L.off_px[L.S], st);
    if (rc != DFE_OK) return rc;
    k_geom_scatter_bound<<<1, 64, 0, st>>>(D, G, reinterpret_cast<unsigned*>(ws + L.o_scq));
    DFE_LAUNCH_CHECK();
  }
  // ... and its sums become the source frames' disparity gradients before the smoothness kernels add to them
  auto finish_scatter = [&]() -> int {
    if (!G.rmw_all) return DFE_OK;
    for (int fi = 0; fi < 2; ++fi)
      for (int s = 0; s < L.S; ++s)
        if (a->grad_disp[2 * fi][s]) {
          const int rc = scatter_finish_at(G.scq_header, G.gdq[fi][s], a->grad_disp[2 * fi][s], static_cast<long>(L.B) * L.N[s], st);
          if (rc != DFE_OK) return rc;
        }
    return DFE_OK;
  };
  if (a->mode == 2) {
    k_geom_ssim_bwd_roll<<<dim3(L.rollb_start[L.S], L.B * 2), 64, 0, st>>>(D, G, 0);
    DFE_LAUNCH_CHECK();
    DFE_MARK();
    k_flow_point_bwd<<<dim3(nblk_total, L.B), GS_BLOCK, 0, st>>>(D, G);
    DFE_LAUNCH_CHECK();
    DFE_MARK();
    k_geom_flow_smooth_bwd<<<dim3(L.rollb_start[L.S], L.B), 64, 0, st>>>(D, G);
    DFE_LAUNCH_CHECK();
    DFE_MARK(); DFE_MARK(); DFE_MARK(); DFE_MARK();
    return DFE_OK;
  }
  if (a->mode == 1) {
    if (L.dt & DFE_DEPTH_TERM_SSIM) {
      k_geom_ssim_bwd_roll<<<dim3(L.rollb_start[L.S], L.B * 2), 64, 0, st>>>(D, G, 1);
      DFE_LAUNCH_CHECK();
    }
    DFE_MARK();
    if (L.dt) k_depth_point_bwd<true><<<dim3(nblk_total, L.B), GS_BLOCK, 0, st>>>(D, G);
    else k_depth_point_bwd<false><<<dim3(nblk_total, L.B), GS_BLOCK, 0, st>>>(D, G);
    DFE_LAUNCH_CHECK();
    { const int rc = finish_scatter(); if (rc != DFE_OK) return rc; }
    DFE_MARK(); DFE_MARK();
  } else {
    k_geom_ssim_bwd_roll<<<dim3(L.rollb_start[L.S], L.B * 2), 64, 0, st>>>(D, G, 0);
    DFE_LAUNCH_CHECK();
    if (L.dt & DFE_DEPTH_TERM_SSIM) {
      k_geom_ssim_bwd_roll<<<dim3(L.rollb_start[L.S], L.B * 2), 64, 0, st>>>(D, G, 1);
      DFE_LAUNCH_CHECK();
    }
    DFE_MARK();
    if (L.dt) k_geom_point_bwd<true><<<dim3(nblk_total, L.B), GS_BLOCK, 0, st>>>(D, T, G);
    else k_geom_point_bwd<false><<<dim3(nblk_total, L.B), GS_BLOCK, 0, st>>>(D, T, G);
    DFE_LAUNCH_CHECK();
    { const int rc = finish_scatter(); if (rc != DFE_OK) return rc; }
    DFE_MARK();
    k_geom_flow_smooth_bwd<<<dim3(L.rollb_start[L.S], L.B), 64, 0, st>>>(D, G);
    DFE_LAUNCH_CHECK();
    DFE_MARK();
  }
  {
    const dim3 g(L.dsm_units, 3 * L.B);
    with_num_scales(L.S, [&](auto ns) { k_geom_disp_smooth_bwd1<decltype(ns)::value><<<g, 64, 0, st>>>(D, G, L.dsm_strips); });
  }
  DFE_LAUNCH_CHECK();
  DFE_MARK();
  if (L.S > 1) {
    if (L.adj_mode != 0) {
      k_geom_disp_smooth_bwd2<<<dim3(nblk_total - L.blk_start[1], 3 * L.B), GS_BLOCK, 0, st>>>(D, G);
      DFE_LAUNCH_CHECK();
    }
    // the adjoint in two passes, rows then columns (every level, or in "mixed" mode the levels coarser than 1/4)
    const int s0 = L.adj_s0;
    if (s0 < L.S) {
      if (L.adj_mode == 2) {
        long units = 0;
        for (int s = s0; s < L.S; ++s) units += (static_cast<long>(L.N[s]) * (coarse_group(L.W[0], L.W[s]) / 16) + 3) / 4;
        k_geom_disp_smooth_bwd2_coarse<<<dim3(static_cast<unsigned>((units + GS_BLOCK / 64 - 1) / (GS_BLOCK / 64)), 3 * L.B), GS_BLOCK, 0, st>>>(D, G, s0);
        DFE_LAUNCH_CHECK();
      } else {
        const int sgroups = ((L.W[0] + 63) / 64 + 3) / 4;
        k_geom_adj_rows<<<dim3(sgroups * L.adj_nseg, 3 * L.B, L.S - s0), 256, 0, st>>>(D, G);
        DFE_LAUNCH_CHECK();
        unsigned nb = 0;
        for (int s = s0; s < L.S; ++s) nb += (L.N[s] + GS_BLOCK - 1) / GS_BLOCK;
        k_geom_adj_cols<<<dim3(nb, 3 * L.B), GS_BLOCK, 0, st>>>(D, G);
        DFE_LAUNCH_CHECK();
      }
    }
  }
  DFE_MARK();
  if (a->grad_pose) {
    k_geom_pose_finalize<<<L.B * 2, 256, 0, st>>>(D, G, a->grad_pose);
    DFE_LAUNCH_CHECK();
  }
  DFE_MARK();
  return DFE_OK;
}

extern "C" int dfe_geom_loss_bwd(const dfe_geom_args* a, void* stream) { return geom_bwd_impl(a, stream, nullptr); }

extern "C" int dfe_geom_loss_bwd_profiled(const dfe_geom_args* a, void* stream, float* ms_host) {
  return geom_profiled(geom_bwd_impl, DFE_GEOM_BWD_SEGMENTS, a, stream, ms_host);
}

// see dfe_geom_loss_fwd_timed: the same handle, collected by dfe_geom_timed_collect
extern "C" int dfe_geom_loss_bwd_timed(const dfe_geom_args* a, void* stream, void** handle) {
  return geom_timed(geom_bwd_impl, DFE_GEOM_BWD_SEGMENTS, a, stream, handle);
}
