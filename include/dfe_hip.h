/* libdfe_hip.so -- C ABI of the MI355X (gfx950) photometric-warping loss stack.
 *
 * Drop-in boundary for the hot path of jianfenglihg/Unsupervised_depth_OpticalFlow_egomotion.
 * The reference has no FFI: its boundary is the Python signatures cited on each entry point
 * below (paths relative to the reference checkout).  A maintainer binds these symbols with
 * ctypes from the cited Python function (see INTEGRATION.md for the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous fp32 NCHW data unless it says "host";
 *   - the caller owns every buffer (inputs, outputs, workspaces); nothing here allocates,
 *     frees or synchronises; all work is enqueued on `stream` (a hipStream_t, NULL = default);
 *   - return value: DFE_OK (0) or a negative DFE_ERR_* code; no C++ exception crosses the ABI;
 *   - no module-global state: entry points are re-entrant and may be called from the autograd
 *     backward thread (contrast the racy pixel_coords cache, inverse_warp.py:6-18);
 *   - `align_corners` is the grid_sample convention (the reference leaves it to the installed
 *     torch; 0 is what torch >= 1.3 does, 1 is torch <= 1.2).
 */
#ifndef DFE_HIP_H
#define DFE_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define DFE_OK 0
#define DFE_ERR_NULL (-1)        /* a required pointer is NULL */
#define DFE_ERR_DIMS (-2)        /* a dimension is out of range */
#define DFE_ERR_LAUNCH (-3)      /* hipGetLastError() reported a launch failure */
#define DFE_ERR_UNSUPPORTED (-4) /* argument value outside what the kernels implement */
#define DFE_ERR_WORKSPACE (-5)   /* workspace too small */

#define DFE_MAX_SCALES 8
/* Bumped whenever an exported signature changes, an entry point is removed or the host side starts to rely on a new one
 * (2: round 5 changed dfe_wino_wgrad3x3 and removed dfe_thin_conv3x3 / dfe_cast_*; 3: round 6 added dfe_pwc_level_map_bytes /
 * _fwd_map / _bwd_map, which ops.py calls; 4: dfe_sconv_fwd / _dgrad and dfe_conv1x1s2_fwd / _wgrad with their host-only queries,
 * which the deterministic mode calls).  _lib.py compares the library's value with this header's.  It also reads every
 * ctypes argument and return type from the prototypes below (a new entry point is bound by declaring it here), so a prototype
 * stays within: pointers of any kind, int, long, float, double, unsigned long long; returning int, long or const char*. */
#define DFE_ABI_VERSION 4

int dfe_abi_version(void);
const char* dfe_error_string(int code);

/* ---- cameras ----------------------------------------------------------------------------
 * Per (sample, direction, scale) projection block: K_s = K with rows 0-1 / downscale[s]
 * (model_geometry.py:92-93,696-697), K_s^-1, A = K_s R, b = K_s t with R = Rx Ry Rz
 * (inverse_warp.py:110-145,172-187,284-291).  pose [B,ndir,6]; K [B,3,3];
 * cams: B*ndir*nscale*dfe_camera_floats() floats, index (b*ndir+d)*nscale+s;
 * downscale_host: nscale host floats.
 * Memory contract: reads pose [B*ndir*6] and K [B*9], writes exactly B*ndir*nscale*dfe_camera_floats() floats of cams (one
 * thread per camera, 64 per block) and nothing else; no scratch.  Every device pointer needs dword alignment only.  A refusal
 * (a NULL pointer, a dimension <= 0, nscale above the library's limit) comes before the launch and leaves cams untouched. */
int dfe_camera_floats(void);
int dfe_prepare_cameras(const float* pose, const float* K, float* cams, int B, int ndir, int nscale,
                        const float* downscale_host, void* stream);

/* pose_vec2mat (inverse_warp.py:172-187) -> T34 [n,3,4] and/or compute_essential_matrix
 * (inverse_warp.py:354-364) -> E [n,3,3]; either output may be NULL.
 * Memory contract: the forward reads vec [n,6] and writes every element of whichever of T34 / E is given; the backward reads
 * vec and whichever of gT34 / gE is given (not both NULL) and writes every element of gvec [n,6].  Nothing else is read or
 * written, no scratch; every pointer needs dword alignment only and the result does not depend on it.  The forward matrices
 * are the reference's fp32 arithmetic bit for bit (correctly rounded cos / sin); the backward sums in double. */
int dfe_pose_vec2mat_fwd(const float* vec, float* T34, float* E, int n, void* stream);
int dfe_pose_vec2mat_bwd(const float* vec, const float* gT34, const float* gE, float* gvec, int n, void* stream);

/* ---- Adam update of many tensors in one launch  train.py:85-87 (torch.optim.Adam, default betas / eps) ---------------
 * table: device array of ntensors records {float* p, const float* g, float* m, float* v, int64 n} (5 x 8 bytes);
 * blockmap: device int32 pairs (tensor, chunk), one per block of dfe_adam_chunk() elements; bias_correction1 / 2 =
 * 1 - beta^t of the step count t.  m = m + (1-b1)(g-m); v = b2 v + (1-b2) g g; p -= (lr/c1) m / (sqrt(v)/sqrt(c2) + eps). */
int dfe_adam_chunk(void);
int dfe_adam_step(const void* table, const int* blockmap, int nblocks, double lr, double beta1, double beta2, double eps,
                  double bias_correction1, double bias_correction2, void* stream);
/* the same update with the step count on the device (a step replayed from a hipGraph: train.py --graph): one extra one-thread
 * launch increments *step_count (a device double) and forms the two bias-correction coefficients in coef (two device floats),
 * which the update kernel reads. */
int dfe_adam_step_dev(const void* table, const int* blockmap, int nblocks, double lr, double beta1, double beta2, double eps,
                      double* step_count, float* coef, void* stream);

/* ---- gradient guard in front of the Adam update: torch.nn.utils.clip_grad_norm_(params, max_norm) and GradScaler's
 * "skip the step whose gradients are not finite" (without the scaling), decided on the device so that a captured step can
 * take them.  The gradients are READ once more and never written: the update multiplies by the coefficient on the fly.
 * dfe_grad_guard: (1) one block per block-map entry sums the squares of its gradient chunk in double (fp32 x fp32 is exact
 * in double; a gradient of 1e30 gives a large finite norm) in a fixed order and notes whether an element is NaN / +-inf
 * (from the exponent bits) -> ws: nblocks doubles followed by nblocks int32 flags, dfe_grad_guard_ws_bytes(nblocks) bytes,
 * 8-byte aligned, every byte written on every call; (2) one block adds the partials in a fixed order and writes record
 * (dfe_grad_guard_record_bytes() = 32 bytes, 8-byte aligned):
 *   double norm    = sqrt(sum g^2) over every element the block map covers
 *   double skipped   running count of skipped steps (the caller zeroes it once)
 *   float  c       = float(min(1, max_norm / (norm + 1e-6))) formed in double; exactly 1 when max_norm <= 0 (no clipping)
 *   int32  finite  = no element is NaN / +-inf;  int32 skip = skip_nonfinite && !finite;  int32 0
 * not skipping, it then does what dfe_adam_step_dev's first launch does (*step_count += 1, the two coefficients into coef);
 * skipping, the count stays and skipped += 1.  With clipping on and skip_nonfinite off a non-finite norm goes through the
 * formula as in torch: c = 0 for an inf norm, NaN for a NaN norm.
 * dfe_adam_tick_guarded: the same conditional count + coefficients for one more param group that shares the record
 * (one global norm over several groups: its table and block map cover all of them, each group steps with its own).
 * dfe_adam_step_guarded: dfe_adam_step_dev's update with the gradient fl32(g * c) (one fp32 product; g itself when c == 1);
 * when record says skip, no p, m or v is read or written. */
int dfe_grad_guard_ws_bytes(int nblocks);
int dfe_grad_guard_record_bytes(void);
int dfe_grad_guard(const void* table, const int* blockmap, int nblocks, double max_norm, int skip_nonfinite, double lr, double beta1,
                   double beta2, void* ws, double* step_count, float* coef, void* record, void* stream);
int dfe_adam_tick_guarded(double lr, double beta1, double beta2, double* step_count, float* coef, const void* record, void* stream);
int dfe_adam_step_guarded(const void* table, const int* blockmap, int nblocks, double beta1, double beta2, double eps,
                          const float* coef, const void* record, void* stream);

/* ---- order-independent scatter-add workspace (csrc/dfe_scatter.h) -----------------------------
 * Adjoint of a bilinear gather with respect to the sampled tensor: contributions are scaled by a power of two, rounded
 * once to 64-bit integers, added with integer atomics (associative: no dependence on the order the atomics retire in)
 * and converted back in one pass -- bitwise reproducible, no float atomics anywhere in the library.  A scatter into
 * n floats needs a 16-byte aligned workspace of dfe_scatter_ws_bytes(n) bytes (64 + 8 n); the library zero-fills it. */
long dfe_scatter_ws_bytes(long n);

/* ---- warp_flow(x, flow, use_mask)  net_utils.py:16-54 --------------------------------------
 * x [B,C,H,W], flow [B,2,H,W] -> out [B,C,H,W].  Backward: gflow [B,2,H,W] (NULL to skip),
 * gx [B,C,H,W] (NULL to skip; every element written, no zero-fill needed) through the scatter workspace gx_ws
 * (dfe_scatter_ws_bytes(B*C*H*W) bytes; may be NULL when gx is);
 * gflow is written once per pixel from fixed-order partial sums.  Both are bitwise reproducible.
 * Memory contract: the forward reads x and flow and writes every element of out; the backward reads x, flow and gout and writes
 * every element of the gradients requested, and gx_ws, whose contents are undefined on entry and on return (the library
 * initialises what it uses).  gx_ws must be 16-byte aligned (DFE_ERR_DIMS otherwise); every other pointer needs dword alignment only.
 * Where the gradient is gathered (C >= 8 and 512 <= H*W < 2^28) the lists of the gather are laid out inside the
 * dfe_scatter_ws_bytes(B*C*H*W) bytes, which hold them because C >= 8.  The gather and the scatter
 * (forced by DFE_WARP_SCATTER in the environment, read at every call) return the same bits. */
int dfe_warp_flow_fwd(const float* x, const float* flow, float* out, int B, int C, int H, int W, int use_mask,
                      int align_corners, void* stream);
int dfe_warp_flow_bwd(const float* x, const float* flow, const float* gout, float* gflow, float* gx, void* gx_ws, int B,
                      int C, int H, int W, int use_mask, int align_corners, void* stream);

/* ---- inverse_warp2(img, depth, ref_depth, pose, intrinsics)  inverse_warp.py:263-303 -------
 * cams from dfe_prepare_cameras(pose[B,6], K, cams, B, 1, 1, {1}).  Outputs: projected image
 * [B,3,H,W], valid mask [B,1,H,W], projected depth [B,1,H,W], computed depth [B,1,H,W]
 * (the last three may be NULL).  Backward: g_depth [B,1,H,W], g_refdepth [B,1,H,W]
 * (NULL to skip; every element written, through the scatter workspace g_refdepth_ws of
 * dfe_scatter_ws_bytes(B*H*W) bytes), g_pose [B,6]; partials: workspace of
 * dfe_pose_partials_floats(B,H,W) floats.
 * Memory contract: the forward reads img, depth, cams (B blocks) and, when out_pdepth is given, ref_depth, and writes every
 * element of out_img and of each optional output given; the 2x2 footprint is fetched as two dword-aligned 8-byte loads clamped
 * into the plane.  The backward reads the same inputs and the cotangents given (g_pdepth and g_cdepth may be NULL) and
 * writes every element of g_depth, g_pose, of g_refdepth when given (which needs g_pdepth and g_refdepth_ws) and of partials:
 * B * ceil(H*W / 256) rows of 12 floats, one per 256-pixel block, added per sample in block order in double -- bitwise
 * reproducible, as is the fixed-point scatter behind g_refdepth.  partials and g_refdepth_ws need no initialisation; the library
 * writes inside dfe_pose_partials_floats / dfe_scatter_ws_bytes(B*H*W) only.  g_refdepth_ws on 16 bytes; every other pointer
 * needs dword alignment only, and the result does not depend on it.  H < 2 or W < 2 is DFE_ERR_DIMS; every refusal comes
 * before the first launch and leaves all outputs untouched. */
int dfe_pose_partials_floats(int B, int H, int W);
int dfe_inverse_warp2_fwd(const float* img, const float* depth, const float* ref_depth, const float* cams,
                          float* out_img, float* out_valid, float* out_pdepth, float* out_cdepth, int B, int H, int W,
                          int align_corners, void* stream);
int dfe_inverse_warp2_bwd(const float* img, const float* depth, const float* ref_depth, const float* cams,
                          const float* g_img, const float* g_pdepth, const float* g_cdepth, float* g_depth,
                          float* g_refdepth, void* g_refdepth_ws, float* g_pose, float* partials, int B, int H, int W,
                          int align_corners, void* stream);

/* ---- calculate_rigid_flow(depth, pose, intrinsics)  inverse_warp.py:311-342 ----------------
 * Memory contract: the forward reads depth [B,1,H,W] and cams (B blocks) and writes every element of out [B,2,H,W]; the
 * backward reads depth, cams and gout [B,2,H,W] and writes every element of g_depth [B,1,H,W], g_pose [B,6] and partials
 * (dfe_pose_partials_floats(B,H,W) floats, no initialisation needed, summed as in dfe_inverse_warp2_bwd).  Nothing else is
 * touched; every pointer needs dword alignment only; H = W = 1 is accepted.  Refusals come before the first launch. */
int dfe_rigid_flow_fwd(const float* depth, const float* cams, float* out, int B, int H, int W, void* stream);
int dfe_rigid_flow_bwd(const float* depth, const float* cams, const float* gout, float* g_depth, float* g_pose,
                       float* partials, int B, int H, int W, void* stream);

/* ---- mask decisions of the per-method API -----------------------------------------------------
 * compute_occ_weight (model_geometry.py:105-132): from_l/tgt/from_r [B,3,H,W] (masked flow warps and the
 *   target level) -> occ_bwd/occ_fwd = (1 - softmax([dl, dr]) > 0.48), valid_bwd/valid_fwd = 1 - prod_c(warp == 0),
 *   all [B,1,H,W] in {0,1};
 * compute_texture_mask (model_geometry.py:134-140): (mean_c|img - warped| < mean_c|img - source|) -> [B,1,H,W];
 * compute_dynamic_mask (model_geometry.py:699-711): flow, rigid [B,2,H,W] -> mask = (n(|rigid-flow|)^2 <
 *   alpha (n(flow)^2 + n(rigid)^2) + beta), score = 1 / (1e-4 + n(|rigid-flow|)) (score may be NULL).
 * Same device arithmetic as the fused stack: masks are bit-identical to dfe_geom_loss_fwd's mask pack.
 * Memory contract: each entry point reads its two or three dense inputs and writes every element of each output ([B,1,H,W];
 * all four of dfe_occ_masks are required, score may be NULL), one thread per pixel, nothing else; no scratch; every pointer
 * needs dword alignment only.  B > 65535 is DFE_ERR_DIMS; refusals come before the launch and write nothing. */
int dfe_occ_masks(const float* from_l, const float* tgt, const float* from_r, float* occ_bwd, float* occ_fwd,
                  float* valid_bwd, float* valid_fwd, int B, int H, int W, void* stream);
int dfe_texture_mask(const float* img, const float* warped, const float* source, float* out, int B, int H, int W,
                     void* stream);
int dfe_dynamic_mask(const float* flow, const float* rigid, float* mask, float* score, float alpha, float beta, int B,
                     int H, int W, void* stream);

/* ---- device-side input pipeline  core/dataset/kitti_prepared.py:63-90,132-152, train.py:171 ------------------
 * in_u8: uint8 [B][3*H0][W0][3] raw stacked triplets (left / target / right along H, channel order as stored);
 * flip: B device bytes (non-zero = horizontal flip of that sample, NULL = none); out: fp32 [B][3][3*H][W] in [0,1]:
 * per frame bilinear resize (half-pixel centres, edge replication) to H x W, flip, / 255, HWC -> CHW.
 * Memory contract: reads in_u8 (B*3*H0*W0*3 bytes) and, when given, the B bytes of flip, byte by byte -- neither needs any
 * alignment -- and writes every element of out (dword alignment), nothing else; no scratch.  The source coordinate is fp32:
 * at W0 = 300 it carries ~300 * 2^-24 of a pixel, which is the accuracy of the result.  Refusals write nothing. */
int dfe_prepare_triplets(const unsigned char* in_u8, const unsigned char* flip, float* out, int B, int H0, int W0,
                         int H, int W, void* stream);

/* ---- the same image half in the reference's own 8-bit arithmetic  core/dataset/kitti_prepared.py:63-90,132-152 -----
 * cv2.imread (BGR) -> per frame cv2.resize(frame, (W, H)) (INTER_LINEAR on uint8) -> cv2.flip(img, 1) -> / 255.0, for a
 * batch whose samples each have their own raw size.  OpenCV 4.1.1 modules/imgproc/src/resize.cpp, restated: cv::resize
 * (same size: copy), cv::hal::resize (exact 1/2 on both axes: INTER_AREA), resizeGeneric_ with HResizeLinear (11-bit
 * fixed-point coefficients saturate_cast<short>((1 - fx) * 2048), saturate_cast<short>(fx * 2048)), VResizeLinear with
 * FixedPtCast<int, uchar, 22> (scalar rule) and VResizeLinearVec_32s8u (vector rule), resizeAreaFast_.  The host
 * (ops.prepare_triplets_u8) builds the per-size tables; this entry point is integer-only up to the final table lookup.
 *   in_u8 : sample b is uint8 [3*h0][w0][3] (frames stacked along H) at byte desc[b].offset
 *   desc  : B descriptors (below); flip = cv2.flip(img, 1) of the resized strip
 *   xtab  : int pairs (x0, a0 | a1 << 16), W per size, sample b's at pair index desc[b].xtab
 *   ytab  : int quads (y0, y1, b0 | b1 << 16, 0), H per size (rows already clamped), at quad index desc[b].ytab
 *   lut   : 256 floats, lut[u] = float32(u / 255.0) computed in double
 *   out   : fp32 [B][3][3*H][W] (channels B, G, R)
 *   nvec  : bytes of each resized row (3*W of them) that take the vector rule; the rest take the scalar rule
 *   rgb   : non-zero when in_u8 holds R, G, B (a PIL decode): written in cv2.imread's B, G, R order
 * All pointers are device pointers. */
typedef struct {
  long long offset;   /* byte offset of the sample's strip in in_u8 */
  int h0, w0;         /* frame size: the strip is 3*h0 rows of w0 pixels */
  int xtab, ytab;     /* first pair / quad of this size's tables */
  int flip, pad;
} dfe_u8_desc;
int dfe_prepare_triplets_u8(const unsigned char* in_u8, const dfe_u8_desc* desc, const int* xtab, const int* ytab,
                            const float* lut, float* out, int B, int H, int W, int nvec, int rgb, void* stream);

/* ---- a training set resident in device memory: the resized 8-bit frames kept, a batch gathered in one launch -------
 * The image half above is deterministic per frame up to the resized byte; only the flip, the / 255 and the choice of sample
 * vary per step.  dfe_resize_strips_u8 keeps the bytes (once per frame); dfe_gather_triplets_u8 makes a batch from them.
 *
 * dfe_resize_strips_u8: in_u8, desc (every flip must be 0), xtab, ytab, nvec, rgb as for dfe_prepare_triplets_u8, from the same
 * device code (csrc/ops_input.hip: resized_bgr_u8), so store holds exactly the bytes u whose lut[u] that entry point writes.
 *   slot  : long long [B][3], the destination frame of (sample b, frame f) in store; -1 = do not write (stored already)
 *   store : uint8 [F][3 (B,G,R)][H][W]
 * Memory contract: reads what dfe_prepare_triplets_u8 reads, plus the 3B values of slot; writes exactly the 3*H*W bytes of
 * each slot >= 0 and nothing else (a value >= F writes nothing either: the kernel predicates on it; the host wrapper refuses
 * it); byte accesses, no alignment needed beyond slot's 8 and the tables'; no scratch.  F <= 0, B, H, W <= 0 or nvec outside
 * [0, 3W] is DFE_ERR_DIMS before the launch, with nothing written.
 *
 * dfe_gather_triplets_u8: one batch in one launch (B > 64: one launch per 64 samples).
 *   store : as above, F frames               tri  : int [N][3], the frame slots of triplet i (left / target / right)
 *   ktab  : fp32 [N][2][S][3][3], K_ms then K_inv_ms of triplet i            lut : the 256 floats above
 *   idx_host  : HOST pointer, int [B], the triplet of each sample            (these two are the only host pointers of this
 *   flip_host : HOST pointer, B bytes, non-zero = flipped; NULL = none        file's image entry points: they are read during
 *                                                                             the call and travel in the kernel's arguments)
 *   out : fp32 [B][3][3*H][W];  K_ms, K_inv_ms : fp32 [B][S][3][3]
 * Result: out[b][c][f*H + y][x] = lut[store[tri[idx[b]][f]][c][y][flip[b] ? W-1-x : x]], K_ms[b] = ktab[idx[b]][0],
 * K_inv_ms[b] = ktab[idx[b]][1].  No pinned staging buffer and no copy: nothing for the stream to wait on but the kernel.
 * Memory contract: reads tri and ktab at the rows idx names, lut, and the 3*H*W bytes of each named frame whose slot lies in
 * [0, F) -- a slot outside is never dereferenced (its rows are written as lut[0]); writes every element of out, K_ms and
 * K_inv_ms and nothing else; no scratch.  With W % 16 == 0 and store, out on 16 bytes a lane moves 16 bytes per load and store;
 * otherwise (any W, dword-aligned out, store unaligned) one element per lane, the same bits.  A NULL pointer (flip_host
 * excepted) is DFE_ERR_NULL; F, N, B, S, H, W <= 0, S > DFE_MAX_SCALES, 9*H*W >= 2^25 or an idx_host[b] outside [0, N) is
 * DFE_ERR_DIMS, checked on the host before the first launch, with nothing written. */
int dfe_resize_strips_u8(const unsigned char* in_u8, const dfe_u8_desc* desc, const int* xtab, const int* ytab,
                         const long long* slot, unsigned char* store, long F, int B, int H, int W, int nvec, int rgb,
                         void* stream);
int dfe_gather_triplets_u8(const unsigned char* store, long F, const int* tri, const float* ktab, int N, const float* lut,
                           const int* idx_host, const unsigned char* flip_host, float* out, float* K_ms, float* K_inv_ms,
                           int B, int S, int H, int W, void* stream);

/* ---- forward-splat occlusion map  core/networks/model_flow.py:33-39 (get_occlusion_mask_from_flow) -----------
 * The reference calls an undefined `transformerFwd`; this is its TrianFlow meaning: out [B,1,H,W] = bilinear forward
 * warp of a ones image by flow [B,2,H,W] (optionally clamped to [0,1]).  Order-independent scatter through ws
 * (dfe_scatter_ws_bytes(B*H*W) bytes); every element of out is written; bitwise reproducible.
 * Memory contract: reads flow, writes every element of out and, inside dfe_scatter_ws_bytes(B*H*W) bytes only, ws, which needs
 * no initialisation and holds nothing of use afterwards.  ws on 16 bytes; flow and out need dword alignment only.  A source
 * pixel whose target is NaN or not inside (-1, W) x (-1, H) deposits nothing; a tap outside the image is dropped, the others of
 * that pixel are kept.  Each weight is one fp32 product rounded to a grid of 2^-35.  clamp01 clamps the finished map in place. */
int dfe_forward_splat_ones(const float* flow, float* out, void* ws, int B, int H, int W, int clamp01, void* stream);

/* ---- self-test of the short correctly rounded fp32 sequences (csrc/loss_stack_exact.h) ------------------------
 * The mask-deciding expressions of the reference use IEEE division and square root (torch CPU); the pointwise kernels
 * evaluate them with 3 / 5-instruction sequences that must return the SAME bits.  This entry point checks that
 * exhaustively on the device: counts (4 device uint64) receive the numbers of mismatches of
 *   [0] RN(1/z) over every fp32 z whose reciprocal is normal, [1] sqrt over every non-negative finite fp32,
 *   [2] x/z over `npairs` pseudo-random pairs, [3] the same with all-ones divisor significands.  All must be 0. */
int dfe_exact_math_selftest(unsigned long long* counts, unsigned long long npairs, void* stream);

/* ---- SSIM(x, y)  pytorch_ssim/ssim.py:4-19 --------------------------------------------------
 * Memory contract: the forward reads x, y [B,C,H,W] and writes every element of out; the backward reads x, y and gout and writes
 * every element of whichever of gx / gy is given (not both NULL; one alone returns the bits of the pair).  Tiles of 32 x 8 with a
 * zero-padded halo staged in LDS: nothing outside the planes is read.  No scratch; dword alignment only.  B*C > 65535 (a grid
 * dimension) is DFE_ERR_DIMS, before the launch, with nothing written. */
int dfe_ssim_fwd(const float* x, const float* y, float* out, int B, int C, int H, int W, void* stream);
int dfe_ssim_bwd(const float* x, const float* y, const float* gout, float* gx, float* gy, int B, int C, int H, int W,
                 void* stream);

/* ---- PWC_tf.corr_naive(input1, input2, d=4)  pwc_tf.py:97-106 ------------------------------
 * out [B,(2d+1)^2,H,W]; only d == 4 is implemented (DFE_ERR_UNSUPPORTED otherwise).
 * Memory contract: the forward reads f1, f2 [B,C,H,W] and writes every element of out, nothing else; the backward reads f1, f2
 * and gout [B,81,H,W] and writes every element of g1 and / or g2 [B,C,H,W] (either may be NULL, not both), nothing else.  No
 * scratch, no initialisation of an output.  Every pointer needs dword alignment only: with W % 4 == 0 and every pointer on 16
 * bytes the kernels use 16-byte accesses, otherwise dword ones, and both return the same bits. */
int dfe_corr_fwd(const float* f1, const float* f2, float* out, int B, int C, int H, int W, int d, void* stream);
int dfe_corr_bwd(const float* f1, const float* f2, const float* gout, float* g1, float* g2, int B, int C, int H, int W,
                 int d, void* stream);
/* The launch plan the two entry points above (and the PWC level below) pick for a shape: host only, nothing is launched and no
 * device is needed; the tuning overrides of the environment are honoured as the launchers honour them.  `vec`: non-zero when
 * every pointer and batch stride of the call is 16-byte aligned; `sides`: gradients requested (1 or 2).  DFE_ERR_UNSUPPORTED
 * where the launcher would refuse the shape.
 *   forward, 12 ints: tile rows TH, tile quads TXQ, tiles across ntx, channel split KS, channels per chunk CC, displacement
 *     rows per block DYG, staged f2 quads per thread PF2, threads, bytes of LDS, chunks, coarse (0 / 1), 16-byte kernel (0 / 1);
 *   backward, 10 ints: TH, TXQ, ntx, channel groups per block NCG, channel ranges ncr, displacement-row split IS, threads,
 *     bytes of LDS, staging batches, 16-byte kernel (0 / 1). */
int dfe_corr_fwd_plan(int B, int C, int H, int W, int vec, int* plan);
int dfe_corr_bwd_plan(int B, int C, int H, int W, int sides, int vec, int* plan);

/* ---- ResNet stem max pooling  nn.MaxPool2d(3, 2, 1) of torchvision's resnet as ResnetEncoder runs it
 * (core/networks/structures/depth_model.py:60-95).  x [planes,H,W] -> y [planes,Ho,Wo], Ho = (H-1)/2+1; `idx` keeps the
 * winning window position (0..8, row-major) as one byte per output.  Values, tie-breaking (first maximum in window
 * scan order, NaN wins) and the gradient's accumulation order are ATen's: bit-identical to F.max_pool2d. */
int dfe_maxpool3x3s2_out(int n);
int dfe_maxpool3x3s2_fwd(const float* x, float* y, unsigned char* idx, int planes, int H, int W, void* stream);
int dfe_maxpool3x3s2_bwd(const float* gy, const unsigned char* idx, float* gx, int planes, int H, int W, void* stream);

/* ---- one PWC decoder level's input  pwc_tf.py:119-121 (and :131-133, :143-145, :155-157) --------
 *   warp = self.warp(c2, up_flow); corr = self.corr(c1, warp); x = torch.cat((corr, c1, up_flow), 1)
 * as ONE operator: the cost volume is written straight into planes [0,81) of x [B, 81+C+2, H, W] (caller-allocated),
 * c1 and the flow are copied behind it; `warped` [B,C,H,W] is kept for the backward pass.  The backward pass reads
 * the three channel slices of gx = dL/dx in place and returns complete gradients:
 *   g_c1 = dcorr/dc1 + gx[:,81:81+C];  g_flow = dwarp/dflow + gx[:,81+C:];  g_c2 (order-independent scatter through
 *   g_c2_ws, dfe_scatter_ws_bytes(B*C*H*W) bytes; every element of g_c2 is written).
 * g_warped [B,C,H,W] is scratch.  g_c2 (with g_c2_ws) or g_flow may be NULL (not both).
 * Memory contract: the forward reads c1, c2, flow and writes every element of warped [B,C,H,W] and of x (dense), nothing else;
 * planes [81,81+C) and [81+C,81+C+2) of x are bit copies of c1 and flow.  The backward reads c1, c2, flow, warped and gx (dense,
 * [B,81+C+2,H,W]) and writes every element of g_warped (dL/dwarped: scratch that needs no initialisation), g_c1 and of whichever
 * of g_c2 / g_flow is given.  g_c2_ws (dfe_scatter_ws_bytes(B*C*H*W) bytes) and map (dfe_pwc_level_map_bytes bytes) need no
 * initialisation; the library writes inside those sizes only.  16 bytes are required of map and of g_c2_ws (DFE_ERR_DIMS otherwise: the
 * gather, taken where C >= 8 and 512 <= H*W < 2^28, lays its lists out inside g_c2_ws).  Every other pointer needs dword
 * alignment only.  The forward uses 16-byte accesses when W % 4 == 0 and c1, warped, x and flow are all on 16 bytes; the backward
 * when W % 4 == 0 and c1, warped, gx, g_warped and g_c1 are.  Otherwise both use dword accesses, with the same bits either way.
 * Gather, scatter (DFE_WARP_SCATTER in the environment), the map built in one launch (H*W <= 1024) or in three
 * (DFE_WFG_MAP_LARGE in the environment) and the plain / _map pairs all return the same bits; both switches are read at every
 * call. */
int dfe_pwc_level_channels(int C);   /* 81 + C + 2 */
int dfe_pwc_level_fwd(const float* c1, const float* c2, const float* flow, float* warped, float* x, int B, int C, int H,
                      int W, int align_corners, void* stream);
int dfe_pwc_level_bwd(const float* c1, const float* c2, const float* flow, const float* warped, const float* gx,
                      float* g_warped, float* g_c1, float* g_c2, void* g_c2_ws, float* g_flow, int B, int C, int H,
                      int W, int align_corners, void* stream);
/* The same operator with the backward's inverse map built in the FORWARD pass (ABI 3; C >= 8): `map` (dfe_pwc_level_map_bytes
 * bytes, 16-byte aligned, caller-allocated, contents undefined on entry) receives, per pixel of c2, the list of (source pixel,
 * bilinear weight) taps of warp(c2, flow) that read it -- the feature warp counts them while it samples -- and must reach
 * dfe_pwc_level_bwd_map unchanged.  That backward is three launches at every level (correlation gradients, flow gradient, gather)
 * and returns the bits dfe_pwc_level_bwd returns.  DFE_ERR_UNSUPPORTED for C < 8 (use the pair above). */
long dfe_pwc_level_map_bytes(int B, int H, int W);
int dfe_pwc_level_fwd_map(const float* c1, const float* c2, const float* flow, float* warped, float* x, void* map, int B, int C,
                          int H, int W, int align_corners, void* stream);
int dfe_pwc_level_bwd_map(const float* c1, const float* c2, const float* flow, const float* warped, const float* gx,
                          float* g_warped, float* g_c1, float* g_c2, void* map, float* g_flow, int B, int C, int H, int W,
                          int align_corners, void* stream);

/* ---- pyramids: mode 0 = F.interpolate(bilinear, align_corners=False) (model_geometry.py:65-72),
 * mode 1 = F.interpolate(area) == adaptive_avg_pool2d (model_geometry.py:91, model_flow.py:58-64). */
int dfe_resize(const float* in, float* out, int planes, int inH, int inW, int outH, int outW, int mode, void* stream);
/* Differentiable bilinear resize with the scalar PWC_tf puts on either side of F.interpolate (pwc_tf.py:118-119:
 * `F.interpolate(flow6, scale_factor=2.0, mode='bilinear') * 2.0`; :175-178: `F.interpolate(flow2 * 4.0, [h, w])`):
 * pre_scale = 1: out = resize(in * mult); 0: out = resize(in) * mult -- each rounded like the ATen (CPU) composition.
 * The backward pass is the adjoint as a gather per input element (no atomics, unlike ATen's upsample backward);
 * DFE_ERR_UNSUPPORTED when the up-sampling ratio exceeds 4 per axis.
 * Memory contract (dfe_resize and the pair below): `in` [planes,inH,inW] is read, every element of `out` [planes,outH,outW]
 * written (the backward: gout read, every element of gin [planes,inH,inW] written), one thread per written element, nothing else;
 * no scratch; dword alignment only, and the result does not depend on it.  Mode 0 and dfe_resize_bilinear_fwd return ATen's
 * (CPU) bits on both sides of its kernel switch at outH + outW = 128.  The backward's refusal (2 out > 8 in on an axis: the
 * 12 candidates per axis of its register path) comes before the launch and leaves gin untouched; the forward has no such limit. */
int dfe_resize_bilinear_fwd(const float* in, float* out, int planes, int inH, int inW, int outH, int outW, float mult,
                            int pre_scale, void* stream);
int dfe_resize_bilinear_bwd(const float* gout, float* gin, int planes, int inH, int inW, int outH, int outW, float mult,
                            int pre_scale, void* stream);

/* ---- depth-decoder glue between the MIOpen convolutions (depth_model.py:60-211:
 * Conv3x3 = ReflectionPad2d(1) + conv, ConvBlock = Conv3x3 + ELU, stage = ConvBlock, bilinear x2, cat(skip), ConvBlock).
 * The convolutions are called without their bias; x is such an output and ``bias`` [C] (or NULL) is added on read.
 * dfe_elu_pad:          out [B,C,H+2,W+2] = reflect_pad1(apply_elu ? elu(x + bias) : x + bias),  x [B,C,H,W]
 * dfe_elu_up2_cat_pad:  out [B,C1+C2,2h+2,2w+2] = reflect_pad1(cat(bilinear_x2(elu(x + bias)), skip)),
 *                       x [B,C1,h,w], skip [B,C2,2h,2w] or NULL with C2 = 0.
 * Backward: gout has the padded shape; gx = gradient wrt x (= wrt x + bias); gbias [C] (or NULL) = its sum over
 * (b,h,w), which needs ``partials`` = dfe_glue_partials_floats(B,C,H,W) floats of scratch (H,W of x);
 * gskip may be NULL (ignored when C2 = 0). */
long dfe_glue_partials_floats(int B, int C, int H, int W);
int dfe_elu_pad_fwd(const float* x, const float* bias, float* out, int B, int C, int H, int W, int apply_elu, void* stream);
int dfe_elu_pad_bwd(const float* x, const float* bias, const float* gout, float* gx, float* gbias, float* partials,
                    int B, int C, int H, int W, int apply_elu, void* stream);
int dfe_elu_up2_cat_pad_fwd(const float* x, const float* bias, const float* skip, float* out, int B, int C1, int C2,
                            int h, int w, void* stream);
int dfe_elu_up2_cat_pad_bwd(const float* x, const float* bias, const float* gout, float* gx, float* gskip, float* gbias,
                            float* partials, int B, int C1, int C2, int h, int w, void* stream);

/* ---- disparity head of the depth decoder (depth_model.py: dispconv = Conv3x3(C -> 1) + Sigmoid per output scale):
 * out [B,1,H,W] = sigmoid(conv3x3(p) + bias[0]) on the reflection-padded activation p [B,C,H+2,W+2], weight [1,C,3,3];
 * C must be a multiple of 16 (DFE_ERR_UNSUPPORTED otherwise).  Backward: gp [B,C,H+2,W+2] (every element written),
 * gweight [C*9] / gbias [1] (may both be NULL); partials: dfe_disp_head_partials_floats floats of scratch. */
long dfe_disp_head_partials_floats(int B, int C, int H, int W);
int dfe_disp_head_fwd(const float* p, const float* weight, const float* bias, float* out, int B, int C, int H, int W,
                      void* stream);
int dfe_disp_head_bwd(const float* p, const float* weight, const float* out, const float* gout, float* gp, float* gweight,
                      float* gbias, float* partials, int B, int C, int H, int W, void* stream);

/* ---- flow head  pwc_tf.py:39-40  predict_flow = Conv2d(C, 2, kernel_size=3, stride=1, padding=1, bias=True) ----------
 * The same rolling-window kernels with two output channels on the unpadded activation x [B,C,H,W] (zero padding is
 * virtual): out [B,2,H,W] = conv3x3(x, weight [2,C,3,3]) + bias [2].  MIOpen has no matrix to feed with two output
 * channels (4-5 TFLOP/s: 69 / 26 / 99 us forward / data / weight gradient at C = 96, 64x208, 8 images).
 * Backward: gx [B,C,H,W] (every element written), gweight [2*C*9] / gbias [2] (may both be NULL), fixed-order sums;
 * partials: dfe_flow_head_partials_floats floats of scratch.  C must be a multiple of 8 (DFE_ERR_UNSUPPORTED otherwise). */
long dfe_flow_head_partials_floats(int B, int C, int H, int W);
int dfe_flow_head_fwd(const float* x, const float* weight, const float* bias, float* out, int B, int C, int H, int W,
                      void* stream);
int dfe_flow_head_bwd(const float* x, const float* weight, const float* gout, float* gx, float* gweight, float* gbias,
                      float* partials, int B, int C, int H, int W, void* stream);

/* ---- weight gradient of the thin, wide 3x3 convolutions of the depth decoder on pre-padded inputs (fp32 MFMA):
 * gweight [Co,Ci,3,3] = sum_{b,y,x} gy[b,co,y,x] * p[b,ci,y+ky,x+kx],  p [B,Ci,H+2,W+2], gy [B,Co,H,W].
 * Requires Ci % 16 == 0, Co % 16 == 0, W % 16 == 0, p 8-byte and gy 16-byte aligned (DFE_ERR_UNSUPPORTED otherwise: the
 * caller then keeps MIOpen's weight gradient).  partials: dfe_wgrad3x3_partials_floats floats of scratch. */
long dfe_wgrad3x3_partials_floats(int B, int Ci, int Co, int H, int W);
int dfe_wgrad3x3_fwd(const float* p, const float* gy, float* gweight, float* partials, int B, int Ci, int Co, int H, int W,
                     void* stream);

/* ---- 3x3 / stride 1 / pad 1 convolutions on small planes (H*W <= 4096 per sample) on the fp32 matrix cores: PWC's decoder
 * levels 6 and 5 (pwc_tf.py:28-47 conv6_0 .. conv5_4 = Conv2d(3x3, pad 1, bias) + LeakyReLU(0.1), called at
 * pwc_tf.py:113-135), where MIOpen's kernels are launch- and layout-bound (10-45 us forward, 26-126 us per weight gradient
 * for 0.1-0.4 GFLOP).  x [B,Ci,H,W], weight [Co,Ci,3,3], all fp32 NCHW contiguous.
 * dfe_planeconv_fwd:   y = act(conv(x, weight) + bias[co]) (bias may be NULL; act(v) = v > 0 ? v : slope * v, slope 1 = none)
 *                      written to dst1 and (optional) dst2: element (b,co,i) at dst + b * batch_stride + co*H*W + i, so the
 *                      output lands in the channel slices of the concatenated buffers that consume it.
 * dfe_planeconv_dgrad: gx [B,Ci,H,W] = the data gradient of conv(x, weight) for the output gradient gy [B,Co,H,W].
 * dfe_planeconv_wgrad: gweight [Co,Ci,3,3] = the weight gradient.
 * ws: dfe_planeconv_ws_floats floats of scratch (partial sums of the split reductions; every sum is added in a fixed order:
 * results are reproducible).  DFE_ERR_UNSUPPORTED (dfe_planeconv_supported == 0) for larger planes: the caller keeps MIOpen.
 * Memory: every pointer needs dword alignment only; ws needs no initialisation; only the B samples of Co*H*W floats of dst1 /
 * dst2 are written (batch strides below that: DFE_ERR_DIMS). */
int dfe_planeconv_supported(int B, int Ci, int Co, int H, int W);
long dfe_planeconv_ws_floats(int B, int Ci, int Co, int H, int W);
int dfe_planeconv_fwd(const float* x, const float* weight, const float* bias, float slope, float* dst1, long dst1_batch_stride,
                      float* dst2, long dst2_batch_stride, float* ws, int B, int Ci, int Co, int H, int W, void* stream);
int dfe_planeconv_dgrad(const float* gy, const float* weight, float* gx, float* ws, int B, int Ci, int Co, int H, int W,
                        void* stream);
int dfe_planeconv_wgrad(const float* gy, const float* x, float* gweight, float* ws, int B, int Ci, int Co, int H, int W,
                        void* stream);

/* ---- 3x3 / stride 1 convolutions of the networks' large layers as Winograd F(2x2, 3x3) on the fp32 matrix cores, one fused
 * kernel (depth_model.py:60-211 ResNet encoder / decoder, pwc_tf.py:28-95 decoder and context network, feature_pyramid.py:7-36;
 * MIOpen runs the same algorithm on the vector ALU).  x [B,Ci,H,W]; y [B,Co,Ho,Wo], Ho = H + 2P - 2, Wo = W + 2P - 2, P = 1
 * (zero padding), 0 (valid) or 2 (full: the data gradient of a valid convolution); element (b,co,i) of y at
 * y + b * y_batch_stride + co * Ho*Wo + i.
 * transposed_weight = 0: weight [Co,Ci,3,3], y = conv(x, weight) (no bias).
 * transposed_weight = 1: weight [Ci,Co,3,3] is the FORWARD filter of a convolution whose output gradient is x: y is its data
 *                        gradient, i.e. conv(x, w') with w'[co][ci][ky][kx] = weight[ci][co][2-ky][2-kx] (P = 1 for a forward
 *                        P = 1, P = 2 for a forward P = 0).
 * wbuf: scratch, 16-byte aligned, wbuf_floats floats: at least dfe_wino_weight_floats(Ci, Co) (the transformed filters);
 * with dfe_wino_scratch_floats(B, Ci, Co, H, W, P) the planes that cannot fill the chip (few tiles, many channels) split their
 * input channels over several blocks whose partial outputs are added in a fixed order.
 * DFE_ERR_DIMS when B*Ci*H*W >= 2^30 (32-bit offsets).
 * Memory: x, weight, bias, y and y2 need dword alignment only; x 8-byte aligned with W even selects the pair loads, y (y2)
 * 8-byte aligned with an even batch stride and Wo even the 8-byte stores -- the same bits either way.  wbuf / U / part must be
 * 16-byte aligned (DFE_ERR_UNSUPPORTED otherwise) and need no initialisation.  Reads stay inside x [B*Ci*H*W], weight, bias
 * [Co] and U; writes inside the B samples of Co*Ho*Wo floats of y / y2 (the gaps of a larger batch stride are not touched)
 * and the stated floats of the scratch. */
long dfe_wino_weight_floats(int Ci, int Co);
long dfe_wino_scratch_floats(int B, int Ci, int Co, int H, int W, int P);
int dfe_wino_conv3x3(const float* x, const float* weight, float* y, long y_batch_stride, float* wbuf, long wbuf_floats, int B, int Ci,
                     int Co, int H, int W, int P, int transposed_weight, void* stream);
/* weight gradient of the same convolutions in the Winograd domain (replaces aten::convolution_backward's weight output for the
 * reference's 3x3 stride-1 layers, depth_model.py:13-58,135-191, pwc_tf.py:28-95): gweight [Co,Ci,3,3] = d/dw of
 * conv(x [B,Ci,H,W], w, padding P in {0, 1}) for the output gradient gy; element (b,ci,i) of x at x + b * x_batch_stride +
 * ci * H*W + i, element (b,co,i) of gy at gy + b * gy_batch_stride + co * Ho*Wo + i.  Straight from NCHW: no layout
 * transposes, no zero fill, no atomics (fixed-order partial sums in ws: dfe_wino_wgrad_floats floats); any size and
 * channel count.  A dilated layer (pwc_tf.py:31-36) is this call on its dilation x dilation phase images (B d^2 samples of
 * H/d x W/d pixels, P = 1), which the caller gathers.
 * Memory: x and gy need dword alignment only (any float offset, any batch stride >= the dense sample size) and may be views of
 * any size, down to a single float: nothing outside the B samples of Ci*H*W / Co*Ho*Wo floats is read (the staging loads' safe
 * address is the workspace).  gweight and ws need dword alignment; ws needs no initialisation and nothing outside
 * dfe_wino_wgrad_floats floats of it is touched. */
long dfe_wino_wgrad_floats(int B, int Ci, int Co, int H, int W, int P);
/* tuning hook (process-wide, not for concurrent use): tile = 0 (by shape) / 11 / 12 / 21 forces the wave tile (16 MH x 16 NH
 * channels); blocks1 / blocks2 > 0: the grid-size targets of the 64- / 128-accumulator kernels; chunk = 8 / 12 tiles per
 * barrier (0: keep).  The workspace size follows the setting: query dfe_wino_wgrad_floats after changing it. */
int dfe_wino_wgrad_tune(int tile, int blocks1, int blocks2, int chunk);
int dfe_wino_wgrad3x3(const float* x, long x_batch_stride, const float* gy, long gy_batch_stride, float* gweight, float* ws, int B,
                      int Ci, int Co, int H, int W, int P, void* stream);
/* Weight gradient of a STRIDED convolution straight from NCHW on the fp32 matrix cores (csrc/ops_sconv.hip; replaces MIOpen's
 * transposed NHWC calls for nn.Conv2d(..., stride=2): depth_model.py:60-95 ResNet stem, feature_pyramid.py:7-36, pose_cnn.py:14-36).
 * x [B,Ci,H,W], gy [B,Co,Ho,Wo] (Ho = (H + 2P - K) / stride + 1), both with a batch stride in floats; K x K filters, K <= 7.
 * dfe_sconv_wgrad: gweight [Co,Ci,K,K] = the weight gradient; ws holds dfe_sconv_wgrad_floats(...) floats of split partials,
 * added in split order (no atomics: bit-reproducible).  0 floats / DFE_ERR_UNSUPPORTED: a shape outside the kernel family
 * (3x3 with Ci >= 16; Ci K K <= 160; Ci K K <= 448 with Co <= 32).  dfe_sconv_tune: blocks >= 0 the grid-size target (0: two or
 * three resident blocks per CU, by kernel); rows >= 0 caps the output rows per chunk (0: no cap); negative: keep.
 * Memory: as dfe_wino_wgrad3x3 (dword-aligned, batch-strided views; ws uninitialised), except that the staging loads' safe
 * address is the first 16 bytes of a sample: a sample of x or gy of fewer than 4 floats (Ci*H*W < 4 or Co*Ho*Wo < 4) is
 * outside the kernel family (0 floats / DFE_ERR_UNSUPPORTED). */
int dfe_sconv_tune(int blocks, int rows);
long dfe_sconv_wgrad_floats(int B, int Ci, int Co, int H, int W, int K, int stride, int P);
int dfe_sconv_wgrad(const float* x, long x_batch_stride, const float* gy, long gy_batch_stride, float* gweight, float* ws, int B,
                    int Ci, int Co, int H, int W, int K, int stride, int P, void* stream);
/* Forward pass and data gradient of the same layers (stride 2, padding K / 2; csrc/ops_sconv.hip), one launch each after a
 * filter re-layout; only the deterministic mode (convs.set_deterministic) routes layers here: every sum has one fixed order,
 * whatever the allocator hands out.  Ho = (H + 2 (K / 2) - K) / 2 + 1, Wo alike.
 * dfe_sconv_fwd:   y [B,Co,Ho,Wo] = act(conv(x [B,Ci,H,W], weight [Co,Ci,K,K]) + bias[co]), K in {3, 5, 7}; bias may be NULL;
 *                  act(v) = v > 0 ? v : slope * v (slope 1: none, 0: ReLU).
 * dfe_sconv_dgrad: gx [B,Ci,H,W] = the data gradient for gy [B,Co,Ho,Wo], K in {1, 3, 5} (K = 1: the 1x1 stride-2 shortcuts;
 *                  the odd rows and columns of gx are written with zeros).  Every element of gx is written.
 * ws: dfe_sconv_fwd_floats / dfe_sconv_dgrad_floats floats (host-only queries): the packed filter and, for layers whose tiles
 * cannot fill the chip, the partial outputs of the channel splits, added in split order.  0 floats / DFE_ERR_UNSUPPORTED: a
 * shape outside the kernel family (another K; a sample of x -- for the data gradient, of gy -- of fewer than 4 floats).
 * Memory: x, gy, weight, bias, y and gx need dword alignment only and may be batch-strided views (any batch stride >= the dense
 * sample, DFE_ERR_DIMS below it); the staging loads' safe address is the first 16 bytes of a sample of x (of gy), hence the
 * 4-float rule.  Reads stay inside the B samples of x / gy, weight and bias [Co]; writes inside the B samples of y / gx (the
 * gaps of a larger batch stride are not touched) and the first *_floats() floats of ws.  ws must be 16-byte aligned
 * (DFE_ERR_UNSUPPORTED otherwise) and needs no initialisation.  Every refusal comes before the first launch. */
long dfe_sconv_fwd_floats(int B, int Ci, int Co, int H, int W, int K);
int dfe_sconv_fwd(const float* x, long x_batch_stride, const float* weight, const float* bias, float slope, float* y,
                  long y_batch_stride, float* ws, int B, int Ci, int Co, int H, int W, int K, void* stream);
long dfe_sconv_dgrad_floats(int B, int Ci, int Co, int H, int W, int K);
int dfe_sconv_dgrad(const float* gy, long gy_batch_stride, const float* weight, float* gx, long gx_batch_stride, float* ws, int B,
                    int Ci, int Co, int H, int W, int K, void* stream);
/* The 1x1 stride-2 convolutions without padding or bias (depth_model.py:31-36, the ResNet down-sampling shortcuts 64 -> 128,
 * 128 -> 256, 256 -> 512; a BatchNorm follows) for the same mode (csrc/ops_conv1x1s2.hip; the data gradient is dfe_sconv_dgrad
 * with K = 1).  x [B,Ci,H,W], weight [Co,Ci] (= [Co,Ci,1,1]), Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1.
 * dfe_conv1x1s2_fwd:   y [B,Co,Ho,Wo] = sum_ci weight[co][ci] x[b][ci][2 oy][2 ox].  No workspace.
 * dfe_conv1x1s2_wgrad: gweight [Co,Ci] = sum over b and the output pixels of gy[b][co][oy][ox] x[b][ci][2 oy][2 ox]; the pixel
 *                      range is split over one resident round of blocks and the partials (ws: dfe_conv1x1s2_wgrad_floats
 *                      floats) are added in split order: no atomics.
 * dfe_conv1x1s2_supported / _wgrad_floats are host-only; 0 / DFE_ERR_UNSUPPORTED: B Ho Wo, a sample or the filter >= 2^30.
 * Memory: every pointer needs dword alignment only; x, y and gy may be batch-strided views of any size (every access is
 * predicated on its own index: nothing outside the B samples of x -- of which only even rows and columns are read -- , gy,
 * weight, the B samples of y, gweight and the stated floats of ws is touched); ws needs no initialisation. */
int dfe_conv1x1s2_supported(int B, int Ci, int Co, int H, int W);
int dfe_conv1x1s2_fwd(const float* x, long x_batch_stride, const float* weight, float* y, long y_batch_stride, int B, int Ci, int Co,
                      int H, int W, void* stream);
long dfe_conv1x1s2_wgrad_floats(int B, int Ci, int Co, int H, int W);
int dfe_conv1x1s2_wgrad(const float* x, long x_batch_stride, const float* gy, long gy_batch_stride, float* gweight, float* ws, int B,
                        int Ci, int Co, int H, int W, void* stream);
/* the same for a DILATED 3x3 convolution with padding = dilation (pwc_tf.py:31-36 context network: dilation 2, 4, 8, 16): the
 * Winograd tiles live on the dilation x dilation phase images; H and W must be multiples of the dilation.  y has x's size. */
int dfe_wino_conv3x3_dilated(const float* x, const float* weight, float* y, long y_batch_stride, float* wbuf, int B, int Ci, int Co,
                             int H, int W, int dilation, int transposed_weight, void* stream);
/* Transformed filters kept across calls (a training step transforms every filter twice -- forward and data gradient -- although
 * it only changes once, in the optimiser step; nn.Conv2d has no such state, depth_model.py:60-211 / pwc_tf.py:28-95):
 * dfe_wino_transform_weights_multi transforms n filters in ONE launch, bit-identically to what dfe_wino_conv3x3 computes for
 * itself.  table (device): 6 longs per filter = {weight pointer, U pointer (dfe_wino_weight_floats(Ci, Co) floats, 16-byte
 * aligned), K, C, transposed_weight, first block}, where (K, C) = (Co, Ci) of the convolution the U is FOR (transposed_weight = 1:
 * weight is [C,K,3,3]); a filter takes dfe_wino_transform_blocks(Ci = C, Co = K) consecutive blocks; blockmap (device): the
 * filter index of each of the n_blocks blocks.
 * dfe_wino_conv3x3_u is dfe_wino_conv3x3 / _dilated (dilation > 1: P is ignored) on such a U; part: part_floats floats of
 * scratch for the channel splits (dfe_wino_scratch_floats - dfe_wino_weight_floats; may be null / 0: no splits). */
long dfe_wino_transform_blocks(int Ci, int Co);
int dfe_wino_transform_weights_multi(const long* table, const int* blockmap, int n_blocks, void* stream);
int dfe_wino_conv3x3_u(const float* x, const float* U, float* y, long y_batch_stride, float* part, long part_floats, int B, int Ci,
                       int Co, int H, int W, int P, int dilation, void* stream);
/* dfe_wino_conv3x3_u with the bias + activation epilogue inside the output transform (net_utils.py:7-11 conv() = Conv2d +
 * LeakyReLU(0.1); pwc_tf.py:113-118): y = act(conv(x) + bias[co]), act(v) = v > 0 ? v : slope * v (slope 1: bias only; bias may
 * be null) -- bit for bit what dfe_bias_act_fwd makes of dfe_wino_conv3x3_u's output -- written to y and, when y2 is not null,
 * to the same (b, co, i) of y2 (batch stride y2_batch_stride): the two concatenated buffers a PWC decoder layer feeds. */
int dfe_wino_conv3x3_u_act(const float* x, const float* U, const float* bias, float slope, float* y, long y_batch_stride, float* y2,
                           long y2_batch_stride, float* part, long part_floats, int B, int Ci, int Co, int H, int W, int P,
                           int dilation, void* stream);

/* ---- 1x1 convolutions on tiny planes (H*W <= 256, B*H*W <= 4096): PoseCNN's pose_conv and refinement head
 * (pose_cnn.py:32,43,48: Conv2d(256 | 24 | 12, 12, 1) on 2x7 planes).  x [B,Ci,H,W], weight [Co,Ci] (= [Co,Ci,1,1]).
 * dfe_conv1x1_small_fwd: y = act(conv1x1(x, weight) + bias[co]) (bias may be NULL; act as in dfe_planeconv_fwd).
 * dfe_conv1x1_small_bwd: gx [B,Ci,H,W] and / or gweight [Co,Ci] (either may be NULL) for the output gradient gy [B,Co,H,W]
 * (of the pre-activation: apply dfe_bias_act_bwd first).  One thread per output, serial sums: reproducible.
 * Memory contract: the forward reads x, weight and bias (when given) and writes every element of y; the backward reads gy,
 * weight (for gx) and x (for gweight) and writes every element of whichever of gx / gweight is given -- each returns the same
 * bits alone or together.  Nothing else is touched; no scratch; every pointer needs dword alignment only and the result does not
 * depend on it.  H*W > 256, B*H*W > 4096 or more than 4096 channels on either side is DFE_ERR_UNSUPPORTED
 * (dfe_conv1x1_small_supported == 0) from both entry points, before any launch, with nothing written. */
int dfe_conv1x1_small_supported(int B, int Ci, int Co, int H, int W);
int dfe_conv1x1_small_fwd(const float* x, const float* weight, const float* bias, float slope, float* y, int B, int Ci, int Co,
                          int H, int W, void* stream);
int dfe_conv1x1_small_bwd(const float* gy, const float* x, const float* weight, float* gx, float* gweight, int B, int Ci, int Co,
                          int H, int W, void* stream);

/* ---- grouped training-mode BatchNorm2d (+ residual + ReLU) of the depth encoder (SURVEY.md 8(f) rank 1;
 * depth_model.py:60-95 = torchvision BasicBlock conv-bn-relu-conv-bn-(+identity)-relu; model_geometry.py:786-788 calls the
 * depth net once per frame).  x [G*Bg,C,H,W] is G groups of Bg consecutive samples: statistics are per (group, channel)
 * and running_mean / running_var (may be NULL) receive the G momentum updates in group order, i.e. what G sequential
 * nn.BatchNorm2d calls on the groups do.  y = act((x - mean) * invstd * weight + bias [+ residual]), act = ReLU if relu.
 * save_mean / save_invstd: [G*C] outputs for the backward pass; partials: dfe_bn_partials_floats floats of scratch.
 * Backward: g' = gy masked by y > 0 when relu; gx, gres (= g', may be NULL), gweight / gbias [C] (may be NULL);
 * scratch_means: 2*G*C floats. */
long dfe_bn_partials_floats(int G, int Bg, int C, int H, int W);
int dfe_bn_fwd(const float* x, const float* residual, const float* weight, const float* bias, float* running_mean,
               float* running_var, float* y, float* save_mean, float* save_invstd, float* partials, int G, int Bg, int C,
               int H, int W, float eps, float momentum, int relu, void* stream);
int dfe_bn_bwd(const float* x, const float* y, const float* gy, const float* weight, const float* save_mean,
               const float* save_invstd, float* gx, float* gres, float* gweight, float* gbias, float* partials,
               float* scratch_means, int G, int Bg, int C, int H, int W, int relu, void* stream);

/* ---- eval-mode BatchNorm2d (+ residual + ReLU) of the depth encoder, forward only (inference.py).
 * dfe_bn_fold: one launch; per channel, in double, s = weight / sqrt((double)running_var + eps) and t = bias - running_mean * s
 *              (the unrounded s), each rounded once to fp32 into scale / shift [C].  weight / bias may be NULL (1 / 0).
 * dfe_bn_eval_fwd: y = act(x * scale[c] + shift[c] [+ residual]) over x [B,C,H,W], act = ReLU if relu; the product, the add and the
 *              residual add are each rounded once, in that order (no FMA).  residual may be NULL.  y == x (in place) is allowed;
 *              residual must not alias y.  One read of x (and residual), one write of y, no workspace; 16-byte accesses when
 *              H*W % 4 == 0 and x, y and residual are 16-byte aligned, dword accesses otherwise; every access stays inside
 *              [0, B*C*H*W) of its tensor.  B*C is not limited by a grid dimension; DFE_ERR_DIMS when H*W >= 2^31 or
 *              B*C*ceil(H*W / 512) >= 2^30. */
int dfe_bn_fold(const float* weight, const float* bias, const float* running_mean, const float* running_var, float eps,
                float* scale, float* shift, int C, void* stream);
int dfe_bn_eval_fwd(const float* x, const float* residual, const float* scale, const float* shift, float* y, int B, int C, int H,
                    int W, int relu, void* stream);

/* ---- convolution epilogue of the flow nets (net_utils.py conv() = Conv2d(bias) + LeakyReLU(0.1),
 * feature_pyramid.py:7-36, pwc_tf.py:16-95): the convolution itself runs on MIOpen *without* its bias, then
 * dfe_bias_act_fwd: z [B,C,H,W] <- act(z + bias[c]) in place; act(v) = v > 0 ? v : slope*v (0.1 LeakyReLU, 0 ReLU, 1 none);
 *                   bias may be NULL.
 * dfe_bias_act_bwd: gz = gy * act'(y) (decided on the sign of the output y), gbias[c] = sum_{b,h,w} gz (gbias may be NULL).
 *                   gy may be a channel slice of a wider tensor: element (b,c,i) at gy + b*gy_batch_stride + c*H*W + i.
 *                   partials: dfe_bias_act_partials_floats(B,C,H,W) floats of scratch (needed when gbias != NULL). */
long dfe_bias_act_partials_floats(int B, int C, int H, int W);
int dfe_bias_act_fwd(float* z, const float* bias, int B, int C, int H, int W, float slope, void* stream);
int dfe_bias_act_bwd(const float* y, const float* gy, long gy_batch_stride, float* gz, float* gbias, float* partials,
                     int B, int C, int H, int W, float slope, void* stream);

/* The same epilogue inside a DenseNet-style block (PWC_tf's decoder levels, pwc_tf.py:113-117 and the same five lines
 * per level: x2 = conv(cat(x0, x1)), x3 = conv(cat(x1, x2)) ...): act(z + bias) is written straight into the channel
 * slices of the concatenated buffers that consume it (dst2 optional; dst1 may be z), and the backward pass sums the
 * matching slices of the consumers' input gradients (g2 optional) and reads y from its slice.  Every slice is a base
 * pointer + a batch stride in floats; channel planes are contiguous inside a sample. */
int dfe_bias_act_fwd2(const float* z, const float* bias, float* dst1, long dst1_batch_stride, float* dst2,
                      long dst2_batch_stride, int B, int C, int H, int W, float slope, void* stream);
int dfe_bias_act_bwd2(const float* y, long y_batch_stride, const float* g1, long g1_batch_stride, const float* g2,
                      long g2_batch_stride, float* gz, float* gbias, float* partials, int B, int C, int H, int W,
                      float slope, void* stream);
/* With gbias == NULL and partials != NULL dfe_bias_act_bwd / dfe_bias_act_bwd2 only write the per-block partial sums; the
 * bias gradients of up to 8 such layers of one plane size (a PWC decoder level: pwc_tf.py:113-117) are then finished by
 * ONE launch: host arrays of n device pointers / channel counts; same summation order as the single-layer finish. */
int dfe_bias_grad_final_multi(const float* const* partials, float* const* gbias, const int* C, int n, int B, int H, int W,
                              void* stream);

/* ---- fused loss stack: everything from model_geometry.py:797 to :951 given the nets' outputs ---
 * One call computes the active loss_pack vectors of Model_geometry.forward (mode 0) for a batch:
 * pyramids (:65-72,:91), rigid view synthesis (:80-103), texture / occlusion / validity / dynamic
 * masks (:105-140,:685-713), flow warps (:74-78), masked L1 (:143-153), SSIM (:212-223),
 * smoothness (:225-279), flow consistency (:195-210), depth-flow consistency (:716-732) and the
 * epipolar distance (:355-418).  The backward call consumes d(total)/d(loss vectors) and writes
 * gradients wrt disparities, flows and pose (recompute-in-backward; only the 1-byte mask pack and
 * the masked warped images are kept in the workspace).
 *
 * loss rows of `losses` / `grad_losses` ([DFE_NUM_LOSSES][B], fp32): */
#define DFE_LOSS_DEPTH_PIXEL 0
#define DFE_LOSS_DEPTH_SMOOTH 1
#define DFE_LOSS_FLOW_PIXEL 2
#define DFE_LOSS_FLOW_SSIM 3
#define DFE_LOSS_FLOW_SMOOTH 4
#define DFE_LOSS_FLOW_CONSIS 5
#define DFE_LOSS_DEPTH_FLOW_CONSIS 6
#define DFE_LOSS_EPIPOLAR 7
/* the two depth terms the reference ships commented out (model_geometry.py:889-891,897-899):
 * rows 8 / 9 are written (and differentiated) only when the matching bit of dfe_geom_args.depth_terms is set, 0 otherwise */
#define DFE_LOSS_DEPTH_SSIM 8
#define DFE_LOSS_DEPTH_CONSIS 9
#define DFE_NUM_LOSSES 10
#define DFE_DEPTH_TERM_SSIM 1    /* compute_ssim_loss(img_list, reconstructed_imgs_from_{l,r}, {bwd,fwd}_mask_texture) */
#define DFE_DEPTH_TERM_CONSIS 2  /* compute_consis_loss(predicted_depths_to_{l,r}, computed_depths_to_{l,r}, ..._mask_texture), model_geometry.py:182-193 */

/* mask pack: one byte per pixel of every scale, [scale][B][Hs*Ws] */
#define DFE_MASK_VALID_BWD 0x01
#define DFE_MASK_VALID_FWD 0x02
#define DFE_MASK_OCC_BWD 0x04
#define DFE_MASK_OCC_FWD 0x08
#define DFE_MASK_DYNA_BWD 0x10
#define DFE_MASK_DYNA_FWD 0x20
#define DFE_MASK_TEX_BWD 0x40
#define DFE_MASK_TEX_FWD 0x80

typedef struct dfe_geom_args {
  int B, H, W;               /* batch, full-resolution frame size */
  int num_scales;            /* S <= DFE_MAX_SCALES; scale s is int(H/2^s) x int(W/2^s) */
  int align_corners;
  int mode;                  /* 0 = Model_geometry loss stack; 1 = Model_depth loss stack (model_depth.py:272-337:
                                depth pixel + smoothness terms; flow / K_inv pointers are ignored); 2 = Model_flow
                                loss stack (model_flow.py:209-261: box-mean pyramids, soft occlusion weights;
                                disp / pose / K / K_inv pointers are ignored) */
  float alpha, beta;         /* flow_consist_alpha / flow_consist_beta (model_geometry.py:25-26) */
  const float* img[3];       /* left, target, right frames [B,3,H,W] */
  const float* disp[3][DFE_MAX_SCALES]; /* depth_net outputs per frame (l,t,r) and scale [B,1,Hs,Ws] */
  const float* flow[2][DFE_MAX_SCALES]; /* pwc flows, dir 0 = target->left (bwd), 1 = target->right (fwd), [B,2,Hs,Ws] */
  const float* pose;         /* [B,2,6]; index 0 = bwd, 1 = fwd (model_geometry.py:789-790) */
  const float* K;            /* [B,3,3] scale-0 intrinsics */
  const float* K_inv;        /* [B,3,3] */
  float* workspace;          /* dfe_geom_workspace_floats(args) floats, kept from forward to backward */
  long workspace_floats;
  float* losses;             /* forward out */
  const float* grad_losses;  /* backward in */
  float* grad_disp[3][DFE_MAX_SCALES]; /* backward out, same shapes as disp (NULL = skip) */
  float* grad_flow[2][DFE_MAX_SCALES]; /* backward out, same shapes as flow (NULL = skip) */
  float* grad_pose;          /* backward out [B,2,6] (NULL = skip) */
  int depth_terms;           /* modes 0 and 1: DFE_DEPTH_TERM_* bits; 0 = the reference as shipped (mode 1 = the same two
                                lines of Model_depth, model_depth.py:326-327,332-333: mask = validity x texture, the
                                consistency term unmasked).  With
                                DFE_DEPTH_TERM_CONSIS the SOURCE disparities grad_disp[0], grad_disp[2] also receive the
                                gradient of the projected depth: a bilinear scatter in 64-bit fixed point (integer
                                atomics, csrc/dfe_scatter.h), so these gradients are bitwise reproducible like all others. */
} dfe_geom_args;

/* Memory contract of dfe_geom_loss_fwd / dfe_geom_loss_bwd.  The forward reads the frames, the disparities (modes 0, 1), the
 * flows (modes 0, 2), pose and K (modes 0, 1), K_inv (mode 0); it writes every element of losses [DFE_NUM_LOSSES][B] (all ten
 * rows in every mode; only the rows of the mode's terms carry meaning) and the workspace, nothing else.  The backward reads the
 * same inputs, grad_losses and the workspace; it writes every element of each gradient that is not NULL and the workspace,
 * nothing else.  A NULL gradient is skipped -- no kernel stores through it -- and the others keep their bits.  Inputs are
 * never written.
 * workspace: dfe_geom_workspace_floats(args) floats (the size depends on B, H, W, num_scales, mode, depth_terms and on
 * DFE_ADJ_MODE in the environment, not on any pointer); nothing outside them is touched; a smaller workspace_floats is
 * DFE_ERR_WORKSPACE before any launch.  Contents are undefined on entry to the forward: every region is written before it is
 * read, so one workspace may serve calls of other shapes, modes and depth_terms one after another.  The backward relies on
 * what the forward of the SAME arguments left there -- cameras and epipolar blocks, pyramid levels >= 1, the mask pack
 * (modes 0, 1; mode 2 leaves it unwritten), the masked warped images and rigid reconstructions, the soft weights of mode 2,
 * the normalisers -- and leaves all of that unchanged: it writes its own scratch regions only, so it may run more than once on
 * one forward and the mask pack may be decoded after it.
 * Alignment: workspace on 16 bytes (DFE_ERR_DIMS otherwise, from both entry points, before any launch: every region starts a
 * multiple of 16 bytes into it, the pyramid levels are stored in pairs and the depth-consistency term keeps a scatter
 * workspace of 64-bit accumulators there, csrc/dfe_scatter.h); every other pointer needs dword alignment only.  With
 * H % 4 == 0, W % 4 == 0, num_scales >= 3, mode 0 or 1 and all three frames on 16 bytes the pyramid levels 1 and 2 come from one
 * kernel that reads the frames with 16-byte loads, otherwise from the per-level kernel: the same bits either way
 * (DFE_PYRAMIDS_GENERIC in the environment, read at every call, forces the latter). */
long dfe_geom_workspace_floats(const dfe_geom_args* args);
/* byte offset of the mask pack inside the workspace, and its size in bytes per scale start */
long dfe_geom_maskpack_offset_bytes(const dfe_geom_args* args, int scale);
int dfe_geom_loss_fwd(const dfe_geom_args* args, void* stream);
int dfe_geom_loss_bwd(const dfe_geom_args* args, void* stream);
/* The launch plan the two entry points above pick for `args`: host only, nothing is launched, no device is needed and no
 * pointer is followed (the three frame pointers are looked at for their alignment; every other pointer may be NULL).
 * DFE_PYRAMIDS_GENERIC and DFE_ADJ_MODE are honoured as the launchers honour them.  Errors as dfe_geom_workspace_floats.
 * plan receives DFE_GEOM_PLAN_INTS ints:
 *   [0] S  [1] pyramid levels 1-2 from the two-level kernel (0 / 1)  [2] (frame, level) jobs of the per-level kernel
 *   [3] box-mean jobs of k_geom_area_coarse  [4] adj_mode (0 separable, 1 mixed, 2 gather)  [5] adj_s0 (first level of the
 *   two-pass adjoint; S = none)  [6] adj_nseg  [7] nblk_total, [8] fs_start[S]: the pointwise blocks and the flow-smoothness
 *   units per sample, whose maximum sizes the flow-smoothness partials  [9] dsm_units, [10] nblk0: disparity-smoothness units
 *   and full-resolution blocks, whose maximum sizes the disparity-smoothness partials  [11] DFE_DEPTH_TERM_* bits in effect
 *   [12] total workspace floats, low 31 bits  [13] total >> 31  [14] rows per block of the forward rolling kernels  [15] of the
 *   backward ones;
 *   then DFE_GEOM_PLAN_PER_SCALE ints per scale s at DFE_GEOM_PLAN_HEAD + DFE_GEOM_PLAN_PER_SCALE * s:
 *   H_s, W_s, forward strips (62 valid columns: SSIM, flow and disparity smoothness), valid columns of the last forward strip,
 *   backward strips (60: SSIM and flow-smoothness backward), valid columns of the last backward strip, rows of the last row
 *   block. */
#define DFE_GEOM_PLAN_HEAD 16
#define DFE_GEOM_PLAN_PER_SCALE 7
#define DFE_GEOM_PLAN_INTS (DFE_GEOM_PLAN_HEAD + DFE_GEOM_PLAN_PER_SCALE * DFE_MAX_SCALES)
int dfe_geom_plan(const dfe_geom_args* args, int* plan);

/* Diagnostic variants used by bench.py: identical launches with a hipEvent recorded on `stream`
 * between them; they synchronise on the last event and return the per-segment durations in
 * milliseconds in `ms_host` (host array).  Forward segments: 0 cameras+epipolar prep, 1 pyramids,
 * 2 k_geom_point_fwd (warp stage), 3 k_geom_ssim_fwd, 4 flow smoothness, 5 disparity smoothness,
 * 6 finalize.  Backward segments: 0 k_geom_ssim_bwd, 1 k_geom_point_bwd, 2 flow smoothness,
 * 3 disparity smoothness stage 1, 4 stage 2, 5 pose finalize. */
#define DFE_GEOM_FWD_SEGMENTS 7
#define DFE_GEOM_BWD_SEGMENTS 6
int dfe_geom_loss_fwd_profiled(const dfe_geom_args* args, void* stream, float* ms_host);
int dfe_geom_loss_bwd_profiled(const dfe_geom_args* args, void* stream, float* ms_host);

/* Deferred read-out of the same events: the launches and the event records are enqueued on `stream` with no host
 * synchronisation (usable inside a running training step); *handle owns the events.  dfe_geom_timed_collect waits
 * for the last event of that call, writes the segment durations (7 forward / 6 backward floats) and frees the
 * handle; every handle must be collected exactly once. */
int dfe_geom_loss_fwd_timed(const dfe_geom_args* args, void* stream, void** handle);
int dfe_geom_loss_bwd_timed(const dfe_geom_args* args, void* stream, void** handle);
int dfe_geom_timed_collect(void* handle, float* ms_host);

/* ---- evaluation metrics on a device-resident set (evaluate_flow.py:85-174, evaluate_depth.py:13-52, evaluation_utils.py:11-32)
 * A set of N samples of differing sizes lies in planes padded to [N,Hmax,Wmax] (Wmax a multiple of 4, the planes on 16 bytes:
 * DFE_ERR_DIMS otherwise) with an int table per sample: flow `dims` [N,2] = H, W; depth `dims` [N,6] = H, W and the crop box
 * y0, y1, x0, x1 (half open, computed by the host as evaluate_depth.py does).  A call takes a batch of n <= 1024 predictions at
 * the training size (h, w) for the set rows first .. first+n-1 and writes one float64 record per sample to records[0 .. n).
 * The prediction is resized to (H_i, W_i) bilinearly with half-pixel centres and edge replication: the source coordinate in
 * double, its weight rounded to fp32, top = a (1 - wx) + b wx, bot likewise, top (1 - wy) + bot wy in fp32.  Per-pixel
 * arithmetic is the reference's in fp32; every sum is in double and added in an order fixed by sample, block and thread index,
 * so a record does not depend on the batch it ran in, the stream or the run.  The only atomics are integer adds on histogram
 * bins.  The size table is read on the device and clamped to the planes: no entry can carry an access outside them.  Padding
 * (columns >= W_i, rows >= H_i) may hold anything; it reaches no sum.
 *
 * dfe_eval_flow: pred [n,2,h,w]; gt_u, gt_v fp32 planes; flags a byte plane, bit 0 valid, bit 1 noc, bit 2 moving.  Each tap is
 *   scaled by fl32(W_i / w) (u) or fl32(H_i / h) (v) before the resize; epe = sqrt(du^2 + dv^2); an outlier is
 *   epe > 3 and epe / max(sqrt(u^2 + v^2), 1e-10) > 0.05.  Record, dfe_eval_flow_record_doubles() = 16 doubles:
 *     0 sum epe valid   1 sum epe noc   2 sum epe (valid - noc)   3 sum epe valid mv   4 sum epe valid (1 - mv)
 *     5 sum valid       6 sum noc       7 sum (valid - noc): a pixel with noc = 1, valid = 0 counts -1, as in the reference
 *     8 outliers under valid   9 under valid mv   10 under valid (1 - mv)   11 sum valid mv   12 sum valid (1 - mv)   13-15 zero
 *   Two launches: blocks -> ws (dfe_eval_flow_ws_bytes(n) bytes, 8-byte aligned, no initialisation), then the blocks of a sample
 *   in index order -> its record.
 * dfe_eval_flow_finish: the records of a whole task -> table[8] = epe, epe_noc, epe_occ, err_rate, epe_move, epe_static,
 *   move_err_rate, static_err_rate: the ratio per sample (the occ denominator clamped to >= 1), the mean over the samples in
 *   index order, in double; the last four are 0 without has_moving (eval_flow_avg without moving masks).
 * dfe_eval_depth: disp [n,1,h,w]; gt one fp32 plane.  mask = gt > min_depth and gt < max_depth inside the crop box;
 *   pred = 1 / (resize(disp) + 1e-4), written to the workspace for the masked pixels only and read from there by the later
 *   passes; the medians of gt[mask] and pred[mask] in numpy's sense (the mean of the two middle values for an even count) by an
 *   exact radix select over the bit patterns (positive floats order as unsigned integers): per 8-bit digit a histogram launch
 *   (an LDS histogram per block, folded into a per-sample global integer histogram) and a pick launch, both middle ranks of both
 *   planes carried through the same four passes; then pred *= med_gt / med_pred, both clamped to [min_depth, max_depth], and
 *   the seven sums.  Record, dfe_eval_depth_record_doubles() = 10 doubles: abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3,
 *   median(gt[mask]), median(pred[mask]) (each an fp32 value), the masked count.  An empty mask gives NaN metrics.
 *   ws: dfe_eval_depth_ws_bytes(n, Hmax, Wmax) bytes on 16 bytes, no initialisation; n planes of pred first.  All samples of the
 *   batch run in one grid (blocks per sample, n); eleven enqueued operations per call.
 * A smaller ws_bytes is DFE_ERR_WORKSPACE; every refusal comes before the first launch and writes nothing. */
int dfe_eval_flow_record_doubles(void);
int dfe_eval_depth_record_doubles(void);
long dfe_eval_flow_ws_bytes(int n);
long dfe_eval_depth_ws_bytes(int n, int Hmax, int Wmax);
int dfe_eval_flow(const float* pred, int n, int h, int w, const float* gt_u, const float* gt_v, const unsigned char* flags,
                  const int* dims, int N, int Hmax, int Wmax, int first, void* ws, long ws_bytes, double* records, void* stream);
int dfe_eval_flow_finish(const double* records, int N, int has_moving, double* table, void* stream);
int dfe_eval_depth(const float* disp, int n, int h, int w, const float* gt, const int* dims, int N, int Hmax, int Wmax, int first,
                   float min_depth, float max_depth, void* ws, long ws_bytes, double* records, void* stream);

/* ---- top-k selection in pixel order  model_geometry.py:427-437 (top_ratio_sample) ------------------------------------------
 * scores [planes, n] -> idx int32 [planes, k]: the pixel indices of the k largest scores of each plane in ASCENDING pixel order.
 * Order of torch.topk: NaN ranks above +inf, -0 equals +0; equal scores at the threshold go to the lower pixel index.  One
 * workgroup per plane: a radix select over order-preserving keys (LDS integer histograms), then an ordered compaction.  No float
 * atomics and no host read: bitwise reproducible and capturable.
 * Memory contract: reads scores [planes * n], writes every element of idx [planes * k] and of ws, dfe_topk_ws_bytes(planes, n, k)
 * bytes on 4 bytes, no initialisation: per plane four words -- the threshold's key, the count of scores above it, the count of
 * ties taken, 0.  1 <= k <= n, or DFE_ERR_DIMS before the launch. */
long dfe_topk_ws_bytes(int planes, int n, int k);
int dfe_topk_select(const float* scores, int* idx, void* ws, int planes, int n, int k, void* stream);

/* ---- triangulation loss  model_geometry.py:569-683, call site :939-940 -------------------------------------------------------
 * Point (d, b, j), d < 2 directions (0: target -> left, 1: target -> right), b < B, j < num, is the pixel
 * idx[d*B + b][pick[j]] (idx int32 [2B, k] from dfe_topk_select, pick int64 [num] in [0, k); both are clamped on the device, so
 * no entry can carry an access outside the planes).  flow_bwd / flow_fwd [B,2,H,W] scale-0 flows, disp_t / disp_l / disp_r
 * [B,1,H,W], T34 [B,2,12] (pose_vec2mat of both directions), K / K_inv [B,9].  The match (x, y, x + u, y + v) is mid-point
 * triangulated under P1 = K [I|0], P2 = K T34, reprojected into both views, disp_t is sampled at the first coordinate and the
 * source disparity at the second (bilinear, reflection padding, align_corners as given) -- the reference's expressions and
 * epsilons, evaluated in double.
 * dfe_triangulate_fwd: writes rec, 2*B*num records of four doubles (inter1, z1, inter2, z2).
 * dfe_triangulate_stats: per (b, d, view) the lower medians of inter and z (torch.median: rank (num-1)/2; radix select in LDS,
 *   num <= 16384 or DFE_ERR_UNSUPPORTED), the detached scale and scale_adapt's a, the view's loss -> stats [B,2,2,4] doubles
 *   (scale, a, a / (scale + 1e-12), loss), then loss[b] = (L00 + L01) + (L10 + L11).  Sums in double, order fixed by thread index.
 * dfe_triangulate_bwd: from gloss [B]: grads, 7*B*H*W floats = the gradients of flow_bwd, flow_fwd (2*B*H*W each), disp_t, disp_l,
 *   disp_r (B*H*W each), every element written; gT34 [B,2,12].  scale and a are constants, as in the reference.  Per-point
 *   derivatives by forward-mode duals; points repeat, so every scatter goes through 64-bit fixed-point accumulators (integer
 *   atomics); gT34 from per-block partial sums added in block order.  ws: dfe_triangulate_ws_bytes(B, H, W, num) bytes on 16
 *   bytes, no initialisation.  A memset and three launches.
 * Every result is bitwise reproducible.  H, W >= 2, H*W < 2^28, k <= H*W; refusals come before the first launch. */
long dfe_triangulate_ws_bytes(int B, int H, int W, int num);
int dfe_triangulate_fwd(const float* flow_bwd, const float* flow_fwd, const float* disp_t, const float* disp_l,
                        const float* disp_r, const float* T34, const float* K, const float* K_inv, const int* idx,
                        const long long* pick, double* rec, int B, int H, int W, int k, int num, int align_corners, void* stream);
int dfe_triangulate_stats(const double* rec, double* stats, float* loss, int B, int num, void* stream);
int dfe_triangulate_bwd(const float* flow_bwd, const float* flow_fwd, const float* disp_t, const float* disp_l,
                        const float* disp_r, const float* T34, const float* K, const float* K_inv, const int* idx,
                        const long long* pick, const double* stats, const float* gloss, float* grads, float* gT34, void* ws,
                        int B, int H, int W, int k, int num, int align_corners, void* stream);

/* ---- eight-point loss  model_geometry.py:532-566, call site :949-950 ---------------------------------------------------------
 * The robust fundamental matrix of the sampled matches (the FM_RANSAC branch of GeometrySolvers.compute_fundmental_mat, step for
 * step, all estimation arithmetic in double) and the smooth-L1 loss against the pose's K^-T ([t]x R) K^-1.
 * Plane p = d*B + b (d = 0: target -> left from flow_bwd, 1: target -> right from flow_fwd).  Match j < num of plane p is the
 * pixel idx[p][pick[j]] -- idx int32 [2B, k], pick int64 [num], as dfe_triangulate_fwd takes them and clamped on the device in the
 * same way -- as (x, y, x + u, y + v), the sums formed in fp32 and then widened.  sets int32 [B, hyp, 8]: the minimal sets,
 * indices into [0, num) (clamped on the device); both directions of sample b use sets[b].
 * dfe_fundamental_ransac: a memset of the counts and four launches, no host read.
 *   1. matches [2B, num, 4] doubles.
 *   2. per (plane, hypothesis) the normalised eight-point solve of its 8 matches: Hartley normalisation with unit weights (the
 *      + 1e-12 included), the 9x9 normal matrix (in LDS, 162 doubles per thread), its smallest eigenvector by cyclic Jacobi (at
 *      most 20 sweeps), rank 2 by a one-sided Jacobi on the 3x3 (at most 12 sweeps), un-normalised.  A hypothesis only votes.
 *   3. per (plane, hypothesis) the count of matches whose residual -- the larger of the two squared point-to-line distances, with
 *      the 1e-300 guards -- is <= thresh^2; a non-finite residual is an outlier.  Blocks hold a tile of 256 matches and pass the
 *      hypotheses through LDS in tiles of 64; integer atomics only.
 *   4. per plane: the hypothesis with the most inliers (ties: the lowest index) and its inlier set, all matches if that set has
 *      fewer than 8; the weighted normalised eight-point over the set (the normal matrix summed in double in an order fixed by
 *      thread index); the inlier set of that refit (fewer than 8: the previous set) and one more refit; F / F[2][2].
 *   Writes every element of F64 [2B, 9] doubles, of F32 [2B, 9] (the same values rounded once) and of info int32 [2B, 4]: the
 *   winning hypothesis, its count, the sizes of the two refit sets.  NaN or inf in a plane's flows at a sampled pixel gives a
 *   non-finite F for that plane; every loop has a fixed bound.
 *   ws: dfe_eight_point_ws_bytes(B, num, hyp) bytes on 16 bytes, no initialisation, every byte of the five sections' payload
 *   written.  Sections, each starting on 16 bytes, r16 = rounded up to 16: matches at 0 (32*2B*num bytes); the hypotheses'
 *   F [2B, hyp, 9] doubles at 64*B*num; the counts int32 [2B, hyp] at 64*B*num + r16(144*B*hyp); the 0/1 weights of the first
 *   refit int32 [2B, num] after r16(8*B*hyp) more; those of the second refit after r16(8*B*num) more.
 *   Refusals before the first launch: num < 8, hyp < 1, k > H*W, k < 1, H*W >= 2^28 -> DFE_ERR_DIMS; num > 16384 or hyp > 4096 ->
 *   DFE_ERR_UNSUPPORTED; ws not on 16 bytes or F64 not on 8 -> DFE_ERR_DIMS.  FM_RANSAC only (no LMedS).
 * dfe_eight_point_loss_fwd: E [2B, 9] (dfe_pose_vec2mat_fwd's second output for pose.reshape(2B, 6): row b*2 + d), Kt_inv and
 *   K_inv [B, 9], F32 [2B, 9] (plane d*B + b).  F_meta = E K_inv, F_pred = Kt_inv F_meta in fp32 (sums in index order);
 *   loss[b] = mean_9 smooth_l1(F_pred - F)(d = 0) + mean_9 smooth_l1(F_pred - F)(d = 1), beta = 1.  Reads the four inputs, writes
 *   every element of loss [B]; no workspace; one launch.
 * dfe_eight_point_loss_bwd: from gloss [B] writes every element of gE [2B, 9]; F is a constant.  No workspace; one launch.
 * Every result is bitwise reproducible (no float atomics). */
long dfe_eight_point_ws_bytes(int B, int num, int hyp);
int dfe_fundamental_ransac(const float* flow_bwd, const float* flow_fwd, const int* idx, const long long* pick, const int* sets,
                           double* F64, float* F32, int* info, void* ws, int B, int H, int W, int k, int num, int hyp,
                           double thresh, void* stream);
int dfe_eight_point_loss_fwd(const float* E, const float* Kt_inv, const float* K_inv, const float* F32, float* loss, int B,
                             void* stream);
int dfe_eight_point_loss_bwd(const float* E, const float* Kt_inv, const float* K_inv, const float* F32, const float* gloss,
                             float* gE, int B, void* stream);

/* ---- PnP loss  model_geometry.py:473-530, call site :944-945 -----------------------------------------------------------------
 * The robust pose that reprojects the target frame's back-projected matches onto their matched pixels (the robust branch of
 * GeometrySolvers.pnp -- _pnp_hypotheses, scoring, consensus, _pnp_refine, re-score, _pnp_refine -- step for step, all
 * estimation arithmetic in double) and the L1 loss between that pose and the pose vector.
 * Planes, idx and pick as the eight-point entry takes them and clamps them.  Match j of plane p = d*B + b at pixel (x, y) is the
 * point X = K_inv[b] (x, y, 1) * disp_t[b][pixel], formed in double from the fp32 inputs (the composition's compute_pnp_loss
 * rounds it to fp32 first: a deliberate deviation), and the pixel (x + u, y + v), the sums formed in fp32 and then widened.  As at
 * the commented call site the raw scale-0 disparity of the target frame is the "depth" of both directions.  sets int32
 * [B, hyp, 6]: the minimal sets, indices into [0, num) (clamped on the device); both directions of sample b use sets[b].
 * K, K_inv fp32 [B, 9]: K[b] projects sample b (fx, fy, cx, cy = K[0], K[4], K[2], K[5]; its inverse, formed in double as the
 * adjugate over the determinant, normalises the hypotheses' pixels), K_inv[b] back-projects it.
 * The pnp ransac entry: a memset of the counts and four launches, no host read.
 *   1. points [2B, num, 5] doubles: X, Y, Z, x + u, y + v.
 *   2. per (plane, hypothesis) the six-point DLT pose of its 6 matches: the 12x12 normal matrix of the system
 *      [Xh, 0, -u Xh; 0, Xh, -v Xh] (in LDS, 288 doubles per thread with the eigenvectors), its smallest eigenvector by cyclic
 *      Jacobi (at most 24 sweeps), the left 3x3 projected onto SO(3) by a one-sided Jacobi (at most 12 sweeps), the scale from the
 *      mean singular value (at least 1e-300), the sign from the determinant.  A hypothesis only votes.
 *   3. per (plane, hypothesis) the count of matches with eu^2 + ev^2 <= thresh^2 and z > 0, the projection dividing by
 *      max(z, 1e-9); a non-finite residual is an outlier.  Blocks hold a tile of 256 matches and pass the hypotheses through LDS
 *      in tiles of 64; integer atomics only.
 *   4. per plane: the hypothesis with the most inliers (ties: the lowest index) and its inlier set, all matches if that set has
 *      fewer than 6; iters Levenberg-Marquardt iterations on SE(3) over the set (left-multiplied exp([omega]x), damping scaled by
 *      max(diag H, 1e-12), accept on cn < cost, lambda * 0.3 on accept and * 5 on reject within [1e-9, 1e6], lambda = 1e-3 at the
 *      start; the 28 sums of an iteration -- 21 of H, 6 of g, the cost -- reduced in double in an order fixed by thread index;
 *      the 6x6 solve by elimination with partial pivoting); the inlier set of the refined pose (fewer than 6: the previous set);
 *      max(iters / 2, 1) more iterations on it; the rotation's logarithm.
 *   Writes every element of P64 [2B, 6] doubles = (T, axis-angle), of P32 [2B, 6] (the same values rounded once) and of info int32
 *   [2B, 4]: the winning hypothesis, its count, the sizes of the two refinement sets after their fall-backs.  NaN or inf in a
 *   sample's flows or disparity at a sampled pixel gives an unspecified, possibly non-finite pose for that sample's planes and
 *   leaves the other samples' bits alone; every loop has a fixed bound.
 *   ws: the ws_bytes entry's answer for (B, num, hyp), bytes on 16 bytes, no initialisation, every byte of the five sections'
 *   payload written.  Sections, each starting on 16 bytes, r16 = rounded up to 16: points at 0 (40*2B*num bytes); the hypotheses'
 *   (R row-major, T) [2B, hyp, 12] doubles at 80*B*num; the counts int32 [2B, hyp] at 80*B*num + 192*B*hyp; the 0/1 weights of the
 *   first refinement int32 [2B, num] after r16(8*B*hyp) more; those of the second refinement after r16(8*B*num) more.
 *   Refusals before the first launch: num < 6, hyp < 1, k > H*W, k < 1, H*W >= 2^28, iters < 1 -> DFE_ERR_DIMS; num > 16384 or
 *   hyp > 4096 -> DFE_ERR_UNSUPPORTED; ws not on 16 bytes or P64 not on 8 -> DFE_ERR_DIMS.
 * The loss entries: pose fp32 [B, 2, 6] (row b*2 + d), P32 [2B, 6] (plane d*B + b), beta the rotation part's weight.
 *   forward: loss[b] = sum over d of mean_3(|P[:3] - pose[:3]| + beta |P[3:] - pose[3:]|) in fp32 -- (T, axis-angle) against
 *   (translation, Euler angles), the reference's comparison as written.  Writes every element of loss [B]; one launch.
 *   backward: from gloss [B] writes every element of gpose [B, 2, 6] = gloss[b] / 3 * sign(pose - P) * (1 | beta), sign(0) = 0;
 *   P is a constant.  No workspace; one launch.
 * Every result is bitwise reproducible (no float atomics). */
long dfe_pnp_ws_bytes(int B, int num, int hyp);
int dfe_pnp_ransac(const float* flow_bwd, const float* flow_fwd, const float* disp_t, const int* idx, const long long* pick,
                   const int* sets, const float* K, const float* K_inv, double* P64, float* P32, int* info, void* ws, int B, int H,
                   int W, int k, int num, int hyp, int iters, double thresh, void* stream);
int dfe_pnp_loss_fwd(const float* pose, const float* P32, float* loss, int B, float beta, void* stream);
int dfe_pnp_loss_bwd(const float* pose, const float* P32, const float* gloss, float* gpose, int B, float beta, void* stream);

/* ---- eight-point epipolar map  model_geometry.py:318-353 (compute_epipolar_map_8pF), call site :831-835 ------------------------
 * The dense epipolar distance of a flow under a GIVEN fundamental matrix (dfe_fundamental_ransac's F32, not the pose's), its plain
 * mean (compute_epipolar_loss, :413-418) and that mean's gradient to the flow.  Per pixel (x, y) of a plane with flow (u, v) and
 * F row-major, in fp32, evaluated as written (no contraction):
 *   l = F (x, y, 1)^T, each row as fma(F1, y, F0 * x) + F2;   s = ((x + u) * l0 + (y + v) * l1) + l2;
 *   div = sqrtf(l0*l0 + l1*l1) + 1e-6f;   dist = |s| / div, sqrtf and the division correctly rounded (the map feeds masks).
 * Plane p = d*B + b of the loss entries is direction d of sample b (d = 0: flow_bwd, 1: flow_fwd) and reads F32[p].  F is a
 * constant.  A thread owns quads of four consecutive pixels; where H*W % 4 == 0 and every flow, map and gradient pointer of
 * the call is on 16 bytes a quad moves as 16-byte accesses, otherwise as element accesses -- same assignment, same arithmetic, same
 * bits.  Every loop is bounded by the shape; a non-finite F or flow makes that plane's (that sample's) results non-finite and
 * nothing else.  No float atomics, no arrival ticket: bitwise reproducible.
 * dfe_epipolar_map: reads flow [P,2,H,W] and F32 [P,9], writes every element of dist [P,H,W]; plane p reads flow[p] and F32[p].
 *   One launch, no workspace.
 * dfe_epipolar_loss_fwd: reads flow_bwd, flow_fwd [B,2,H,W] and F32 [2B,9]; loss[b] = mean_HW dist(plane b) + mean_HW dist(plane
 *   B + b), every element of loss [B] written.  Sums in double: per block its threads' sums by a fixed tree -> ws, then one block
 *   per sample adds the partials of its two planes in an order fixed by block and thread index, divides each by H*W, adds, rounds
 *   once.  ws: dfe_epipolar_ws_bytes(B, H, W) bytes (one double per block and plane) on 8 bytes, no initialisation, every byte
 *   written.  Two launches.
 * dfe_epipolar_loss_bwd: reads the same inputs and gloss [B] (l, s and div are recomputed: nothing else is saved); writes every
 *   element of gflow_bwd and gflow_fwd [B,2,H,W]: (gloss[b] / (float)(H*W)) * sgn(s) * (l0, l1) / div, sgn(0) = 0.  One launch, no
 *   workspace.
 * Refusals before the first launch: a null pointer -> DFE_ERR_NULL; B (P) < 1, B > 16384 (P > 32768), H or W < 1, H*W >= 2^28, ws
 * not on 8 bytes -> DFE_ERR_DIMS.  flows, maps, gradients: 4-byte alignment suffices. */
long dfe_epipolar_ws_bytes(int B, int H, int W);
int dfe_epipolar_loss_fwd(const float* flow_bwd, const float* flow_fwd, const float* F32, float* loss, void* ws, int B, int H, int W,
                          void* stream);
int dfe_epipolar_loss_bwd(const float* flow_bwd, const float* flow_fwd, const float* F32, const float* gloss, float* gflow_bwd,
                          float* gflow_fwd, int B, int H, int W, void* stream);
int dfe_epipolar_map(const float* flow, const float* F32, float* dist, int P, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DFE_HIP_H */
