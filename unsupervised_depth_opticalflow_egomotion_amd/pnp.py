"""The PnP term (model_geometry.py:473-530, call site :944-945) on the device: the kernels of csrc/ops_pnp.hip under autograd.

``pnp_ransac`` gives the robust pose of both directions -- from the pixels ``idx[p][pick[j]]`` of the scale-0 flows, as the other
two geometric terms take them, back-projected with the target frame's scale-0 disparity -- by the robust branch of
``GeometrySolvers.pnp``, step for step, in double, with the minimal sets as an argument.  It is a constant of the step (the
reference builds it from numpy), so it has no backward.  ``PnpLossFn`` is the L1 loss between that (T, axis-angle) and the pose
vector; its gradient reaches the pose alone.  Nothing here reads a value back to the host, so a training step with the term can
be captured in a hipGraph; every output is bitwise reproducible.

Fidelity:
* the reference compares (T, axis-angle) with the pose vector's (translation, Euler angles) as they stand
  (model_geometry.py:525-528); that comparison is reproduced as written, not repaired;
* line 509 hands ``K[0]`` to ``pnp`` for every sample of the batch while the back-projection uses each sample's own ``K_inv``.
  ``pnp_ransac`` takes one camera matrix per sample; ``Model_geometry.pnp_term`` passes ``K[0]`` for all of them: as written, not
  repaired;
* the 3-D point is formed in double from the fp32 inputs; ``compute_pnp_loss`` rounds it to fp32 first.  Deliberate: the rounding
  (6e-8 of a depth) would sit in every residual and serves nothing;
* the draw deviations are the triangulation term's: the pixel-ordered top-k set, and no "some scores are zero" branch;
* as at the commented call site, the raw disparity is passed as "depth" (SURVEY.md A.7);
* cv2's own RANSAC and refinement cannot be pinned (cv2 is not available): the reference of the tests is this project's float64
  composition (``GeometrySolvers.pnp``) on the same sets, plus the analytic pose of synthetic two-view problems."""
import torch

from . import _ransac
from ._lib import check, f32c, get_lib, ptr, ptr_any, stream_ptr


def workspace_sections(B, num, hyp):
    """Byte offsets of the sections of dfe_pnp_ransac's workspace, as include/dfe_hip.h states them: dict(points, Ph, counts, w1,
    w2, bytes)."""
    return _ransac.workspace_sections(B, num, hyp, 5, 12, "points", "Ph")


def pnp_ransac(flow_bwd0, flow_fwd0, disp_t0, idx, pick, sets, K, K_inv, iters=20, thresh=1.0, return_ws=False):
    """(flow_bwd0, flow_fwd0 [B,2,H,W], disp_t0 [B,1,H,W], idx int32 [2B,k] (planes: direction-major), pick int64 [num], sets int32
    [B,hyp,6], K, K_inv [B,3,3]) -> (P32 [2B,6] fp32 = (T, axis-angle), P64 [2B,6] float64, info int32 [2B,4]: winning hypothesis,
    its count, the sizes of the two refinement sets).  ``return_ws``: also the workspace (uint8; ``workspace_sections`` gives the
    offsets of the counts and the weights)."""
    lib = get_lib()
    flow_bwd0, flow_fwd0, disp_t0 = f32c(flow_bwd0.detach()), f32c(flow_fwd0.detach()), f32c(disp_t0.detach())
    B, H, W, k, num, hyp = _ransac.check_draw(flow_bwd0, flow_fwd0, idx, pick, sets, 6, "pnp_ransac", "the six-point DLT")
    if disp_t0.numel() != B * H * W:
        raise ValueError("pnp_ransac: disp_t0 [B,1,H,W] of the flows' scale expected")
    K, K_inv = f32c(K.detach()), f32c(K_inv.detach())
    if tuple(K.shape) != (B, 3, 3) or tuple(K_inv.shape) != (B, 3, 3):
        raise ValueError("pnp_ransac: K and K_inv [B,3,3] expected")
    if int(iters) < 1:
        raise ValueError("pnp_ransac: at least one refinement iteration expected")
    idx, pick, sets = idx.contiguous(), pick.contiguous(), sets.contiguous()
    dev = flow_bwd0.device
    P64 = torch.empty(2 * B, 6, device=dev, dtype=torch.float64)
    P32 = torch.empty(2 * B, 6, device=dev, dtype=torch.float32)
    info = torch.empty(2 * B, 4, device=dev, dtype=torch.int32)
    ws = torch.empty(lib.dfe_pnp_ws_bytes(B, num, hyp), device=dev, dtype=torch.uint8)
    check(lib.dfe_pnp_ransac(ptr(flow_bwd0), ptr(flow_fwd0), ptr(disp_t0), ptr(idx), ptr(pick), ptr(sets), ptr(K), ptr(K_inv),
                             ptr_any(P64), ptr(P32), ptr(info), ptr(ws), B, H, W, k, num, hyp, int(iters), float(thresh),
                             stream_ptr()), "dfe_pnp_ransac")
    return (P32, P64, info, ws) if return_ws else (P32, P64, info)


class PnpLossFn(torch.autograd.Function):
    """(pose [B,2,6], P32 [2B,6] (plane d*B + b), beta) -> loss [B] = sum over d of mean_3(|P[:3] - pose[:3]| + beta |P[3:] -
    pose[3:]|).  The mean over b is the reference's scalar.  ``P32`` is a constant."""

    @staticmethod
    def forward(ctx, pose, P32, beta):
        lib = get_lib()
        pose, P32 = f32c(pose), f32c(P32)
        B = pose.shape[0]
        if tuple(pose.shape) != (B, 2, 6) or P32.numel() != 2 * B * 6:
            raise ValueError("PnpLossFn: pose [B,2,6] and P32 [2B,6] expected")
        loss = torch.empty(B, device=pose.device, dtype=torch.float32)
        check(lib.dfe_pnp_loss_fwd(ptr(pose), ptr(P32), ptr(loss), B, float(beta), stream_ptr()), "dfe_pnp_loss_fwd")
        ctx.save_for_backward(pose, P32)
        ctx.beta = float(beta)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        lib = get_lib()
        pose, P32 = ctx.saved_tensors
        gloss = f32c(gloss)
        gpose = torch.empty_like(pose)
        check(lib.dfe_pnp_loss_bwd(ptr(pose), ptr(P32), ptr(gloss), ptr(gpose), pose.shape[0], ctx.beta, stream_ptr()),
              "dfe_pnp_loss_bwd")
        return gpose, None, None
