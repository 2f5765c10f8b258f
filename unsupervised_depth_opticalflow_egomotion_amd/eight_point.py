"""The eight-point term (model_geometry.py:532-566, call site :949-950) on the device: the kernels of csrc/ops_eight_point.hip
under autograd.

``fundamental_ransac`` gives the robust fundamental matrix of the matches of both directions -- the pixels ``idx[p][pick[j]]``
of the scale-0 flows, as the triangulation term takes them -- by the FM_RANSAC branch of
``GeometrySolvers.compute_fundmental_mat``, step for step, in double, with the minimal sets as an argument.  It is a constant of
the step (the reference builds it from numpy), so it has no backward.  ``EightPointLossFn`` is the smooth-L1 loss between that
matrix and the pose's ``K^-T ([t]x R) K^-1``; its gradient reaches the pose through ``PoseMatsFn``'s essential matrix alone.
Nothing here reads a value back to the host, so a training step with the term can be captured in a hipGraph; every output is
bitwise reproducible.

Fidelity:
* the reference compares an UNNORMALISED ``F_pred`` with cv2's ``F[2,2] = 1`` matrix (model_geometry.py:565); that line is
  reproduced as written, not repaired;
* the draw deviations are the triangulation term's: the pixel-ordered top-k set, and no "some scores are zero" branch;
* cv2's own RANSAC draw cannot be pinned (cv2 is not available): the reference of the tests is this project's float64
  composition (``compute_fundmental_mat``) on the same sets, plus the analytic ``F`` of synthetic two-view problems;
* FM_RANSAC only: the LMedS branch (dataset ``nyuv2``) is not built;
* ``torch.inverse(K^T)`` checks its status flag on the host, which a capture refuses; the 3x3 inverse is formed in torch as the
  adjugate over the determinant instead (``inverse_transposed``)."""
import torch

from . import _ransac
from ._lib import check, f32c, get_lib, ptr, ptr_any, stream_ptr


def workspace_sections(B, num, hyp):
    """Byte offsets of the sections of dfe_fundamental_ransac's workspace, as include/dfe_hip.h states them: dict(matches, Fh,
    counts, w1, w2, bytes)."""
    return _ransac.workspace_sections(B, num, hyp, 4, 9, "matches", "Fh")


def fundamental_ransac(flow_bwd0, flow_fwd0, idx, pick, sets, thresh=0.1, return_ws=False):
    """(flow_bwd0, flow_fwd0 [B,2,H,W], idx int32 [2B,k] (planes: direction-major), pick int64 [num], sets int32 [B,hyp,8]) ->
    (F32 [2B,3,3] fp32, F64 [2B,3,3] float64, info int32 [2B,4]: winning hypothesis, its count, the sizes of the two refit sets).
    ``return_ws``: also the workspace (uint8; ``workspace_sections`` gives the offsets of the counts and the weights)."""
    lib = get_lib()
    flow_bwd0, flow_fwd0 = f32c(flow_bwd0.detach()), f32c(flow_fwd0.detach())
    B, H, W, k, num, hyp = _ransac.check_draw(flow_bwd0, flow_fwd0, idx, pick, sets, 8, "fundamental_ransac",
                                              "the eight-point algorithm")
    idx, pick, sets = idx.contiguous(), pick.contiguous(), sets.contiguous()
    dev = flow_bwd0.device
    F64 = torch.empty(2 * B, 3, 3, device=dev, dtype=torch.float64)
    F32 = torch.empty(2 * B, 3, 3, device=dev, dtype=torch.float32)
    info = torch.empty(2 * B, 4, device=dev, dtype=torch.int32)
    ws = torch.empty(lib.dfe_eight_point_ws_bytes(B, num, hyp), device=dev, dtype=torch.uint8)
    check(lib.dfe_fundamental_ransac(ptr(flow_bwd0), ptr(flow_fwd0), ptr(idx), ptr(pick), ptr(sets), ptr_any(F64), ptr(F32), ptr(info),
                                     ptr(ws), B, H, W, k, num, hyp, float(thresh), stream_ptr()), "dfe_fundamental_ransac")
    return (F32, F64, info, ws) if return_ws else (F32, F64, info)


def inverse_transposed(K):
    """inverse(K^T) of K [B,3,3] as the adjugate over the determinant, in torch elementwise operations (no status flag, no host
    read): the rows of inverse(K^T) are the cross products of K's rows over det K."""
    r0, r1, r2 = K[:, 0], K[:, 1], K[:, 2]
    c0 = torch.linalg.cross(r1, r2)
    adj = torch.stack([c0, torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)], 1)
    return adj / (r0 * c0).sum(1).view(-1, 1, 1)


class EightPointLossFn(torch.autograd.Function):
    """(E [2B,3,3] (PoseMatsFn's second output for pose.reshape(2B, 6): row b*2 + d), K, K_inv [B,3,3], F32 [2B,3,3] (plane
    d*B + b)) -> loss [B] = mean_9 smooth_l1(F_pred - F) of direction 0 + the same of direction 1, F_pred = inverse(K^T) E K^-1.
    The mean over b is the reference's scalar.  ``F32`` is a constant."""

    @staticmethod
    def forward(ctx, E, K, K_inv, F32):
        lib = get_lib()
        E, K, K_inv, F32 = f32c(E), f32c(K), f32c(K_inv), f32c(F32)
        B = K.shape[0]
        if tuple(K.shape) != (B, 3, 3) or tuple(K_inv.shape) != (B, 3, 3):
            raise ValueError("EightPointLossFn: K and K_inv [B,3,3] expected")
        if E.numel() != 2 * B * 9 or F32.numel() != 2 * B * 9:
            raise ValueError("EightPointLossFn: E and F32 [2B,3,3] expected")
        with torch.no_grad():
            Kt_inv = inverse_transposed(K).contiguous()
        loss = torch.empty(B, device=E.device, dtype=torch.float32)
        check(lib.dfe_eight_point_loss_fwd(ptr(E), ptr(Kt_inv), ptr(K_inv), ptr(F32), ptr(loss), B, stream_ptr()),
              "dfe_eight_point_loss_fwd")
        ctx.save_for_backward(E, Kt_inv, K_inv, F32)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        lib = get_lib()
        E, Kt_inv, K_inv, F32 = ctx.saved_tensors
        B = K_inv.shape[0]
        gloss = f32c(gloss)
        gE = torch.empty_like(E)
        check(lib.dfe_eight_point_loss_bwd(ptr(E), ptr(Kt_inv), ptr(K_inv), ptr(F32), ptr(gloss), ptr(gE), B, stream_ptr()),
              "dfe_eight_point_loss_bwd")
        return gE, None, None, None
