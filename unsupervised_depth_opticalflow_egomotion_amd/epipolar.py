"""The eight-point epipolar term (model_geometry.py:318-353, call site :831-835) on the device: the kernels of
csrc/ops_epipolar.hip under autograd.

``epipolar_map`` is the dense distance of every pixel's match ``(x + u, y + v)`` to its epipolar line under a GIVEN fundamental
matrix -- ``compute_epipolar_map_8pF``'s map once ``F`` is there; ``EpipolarLossFn`` is ``compute_epipolar_loss`` of both directions
summed (the plain mean the reference returns, :413-418) with its gradient to the two scale-0 flows.  ``F`` is the robust matrix of
the step's sampled matches (``eight_point.fundamental_ransac``), a constant as in the reference, which builds it from numpy: the
flow is pulled towards the epipolar geometry its own best matches agree on and the pose net gets nothing from the term.  Nothing
here reads a value back to the host, so a step with the term can be captured in a hipGraph; every output is bitwise reproducible
(double sums in a fixed order, no float atomics).

Fidelity: the expression is the reference's, each line row as ``fma(F1, y, F0 * x) + F2`` -- the order the fused stack's own
epipolar term uses for ``f_mat.bmm(p1)`` -- with the correctly rounded square root and division (the map feeds
``get_rigid_mask``).  The cross-check is ``LossTerms.compute_epipolar_map_8pF`` in plain torch."""
import torch

from ._lib import check, f32c, get_lib, ptr, stream_ptr


def _planes(flow, F32, planes, what):
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError("%s: a flow [B,2,H,W] expected" % what)
    if F32.numel() != planes * 9:
        raise ValueError("%s: F32 [%d,3,3] expected" % (what, planes))


def epipolar_map(flow, F32):
    """(flow [P,2,H,W], F32 [P,3,3]) -> dist [P,1,H,W]: plane p under F32[p].  No gradient."""
    lib = get_lib()
    flow, F32 = f32c(flow.detach()), f32c(F32.detach())
    P, _, H, W = (int(v) for v in flow.shape) if flow.dim() == 4 else (0, 0, 0, 0)
    _planes(flow, F32, P, "epipolar_map")
    dist = torch.empty(P, 1, H, W, device=flow.device, dtype=torch.float32)
    check(lib.dfe_epipolar_map(ptr(flow), ptr(F32), ptr(dist), P, H, W, stream_ptr()), "dfe_epipolar_map")
    return dist


class EpipolarLossFn(torch.autograd.Function):
    """(flow_bwd0, flow_fwd0 [B,2,H,W], F32 [2B,3,3] (plane d*B + b, d = 0: backward flow)) -> loss [B] = mean_HW dist of the
    backward plane + mean_HW dist of the forward plane.  The mean over b is the reference's scalar.  The gradients go to the two
    flows; ``F32`` is a constant.  Nothing but the inputs is saved: the backward pass recomputes the lines."""

    @staticmethod
    def forward(ctx, flow_bwd0, flow_fwd0, F32):
        lib = get_lib()
        flow_bwd0, flow_fwd0, F32 = f32c(flow_bwd0), f32c(flow_fwd0), f32c(F32)
        if flow_bwd0.shape != flow_fwd0.shape:
            raise ValueError("EpipolarLossFn: two flows of one shape expected")
        B = int(flow_bwd0.shape[0])
        _planes(flow_bwd0, F32, 2 * B, "EpipolarLossFn")
        H, W = int(flow_bwd0.shape[2]), int(flow_bwd0.shape[3])
        loss = torch.empty(B, device=flow_bwd0.device, dtype=torch.float32)
        ws = torch.empty(lib.dfe_epipolar_ws_bytes(B, H, W), device=flow_bwd0.device, dtype=torch.uint8)
        check(lib.dfe_epipolar_loss_fwd(ptr(flow_bwd0), ptr(flow_fwd0), ptr(F32), ptr(loss), ptr(ws), B, H, W, stream_ptr()),
              "dfe_epipolar_loss_fwd")
        ctx.save_for_backward(flow_bwd0, flow_fwd0, F32)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        lib = get_lib()
        flow_bwd0, flow_fwd0, F32 = ctx.saved_tensors
        B, _, H, W = (int(v) for v in flow_bwd0.shape)
        gloss = f32c(gloss)
        g_bwd, g_fwd = torch.empty_like(flow_bwd0), torch.empty_like(flow_fwd0)
        check(lib.dfe_epipolar_loss_bwd(ptr(flow_bwd0), ptr(flow_fwd0), ptr(F32), ptr(gloss), ptr(g_bwd), ptr(g_fwd), B, H, W,
                                        stream_ptr()), "dfe_epipolar_loss_bwd")
        return g_bwd, g_fwd, None
