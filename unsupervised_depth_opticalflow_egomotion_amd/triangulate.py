"""The triangulation term (model_geometry.py:569-683, call site :939-940) on the device: the selection kernel and the three
point kernels of csrc/ops_select.hip / csrc/ops_triangulate.hip under autograd.

``topk_select`` gives the pixel-ordered top-k set of every score plane, ``TriangulateFn`` the (B,) loss of both directions
from the scale-0 flows, the three scale-0 disparities and the pose matrices, given that set (``idx``) and one draw
(``pick``) shared by the batch and both directions.  Nothing here reads a value back to the host, so a training step with
the term can be captured in a hipGraph; every output is bitwise reproducible."""
import torch

from ._lib import check, f32c, get_lib, ptr, ptr_any, stream_ptr

MAX_NUM = 16384        # dfe_triangulate_stats stages ``num`` 8-byte keys in LDS


def topk_select(scores, k):
    """scores [planes, n] fp32 -> int32 [planes, k]: the indices of the k largest scores of each plane in ascending index
    order (torch.topk's order: NaN above +inf, -0 equal to +0; ties at the threshold go to the lower index)."""
    lib = get_lib()
    scores = f32c(scores.detach())
    planes, n = scores.shape
    k = int(k)
    idx = torch.empty(planes, k, device=scores.device, dtype=torch.int32)
    ws = torch.empty(max(lib.dfe_topk_ws_bytes(planes, n, k), 4) // 4, device=scores.device, dtype=torch.int32)
    check(lib.dfe_topk_select(ptr(scores), ptr(idx), ptr(ws), planes, n, k, stream_ptr()), "dfe_topk_select")
    return idx


class TriangulateFn(torch.autograd.Function):
    """(flow_bwd0, flow_fwd0 [B,2,H,W], disp_t0, disp_l0, disp_r0 [B,1,H,W], T34 [B,2,3,4], K, K_inv [B,3,3],
    idx int32 [2B,k] (planes: direction-major), pick int64 [num], align_corners) -> loss [B].  ``scale`` and ``a`` of
    register_depth are constants in the backward, as in the reference."""

    @staticmethod
    def forward(ctx, flow_bwd, flow_fwd, disp_t, disp_l, disp_r, T34, K, K_inv, idx, pick, align_corners):
        lib = get_lib()
        flow_bwd, flow_fwd, disp_t, disp_l, disp_r = (f32c(t) for t in (flow_bwd, flow_fwd, disp_t, disp_l, disp_r))
        T34, K, K_inv = f32c(T34), f32c(K), f32c(K_inv)
        B, _, H, W = flow_bwd.shape
        if tuple(flow_fwd.shape) != (B, 2, H, W) or any(tuple(d.shape) != (B, 1, H, W) for d in (disp_t, disp_l, disp_r)):
            raise ValueError("TriangulateFn: flows [B,2,H,W] and disparities [B,1,H,W] of one scale expected")
        if tuple(T34.shape) != (B, 2, 3, 4) or tuple(K.shape) != (B, 3, 3) or tuple(K_inv.shape) != (B, 3, 3):
            raise ValueError("TriangulateFn: T34 [B,2,3,4], K and K_inv [B,3,3] expected")
        if idx.dtype != torch.int32 or idx.dim() != 2 or idx.shape[0] != 2 * B or pick.dtype != torch.int64 or pick.dim() != 1:
            raise ValueError("TriangulateFn: idx int32 [2B,k] and pick int64 [num] expected")
        idx, pick = idx.contiguous(), pick.contiguous()
        k, num = idx.shape[1], pick.shape[0]
        dev = flow_bwd.device
        rec = torch.empty(2 * B * num, 4, device=dev, dtype=torch.float64)
        stats = torch.empty(B, 2, 2, 4, device=dev, dtype=torch.float64)
        loss = torch.empty(B, device=dev, dtype=torch.float32)
        ac = int(bool(align_corners))
        check(lib.dfe_triangulate_fwd(ptr_any(flow_bwd), ptr_any(flow_fwd), ptr_any(disp_t), ptr_any(disp_l), ptr_any(disp_r),
                                      ptr_any(T34), ptr_any(K), ptr_any(K_inv), ptr_any(idx), ptr_any(pick), ptr_any(rec),
                                      B, H, W, k, num, ac, stream_ptr()), "dfe_triangulate_fwd")
        check(lib.dfe_triangulate_stats(ptr_any(rec), ptr_any(stats), ptr_any(loss), B, num, stream_ptr()),
              "dfe_triangulate_stats")
        ctx.save_for_backward(flow_bwd, flow_fwd, disp_t, disp_l, disp_r, T34, K, K_inv, idx, pick, stats)
        ctx.ac = ac
        return loss

    @staticmethod
    def backward(ctx, gloss):
        lib = get_lib()
        flow_bwd, flow_fwd, disp_t, disp_l, disp_r, T34, K, K_inv, idx, pick, stats = ctx.saved_tensors
        B, _, H, W = flow_bwd.shape
        k, num = idx.shape[1], pick.shape[0]
        dev = flow_bwd.device
        gloss = f32c(gloss)
        grads = torch.empty(7 * B * H * W, device=dev, dtype=torch.float32)          # every element written by the library
        gT = torch.empty(B, 2, 3, 4, device=dev, dtype=torch.float32)
        ws = torch.empty(lib.dfe_triangulate_ws_bytes(B, H, W, num), device=dev, dtype=torch.uint8)
        check(lib.dfe_triangulate_bwd(ptr_any(flow_bwd), ptr_any(flow_fwd), ptr_any(disp_t), ptr_any(disp_l), ptr_any(disp_r),
                                      ptr_any(T34), ptr_any(K), ptr_any(K_inv), ptr_any(idx), ptr_any(pick), ptr_any(stats),
                                      ptr_any(gloss), ptr_any(grads), ptr_any(gT), ptr_any(ws), B, H, W, k, num, ctx.ac,
                                      stream_ptr()), "dfe_triangulate_bwd")
        n = B * H * W
        g_fb, g_ff = grads[:2 * n].view(B, 2, H, W), grads[2 * n:4 * n].view(B, 2, H, W)
        g_t, g_l, g_r = (grads[(4 + i) * n:(5 + i) * n].view(B, 1, H, W) for i in range(3))
        return g_fb, g_ff, g_t, g_l, g_r, gT, None, None, None, None, None


def triangulate_loss(flow_bwd, flow_fwd, disp_t, disp_l, disp_r, T34, K, K_inv, idx, pick, align_corners):
    if pick.shape[0] > MAX_NUM:
        raise ValueError("the triangulation term draws at most %d matches per sample and direction (got %d)" % (MAX_NUM, pick.shape[0]))
    return TriangulateFn.apply(flow_bwd, flow_fwd, disp_t, disp_l, disp_r, T34, K, K_inv, idx, pick, bool(align_corners))
