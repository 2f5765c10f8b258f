"""torch.autograd wrappers over the C ABI (include/dfe_hip.h).

Each Function is the device-side implementation of one reference free function; the
reference-signature shims live in ``structures/`` and ``pytorch_ssim``.  PyTorch supplies
device memory, the current HIP stream and the autograd graph -- the arithmetic is in
libdfe_hip.so.  There is no CPU fallback: CPU tensors raise ``DfeError``."""
from __future__ import annotations

import ctypes
import os
import threading

import torch

from . import _lib
from ._lib import DfeError, check, f32c, get_lib, ptr, stream_ptr

_ALIGN_CORNERS = False


def set_align_corners(flag: bool):
    """grid_sample convention used by every warp (the reference leaves it to the installed torch;
    False = torch>=1.3 default = what the golden vectors of this container use)."""
    global _ALIGN_CORNERS
    _ALIGN_CORNERS = bool(flag)


def get_align_corners() -> bool:
    return _ALIGN_CORNERS


def _ac(flag):
    return int(_ALIGN_CORNERS if flag is None else bool(flag))


def scatter_ws(n, device):
    """Workspace of the order-independent scatter-add into ``n`` floats (csrc/dfe_scatter.h; zero-filled by the library)."""
    return torch.empty(get_lib().dfe_scatter_ws_bytes(int(n)), device=device, dtype=torch.uint8)


def _dense_chw(t):
    """fp32 [B,C,H,W] whose samples are dense C x H x W planes, a batch stride of at least C*H*W floats apart: a contiguous
    tensor or a channel slice of a wider one (the gradient of a torch.cat).  The entry points that take a batch stride read
    such a view in place (``ptr(t, strided=True)``, ``t.stride(0)``); anything else goes through ``f32c`` first."""
    _, C, H, W = t.shape
    return (t.dtype == torch.float32 and t.stride(3) == 1 and t.stride(2) == W and t.stride(1) == H * W
            and t.stride(0) >= C * H * W)


def _chan_ptr(t, off):
    """Device pointer of channel ``off`` of sample 0 of an fp32 tensor with dense planes (None -> NULL): with ``t.stride(0)``
    as the batch stride, the channel slice ``t[:, off:]``."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr() + 4 * int(off) * t.shape[2] * t.shape[3])


# --------------------------------------------------------------------------- cameras
def prepare_cameras(pose, K, downscales):
    """pose [B,ndir,6] or [B,6], K [B,3,3] -> opaque camera buffer [B*ndir*len(downscales), 66]."""
    lib = get_lib()
    pose = f32c(pose.detach())
    if pose.dim() == 2:
        pose = pose.unsqueeze(1)
    B, ndir = pose.shape[0], pose.shape[1]
    K = f32c(K.detach())
    n = len(downscales)
    cams = torch.empty(B * ndir * n, lib.dfe_camera_floats(), device=pose.device, dtype=torch.float32)
    ds = (ctypes.c_float * n)(*[float(d) for d in downscales])
    check(lib.dfe_prepare_cameras(ptr(pose), ptr(K), ptr(cams), B, ndir, n, ctypes.cast(ds, ctypes.c_void_p),
                                  stream_ptr()), "dfe_prepare_cameras")
    return cams


# --------------------------------------------------------------------------- warp_flow
class WarpFlowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flow, use_mask, align_corners):
        lib = get_lib()
        x, flow = f32c(x), f32c(flow)
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        check(lib.dfe_warp_flow_fwd(ptr(x), ptr(flow), ptr(out), B, C, H, W, int(use_mask), align_corners,
                                    stream_ptr()), "dfe_warp_flow_fwd")
        ctx.save_for_backward(x, flow)
        ctx.cfg = (int(use_mask), align_corners)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = get_lib()
        x, flow = ctx.saved_tensors
        use_mask, ac = ctx.cfg
        B, C, H, W = x.shape
        gout = f32c(gout)
        gflow = torch.empty_like(flow) if ctx.needs_input_grad[1] else None
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None         # every element written by the library
        if gflow is None and gx is None:
            return None, None, None, None
        ws = scatter_ws(x.numel(), x.device) if gx is not None else None
        check(lib.dfe_warp_flow_bwd(ptr(x), ptr(flow), ptr(gout), ptr(gflow), ptr(gx), ptr(ws), B, C, H, W, use_mask, ac,
                                    stream_ptr()), "dfe_warp_flow_bwd")
        return gx, gflow, None, None


def warp_flow(x, flow, use_mask=False, align_corners=None):
    B, C, H, W = x.size()
    if tuple(flow.shape) != (B, 2, H, W):
        raise ValueError("the shape of grid {0} is not equal to the shape of flow {1}.".format(
            torch.Size((B, 2, H, W)), flow.shape))
    return WarpFlowFn.apply(x, flow, bool(use_mask), _ac(align_corners))


# --------------------------------------------------------------------------- pose matrices
class PoseMatsFn(torch.autograd.Function):
    """vec [n,6] -> (T34 [n,3,4], E [n,3,3])."""

    @staticmethod
    def forward(ctx, vec):
        lib = get_lib()
        vec = f32c(vec)
        n = vec.shape[0]
        T = torch.empty(n, 3, 4, device=vec.device, dtype=torch.float32)
        E = torch.empty(n, 3, 3, device=vec.device, dtype=torch.float32)
        check(lib.dfe_pose_vec2mat_fwd(ptr(vec), ptr(T), ptr(E), n, stream_ptr()), "dfe_pose_vec2mat_fwd")
        ctx.save_for_backward(vec)
        return T, E

    @staticmethod
    def backward(ctx, gT, gE):
        lib = get_lib()
        (vec,) = ctx.saved_tensors
        gvec = torch.empty_like(vec)
        gT = f32c(gT) if gT is not None else None
        gE = f32c(gE) if gE is not None else None
        check(lib.dfe_pose_vec2mat_bwd(ptr(vec), ptr(gT), ptr(gE), ptr(gvec), vec.shape[0], stream_ptr()),
              "dfe_pose_vec2mat_bwd")
        return gvec


# --------------------------------------------------------------------------- inverse_warp2
class InverseWarp2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, depth, ref_depth, pose, intrinsics, align_corners):
        lib = get_lib()
        img, depth, ref_depth = f32c(img), f32c(depth), f32c(ref_depth)
        pose, intrinsics = f32c(pose), f32c(intrinsics)
        B, _, H, W = img.shape
        cams = prepare_cameras(pose, intrinsics, [1.0])
        dev = img.device
        o_img = torch.empty(B, 3, H, W, device=dev)
        o_valid = torch.empty(B, 1, H, W, device=dev)
        o_pd = torch.empty(B, 1, H, W, device=dev)
        o_cd = torch.empty(B, 1, H, W, device=dev)
        check(lib.dfe_inverse_warp2_fwd(ptr(img), ptr(depth), ptr(ref_depth), ptr(cams), ptr(o_img), ptr(o_valid),
                                        ptr(o_pd), ptr(o_cd), B, H, W, align_corners, stream_ptr()),
              "dfe_inverse_warp2_fwd")
        ctx.save_for_backward(img, depth, ref_depth, cams)
        ctx.ac = align_corners
        ctx.mark_non_differentiable(o_valid)
        return o_img, o_valid, o_pd, o_cd

    @staticmethod
    def backward(ctx, g_img, g_valid, g_pd, g_cd):
        lib = get_lib()
        img, depth, ref_depth, cams = ctx.saved_tensors
        B, _, H, W = img.shape
        dev = img.device
        if ctx.needs_input_grad[0]:
            raise _lib.DfeError("gradient wrt the source image of inverse_warp2 is not implemented "
                                "(images are inputs on the reference's path)")
        g_img = f32c(g_img) if g_img is not None else None
        g_pd = f32c(g_pd) if g_pd is not None else None
        g_cd = f32c(g_cd) if g_cd is not None else None
        g_depth = torch.empty(B, 1, H, W, device=dev)
        g_ref = torch.empty(B, 1, H, W, device=dev) if (ctx.needs_input_grad[2] and g_pd is not None) else None
        g_ref_ws = scatter_ws(B * H * W, dev) if g_ref is not None else None
        g_pose = torch.empty(B, 6, device=dev)
        ws = torch.empty(lib.dfe_pose_partials_floats(B, H, W), device=dev)
        check(lib.dfe_inverse_warp2_bwd(ptr(img), ptr(depth), ptr(ref_depth), ptr(cams), ptr(g_img), ptr(g_pd),
                                        ptr(g_cd), ptr(g_depth), ptr(g_ref), ptr(g_ref_ws), ptr(g_pose), ptr(ws), B, H, W,
                                        ctx.ac, stream_ptr()), "dfe_inverse_warp2_bwd")
        return None, g_depth, g_ref, g_pose, None, None


# --------------------------------------------------------------------------- rigid flow
class RigidFlowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, pose, intrinsics):
        lib = get_lib()
        depth, pose, intrinsics = f32c(depth), f32c(pose), f32c(intrinsics)
        B, _, H, W = depth.shape
        cams = prepare_cameras(pose, intrinsics, [1.0])
        out = torch.empty(B, 2, H, W, device=depth.device)
        check(lib.dfe_rigid_flow_fwd(ptr(depth), ptr(cams), ptr(out), B, H, W, stream_ptr()), "dfe_rigid_flow_fwd")
        ctx.save_for_backward(depth, cams)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = get_lib()
        depth, cams = ctx.saved_tensors
        B, _, H, W = depth.shape
        g_depth = torch.empty_like(depth)
        g_pose = torch.empty(B, 6, device=depth.device)
        ws = torch.empty(lib.dfe_pose_partials_floats(B, H, W), device=depth.device)
        check(lib.dfe_rigid_flow_bwd(ptr(depth), ptr(cams), ptr(f32c(gout)), ptr(g_depth), ptr(g_pose), ptr(ws),
                                     B, H, W, stream_ptr()), "dfe_rigid_flow_bwd")
        return g_depth, g_pose, None


# --------------------------------------------------------------------------- SSIM
class SSIMFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        lib = get_lib()
        x, y = f32c(x), f32c(y)
        B, C, H, W = x.shape
        out = torch.empty_like(x)
        check(lib.dfe_ssim_fwd(ptr(x), ptr(y), ptr(out), B, C, H, W, stream_ptr()), "dfe_ssim_fwd")
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = get_lib()
        x, y = ctx.saved_tensors
        B, C, H, W = x.shape
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        if gx is None and gy is None:
            return None, None
        check(lib.dfe_ssim_bwd(ptr(x), ptr(y), ptr(f32c(gout)), ptr(gx), ptr(gy), B, C, H, W, stream_ptr()),
              "dfe_ssim_bwd")
        return gx, gy


# --------------------------------------------------------------------------- correlation
class CorrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f1, f2, d):
        lib = get_lib()
        f1, f2 = f32c(f1), f32c(f2)
        B, C, H, W = f1.shape
        out = torch.empty(B, (2 * d + 1) ** 2, H, W, device=f1.device)
        check(lib.dfe_corr_fwd(ptr(f1), ptr(f2), ptr(out), B, C, H, W, d, stream_ptr()), "dfe_corr_fwd")
        ctx.save_for_backward(f1, f2)
        ctx.d = d
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = get_lib()
        f1, f2 = ctx.saved_tensors
        B, C, H, W = f1.shape
        g1 = torch.empty_like(f1) if ctx.needs_input_grad[0] else None
        g2 = torch.empty_like(f2) if ctx.needs_input_grad[1] else None
        if g1 is None and g2 is None:
            return None, None, None
        check(lib.dfe_corr_bwd(ptr(f1), ptr(f2), ptr(f32c(gout)), ptr(g1), ptr(g2), B, C, H, W, ctx.d, stream_ptr()),
              "dfe_corr_bwd")
        return g1, g2, None


def corr81(f1, f2, d=4):
    assert f1.shape == f2.shape
    if d != 4:
        raise _lib.DfeError("corr_naive: only d=4 (81 taps) is implemented in HIP")
    return CorrFn.apply(f1, f2, int(d))


class MaxPool3x3s2Fn(torch.autograd.Function):
    """F.max_pool2d(x, 3, 2, 1) (the ResNet stem, depth_model.py:60-95) with a 1-byte window position instead of
    int64 indices; values and gradients bit-identical to ATen's."""

    @staticmethod
    def forward(ctx, x):
        lib = get_lib()
        x = f32c(x)
        B, C, H, W = x.shape
        Ho, Wo = lib.dfe_maxpool3x3s2_out(H), lib.dfe_maxpool3x3s2_out(W)
        y = torch.empty(B, C, Ho, Wo, device=x.device, dtype=torch.float32)
        idx = torch.empty(B, C, Ho, Wo, device=x.device, dtype=torch.uint8)
        check(lib.dfe_maxpool3x3s2_fwd(ptr(x), ptr(y), ptr(idx), B * C, H, W, stream_ptr()), "dfe_maxpool3x3s2_fwd")
        ctx.save_for_backward(idx)
        ctx.hw = (H, W)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = get_lib()
        idx, = ctx.saved_tensors
        B, C = idx.shape[:2]
        H, W = ctx.hw
        gx = torch.empty(B, C, H, W, device=gy.device, dtype=torch.float32)
        check(lib.dfe_maxpool3x3s2_bwd(ptr(f32c(gy)), ptr(idx), ptr(gx), B * C, H, W, stream_ptr()), "dfe_maxpool3x3s2_bwd")
        return gx


def maxpool3x3s2(x):
    if x.dim() != 4:
        raise ValueError("maxpool3x3s2: x must be [B,C,H,W]")
    if x.shape[0] * x.shape[1] > 65535:
        raise _lib.DfeError("maxpool3x3s2: more than 65535 planes")
    return MaxPool3x3s2Fn.apply(x)


PWC_LEVEL_MAP = os.environ.get("DFE_PWC_LEVEL_MAP", "1") != "0"      # the PWC level's inverse map built in its forward pass (PwcLevelInputFn)


class PwcLevelInputFn(torch.autograd.Function):
    """x = cat(corr(c1, warp(c2, flow)), c1, flow) of one PWC decoder level (pwc_tf.py:119-121) as one operator."""

    @staticmethod
    def forward(ctx, c1, c2, flow, align_corners):
        lib = get_lib()
        c1, c2, flow = f32c(c1), f32c(c2), f32c(flow)
        B, C, H, W = c1.shape
        warped = torch.empty_like(c2)
        x = torch.empty(B, lib.dfe_pwc_level_channels(C), H, W, device=c1.device, dtype=torch.float32)
        # when dL/dc2 will be asked for, the feature warp also counts its taps per target pixel and the inverse map the backward's
        # gather walks is finished here (dfe_pwc_level_fwd_map): the backward pass is then three launches at every level
        ctx.map = None
        if PWC_LEVEL_MAP and ctx.needs_input_grad[1] and C >= 8:
            ctx.map = torch.empty(lib.dfe_pwc_level_map_bytes(B, H, W), device=c1.device, dtype=torch.uint8)
            check(lib.dfe_pwc_level_fwd_map(ptr(c1), ptr(c2), ptr(flow), ptr(warped), ptr(x), ptr(ctx.map), B, C, H, W, align_corners,
                                            stream_ptr()), "dfe_pwc_level_fwd_map")
        else:
            check(lib.dfe_pwc_level_fwd(ptr(c1), ptr(c2), ptr(flow), ptr(warped), ptr(x), B, C, H, W, align_corners,
                                        stream_ptr()), "dfe_pwc_level_fwd")
        ctx.save_for_backward(c1, c2, flow, warped)
        ctx.ac = align_corners
        return x

    @staticmethod
    def backward(ctx, gx):
        lib = get_lib()
        c1, c2, flow, warped = ctx.saved_tensors
        B, C, H, W = c1.shape
        gx = f32c(gx)
        g_c1 = torch.empty_like(c1)
        g_c2 = torch.empty_like(c2) if ctx.needs_input_grad[1] else None    # every element written by the library
        g_flow = torch.empty_like(flow) if (ctx.needs_input_grad[2] or g_c2 is None) else None
        g_warped = torch.empty_like(c2)
        if ctx.map is not None and g_c2 is not None:
            check(lib.dfe_pwc_level_bwd_map(ptr(c1), ptr(c2), ptr(flow), ptr(warped), ptr(gx), ptr(g_warped), ptr(g_c1),
                                            ptr(g_c2), ptr(ctx.map), ptr(g_flow), B, C, H, W, ctx.ac, stream_ptr()), "dfe_pwc_level_bwd_map")
        else:
            ws = scatter_ws(c2.numel(), c2.device) if g_c2 is not None else None
            check(lib.dfe_pwc_level_bwd(ptr(c1), ptr(c2), ptr(flow), ptr(warped), ptr(gx), ptr(g_warped), ptr(g_c1),
                                        ptr(g_c2), ptr(ws), ptr(g_flow), B, C, H, W, ctx.ac, stream_ptr()), "dfe_pwc_level_bwd")
        return g_c1, g_c2, (g_flow if ctx.needs_input_grad[2] else None), None


def pwc_level_input(c1, c2, flow, align_corners=None):
    """``torch.cat((corr(c1, warp(c2, flow)), c1, flow), 1)`` [B, 81+C+2, H, W]."""
    if c1.shape != c2.shape or tuple(flow.shape) != (c1.shape[0], 2, c1.shape[2], c1.shape[3]):
        raise ValueError("pwc_level_input: c1 %s, c2 %s, flow %s" % (tuple(c1.shape), tuple(c2.shape), tuple(flow.shape)))
    return PwcLevelInputFn.apply(c1, c2, flow, _ac(align_corners))


# --------------------------------------------------------------------------- resize (no grad)
def resize(img, out_hw, mode):
    """mode 'bilinear' (align_corners=False) or 'area'; images carry no gradient on this path."""
    lib = get_lib()
    img = f32c(img.detach())
    B, C, H, W = img.shape
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty(B, C, oh, ow, device=img.device)
    check(lib.dfe_resize(ptr(img), ptr(out), B * C, H, W, oh, ow, {"bilinear": 0, "area": 1}[mode], stream_ptr()),
          "dfe_resize")
    return out


# --------------------------------------------------------------------------- device-side input pipeline
class ResizeBilinearFn(torch.autograd.Function):
    """F.interpolate(x, size, mode='bilinear', align_corners=False) with a scalar on one side of it, as PWC_tf writes
    it (pwc_tf.py:118-119, 175-178): ``pre`` -> resize(x * mult), else resize(x) * mult.  Forward in ATen's (CPU)
    association, backward as a gather (reproducible)."""

    @staticmethod
    def forward(ctx, x, out_hw, mult, pre):
        lib = get_lib()
        x = f32c(x)
        B, C, H, W = x.shape
        oh, ow = int(out_hw[0]), int(out_hw[1])
        out = torch.empty(B, C, oh, ow, device=x.device, dtype=torch.float32)
        check(lib.dfe_resize_bilinear_fwd(ptr(x), ptr(out), B * C, H, W, oh, ow, float(mult), int(pre), stream_ptr()),
              "dfe_resize_bilinear_fwd")
        ctx.cfg = (B, C, H, W, oh, ow, float(mult), int(pre))
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = get_lib()
        B, C, H, W, oh, ow, mult, pre = ctx.cfg
        gin = torch.empty(B, C, H, W, device=gout.device, dtype=torch.float32)
        check(lib.dfe_resize_bilinear_bwd(ptr(f32c(gout)), ptr(gin), B * C, H, W, oh, ow, mult, pre, stream_ptr()),
              "dfe_resize_bilinear_bwd")
        return gin, None, None, None


def resize_bilinear(x, out_hw, mult=1.0, pre=False):
    """Differentiable ``F.interpolate(x * mult if pre else x, out_hw, mode='bilinear') * (1 if pre else mult)``;
    up-sampling ratios of at most 4 per axis (DfeError beyond that in the backward pass)."""
    return ResizeBilinearFn.apply(x, (int(out_hw[0]), int(out_hw[1])), float(mult), bool(pre))


def prepare_triplets(raw_u8, img_hw, flip=None):
    """KITTI_Prepared.__getitem__'s image half (kitti_prepared.py:63-90,132-152) for a whole batch on the device.

    raw_u8: uint8 [B, 3*H0, W0, 3] stacked triplets as stored (pin + ``.to(device, non_blocking=True)`` it); flip: optional
    uint8 / bool [B]; returns fp32 [B, 3, 3*H, W] in [0,1] -- the ``images`` entry of the models' ``inputs``."""
    lib = get_lib()
    if raw_u8.dtype != torch.uint8 or raw_u8.dim() != 4 or raw_u8.shape[3] != 3 or raw_u8.shape[1] % 3:
        raise ValueError("raw_u8 must be uint8 [B, 3*H0, W0, 3]")
    raw_u8 = raw_u8.contiguous()
    B, H0, W0 = raw_u8.shape[0], raw_u8.shape[1] // 3, raw_u8.shape[2]
    H, W = int(img_hw[0]), int(img_hw[1])
    fl = None if flip is None else flip.to(device=raw_u8.device, dtype=torch.uint8).contiguous()
    out = torch.empty(B, 3, 3 * H, W, device=raw_u8.device)
    check(lib.dfe_prepare_triplets(ptr(raw_u8), ptr(fl), ptr(out), B, H0, W0, H, W, stream_ptr()), "dfe_prepare_triplets")
    return out


def _cv_linear_axis(n_out, n_in, clamp):
    """OpenCV 4.1.1 resize.cpp's coordinate set-up for INTER_LINEAR on 8-bit data along one axis: ``scale = 1. / ((double)
    n_out / n_in)``, ``f = (float)((d + 0.5) * scale - 0.5)``, ``s = cvFloor(f)``, ``f -= s`` (float), the x axis clamped
    (``s < 0 -> f = 0, s = 0``; ``s >= n_in - 1 -> f = 0, s = n_in - 1``), the y axis not; coefficients
    ``saturate_cast<short>((1.f - f) * 2048)`` and ``saturate_cast<short>(f * 2048)`` (round half to even).  float32 where
    OpenCV computes in float, float64 where it computes in double; numpy contracts nothing into an FMA."""
    import numpy as np
    scale = 1.0 / (float(n_out) / float(n_in))
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    if clamp:
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= n_in - 1
        f[hi], s[hi] = 0, n_in - 1
    c0 = np.rint((np.float32(1.0) - f) * np.float32(2048)).astype(np.int64)
    c1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return s, c0, c1


def resize_u8_tables(h0, w0, h, w):
    """Host tables of ``dfe_prepare_triplets_u8`` for a (h0, w0) -> (h, w) frame: int32 xtab [w, 2] = (x0, a0 | a1 << 16) and
    ytab [h, 4] = (y0, y1, b0 | b1 << 16, 0).  Same size: cv::resize copies (x0 = dx, a = (2048, 0): both vertical rules
    return the byte).  Exact 1/2 on both axes: cv::hal::resize switches to INTER_AREA, (a + b + c + d + 2) >> 2 (a = b =
    (1024, 1024) on the pixel pairs: both vertical rules reduce to it exactly).  Otherwise INTER_LINEAR (_cv_linear_axis)."""
    import numpy as np
    h0, w0, h, w = int(h0), int(w0), int(h), int(w)
    xt, yt = np.zeros((w, 2), np.int32), np.zeros((h, 4), np.int32)
    if (h0, w0) == (h, w):
        xs, ys = np.arange(w), np.arange(h)
        xt[:, 0], xt[:, 1] = xs, 2048
        yt[:, 0], yt[:, 1], yt[:, 2] = ys, ys, 2048
    elif w0 == 2 * w and h0 == 2 * h:
        xt[:, 0], xt[:, 1] = 2 * np.arange(w), 1024 | (1024 << 16)
        yt[:, 0], yt[:, 1], yt[:, 2] = 2 * np.arange(h), 2 * np.arange(h) + 1, 1024 | (1024 << 16)
    else:
        sx, a0, a1 = _cv_linear_axis(w, w0, True)
        sy, b0, b1 = _cv_linear_axis(h, h0, False)
        xt[:, 0], xt[:, 1] = sx, a0 | (a1 << 16)
        yt[:, 0], yt[:, 1], yt[:, 2] = np.clip(sy, 0, h0 - 1), np.clip(sy + 1, 0, h0 - 1), b0 | (b1 << 16)
    return xt, yt


def resize_u8_vector_bytes(w):
    """Bytes of a resized 3-channel row of width w that VResizeLinearVec_32s8u covers: 16 * floor(n / 16) of n = 3w, plus 8 when
    more than 8 remain; the rest take VResizeLinear's scalar rule.  This split is a reading of OpenCV 4.1.1, not pinned
    against cv2; at the training width 832 (2496 bytes) the whole row is vector."""
    n = 3 * int(w)
    v = 16 * (n // 16)
    return v + 8 if n - v > 8 else v


class _U8Tables:
    """Device copy of every (h0, w0, h, w) table set seen so far, concatenated (one xtab, one ytab), plus the 256-entry lut.  A new
    size re-uploads the concatenation; the superseded tensors are kept (a few KB each) because a launch still in flight on another
    stream may read them."""

    def __init__(self):
        self.lock = threading.Lock()
        self.keys, self.host_x, self.host_y = {}, [], []
        self.dev = {}          # device index -> (xtab, ytab, lut, number of keys uploaded)
        self.retired = []

    def get(self, keys, device):
        """([(xtab, ytab) first entry per key], xtab, ytab, lut) on ``device``, uploading new keys' tables first."""
        import numpy as np
        with self.lock:
            for k in keys:
                if k not in self.keys:
                    xt, yt = resize_u8_tables(*k)
                    self.keys[k] = (sum(len(a) for a in self.host_x), sum(len(a) for a in self.host_y))
                    self.host_x.append(xt)
                    self.host_y.append(yt)
            cur = self.dev.get(device.index)
            if cur is None or cur[3] != len(self.keys):
                if cur is not None:
                    self.retired.append(cur)
                lut = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
                # blocking uploads: complete before any stream reads them
                self.dev[device.index] = cur = (torch.from_numpy(np.concatenate(self.host_x)).to(device),
                                                torch.from_numpy(np.concatenate(self.host_y)).to(device),
                                                torch.from_numpy(lut).to(device), len(self.keys))
            return [self.keys[k] for k in keys], cur[0], cur[1], cur[2]


_u8_tables = _U8Tables()
# dfe_u8_desc (include/dfe_hip.h), 32 bytes
U8_DESC = [("offset", "<i8"), ("h0", "<i4"), ("w0", "<i4"), ("xtab", "<i4"), ("ytab", "<i4"), ("flip", "<i4"), ("pad", "<i4")]


def prepare_triplets_u8(raw_u8, sizes, img_hw, flip=None, offsets=None, rgb=False):
    """KITTI_Prepared.__getitem__'s image half (kitti_prepared.py:63-90,132-152) in the reference's 8-bit arithmetic
    (dfe_prepare_triplets_u8: cv2.resize INTER_LINEAR on uint8 as OpenCV 4.1.1 computes it, cv2.flip, / 255.0) for a batch of
    stacked triplets that may each have their own raw size.

    raw_u8: uint8 device tensor holding sample b's strip [3*h0_b, w0_b, 3] at byte ``offsets[b]`` (a [B, 3*H0, W0, 3] tensor
    with ``offsets`` None is the uniform case); sizes: B (h0, w0) frame sizes (the strip's rows are 3*h0); flip: B host values
    (non-zero = cv2.flip(img, 1)); rgb: the bytes are R, G, B (a PIL decode) and are written in cv2.imread's B, G, R order.
    Returns a fresh fp32 [B, 3, 3*H, W] tensor (the models' ``images``) whose values are float32(u / 255.0) for the bytes u cv2
    would produce."""
    import numpy as np
    if not isinstance(raw_u8, torch.Tensor) or not raw_u8.is_cuda:
        raise DfeError("prepare_triplets_u8 takes a uint8 tensor on a HIP device; there is no CPU fallback in the product path")
    lib = get_lib()
    if raw_u8.dtype != torch.uint8 or not raw_u8.is_contiguous():
        raise ValueError("raw_u8 must be a contiguous uint8 tensor")
    sizes = [(int(a), int(b)) for a, b in sizes]
    B = len(sizes)
    H, W = int(img_hw[0]), int(img_hw[1])
    if B == 0 or H <= 0 or W <= 0 or any(a <= 0 or b <= 0 for a, b in sizes):
        raise ValueError("prepare_triplets_u8: empty batch or a non-positive size")
    nbytes = [9 * a * b for a, b in sizes]
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).tolist()
    offsets = [int(o) for o in offsets]
    if len(offsets) != B or any(o < 0 or o + n > raw_u8.numel() for o, n in zip(offsets, nbytes)):
        raise ValueError("prepare_triplets_u8: a strip lies outside raw_u8 (%d bytes)" % raw_u8.numel())
    fl = [0] * B if flip is None else [int(v) for v in (flip.tolist() if isinstance(flip, torch.Tensor) else flip)]
    if len(fl) != B:
        raise ValueError("prepare_triplets_u8: flip must have one entry per sample")
    index, xtab, ytab, lut = _u8_tables.get([(a, b, H, W) for a, b in sizes], raw_u8.device)
    desc = np.zeros(B, U8_DESC)
    desc["offset"], desc["flip"] = offsets, [1 if v else 0 for v in fl]
    desc["h0"], desc["w0"] = [a for a, _ in sizes], [b for _, b in sizes]
    desc["xtab"], desc["ytab"] = [i[0] for i in index], [i[1] for i in index]
    # pinned staging (torch's caching host allocator keeps the block until the copy has run): no host sync behind the stream
    d_desc = torch.from_numpy(desc.view(np.uint8)).pin_memory().to(raw_u8.device, non_blocking=True)
    return prepare_triplets_u8_desc(raw_u8, d_desc, B, (H, W), (xtab, ytab, lut), rgb)


def prepare_triplets_u8_desc(raw_u8, desc_u8, B, img_hw, tables, rgb=False):
    """The launch under ``prepare_triplets_u8`` for a caller that built the B ``U8_DESC`` descriptors itself (``u8_tables`` gives the
    table offsets) and placed them in device memory: prepared_data.PreparedFeeder uploads them with the strips in one copy.  The
    caller guarantees every descriptor's strip lies inside raw_u8 and its table offsets come from ``tables``."""
    H, W = int(img_hw[0]), int(img_hw[1])
    xtab, ytab, lut = tables
    out = torch.empty(B, 3, 3 * H, W, device=raw_u8.device)
    check(get_lib().dfe_prepare_triplets_u8(ptr(raw_u8), ptr(desc_u8), ptr(xtab), ptr(ytab), ptr(lut), ptr(out), B, H, W,
                                            resize_u8_vector_bytes(W), 1 if rgb else 0, stream_ptr()), "dfe_prepare_triplets_u8")
    return out


def u8_tables(sizes, img_hw, device):
    """Device tables for frames of ``sizes`` [(h0, w0)] resized to img_hw: ({(h0, w0): (xtab, ytab) first entries}, (xtab, ytab,
    lut)), uploaded once per size and kept."""
    H, W = int(img_hw[0]), int(img_hw[1])
    sizes = sorted(set((int(a), int(b)) for a, b in sizes))
    index, xtab, ytab, lut = _u8_tables.get([(a, b, H, W) for a, b in sizes], torch.device(device))
    return dict(zip(sizes, index)), (xtab, ytab, lut)


def _need(t, what, dtype, contiguous=True):
    """A HIP tensor of ``dtype`` (DfeError for a host tensor, ValueError for the rest), before the library is called."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise DfeError("%s must be a tensor on a HIP device; there is no CPU fallback in the product path" % what)
    if t.dtype != dtype:
        raise ValueError("%s must be %s, not %s" % (what, dtype, t.dtype))
    if contiguous and not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    return t


def resize_strips_u8(raw_u8, sizes, img_hw, slot, store, offsets=None, rgb=False):
    """The resized 8-bit frames of ``prepare_triplets_u8``'s strips, kept (dfe_resize_strips_u8: the same device code up to the byte,
    so ``lut[store]`` is what prepare_triplets_u8 returns unflipped).

    raw_u8, sizes, offsets, rgb: as for ``prepare_triplets_u8``.  slot: B x 3 host integers, the frame of ``store`` (uint8 device
    tensor [F, 3 (B,G,R), H, W], written in place) that (strip b, frame f) goes to; -1 = do not write.  Values outside [-1, F)
    are refused here, before the library is called."""
    import numpy as np
    _need(raw_u8, "raw_u8", torch.uint8)
    H, W = int(img_hw[0]), int(img_hw[1])
    _need(store, "store", torch.uint8)
    if store.device != raw_u8.device or store.dim() != 4 or tuple(store.shape[1:]) != (3, H, W) or store.shape[0] < 1:
        raise ValueError("store must be uint8 [F, 3, %d, %d] on raw_u8's device" % (H, W))
    sizes = [(int(a), int(b)) for a, b in sizes]
    B, F = len(sizes), int(store.shape[0])
    if B == 0 or H <= 0 or W <= 0 or any(a <= 0 or b <= 0 for a, b in sizes):
        raise ValueError("resize_strips_u8: empty batch or a non-positive size")
    nbytes = [9 * a * b for a, b in sizes]
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(nbytes)[:-1]]).tolist()
    offsets = [int(o) for o in offsets]
    if len(offsets) != B or any(o < 0 or o + n > raw_u8.numel() for o, n in zip(offsets, nbytes)):
        raise ValueError("resize_strips_u8: a strip lies outside raw_u8 (%d bytes)" % raw_u8.numel())
    slot = np.ascontiguousarray(np.asarray(slot, dtype=np.int64))
    if slot.shape != (B, 3) or bool(((slot < -1) | (slot >= F)).any()):
        raise ValueError("resize_strips_u8: slot must be [%d, 3] integers in [-1, %d)" % (B, F))
    index, xtab, ytab, _ = _u8_tables.get([(a, b, H, W) for a, b in sizes], raw_u8.device)
    desc = np.zeros(B, U8_DESC)
    desc["offset"] = offsets
    desc["h0"], desc["w0"] = [a for a, _ in sizes], [b for _, b in sizes]
    desc["xtab"], desc["ytab"] = [i[0] for i in index], [i[1] for i in index]
    d_desc = torch.from_numpy(desc.view(np.uint8)).to(raw_u8.device)     # blocking uploads: this is the build, not the step
    d_slot = torch.from_numpy(slot).to(raw_u8.device)
    check(get_lib().dfe_resize_strips_u8(ptr(raw_u8), ptr(d_desc), ptr(xtab), ptr(ytab), ptr(d_slot), ptr(store), F, B, H, W,
                                         resize_u8_vector_bytes(W), 1 if rgb else 0, stream_ptr()), "dfe_resize_strips_u8")
    return store


def gather_triplets_u8(set_tensors, idx, flip=None, out=None):
    """One training batch from a device-resident set in one launch on the current stream (dfe_gather_triplets_u8).

    set_tensors: (store uint8 [F,3,H,W], tri int32 [N,3], ktab fp32 [N,2,S,3,3], lut fp32 [256]) on one HIP device; idx: B host
    integers in [0, N) (the triplets); flip: B host values or None.  The indices and flips travel in the kernel's arguments: no
    staging buffer, no copy.  Returns [images fp32 [B,3,3H,W], K_ms [B,S,3,3], K_inv_ms [B,S,3,3]]: fresh tensors, or the three
    of ``out`` (contiguous fp32 of those shapes; how a replayed graph's static inputs are fed).  Everything is checked here,
    before the library is called."""
    store, tri, ktab, lut = set_tensors
    _need(store, "store", torch.uint8), _need(tri, "tri", torch.int32), _need(ktab, "ktab", torch.float32), _need(lut, "lut", torch.float32)
    if store.dim() != 4 or store.shape[1] != 3 or tri.dim() != 2 or tri.shape[1] != 3 or ktab.dim() != 5 or \
            tuple(ktab.shape[2:]) != (ktab.shape[2], 3, 3) or ktab.shape[:2] != (tri.shape[0], 2) or lut.numel() != 256:
        raise ValueError("gather_triplets_u8: set tensors must be store [F,3,H,W], tri [N,3], ktab [N,2,S,3,3], lut [256]")
    if any(t.device != store.device for t in (tri, ktab, lut)):
        raise ValueError("gather_triplets_u8: the set's tensors must live on one device")
    F, _, H, W = (int(v) for v in store.shape)
    N, S = int(tri.shape[0]), int(ktab.shape[2])
    idx = [int(i) for i in idx]
    B = len(idx)
    if B == 0 or F == 0 or N == 0:
        raise ValueError("gather_triplets_u8: empty batch or empty set")
    if any(i < 0 or i >= N for i in idx):
        raise ValueError("gather_triplets_u8: a triplet index lies outside [0, %d)" % N)
    c_flip = None
    if flip is not None:
        fl = [1 if v else 0 for v in (flip.tolist() if isinstance(flip, torch.Tensor) else flip)]
        if len(fl) != B:
            raise ValueError("gather_triplets_u8: flip must have one entry per sample")
        c_flip = (ctypes.c_ubyte * B)(*fl)
    shapes = ((B, 3, 3 * H, W), (B, S, 3, 3), (B, S, 3, 3))
    if out is None:
        out = [torch.empty(s, device=store.device) for s in shapes]
    else:
        out = list(out)
        if len(out) != 3:
            raise ValueError("gather_triplets_u8: out takes the three destination tensors")
        for t, s, name in zip(out, shapes, ("out[0] (images)", "out[1] (K_ms)", "out[2] (K_inv_ms)")):
            _need(t, name, torch.float32)
            if tuple(t.shape) != s or t.device != store.device:
                raise ValueError("gather_triplets_u8: %s must be %s on the set's device" % (name, list(s)))
    check(get_lib().dfe_gather_triplets_u8(ptr(store), F, ptr(tri), ptr(ktab), N, ptr(lut), (ctypes.c_int * B)(*idx), c_flip,
                                           ptr(out[0]), ptr(out[1]), ptr(out[2]), B, S, H, W, stream_ptr()), "dfe_gather_triplets_u8")
    return out


def rescale_intrinsics(K, img_hw_orig, img_hw_new, num_scales):
    """rescale_intrinsics + get_multiscale_intrinsics (kitti_prepared.py:110-130): K [3,3] float64 numpy ->
    (K_ms, K_inv_ms) float32 tensors [S,3,3] (host side: a few dozen flops per sample)."""
    import numpy as np
    K = np.array(K, dtype=np.float64, copy=True)
    K[0, :] = K[0, :] * img_hw_new[1] / img_hw_orig[1]
    K[1, :] = K[1, :] * img_hw_new[0] / img_hw_orig[0]
    ks, kis = [], []
    for s in range(num_scales):
        k = K.copy()
        k[0, :] /= 2 ** s
        k[1, :] /= 2 ** s
        ks.append(k); kis.append(np.linalg.inv(k))
    return torch.from_numpy(np.stack(ks)).float(), torch.from_numpy(np.stack(kis)).float()


# --------------------------------------------------------------------------- forward splat (no grad)
def forward_splat_ones(flow, clamp=True):
    """Bilinear forward warp of a ones image by ``flow`` [B,2,H,W] -> [B,1,H,W] (model_flow.py:33-39's intent)."""
    lib = get_lib()
    fl = f32c(flow.detach())
    B, C, H, W = fl.shape
    if C != 2:
        raise ValueError("flow must be [B,2,H,W]")
    out = torch.empty(B, 1, H, W, device=fl.device)
    ws = scatter_ws(B * H * W, fl.device)
    check(lib.dfe_forward_splat_ones(ptr(fl), ptr(out), ptr(ws), B, H, W, int(bool(clamp)), stream_ptr()),
          "dfe_forward_splat_ones")
    return out


# --------------------------------------------------------------------------- mask decisions (no grad)
def occ_masks(from_l, tgt, from_r):
    """compute_occ_weight's decisions (model_geometry.py:105-132) -> occ_bwd, occ_fwd, valid_bwd, valid_fwd [B,1,H,W]."""
    lib = get_lib()
    il, it, ir = (f32c(t.detach()) for t in (from_l, tgt, from_r))
    B, C, H, W = it.shape
    if C != 3 or il.shape != it.shape or ir.shape != it.shape:
        raise ValueError("occ_masks expects three [B,3,H,W] tensors")
    outs = [torch.empty(B, 1, H, W, device=it.device) for _ in range(4)]
    check(lib.dfe_occ_masks(ptr(il), ptr(it), ptr(ir), *[ptr(o) for o in outs], B, H, W, stream_ptr()), "dfe_occ_masks")
    return outs


def texture_mask(img, warped, source):
    """compute_texture_mask's decision (model_geometry.py:134-140) -> [B,1,H,W] in {0,1}."""
    lib = get_lib()
    a, b, c = (f32c(t.detach()) for t in (img, warped, source))
    B, C, H, W = a.shape
    if C != 3 or b.shape != a.shape or c.shape != a.shape:
        raise ValueError("texture_mask expects three [B,3,H,W] tensors")
    out = torch.empty(B, 1, H, W, device=a.device)
    check(lib.dfe_texture_mask(ptr(a), ptr(b), ptr(c), ptr(out), B, H, W, stream_ptr()), "dfe_texture_mask")
    return out


def dynamic_mask(flow, rigid, alpha, beta):
    """compute_dynamic_mask's decision and score (model_geometry.py:699-711) -> mask, score [B,1,H,W]."""
    lib = get_lib()
    f, r = f32c(flow.detach()), f32c(rigid.detach())
    B, C, H, W = f.shape
    if C != 2 or r.shape != f.shape:
        raise ValueError("dynamic_mask expects two [B,2,H,W] tensors")
    mask, score = torch.empty(B, 1, H, W, device=f.device), torch.empty(B, 1, H, W, device=f.device)
    check(lib.dfe_dynamic_mask(ptr(f), ptr(r), ptr(mask), ptr(score), float(alpha), float(beta), B, H, W, stream_ptr()),
          "dfe_dynamic_mask")
    return mask, score


# --------------------------------------------------------------------------- depth-decoder glue
class EluPadFn(torch.autograd.Function):
    """reflect_pad1(elu(x + bias)) (elu, bias optional): the input of a Conv3x3 whose producer is a ConvBlock
    (depth_model.py); x is that block's convolution output computed without its bias."""

    @staticmethod
    def forward(ctx, x, bias, apply_elu):
        lib = get_lib()
        x = f32c(x)
        bias = f32c(bias) if bias is not None else None
        B, C, H, W = x.shape
        out = torch.empty(B, C, H + 2, W + 2, device=x.device)
        check(lib.dfe_elu_pad_fwd(ptr(x), ptr(bias), ptr(out), B, C, H, W, int(apply_elu), stream_ptr()), "dfe_elu_pad_fwd")
        ctx.apply_elu = int(apply_elu)
        ctx.shape = (B, C, H, W)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x if apply_elu else x.new_empty(0), bias if bias is not None else x.new_empty(0))
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = get_lib()
        x, bias = ctx.saved_tensors
        B, C, H, W = ctx.shape
        gout = f32c(gout)
        gx = torch.empty(B, C, H, W, device=gout.device)
        gb = part = None
        if ctx.has_bias and ctx.needs_input_grad[1]:
            gb = torch.empty(C, device=gout.device)
            part = torch.empty(lib.dfe_glue_partials_floats(B, C, H, W), device=gout.device)
        check(lib.dfe_elu_pad_bwd(ptr(x) if ctx.apply_elu else None, ptr(bias) if ctx.has_bias else None, ptr(gout), ptr(gx),
                                  ptr(gb), ptr(part), B, C, H, W, ctx.apply_elu, stream_ptr()), "dfe_elu_pad_bwd")
        return gx, gb, None


class EluUp2CatPadFn(torch.autograd.Function):
    """reflect_pad1(cat(bilinear_x2(elu(x + bias)), skip)): one decoder stage's glue (depth_model.py: ELU, upsample,
    cat, pad); x is the stage's first convolution output computed without its bias."""

    @staticmethod
    def forward(ctx, x, bias, skip):
        lib = get_lib()
        x = f32c(x)
        bias = f32c(bias) if bias is not None else None
        B, C1, h, w = x.shape
        C2 = 0
        if skip is not None:
            skip = f32c(skip)
            C2 = skip.shape[1]
            if tuple(skip.shape) != (B, C2, 2 * h, 2 * w):
                raise ValueError("skip must be [B,C2,2h,2w] = %s, got %s" % ((B, C2, 2 * h, 2 * w), tuple(skip.shape)))
        out = torch.empty(B, C1 + C2, 2 * h + 2, 2 * w + 2, device=x.device)
        check(lib.dfe_elu_up2_cat_pad_fwd(ptr(x), ptr(bias), ptr(skip), ptr(out), B, C1, C2, h, w, stream_ptr()),
              "dfe_elu_up2_cat_pad_fwd")
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, bias if bias is not None else x.new_empty(0))
        ctx.dims = (B, C1, C2, h, w)
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = get_lib()
        x, bias = ctx.saved_tensors
        B, C1, C2, h, w = ctx.dims
        gout = f32c(gout)
        want_b = ctx.has_bias and ctx.needs_input_grad[1]
        gx = torch.empty_like(x) if (ctx.needs_input_grad[0] or want_b) else None
        gskip = torch.empty(B, C2, 2 * h, 2 * w, device=x.device) if (C2 > 0 and ctx.needs_input_grad[2]) else None
        if gx is None and gskip is None:
            return None, None, None
        gb = part = None
        if want_b:
            gb = torch.empty(C1, device=x.device)
            part = torch.empty(lib.dfe_glue_partials_floats(B, C1, h, w), device=x.device)
        check(lib.dfe_elu_up2_cat_pad_bwd(ptr(x), ptr(bias) if ctx.has_bias else None, ptr(gout), ptr(gx), ptr(gskip), ptr(gb),
                                          ptr(part), B, C1, C2, h, w, stream_ptr()), "dfe_elu_up2_cat_pad_bwd")
        return gx, gb, gskip


def elu_pad(x, bias=None, apply_elu=True):
    return EluPadFn.apply(x, bias, bool(apply_elu))


def elu_up2_cat_pad(x, bias=None, skip=None):
    return EluUp2CatPadFn.apply(x, bias, skip)


# --------------------------------------------------------------------------- convolution epilogue (bias + activation)
def _bias_act_bwd(y, gy, slope, want_bias):
    """(gz, gbias) of y = act(z + bias) on dfe_bias_act_bwd: gz = gy act'(y), gbias = its sum over (b,h,w) (None unless
    ``want_bias``).  ``gy`` is fp32 with dense planes (``_dense_chw``) and is read with its own batch stride."""
    lib = get_lib()
    B, C, H, W = y.shape
    gz = torch.empty_like(y)
    gb = part = None
    if want_bias:
        gb = torch.empty(C, device=y.device, dtype=torch.float32)
        part = torch.empty(lib.dfe_bias_act_partials_floats(B, C, H, W), device=y.device, dtype=torch.float32)
    check(lib.dfe_bias_act_bwd(ptr(y), ptr(gy, strided=True), gy.stride(0), ptr(gz), ptr(gb), ptr(part), B, C, H, W, slope,
                               stream_ptr()), "dfe_bias_act_bwd")
    return gz, gb


class BiasActFn(torch.autograd.Function):
    """z <- act(z + bias[c]) in place on a fresh convolution output; act(v) = v > 0 ? v : slope * v."""

    @staticmethod
    def forward(ctx, z, bias, slope):
        lib = get_lib()
        if not z.is_contiguous() or z.dtype != torch.float32:
            raise _lib.DfeError("bias_act expects a contiguous fp32 convolution output")
        B, C, H, W = z.shape
        b = f32c(bias) if bias is not None else None
        check(lib.dfe_bias_act_fwd(ptr(z), ptr(b), B, C, H, W, float(slope), stream_ptr()), "dfe_bias_act_fwd")
        ctx.mark_dirty(z)
        ctx.save_for_backward(z)
        ctx.slope = float(slope)
        ctx.has_bias = bias is not None
        return z

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        # a channel slice of a wider contiguous tensor (the gradient of a torch.cat) is read in place
        gz, gb = _bias_act_bwd(y, gy if _dense_chw(gy) else f32c(gy), ctx.slope, ctx.has_bias and ctx.needs_input_grad[1])
        return gz, gb, None


def bias_act(z, bias, slope):
    return BiasActFn.apply(z, bias, float(slope))


# --------------------------------------------------------------------------- small-plane 3x3 convolutions (fp32 MFMA)
def _planeconv_ws(B, Ci, Co, H, W, dev):
    return torch.empty(get_lib().dfe_planeconv_ws_floats(B, Ci, Co, H, W), device=dev, dtype=torch.float32)


def planeconv_fwd_into(x, w, bias, slope, d1, d1_off=0, d2=None, d2_off=0):
    """act(conv3x3(x, w) + bias) into channels d1_off.. of d1 and (optionally) d2_off.. of d2 (contiguous NCHW buffers)."""
    B, Ci, H, W = x.shape
    Co = int(w.shape[0])
    ws = _planeconv_ws(B, Ci, Co, H, W, x.device)
    check(get_lib().dfe_planeconv_fwd(ptr(x), ptr(w), ptr(bias), float(slope), _chan_ptr(d1, d1_off), d1.stride(0), _chan_ptr(d2, d2_off),
                                      d2.stride(0) if d2 is not None else 0, ptr(ws), B, Ci, Co, H, W, stream_ptr()),
          "dfe_planeconv_fwd")


def planeconv_forward(x, w, bias=None, slope=1.0):
    x, w = f32c(x), f32c(w)
    y = torch.empty(x.shape[0], w.shape[0], x.shape[2], x.shape[3], device=x.device, dtype=torch.float32)
    planeconv_fwd_into(x, w, None if bias is None else f32c(bias), slope, y)
    return y


def planeconv_backward(gy, x, w, want_x=True, want_w=True):
    """(gx, gw) of conv3x3(x, w), pad 1."""
    gy, x, w = f32c(gy), f32c(x), f32c(w)
    B, Ci, H, W = x.shape
    Co = int(w.shape[0])
    lib = get_lib()
    ws = _planeconv_ws(B, Ci, Co, H, W, x.device)
    gx = gw = None
    if want_x:
        gx = torch.empty_like(x)
        check(lib.dfe_planeconv_dgrad(ptr(gy), ptr(w), ptr(gx), ptr(ws), B, Ci, Co, H, W, stream_ptr()), "dfe_planeconv_dgrad")
    if want_w:
        gw = torch.empty_like(w)
        check(lib.dfe_planeconv_wgrad(ptr(gy), ptr(x), ptr(gw), ptr(ws), B, Ci, Co, H, W, stream_ptr()), "dfe_planeconv_wgrad")
    return gx, gw


# --------------------------------------------------------------------------- Winograd F(2x2, 3x3) on the fp32 matrix cores
class WinoWeightCache:
    """Transformed filters (U = G g G^T, both orientations) of the parameters the Winograd kernel has been called with, kept
    across steps.  A training step uses every filter twice (forward, data gradient) and each call used to launch its own
    transform (96 launches of ~5.6 us per step of the joint model); the filters only change in the optimiser step, so
    ``optim.FusedAdam.step`` calls ``refresh()``: ONE launch (dfe_wino_transform_weights_multi) on the optimiser's stream,
    right behind the update -- whatever orders the next step's network streams behind the update orders them behind this.

    Validity: an entry is used only while the parameter object it was made for is alive, still owns the same storage and its
    autograd version counter equals the one recorded at the refresh -- ``load_state_dict``, ``copy_`` or any other in-place
    torch operation makes the entry miss, and the call transforms for itself (into its own scratch, on its own stream) as
    before.  FusedAdam writes parameters through raw pointers (no version bump), which is why it is the one that refreshes.
    Only ``refresh`` writes the cached buffers.  ``DFE_WINO_CACHE=0`` turns the cache off."""

    def __init__(self):
        self.enabled = os.environ.get("DFE_WINO_CACHE", "1") != "0"
        # DFE_WINO_CACHE_VERIFY=1: every hit re-transforms the filter and compares (synchronises; a debugging mode that catches
        # writes the version counters cannot see)
        self.verify = os.environ.get("DFE_WINO_CACHE_VERIFY", "0") == "1"
        self.entries = {}        # (data_ptr, Co, Ci of the weight tensor) -> entry
        self.table = None        # device tables of the last refresh (rebuilt when the membership changes)
        self.blockmap = None
        self.members = None
        self.hits = self.misses = 0
        if os.environ.get("DFE_WINO_CACHE_STATS"):
            import atexit
            import sys
            atexit.register(lambda: sys.stderr.write("[dfe] wino weight cache: %d filters, %d hits, %d misses\n"
                                                     % (len(self.entries), self.hits, self.misses)))

    def lookup(self, w, transposed):
        """The cached U for this call or None (transform per call).  Registers the parameter on first sight."""
        if not self.enabled or not w.is_cuda or w.dim() != 4:
            return None
        key = (w.data_ptr(), int(w.shape[0]), int(w.shape[1]))
        e = self.entries.get(key)
        if e is None:
            # only leaf parameters are worth keeping (a temporary's address is reused by unrelated tensors)
            # (and only what refresh() can transform: a non-fp32 / non-contiguous parameter would be registered again on every call)
            if isinstance(w, torch.nn.Parameter) and w.dtype == torch.float32 and w.is_contiguous():
                import weakref
                self.entries[key] = {"ref": weakref.ref(w), "version": -1, "U": None, "device": w.device}
                self.members = None      # the device table of the last refresh no longer describes the membership
            self.misses += 1
            return None
        p = e["ref"]()
        if p is None or p.data_ptr() != key[0]:
            # the Parameter died (its address may already belong to another tensor -- or to a NEW Parameter of the same shape,
            # which would re-register under the same key: the table must be rebuilt, its U pointers are about to be freed)
            del self.entries[key]
            self.members = None
            self.misses += 1
            return None
        if e["U"] is None or e["version"] != w._version or e["version"] != p._version:
            self.misses += 1
            return None
        self.hits += 1
        U = e["U"][1 if transposed else 0]
        if self.verify and not torch.equal(U, self.transform_now(w, transposed)):
            raise _lib.DfeError("WinoWeightCache: the cached filters of a %s parameter are stale -- it was written without a version "
                                "bump (p.data.mul_/copy_, a raw-pointer kernel) after the last refresh; call "
                                "ops.wino_weights.invalidate() after such writes" % (tuple(w.shape),))
        return U

    @staticmethod
    def transform_now(w, transposed):
        """U of ``w`` by a one-entry launch of the same kernel refresh() uses (DFE_WINO_CACHE_VERIFY=1; tests)."""
        lib = get_lib()
        Co, Ci = int(w.shape[0]), int(w.shape[1])
        K, C = (Ci, Co) if transposed else (Co, Ci)
        U = torch.empty(lib.dfe_wino_weight_floats(C, K), device=w.device, dtype=torch.float32)
        n = int(lib.dfe_wino_transform_blocks(C, K))
        table = torch.tensor([[w.data_ptr(), U.data_ptr(), K, C, int(bool(transposed)), 0]], dtype=torch.int64).to(w.device)
        bmap = torch.zeros(n, dtype=torch.int32, device=w.device)
        check(lib.dfe_wino_transform_weights_multi(ptr(table), ptr(bmap), n, stream_ptr()), "dfe_wino_transform_weights_multi")
        return U

    def invalidate(self):
        """Call after any write to a registered parameter that does not bump its autograd version counter (``p.data.copy_`` /
        ``mul_``, EMA or weight surgery through ``.data``, another raw-pointer kernel): every entry misses until the next
        refresh().  ddp.FlatAllReduce (after its ``.data`` broadcast) and the checkpoint loaders call it."""
        for e in self.entries.values():
            e["version"] = -1

    def refresh(self):
        """Transform every registered filter (forward and data-gradient orientation) in one launch on the current stream."""
        if not self.enabled or not self.entries:
            return
        lib = get_lib()
        live = []
        for key, e in list(self.entries.items()):
            p = e["ref"]()
            if p is None or p.data_ptr() != key[0] or not p.is_contiguous() or p.dtype != torch.float32:
                del self.entries[key]
                self.members = None
                continue
            live.append((key, e, p))
        if not live:
            return
        dev = live[0][2].device
        live = [t for t in live if t[2].device == dev]
        # the table is rebuilt whenever the membership changed OR any live entry has no buffers yet (a re-registered key)
        members = tuple((k, id(e)) for k, e, _ in live)
        if members != self.members or any(e["U"] is None for _, e, _ in live):
            rows, bmap, nb = [], [], 0
            for key, e, p in live:
                Co, Ci = key[1], key[2]
                if e["U"] is None:
                    e["U"] = (torch.empty(lib.dfe_wino_weight_floats(Ci, Co), device=dev, dtype=torch.float32),
                              torch.empty(lib.dfe_wino_weight_floats(Co, Ci), device=dev, dtype=torch.float32))
                # forward: conv Ci -> Co, U[Kpad(Co)][Ci]; data gradient: conv Co -> Ci on the transposed, flipped filter
                for tr, (K, C) in enumerate(((Co, Ci), (Ci, Co))):
                    n = int(lib.dfe_wino_transform_blocks(C, K))
                    rows.append([key[0], e["U"][tr].data_ptr(), K, C, tr, nb])
                    bmap.extend([len(rows) - 1] * n)
                    nb += n
            self.table = torch.tensor(rows, dtype=torch.int64).to(dev)
            self.blockmap = torch.tensor(bmap, dtype=torch.int32).to(dev)
            self.members = members
        for _, e, _ in live:         # exception-safe: nothing is valid until the launch has been enqueued
            e["version"] = -1
        check(lib.dfe_wino_transform_weights_multi(ptr(self.table), ptr(self.blockmap), int(self.blockmap.numel()), stream_ptr()),
              "dfe_wino_transform_weights_multi")
        for _, e, p in live:
            e["version"] = p._version


wino_weights = WinoWeightCache()


def wino_conv3x3(x, w, padding=1, transposed=False, dilation=1, bias=None, slope=1.0, out=None, out_off=0, out2=None, out2_off=0):
    """3x3 stride-1 convolution of x [B,Ci,H,W] on dfe_wino_conv3x3.  ``transposed``: w is the forward filter [Ci,Co,3,3] of a
    convolution whose output gradient is x; the result is its data gradient.  ``dilation`` > 1: a dilated convolution with
    padding = dilation (``padding`` is ignored).  Parameters' transformed filters come from ``wino_weights`` when it holds
    them (dfe_wino_conv3x3_u).

    ``bias`` / ``slope`` / ``out`` / ``out2`` (round 5): the epilogue act(conv + bias), act(v) = v > 0 ? v : slope v, inside the
    kernel's output transform (dfe_wino_conv3x3_u_act), written to channels out_off.. of ``out`` (a contiguous NCHW buffer with
    at least that many channels; default: a fresh tensor) and, if given, to channels out2_off.. of ``out2`` as well."""
    fused = bias is not None or float(slope) != 1.0 or out is not None or out2 is not None
    U = wino_weights.lookup(w, transposed)
    x, w = f32c(x), f32c(w)
    B, Ci, H, W = x.shape
    Co = int(w.shape[1] if transposed else w.shape[0])
    P, d = int(padding), int(dilation)
    lib = get_lib()
    Ho, Wo = (H, W) if d > 1 else (H + 2 * P - 2, W + 2 * P - 2)

    def split_scratch():
        """(part, part_floats) of dfe_wino_conv3x3_u / _u_act: the partial outputs of the input-channel splits (None, 0: no splits)"""
        n = 0 if d > 1 else lib.dfe_wino_scratch_floats(B, Ci, Co, H, W, P) - lib.dfe_wino_weight_floats(Ci, Co)
        return (torch.empty(n, device=x.device, dtype=torch.float32) if n > 0 else None), n
    if fused:
        if U is None:
            U = WinoWeightCache.transform_now(w, transposed)
        y = torch.empty(B, Co, Ho, Wo, device=x.device, dtype=torch.float32) if out is None else out
        for t in (y, out2):
            if t is not None and not (t.is_contiguous() and t.dtype == torch.float32 and tuple(t.shape[2:]) == (Ho, Wo) and t.shape[0] == B):
                raise _lib.DfeError("wino_conv3x3: out / out2 must be contiguous fp32 [B, >= Co, Ho, Wo] buffers")
        if y.shape[1] < int(out_off) + Co or (out2 is not None and out2.shape[1] < int(out2_off) + Co):
            raise _lib.DfeError("wino_conv3x3: the output channels do not fit the destination buffer")
        part, npart = split_scratch()
        check(lib.dfe_wino_conv3x3_u_act(ptr(x), ptr(U), ptr(f32c(bias)) if bias is not None else None, float(slope),
                                         _chan_ptr(y, out_off), y.stride(0), _chan_ptr(out2, out2_off),
                                         out2.stride(0) if out2 is not None else 0, ptr(part), npart, B, Ci, Co, H, W, P, d, stream_ptr()),
              "dfe_wino_conv3x3_u_act")
        return y
    y = torch.empty(B, Co, Ho, Wo, device=x.device, dtype=torch.float32)
    if U is not None:
        part, npart = split_scratch()
        check(lib.dfe_wino_conv3x3_u(ptr(x), ptr(U), ptr(y), y.stride(0), ptr(part), npart, B, Ci, Co, H, W, P, d, stream_ptr()),
              "dfe_wino_conv3x3_u")
        return y
    nws = lib.dfe_wino_weight_floats(Ci, Co) if d > 1 else lib.dfe_wino_scratch_floats(B, Ci, Co, H, W, P)
    wbuf = torch.empty(nws, device=x.device, dtype=torch.float32)
    if d > 1:
        check(lib.dfe_wino_conv3x3_dilated(ptr(x), ptr(w), ptr(y), y.stride(0), ptr(wbuf), B, Ci, Co, H, W, d, int(bool(transposed)),
                                           stream_ptr()), "dfe_wino_conv3x3_dilated")
        return y
    check(lib.dfe_wino_conv3x3(ptr(x), ptr(w), ptr(y), y.stride(0), ptr(wbuf), nws, B, Ci, Co, H, W, P, int(bool(transposed)),
                               stream_ptr()), "dfe_wino_conv3x3")
    return y


def phase_images(t, d):
    """[B,C,H,W] -> [B d^2, C, H/d, W/d]: the d x d phase images x[:, :, p::d, q::d] stacked along the batch (one strided copy).
    A dilation-d 3x3 convolution with padding d is a dense 3x3 convolution with padding 1 on them."""
    B, C, H, W = t.shape
    return t.reshape(B, C, H // d, d, W // d, d).permute(0, 3, 5, 1, 2, 4).reshape(B * d * d, C, H // d, W // d)


def wino_wgrad3x3(x, gy, padding=1, dilation=1):
    """Weight gradient [Co,Ci,3,3] of a 3x3 stride-1 convolution of x [B,Ci,H,W] with ``padding`` in {0, 1} (or dilated with
    padding = dilation: on the phase images) for the output gradient gy [B,Co,Ho,Wo], on dfe_wino_wgrad3x3 (Winograd domain,
    fp32 MFMA).  x and gy may be batch-strided views (channel slices of concatenated buffers)."""
    d = int(dilation)
    if d > 1:
        if x.shape[2] % d or x.shape[3] % d or gy.shape[2:] != x.shape[2:]:
            raise _lib.DfeError("wino_wgrad3x3: a dilated layer needs H and W to be multiples of the dilation and padding = dilation")
        x, gy, padding = phase_images(x, d), phase_images(gy, d), 1
    x = x if _dense_chw(x) else f32c(x)
    gy = gy if _dense_chw(gy) else f32c(gy)
    B, Ci, H, W = x.shape
    Co, P = int(gy.shape[1]), int(padding)
    lib = get_lib()
    gw = torch.empty(Co, Ci, 3, 3, device=x.device, dtype=torch.float32)
    n = lib.dfe_wino_wgrad_floats(B, Ci, Co, H, W, P)
    if n <= 0:
        raise _lib.DfeError("dfe_wino_wgrad3x3: unsupported shape %s padding %d" % (tuple(x.shape), P))
    ws = torch.empty(n, device=x.device, dtype=torch.float32)
    check(lib.dfe_wino_wgrad3x3(ptr(x, strided=True), x.stride(0), ptr(gy, strided=True), gy.stride(0), ptr(gw), ptr(ws), B, Ci, Co, H, W, P,
                                stream_ptr()), "dfe_wino_wgrad3x3")
    return gw


def sconv_wgrad_supported(x_shape, co, k, stride, padding):
    """Whether dfe_sconv_wgrad takes the layer (csrc/ops_sconv.hip: 3x3 with Ci >= 16, the 3- / 9-channel stems, 5x5 x 16)."""
    B, Ci, H, W = (int(v) for v in x_shape)
    return get_lib().dfe_sconv_wgrad_floats(B, Ci, int(co), H, W, int(k), int(stride), int(padding)) > 0


def sconv_wgrad(x, gy, k, stride, padding):
    """Weight gradient [Co,Ci,k,k] of a strided k x k convolution of x [B,Ci,H,W] for the output gradient gy [B,Co,Ho,Wo], on
    dfe_sconv_wgrad (fp32 MFMA straight from NCHW; depth_model.py:60-95, feature_pyramid.py:7-36, pose_cnn.py:14-36).  x and gy may
    be batch-strided views."""
    x = x if _dense_chw(x) else f32c(x)
    gy = gy if _dense_chw(gy) else f32c(gy)
    B, Ci, H, W = x.shape
    Co, k, s, P = int(gy.shape[1]), int(k), int(stride), int(padding)
    if tuple(gy.shape[2:]) != ((H + 2 * P - k) // s + 1, (W + 2 * P - k) // s + 1) or gy.shape[0] != B:
        raise _lib.DfeError("sconv_wgrad: gy %s does not belong to x %s with k %d stride %d padding %d" % (tuple(gy.shape), tuple(x.shape), k, s, P))
    lib = get_lib()
    n = lib.dfe_sconv_wgrad_floats(B, Ci, Co, H, W, k, s, P)
    if n <= 0:
        raise _lib.DfeError("dfe_sconv_wgrad: unsupported layer %s -> %d, k %d stride %d padding %d" % (tuple(x.shape), Co, k, s, P))
    gw = torch.empty(Co, Ci, k, k, device=x.device, dtype=torch.float32)
    ws = torch.empty(n, device=x.device, dtype=torch.float32)
    check(lib.dfe_sconv_wgrad(ptr(x, strided=True), x.stride(0), ptr(gy, strided=True), gy.stride(0), ptr(gw), ptr(ws), B, Ci, Co, H, W, k, s, P,
                              stream_ptr()), "dfe_sconv_wgrad")
    return gw


# The deterministic mode's forward / data-gradient kernels of the stride-2 layers.  The *_supported queries are host-only.
def sconv_fwd_supported(x_shape, co, k):
    B, Ci, H, W = (int(v) for v in x_shape)
    return get_lib().dfe_sconv_fwd_floats(B, Ci, int(co), H, W, int(k)) > 0


def sconv_fwd(x, w, bias=None, slope=1.0):
    """act(conv2d(x, w, stride 2, padding k // 2) + bias) for k in {3, 5, 7} on dfe_sconv_fwd (fp32 MFMA straight from NCHW;
    depth_model.py:60-95, feature_pyramid.py:7-36, pose_cnn.py:14-36).  slope: 1 none, 0 ReLU, 0.1 LeakyReLU."""
    x = x if _dense_chw(x) else f32c(x)
    w = f32c(w)
    B, Ci, H, W = x.shape
    Co, k = int(w.shape[0]), int(w.shape[2])
    lib = get_lib()
    n = lib.dfe_sconv_fwd_floats(B, Ci, Co, H, W, k)
    if n <= 0 or w.shape[1] != Ci or w.shape[3] != k:
        raise _lib.DfeError("dfe_sconv_fwd: unsupported layer %s * %s" % (tuple(x.shape), tuple(w.shape)))
    P = k // 2
    y = torch.empty(B, Co, (H + 2 * P - k) // 2 + 1, (W + 2 * P - k) // 2 + 1, device=x.device, dtype=torch.float32)
    ws = torch.empty(n, device=x.device, dtype=torch.float32)
    check(lib.dfe_sconv_fwd(ptr(x, strided=True), x.stride(0), ptr(w), None if bias is None else ptr(f32c(bias)), float(slope), ptr(y),
                            y.stride(0), ptr(ws), B, Ci, Co, H, W, k, stream_ptr()), "dfe_sconv_fwd")
    return y


def sconv_dgrad_supported(x_shape, co, k):
    B, Ci, H, W = (int(v) for v in x_shape)
    return get_lib().dfe_sconv_dgrad_floats(B, Ci, int(co), H, W, int(k)) > 0


def sconv_dgrad(gy, w, x_shape):
    """Data gradient [B,Ci,H,W] of conv2d(x, w, stride 2, padding k // 2), k in {1, 3, 5}, for gy, on dfe_sconv_dgrad."""
    gy = gy if _dense_chw(gy) else f32c(gy)
    w = f32c(w)
    B, Ci, H, W = (int(v) for v in x_shape)
    Co, k = int(w.shape[0]), int(w.shape[2])
    lib = get_lib()
    n = lib.dfe_sconv_dgrad_floats(B, Ci, Co, H, W, k)
    P = k // 2
    if n <= 0 or w.shape[1] != Ci or w.shape[3] != k or tuple(gy.shape) != (B, Co, (H + 2 * P - k) // 2 + 1, (W + 2 * P - k) // 2 + 1):
        raise _lib.DfeError("dfe_sconv_dgrad: unsupported layer gy %s * %s -> %s" % (tuple(gy.shape), tuple(w.shape), tuple(x_shape)))
    gx = torch.empty(B, Ci, H, W, device=gy.device, dtype=torch.float32)
    ws = torch.empty(n, device=gy.device, dtype=torch.float32)
    check(lib.dfe_sconv_dgrad(ptr(gy, strided=True), gy.stride(0), ptr(w), ptr(gx), gx.stride(0), ptr(ws), B, Ci, Co, H, W, k, stream_ptr()),
          "dfe_sconv_dgrad")
    return gx


def conv1x1s2_supported(x_shape, co):
    B, Ci, H, W = (int(v) for v in x_shape)
    return get_lib().dfe_conv1x1s2_supported(B, Ci, int(co), H, W) == 1


def conv1x1s2_fwd(x, w):
    """conv2d(x, w [Co,Ci,1,1], stride 2, padding 0) without bias on dfe_conv1x1s2_fwd (depth_model.py:31-36)."""
    x = x if _dense_chw(x) else f32c(x)
    w = f32c(w)
    B, Ci, H, W = x.shape
    Co = int(w.shape[0])
    if tuple(w.shape[1:]) != (Ci, 1, 1) or not conv1x1s2_supported(x.shape, Co):
        raise _lib.DfeError("dfe_conv1x1s2_fwd: unsupported layer %s * %s" % (tuple(x.shape), tuple(w.shape)))
    y = torch.empty(B, Co, (H - 1) // 2 + 1, (W - 1) // 2 + 1, device=x.device, dtype=torch.float32)
    check(get_lib().dfe_conv1x1s2_fwd(ptr(x, strided=True), x.stride(0), ptr(w), ptr(y), y.stride(0), B, Ci, Co, H, W, stream_ptr()),
          "dfe_conv1x1s2_fwd")
    return y


def conv1x1s2_wgrad(x, gy):
    """Weight gradient [Co,Ci,1,1] of the same layer for the output gradient gy, on dfe_conv1x1s2_wgrad (fixed-order split sums)."""
    x = x if _dense_chw(x) else f32c(x)
    gy = gy if _dense_chw(gy) else f32c(gy)
    B, Ci, H, W = x.shape
    Co = int(gy.shape[1])
    lib = get_lib()
    n = lib.dfe_conv1x1s2_wgrad_floats(B, Ci, Co, H, W)
    if n <= 0 or tuple(gy.shape) != (B, Co, (H - 1) // 2 + 1, (W - 1) // 2 + 1):
        raise _lib.DfeError("dfe_conv1x1s2_wgrad: gy %s does not belong to x %s" % (tuple(gy.shape), tuple(x.shape)))
    gw = torch.empty(Co, Ci, 1, 1, device=x.device, dtype=torch.float32)
    ws = torch.empty(n, device=x.device, dtype=torch.float32)
    check(lib.dfe_conv1x1s2_wgrad(ptr(x, strided=True), x.stride(0), ptr(gy, strided=True), gy.stride(0), ptr(gw), ptr(ws), B, Ci, Co, H, W,
                                  stream_ptr()), "dfe_conv1x1s2_wgrad")
    return gw


class PlaneConvActFn(torch.autograd.Function):
    """act(conv3x3(x, w, pad 1) + bias) on a small plane as one operator (PoseCNN's refinement convolutions,
    pose_cnn.py:43-46, 66-69: Conv2d(12, 12, 3, 1, 1) + ReLU on 2x7 planes): dfe_planeconv_fwd with the epilogue inside;
    backward = dfe_bias_act_bwd (activation mask from the output, bias gradient) + dfe_planeconv_dgrad / _wgrad."""

    @staticmethod
    def forward(ctx, x, w, bias, slope):
        x, w = f32c(x), f32c(w)
        y = torch.empty(x.shape[0], w.shape[0], x.shape[2], x.shape[3], device=x.device, dtype=torch.float32)
        planeconv_fwd_into(x, w, None if bias is None else f32c(bias), slope, y)
        ctx.save_for_backward(x, w, y)
        ctx.slope, ctx.has_bias = float(slope), bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w, y = ctx.saved_tensors
        gz, gb = _bias_act_bwd(y, f32c(gy), ctx.slope, ctx.has_bias and ctx.needs_input_grad[2])
        gx, gw = planeconv_backward(gz, x, w, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gw, gb, None


def planeconv_act(x, w, bias, slope):
    return PlaneConvActFn.apply(x, w, bias, float(slope))


class Conv1x1SmallFn(torch.autograd.Function):
    """act(conv1x1(x, w) + bias) on a tiny plane (PoseCNN's pose_conv / refinement 1x1 convolutions on 2x7 planes,
    pose_cnn.py:32,43,48) as one operator: dfe_conv1x1_small_fwd; backward = dfe_bias_act_bwd + dfe_conv1x1_small_bwd."""

    @staticmethod
    def forward(ctx, x, w, bias, slope):
        x, w = f32c(x), f32c(w)
        B, Ci, H, W = x.shape
        Co = int(w.shape[0])
        y = torch.empty(B, Co, H, W, device=x.device, dtype=torch.float32)
        check(get_lib().dfe_conv1x1_small_fwd(ptr(x), ptr(w), ptr(None if bias is None else f32c(bias)), float(slope), ptr(y),
                                              B, Ci, Co, H, W, stream_ptr()), "dfe_conv1x1_small_fwd")
        ctx.save_for_backward(x, w, y)
        ctx.slope, ctx.has_bias = float(slope), bias is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = get_lib()
        x, w, y = ctx.saved_tensors
        B, Co, H, W = y.shape
        Ci = int(x.shape[1])
        gz, gb = _bias_act_bwd(y, f32c(gy), ctx.slope, ctx.has_bias and ctx.needs_input_grad[2])
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if ctx.needs_input_grad[1] else None
        check(lib.dfe_conv1x1_small_bwd(ptr(gz), ptr(x), ptr(w), ptr(gx), ptr(gw), B, Ci, Co, H, W, stream_ptr()),
              "dfe_conv1x1_small_bwd")
        return gx, gw, gb, None


def conv1x1_small(x, conv, slope):
    """``act(conv(x))`` for an nn.Conv2d with a 1x1 kernel on a tiny plane; slope 1 = no activation."""
    return Conv1x1SmallFn.apply(x, conv.weight, conv.bias, float(slope))


# --------------------------------------------------------------------------- grouped BatchNorm (+ residual + ReLU)
class GroupedBatchNormFn(torch.autograd.Function):
    """Training-mode BatchNorm2d over G groups of consecutive samples (statistics per (group, channel); the running
    statistics get the G momentum updates in group order) fused with an optional residual add and ReLU."""

    @staticmethod
    def forward(ctx, x, residual, weight, bias, running_mean, running_var, groups, eps, momentum, relu):
        lib = get_lib()
        x = f32c(x)
        N, C, H, W = x.shape
        G = int(groups)
        if N % G:
            raise ValueError("batch %d is not divisible into %d groups" % (N, G))
        Bg = N // G
        residual = f32c(residual) if residual is not None else None
        if residual is not None and residual.shape != x.shape:
            raise ValueError("residual must have the shape of x")
        dev = x.device
        y = torch.empty_like(x)
        mean = torch.empty(G * C, device=dev)
        invstd = torch.empty(G * C, device=dev)
        npart = lib.dfe_bn_partials_floats(G, Bg, C, H, W)
        part = torch.empty(max(npart, 1), device=dev)
        check(lib.dfe_bn_fwd(ptr(x), ptr(residual), ptr(weight), ptr(bias), ptr(running_mean), ptr(running_var), ptr(y),
                             ptr(mean), ptr(invstd), ptr(part), G, Bg, C, H, W, float(eps), float(momentum), int(relu),
                             stream_ptr()), "dfe_bn_fwd")
        ctx.save_for_backward(x, y if relu else x.new_empty(0), weight if weight is not None else x.new_empty(0), mean, invstd)
        ctx.cfg = (G, Bg, C, H, W, int(relu), residual is not None, weight is not None)
        ctx.mark_non_differentiable(mean, invstd)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = get_lib()
        x, y, weight, mean, invstd = ctx.saved_tensors
        G, Bg, C, H, W, relu, has_res, has_w = ctx.cfg
        gy = f32c(gy)
        dev = x.device
        gx = torch.empty_like(x)
        # without a ReLU the residual's gradient is gy itself
        gres = (torch.empty_like(x) if relu else None) if (has_res and ctx.needs_input_grad[1]) else None
        gw = torch.empty(C, device=dev) if (has_w and ctx.needs_input_grad[2]) else None
        gb = torch.empty(C, device=dev) if ctx.needs_input_grad[3] else None
        part = torch.empty(max(lib.dfe_bn_partials_floats(G, Bg, C, H, W), 1), device=dev)
        scratch = torch.empty(2 * G * C, device=dev)
        check(lib.dfe_bn_bwd(ptr(x), ptr(y) if relu else None, ptr(gy), ptr(weight) if has_w else None, ptr(mean), ptr(invstd),
                             ptr(gx), ptr(gres), ptr(gw), ptr(gb), ptr(part), ptr(scratch), G, Bg, C, H, W, relu,
                             stream_ptr()), "dfe_bn_bwd")
        if has_res and ctx.needs_input_grad[1] and not relu:
            gres = gy
        return gx, gres, gw, gb, None, None, None, None, None, None


def grouped_batch_norm(x, weight, bias, running_mean, running_var, groups=1, eps=1e-5, momentum=0.1, residual=None,
                       relu=False):
    return GroupedBatchNormFn.apply(x, residual, weight, bias, running_mean, running_var, int(groups), float(eps),
                                    float(momentum), bool(relu))


# --------------------------------------------------------------------------- eval-mode BatchNorm (+ residual + ReLU), forward only
def _forward_only(what, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise DfeError("%s is forward-only (it has no backward pass): call it under torch.no_grad(), or detach its inputs" % what)


def bn_fold(bn, out=None):
    """(scale, shift) [C] of an eval-mode ``nn.BatchNorm2d``: in double, scale = weight / sqrt(running_var + eps) and
    shift = bias - running_mean * scale, each rounded once to fp32 (dfe_bn_fold, one launch).  ``out``: a (scale, shift) pair of
    earlier tables to fold into in place -- whatever holds their addresses (a captured graph) reads the new values."""
    if bn.running_mean is None or bn.running_var is None:
        raise DfeError("bn_fold: the layer tracks no running statistics")
    _forward_only("bn_fold", bn.weight, bn.bias, bn.running_mean, bn.running_var)
    C = int(bn.running_mean.numel())
    scale, shift = out if out is not None else (torch.empty(C, device=bn.running_mean.device, dtype=torch.float32) for _ in range(2))
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.numel() != C:
            raise DfeError("bn_fold: out must be two fp32 tensors of %d elements" % C)
    w, b = (None if t is None else f32c(t.detach()) for t in (bn.weight, bn.bias))
    check(get_lib().dfe_bn_fold(ptr(w), ptr(b), ptr(f32c(bn.running_mean)), ptr(f32c(bn.running_var)), float(bn.eps), ptr(scale),
                                ptr(shift), C, stream_ptr()), "dfe_bn_fold")
    return scale, shift


def bn_eval(x, scale, shift, residual=None, relu=False, out=None):
    """act(x * scale[c] + shift[c] [+ residual]) over x [B,C,H,W] with the tables of ``bn_fold``: one streaming pass
    (dfe_bn_eval_fwd), the product and the adds rounded once each.  ``out``: the destination (default: a fresh tensor); ``out is x``
    runs in place.  ``residual`` must not share memory with ``out``."""
    _forward_only("bn_eval", x, scale, shift, residual)
    if x.dim() != 4:
        raise DfeError("bn_eval: x must be [B,C,H,W], got %s" % (tuple(x.shape),))
    x = x if out is x else f32c(x)
    B, C, H, W = x.shape
    residual = f32c(residual) if residual is not None else None
    if residual is not None and residual.shape != x.shape:
        raise DfeError("bn_eval: residual must have the shape of x")
    if any(t.dtype != torch.float32 or t.numel() != C for t in (scale, shift)):
        raise DfeError("bn_eval: scale / shift must be fp32 tensors of %d channels (ops.bn_fold's)" % C)
    y = torch.empty_like(x) if out is None else out
    if y.shape != x.shape or y.dtype != torch.float32 or x.dtype != torch.float32:
        raise DfeError("bn_eval: out must be an fp32 tensor of the shape of x")
    if residual is not None and residual.data_ptr() == y.data_ptr():
        raise DfeError("bn_eval: residual must not alias out")
    check(get_lib().dfe_bn_eval_fwd(ptr(x), ptr(residual), ptr(scale), ptr(shift), ptr(y), B, C, H, W, int(bool(relu)), stream_ptr()),
          "dfe_bn_eval_fwd")
    return y


# --------------------------------------------------------------------------- disparity head (Conv3x3(C -> 1) + sigmoid)
class DispHeadFn(torch.autograd.Function):
    """sigmoid(conv3x3(p) + bias) on a reflection-padded activation p [B,C,H+2,W+2] -> [B,1,H,W]."""

    @staticmethod
    def forward(ctx, p, weight, bias):
        lib = get_lib()
        p, weight = f32c(p), f32c(weight)
        bias = f32c(bias) if bias is not None else None
        B, C, Hp, Wp = p.shape
        if tuple(weight.shape) != (1, C, 3, 3):
            raise ValueError("weight must be [1,%d,3,3], got %s" % (C, tuple(weight.shape)))
        H, W = Hp - 2, Wp - 2
        out = torch.empty(B, 1, H, W, device=p.device)
        check(lib.dfe_disp_head_fwd(ptr(p), ptr(weight), ptr(bias), ptr(out), B, C, H, W, stream_ptr()), "dfe_disp_head_fwd")
        ctx.save_for_backward(p, weight, out)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        lib = get_lib()
        p, weight, out = ctx.saved_tensors
        B, C, Hp, Wp = p.shape
        H, W = Hp - 2, Wp - 2
        gout = f32c(gout)
        gp = torch.empty_like(p)
        gw = torch.empty_like(weight) if ctx.needs_input_grad[1] else None
        gb = torch.empty(1, device=p.device) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        part = torch.empty(lib.dfe_disp_head_partials_floats(B, C, H, W), device=p.device)
        check(lib.dfe_disp_head_bwd(ptr(p), ptr(weight), ptr(out), ptr(gout), ptr(gp), ptr(gw), ptr(gb), ptr(part), B, C, H, W,
                                    stream_ptr()), "dfe_disp_head_bwd")
        return gp, gw, gb


def disp_head(p, weight, bias):
    return DispHeadFn.apply(p, weight, bias)


# --------------------------------------------------------------------------- thin 3x3 convolution (MFMA weight gradient)
def flow_head_fwd_raw(x, weight, bias):
    """Conv2d(C, 2, 3, 1, 1) forward on a contiguous fp32 HIP tensor (no autograd of its own)."""
    lib = get_lib()
    B, C, H, W = x.shape
    out = torch.empty(B, 2, H, W, device=x.device, dtype=torch.float32)
    check(lib.dfe_flow_head_fwd(ptr(x), ptr(weight), ptr(bias), ptr(out), B, C, H, W, stream_ptr()), "dfe_flow_head_fwd")
    return out


def flow_head_bwd_raw(x, weight, gout, want_w=True, want_b=True):
    """(gx, gweight, gbias) of the flow head."""
    lib = get_lib()
    B, C, H, W = x.shape
    gx = torch.empty_like(x)
    gw = torch.empty_like(weight) if want_w else None
    gb = torch.empty(2, device=x.device, dtype=torch.float32) if want_b else None
    part = torch.empty(lib.dfe_flow_head_partials_floats(B, C, H, W), device=x.device, dtype=torch.float32)
    check(lib.dfe_flow_head_bwd(ptr(x), ptr(weight), ptr(gout), ptr(gx), ptr(gw), ptr(gb), ptr(part), B, C, H, W,
                                stream_ptr()), "dfe_flow_head_bwd")
    return gx, gw, gb


class FlowHeadFn(torch.autograd.Function):
    """``F.conv2d(x, weight, bias, 1, 1)`` with two output channels on the rolling-window head kernels
    (csrc/ops_disphead.hip)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x, weight, bias = f32c(x), f32c(weight), f32c(bias)
        ctx.save_for_backward(x, weight)
        return flow_head_fwd_raw(x, weight, bias)

    @staticmethod
    def backward(ctx, gout):
        x, weight = ctx.saved_tensors
        gx, gw, gb = flow_head_bwd_raw(x, weight, f32c(gout), ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return (gx if ctx.needs_input_grad[0] else None), gw, gb


def wgrad3x3(p, gy):
    """Weight gradient [Co,Ci,3,3] of a valid 3x3 convolution of the pre-padded activation p [B,Ci,H+2,W+2] for the output gradient
    gy [B,Co,H,W], on dfe_wgrad3x3_fwd (fp32 MFMA straight from NCHW): the depth decoder's thin full-resolution layers."""
    lib = get_lib()
    p, gy = f32c(p), f32c(gy)
    B, Ci, Hp, Wp = p.shape
    Co, H, W = int(gy.shape[1]), Hp - 2, Wp - 2
    gw = torch.empty(Co, Ci, 3, 3, device=p.device, dtype=torch.float32)
    part = torch.empty(lib.dfe_wgrad3x3_partials_floats(B, Ci, Co, H, W), device=p.device)
    check(lib.dfe_wgrad3x3_fwd(ptr(p), ptr(gy), ptr(gw), ptr(part), B, Ci, Co, H, W, stream_ptr()), "dfe_wgrad3x3_fwd")
    return gw
