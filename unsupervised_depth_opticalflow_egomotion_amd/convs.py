"""The one door to the networks' convolutions: MIOpen's, or this build's fp32 matrix-core kernels where they win -- or, in the
deterministic mode (``set_deterministic``), this build's kernels for every pass and an error where there is none.  Everything is fp32.

``plan`` is the one place that decides which kernel a convolution's forward pass, data gradient and weight gradient run on;
every door below (``conv2d``, ``Conv2d``, ``conv_act``, ``conv3x3_valid``, ``dense_decode``, ``raw_forward`` / ``raw_backward``)
executes its record.  tests/golden/conv_routes.json pins the record of every convolution of a training step.  The kernels'
ctypes wrappers live in ops.py, which knows nothing of this module.  What each route was measured to buy, and what was tried
and dropped (bf16 at the door, MIOpen's backward-data kernels for the forward pass): DESIGN.md section 4, EXPERIMENT_LOG.md."""
from __future__ import annotations

import collections
import ctypes
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import miopen_tuning, ops
from ._lib import DfeError, check, f32c, get_lib, ptr, stream_ptr

miopen_tuning.activate()      # before the first convolution: MIOpen reads MIOPEN_USER_DB_PATH when it first opens its databases

_cb = torch.ops.aten.convolution_backward

# The routing switches, each read from its environment variable once, here (246 environment reads per step before).  plan()
# reads the module constants at call time, so a test or a tool may set them on this module.
WINO_MIN_TILES = int(os.environ.get("DFE_WINO_MIN_TILES", "500"))      # smallest B * ceil(Ho/2) * ceil(Wo/2) on dfe_wino_conv3x3; 0 = never
WINO_MIN_CHANNELS = int(os.environ.get("DFE_WINO_MIN_CHANNELS", "16"))
WINO_DILATED = os.environ.get("DFE_WINO_DILATED", "1") == "1"     # dilated layers too (instead of MIOpen / the phase-image path)
WINO_EPILOGUE = os.environ.get("DFE_WINO_EPILOGUE", "1") != "0"   # bias + activation inside the Winograd kernel's output transform
WINO_WGRAD = os.environ.get("DFE_WINO_WGRAD", "1") != "0"         # dfe_wino_wgrad3x3; 0 = MIOpen's weight gradients everywhere
WINO_WGRAD_MIN_MACS = float(os.environ.get("DFE_WINO_WGRAD_MIN_GMAC", "0.8")) * 1e9      # direct multiply-adds of the layer
# dilated layers run it on the d x d phase images up to this dilation; at 8 / 16 they are 8x26 / 4x13 pixels, too short for its 12-tile chunks
WINO_WGRAD_MAX_DILATION = int(os.environ.get("DFE_WINO_WGRAD_MAX_DILATION", "4"))
SCONV = os.environ.get("DFE_SCONV", "1") != "0"                   # dfe_sconv_wgrad for the stride-2 layers with thin inputs
SCONV_WGRAD_MAX_CI = int(os.environ.get("DFE_SCONV_WGRAD_MAX_CI", "16"))      # (wider layers: MIOpen at 64 - 70 TFLOP/s, this kernel at 50 - 57)
# smallest dilation whose 3x3 "same" layer runs as a dense convolution on its d*d phase images x[:, :, p::d, q::d] (same products,
# same sums, a kernel MIOpen solves with Winograd); 0 = off.  8: the two layers that gain most, half the re-layout copies
PHASE_MIN_DILATION = int(os.environ.get("DFE_PHASE_CONV", "8"))
# planes of at most this many pixels per sample take the dfe_planeconv_* / dfe_conv1x1_small_* kernels (PWC levels 6 and 5 of a
# 256x832 frame: 52 and 208 pixels; PoseCNN's 2x7 planes); 0 = every such layer stays on MIOpen
PLANECONV_MAX_HW = int(os.environ.get("DFE_PLANECONV_MAX_HW", "208"))
FLOW_HEAD = os.environ.get("DFE_FLOW_HEAD", "1") != "0"           # PWC's two-channel flow heads on the rolling-window head kernels
# The deterministic mode: no convolution of a HIP tensor reaches MIOpen / ATen.  Every stride-2 layer runs on dfe_sconv_* /
# dfe_conv1x1s2_*, every 3x3 stride-1 layer on the Winograd kernels whatever the thresholds above say (they, DFE_SCONV, DFE_WINO_WGRAD
# and DFE_WINO_DILATED do not limit here), the small-plane / flow-head / wgrad3x3 layers stay where they are, and a layer no kernel
# of this build takes raises DfeError.  MIOpen's weight gradients add with float atomics and its solver choice follows the workspace
# the allocator happens to hand it; these kernels add in one fixed order.  What it promises and costs: README "Reproducible".
DETERMINISTIC = os.environ.get("DFE_DETERMINISTIC", "0") == "1"

# The kernel of each pass of one layer: "miopen", or "wino" (dfe_wino_conv3x3; as a data gradient, on the transposed filter), "wino_act"
# (with the bias + activation epilogue), "phase" (a dense convolution on the phase images, itself planned), "wino_wgrad", "sconv_wgrad",
# "wgrad3x3" (dfe_wgrad3x3_fwd), and "plane" / "conv1x1" / "flow_head", whose three passes are their own (dfe_planeconv_*, ...).
# The deterministic mode adds "sconv" (dfe_sconv_fwd / dfe_sconv_dgrad), "sconv_act" (with the bias + activation epilogue),
# "conv1x1s2" (dfe_conv1x1s2_fwd / _wgrad) and, as a data gradient only, "none": no kernel takes it, and asking for it raises
# (the 7x7 stems, whose input is the image).
Plan = collections.namedtuple("Plan", "fwd dgrad wgrad")
MIOPEN = Plan("miopen", "miopen", "miopen")
_PLANE, _CONV1X1, _HEAD = Plan("plane", "plane", "plane"), Plan("conv1x1", "conv1x1", "conv1x1"), Plan("flow_head", "flow_head", "flow_head")
_plans = {}


def set_deterministic(flag):
    """Switch the deterministic mode (DFE_DETERMINISTIC) after import; plans are memoised per setting."""
    global DETERMINISTIC
    DETERMINISTIC = bool(flag)


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def _out_hw(shape, w, stride, padding, dilation):
    return ((shape[2] + 2 * padding[0] - dilation[0] * (w[2] - 1) - 1) // stride[0] + 1,
            (shape[3] + 2 * padding[1] - dilation[1] * (w[3] - 1) - 1) // stride[1] + 1)


def _wino(f32, shape, w, cin, stride, padding, dilation, det=False):
    """[B,cin,H,W] convolved 3x3 / stride 1 with ``padding`` in {0, 1} (or dilated with padding = dilation dividing H and W):
    enough tiles and reduction channels for dfe_wino_conv3x3?  ``det``: whether the kernel takes the layer at all."""
    if (WINO_MIN_TILES <= 0 and not det) or not f32 or w[2:] != (3, 3) or stride != (1, 1) or dilation[0] != dilation[1]:
        return False
    B, C, H, W = shape
    d = dilation[0]
    if d > 1:
        if padding != (d, d) or H % d or W % d or H // d < 2 or W // d < 2 or not (WINO_DILATED or det):
            return False
        Ho, Wo, tiles_b = H // d, W // d, B * d * d
    else:
        if padding not in ((0, 0), (1, 1)):
            return False
        Ho, Wo, tiles_b = H + 2 * padding[0] - 2, W + 2 * padding[0] - 2, B
    if C != cin or Ho < 1 or Wo < 1:
        return False
    return (det or (tiles_b * ((Ho + 1) // 2) * ((Wo + 1) // 2) >= WINO_MIN_TILES and C >= WINO_MIN_CHANNELS)) and B * C * H * W < (1 << 30)


def _wino_wgrad(f32, shape, w, stride, padding, dilation, det=False):
    """dfe_wino_wgrad3x3 for the filter of a 3x3 stride-1 layer on x [B,Ci,H,W]: >= 16 channels on both sides, enough work
    (``det``: any channel count, any amount of work, any dilation whose phase images are whole)"""
    d = dilation[0]
    if not (WINO_WGRAD or det) or not f32 or w[2:] != (3, 3) or stride != (1, 1) or dilation != (d, d):
        return False
    if d > 1 and not ((det or d <= WINO_WGRAD_MAX_DILATION) and padding == (d, d) and shape[2] % d == 0 and shape[3] % d == 0):
        return False
    if d == 1 and padding not in ((0, 0), (1, 1)):
        return False
    Co, Ci = w[0], w[1]
    ho, wo = _out_hw(shape, w, stride, padding, dilation)
    if Ci != shape[1] or (min(Co, Ci) < 16 and not det) or ho < 1 or wo < 1:      # (16 -> 16 at 128x416 x 12: 83 against MIOpen's 129 us)
        return False
    n_out = shape[0] * Co * ho * wo
    return (det or float(n_out) * Ci * 9 >= WINO_WGRAD_MIN_MACS) and shape[0] * shape[1] * shape[2] * shape[3] < (1 << 30) and n_out < (1 << 30)


def _sconv_wgrad(f32, shape, w, stride, padding, dilation):
    """dfe_sconv_wgrad for a stride-2 k x k layer (k in {3, 5, 7}, padding k // 2) with a thin input"""
    k = w[2]
    return (SCONV and f32 and stride == (2, 2) and dilation == (1, 1) and w[3] == k and k in (3, 5, 7) and padding == (k // 2, k // 2)
            and w[1] <= SCONV_WGRAD_MAX_CI and shape[0] * shape[1] * shape[2] * shape[3] < (1 << 30)
            and ops.sconv_wgrad_supported(shape, w[0], k, 2, k // 2))


def _raw(f32, shape, w, stride, padding, dilation):
    """A bias-free fp32 layer inside an autograd Function: Winograd forward / data gradient where there are enough tiles (the
    data gradient is judged on the output gradient, whose channels are the filter's outputs, as a padding-1 layer -- it is
    launched with padding 2 for a valid convolution), the weight gradient in the Winograd domain or on dfe_sconv_wgrad."""
    if DETERMINISTIC:
        return _det_raw(f32, shape, w, stride, padding, dilation, 1)
    d = dilation[0]
    gy = (shape[0], w[0]) + _out_hw(shape, w, stride, padding, dilation)
    return Plan("wino" if _wino(f32, shape, w, w[1], stride, padding, dilation) else "miopen",
                "wino" if (padding in ((1, 1), (0, 0)) or (d > 1 and padding == (d, d)))
                and _wino(f32, gy, w, w[0], stride, (d, d) if d > 1 else (1, 1), dilation) else "miopen",
                "wino_wgrad" if _wino_wgrad(f32, shape, w, stride, padding, dilation) else
                "sconv_wgrad" if _sconv_wgrad(f32, shape, w, stride, padding, dilation) else "miopen")


def _det_raw(f32, shape, w, stride, padding, dilation, groups):
    """The deterministic mode's kernels of a bias-free layer, or DfeError naming it: stride 2 on dfe_sconv_* (k in {3, 5, 7}, padding
    k // 2; no data gradient at k = 7) or dfe_conv1x1s2_* (k = 1, padding 0; its data gradient is dfe_sconv_dgrad's k = 1), 3x3 stride 1
    on the Winograd kernels at any size."""
    k, d = w[2], dilation[0]
    if f32 and groups == 1 and w[1] == shape[1] and w[3] == k and shape[0] * shape[1] * shape[2] * shape[3] < (1 << 30):
        if stride == (2, 2) and dilation == (1, 1):
            if (k in (3, 5, 7) and padding == (k // 2, k // 2) and ops.sconv_fwd_supported(shape, w[0], k)
                    and ops.sconv_wgrad_supported(shape, w[0], k, 2, k // 2)):
                return Plan("sconv", "sconv" if ops.sconv_dgrad_supported(shape, w[0], k) else "none", "sconv_wgrad")
            if k == 1 and padding == (0, 0) and ops.conv1x1s2_supported(shape, w[0]) and ops.sconv_dgrad_supported(shape, w[0], 1):
                return Plan("conv1x1s2", "sconv", "conv1x1s2")
        gy = (shape[0], w[0]) + _out_hw(shape, w, stride, padding, dilation)
        if (_wino(f32, shape, w, w[1], stride, padding, dilation, True) and _wino_wgrad(f32, shape, w, stride, padding, dilation, True)
                and _wino(f32, gy, w, w[0], stride, (d, d) if d > 1 else (1, 1), dilation, True)):
            return Plan("wino", "wino", "wino_wgrad")
    raise DfeError("deterministic mode (DFE_DETERMINISTIC / convs.set_deterministic): no fixed-order kernel of this build takes the "
                   "convolution of x %s (%s) with w %s, stride %s, padding %s, dilation %s, groups %d; MIOpen would, and is not "
                   "reproducible" % (tuple(shape), "fp32" if f32 else "not fp32", tuple(w), stride, padding, dilation, groups))


def _phase(shape, w, stride, padding, dilation):
    """a dilated 3x3 "same" layer whose d x d phase images are whole"""
    d = dilation[0]
    return (0 < PHASE_MIN_DILATION <= d and dilation == (d, d) and stride == (1, 1) and padding == (d, d) and w[2:] == (3, 3)
            and shape[2] % d == 0 and shape[3] % d == 0)


def _conv2d(f32, shape, w, stride, padding, dilation, groups):
    """``conv2d``: a layer none of whose forward pass and weight gradient is ours is one ATen call (its data gradient MIOpen's too)"""
    if DETERMINISTIC:
        return _det_raw(f32, shape, w, stride, padding, dilation, groups)
    if groups != 1:
        return MIOPEN
    r = _raw(f32, shape, w, stride, padding, dilation)
    d = dilation[0]
    if d > 1 and r.fwd != "wino" and _phase(shape, w, stride, padding, dilation):
        inner = _conv2d(f32, (shape[0] * d * d, shape[1], shape[2] // d, shape[3] // d), w, (1, 1), (1, 1), (1, 1), 1)
        return Plan("phase", inner.dgrad, inner.wgrad)
    return r if r.fwd == "wino" or r.wgrad != "miopen" else MIOPEN


def _plane(f32, shape, w):
    return (PLANECONV_MAX_HW > 0 and f32 and w[1:] == (shape[1], 3, 3) and shape[2] * shape[3] <= PLANECONV_MAX_HW
            and get_lib().dfe_planeconv_supported(shape[0], shape[1], w[0], shape[2], shape[3]) == 1)


def _flow_head(f32, shape, w, bias):
    """PWC's predict_flow layers (pwc_tf.py:39-40): two output channels, 3x3, channel count a multiple of 8."""
    return FLOW_HEAD and f32 and w[2:] == (3, 3) and w[0] == 2 and w[1] == shape[1] and shape[1] % 8 == 0 and bias


def _thin(f32, contiguous, shape, w):
    """pre-padded layers the MFMA weight gradient wins on: <= 32 output channels at >= 64x208 pixels, channels and width multiples of 16"""
    return (f32 and contiguous and w[2:] == (3, 3) and w[0] <= 32 and w[0] % 16 == 0 and w[1] % 16 == 0 and (shape[3] - 2) % 16 == 0
            and (shape[2] - 2) * (shape[3] - 2) >= 64 * 208)


def _route(ctx, f32, shape, w, stride, padding, dilation, groups, bias, fuse, act, plane, contiguous):
    det = DETERMINISTIC
    if len(shape) != 4:
        if det:
            raise DfeError("deterministic mode: no kernel of this build takes a convolution of a %d-dimensional input %s" % (len(shape), tuple(shape)))
        return MIOPEN
    std3 = w[2:] == (3, 3) and stride == (1, 1) and padding == (1, 1) and dilation == (1, 1) and groups == 1
    if ctx == "raw":
        return _raw(f32, shape, w, stride, padding, dilation)
    if ctx == "conv_act":
        if "plane" in fuse and std3 and _plane(f32, shape, w):      # FeaturePyramid's top levels (8x26, 4x13), PoseCNN's 2x7 planes
            return _PLANE
        if ("wino_act" in fuse and WINO_EPILOGUE and bias and groups == 1 and _wino(f32, shape, w, w[1] * groups, stride, padding, dilation, det)
                and padding == ((1, 1) if dilation == (1, 1) else dilation)):
            return _raw(f32, shape, w, stride, padding, dilation)._replace(fwd="wino_act")
        if det and "sconv_act" in fuse and bias and stride == (2, 2) and w[2] > 1:      # bias + activation inside dfe_sconv_fwd
            r = _det_raw(f32, shape, w, stride, padding, dilation, groups)
            return r._replace(fwd="sconv_act") if r.fwd == "sconv" else r
        if ("conv1x1" in fuse and PLANECONV_MAX_HW > 0 and f32 and w[2:] == (1, 1) and stride == (1, 1) and padding == (0, 0) and groups == 1
                and get_lib().dfe_conv1x1_small_supported(shape[0], shape[1], w[0], shape[2], shape[3]) == 1):
            return _CONV1X1
        ctx = "conv2d" if act else "module"      # unfused: bias_act(conv2d(x)), or the module's own forward where no activation follows
    if ctx == "module" and std3 and _flow_head(f32, shape, w, bias):
        return _HEAD
    if ctx in ("module", "conv2d"):
        return _conv2d(f32, shape, w, stride, padding, dilation, groups)
    if ctx == "dense":          # a PWC dense block's layer: ``plane`` is the block's decision, taken once from its first layer
        if _plane(f32, shape, w) if plane is None else plane:
            return _PLANE
        r = _raw(f32, shape, w, stride, padding, dilation)
        return r._replace(fwd="wino_act") if WINO_EPILOGUE and r.fwd == "wino" else r
    if ctx == "dense_head":     # the block's flow head; unfused it is F.conv2d forward, raw_backward (with the bias gradient) backward
        if _flow_head(f32, shape, w, bias):
            return _HEAD
        r = _raw(f32, shape, w, stride, padding, dilation)
        return r if det else r._replace(fwd="miopen")
    if ctx == "prepadded":      # the depth decoder's valid 3x3 layers on a reflection-padded activation
        if _thin(f32, contiguous, shape, w):
            # the weight gradient is ours whatever its size: the Winograd-domain kernel from 32 input channels (96 -> 32 at 130x418 x 12:
            # 229 against 374 us; 32 -> 16: 102 against ~124), dfe_wgrad3x3_fwd for the 16 -> 16 layer at 258x834 (133 against 304)
            return _raw(f32, shape, w, stride, padding, dilation)._replace(wgrad="wino_wgrad" if w[1] >= 32 and (WINO_WGRAD or det) else "wgrad3x3")
        return _conv2d(f32, shape, w, stride, padding, dilation, groups)
    raise ValueError("convs.plan: unknown context %r" % (ctx,))


def plan(x, w_shape, stride=1, padding=0, dilation=1, groups=1, bias=False, act=False, ctx="conv2d", fuse=(), plane=None):
    """The kernels of one layer, as a ``Plan``: shape and switch logic only.

    x: the input tensor, or its (is_cuda, dtype, shape); w_shape: the filter's shape; bias / act: whether a bias and an activation
    follow.  ctx, the door the layer came through: "conv2d" (the functional), "module" (``Conv2d.forward``: the flow head first),
    "conv_act" (``conv_act``; ``fuse`` names the fused kernels the caller admits, of "plane", "wino_act", "conv1x1", "sconv_act"), "raw"
    (``raw_forward`` / ``raw_backward``), "dense" / "dense_head" (``DenseDecodeFn``; ``plane``: the block's small-plane decision,
    None = decide it from this layer), "prepadded" (``conv3x3_valid``).  Host tensors are all MIOpen/ATen, decided before the
    library is touched.  In the deterministic mode no plan of a HIP tensor names "miopen" and a layer without a kernel raises DfeError
    here.  Memoised with the switches in the key: at batch 1 the step is bound by the host's enqueue time."""
    is_cuda, dtype, shape = x if isinstance(x, tuple) else (x.is_cuda, x.dtype, x.shape)
    if not is_cuda:
        return MIOPEN
    contiguous = ctx != "prepadded" or isinstance(x, tuple) or x.is_contiguous()
    exact = lambda v: v if type(v) is tuple else _pair(v)      # noqa: E731  (modules and the doors below pass pairs of ints)
    key = (ctx, dtype, shape if isinstance(shape, tuple) else tuple(shape), w_shape if isinstance(w_shape, tuple) else tuple(w_shape),
           exact(stride), exact(padding), exact(dilation), groups, bool(bias), fuse, act, plane, contiguous,
           WINO_MIN_TILES, WINO_MIN_CHANNELS, WINO_DILATED, WINO_EPILOGUE, WINO_WGRAD, WINO_WGRAD_MIN_MACS, WINO_WGRAD_MAX_DILATION,
           SCONV, SCONV_WGRAD_MAX_CI, PHASE_MIN_DILATION, PLANECONV_MAX_HW, FLOW_HEAD, DETERMINISTIC)
    p = _plans.get(key)
    if p is None:
        if len(_plans) > 4096:
            _plans.clear()
        p = _plans[key] = _route(ctx, dtype == torch.float32, *key[2:13])
    return p


# one-line readers of the plan and of its rules (tests and tools ask them)
def planeconv_eligible(x, w):
    return plan(x, w.shape, 1, 1, ctx="conv_act", fuse=("plane",), act=True).fwd == "plane"


def conv1x1_small_eligible(x, conv):
    return plan(x, conv.weight.shape, conv.stride, conv.padding, conv.dilation, conv.groups, ctx="conv_act", fuse=("conv1x1",)).fwd == "conv1x1"


def flow_head_eligible(x, weight, bias=None):
    return plan(x, weight.shape, 1, 1, bias=bias is not None, ctx="dense_head").fwd == "flow_head"


def conv_bias_act_eligible(x, conv):
    return plan(x, conv.weight.shape, conv.stride, conv.padding, conv.dilation, conv.groups, conv.bias is not None, True, "conv_act",
                ("wino_act",)).fwd == "wino_act"


def thin_conv3x3_eligible(p, weight):
    return p.is_cuda and _thin(p.dtype == torch.float32, p.is_contiguous(), p.shape, tuple(weight.shape))


def _phase_eligible(x, w, stride, padding, dilation, groups):      # the rule alone: conv2d asks the Winograd kernel first
    return x.is_cuda and groups == 1 and x.dim() == 4 and _phase(x.shape, tuple(w.shape), stride, padding, dilation)


# ------------------------------------------------------------------------------------------------------ executing it
def raw_forward(x, w, stride=(1, 1), padding=(0, 0), dilation=(1, 1), route=None):
    """y = conv(x, w) without bias, fp32 in / fp32 out, no autograd of its own."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    fwd = (route or plan(x, w.shape, stride, padding, dilation, ctx="raw")).fwd
    if fwd == "wino":
        return ops.wino_conv3x3(x, w, padding[0], dilation=dilation[0])
    if fwd == "sconv":
        return ops.sconv_fwd(x, w)
    if fwd == "conv1x1s2":
        return ops.conv1x1s2_fwd(x, w)
    return F.conv2d(x, w, None, stride, padding, dilation)


def raw_backward(gy, x, w, stride=(1, 1), padding=(0, 0), dilation=(1, 1), want_x=True, want_w=True, want_b=False, route=None):
    """(gx, gw, gb) of y = conv(x, w) + b; fp32 in / fp32 out."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    route = route or plan(x, w.shape, stride, padding, dilation, ctx="raw")
    bias_sizes = [int(w.shape[0])] if want_b else None
    d = dilation[0]
    gx = gw = gb = None
    if want_w and route.wgrad == "sconv_wgrad":
        gw = ops.sconv_wgrad(x, gy, int(w.shape[2]), 2, int(w.shape[2]) // 2)
        want_w = False
    if want_w and route.wgrad == "conv1x1s2":
        gw = ops.conv1x1s2_wgrad(x, gy)
        want_w = False
    if want_x and route.dgrad == "sconv":
        gx = ops.sconv_dgrad(gy, w, x.shape)
        want_x = False
    if want_x and route.dgrad == "wino":
        # the data gradient = the same kernel on the transposed filter (full correlation, padding 2, for a valid convolution)
        gx = ops.wino_conv3x3(gy, w, 1 if padding != (0, 0) else 2, transposed=True, dilation=d)
        want_x = False
    if want_w and route.wgrad in ("wino_wgrad", "wgrad3x3"):
        gw = ops.wino_wgrad3x3(x, gy, padding[0] if d == 1 else 1, d) if route.wgrad == "wino_wgrad" else ops.wgrad3x3(x, gy)
        want_w = False
    if DETERMINISTIC and x.is_cuda:
        if want_b:      # a bias gradient alone never goes through aten::convolution_backward: the epilogue's fixed-order reduction
            gb = ops._bias_act_bwd(gy, gy, 1.0, True)[1]
            want_b = False
        if want_x or want_w:
            raise DfeError("deterministic mode: no kernel of this build takes the %s of the convolution of x %s with w %s, stride %s, "
                           "padding %s, dilation %s" % ("data gradient" if want_x else "weight gradient", tuple(x.shape), tuple(w.shape),
                                                        stride, padding, dilation))
    if want_x or want_w or want_b:
        r = _cb(gy, x, w, bias_sizes, list(stride), list(padding), list(dilation), False, [0, 0], 1, [want_x, want_w, want_b])
        gx = r[0] if want_x else gx
        gw = r[1] if want_w else gw
        gb = r[2] if want_b else gb
    return gx, gw, gb


class _RawConvFn(torch.autograd.Function):
    """A routed fp32 layer as one autograd node over raw_forward / raw_backward.  With ``route.fwd`` "wino_act" it is
    ``act(conv(x, w) + bias)`` -- net_utils.conv() = Conv2d + LeakyReLU(0.1): FeaturePyramid's stride-1 layers, PWC's context
    network -- as ONE launch forward (the epilogue inside the Winograd kernel's output transform); its backward is
    dfe_bias_act_bwd (gz = gy act'(y), bias gradient) in front of the convolution's data / weight gradients."""

    @staticmethod
    def forward(ctx, x, w, stride, padding, dilation, route, bias=None, slope=1.0):
        ctx.cfg = (stride, padding, dilation, route, float(slope), bias is not None)
        if route.fwd not in ("wino_act", "sconv_act"):
            ctx.save_for_backward(x, w)
            return raw_forward(x, w, stride, padding, dilation, route)
        if route.fwd == "sconv_act":
            y = ops.sconv_fwd(x, w, bias, slope)
        else:
            y = ops.wino_conv3x3(x, w, padding[0], dilation=dilation[0], bias=bias, slope=slope)
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors[:2]
        stride, padding, dilation, route, slope, has_bias = ctx.cfg
        gb = None
        if route.fwd in ("wino_act", "sconv_act"):
            gy, gb = ops._bias_act_bwd(ctx.saved_tensors[2], gy if ops._dense_chw(gy) else f32c(gy), slope, has_bias and ctx.needs_input_grad[6])
        gx, gw, _ = raw_backward(gy.contiguous(), x, w, stride, padding, dilation, ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                 route=route)
        return gx, gw, None, None, None, None, gb, None


def _phase_conv(x, w, d):
    B, C, H, W = x.shape
    ys = conv2d(ops.phase_images(x, d), w, None, 1, 1, 1)
    return ys.view(B, d, d, w.shape[0], H // d, W // d).permute(0, 3, 4, 1, 5, 2).reshape(B, w.shape[0], H, W)


def _run(route, x, w, bias, stride, padding, dilation, groups):
    """Execute a plan whose forward is "miopen", "wino" or "phase"; a bias is added to a routed layer's output."""
    if route == MIOPEN:
        return F.conv2d(x, w, bias, stride, padding, dilation, groups)
    y = _phase_conv(x, w, dilation[0]) if route.fwd == "phase" else _RawConvFn.apply(x, w, stride, padding, dilation, route)
    return y if bias is None else y + bias.view(1, -1, 1, 1)


def conv2d(x, w, bias=None, stride=1, padding=0, dilation=1, groups=1):
    """``F.conv2d`` with this build's kernels where they are eligible (fp32 HIP tensors, groups == 1)."""
    stride, padding, dilation = _pair(stride), _pair(padding), _pair(dilation)
    return _run(plan(x, w.shape, stride, padding, dilation, groups), x, w, bias, stride, padding, dilation, groups)


def conv3x3_valid(p, weight):
    """3x3 convolution without padding or bias of a pre-padded activation (the decoder's ConvBlock convolutions): on the thin
    full-resolution layers (at most 32 output channels at >= 64x208 pixels) the weight gradient always takes a kernel of this build."""
    return _run(plan(p, weight.shape, ctx="prepadded"), p, weight, None, (1, 1), (0, 0), (1, 1), 1)


class Conv2d(nn.Conv2d):
    """nn.Conv2d (same parameters and state-dict keys) whose forward goes through the plan."""

    def forward(self, x):
        if self.padding_mode != "zeros" or isinstance(self.padding, str):
            return super().forward(x)
        route = plan(x, self.weight.shape, self.stride, self.padding, self.dilation, self.groups, self.bias is not None, ctx="module")
        if route.fwd == "flow_head":                   # PWC's flow heads (pwc_tf.py:39-40): rolling-window HIP kernels
            return ops.FlowHeadFn.apply(x, self.weight, self.bias)
        return _run(route, x, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups)


def conv_bias_act(x, conv, slope):
    return conv_act(x, conv, slope, ("wino_act",))      # the fused epilogue where ``conv_bias_act_eligible``


def conv_act(x, conv, slope, fuse=("plane", "wino_act", "conv1x1", "sconv_act")):
    """``act(conv(x))`` of an nn.Conv2d on the GPU, act(v) = v > 0 ? v : slope v (slope 1: no activation): one fused kernel where
    the plan names one of ``fuse``; otherwise the convolution runs without its bias and the bias + activation epilogue is one
    in-place HIP pass whose backward also yields the bias gradient (ops.bias_act) -- or, with no activation to apply, the
    module's own forward."""
    act = float(slope) != 1.0
    route = plan(x, conv.weight.shape, conv.stride, conv.padding, conv.dilation, conv.groups, conv.bias is not None, act, "conv_act", fuse)
    if route.fwd == "plane":
        return ops.planeconv_act(x, conv.weight, conv.bias, slope)
    if route.fwd in ("wino_act", "sconv_act"):
        return _RawConvFn.apply(x, conv.weight, conv.stride, conv.padding, conv.dilation, route, conv.bias, float(slope))
    if route.fwd == "conv1x1":
        return ops.conv1x1_small(x, conv, slope)
    if not act:
        return conv(x)
    return ops.bias_act(_run(route, x, conv.weight, None, conv.stride, conv.padding, conv.dilation, conv.groups), conv.bias, slope)


class DenseDecodeFn(torch.autograd.Function):
    """One PWC decoder level's DenseNet-style block (pwc_tf.py:113-118 and the same six lines per level)::

        x0 = conv_0(x); x1 = conv_1(x0); x2 = conv_2(cat(x0, x1)); x3 = conv_3(cat(x1, x2)); x4 = conv_4(cat(x2, x3))
        flow = predict_flow(cat(x3, x4))                                      -> (flow, x4)

    with every ``conv_k`` = Conv2d(3x3, pad 1, bias) + LeakyReLU(slope).  The convolutions are planned layer by layer (bias-free);
    the bias + activation epilogue writes each layer output straight into the channel slices of the two concatenated
    buffers that consume it (``dfe_bias_act_fwd2``, or the kernel's own epilogue), so no ``torch.cat`` copies exist; the backward
    pass goes layer by layer and the epilogue's backward sums the two consumers' gradient slices in place
    (``dfe_bias_act_bwd2``): no slice copies, no gradient-accumulation adds.  Same arithmetic as the composition."""

    @staticmethod
    def forward(ctx, slope, x, *wb):
        lib = get_lib()
        x = f32c(x)
        w, b = list(wb[0:12:2]), list(wb[1:12:2])          # conv_0..conv_4, predict_flow
        B, _, H, W = x.shape
        co = [int(t.shape[0]) for t in w[:5]]              # 128, 128, 96, 64, 32
        dev = x.device
        cat = [torch.empty(B, co[k] + co[k + 1], H, W, device=dev, dtype=torch.float32) for k in range(4)]   # [x_k | x_k+1]
        st = stream_ptr()

        # levels 6 / 5: the convolution and its epilogue are this build's small-plane kernels; decided once per block, from its first layer
        plane = plan(x, w[0].shape, (1, 1), (1, 1), bias=True, act=True, ctx="dense").fwd == "plane"

        def layer(inp, k, d1, d1_off, d2, d2_off):
            """act(conv_k(inp) + b_k) into channels d1_off.. of d1 (None: a fresh tensor, returned) and d2_off.. of d2"""
            route = plan(inp, w[k].shape, (1, 1), (1, 1), bias=True, act=True, ctx="dense", plane=plane)
            if route.fwd == "plane":
                d1 = torch.empty(B, co[k], H, W, device=dev, dtype=torch.float32) if d1 is None else d1
                ops.planeconv_fwd_into(inp, w[k], b[k], slope, d1, d1_off, d2, d2_off)
                return d1
            if route.fwd == "wino_act":      # round 5: the epilogue inside the Winograd kernel's output transform (one launch, no pass over z)
                return ops.wino_conv3x3(inp, w[k], 1, bias=b[k], slope=slope, out=d1, out_off=d1_off, out2=d2, out2_off=d2_off)
            z = raw_forward(inp, w[k], 1, 1, route=route)
            d1 = z if d1 is None else d1
            check(lib.dfe_bias_act_fwd2(ptr(z), ptr(b[k]), ops._chan_ptr(d1, d1_off), d1.stride(0), ops._chan_ptr(d2, d2_off),
                                        d2.stride(0) if d2 is not None else 0, B, co[k], H, W, slope, st), "dfe_bias_act_fwd2")
            return z
        z0 = layer(x, 0, None, 0, cat[0], 0)                                # x0: conv_1's input + cat0[:, :128]
        layer(z0, 1, cat[0], co[0], cat[1], 0)                              # x1
        layer(cat[0], 2, cat[1], co[1], cat[2], 0)                          # x2
        layer(cat[1], 3, cat[2], co[2], cat[3], 0)                          # x3
        x4 = layer(cat[2], 4, None, 0, cat[3], co[3])                       # x4: returned + cat3[:, 64:]
        head = plan(cat[3], w[5].shape, (1, 1), (1, 1), bias=b[5] is not None, ctx="dense_head").fwd
        if head == "flow_head":
            flow = ops.flow_head_fwd_raw(cat[3], f32c(w[5]), f32c(b[5]))
        elif head == "wino":        # the deterministic mode with the head kernels switched off
            flow = ops.wino_conv3x3(cat[3], w[5], 1, bias=b[5])
        else:
            flow = F.conv2d(cat[3], w[5], b[5], 1, 1)
        ctx.save_for_backward(x, z0, *cat, *w)
        ctx.slope, ctx.co, ctx.plane = slope, co, plane
        ctx.set_materialize_grads(False)
        return flow, x4

    @staticmethod
    def backward(ctx, g_flow, g_x4):
        lib = get_lib()
        saved = ctx.saved_tensors
        x, x0, cat, w = saved[0], saved[1], list(saved[2:6]), list(saved[6:12])
        co, slope = ctx.co, ctx.slope
        B, _, H, W = x.shape
        dev = x.device
        st = stream_ptr()
        need = ctx.needs_input_grad          # (slope, x, w0, b0, ..., wp, bp)
        nw = lambda k: bool(need[2 + 2 * k])
        nb = lambda k: bool(need[3 + 2 * k])
        def cb(g, inp, wt, want_in, want_w, bias_sizes=None, want_b=False):
            if ctx.plane and not want_b:
                return ops.planeconv_backward(g, inp, wt, want_in, want_w) + (None,)
            return raw_backward(g, inp, wt, 1, 1, 1, want_in, want_w, want_b)

        def epilogue_bwd(k, ysrc, y_off, g1, g1_off, g2, g2_off):
            c = co[k]
            gz = torch.empty(B, c, H, W, device=dev, dtype=torch.float32)
            gb = part = None
            if nb(k):       # only the per-block partial sums now; the level's bias gradients are finished by ONE launch below
                gb = torch.empty(c, device=dev, dtype=torch.float32)
                part = torch.empty(lib.dfe_bias_act_partials_floats(B, c, H, W), device=dev, dtype=torch.float32)
                pending.append((part, gb, c))
            check(lib.dfe_bias_act_bwd2(ops._chan_ptr(ysrc, y_off), ysrc.stride(0), ops._chan_ptr(g1, g1_off), g1.stride(0),
                                        ops._chan_ptr(g2, g2_off), g2.stride(0) if g2 is not None else 0,
                                        ptr(gz), None, ptr(part), B, c, H, W, slope, st), "dfe_bias_act_bwd2")
            return gz, gb

        pending, gw, gbias = [], [None] * 6, [None] * 6
        if g_flow is not None:
            g_flow = f32c(g_flow)
            if plan(cat[3], w[5].shape, (1, 1), (1, 1), bias=True, ctx="dense_head").fwd == "flow_head":
                g3, gw[5], gbias[5] = ops.flow_head_bwd_raw(cat[3], f32c(w[5]), g_flow, nw(5), nb(5))
            else:
                g3, gw[5], gbias[5] = cb(g_flow, cat[3], w[5], True, nw(5), [2], nb(5))       # d/d cat(x3, x4)
        else:
            g3 = torch.zeros_like(cat[3])
        if g_x4 is not None and not ops._dense_chw(g_x4):     # usually a channel slice of the gradient of torch.cat([flow, x4]): read in place
            g_x4 = f32c(g_x4)
        gz, gbias[4] = epilogue_bwd(4, cat[3], co[3], g3, co[3], g_x4, 0)                 # x4: cat3 slice + the returned copy
        g2, gw[4], _ = cb(gz, cat[2], w[4], True, nw(4))                                  # d/d cat(x2, x3)
        gz, gbias[3] = epilogue_bwd(3, cat[3], 0, g3, 0, g2, co[2])                       # x3
        g1, gw[3], _ = cb(gz, cat[1], w[3], True, nw(3))                                  # d/d cat(x1, x2)
        gz, gbias[2] = epilogue_bwd(2, cat[2], 0, g2, 0, g1, co[1])                       # x2
        g0, gw[2], _ = cb(gz, cat[0], w[2], True, nw(2))                                  # d/d cat(x0, x1)
        gz, gbias[1] = epilogue_bwd(1, cat[1], 0, g1, 0, g0, co[0])                       # x1
        gx0, gw[1], _ = cb(gz, x0, w[1], True, nw(1))                                     # d/d x0 through conv_1
        gz, gbias[0] = epilogue_bwd(0, cat[0], 0, g0, 0, gx0, 0)                          # x0
        if pending:
            n = len(pending)
            parts = (ctypes.c_void_p * n)(*[t[0].data_ptr() for t in pending])
            outs = (ctypes.c_void_p * n)(*[t[1].data_ptr() for t in pending])
            chans = (ctypes.c_int * n)(*[t[2] for t in pending])
            check(lib.dfe_bias_grad_final_multi(parts, outs, chans, n, B, H, W, st), "dfe_bias_grad_final_multi")
        gx, gw[0], _ = cb(gz, x, w[0], bool(need[1]), nw(0))
        return (None, gx) + tuple(t for k in range(6) for t in (gw[k], gbias[k]))


def dense_decode(x, layers, predict_flow, slope=0.1):
    """(flow, x4) of one PWC decoder level; ``layers``: the five Conv2d modules, ``predict_flow``: the 3x3 flow head."""
    return DenseDecodeFn.apply(float(slope), x, *[t for c in list(layers) + [predict_flow] for t in (c.weight, c.bias)])
