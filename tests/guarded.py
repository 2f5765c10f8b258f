"""Helpers of the guarded convolution tests (test_hip_conv_guarded.py, test_hip_conv_wgrad_guarded.py,
test_hip_planeconv_guarded.py; self-tests in test_guarded_cpu.py), further down of the glue / head and of the PWC-level tests.
Not a conftest: imported explicitly.

``Carved``: a tensor view inside one int32 buffer pre-filled with a NaN bit pattern, at a chosen float offset past a 16-byte
boundary, with guard bands on both sides and (optionally) sentinel gaps between its samples: a stray store breaks
``intact()``, a stray load that reaches a sum makes the output NaN, an output element nobody wrote stays NaN.

The per-element yardstick: e = |out - ref64| / (2^-24 A) with A the absolute sum of the algorithm that made the element --
sum |a||b| for the direct-sum kernels, the Winograd-domain absolute sum for the Winograd kernels (a 3x3 window of zeros
inside a non-zero 4x4 patch has a direct sum of exactly 0 and a Winograd result that is a rounding residue).  A kernel is
held to 4 x max(1, e of a plain fp32 implementation of the same algorithm on the same inputs): 1 = the final rounding alone,
4 = another association order (MFMA's 4-channel steps, channel / tile splits, transform order) and the spread of a
maximum over a few thousand elements.  A dropped or misplaced product is ~A / (9 Ci): orders of magnitude above."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = 0x7FC5A5A5      # a quiet NaN with a recognisable payload (as int32: positive)
GUARD = 64                 # guard floats on either side of a view (a multiple of 4: the view's alignment is offset_floats)
U24 = 2.0 ** -24
FAMILIES = ("randn", "act", "sparse")


def default_device():
    return torch.device("cuda:0" if torch.cuda.is_available() else "cpu")


class Carved:
    """A view of ``shape`` that starts ``offset_floats`` floats past a 16-byte boundary inside a sentinel-filled buffer.
    shape[0] is the batch: with ``batch_stride`` (floats) above the dense sample size the gaps between the samples are
    sentinel too.  ``fill``: the values (None: the payload keeps the NaN pattern -- outputs and workspaces)."""

    def __init__(self, shape, offset_floats=0, batch_stride=None, fill=None, device=None):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        assert len(shape) >= 1 and all(s > 0 for s in shape) and 0 <= offset_floats < 4
        dense = math.prod(shape[1:])
        bs = dense if batch_stride is None else int(batch_stride)
        assert bs >= dense
        span = (shape[0] - 1) * bs + dense
        total = (GUARD + offset_floats + span + GUARD + 3) // 4 * 4
        dev = default_device() if device is None else device
        self.bits = torch.full((total,), SENTINEL, dtype=torch.int32, device=dev)
        assert self.bits.data_ptr() % 16 == 0
        self.lo, self.span, self.batch_stride = GUARD + offset_floats, span, bs
        strides = [1] * len(shape)
        for i in range(len(shape) - 2, 0, -1):
            strides[i] = strides[i + 1] * shape[i + 1]
        strides[0] = bs
        self.view = self.bits.view(torch.float32).as_strided(shape, strides, self.lo)
        assert self.view.data_ptr() % 16 == 4 * offset_floats
        self.guard = torch.ones(total, dtype=torch.bool, device=dev)
        self.guard.as_strided(shape, strides, self.lo).fill_(False)
        assert int(self.guard.sum()) >= 2 * GUARD + (shape[0] - 1) * (bs - dense)
        if fill is not None:
            self.view.copy_(fill.to(torch.float32).reshape(shape))

    @property
    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        """guards and batch gaps still hold the sentinel bits"""
        return bool((self.bits[self.guard] == SENTINEL).all())

    def untouched(self):
        """the payload still holds the sentinel bits (nothing was written)"""
        return bool((self.bits[~self.guard] == SENTINEL).all())

    def written(self):
        """every payload element was written with a finite value"""
        return bool(torch.isfinite(self.view).all())

    def cpu(self):
        return self.view.detach().cpu().contiguous()


# --------------------------------------------------------------------------------------------------------- inputs
def make_input(shape, family, gen):
    """randn / activation-like relu(randn) + 1 / sparse relu(randn - 1) with a few whole 4x4-aligned blocks (all channels)
    and one whole channel zeroed.  shape [B,C,H,W], CPU fp32."""
    x = torch.randn(shape, generator=gen, dtype=torch.float32)
    if family == "act":
        x = torch.relu(x) + 1.0
    elif family == "sparse":
        x = torch.relu(x - 1.0)
        B, C, H, W = shape
        ylast, xlast = 4 * ((H - 1) // 4), 4 * ((W - 1) // 4)
        for b, y0, x0 in ((0, 0, 0), (B - 1, ylast, xlast), (0, 0, xlast), (B - 1, ylast, 0)):
            x[b, :, y0:y0 + 4, x0:x0 + 4] = 0.0
        x[:, C // 2] = 0.0
    else:
        assert family == "randn"
    return x


def make_weight(Co, Ci, K, gen):
    return torch.randn(Co, Ci, K, K, generator=gen, dtype=torch.float32) / (3.0 * Ci ** 0.5)


# --------------------------------------------------------------------------------------------------------- the bound
def norm_err(out, ref64, A):
    """(max over A > 0 of |out - ref64| / (2^-24 A), whether out is +-0 wherever A == 0)"""
    out = out.detach().double().cpu()
    zero = A == 0
    e = ((out - ref64).abs() / (U24 * A.clamp_min(1e-300)))[~zero]
    return (float(e.max()) if e.numel() else 0.0), bool((out[zero] == 0).all())


def check_bound(tag, out, yard, ref64, A):
    """max e(kernel) <= 4 max(1, max e(yardstick)); prints both figures (pytest -s collects them for the log)"""
    assert out.shape == ref64.shape == yard.shape == A.shape, (tag, out.shape, ref64.shape, yard.shape, A.shape)
    assert bool(torch.isfinite(out).all()), tag
    ek, zk = norm_err(out, ref64, A)
    ey, _ = norm_err(yard, ref64, A)
    print("EBOUND %s kernel %.3f yardstick %.3f" % (tag, ek, ey))
    assert zk, (tag, "non-zero output where the absolute sum is 0")
    assert ek <= 4.0 * max(1.0, ey), (tag, ek, ey)
    return ek, ey


# --------------------------------------------------------------------------------------------------------- direct sums
def conv_ref(x, w, stride, P, dil, dtype):
    return F.conv2d(x.to(dtype), w.to(dtype), None, stride, P, dil)


def conv_dgrad_ref(gy, w, in_shape, stride, P, dil, dtype):
    x0 = torch.zeros(in_shape, dtype=dtype)
    return torch.ops.aten.convolution_backward(gy.to(dtype), x0, w.to(dtype), None, [stride] * 2, [P] * 2, [dil] * 2, False, [0, 0], 1,
                                               [True, False, False])[0]


def conv_wgrad_ref(gy, x, K, stride, P, dil, dtype):
    w0 = torch.zeros(gy.shape[1], x.shape[1], K, K, dtype=dtype)
    return torch.ops.aten.convolution_backward(gy.to(dtype), x.to(dtype), w0, None, [stride] * 2, [P] * 2, [dil] * 2, False, [0, 0], 1,
                                               [False, True, False])[1]


# --------------------------------------------------------------------------------------------------------- Winograd F(2x2, 3x3)
# The matrices and the order of the additions are the kernels' (csrc/ops_wino.hip, csrc/ops_wino_wgrad.hip); every operation is
# one rounding in ``dtype``; the channel (forward) and tile (weight gradient) sums are sequential.
def _bt_d_b(d):            # [..., 4, 4] -> B^T d B
    t = torch.stack([d[..., 0, :] - d[..., 2, :], d[..., 1, :] + d[..., 2, :], d[..., 2, :] - d[..., 1, :], d[..., 1, :] - d[..., 3, :]], -2)
    return torch.stack([t[..., 0] - t[..., 2], t[..., 1] + t[..., 2], t[..., 2] - t[..., 1], t[..., 1] - t[..., 3]], -1)


def _g_g_gt(g):            # [..., 3, 3] -> G g G^T
    r = torch.stack([g[..., 0, :], 0.5 * ((g[..., 0, :] + g[..., 1, :]) + g[..., 2, :]), 0.5 * ((g[..., 0, :] - g[..., 1, :]) + g[..., 2, :]),
                     g[..., 2, :]], -2)
    return torch.stack([r[..., 0], 0.5 * ((r[..., 0] + r[..., 1]) + r[..., 2]), 0.5 * ((r[..., 0] - r[..., 1]) + r[..., 2]), r[..., 2]], -1)


def _at_m_a(m, s):         # [..., 4, 4] -> A^T m A (s = -1) or |A^T| m |A| (s = +1)
    t = torch.stack([(m[..., 0, :] + m[..., 1, :]) + m[..., 2, :], (m[..., 1, :] + s * m[..., 2, :]) + s * m[..., 3, :]], -2)
    return torch.stack([(t[..., 0] + t[..., 1]) + t[..., 2], (t[..., 1] + s * t[..., 2]) + s * t[..., 3]], -1)


def _patches(x, P, TH, TW):
    H, W = x.shape[2:]
    xp = F.pad(x, (P, 2 * TW + 2 - W - P, P, 2 * TH + 2 - H - P))
    return xp.unfold(2, 4, 2).unfold(3, 4, 2)           # [B,C,TH,TW,4,4]


def wino_fwd(x, w, P, dtype, absolute=False):
    """F(2x2, 3x3) convolution of x [B,C,H,W] with w [K,C,3,3], padding P in {0,1,2}.  absolute: the Winograd-domain absolute
    sum S_w = |A^T| [sum_c |G g G^T| (.) |B^T d B|] |A|."""
    x, w = x.to(dtype), w.to(dtype)
    B, C, H, W = x.shape
    K = w.shape[0]
    Ho, Wo = H + 2 * P - 2, W + 2 * P - 2
    TH, TW = (Ho + 1) // 2, (Wo + 1) // 2
    V, U = _bt_d_b(_patches(x, P, TH, TW)), _g_g_gt(w)
    if absolute:
        V, U = V.abs(), U.abs()
    M = torch.zeros(B, K, TH, TW, 4, 4, dtype=dtype)
    for c in range(C):
        M += U[None, :, c, None, None] * V[:, None, c]
    Y = _at_m_a(M, 1.0 if absolute else -1.0)            # [B,K,TH,TW,2,2]
    return Y.permute(0, 1, 2, 4, 3, 5).reshape(B, K, 2 * TH, 2 * TW)[:, :, :Ho, :Wo].contiguous()


def to_phases(x, d):
    B, C, H, W = x.shape
    return x.reshape(B, C, H // d, d, W // d, d).permute(0, 3, 5, 1, 2, 4).reshape(B * d * d, C, H // d, W // d)


def from_phases(y, d, B):
    _, C, Hq, Wq = y.shape
    return y.reshape(B, d, d, C, Hq, Wq).permute(0, 3, 4, 1, 5, 2).reshape(B, C, Hq * d, Wq * d).contiguous()


def wino_conv(x, w, P, dil, transposed, dtype, absolute=False):
    """what dfe_wino_conv3x3* computes: transposed = the data-gradient form on the forward filter w [C,K,3,3]; dil > 1: on
    the phase images with padding 1"""
    if transposed:
        w = w.transpose(0, 1).flip(2, 3)
    if dil == 1:
        return wino_fwd(x, w, P, dtype, absolute)
    return from_phases(wino_fwd(to_phases(x, dil), w, 1, dtype, absolute), dil, x.shape[0])


def wino_conv_ref64(x, w, P, dil, transposed):
    if transposed:
        w = w.transpose(0, 1).flip(2, 3)
    return F.conv2d(x.double(), w.double(), None, 1, dil if dil > 1 else P, dil)


def wino_wgrad(x, gy, P, dtype, absolute=False):
    """F(3x3, 2x2)-form weight gradient: G^T [sum_tiles (A dY A^T) (.) (B^T d B)] G with A = [[1,0],[1,1],[1,-1],[0,-1]]; as in
    the kernel the signs of A's last row are applied after the tile sum (negation is exact)."""
    x, gy = x.to(dtype), gy.to(dtype)
    B, C, H, W = x.shape
    K, Ho, Wo = gy.shape[1:]
    assert (Ho, Wo) == (H + 2 * P - 2, W + 2 * P - 2)
    TH, TW = (Ho + 1) // 2, (Wo + 1) // 2
    V = _bt_d_b(_patches(x, P, TH, TW))                                      # [B,C,TH,TW,4,4]
    g = F.pad(gy, (0, 2 * TW - Wo, 0, 2 * TH - Ho)).unfold(2, 2, 2).unfold(3, 2, 2)      # [B,K,TH,TW,2,2]
    r0, r1 = g[..., 0, :], g[..., 1, :]
    a = torch.stack([r0, r0 + r1, r0 - r1, r1], -2)                          # [...,4,2]
    m = torch.stack([a[..., 0], a[..., 0] + a[..., 1], a[..., 0] - a[..., 1], a[..., 1]], -1)
    if absolute:
        V, m = V.abs(), m.abs()
    acc = torch.zeros(K, C, 4, 4, dtype=dtype)
    for b in range(B):
        for ty in range(TH):
            for tx in range(TW):
                acc += m[b, :, ty, tx][:, None] * V[b, :, ty, tx][None]
    s = 1.0
    if not absolute:
        s = -1.0
        sign = torch.ones(4, 4, dtype=dtype)
        sign[3, :3] = -1.0
        sign[:3, 3] = -1.0
        acc = acc * sign
    u = acc
    tm = torch.stack([u[..., 0, :] + 0.5 * (u[..., 1, :] + u[..., 2, :]), 0.5 * (u[..., 1, :] + s * u[..., 2, :]),
                      0.5 * (u[..., 1, :] + u[..., 2, :]) + u[..., 3, :]], -2)                      # [K,C,3,4]
    return torch.stack([tm[..., 0] + 0.5 * (tm[..., 1] + tm[..., 2]), 0.5 * (tm[..., 1] + s * tm[..., 2]),
                        0.5 * (tm[..., 1] + tm[..., 2]) + tm[..., 3]], -1).contiguous()             # [K,C,3,3]


def leaky(v, slope):
    return torch.where(v > 0, v, v * slope)


# ========================================================================================================= glue and head kernels
# Helpers of test_hip_glue_guarded.py and test_hip_head_guarded.py: a byte carve, float64 references (``dtype`` = float64) and
# fp32 yardsticks (the same expression with ``dtype`` = float32, run by ATen on the host), absolute-sum companions A, the margin
# every thresholded decision keeps, and plain restatements of the launchers' branch rules (csrc/ops_decoder.hip,
# ops_epilogue.hip, ops_bn.hip, ops_disphead.hip) so that a test can say which kernel a case runs.
BYTE_SENTINEL = 0xA5       # not a window position (0..8)
BYTE_GUARD = 64
MARGIN = 64 * U24          # a decision's distance from its threshold, in units of its absolute sum


class CarvedBytes:
    """``Carved`` for a dense uint8 view (the window positions of the max pooling): ``offset_bytes`` past a 16-byte boundary."""

    def __init__(self, shape, offset_bytes=0, device=None):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        assert all(s > 0 for s in shape) and 0 <= offset_bytes < 16
        n = math.prod(shape)
        total = (BYTE_GUARD + offset_bytes + n + BYTE_GUARD + 15) // 16 * 16
        dev = default_device() if device is None else device
        self.bits = torch.full((total,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
        assert self.bits.data_ptr() % 16 == 0
        self.lo, self.span = BYTE_GUARD + offset_bytes, n
        self.view = self.bits[self.lo:self.lo + n].view(shape)
        self.guard = torch.ones(total, dtype=torch.bool, device=dev)
        self.guard[self.lo:self.lo + n] = False

    @property
    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.bits[self.guard] == BYTE_SENTINEL).all())

    def untouched(self):
        return bool((self.bits[~self.guard] == BYTE_SENTINEL).all())

    def written(self):
        """every byte is a window position"""
        return bool((self.view <= 8).all())

    def cpu(self):
        return self.view.detach().cpu().contiguous()


def bits_equal(a, b):
    """bit for bit (NaN payloads and the sign of zero included)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def margin_ok(value64, A):
    """every decision ``value > 0`` of the float64 reference is at least MARGIN * A away from its threshold"""
    return bool((value64.abs() >= MARGIN * A).all())


def _bc(t, dtype):
    return 0.0 if t is None else t.to(dtype)[None, :, None, None]


def _abc(t):
    return 0.0 if t is None else t.double().abs()[None, :, None, None]


def vjp(fn, in_shape, g, dtype):
    """the adjoint of the linear map fn applied to g"""
    v = torch.zeros(in_shape, dtype=dtype, requires_grad=True)
    return torch.autograd.grad(fn(v), v, g.to(dtype))[0]


# --------------------------------------------------------------------------------------------------------- epilogue
def away_from_zero(shape, gen, scale=1.0):
    """randn with every |value| >= 2^-10"""
    t = torch.randn(shape, generator=gen, dtype=torch.float32) * scale
    return torch.where(t.abs() < 2.0 ** -10, torch.full_like(t, 2.0 ** -10).copysign(t), t)


def bias_act_ref(z, bias, slope, dtype):
    return leaky(z.to(dtype) + _bc(bias, dtype), slope)


def bias_act_A(z, bias):
    return z.double().abs() + _abc(bias)


def bias_act_bwd_ref(y, g, slope):
    """exact in the gradient's own type: one selection, one product"""
    return torch.where(y > 0, g, g * slope)


def plane_sums(v, dtype):
    """[B,C,H,W] -> [C]"""
    return v.to(dtype).sum((0, 2, 3))


# --------------------------------------------------------------------------------------------------------- decoder glue
def elu_ref(v):
    return torch.where(v > 0, v, torch.expm1(v))


def elu_slope_ref(v):
    return torch.where(v > 0, torch.ones_like(v), torch.exp(v))


def pad1(v):
    return F.pad(v, (1, 1, 1, 1), mode="reflect")


def up2(v):
    return F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)


def elu_A(x, bias):
    """ELU value and slope pass through the hardware exponential: |x| + |b| + 1"""
    return x.double().abs() + _abc(bias) + 1.0


def elu_pad_ref(x, bias, apply_elu, dtype):
    v = x.to(dtype) + _bc(bias, dtype)
    return pad1(elu_ref(v) if apply_elu else v)


def elu_pad_bwd_ref(x, bias, gout, apply_elu, dtype, absolute=False):
    """gx = pad1^T(gout) * elu'(x + bias); absolute: pad1^T(|gout|) * (|x| + |b| + 1) (or * 1 without the ELU)"""
    B, C, Hp, Wp = gout.shape
    shape = (B, C, Hp - 2, Wp - 2)
    if absolute:
        g = vjp(pad1, shape, gout.abs(), torch.float64)
        return g * elu_A(x, bias) if apply_elu else g
    g = vjp(pad1, shape, gout, dtype)
    return g * elu_slope_ref(x.to(dtype) + _bc(bias, dtype)) if apply_elu else g


def up2_cat_pad_ref(x, bias, skip, dtype):
    v = up2(elu_ref(x.to(dtype) + _bc(bias, dtype)))
    return pad1(v if skip is None else torch.cat([v, skip.to(dtype)], 1))


def up2_cat_pad_A(x, bias):
    """of the C1 interpolated channels (the skip channels are copies)"""
    return pad1(up2(elu_A(x, bias)))


def up2_cat_pad_bwd_ref(x, bias, gout, dtype, absolute=False):
    """(gx, gskip or None): gx = (pad1 . up2)^T(gout[:, :C1]) * elu'(x + bias), gskip = pad1^T(gout[:, C1:])"""
    B, C1, h, w = x.shape
    C2 = gout.shape[1] - C1
    g = gout.abs().double() if absolute else gout.to(dtype)
    dt = torch.float64 if absolute else dtype
    gv = vjp(lambda v: pad1(up2(v)), x.shape, g[:, :C1], dt)
    gx = gv * (elu_A(x, bias) if absolute else elu_slope_ref(x.to(dtype) + _bc(bias, dtype)))
    gskip = vjp(pad1, (B, C2, 2 * h, 2 * w), g[:, C1:], dt) if C2 else None
    return gx, gskip


# --------------------------------------------------------------------------------------------------------- grouped batch norm
def bn_fwd_ref(x, res, weight, bias, rmean, rvar, G, Bg, eps, momentum, relu):
    """float64.  Returns a dict: pre (before the ReLU), y, mean, invstd [G*C], rmean, rvar [C] after the G updates in group order,
    and the companions A_* (A_y includes the cancellation in x - mean: (|x| + mean|x|) invstd |w| + |b| + |res|)."""
    N, C, H, W = x.shape
    assert N == G * Bg
    xg = x.double().view(G, Bg, C, H, W)
    n = Bg * H * W
    mean = xg.mean((1, 3, 4), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3, 4), keepdim=True)
    invstd = 1.0 / torch.sqrt(var + eps)
    w = torch.ones(C, dtype=torch.float64) if weight is None else weight.double()
    b = torch.zeros(C, dtype=torch.float64) if bias is None else bias.double()
    r = torch.zeros_like(xg) if res is None else res.double().view(G, Bg, C, H, W)
    pre = (xg - mean) * invstd * w[None, None, :, None, None] + b[None, None, :, None, None] + r
    amean = xg.abs().mean((1, 3, 4), keepdim=True)
    xa = xg.abs() + amean
    A_y = xa * invstd * w.abs()[None, None, :, None, None] + b.abs()[None, None, :, None, None] + r.abs()
    A_var = (xa ** 2).mean((1, 3, 4))                                        # [G,C]: d^2 with d = x - mean rounded at |x| + mean|x|
    unb = n / (n - 1.0) if n > 1 else 1.0
    rm = torch.zeros(C, dtype=torch.float64) if rmean is None else rmean.double().clone()
    rv = torch.zeros(C, dtype=torch.float64) if rvar is None else rvar.double().clone()
    A_rm, A_rv = rm.abs(), rv.abs()
    for g in range(G):
        rm = (1.0 - momentum) * rm + momentum * mean[g, 0, :, 0, 0]
        rv = (1.0 - momentum) * rv + momentum * var[g, 0, :, 0, 0] * unb
        A_rm = (1.0 - momentum) * A_rm + momentum * amean[g, 0, :, 0, 0]
        A_rv = (1.0 - momentum) * A_rv + momentum * A_var[g] * unb
    flat = lambda t: t.reshape(G * C)
    return dict(pre=pre.view(N, C, H, W), y=(pre.clamp_min(0.0) if relu else pre).view(N, C, H, W), A_y=A_y.view(N, C, H, W),
                mean=flat(mean), A_mean=flat(amean), invstd=flat(invstd), A_invstd=flat(invstd) + 0.5 * flat(invstd) ** 3 * flat(A_var),
                rmean=rm, A_rmean=A_rm, rvar=rv, A_rvar=A_rv)


def bn_fwd_yard(x, res, weight, bias, rmean, rvar, G, Bg, eps, momentum, relu):
    """ATen's fp32 batch norm on the host, group by group.  (y, mean [G*C], invstd [G*C], rmean, rvar)"""
    rm = None if rmean is None else rmean.clone()
    rv = None if rvar is None else rvar.clone()
    ys, ms, iss = [], [], []
    for g in range(G):
        y, m, i = torch.native_batch_norm(x[g * Bg:(g + 1) * Bg], weight, bias, rm, rv, True, momentum, eps)
        ys.append(y), ms.append(m), iss.append(i)
    y = torch.cat(ys, 0)
    if res is not None:
        y = y + res
    return (y.clamp_min(0.0) if relu else y), torch.cat(ms), torch.cat(iss), rm, rv


def bn_bwd_ref(x, y, gy, weight, mean, invstd, G, Bg, relu):
    """float64 on the given inputs (mean / invstd [G*C] as the forward saved them, y the forward's output).  dict: gx, gres,
    gweight, gbias and A_*."""
    N, C, H, W = x.shape
    n = Bg * H * W
    sh = (G, Bg, C, H, W)
    xg, gg = x.double().view(sh), gy.double().view(sh)
    if relu:
        gg = torch.where(y.view(sh) > 0, gg, torch.zeros_like(gg))
    mu, isd = mean.double().view(G, 1, C, 1, 1), invstd.double().view(G, 1, C, 1, 1)
    w = (torch.ones(C, dtype=torch.float64) if weight is None else weight.double())[None, None, :, None, None]
    xh = (xg - mu) * isd
    xa = (xg.abs() + xg.abs().mean((1, 3, 4), keepdim=True)) * isd
    m0, m1 = gg.mean((1, 3, 4), keepdim=True), (gg * xh).mean((1, 3, 4), keepdim=True)
    a0, a1 = gg.abs().mean((1, 3, 4), keepdim=True), (gg.abs() * xa).mean((1, 3, 4), keepdim=True)
    gx = w * isd * (gg - m0 - xh * m1)
    A_gx = w.abs() * isd * (gg.abs() + a0 + xa * a1)
    return dict(gx=gx.view(N, C, H, W), A_gx=A_gx.view(N, C, H, W), gres=gg.view(N, C, H, W), gweight=(gg * xh).sum((0, 1, 3, 4)),
                A_gweight=(gg.abs() * xa).sum((0, 1, 3, 4)), gbias=gg.sum((0, 1, 3, 4)), A_gbias=gg.abs().sum((0, 1, 3, 4)), n=n)


def bn_bwd_yard(x, y, gy, weight, mean, invstd, G, Bg, relu, eps):
    """ATen's fp32 batch-norm backward on the host, group by group.  (gx, gweight, gbias)"""
    g = torch.where(y > 0, gy, torch.zeros_like(gy)) if relu else gy
    C = x.shape[1]
    gxs, gw, gb = [], torch.zeros(C), torch.zeros(C)
    for k in range(G):
        s = slice(k * Bg, (k + 1) * Bg)
        a, b, c = torch.ops.aten.native_batch_norm_backward(g[s].contiguous(), x[s].contiguous(), weight, None, None, mean[k * C:(k + 1) * C].contiguous(),
                                                            invstd[k * C:(k + 1) * C].contiguous(), True, eps, [True, True, True])
        gxs.append(a)
        gw, gb = gw + b, gb + c
    return torch.cat(gxs, 0), gw, gb


def bn_case(G, Bg, C, H, W, relu, with_res, seed, affine=True, eps=1e-5, momentum=0.1):
    """inputs of one batch-norm case whose ReLU decisions keep the margin: the first seed from ``seed`` on (CPU only; a handful
    of tries at these sizes).  dict of fp32 tensors + ref (bn_fwd_ref's dict)."""
    for s in range(seed, seed + 40):
        gen = torch.Generator().manual_seed(s)
        x = torch.randn(G * Bg, C, H, W, generator=gen) * 1.5 + torch.randn(1, C, 1, 1, generator=gen)
        res = torch.randn(G * Bg, C, H, W, generator=gen) if with_res else None
        weight = torch.rand(C, generator=gen) + 0.5 if affine else None
        bias = torch.randn(C, generator=gen) * 0.5 if affine else None
        rmean, rvar = torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5
        gy = torch.randn(G * Bg, C, H, W, generator=gen)
        ref = bn_fwd_ref(x, res, weight, bias, rmean, rvar, G, Bg, eps, momentum, relu)
        if not relu or margin_ok(ref["pre"], ref["A_y"]):
            return dict(x=x, res=res, weight=weight, bias=bias, rmean=rmean, rvar=rvar, gy=gy, ref=ref, seed=s, eps=eps, momentum=momentum)
    raise AssertionError("no seed keeps the ReLU margin")


# --------------------------------------------------------------------------------------------------------- max pooling
def pool_input(planes, H, W, gen):
    """post-ReLU values on a grid of 1/8 (ties are exact ties: tied zeros and tied positives), a few -inf and NaN"""
    x = torch.relu(torch.round(torch.randn(planes, H, W, generator=gen) * 8.0) / 8.0)
    flat = x.view(-1)
    n = flat.numel()
    k = max(1, n // 37)
    pos = torch.randperm(n, generator=gen)
    flat[pos[:k]] = float("-inf")
    flat[pos[k:k + max(1, n // 61)]] = float("nan")
    return x


def pool_ref(x, gy):
    """F.max_pool2d(3, 2, 1) of x [planes,H,W] on the host: (y, gx, window position 0..8 of every output)"""
    planes, H, W = x.shape
    xr = x[None].clone().requires_grad_(True)
    y, ind = F.max_pool2d(xr, 3, 2, 1, return_indices=True)
    gx = torch.autograd.grad(y, xr, gy[None])[0][0]
    ind = ind[0]
    Ho, Wo = ind.shape[1:]
    oy, ox = torch.arange(Ho)[None, :, None], torch.arange(Wo)[None, None, :]
    pos = (ind // W - (2 * oy - 1)) * 3 + (ind % W - (2 * ox - 1))
    return y[0].detach(), gx, pos


# --------------------------------------------------------------------------------------------------------- heads
def disp_head_ref(p, w, bias, dtype, absolute=False):
    if absolute:
        return 0.25 * F.conv2d(p.double().abs(), w.double().abs()) + (0.0 if bias is None else 0.25 * bias.double().abs()[None, :, None, None]) + 1.0
    return torch.sigmoid(F.conv2d(p.to(dtype), w.to(dtype), None if bias is None else bias.to(dtype)))


def disp_head_bwd_ref(p, w, out, gout, dtype, absolute=False):
    """(gp, gweight, gbias) on the given out: g = gout * out * (1 - out)"""
    g = gout.to(dtype) * (out.to(dtype) * (1.0 - out.to(dtype)))
    if absolute:
        g, p, w, dtype = g.double().abs(), p.abs(), w.abs(), torch.float64
    return (conv_dgrad_ref(g, w, p.shape, 1, 0, 1, dtype), conv_wgrad_ref(g, p, 3, 1, 0, 1, dtype), g.to(dtype).sum((0, 2, 3)))


def flow_head_ref(x, w, bias, dtype, absolute=False):
    if absolute:
        return F.conv2d(x.double().abs(), w.double().abs(), None if bias is None else bias.double().abs(), 1, 1)
    return F.conv2d(x.to(dtype), w.to(dtype), None if bias is None else bias.to(dtype), 1, 1)


def flow_head_bwd_ref(x, w, gout, dtype, absolute=False):
    if absolute:
        x, w, gout, dtype = x.abs(), w.abs(), gout.abs(), torch.float64
    return (conv_dgrad_ref(gout, w, x.shape, 1, 1, 1, dtype), conv_wgrad_ref(gout, x, 3, 1, 1, 1, dtype), gout.to(dtype).sum((0, 2, 3)))


# --------------------------------------------------------------------------------------------------------- launch rules
# Offsets are in floats past a 16-byte boundary: 8-byte aligned iff even, 16-byte aligned iff a multiple of 4.
def _a8(off):
    return off % 2 == 0


def _a16(off):
    return off % 4 == 0


def rule_elu_pad_fwd(W, out_off):
    return "pair" if W % 2 == 0 and W >= 4 and _a8(out_off) else "scalar"


def rule_elu_pad_bwd(W, gx_off, x_off, apply_elu):
    if W % 4 == 0 and W >= 8 and _a16(gx_off) and (not apply_elu or _a16(x_off)):
        return "quad"
    if W % 2 == 0 and W >= 4 and _a8(gx_off) and (not apply_elu or _a8(x_off)):
        return "pair"
    return "scalar"


def rule_up2_fwd(w, out_off):
    return "pair" if w >= 2 and _a8(out_off) else "scalar"


def rule_up2_bwd(h, w, gout_off):
    """{'tile32', 'tile64', 'tile64-inner', 'element', 'element-interior'}: what the gradient wrt x runs through"""
    nb = (h * w + 255) // 256
    tw = 32 if w <= 32 else 64
    tx, ty = (w + tw - 1) // tw, (h + 15) // 16
    if _a8(gout_off) and tx * ty <= nb:
        out = {"tile%d" % tw}
        for i0 in range(0, h, 16):
            for j0 in range(0, w, tw):
                if i0 >= 2 and i0 + 16 <= h - 2 and j0 >= 2 and j0 + tw <= w - 2:
                    out.add("tile%d-inner" % tw)
        return out
    return {"element", "element-interior"} if h >= 5 and w >= 5 else {"element"}


def up2_bwd_blocks(h, w, gout_off):
    """partial sums per plane the launcher finishes"""
    nb = (h * w + 255) // 256
    tw = 32 if w <= 32 else 64
    t = ((w + tw - 1) // tw) * ((h + 15) // 16)
    return t if _a8(gout_off) and t <= nb else nb


def rule_skip(w, gskip_off):
    if w % 2 == 0 and w >= 4 and _a16(gskip_off):
        return "quad"
    return "pair" if w >= 2 and _a8(gskip_off) else "scalar"


def rule_epilogue_vec(hw, offs, strides):
    """offs: the offsets of the pointers given (None skipped); strides: the batch strides of the strided ones"""
    return hw % 4 == 0 and all(_a16(o) for o in offs if o is not None) and all(s % 4 == 0 for s in strides if s is not None)


EP_CHUNK = 2048
BN_CHUNK = 2048


def rule_bn(G, Bg, hw, offs):
    """('small', GB, T) / ('three', 'vec') / ('three', 'scalar'); offs: the offsets of the tensors the launcher looks at"""
    vec = hw % 4 == 0 and all(_a16(o) for o in offs if o is not None)
    if vec and hw <= 4096 and Bg <= 4:
        return ("small", 3 if G == 3 else 1, 64 if hw <= 256 else 256 if hw <= 1024 else 1024)
    return ("three", "vec" if vec else "scalar")


def rule_head_fwd(B, C, H, W, flow):
    """dict(par, R, ns, nrb): the forward plan of the disparity (flow=False) / flow head"""
    ns = (W + 61) // 62
    if flow and 4 <= C // 8 <= 16:
        return dict(par=True, R=4, ns=ns, nrb=(H + 3) // 4)
    R = 16
    while R > 2 and B * ns * ((H + R - 1) // R) < 2048:
        R //= 2
    return dict(par=False, R=R, ns=ns, nrb=(H + R - 1) // R)


def rule_head_bwd(C, H, W, flow):
    """dict(ns, nrb, nz) of the backward grid (strips and 16-row blocks of the PADDED plane)"""
    return dict(ns=(W + 2 + 61) // 62, nrb=(H + 2 + 15) // 16, nz=C // (8 if flow else 16))


# --------------------------------------------------------------------------------------------------------- inputs with margins
def epilogue_input(shape, seed):
    """(z, bias): z = t - bias with |t| >= 2^-10, so the sign of z + bias is decided ~2^-10 away from zero"""
    gen = torch.Generator().manual_seed(seed)
    bias = torch.randn(shape[1], generator=gen) * 0.5
    return away_from_zero(shape, gen) - bias[None, :, None, None], bias


def elu_input(shape, with_bias, seed):
    """(x, bias or None): x + bias = t with |t| >= 2^-10 (the ELU branch), |t| up to ~6"""
    gen = torch.Generator().manual_seed(seed)
    bias = torch.randn(shape[1], generator=gen) * 0.5 if with_bias else None
    t = away_from_zero(shape, gen, 2.0)
    return (t - bias[None, :, None, None] if with_bias else t), bias


def bn_seed(case, with_res):
    return 1000 * sum(case[:5]) + 500 * int(with_res)


# ========================================================================================================= PWC decoder level
# Helpers of test_hip_corr_guarded.py, test_hip_warp_guarded.py and test_hip_pwc_level_guarded.py (cases: tests/pwc_cases.py):
# the cost volume and its two gradients as direct sums (float64 reference, absolute sum, plain fp32 in channel / displacement
# order), the feature warp from a numpy-float32 restatement of flow_coords and make_tap (csrc/dfe_device.h) whose weights are
# then exact inputs of float64 sums, the bound of the fixed-point scatter, a device-side bit comparison and the three one-line
# launch rules of csrc/ops_basic.hip.  The two tiling functions of csrc/ops_corr.hip are NOT restated: dfe_corr_fwd_plan /
# dfe_corr_bwd_plan answer for them.
CR_D, CR_K, CR_NK = 4, 9, 81
FWD_PLAN = ("TH", "TXQ", "ntx", "KS", "CC", "DYG", "PF2", "threads", "lds", "chunks", "coarse", "vec")
BWD_PLAN = ("TH", "TXQ", "ntx", "NCG", "ncr", "IS", "threads", "lds", "batches", "vec")
FLOW_KINDS = ("smooth", "rough", "out", "zero", "collapse")


def corr_plan(lib, shape, vec=1, sides=None):
    """the launcher's own decision: dict of FWD_PLAN (sides None) or BWD_PLAN"""
    import ctypes
    names = FWD_PLAN if sides is None else BWD_PLAN
    buf = (ctypes.c_int * len(names))()
    rc = lib.dfe_corr_fwd_plan(*shape, int(vec), buf) if sides is None else lib.dfe_corr_bwd_plan(*shape, int(sides), int(vec), buf)
    assert rc == 0, (shape, sides, rc)
    return dict(zip(names, buf))


def rule_corr_vec(W, offs, strides=()):
    """launch_corr_fwd / launch_corr_bwd: every pointer looked at on 16 bytes, every batch stride a multiple of 4 floats"""
    return W % 4 == 0 and all(_a16(o) for o in offs if o is not None) and all(s % 4 == 0 for s in strides)


def rule_warp_bwd_groups(C, H, W):
    """channel groups per block of k_warp_flow_bwd"""
    return 16 if H * W < 2048 and C > 32 else 4


def rule_wfg_eligible(C, HW):
    """gx of the feature warp by the gather (otherwise by the 64-bit scatter)"""
    return C >= 8 and 512 <= HW < 2 ** 28


def rule_map_small(HW, forced_large=False):
    """dfe_pwc_level_fwd_map: the map in one launch (otherwise count / scan / fill)"""
    return HW <= 1024 and not forced_large


def bits_equal_dev(a, b):
    """bits_equal for two fp32 tensors of one device, compared there"""
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def make_flow(kind, B, H, W, gen):
    """smooth (4x4 blocks of one vector, +-2 px), rough (+-4 px per pixel), out (sample 0 wholly out of view, the others +-30 px),
    zero, collapse (every pixel sampled at one interior point, quarter-pixel offsets).  [B,2,H,W] fp32"""
    if kind == "smooth":
        c = torch.randn(B, 2, (H + 3) // 4, (W + 3) // 4, generator=gen) * 2.0
        return c.repeat_interleave(4, 2).repeat_interleave(4, 3)[:, :, :H, :W].contiguous()
    if kind == "rough":
        return torch.randn(B, 2, H, W, generator=gen) * 4.0
    if kind == "out":
        f = torch.randn(B, 2, H, W, generator=gen) * 30.0
        f[0, 0] += W + 40.0
        return f
    if kind == "zero":
        return torch.zeros(B, 2, H, W)
    assert kind == "collapse"
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    return torch.stack([W // 2 + 0.25 - xs, H // 2 + 0.25 - ys])[None].repeat(B, 1, 1, 1).contiguous()


# --------------------------------------------------------------------------------------------------------- cost volume
def corr_ref(f1, f2, dtype, absolute=False):
    """out[b, i*9+j, y, x] = 1/C sum_c f1[b,c,y,x] f2[b,c,y+i-4,x+j-4]; float32: products and additions rounded one by one in
    channel order, then one division; absolute: 1/C sum |f1||f2| in float64"""
    B, C, H, W = f1.shape
    a, b = (f1.double().abs(), f2.double().abs()) if absolute else (f1.to(dtype), f2.to(dtype))
    dt = torch.float64 if absolute else dtype
    bp = F.pad(b, (CR_D,) * 4)
    out = torch.empty(B, CR_NK, H, W, dtype=dt)
    for i in range(CR_K):
        for j in range(CR_K):
            win = bp[:, :, i:i + H, j:j + W]
            if dt == torch.float64:
                out[:, i * CR_K + j] = (a * win).sum(1)
            else:
                acc = torch.zeros(B, H, W, dtype=dt)
                for c in range(C):
                    acc += a[:, c] * win[:, c]
                out[:, i * CR_K + j] = acc
    return out / C


def corr_bwd_ref(f1, f2, gout, dtype, absolute=False):
    """(g1, g2): g1[b,c,p] = 1/C sum_k gout[b,k,p] f2[b,c,p+d_k]; g2[b,c,q] = 1/C sum_k gout[b,k,q-d_k] f1[b,c,q-d_k]; the sums run
    in displacement order, every operation rounded in ``dtype``"""
    B, C, H, W = f1.shape
    if absolute:
        f1, f2, gout, dtype = f1.abs(), f2.abs(), gout.abs(), torch.float64
    a, g = f1.to(dtype), gout.to(dtype)
    bp = F.pad(f2.to(dtype), (CR_D,) * 4)
    g1, g2p = torch.zeros(B, C, H, W, dtype=dtype), torch.zeros(B, C, H + 2 * CR_D, W + 2 * CR_D, dtype=dtype)
    for i in range(CR_K):
        for j in range(CR_K):
            gk = g[:, i * CR_K + j, None]
            g1 += gk * bp[:, :, i:i + H, j:j + W]
            g2p[:, :, i:i + H, j:j + W] += gk * a
    return g1 / C, g2p[:, :, CR_D:CR_D + H, CR_D:CR_D + W] / C


# --------------------------------------------------------------------------------------------------------- feature warp
def warp_taps(flow, ac):
    """flow_coords + make_tap (csrc/dfe_device.h) in numpy float32, operation by operation; the one FMA of unnormalize is
    evaluated in float64 and rounded once.  flow [B,2,H,W] (torch fp32).  dict of numpy arrays [B,H*W] (lists: nw, ne, sw, se)"""
    f32 = np.float32
    fl = flow.numpy().astype(f32)
    B, _, H, W = fl.shape

    def coord(p, u, size):
        g = (f32(2.0) * (p + u)) / f32(size - 1 if size > 1 else 1) - f32(1.0)
        g1 = g + f32(1.0)
        if ac:
            return g1 * (f32(size - 1) / f32(2.0))
        return (g1.astype(np.float64) * (size / 2.0) - 0.5).astype(f32)
    ix = coord(np.arange(W, dtype=f32)[None, None, :], fl[:, 0], W).reshape(B, H * W)
    iy = coord(np.arange(H, dtype=f32)[None, :, None], fl[:, 1], H).reshape(B, H * W)
    assert ix.dtype == f32 and iy.dtype == f32
    xw, yn = np.floor(ix), np.floor(iy)
    w, n = ix - xw, iy - yn
    e, s = f32(1.0) - w, f32(1.0) - n
    wts = [s * e, s * w, n * e, n * w]
    xin0, xin1 = (xw > -1) & (xw < W), (xw + 1 > -1) & (xw + 1 < W)
    yin0, yin1 = (yn > -1) & (yn < H), (yn + 1 > -1) & (yn + 1 < H)
    inb = [xin0 & yin0, xin1 & yin0, xin0 & yin1, xin1 & yin1]
    x0, y0 = np.clip(xw, -2, W + 1).astype(np.int64), np.clip(yn, -2, H + 1).astype(np.int64)
    cover = np.where(inb[0], wts[0], f32(0))
    for k in (1, 2, 3):
        cover = cover + np.where(inb[k], wts[k], f32(0))
    assert cover.dtype == f32 and all(t.dtype == f32 for t in wts)
    idx = [np.where(inb[k], (y0 + k // 2) * W + x0 + k % 2, 0) for k in range(4)]
    return dict(w=wts, inb=inb, idx=idx, wx=w, wy=n, e=e, s=s, cover=cover, H=H, W=W)


def _keep(taps, use_mask):
    return torch.from_numpy((taps["cover"] >= np.float32(0.9999)).astype(np.float64) if use_mask else np.ones_like(taps["cover"], dtype=np.float64))


def _corners(x, taps, dtype):
    """the four corner values of every sample, zero outside the image: list of [B,C,HW]"""
    B, C, H, W = x.shape
    flat = x.to(dtype).reshape(B, C, H * W)
    out = []
    for k in range(4):
        idx = torch.from_numpy(taps["idx"][k])[:, None, :].expand(B, C, H * W)
        out.append(flat.gather(2, idx) * torch.from_numpy(taps["inb"][k])[:, None, :].to(dtype))
    return out


def _t(a, dtype):
    return torch.from_numpy(a)[:, None, :].to(dtype)


def warp_fwd_ref(x, taps, use_mask, dtype, absolute=False):
    """sum of the four corner values times their (exact fp32) weights, in the kernel's order nw, ne, sw, se; [B,C,H,W]"""
    dt = torch.float64 if absolute else dtype
    v = _corners(x.abs() if absolute else x, taps, dt)
    r = v[0] * _t(taps["w"][0], dt)
    for k in (1, 2, 3):
        r = r + v[k] * _t(taps["w"][k], dt)
    return (r * _keep(taps, use_mask)[:, None, :].to(dt)).reshape(x.shape)


def warp_gflow_ref(x, taps, gout, use_mask, ac, add, dtype, absolute=False):
    """gflow [B,2,H,W] = (sum_c g_c d interp_c / d(ix, iy)) * d(ix, iy)/d(u, v) + add; channel order, every operation rounded in
    ``dtype``; absolute: with |g|, |corner| + |corner| for every difference and |add|"""
    B, C, H, W = x.shape
    dt = torch.float64 if absolute else dtype
    v = _corners(x.abs() if absolute else x, taps, dt)
    g = (gout.abs() if absolute else gout).to(dt).reshape(B, C, H * W) * _keep(taps, use_mask)[:, None, :].to(dt)
    s, e, wx, wy = (_t(taps[k], dt) for k in ("s", "e", "wx", "wy"))
    sg = 1.0 if absolute else -1.0
    dx = (v[1] + sg * v[0]) * s + (v[3] + sg * v[2]) * wy
    dy = (v[2] + sg * v[0]) * e + (v[3] + sg * v[1]) * wx
    gix, giy = torch.zeros(B, H * W, dtype=dt), torch.zeros(B, H * W, dtype=dt)
    for c in range(C):
        gix = gix + g[:, c] * dx[:, c]
        giy = giy + g[:, c] * dy[:, c]

    def scale(size):
        den = np.float32(size - 1 if size > 1 else 1)
        return float(np.float32(size - 1) / den if ac else np.float32(size) / den)
    out = torch.stack([gix * scale(W), giy * scale(H)], 1).reshape(B, 2, H, W)
    if add is not None:
        out = out + (add.abs() if absolute else add).to(dt)
    return out


def warp_gx_ref(taps, gout, use_mask):
    """the adjoint wrt the sampled tensor as a float64 scatter of the contributions g * w (weights exact): (ref64, mass = the same
    with |g|, taps = contributions per target element), each [B,C,H,W] / [B,1,H,W]"""
    B, C, H, W = gout.shape
    g = gout.double().reshape(B, C, H * W) * _keep(taps, use_mask)[:, None, :]
    ref, mass, cnt = torch.zeros(B, C, H * W, dtype=torch.float64), torch.zeros(B, C, H * W, dtype=torch.float64), torch.zeros(B, 1, H * W, dtype=torch.float64)
    live = _keep(taps, use_mask)
    for k in range(4):
        w = torch.from_numpy(taps["w"][k]).double() * torch.from_numpy(taps["inb"][k]).double()
        idx = torch.from_numpy(taps["idx"][k])
        for b in range(B):
            ref[b].index_add_(1, idx[b], g[b] * w[b])
            mass[b].index_add_(1, idx[b], g[b].abs() * w[b])
            cnt[b].index_add_(1, idx[b], ((w[b] != 0).double() * live[b])[None])
    return ref.reshape(B, C, H, W), mass.reshape(B, C, H, W), cnt.reshape(B, 1, H, W)


def check_scatter_bound(tag, out, ref64, mass, cnt, gmax):
    """|out - ref64| <= 2^-24 mass + 1/2 quantum taps + 2^-24 |ref64| (one fp32 product per contribution, its rounding to the
    fixed-point grid, the final conversion); quantum = 2^(k - 36) with gmax = m 2^k, m in [0.5, 1)"""
    assert bool(torch.isfinite(out).all()), tag
    quantum = 2.0 ** (math.frexp(float(gmax))[1] - 36) if gmax > 0 else 0.0
    bound = U24 * mass + 0.5 * quantum * cnt + U24 * ref64.abs()
    err = (out.double().cpu() - ref64).abs()
    worst = float((err / bound.clamp_min(1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0
    print("EBOUND %s scatter err/bound %.3f" % (tag, worst))
    assert bool((err <= bound).all()), (tag, worst)
    return worst
