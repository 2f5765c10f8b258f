"""Helpers of the guarded convolution tests (test_hip_conv_guarded.py, test_hip_conv_wgrad_guarded.py,
test_hip_planeconv_guarded.py; self-tests in test_guarded_cpu.py).  Not a conftest: imported explicitly.

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
