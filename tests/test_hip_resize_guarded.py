"""GPU: the pyramid resizes (dfe_resize), the differentiable bilinear resize (dfe_resize_bilinear_fwd / _bwd; csrc/ops_basic.hip)
and the triplet preparation (dfe_prepare_triplets; csrc/ops_input.hip) through the C ABI in guarded, poisoned buffers
(tests/guarded.py), every pointer rotated through the four dword offsets (the uint8 input through odd byte offsets).

Every call: return code 0, guard bands intact, every output written, inputs unchanged, every offset variant bit-equal to the
first; a refusal touches nothing.  The bilinear forwards equal ATen's composition on the host bit for bit, on both sides of
ATen's kernel switch (output H + W <= 128).  The adjoint keeps e = |out - ref64| / (2^-24 sum |w||g||mult|) within 4 max(1, e of
fp32 autograd of F.interpolate on the host) against the exact float64 adjoint; the area resize the same with A = mean |x|, the
triplets with A = 1 (tests/guarded_geom.py, guarded.check_bound)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import geom_cases as GC
from tests import guarded as G
from tests import guarded_geom as GG

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib(), L.stream_ptr()


def _p(c):
    return None if c is None else ctypes.c_void_p(c.ptr)


def _f(v):
    return ctypes.c_float(v)


def _carve(t, off=0):
    return G.Carved(t.shape, off, fill=t)


def _check(tag, bufs, outs, ins=()):
    torch.cuda.synchronize()
    for i, c in enumerate(bufs):
        assert c.intact(), (tag, "guard band of buffer %d overwritten" % i)
    for i, c in enumerate(outs):
        assert c.written(), (tag, "output %d has unwritten or non-finite elements" % i)
    for i, (c, t) in enumerate(ins):
        assert G.bits_equal(c.cpu(), t.reshape(c.view.shape)), (tag, "input %d changed" % i)


def _interp(x, hw):
    return F.interpolate(x[None], hw, mode="bilinear", align_corners=False)[0]


# ========================================================================================================= dfe_resize
@pytest.mark.parametrize("case", GC.R0_CASES)
def test_resize_bilinear_pyramid_is_atens_on_both_sides_of_its_kernel_switch(case):
    lib, st = _lib()
    (h, w), (H, W) = case
    P = 3
    x = torch.randn(P, h, w, generator=torch.Generator().manual_seed(h * w + H))
    want = _interp(x, (H, W))
    for off in GC.OFFS:
        tag = "resize mode 0 %s small %d off %d" % (case, H + W <= 128, off)
        xc, out = _carve(x, off), G.Carved((P, H, W), (off + 1) % 4)
        assert lib.dfe_resize(_p(xc), _p(out), P, h, w, H, W, 0, st) == 0, tag
        _check(tag, [xc, out], [out], [(xc, x)])
        assert G.bits_equal(out.cpu(), want), (tag, "not ATen's bits")


@pytest.mark.parametrize("case", GC.R1_CASES)
def test_resize_area_against_the_float64_mean(case):
    lib, st = _lib()
    (h, w), (H, W) = case
    P = 3
    x = torch.randn(P, h, w, generator=torch.Generator().manual_seed(h * w + H))
    yard = F.interpolate(x[None], (H, W), mode="area")[0]
    first = None
    for off in GC.OFFS:
        tag = "resize mode 1 %s off %d" % (case, off)
        xc, out = _carve(x, off), G.Carved((P, H, W), (off + 3) % 4)
        assert lib.dfe_resize(_p(xc), _p(out), P, h, w, H, W, 1, st) == 0, tag
        _check(tag, [xc, out], [out], [(xc, x)])
        if first is None:
            first = out.cpu()
            G.check_bound("resize area %s" % (case,), first, yard, GG.area_ref(x, (H, W)), GG.area_ref(x, (H, W), absolute=True))
        assert G.bits_equal(out.cpu(), first), (tag, "the result depends on the alignment")


def test_resize_refuses_an_unknown_mode():
    lib, st = _lib()
    xc, out = _carve(torch.ones(1, 2, 2)), G.Carved((1, 4, 4))
    assert lib.dfe_resize(_p(xc), _p(out), 1, 2, 2, 4, 4, 2, st) == -4
    assert lib.dfe_resize(_p(xc), _p(out), 1, 2, 2, 0, 4, 0, st) == -2
    torch.cuda.synchronize()
    assert out.untouched() and out.intact()


# ========================================================================================================= dfe_resize_bilinear
@pytest.mark.parametrize("case", GC.RB_CASES)
def test_resize_bilinear_forward_and_adjoint(case):
    lib, st = _lib()
    (h, w), (H, W) = case
    P = GC.RB_PLANES
    gen = torch.Generator().manual_seed(h * w + H * W)
    x, g = torch.randn(P, h, w, generator=gen), torch.randn(P, H, W, generator=gen)
    for mult in GC.RB_MULTS:
        for pre in (0, 1):
            name = "resize_bilinear %s mult %g pre %d" % (case, mult, pre)
            x32 = x.clone().requires_grad_(True)
            want = _interp(x32 * mult, (H, W)) if pre else _interp(x32, (H, W)) * mult
            yard = torch.autograd.grad(want, x32, g)[0]
            ref64, A = GG.resize_adjoint_ref(g, (h, w), mult), GG.resize_adjoint_ref(g, (h, w), mult, absolute=True)
            first = None
            for off in GC.OFFS:
                tag = "%s off %d" % (name, off)
                xc, out = _carve(x, off), G.Carved((P, H, W), (off + 1) % 4)
                assert lib.dfe_resize_bilinear_fwd(_p(xc), _p(out), P, h, w, H, W, _f(mult), pre, st) == 0, tag
                _check(tag + " fwd", [xc, out], [out], [(xc, x)])
                assert G.bits_equal(out.cpu(), want.detach()), (tag, "the forward is not ATen's composition")
                gc, gin = _carve(g, (off + 2) % 4), G.Carved((P, h, w), (off + 3) % 4)
                assert lib.dfe_resize_bilinear_bwd(_p(gc), _p(gin), P, h, w, H, W, _f(mult), pre, st) == 0, tag
                _check(tag + " bwd", [gc, gin], [gin], [(gc, g)])
                if first is None:
                    first = gin.cpu()
                    G.check_bound(name + " adjoint", first, yard, ref64, A)
                assert G.bits_equal(gin.cpu(), first), (tag, "the adjoint depends on the alignment")


def test_resize_bilinear_backward_refuses_a_ratio_beyond_four():
    lib, st = _lib()
    (h, w), (H, W) = GC.RB_REFUSED
    g = torch.ones(2, H, W)
    gc, gin = _carve(g), G.Carved((2, h, w))
    assert lib.dfe_resize_bilinear_bwd(_p(gc), _p(gin), 2, h, w, H, W, _f(1.0), 0, st) == -4
    torch.cuda.synchronize()
    assert gin.untouched() and gin.intact() and gc.intact()
    x, out = _carve(torch.randn(2, h, w, generator=torch.Generator().manual_seed(1))), G.Carved((2, H, W), 1)       # the forward has no such limit
    assert lib.dfe_resize_bilinear_fwd(_p(x), _p(out), 2, h, w, H, W, _f(1.0), 0, st) == 0
    _check("resize_bilinear fwd 3x5 -> 13x5", [x, out], [out])
    assert G.bits_equal(out.cpu(), _interp(x.cpu(), (H, W)))


# ========================================================================================================= triplets
@pytest.mark.parametrize("case", GC.TRIPLET_CASES)
def test_prepare_triplets_against_the_float64_resize(case):
    lib, st = _lib()
    (H0, W0), (H, W) = case
    B = GC.TRIPLET_B
    u8 = torch.randint(0, 256, (B, 3 * H0, W0, 3), generator=torch.Generator().manual_seed(H0 * W0 + H), dtype=torch.uint8)
    for flips in (GC.TRIPLET_FLIPS, None):
        ref64, yard = GG.triplets_ref(u8, flips, H, W), GG.triplets_ref(u8, flips, H, W, np.float32)
        first = None
        for k, off in enumerate(GC.OFFS):
            tag = "prepare_triplets %s flip %s off %d" % (case, flips, off)
            ic = G.CarvedBytes(u8.shape, 2 * k + 1)
            ic.view.copy_(u8)
            fc = None
            if flips is not None:
                fc = G.CarvedBytes((B,), (2 * k + 3) % 16)
                fc.view.copy_(torch.tensor(flips, dtype=torch.uint8))
            out = G.Carved((B, 3, 3 * H, W), off)
            assert lib.dfe_prepare_triplets(_p(ic), _p(fc), _p(out), B, H0, W0, H, W, st) == 0, tag
            torch.cuda.synchronize()
            assert ic.intact() and out.intact() and out.written() and (fc is None or fc.intact()), tag
            assert torch.equal(ic.cpu(), u8) and (fc is None or torch.equal(fc.cpu(), torch.tensor(flips, dtype=torch.uint8))), (tag, "an input changed")
            if first is None:
                first = out.cpu()
                G.check_bound("prepare_triplets %s flip %d" % (case, flips is not None), first, yard, ref64, torch.ones_like(ref64))
            assert G.bits_equal(out.cpu(), first), (tag, "the result depends on the alignment")
