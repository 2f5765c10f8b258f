"""GPU: the small-plane convolutions (csrc/ops_planeconv.hip) through the C ABI in guarded, poisoned buffers
(tests/guarded.py): forward into two destinations whose offsets and batch strides differ, data gradient and weight gradient;
workspace of exactly dfe_planeconv_ws_floats, NaN on entry; every pointer also one float off a 16-byte boundary (the header
restricts none of them), bit-equal to the aligned run; per-element bound e = |out - ref64| / (2^-24 sum |a||b|) against aten's
fp32 CPU result on zero-mean, activation-like and sparse inputs."""
import ctypes

import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu

# (B, Ci, Co, H, W)
SHAPES = [(1, 1, 1, 1, 1), (2, 3, 5, 3, 5), (3, 17, 33, 1, 70), (2, 5, 16, 64, 2), (2, 20, 70, 9, 7),
          # the 64-channel block tile (pc_cfg: nsub = 4) needs N > 32 and B * ceil(HW / 64) * ceil(N / 32) * ceil(Ck / 32) >= 1024 --
          # with 33 channels on either side (forward and data gradient) B * ceil(HW / 64) >= 256: the smallest with a second
          # pixel tile and all nine taps inside
          (128, 33, 33, 5, 13)]


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib(), L.stream_ptr()


def _p(c):
    return ctypes.c_void_p(c.ptr) if c is not None else None


def _l(v):
    return ctypes.c_long(int(v))


def _b(t):
    return t[None, :, None, None]


def _check(bufs, outs, tag):
    torch.cuda.synchronize()
    for i, c in enumerate(bufs):
        assert c.intact(), (tag, "guard or gap of buffer %d overwritten" % i)
    for c in outs:
        assert c.written(), (tag, "output elements unwritten or not finite")


@pytest.mark.parametrize("shape", SHAPES)
def test_planeconv_guarded(shape):
    B, Ci, Co, H, W = shape
    lib, st = _lib()
    assert lib.dfe_planeconv_supported(B, Ci, Co, H, W) == 1
    nws = int(lib.dfe_planeconv_ws_floats(B, Ci, Co, H, W))
    assert nws > 0
    HW, slope = H * W, 0.1
    for family in G.FAMILIES:
        gen = torch.Generator().manual_seed(sum(shape) + G.FAMILIES.index(family))
        x, gy = G.make_input((B, Ci, H, W), family, gen), G.make_input((B, Co, H, W), family, gen)
        w, bias = G.make_weight(Co, Ci, 3, gen), torch.randn(Co, generator=gen) * 0.5
        tag = "planeconv %s %s" % (family, shape)
        res = []
        for off in (0, 1):
            xc, gc, wc, bc = G.Carved(x.shape, off, fill=x), G.Carved(gy.shape, off, fill=gy), G.Carved(w.shape, off, fill=w), G.Carved((Co,), off, fill=bias)
            ins = [xc, gc, wc, bc]
            # forward: two destinations, channel slices of wider buffers
            d1, d2 = G.Carved((B, Co, H, W), off, (Co + 5) * HW), G.Carved((B, Co, H, W), (off + 2) % 4, (Co + 3) * HW + 1)
            ws = G.Carved((nws,), off)
            assert lib.dfe_planeconv_fwd(_p(xc), _p(wc), _p(bc), ctypes.c_float(slope), _p(d1), _l(d1.batch_stride), _p(d2), _l(d2.batch_stride),
                                         _p(ws), B, Ci, Co, H, W, st) == 0
            _check(ins + [d1, d2, ws], [d1, d2], tag + " fwd")
            assert torch.equal(d1.cpu(), d2.cpu())
            # data gradient
            gx, ws2 = G.Carved((B, Ci, H, W), off), G.Carved((nws,), off)
            assert lib.dfe_planeconv_dgrad(_p(gc), _p(wc), _p(gx), _p(ws2), B, Ci, Co, H, W, st) == 0
            _check(ins + [gx, ws2], [gx], tag + " dgrad")
            # weight gradient
            gw, ws3 = G.Carved((Co, Ci, 3, 3), off), G.Carved((nws,), off)
            assert lib.dfe_planeconv_wgrad(_p(gc), _p(xc), _p(gw), _p(ws3), B, Ci, Co, H, W, st) == 0
            _check(ins + [gw, ws3], [gw], tag + " wgrad")
            assert torch.equal(xc.cpu(), x) and torch.equal(gc.cpu(), gy) and torch.equal(wc.cpu(), w), (tag, "an input changed")
            res.append((d1.cpu(), gx.cpu(), gw.cpu()))
        for a, b in zip(res[0], res[1]):
            assert torch.equal(a, b), (tag, "the result depends on the alignment")
        y, gx, gw = res[0]
        G.check_bound(tag + " fwd", y, G.leaky(G.conv_ref(x, w, 1, 1, 1, torch.float32) + _b(bias), slope),
                      G.leaky(G.conv_ref(x, w, 1, 1, 1, torch.float64) + _b(bias.double()), slope),
                      G.conv_ref(x.abs(), w.abs(), 1, 1, 1, torch.float64) + _b(bias.double().abs()))
        G.check_bound(tag + " dgrad", gx, G.conv_dgrad_ref(gy, w, x.shape, 1, 1, 1, torch.float32), G.conv_dgrad_ref(gy, w, x.shape, 1, 1, 1, torch.float64),
                      G.conv_dgrad_ref(gy.abs(), w.abs(), x.shape, 1, 1, 1, torch.float64))
        G.check_bound(tag + " wgrad", gw, G.conv_wgrad_ref(gy, x, 3, 1, 1, 1, torch.float32), G.conv_wgrad_ref(gy, x, 3, 1, 1, 1, torch.float64),
                      G.conv_wgrad_ref(gy.abs(), x.abs(), 3, 1, 1, 1, torch.float64))


def test_planeconv_forward_without_bias_and_second_destination():
    B, Ci, Co, H, W = 2, 20, 70, 9, 7
    lib, st = _lib()
    gen = torch.Generator().manual_seed(5)
    x, w = G.make_input((B, Ci, H, W), "act", gen), G.make_weight(Co, Ci, 3, gen)
    xc, wc = G.Carved(x.shape, 1, fill=x), G.Carved(w.shape, 3, fill=w)
    d1, ws = G.Carved((B, Co, H, W), 3), G.Carved((int(lib.dfe_planeconv_ws_floats(B, Ci, Co, H, W)),), 2)
    assert lib.dfe_planeconv_fwd(_p(xc), _p(wc), None, ctypes.c_float(1.0), _p(d1), _l(Co * H * W), None, _l(0), _p(ws), B, Ci, Co, H, W, st) == 0
    _check([xc, wc, d1, ws], [d1], "planeconv fwd plain")
    G.check_bound("planeconv act plain", d1.cpu(), G.conv_ref(x, w, 1, 1, 1, torch.float32), G.conv_ref(x, w, 1, 1, 1, torch.float64),
                  G.conv_ref(x.abs(), w.abs(), 1, 1, 1, torch.float64))


def test_planeconv_refuses_short_strides_and_large_planes():
    """a batch stride below the dense sample size is DFE_ERR_DIMS, a plane of more than 4096 pixels DFE_ERR_UNSUPPORTED (0
    workspace floats): nothing is written"""
    B, Ci, Co, H, W = 2, 3, 5, 3, 5
    lib, st = _lib()
    x, w = G.Carved((B, Ci, H, W), 0, fill=torch.ones(B, Ci, H, W)), G.Carved((Co, Ci, 3, 3), 0, fill=torch.ones(Co, Ci, 3, 3))
    d1, d2 = G.Carved((B, Co, H, W), 0), G.Carved((B, Co, H, W), 0)
    ws = G.Carved((int(lib.dfe_planeconv_ws_floats(B, Ci, Co, H, W)),), 0)
    n = Co * H * W
    assert lib.dfe_planeconv_fwd(_p(x), _p(w), None, ctypes.c_float(1.0), _p(d1), _l(n - 1), None, _l(0), _p(ws), B, Ci, Co, H, W, st) == -2
    assert lib.dfe_planeconv_fwd(_p(x), _p(w), None, ctypes.c_float(1.0), _p(d1), _l(n), _p(d2), _l(n - 1), _p(ws), B, Ci, Co, H, W, st) == -2
    assert lib.dfe_planeconv_ws_floats(1, 4, 4, 65, 64) == 0 and lib.dfe_planeconv_supported(1, 4, 4, 65, 64) == 0
    assert lib.dfe_planeconv_fwd(_p(x), _p(w), None, ctypes.c_float(1.0), _p(d1), _l(4 * 65 * 64), None, _l(0), _p(ws), 1, 4, 4, 65, 64, st) == -4
    assert lib.dfe_planeconv_dgrad(_p(x), _p(w), _p(d1), _p(ws), 1, 4, 4, 65, 64, st) == -4
    assert lib.dfe_planeconv_wgrad(_p(x), _p(x), _p(d1), _p(ws), 1, 4, 4, 65, 64, st) == -4
    torch.cuda.synchronize()
    assert d1.untouched() and d2.untouched() and ws.untouched() and d1.intact() and ws.intact()


# ========================================================================================================= 1x1 on tiny planes
# dfe_conv1x1_small_fwd / _bwd (PoseCNN's pose_conv and refinement head): cases in tests/geom_cases.py, float64 references and the
# serial fp32 sum of the host in tests/guarded_geom.py; A = sum |x||w| + |b|; no pre-activation within MARGIN A of zero.
from tests import geom_cases as GC          # noqa: E402
from tests import guarded_geom as GG        # noqa: E402


def _ins_unchanged(tag, pairs):
    for i, (c, t) in enumerate(pairs):
        assert G.bits_equal(c.cpu(), t.reshape(c.view.shape)), (tag, "input %d changed" % i)


@pytest.mark.parametrize("shape", GC.C1_SHAPES)
def test_conv1x1_small_guarded(shape):
    B, Ci, Co, H, W = shape
    lib, st = _lib()
    assert lib.dfe_conv1x1_small_supported(B, Ci, Co, H, W) == 1
    for with_bias in (True, False):
        x, w, bias, gy, seed = GG.conv1x1_inputs(shape, with_bias, sum(shape))
        pre64, A = GG.conv1x1_ref(x, w, bias), GG.conv1x1_ref(x, w, bias, absolute=True)
        assert G.margin_ok(pre64, A)
        pre32 = GG.conv1x1_ref(x, w, bias, torch.float32)
        name = "conv1x1_small %s bias %d" % (shape, with_bias)
        for slope in GC.C1_SLOPES:
            first = None
            for off in GC.OFFS:
                tag = "%s slope %g off %d" % (name, slope, off)
                xc, wc, y = G.Carved(x.shape, off, fill=x), G.Carved(w.shape, (off + 1) % 4, fill=w), G.Carved((B, Co, H, W), (off + 2) % 4)
                bc = G.Carved((Co,), (off + 3) % 4, fill=bias) if with_bias else None
                assert lib.dfe_conv1x1_small_fwd(_p(xc), _p(wc), _p(bc), ctypes.c_float(slope), _p(y), B, Ci, Co, H, W, st) == 0, tag
                _check([xc, wc, y] + ([bc] if bc else []), [y], tag)
                _ins_unchanged(tag, [(xc, x), (wc, w)] + ([(bc, bias)] if bc else []))
                if first is None:
                    first = y.cpu()
                    G.check_bound(tag, first, G.leaky(pre32, slope), G.leaky(pre64, slope), A)
                assert torch.equal(y.cpu(), first), (tag, "the result depends on the alignment")
        gx32, gx64, gxA = GG.conv1x1_gx_ref(gy, w, torch.float32), GG.conv1x1_gx_ref(gy, w), GG.conv1x1_gx_ref(gy, w, absolute=True)
        gw32, gw64, gwA = GG.conv1x1_gw_ref(gy, x, torch.float32), GG.conv1x1_gw_ref(gy, x), GG.conv1x1_gw_ref(gy, x, absolute=True)
        first = None
        for off in GC.OFFS:
            for mode in ("both", "gx", "gweight"):
                tag = "%s bwd %s off %d" % (name, mode, off)
                gc, xc, wc = G.Carved(gy.shape, off, fill=gy), G.Carved(x.shape, (off + 1) % 4, fill=x), G.Carved(w.shape, (off + 2) % 4, fill=w)
                gx = G.Carved(x.shape, (off + 3) % 4) if mode != "gweight" else None
                gw = G.Carved(w.shape, off) if mode != "gx" else None
                assert lib.dfe_conv1x1_small_bwd(_p(gc), _p(xc), _p(wc), _p(gx), _p(gw), B, Ci, Co, H, W, st) == 0, tag
                _check([c for c in (gc, xc, wc, gx, gw) if c], [c for c in (gx, gw) if c], tag)
                _ins_unchanged(tag, [(gc, gy), (xc, x), (wc, w)])
                if first is None:
                    first = (gx.cpu(), gw.cpu())
                    G.check_bound(name + " gx", first[0], gx32, gx64, gxA)
                    G.check_bound(name + " gweight", first[1], gw32, gw64, gwA)
                assert gx is None or torch.equal(gx.cpu(), first[0]), (tag, "gx depends on the alignment or on what else is requested")
                assert gw is None or torch.equal(gw.cpu(), first[1]), (tag, "gweight depends on the alignment or on what else is requested")


@pytest.mark.parametrize("shape", GC.C1_REFUSED)
def test_conv1x1_small_refuses_larger_planes_and_touches_nothing(shape):
    """H*W = 257 and B*H*W = 4097: DFE_ERR_UNSUPPORTED from both entry points before anything is launched"""
    B, Ci, Co, H, W = shape
    lib, st = _lib()
    assert lib.dfe_conv1x1_small_supported(B, Ci, Co, H, W) == 0
    x, w, gy = G.Carved((B, Ci, H, W), 0, fill=torch.ones(B, Ci, H, W)), G.Carved((Co, Ci), 0, fill=torch.ones(Co, Ci)), G.Carved((B, Co, H, W), 0, fill=torch.ones(B, Co, H, W))
    y, gx, gw = G.Carved((B, Co, H, W), 1), G.Carved((B, Ci, H, W), 2), G.Carved((Co, Ci), 3)
    assert lib.dfe_conv1x1_small_fwd(_p(x), _p(w), None, ctypes.c_float(0.1), _p(y), B, Ci, Co, H, W, st) == -4
    assert lib.dfe_conv1x1_small_bwd(_p(gy), _p(x), _p(w), _p(gx), _p(gw), B, Ci, Co, H, W, st) == -4
    torch.cuda.synchronize()
    assert all(c.untouched() and c.intact() for c in (y, gx, gw))
