"""GPU: the deterministic mode's convolution kernels -- dfe_sconv_fwd, dfe_sconv_dgrad (csrc/ops_sconv.hip), dfe_conv1x1s2_fwd,
dfe_conv1x1s2_wgrad (csrc/ops_conv1x1s2.hip) -- through the C ABI in guarded, NaN-poisoned buffers (tests/guarded.py): every
tensor a dword-aligned, batch-strided view at each float offset in turn, the workspace exactly the floats the library reports
(NaN-filled, then 1e30-filled), results bit-equal across offsets, strides, calls and workspace contents, and the per-element bound
|out - ref64| <= 4 max(1, e_fp32) 2^-24 A of the other convolution tests.  The shapes are the smallest that reach every
launcher branch (asserted on the host from the planners' answers): 32- and 64-channel blocks of every filter size, channel
splits on either side of their rule, one and several pixel splits, both orders of the split sum."""
import ctypes

import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib(), L.stream_ptr()


def _p(c):
    return None if c is None else ctypes.c_void_p(c.ptr)


def _l(v):
    return ctypes.c_long(int(v))


def _out_hw(H, W, K):
    P = K // 2
    return (H + 2 * P - K) // 2 + 1, (W + 2 * P - K) // 2 + 1


def _carve(t, off, extra):
    return G.Carved(tuple(t.shape), off, t[0].numel() + extra, fill=t)


def _intact(tag, **carved):
    for name, c in carved.items():
        if c is not None:
            assert c.intact(), (tag, "guard or batch gap of %s overwritten" % name)


# (offset of input, filter, bias, output; batch stride of input and output above the dense sample): each pointer one float off
# 16 bytes in turn, then mixed offsets with gaps between the samples
BASE = (0, 0, 0, 0, 0, 0)
VARIANTS = [(1, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, 0), (0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 0), (2, 3, 1, 2, 1, 3), (3, 2, 3, 1, 5, 2), (0, 0, 0, 0, 4, 4)]


# ------------------------------------------------------------------------------------------------------------ dfe_sconv_fwd
def _fwd_packed(Ci, Co, K):
    return (Ci + 3) // 4 * 4 * K * K * ((Co + 63) // 64 * 64) + 64


def _fwd_plan(lib, B, Ci, Co, H, W, K):
    """(workspace floats, channel splits, 32-channel block) from the host-only planner"""
    n = int(lib.dfe_sconv_fwd_floats(B, Ci, Co, H, W, K))
    Ho, Wo = _out_hw(H, W, K)
    rest = n - _fwd_packed(Ci, Co, K)
    assert n > 0 and rest >= 0 and rest % (B * Co * Ho * Wo) == 0
    return n, max(1, rest // (B * Co * Ho * Wo)), Co <= 32


def _fwd_case(shape, family, bias, slope, salt=0):
    """inputs whose activation decisions all keep the margin (asserted on the float64 reference), with references"""
    B, Ci, Co, H, W, K = shape
    for s in range(20):
        gen = torch.Generator().manual_seed(1000 * s + sum(shape) + 7 * G.FAMILIES.index(family) + salt)
        x, w = G.make_input((B, Ci, H, W), family, gen), G.make_weight(Co, Ci, K, gen)
        b = torch.randn(Co, generator=gen) * 0.1 if bias else None
        z64 = G.conv_ref(x, w, 2, K // 2, 1, torch.float64) + G._bc(b, torch.float64)
        A = G.conv_ref(x.abs(), w.abs(), 2, K // 2, 1, torch.float64) + G._abc(b)
        if slope == 1.0 or G.margin_ok(z64, A):
            yard = G.leaky(G.conv_ref(x, w, 2, K // 2, 1, torch.float32) + G._bc(b, torch.float32), slope)
            return x, w, b, G.leaky(z64, slope), yard, A
    raise AssertionError("no seed keeps the activation margin for %s" % (shape,))


def _run_fwd(lib, st, shape, x, w, b, slope, variant, tag, ws_fill=None):
    B, Ci, Co, H, W, K = shape
    xo, wo, bo, yo, xbe, ybe = variant
    Ho, Wo = _out_hw(H, W, K)
    nws = int(lib.dfe_sconv_fwd_floats(B, Ci, Co, H, W, K))
    cx, cw = _carve(x, xo, xbe), G.Carved(tuple(w.shape), wo, fill=w)
    cb = None if b is None else G.Carved((Co,), bo, fill=b)
    cy = G.Carved((B, Co, Ho, Wo), yo, Co * Ho * Wo + ybe)
    ws = G.Carved((nws,), 0, fill=None if ws_fill is None else torch.full((nws,), ws_fill))
    calls = 2 if variant == BASE else 1
    outs = []
    for _ in range(calls):          # a second call into the same buffers returns the bits of the first
        rc = lib.dfe_sconv_fwd(_p(cx), _l(cx.batch_stride), _p(cw), _p(cb), float(slope), _p(cy), _l(cy.batch_stride), _p(ws), B, Ci, Co, H, W, K, st)
        assert rc == 0, (tag, variant, rc)
        torch.cuda.synchronize()
        outs.append(cy.cpu())
    _intact(tag, x=cx, weight=cw, bias=cb, y=cy, ws=ws)
    assert cy.written(), (tag, variant, "y elements unwritten or not finite")
    assert torch.equal(cx.cpu(), x) and torch.equal(cw.cpu(), w), (tag, variant, "an input changed")
    assert all(G.bits_equal(o, outs[0]) for o in outs), (tag, "the second call differs")
    return outs[0]


# (B, Ci, Co, H, W, K): the channel pairs of the networks' stride-2 layers on planes from 3x5 to 16x52, odd and even sides
FWD_SHAPES = [(1, 3, 64, 16, 52, 7), (3, 9, 16, 9, 13, 7), (3, 16, 32, 8, 26, 5), (1, 8, 40, 6, 11, 5), (1, 16, 32, 3, 5, 3), (3, 3, 16, 16, 52, 3),
              (1, 32, 64, 7, 9, 3), (3, 96, 128, 8, 26, 3), (1, 128, 196, 8, 26, 3), (3, 256, 256, 4, 13, 3)]
COMBOS = {"randn": ((True, 0.1), (False, 1.0), (True, 0.0), (False, 0.0)), "act": ((True, 0.1),), "sparse": ((True, 0.0), (False, 0.1))}


def test_fwd_shapes_reach_every_launcher_branch():
    lib, _ = _lib()
    seen = set()
    for shape in FWD_SHAPES + FWD_SPLIT_RULE:
        _, nsplit, t32 = _fwd_plan(lib, *shape)
        seen.add((shape[5], t32, nsplit > 1))
    # every filter size with the 32- and the 64-channel block; both with and without channel splits
    assert {(k, t) for k, t, _ in seen} == {(k, t) for k in (3, 5, 7) for t in (True, False)}, seen
    assert {s for _, _, s in seen} == {True, False}
    # the split rule (fewer than 384 blocks and more than one channel chunk): one shape on either side
    (over, under) = FWD_SPLIT_RULE
    assert _fwd_plan(lib, *over)[1] == 1 and over[1] > 8 and _fwd_plan(lib, *under)[1] == 2
    assert _fwd_plan(lib, 1, 8, 64, 7, 9, 3)[1] == 1           # one chunk of channels: nothing to split however few the blocks


@pytest.mark.parametrize("shape", FWD_SHAPES)
def test_sconv_fwd_guarded(shape):
    lib, st = _lib()
    for family in G.FAMILIES:
        for k, (bias, slope) in enumerate(COMBOS[family]):
            x, w, b, ref, yard, A = _fwd_case(shape, family, bias, slope, k)
            tag = "sconv_fwd %s %s bias %d slope %g" % (family, shape, bias, slope)
            base = _run_fwd(lib, st, shape, x, w, b, slope, BASE, tag)
            G.check_bound(tag, base, yard, ref, A)
            if k == 0:
                assert G.bits_equal(_run_fwd(lib, st, shape, x, w, b, slope, BASE, tag, ws_fill=1e30), base), (tag, "y depends on the workspace's contents")
            if family == "act":
                for v in VARIANTS:
                    assert G.bits_equal(_run_fwd(lib, st, shape, x, w, b, slope, v, tag), base), (tag, v, "y depends on the alignment")


# 384 blocks of (128 pixels x 64 channels): no split; 372: two
FWD_SPLIT_RULE = [(3, 16, 196, 128, 128, 3), (3, 16, 196, 124, 128, 3)]


@pytest.mark.parametrize("shape", FWD_SPLIT_RULE)
def test_sconv_fwd_split_rule_guarded(shape):
    lib, st = _lib()
    # (no activation: among ten million outputs some pre-activation always lies inside the margin, whatever the seed)
    x, w, b, ref, yard, A = _fwd_case(shape, "randn", True, 1.0)
    tag = "sconv_fwd split rule %s" % (shape,)
    base = _run_fwd(lib, st, shape, x, w, b, 1.0, BASE, tag)
    G.check_bound(tag, base, yard, ref, A)
    assert G.bits_equal(_run_fwd(lib, st, shape, x, w, b, 1.0, (1, 3, 2, 3, 1, 2), tag), base), tag


def test_sconv_fwd_refusals_write_nothing():
    lib, st = _lib()
    B, Ci, Co, H, W, K = 1, 16, 32, 8, 26, 3
    Ho, Wo = _out_hw(H, W, K)
    nws = int(lib.dfe_sconv_fwd_floats(B, Ci, Co, H, W, K))
    x, w = G.Carved((B, Ci, H, W), 0, fill=torch.ones(B, Ci, H, W)), G.Carved((Co, Ci, K, K), 0, fill=torch.ones(Co, Ci, K, K))
    for ws_off, k, xbs, want in ((1, K, Ci * H * W, -4), (2, K, Ci * H * W, -4), (0, 4, Ci * H * W, -4), (0, K, Ci * H * W - 1, -2)):
        y, ws = G.Carved((B, Co, Ho, Wo), 0), G.Carved((nws,), ws_off)
        assert lib.dfe_sconv_fwd(_p(x), _l(xbs), _p(w), None, 1.0, _p(y), _l(Co * Ho * Wo), _p(ws), B, Ci, Co, H, W, k, st) == want
        torch.cuda.synchronize()
        assert y.untouched() and ws.untouched() and y.intact() and ws.intact()
    # a sample of fewer than 4 floats has no safe address for the staging loads: outside the family
    assert lib.dfe_sconv_fwd_floats(2, 3, 8, 1, 1, 3) == 0 and lib.dfe_sconv_dgrad_floats(2, 8, 3, 1, 1, 3) == 0
    x, w, y, ws = G.Carved((2, 3, 1, 1), 0, fill=torch.ones(2, 3, 1, 1)), G.Carved((8, 3, 3, 3), 0, fill=torch.ones(8, 3, 3, 3)), G.Carved((2, 8, 1, 1), 0), G.Carved((64,), 0)
    assert lib.dfe_sconv_fwd(_p(x), _l(3), _p(w), None, 1.0, _p(y), _l(8), _p(ws), 2, 3, 8, 1, 1, 3, st) == -4
    gy, gx = G.Carved((2, 3, 1, 1), 0, fill=torch.ones(2, 3, 1, 1)), G.Carved((2, 8, 1, 1), 0)
    w2 = G.Carved((3, 8, 3, 3), 0, fill=torch.ones(3, 8, 3, 3))
    assert lib.dfe_sconv_dgrad(_p(gy), _l(3), _p(w2), _p(gx), _l(8), _p(ws), 2, 8, 3, 1, 1, 3, st) == -4
    torch.cuda.synchronize()
    assert y.untouched() and gx.untouched() and ws.untouched()


# ---------------------------------------------------------------------------------------------------------- dfe_sconv_dgrad
def _dg_packed(Ci, Co, K):
    cb = min(8 if K == 5 else 16, (Co + 3) // 4 * 4)
    return ((Co + 3) // 4 * 4 + cb - 1) // cb * cb * K * K * ((Ci + 63) // 64 * 64) + 64


def _dg_plan(lib, B, Ci, Co, H, W, K):
    n = int(lib.dfe_sconv_dgrad_floats(B, Ci, Co, H, W, K))
    rest = n - _dg_packed(Ci, Co, K)
    assert n > 0 and rest >= 0 and rest % (B * Ci * H * W) == 0, (n, rest)
    return n, max(1, rest // (B * Ci * H * W)), Ci <= 32


def _run_dgrad(lib, st, shape, gy, w, variant, tag, ws_fill=None):
    B, Ci, Co, H, W, K = shape
    go, wo, _, xo, gbe, xbe = variant
    nws = int(lib.dfe_sconv_dgrad_floats(B, Ci, Co, H, W, K))
    cg, cw = _carve(gy, go, gbe), G.Carved(tuple(w.shape), wo, fill=w)
    cx = G.Carved((B, Ci, H, W), xo, Ci * H * W + xbe)
    ws = G.Carved((nws,), 0, fill=None if ws_fill is None else torch.full((nws,), ws_fill))
    outs = []
    for _ in range(2 if variant == BASE else 1):
        rc = lib.dfe_sconv_dgrad(_p(cg), _l(cg.batch_stride), _p(cw), _p(cx), _l(cx.batch_stride), _p(ws), B, Ci, Co, H, W, K, st)
        assert rc == 0, (tag, variant, rc)
        torch.cuda.synchronize()
        outs.append(cx.cpu())
    _intact(tag, gy=cg, weight=cw, gx=cx, ws=ws)
    assert cx.written(), (tag, variant, "gx elements unwritten or not finite")
    assert torch.equal(cg.cpu(), gy) and torch.equal(cw.cpu(), w), (tag, variant, "an input changed")
    assert all(G.bits_equal(o, outs[0]) for o in outs), (tag, "the second call differs")
    return outs[0]


# (B, Ci, Co, H, W, K) of the FORWARD layer: gx is [B,Ci,H,W]
DGRAD_SHAPES = [(3, 16, 32, 8, 26, 5), (1, 40, 8, 6, 11, 5), (1, 16, 32, 3, 5, 3), (3, 3, 16, 16, 52, 3), (1, 32, 64, 7, 9, 3), (3, 96, 128, 8, 26, 3),
                (1, 128, 196, 8, 26, 3), (3, 256, 256, 4, 13, 3), (1, 64, 128, 5, 7, 1), (3, 64, 128, 6, 8, 1), (1, 256, 512, 4, 6, 1), (3, 16, 24, 5, 7, 1)]
# 384 blocks of (64 positions x 64 channels): no split; 372: two
DGRAD_SPLIT_RULE = [(3, 196, 32, 64, 128, 3), (3, 196, 32, 62, 128, 3)]


def test_dgrad_shapes_reach_every_launcher_branch():
    lib, _ = _lib()
    seen = set()
    for shape in DGRAD_SHAPES + DGRAD_SPLIT_RULE:
        _, nsplit, t32 = _dg_plan(lib, *shape)
        seen.add((shape[5], t32, nsplit > 1))
    assert {(k, t) for k, t, _ in seen} == {(k, t) for k in (1, 3, 5) for t in (True, False)}, seen
    assert {s for _, _, s in seen} == {True, False}
    (over, under) = DGRAD_SPLIT_RULE
    assert _dg_plan(lib, *over)[1] == 1 and over[2] > 16 and _dg_plan(lib, *under)[1] == 2


def _dgrad_refs(shape, family, gen):
    B, Ci, Co, H, W, K = shape
    Ho, Wo = _out_hw(H, W, K)
    gy, w = G.make_input((B, Co, Ho, Wo), family, gen), G.make_weight(Co, Ci, K, gen)
    args = ((B, Ci, H, W), 2, K // 2, 1)
    return (gy, w, G.conv_dgrad_ref(gy, w, *args, torch.float64), G.conv_dgrad_ref(gy, w, *args, torch.float32),
            G.conv_dgrad_ref(gy.abs(), w.abs(), *args, torch.float64))


@pytest.mark.parametrize("shape", DGRAD_SHAPES)
def test_sconv_dgrad_guarded(shape):
    lib, st = _lib()
    for family in G.FAMILIES:
        gy, w, ref, yard, A = _dgrad_refs(shape, family, torch.Generator().manual_seed(sum(shape) + G.FAMILIES.index(family)))
        tag = "sconv_dgrad %s %s" % (family, shape)
        base = _run_dgrad(lib, st, shape, gy, w, BASE, tag)
        G.check_bound(tag, base, yard, ref, A)
        assert G.bits_equal(_run_dgrad(lib, st, shape, gy, w, BASE, tag, ws_fill=1e30), base), (tag, "gx depends on the workspace's contents")
        if family == "act":
            for v in VARIANTS:
                if v[2] == 0 or v != (0, 0, 1, 0, 0, 0):        # (there is no bias to move)
                    assert G.bits_equal(_run_dgrad(lib, st, shape, gy, w, v, tag), base), (tag, v, "gx depends on the alignment")


@pytest.mark.parametrize("shape", DGRAD_SPLIT_RULE)
def test_sconv_dgrad_split_rule_guarded(shape):
    lib, st = _lib()
    gy, w, ref, yard, A = _dgrad_refs(shape, "randn", torch.Generator().manual_seed(sum(shape)))
    tag = "sconv_dgrad split rule %s" % (shape,)
    base = _run_dgrad(lib, st, shape, gy, w, BASE, tag)
    G.check_bound(tag, base, yard, ref, A)
    assert G.bits_equal(_run_dgrad(lib, st, shape, gy, w, (1, 3, 0, 3, 1, 2), tag), base), tag


# ------------------------------------------------------------------------------------------------- dfe_conv1x1s2_fwd / _wgrad
# (B, Ci, Co, H, W): the issue's planes; channel counts off the 64-blocks and the 16-channel chunks; 66 pixel splits (the long sum)
C1_SHAPES = [(1, 64, 128, 5, 7), (3, 64, 128, 6, 8), (1, 256, 512, 4, 6), (3, 256, 512, 4, 6), (3, 7, 70, 5, 7), (1, 1, 1, 1, 1), (3, 16, 16, 54, 52)]


def _c1_nsplit(lib, B, Ci, Co, H, W):
    n = int(lib.dfe_conv1x1s2_wgrad_floats(B, Ci, Co, H, W))
    assert n > 0 and n % (Co * Ci) == 0
    return n // (Co * Ci)


def test_conv1x1s2_shapes_reach_every_launcher_branch():
    lib, _ = _lib()
    ns = {s: _c1_nsplit(lib, *s) for s in C1_SHAPES}
    assert ns[(1, 64, 128, 5, 7)] == 1 and ns[(3, 64, 128, 6, 8)] == 2 and ns[(3, 16, 16, 54, 52)] == 66       # one split, a few, > 64: the 32-group sum
    assert all(lib.dfe_conv1x1s2_supported(*s) == 1 for s in C1_SHAPES)
    # several channel chunks (Ci > 16) and one; several output-channel blocks and a partial one; more than one pixel block
    assert any(s[1] > 16 for s in C1_SHAPES) and any(s[1] <= 16 for s in C1_SHAPES) and any(s[2] % 64 for s in C1_SHAPES)
    assert any(s[0] * ((s[3] + 1) // 2) * ((s[4] + 1) // 2) > 64 for s in C1_SHAPES)


@pytest.mark.parametrize("shape", C1_SHAPES)
def test_conv1x1s2_fwd_guarded(shape):
    B, Ci, Co, H, W = shape
    lib, st = _lib()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1

    def run(x, w, variant, tag):
        xo, wo, _, yo, xbe, ybe = variant
        cx, cw = _carve(x, xo, xbe), G.Carved((Co, Ci), wo, fill=w)
        cy = G.Carved((B, Co, Ho, Wo), yo, Co * Ho * Wo + ybe)
        outs = []
        for _ in range(2 if variant == BASE else 1):
            rc = lib.dfe_conv1x1s2_fwd(_p(cx), _l(cx.batch_stride), _p(cw), _p(cy), _l(cy.batch_stride), B, Ci, Co, H, W, st)
            assert rc == 0, (tag, variant, rc)
            torch.cuda.synchronize()
            outs.append(cy.cpu())
        _intact(tag, x=cx, weight=cw, y=cy)
        assert cy.written() and torch.equal(cx.cpu(), x) and G.bits_equal(outs[-1], outs[0]), (tag, variant)
        return outs[0]

    for family in G.FAMILIES:
        gen = torch.Generator().manual_seed(sum(shape) + G.FAMILIES.index(family))
        x, w = G.make_input((B, Ci, H, W), family, gen), G.make_weight(Co, Ci, 1, gen)
        tag = "conv1x1s2_fwd %s %s" % (family, shape)
        base = run(x, w, BASE, tag)
        G.check_bound(tag, base, G.conv_ref(x, w, 2, 0, 1, torch.float32), G.conv_ref(x, w, 2, 0, 1, torch.float64),
                      G.conv_ref(x.abs(), w.abs(), 2, 0, 1, torch.float64))
        if family == "act":
            for v in VARIANTS:
                if v != (0, 0, 1, 0, 0, 0):
                    assert G.bits_equal(run(x, w, v, tag), base), (tag, v, "y depends on the alignment")


@pytest.mark.parametrize("shape", C1_SHAPES)
def test_conv1x1s2_wgrad_guarded(shape):
    B, Ci, Co, H, W = shape
    lib, st = _lib()
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    nws = int(lib.dfe_conv1x1s2_wgrad_floats(B, Ci, Co, H, W))

    def run(x, gy, variant, tag, ws_fill=None):
        xo, go, wso, gwo, xbe, gbe = variant
        cx, cg = _carve(x, xo, xbe), _carve(gy, go, gbe)
        gw = G.Carved((Co, Ci), gwo)
        ws = G.Carved((nws,), wso, fill=None if ws_fill is None else torch.full((nws,), ws_fill))
        outs = []
        for _ in range(2 if variant == BASE else 1):
            rc = lib.dfe_conv1x1s2_wgrad(_p(cx), _l(cx.batch_stride), _p(cg), _l(cg.batch_stride), _p(gw), _p(ws), B, Ci, Co, H, W, st)
            assert rc == 0, (tag, variant, rc)
            torch.cuda.synchronize()
            outs.append(gw.cpu())
        _intact(tag, x=cx, gy=cg, gweight=gw, ws=ws)
        assert gw.written() and torch.equal(cx.cpu(), x) and torch.equal(cg.cpu(), gy) and G.bits_equal(outs[-1], outs[0]), (tag, variant)
        return outs[0]

    for family in G.FAMILIES:
        gen = torch.Generator().manual_seed(sum(shape) + G.FAMILIES.index(family))
        x, gy = G.make_input((B, Ci, H, W), family, gen), G.make_input((B, Co, Ho, Wo), family, gen)
        tag = "conv1x1s2_wgrad %s %s" % (family, shape)
        base = run(x, gy, BASE, tag)
        G.check_bound(tag, base.view(Co, Ci, 1, 1), G.conv_wgrad_ref(gy, x, 1, 2, 0, 1, torch.float32), G.conv_wgrad_ref(gy, x, 1, 2, 0, 1, torch.float64),
                      G.conv_wgrad_ref(gy.abs(), x.abs(), 1, 2, 0, 1, torch.float64))
        assert G.bits_equal(run(x, gy, BASE, tag, ws_fill=1e30), base), (tag, "gweight depends on the workspace's contents")
        if family == "act":
            for v in VARIANTS:
                assert G.bits_equal(run(x, gy, v, tag), base), (tag, v, "gweight depends on the alignment")
