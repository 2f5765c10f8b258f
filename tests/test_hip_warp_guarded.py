"""GPU: warp_flow and its two gradients (k_warp_flow_fwd, k_warp_flow_bwd<4 | 16>, the k_wfg_* gather and the 64-bit scatter of
csrc/ops_basic.hip) through the C ABI in guarded, poisoned buffers (tests/guarded.py) on the shapes of tests/pwc_cases.py: C = 5, 8,
40 and 136, planes below one wave, not a multiple of 64 and of 2048 pixels and more (both group counts of the backward, gather and
scatter), use_mask 0 / 1, both align_corners modes, gflow alone, gx alone and both, smooth / rough / out-of-view / zero / collapsing
flows.

Every call: return code 0, guards intact, every output element written and finite, inputs unchanged; the scatter workspace is a
byte carve of exactly dfe_scatter_ws_bytes whose contents are free.  Taps and fp32 weights come from tests/guarded.warp_taps (a
float32 restatement of the device's coordinate arithmetic, held to the oracle in test_guarded_cpu.py); with the weights as exact
inputs the forward and gflow keep e = |out - ref64| / (2^-24 A) within 4 max(1, e of the same sums in plain fp32), and gx keeps
2^-24 mass + 1/2 quantum taps + 2^-24 |ref| with the quantum of max |gout|.  Gather and forced scatter return the same bits,
also with 66 048 taps piled on each of four targets (the gather's integer accumulators)."""
import ctypes

import pytest
import torch

from tests import guarded as G
from tests import pwc_cases as PC

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib(), L.stream_ptr()


def _p(c):
    return None if c is None else ctypes.c_void_p(c.ptr)


def _carve(t, off):
    return G.Carved(t.shape, off, fill=t)


def _check(tag, bufs, outs, ins):
    torch.cuda.synchronize()
    for i, c in enumerate(bufs):
        assert c.intact(), (tag, "guard of buffer %d overwritten" % i)
    for i, c in enumerate(outs):
        assert c.written(), (tag, "output %d has unwritten or non-finite elements" % i)
    for i, (c, t) in enumerate(ins):
        assert G.bits_equal_dev(c.view, t), (tag, "input %d changed" % i)


def _inputs(shape, kind, seed):
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=gen), G.make_flow(kind, B, H, W, gen), torch.randn(shape, generator=gen)


def _fwd(lib, st, x, flow, um, ac, off):
    B, C, H, W = x.shape
    dx, df = x.cuda(), flow.cuda()
    cx, cf, out = _carve(dx, off), _carve(df, (off + 1) % 4 if off else 0), G.Carved(x.shape, off)
    tag = "warp_fwd %s mask %d ac %d off %d" % (tuple(x.shape), um, ac, off)
    assert lib.dfe_warp_flow_fwd(_p(cx), _p(cf), _p(out), B, C, H, W, um, ac, st) == 0, tag
    _check(tag, [cx, cf, out], [out], [(cx, dx), (cf, df)])
    return out


def _bwd(lib, st, x, flow, gout, um, ac, off, want=(True, True)):
    """(gflow, gx) carves (None where not asked for)"""
    B, C, H, W = x.shape
    dx, df, dg = x.cuda(), flow.cuda(), gout.cuda()
    cx, cf, cg = _carve(dx, off), _carve(df, (off + 1) % 4 if off else 0), _carve(dg, (off + 2) % 4 if off else 0)
    gflow = G.Carved(flow.shape, off) if want[0] else None
    gx = G.Carved(x.shape, (off + 3) % 4 if off else 0) if want[1] else None
    nws = int(lib.dfe_scatter_ws_bytes(B * C * H * W))
    assert nws == 64 + 8 * B * C * H * W
    ws = G.CarvedBytes((nws,), 0) if want[1] else None
    tag = "warp_bwd %s mask %d ac %d off %d grads %s" % (tuple(x.shape), um, ac, off, want)
    assert lib.dfe_warp_flow_bwd(_p(cx), _p(cf), _p(cg), _p(gflow), _p(gx), _p(ws), B, C, H, W, um, ac, st) == 0, tag
    outs = [c for c in (gflow, gx) if c]
    _check(tag, [cx, cf, cg] + outs + ([ws] if ws else []), outs, [(cx, dx), (cf, df), (cg, dg)])
    return gflow, gx


@pytest.mark.parametrize("ac", [0, 1])
@pytest.mark.parametrize("shape,kind", PC.WARP)
def test_warp_flow_forward_and_both_gradients(shape, kind, ac, monkeypatch):
    monkeypatch.delenv("DFE_WARP_SCATTER", raising=False)
    lib, st = _lib()
    B, C, H, W = shape
    x, flow, gout = _inputs(shape, kind, sum(shape) + ac)
    taps = G.warp_taps(flow, ac)
    groups, gather = G.rule_warp_bwd_groups(C, H, W), G.rule_wfg_eligible(C, H * W)
    for um in (0, 1):
        tag = "warp %s %s mask %d ac %d groups %d %s" % (shape, kind, um, ac, groups, "gather" if gather else "scatter")
        out = _fwd(lib, st, x, flow, um, ac, 0)
        G.check_bound(tag + " fwd", out.cpu(), G.warp_fwd_ref(x, taps, um, F32), G.warp_fwd_ref(x, taps, um, F64), G.warp_fwd_ref(x, taps, um, F64, absolute=True))
        assert G.bits_equal_dev(_fwd(lib, st, x, flow, um, ac, 1).view, out.view), (tag, "forward bits depend on the alignment")
        gflow, gx = _bwd(lib, st, x, flow, gout, um, ac, 0)
        G.check_bound(tag + " gflow", gflow.cpu(), G.warp_gflow_ref(x, taps, gout, um, ac, None, F32), G.warp_gflow_ref(x, taps, gout, um, ac, None, F64),
                      G.warp_gflow_ref(x, taps, gout, um, ac, None, F64, absolute=True))
        ref, mass, cnt = G.warp_gx_ref(taps, gout, um)
        G.check_scatter_bound(tag + " gx", gx.cpu(), ref, mass, cnt, float(gout.abs().max()))
        f1, none = _bwd(lib, st, x, flow, gout, um, ac, 0, (True, False))
        none2, x1 = _bwd(lib, st, x, flow, gout, um, ac, 0, (False, True))
        assert none is None and none2 is None
        assert G.bits_equal_dev(f1.view, gflow.view) and G.bits_equal_dev(x1.view, gx.view), (tag, "a gradient alone differs from the pair")
        f2, x2 = _bwd(lib, st, x, flow, gout, um, ac, 1)
        assert G.bits_equal_dev(f2.view, gflow.view) and G.bits_equal_dev(x2.view, gx.view), (tag, "gradient bits depend on the alignment")
        if gather:
            monkeypatch.setenv("DFE_WARP_SCATTER", "1")
            f3, x3 = _bwd(lib, st, x, flow, gout, um, ac, 0)
            monkeypatch.delenv("DFE_WARP_SCATTER")
            assert G.bits_equal_dev(f3.view, gflow.view) and G.bits_equal_dev(x3.view, gx.view), (tag, "gather and scatter differ")


def test_warp_gx_of_a_pile_up_above_2_16_taps_is_the_scatters(monkeypatch):
    """every pixel of a 258 x 256 plane sampled at one interior point: 66 048 list entries on each of four targets, more than a
    double adds exactly, so k_wfg_gather walks them with its integer accumulators"""
    monkeypatch.delenv("DFE_WARP_SCATTER", raising=False)
    lib, st = _lib()
    B, C, H, W = PC.PILE
    x, flow, gout = _inputs(PC.PILE, "collapse", 3)
    assert G.rule_wfg_eligible(C, H * W)
    taps = G.warp_taps(flow, 0)
    ref, mass, cnt = G.warp_gx_ref(taps, gout, 0)
    assert float(cnt.max()) == PC.PILE_TAPS > 65536 and int((cnt == PC.PILE_TAPS).sum()) == 4
    _, gx = _bwd(lib, st, x, flow, gout, 0, 0, 0, (False, True))
    monkeypatch.setenv("DFE_WARP_SCATTER", "1")
    _, gs = _bwd(lib, st, x, flow, gout, 0, 0, 0, (False, True))
    assert G.bits_equal_dev(gx.view, gs.view), "gather and scatter differ on the pile-up"
    G.check_scatter_bound("warp pile-up %s gx" % (PC.PILE,), gx.cpu(), ref, mass, cnt, float(gout.abs().max()))


def test_warp_flow_refuses_without_touching_a_buffer():
    lib, st = _lib()
    shape = (1, 8, 16, 32)
    t = torch.ones(shape).cuda()
    cx, cf, cg = _carve(t, 0), _carve(torch.zeros(1, 2, 16, 32).cuda(), 0), _carve(t, 0)
    gflow, gx = G.Carved((1, 2, 16, 32), 0), G.Carved(shape, 0)
    nws = int(lib.dfe_scatter_ws_bytes(8 * 512))
    ws, ws8 = G.CarvedBytes((nws,), 0), G.CarvedBytes((nws,), 8)
    args = (1, 8, 16, 32, 0, 0, st)
    assert lib.dfe_warp_flow_bwd(_p(cx), _p(cf), _p(cg), None, None, _p(ws), *args) == -1           # no gradient asked for
    assert lib.dfe_warp_flow_bwd(_p(cx), _p(cf), _p(cg), _p(gflow), _p(gx), None, *args) == -1      # gx without its workspace
    assert lib.dfe_warp_flow_bwd(_p(cx), _p(cf), _p(cg), _p(gflow), _p(gx), _p(ws8), *args) == -2   # the gather's workspace off 16 bytes
    assert lib.dfe_warp_flow_bwd(_p(cx), _p(cf), _p(cg), _p(gflow), _p(gx), _p(ws8), 1, 4, 16, 32, 0, 0, st) == -2    # ... and the scatter's (C = 4)
    assert lib.dfe_warp_flow_fwd(_p(cx), None, _p(gx), 1, 8, 16, 32, 0, 0, st) == -1
    torch.cuda.synchronize()
    for c in (gflow, gx, ws, ws8):
        assert c.untouched() and c.intact()
    for c in (cx, cf, cg):
        assert c.intact()
    assert bool((cx.view == 1).all()) and bool((cf.view == 0).all())
