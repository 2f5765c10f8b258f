"""GPU: one PWC decoder level (dfe_pwc_level_fwd / _bwd and the _map pair of csrc/ops_basic.hip: feature warp, cost volume written
into x with c1 and the flow behind it, correlation gradients with the concatenated slices of dL/dx folded in, flow gradient, g_c2 by
gather or by the 64-bit scatter) through the C ABI in guarded, poisoned buffers (tests/guarded.py) on the cases of
tests/pwc_cases.py: the fine plans of training's batch on the 16-byte and the dword kernels, gather against scatter at C = 7 / 8 and
H*W = 510 / 512, the map in one launch against three at H*W = 1024 / 1056, DFE_WARP_SCATTER and DFE_WFG_MAP_LARGE on eligible
shapes, g_c2 NULL, g_flow NULL, the _map pair against the plain pair, a second backward through one map.

Every call: return code 0, guards intact, every output element written and finite, inputs unchanged; x and gx are dense
[B, 81+C+2, H, W] carves, warped and g_warped exact-size carves, the scatter workspace and the map byte carves of exactly
dfe_scatter_ws_bytes / dfe_pwc_level_map_bytes on 16 bytes whose contents are free.

Numerics stage by stage, each stage fed the device's own upstream output: warped against the float64 sum over the restated taps;
the cost volume, dL/dwarped and g_c1 against float64 direct sums with A = 1/C sum |.||.| (+ |gx slice| for g_c1) and the plain
fp32 sum as yardstick (tests/guarded.check_bound); the copied planes bit for bit; g_flow against the float64 sum over the taps;
g_c2 within 2^-24 mass + 1/2 quantum taps + 2^-24 |ref| with the quantum of the device's max |dL/dwarped|.  All variants of one
case return the same bits."""
import ctypes
import functools

import pytest
import torch

from tests import guarded as G
from tests import pwc_cases as PC

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
NK = G.CR_NK


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib(), L.stream_ptr()


def _p(c):
    return None if c is None else ctypes.c_void_p(c.ptr)


def _settle(tag, bufs, outs, ins):
    torch.cuda.synchronize()
    for name, c in bufs.items():
        assert c.intact(), (tag, "guard of %s overwritten" % name)
    for name in outs:
        assert bufs[name].written(), (tag, "%s has unwritten or non-finite elements" % name)
    for name, t in ins.items():
        assert G.bits_equal_dev(bufs[name].view, t), (tag, "input %s changed" % name)


@functools.lru_cache(maxsize=None)
def _data(shape, family, kind):
    """(CPU tensors, the same on the device)"""
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(PC.level_seed(shape))
    d = dict(c1=G.make_input(shape, family, gen), c2=G.make_input(shape, family, gen), flow=G.make_flow(kind, B, H, W, gen),
             gx=torch.randn(B, NK + C + 2, H, W, generator=gen))
    return d, {k: v.cuda() for k, v in d.items()}


def _fwd(lib, st, dev, ac, off=None, use_map=False):
    """dict of carves: c1, c2, flow, warped, x (+ map).  off: the pointer moved one float off a 16-byte boundary"""
    B, C, H, W = dev["c1"].shape
    assert lib.dfe_pwc_level_channels(C) == NK + C + 2
    o = lambda name: int(name == off)
    bufs = {k: G.Carved(dev[k].shape, o(k), fill=dev[k]) for k in ("c1", "c2", "flow")}
    bufs["warped"], bufs["x"] = G.Carved((B, C, H, W), o("warped")), G.Carved((B, NK + C + 2, H, W), o("x"))
    tag = "pwc_level_fwd%s %s off %s" % ("_map" if use_map else "", (B, C, H, W), off)
    if use_map:
        nmap = int(lib.dfe_pwc_level_map_bytes(B, H, W))
        assert nmap > 64 + 40 * B * H * W
        bufs["map"] = G.CarvedBytes((nmap,), 0)
        rc = lib.dfe_pwc_level_fwd_map(_p(bufs["c1"]), _p(bufs["c2"]), _p(bufs["flow"]), _p(bufs["warped"]), _p(bufs["x"]), _p(bufs["map"]), B, C, H, W, ac, st)
    else:
        rc = lib.dfe_pwc_level_fwd(_p(bufs["c1"]), _p(bufs["c2"]), _p(bufs["flow"]), _p(bufs["warped"]), _p(bufs["x"]), B, C, H, W, ac, st)
    assert rc == 0, (tag, rc)
    _settle(tag, bufs, ("warped", "x"), {k: dev[k] for k in ("c1", "c2", "flow")})
    return bufs


def _bwd(lib, st, dev, warped, gx, ac, off=None, want=(True, True), fmap=None):
    """dict of carves; want = (g_c2, g_flow); fmap: the map carve of _fwd(use_map=True) -> dfe_pwc_level_bwd_map"""
    B, C, H, W = dev["c1"].shape
    o = lambda name: int(name == off)
    bufs = {k: G.Carved(dev[k].shape, o(k), fill=dev[k]) for k in ("c1", "c2", "flow")}
    bufs["warped"], bufs["gx"] = G.Carved(warped.shape, o("warped"), fill=warped), G.Carved(gx.shape, o("gx"), fill=gx)
    bufs["g_warped"], bufs["g_c1"] = G.Carved((B, C, H, W), o("g_warped")), G.Carved((B, C, H, W), o("g_c1"))
    outs = ["g_warped", "g_c1"]
    if want[0]:
        bufs["g_c2"] = G.Carved((B, C, H, W), o("g_c2"))
        outs.append("g_c2")
    if want[1]:
        bufs["g_flow"] = G.Carved((B, 2, H, W), o("g_flow"))
        outs.append("g_flow")
    tag = "pwc_level_bwd%s %s off %s grads %s" % ("_map" if fmap else "", (B, C, H, W), off, want)
    head = [_p(bufs[k]) for k in ("c1", "c2", "flow", "warped", "gx", "g_warped", "g_c1")] + [_p(bufs.get("g_c2"))]
    if fmap is not None:
        bufs["map"] = fmap
        rc = lib.dfe_pwc_level_bwd_map(*head, _p(fmap), _p(bufs.get("g_flow")), B, C, H, W, ac, st)
    else:
        if want[0]:
            nws = int(lib.dfe_scatter_ws_bytes(B * C * H * W))
            assert nws == 64 + 8 * B * C * H * W
            bufs["ws"] = G.CarvedBytes((nws,), 0)
        rc = lib.dfe_pwc_level_bwd(*head, _p(bufs.get("ws")), _p(bufs.get("g_flow")), B, C, H, W, ac, st)
    assert rc == 0, (tag, rc)
    _settle(tag, bufs, outs, dict(c1=dev["c1"], c2=dev["c2"], flow=dev["flow"], warped=warped, gx=gx))
    return bufs


def _same(tag, a, b, names):
    for n in names:
        assert G.bits_equal_dev(a[n].view, b[n].view), (tag, n, "differs")


def _plans(lib, shape):
    B, C, H, W = shape
    xbs = (NK + C + 2) * H * W
    return (G.corr_plan(lib, shape, G.rule_corr_vec(W, [0, 0, 0, 0], [xbs])), G.corr_plan(lib, shape, G.rule_corr_vec(W, [0] * 5, [xbs, xbs]), sides=2),
            "gather" if G.rule_wfg_eligible(C, H * W) else "scatter", "one launch" if G.rule_map_small(H * W) else "three launches")


def _clean_env(monkeypatch):
    for name in ("DFE_WARP_SCATTER", "DFE_WFG_MAP_LARGE", "DFE_CORR_FWD", "DFE_CORR_BWD", "DFE_CORR_DYG"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("case", range(len(PC.LEVEL)))
def test_level_forward_stage_by_stage(case, monkeypatch):
    _clean_env(monkeypatch)
    lib, st = _lib()
    shape, family, kind = PC.LEVEL[case]
    B, C, H, W = shape
    ac = case % 2
    d, dev = _data(shape, family, kind)
    fplan, _, _, mplan = _plans(lib, shape)
    if shape in PC.ALIGN_SHAPES:
        assert fplan["coarse"] == 0 and fplan["PF2"] == 4 and fplan["threads"] == 512 and fplan["vec"] == int(W % 4 == 0), fplan
    tag = "level_fwd %s %s %s ac %d %s" % (shape, family, kind, ac, fplan)
    fw = _fwd(lib, st, dev, ac)
    warped, x = fw["warped"].cpu(), fw["x"].cpu()
    taps = G.warp_taps(d["flow"], ac)
    G.check_bound(tag + " warped", warped, G.warp_fwd_ref(d["c2"], taps, 0, F32), G.warp_fwd_ref(d["c2"], taps, 0, F64), G.warp_fwd_ref(d["c2"], taps, 0, F64, absolute=True))
    G.check_bound(tag + " cost volume", x[:, :NK].contiguous(), G.corr_ref(d["c1"], warped, F32), G.corr_ref(d["c1"], warped, F64),
                  G.corr_ref(d["c1"], warped, F64, absolute=True))
    assert G.bits_equal(x[:, NK:NK + C], d["c1"]) and G.bits_equal(x[:, NK + C:], d["flow"]), (tag, "the copied planes differ")
    if C >= 8:
        fm = _fwd(lib, st, dev, ac, use_map=True)
        _same(tag + " map built in " + mplan, fm, fw, ("warped", "x"))
        if shape in PC.LEVEL_MAP_LARGE_ENV:
            assert G.rule_map_small(H * W) and not G.rule_map_small(H * W, True)
            monkeypatch.setenv("DFE_WFG_MAP_LARGE", "1")
            _same(tag + " DFE_WFG_MAP_LARGE", _fwd(lib, st, dev, ac, use_map=True), fw, ("warped", "x"))


@pytest.mark.parametrize("case", range(len(PC.LEVEL)))
def test_level_backward_stage_by_stage(case, monkeypatch):
    _clean_env(monkeypatch)
    lib, st = _lib()
    shape, family, kind = PC.LEVEL[case]
    B, C, H, W = shape
    ac = case % 2
    d, dev = _data(shape, family, kind)
    _, bplan, gplan, mplan = _plans(lib, shape)
    if shape in PC.ALIGN_SHAPES:
        assert bplan["TH"] == 8 and bplan["NCG"] == 2 and bplan["IS"] == 1 and bplan["batches"] == 2 and bplan["vec"] == int(W % 4 == 0), bplan
    tag = "level_bwd %s %s %s ac %d %s %s" % (shape, family, kind, ac, bplan, gplan)
    fw = _fwd(lib, st, dev, ac)
    wd = fw["warped"].view.contiguous()
    bw = _bwd(lib, st, dev, wd, dev["gx"], ac)
    warped, gx, gw = wd.cpu(), d["gx"], bw["g_warped"].cpu()
    # dL/dwarped and g_c1: the correlation gradients of (c1, the device's warped) for the first 81 planes of gx
    y32, r64, A = [G.corr_bwd_ref(d["c1"], warped, gx[:, :NK], dt, a) for dt, a in ((F32, False), (F64, False), (F64, True))]
    G.check_bound(tag + " g_warped", gw, y32[1], r64[1], A[1])
    sl = gx[:, NK:NK + C]
    G.check_bound(tag + " g_c1", bw["g_c1"].cpu(), y32[0] + sl, r64[0] + sl.double(), A[0] + sl.double().abs())
    # g_flow and g_c2: the adjoints of the feature warp applied to the device's dL/dwarped
    taps = G.warp_taps(d["flow"], ac)
    add = gx[:, NK + C:]
    G.check_bound(tag + " g_flow", bw["g_flow"].cpu(), G.warp_gflow_ref(d["c2"], taps, gw, 0, ac, add, F32), G.warp_gflow_ref(d["c2"], taps, gw, 0, ac, add, F64),
                  G.warp_gflow_ref(d["c2"], taps, gw, 0, ac, add, F64, absolute=True))
    ref, mass, cnt = G.warp_gx_ref(taps, gw, 0)
    gmax = float(gw.abs().max())
    G.check_scatter_bound(tag + " g_c2", bw["g_c2"].cpu(), ref, mass, cnt, gmax)
    # the variants return the same bits
    _same(tag + " g_c2 NULL", _bwd(lib, st, dev, wd, dev["gx"], ac, want=(False, True)), bw, ("g_warped", "g_c1", "g_flow"))
    _same(tag + " g_flow NULL", _bwd(lib, st, dev, wd, dev["gx"], ac, want=(True, False)), bw, ("g_warped", "g_c1", "g_c2"))
    if shape in PC.LEVEL_SCATTER_ENV:
        assert gplan == "gather"
        monkeypatch.setenv("DFE_WARP_SCATTER", "1")
        _same(tag + " DFE_WARP_SCATTER", _bwd(lib, st, dev, wd, dev["gx"], ac), bw, ("g_warped", "g_c1", "g_c2", "g_flow"))
        monkeypatch.delenv("DFE_WARP_SCATTER")
    if C < 8:
        return
    fm = _fwd(lib, st, dev, ac, use_map=True)
    _same(tag + " _map", _bwd(lib, st, dev, wd, dev["gx"], ac, fmap=fm["map"]), bw, ("g_warped", "g_c1", "g_c2", "g_flow"))
    _same(tag + " _map g_c2 NULL", _bwd(lib, st, dev, wd, dev["gx"], ac, want=(False, True), fmap=fm["map"]), bw, ("g_warped", "g_c1", "g_flow"))
    _same(tag + " _map g_flow NULL", _bwd(lib, st, dev, wd, dev["gx"], ac, want=(True, False), fmap=fm["map"]), bw, ("g_warped", "g_c1", "g_c2"))
    # a second backward through the same map: the first pass's bound is still in its header (the larger of the two is used), so
    # the quantum is the first pass's
    second = _bwd(lib, st, dev, wd, dev["gx"] * 0.375, ac, fmap=fm["map"])
    gw2 = second["g_warped"].cpu()
    assert float(gw2.abs().max()) < gmax
    ref2, mass2, cnt2 = G.warp_gx_ref(taps, gw2, 0)
    G.check_scatter_bound(tag + " g_c2 second pass", second["g_c2"].cpu(), ref2, mass2, cnt2, gmax)
    if shape in PC.LEVEL_MAP_LARGE_ENV:
        monkeypatch.setenv("DFE_WFG_MAP_LARGE", "1")
        fl = _fwd(lib, st, dev, ac, use_map=True)
        monkeypatch.delenv("DFE_WFG_MAP_LARGE")
        _same(tag + " map of DFE_WFG_MAP_LARGE", _bwd(lib, st, dev, wd, dev["gx"], ac, fmap=fl["map"]), bw, ("g_warped", "g_c1", "g_c2", "g_flow"))


@pytest.mark.parametrize("shape", PC.ALIGN_SHAPES)
def test_level_every_pointer_one_float_off_in_turn(shape, monkeypatch):
    """the pointers the correlation launchers look at send the call to the dword kernels (asserted from the launcher's rule and
    the plan query), the others reach the warp kernels only; the bits are those of the aligned run either way.  The lists
    LEVEL_*_VEC_PTRS restate which arguments dfe_pwc_level_fwd / _bwd hand to launch_corr_fwd / launch_corr_bwd: the ``vec``
    assertions name the kernel a run is expected to take and would not notice a change of the launchers' own list; the
    bit-equality is what tests."""
    _clean_env(monkeypatch)
    lib, st = _lib()
    B, C, H, W = shape
    case = [s for s, _, _ in PC.LEVEL].index(shape)
    d, dev = _data(*PC.LEVEL[case])
    xbs = (NK + C + 2) * H * W
    fw = _fwd(lib, st, dev, 0)
    for name in PC.LEVEL_FWD_PTRS:
        offs = [int(name == k) for k in PC.LEVEL_FWD_VEC_PTRS]
        plan = G.corr_plan(lib, shape, G.rule_corr_vec(W, offs, [xbs]))
        assert plan["coarse"] == 0 and plan["vec"] == int(W % 4 == 0 and name not in PC.LEVEL_FWD_VEC_PTRS), (name, plan)
        _same("level_fwd %s %s one float off" % (shape, name), _fwd(lib, st, dev, 0, off=name), fw, ("warped", "x"))
    wd = fw["warped"].view.contiguous()
    bw = _bwd(lib, st, dev, wd, dev["gx"], 0)
    fm = _fwd(lib, st, dev, 0, use_map=True)
    for name in PC.LEVEL_BWD_PTRS:
        offs = [int(name == k) for k in PC.LEVEL_BWD_VEC_PTRS]
        plan = G.corr_plan(lib, shape, G.rule_corr_vec(W, offs, [xbs, xbs]), sides=2)
        assert plan["vec"] == int(W % 4 == 0 and name not in PC.LEVEL_BWD_VEC_PTRS), (name, plan)
        _same("level_bwd %s %s one float off" % (shape, name), _bwd(lib, st, dev, wd, dev["gx"], 0, off=name), bw, ("g_warped", "g_c1", "g_c2", "g_flow"))
        _same("level_bwd_map %s %s one float off" % (shape, name), _bwd(lib, st, dev, wd, dev["gx"], 0, off=name, fmap=fm["map"]), bw,
              ("g_warped", "g_c1", "g_c2", "g_flow"))


def test_level_refuses_without_touching_a_buffer(monkeypatch):
    _clean_env(monkeypatch)
    lib, st = _lib()
    B, C, H, W = 1, 8, 16, 32
    ones = lambda *s: G.Carved(s, 0, fill=torch.ones(s).cuda())
    c1, c2, flow, warped, gx = ones(B, C, H, W), ones(B, C, H, W), ones(B, 2, H, W), ones(B, C, H, W), ones(B, NK + C + 2, H, W)
    ins = (c1, c2, flow, warped, gx)
    out_w, x = G.Carved((B, C, H, W), 0), G.Carved((B, NK + C + 2, H, W), 0)
    g_w, g_c1, g_c2, g_flow = G.Carved((B, C, H, W), 0), G.Carved((B, C, H, W), 0), G.Carved((B, C, H, W), 0), G.Carved((B, 2, H, W), 0)
    nws, nmap = int(lib.dfe_scatter_ws_bytes(B * C * H * W)), int(lib.dfe_pwc_level_map_bytes(B, H, W))
    ws, ws8, mp, mp4 = G.CarvedBytes((nws,), 0), G.CarvedBytes((nws,), 8), G.CarvedBytes((nmap,), 0), G.CarvedBytes((nmap,), 4)
    dims = (B, C, H, W, 0, st)
    bwd_in = (_p(c1), _p(c2), _p(flow), _p(warped), _p(gx), _p(g_w), _p(g_c1))
    assert lib.dfe_pwc_level_bwd(*bwd_in, None, None, None, *dims) == -1                       # neither g_c2 nor g_flow
    assert lib.dfe_pwc_level_bwd(*bwd_in, _p(g_c2), None, _p(g_flow), *dims) == -1             # g_c2 without its workspace
    assert lib.dfe_pwc_level_bwd(*bwd_in, _p(g_c2), _p(ws8), _p(g_flow), *dims) == -2          # the gather's workspace off 16 bytes
    assert lib.dfe_pwc_level_bwd(*bwd_in, _p(g_c2), _p(ws8), _p(g_flow), B, 7, H, W, 0, st) == -2      # ... and the scatter's (C = 7)
    assert lib.dfe_pwc_level_bwd_map(*bwd_in, _p(g_c2), _p(mp4), _p(g_flow), *dims) == -2      # a misaligned map
    assert lib.dfe_pwc_level_bwd_map(*bwd_in, _p(g_c2), None, _p(g_flow), *dims) == -1
    assert lib.dfe_pwc_level_bwd_map(*bwd_in, None, _p(mp), None, *dims) == -1
    assert lib.dfe_pwc_level_bwd_map(*bwd_in, _p(g_c2), _p(mp), _p(g_flow), B, 7, H, W, 0, st) == -4   # the map needs C >= 8
    fwd_in = (_p(c1), _p(c2), _p(flow), _p(out_w), _p(x))
    assert lib.dfe_pwc_level_fwd_map(*fwd_in, _p(mp4), *dims) == -2
    assert lib.dfe_pwc_level_fwd_map(*fwd_in, None, *dims) == -1
    assert lib.dfe_pwc_level_fwd_map(*fwd_in, _p(mp), B, 7, H, W, 0, st) == -4
    assert lib.dfe_pwc_level_fwd(_p(c1), _p(c2), _p(flow), None, _p(x), *dims) == -1
    assert lib.dfe_pwc_level_fwd(*fwd_in, B, C, 0, W, 0, st) == -2
    assert lib.dfe_pwc_level_map_bytes(0, H, W) == -2 and lib.dfe_scatter_ws_bytes(0) == 0
    torch.cuda.synchronize()
    for c in (out_w, x, g_w, g_c1, g_c2, g_flow, ws, ws8, mp, mp4):
        assert c.untouched() and c.intact()
    for c in ins:
        assert c.intact() and bool((c.view == 1).all())
