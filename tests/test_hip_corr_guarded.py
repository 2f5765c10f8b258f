"""GPU: the PWC cost volume and its two gradients (csrc/ops_corr.hip) through the C ABI in guarded, poisoned buffers
(tests/guarded.py) at the launch plans of tests/pwc_cases.py -- the fine forward plan training's batch selects (on the 16-byte and
on the dword kernel), the coarse plan with 10 staged quads, channel splits with empty slots and with KS = C, one / two / three
chunks; the backward with 3 / 2 / 1 channel groups per block, NCG 3 and NCG 2 tiles above 64 KB of LDS, 320 threads, two and three
staging batches,
displacement rows split 9 / 3 / 1 ways, both gradients and each one alone.  What a shape runs is the library's own answer
(dfe_corr_fwd_plan / dfe_corr_bwd_plan), asserted for every case.

Every call: return code 0, guards intact, every output element written and finite, inputs unchanged.  Every element keeps
e = |out - ref64| / (2^-24 A), A = 1/C sum |f1||f2| (forward) or 1/C sum |gout||f| (gradients), within 4 max(1, e of the same sum
in plain fp32 in channel / displacement order).  At the two fine-plan shapes every pointer is moved one float off a 16-byte
boundary in turn: the launcher's rule then picks the dword kernel, and the bits are those of the aligned run."""
import ctypes
import functools

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


def _has(plan, want):
    return all(plan[k] == v for k, v in want.items())


@functools.lru_cache(maxsize=None)
def _inputs(shape, family):
    gen = torch.Generator().manual_seed(sum(shape) + len(family))
    B, C, H, W = shape
    f1, f2 = G.make_input(shape, family, gen), G.make_input(shape, family, gen)
    return f1, f2, torch.randn(B, G.CR_NK, H, W, generator=gen)


@functools.lru_cache(maxsize=None)
def _fwd_refs(shape, family):
    f1, f2, _ = _inputs(shape, family)
    return G.corr_ref(f1, f2, F32), G.corr_ref(f1, f2, F64), G.corr_ref(f1, f2, F64, absolute=True)


@functools.lru_cache(maxsize=None)
def _bwd_refs(shape, family):
    f1, f2, gout = _inputs(shape, family)
    return G.corr_bwd_ref(f1, f2, gout, F32), G.corr_bwd_ref(f1, f2, gout, F64), G.corr_bwd_ref(f1, f2, gout, F64, absolute=True)


def _run_fwd(lib, st, shape, family, offs):
    B, C, H, W = shape
    f1, f2, _ = _inputs(shape, family)
    d1, d2 = f1.cuda(), f2.cuda()
    c1, c2, out = _carve(d1, offs[0]), _carve(d2, offs[1]), G.Carved((B, G.CR_NK, H, W), offs[2])
    tag = "corr_fwd %s offs %s" % (shape, offs)
    assert lib.dfe_corr_fwd(_p(c1), _p(c2), _p(out), B, C, H, W, 4, st) == 0, tag
    _check(tag, [c1, c2, out], [out], [(c1, d1), (c2, d2)])
    return out


def _run_bwd(lib, st, shape, family, offs, want=(True, True)):
    B, C, H, W = shape
    f1, f2, gout = _inputs(shape, family)
    d1, d2, dg = f1.cuda(), f2.cuda(), gout.cuda()
    c1, c2, cg = _carve(d1, offs[0]), _carve(d2, offs[1]), _carve(dg, offs[2])
    g1 = G.Carved(shape, offs[3]) if want[0] else None
    g2 = G.Carved(shape, offs[4]) if want[1] else None
    tag = "corr_bwd %s offs %s grads %s" % (shape, offs, want)
    assert lib.dfe_corr_bwd(_p(c1), _p(c2), _p(cg), _p(g1), _p(g2), B, C, H, W, 4, st) == 0, tag
    outs = [g for g in (g1, g2) if g]
    _check(tag, [c1, c2, cg] + outs, outs, [(c1, d1), (c2, d2), (cg, dg)])
    return g1, g2


@pytest.mark.parametrize("shape,family,want", PC.CORR_FWD)
def test_corr_forward_at_every_plan(shape, family, want):
    lib, st = _lib()
    B, C, H, W = shape
    plan = G.corr_plan(lib, shape, vec=G.rule_corr_vec(W, [0, 0, 0], [G.CR_NK * H * W]))
    assert _has(plan, want), (shape, plan)
    out = _run_fwd(lib, st, shape, family, (0, 0, 0))
    y32, r64, A = _fwd_refs(shape, family)
    G.check_bound("corr_fwd %s %s %s" % (shape, family, plan), out.cpu(), y32, r64, A)
    if B * H * W <= 20000:            # the small shapes also with every tensor off a 16-byte boundary, each by another amount
        assert G.bits_equal_dev(_run_fwd(lib, st, shape, family, (1, 2, 3)).view, out.view), (shape, "the result depends on the alignment")


@pytest.mark.parametrize("shape,family,want2,want1", PC.CORR_BWD)
def test_corr_backward_at_every_plan(shape, family, want2, want1):
    lib, st = _lib()
    B, C, H, W = shape
    vec = G.rule_corr_vec(W, [0] * 5, [G.CR_NK * H * W])
    p2, p1 = G.corr_plan(lib, shape, vec, sides=2), G.corr_plan(lib, shape, vec, sides=1)
    assert _has(p2, want2) and _has(p1, want1), (shape, p2, p1)
    y32, r64, A = _bwd_refs(shape, family)
    g1, g2 = _run_bwd(lib, st, shape, family, (0,) * 5)
    G.check_bound("corr_bwd g1 %s %s %s" % (shape, family, p2), g1.cpu(), y32[0], r64[0], A[0])
    G.check_bound("corr_bwd g2 %s %s %s" % (shape, family, p2), g2.cpu(), y32[1], r64[1], A[1])
    a1, none = _run_bwd(lib, st, shape, family, (0,) * 5, (True, False))
    assert none is None
    G.check_bound("corr_bwd g1 alone %s %s %s" % (shape, family, p1), a1.cpu(), y32[0], r64[0], A[0])
    none, a2 = _run_bwd(lib, st, shape, family, (0,) * 5, (False, True))
    G.check_bound("corr_bwd g2 alone %s %s %s" % (shape, family, p1), a2.cpu(), y32[1], r64[1], A[1])
    if B * H * W <= 20000:
        b1, b2 = _run_bwd(lib, st, shape, family, (1, 2, 3, 1, 2))
        assert G.bits_equal_dev(b1.view, g1.view) and G.bits_equal_dev(b2.view, g2.view), (shape, "the result depends on the alignment")


@pytest.mark.parametrize("shape", PC.ALIGN_SHAPES)
def test_corr_every_pointer_one_float_off_in_turn(shape):
    """What tests here is the bit-equality.  The kernel named for each run comes from guarded.rule_corr_vec, a restatement of the
    launchers' al16 / % 4 list that the plan query only combines with W % 4: a pointer added to or dropped from that list in
    csrc/ops_corr.hip would go unnoticed by the ``vec`` assertions (the query is not told the pointers)."""
    lib, st = _lib()
    B, C, H, W = shape
    family = "randn"
    stride = [G.CR_NK * H * W]
    base = _run_fwd(lib, st, shape, family, (0, 0, 0))
    assert G.corr_plan(lib, shape, G.rule_corr_vec(W, [0, 0, 0], stride))["vec"] == int(W % 4 == 0)
    for k, name in enumerate(PC.CORR_FWD_PTRS):
        offs = tuple(int(i == k) for i in range(3))
        plan = G.corr_plan(lib, shape, G.rule_corr_vec(W, offs, stride))
        assert plan["vec"] == 0 and plan["coarse"] == 0, (name, plan)
        assert G.bits_equal_dev(_run_fwd(lib, st, shape, family, offs).view, base.view), (shape, name, "forward bits depend on the alignment")
    g1, g2 = _run_bwd(lib, st, shape, family, (0,) * 5)
    for k, name in enumerate(PC.CORR_BWD_PTRS):
        offs = tuple(int(i == k) for i in range(5))
        assert G.corr_plan(lib, shape, G.rule_corr_vec(W, offs, stride), sides=2)["vec"] == 0, name
        b1, b2 = _run_bwd(lib, st, shape, family, offs)
        assert G.bits_equal_dev(b1.view, g1.view) and G.bits_equal_dev(b2.view, g2.view), (shape, name, "gradient bits depend on the alignment")


def test_corr_refuses_without_touching_a_buffer():
    lib, st = _lib()
    shape = (1, 3, 4, 6)
    t = torch.ones(shape).cuda()
    c1, c2, cg = _carve(t, 0), _carve(t, 0), _carve(torch.ones(1, 81, 4, 6).cuda(), 0)
    out, g1, g2 = G.Carved((1, 81, 4, 6), 0), G.Carved(shape, 0), G.Carved(shape, 0)
    assert lib.dfe_corr_fwd(_p(c1), _p(c2), _p(out), 1, 3, 4, 6, 3, st) == -4          # d != 4
    assert lib.dfe_corr_bwd(_p(c1), _p(c2), _p(cg), _p(g1), _p(g2), 1, 3, 4, 6, 5, st) == -4
    assert lib.dfe_corr_bwd(_p(c1), _p(c2), _p(cg), None, None, 1, 3, 4, 6, 4, st) == -1      # no gradient asked for
    assert lib.dfe_corr_fwd(_p(c1), None, _p(out), 1, 3, 4, 6, 4, st) == -1
    assert lib.dfe_corr_fwd(_p(c1), _p(c2), _p(out), 1, 0, 4, 6, 4, st) == -2
    torch.cuda.synchronize()
    for c in (out, g1, g2):
        assert c.untouched() and c.intact()
    for c in (c1, c2, cg):
        assert c.intact() and bool((c.view == 1).all())
