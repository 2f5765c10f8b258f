"""CPU: self-tests of tests/guarded.py -- the guard bands notice a write one float before a view, one float after it and into a
batch gap (and nothing else), and the plain-torch Winograd emulations that serve as the fp32 yardstick compute, in float64, what
aten's float64 convolution / weight gradient computes."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import glue_cases as GC
from tests import guarded as G
from tests import loss_stack_cases as LC
from tests import pwc_cases as PC

CPU = torch.device("cpu")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("gap", [0, 1, 5])
def test_carved_guards_notice_stray_writes(off, gap):
    shape, dense = (3, 2, 3, 5), 30
    vals = torch.arange(90, dtype=torch.float32).reshape(shape)
    c = G.Carved(shape, off, dense + gap, fill=vals, device=CPU)
    flat = c.bits.view(torch.float32)
    assert c.view.data_ptr() % 16 == 4 * off and c.view.stride() == (dense + gap, 15, 5, 1)
    assert c.lo >= 64 and c.bits.numel() - (c.lo + c.span) >= 64
    assert c.intact() and c.written() and torch.equal(c.cpu(), vals)
    c.view[1, 1, 2, 4] = -1.0                  # inside the view: allowed
    c.view[2, 1, 2, 4] = -2.0                  # the view's last element
    c.view[0, 0, 0, 0] = -3.0                  # ... and its first
    assert c.intact()
    for pos in [c.lo - 1, c.lo + c.span] + ([c.lo + dense, c.lo + 2 * (dense + gap) - 1] if gap else []):
        old = c.bits[pos].clone()
        flat[pos] = 0.0
        assert not c.intact(), pos
        c.bits[pos] = old
        assert c.intact()
    flat[0] = 1.0                              # the far end of the guard band
    assert not c.intact()


def test_carved_poisoned_payload_and_one_dimensional_views():
    c = G.Carved((7,), 3, device=CPU)
    assert c.intact() and c.untouched() and not c.written() and bool(torch.isnan(c.view).all())
    c.view[:6] = 1.0
    assert not c.written() and not c.untouched()                 # one element nobody wrote
    c.view[6] = float("inf")
    assert not c.written()
    c.view[6] = 0.0
    assert c.written() and c.intact()
    g = G.Carved((2, 4), 0, 6, device=CPU)                       # the gap stays NaN when the payload is filled
    g.view.fill_(2.0)
    assert g.intact() and int(torch.isnan(g.bits.view(torch.float32)[g.lo:g.lo + g.span]).sum()) == 2


def test_sparse_family_has_zero_blocks_and_a_zero_channel():
    gen = torch.Generator().manual_seed(1)
    x = G.make_input((2, 6, 9, 10), "sparse", gen)
    assert float(x[0, :, 0:4, 0:4].abs().max()) == 0.0 and float(x[1, :, 8:, 8:].abs().max()) == 0.0 and float(x[:, 3].abs().max()) == 0.0
    assert float(x.min()) == 0.0 and float(x.max()) > 0.0
    assert float(G.make_input((1, 2, 4, 4), "act", gen).min()) >= 1.0


# (B, Ci, Co, H, W, P, dilation)
EMU_SHAPES = [(1, 512, 4, 6, 6, 1, 1), (2, 5, 3, 3, 3, 0, 1), (2, 6, 17, 3, 4, 0, 1), (1, 4, 33, 1, 2, 1, 1), (2, 12, 20, 7, 9, 1, 1), (2, 8, 8, 6, 8, 2, 1),
              (1, 7, 40, 5, 5, 2, 1), (2, 9, 20, 6, 12, 1, 3), (1, 8, 8, 4, 4, 1, 2)]


@pytest.mark.parametrize("shape", EMU_SHAPES)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_winograd_emulation_in_float64_is_atens_convolution(shape, family):
    """|emulation64 - aten64| <= (Ci + 32) 2^-53 S_w per element (float64 roundings of Ci products and the transforms, each
    bounded by the Winograd-domain absolute sum), forward and data-gradient form."""
    B, Ci, Co, H, W, P, d = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = G.make_input((B, Ci, H, W), family, gen)
    for transposed in (False, True):
        w = G.make_weight(Ci, Co, 3, gen) if transposed else G.make_weight(Co, Ci, 3, gen)
        ref = G.wino_conv_ref64(x, w, P, d, transposed)
        emu = G.wino_conv(x, w, P, d, transposed, torch.float64)
        Sw = G.wino_conv(x, w, P, d, transposed, torch.float64, absolute=True)
        assert emu.shape == ref.shape == Sw.shape
        assert bool(((emu - ref).abs() <= (Ci + 32) * 2.0 ** -53 * Sw).all()), float((emu - ref).abs().max())
        assert float((G.wino_conv(x, w, P, d, transposed, torch.float32).double() - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))


WG_EMU_SHAPES = [(1, 1, 1, 3, 3, 0), (2, 5, 3, 3, 3, 1), (1, 33, 17, 5, 27, 1), (2, 40, 70, 4, 50, 0), (1, 130, 64, 6, 10, 1)]


@pytest.mark.parametrize("shape", WG_EMU_SHAPES)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_winograd_wgrad_emulation_in_float64_is_atens_weight_gradient(shape, family):
    B, Ci, Co, H, W, P = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = G.make_input((B, Ci, H, W), family, gen)
    gy = G.make_input((B, Co, H + 2 * P - 2, W + 2 * P - 2), family, gen)
    ref = G.conv_wgrad_ref(gy, x, 3, 1, P, 1, torch.float64)
    emu = G.wino_wgrad(x, gy, P, torch.float64)
    Sw = G.wino_wgrad(x, gy, P, torch.float64, absolute=True)
    ntiles = B * ((H + 2 * P - 1) // 2) * ((W + 2 * P - 1) // 2)
    assert emu.shape == ref.shape == Sw.shape == (Co, Ci, 3, 3)
    assert bool(((emu - ref).abs() <= (ntiles + 32) * 2.0 ** -53 * Sw).all()), float((emu - ref).abs().max())


# ========================================================================================================= glue and head helpers
# Self-tests of what test_hip_glue_guarded.py and test_hip_head_guarded.py rely on: the byte carve, the float64 references
# against ATen's float64 operators, the restated launch rules on the shapes of the matrices (tests/glue_cases.py), that every
# matrix reaches every branch of its launcher, and the margin of every thresholded decision.


@pytest.mark.parametrize("off", [0, 1, 5, 15])
def test_byte_carve_notices_a_stray_byte(off):
    c = G.CarvedBytes((2, 3, 5), off, device=CPU)
    assert c.view.data_ptr() % 16 == off and c.intact() and c.untouched() and not c.written()
    assert c.lo >= 64 and c.bits.numel() - (c.lo + c.span) >= 64 and G.BYTE_SENTINEL > 8
    c.view.fill_(8)
    c.view[1, 2, 4] = 0
    assert c.intact() and c.written() and not c.untouched()
    c.view[0, 0, 0] = 9                          # not a window position
    assert not c.written()
    c.view[0, 0, 0] = 3
    for pos in (c.lo - 1, c.lo + c.span, 0, c.bits.numel() - 1):
        c.bits[pos] = 0
        assert not c.intact(), pos
        c.bits[pos] = G.BYTE_SENTINEL
        assert c.intact()


def _close64(a, b, A=None):
    """float64 expressions of the same value: a few float64 roundings of the absolute sum apart"""
    A = b.abs() if A is None else A
    return a.shape == b.shape and a.dtype == b.dtype == torch.float64 and bool(((a - b).abs() <= 64 * 2.0 ** -53 * (A + 1e-300)).all())


def test_epilogue_and_decoder_references_are_atens_float64_operators():
    gen = torch.Generator().manual_seed(3)
    x, b = torch.randn(2, 3, 4, 6, generator=gen), torch.randn(3, generator=gen)
    v = (x.double() + b.double()[None, :, None, None]).requires_grad_(True)
    for slope in GC.EP_SLOPES:
        assert torch.equal(G.bias_act_ref(x, b, slope, torch.float64), F.leaky_relu(v, slope).detach())
        y = F.leaky_relu(v, slope)
        g = torch.randn(x.shape, generator=gen, dtype=torch.float64)
        assert torch.equal(G.bias_act_bwd_ref(y.detach(), g, slope), torch.autograd.grad(y, v, g)[0])
    assert torch.equal(G.bias_act_ref(x, None, 0.1, torch.float32), F.leaky_relu(x, 0.1))
    # ELU, reflection pad, bilinear x2: values and gradients through autograd
    for apply_elu in (0, 1):
        ref = F.pad(F.elu(v) if apply_elu else v, (1, 1, 1, 1), mode="reflect")
        assert _close64(G.elu_pad_ref(x, b, apply_elu, torch.float64), ref.detach())
        g = torch.randn(ref.shape, generator=gen)
        assert _close64(G.elu_pad_bwd_ref(x, b, g, apply_elu, torch.float64), torch.autograd.grad(ref, v, g.double())[0],
                        G.elu_pad_bwd_ref(x, b, g, apply_elu, torch.float64, absolute=True))
    skip = torch.randn(2, 2, 8, 12, generator=gen)
    sk = skip.double().requires_grad_(True)
    ref = F.pad(torch.cat([F.interpolate(F.elu(v), scale_factor=2, mode="bilinear", align_corners=False), sk], 1), (1, 1, 1, 1), mode="reflect")
    assert _close64(G.up2_cat_pad_ref(x, b, skip, torch.float64), ref.detach())
    g = torch.randn(ref.shape, generator=gen)
    gx, gs = torch.autograd.grad(ref, (v, sk), g.double())
    rx, rs = G.up2_cat_pad_bwd_ref(x, b, g, torch.float64)
    ax, as_ = G.up2_cat_pad_bwd_ref(x, b, g, torch.float64, absolute=True)
    assert _close64(rx, gx, ax) and _close64(rs, gs, as_) and bool((ax >= rx.abs()).all()) and bool((as_ >= rs.abs()).all())
    assert G.up2_cat_pad_bwd_ref(x, b, g[:, :3], torch.float64)[1] is None
    assert bool((G.up2_cat_pad_A(x, b) >= G.up2_cat_pad_ref(x, b, None, torch.float64).abs()).all())


@pytest.mark.parametrize("G_,relu,with_res", [(1, 0, False), (2, 1, True), (3, 1, False)])
def test_batch_norm_reference_is_atens_float64_batch_norm(G_, relu, with_res):
    Bg, C, H, W = 2, 3, 4, 5
    c = G.bn_case(G_, Bg, C, H, W, relu, with_res, 11)
    x, w, b, ref = c["x"].double(), c["weight"].double(), c["bias"].double(), c["ref"]
    rm, rv = c["rmean"].double().clone(), c["rvar"].double().clone()
    xr = x.clone().requires_grad_(True)
    wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ys = [F.batch_norm(xr[g * Bg:(g + 1) * Bg], rm, rv, wr, br, True, c["momentum"], c["eps"]) for g in range(G_)]
    y = torch.cat(ys, 0)
    res = c["res"].double().requires_grad_(True) if with_res else None
    if with_res:
        y = y + res
    y = y.relu() if relu else y
    assert _close64(ref["y"], y.detach(), ref["A_y"]) and _close64(ref["rmean"], rm, ref["A_rmean"]) and _close64(ref["rvar"], rv, ref["A_rvar"])
    for g in range(G_):
        xs = x[g * Bg:(g + 1) * Bg]
        assert _close64(ref["mean"][g * C:(g + 1) * C], xs.mean((0, 2, 3)), ref["A_mean"][g * C:(g + 1) * C])
        assert _close64(ref["invstd"][g * C:(g + 1) * C], 1.0 / torch.sqrt(xs.var((0, 2, 3), unbiased=False) + c["eps"]), ref["A_invstd"][g * C:(g + 1) * C])
    gy = c["gy"]
    grads = torch.autograd.grad(y, (xr, wr, br) + ((res,) if with_res else ()), gy.double())
    bw = G.bn_bwd_ref(c["x"], ref["y"], gy, c["weight"], ref["mean"], ref["invstd"], G_, Bg, relu)
    assert _close64(bw["gx"], grads[0], bw["A_gx"]) and _close64(bw["gweight"], grads[1], bw["A_gweight"]) and _close64(bw["gbias"], grads[2], bw["A_gbias"])
    if with_res:
        assert torch.equal(bw["gres"], grads[3])
    # the fp32 yardsticks are the same functions
    yy, m, i, rm32, rv32 = G.bn_fwd_yard(c["x"], c["res"], c["weight"], c["bias"], c["rmean"], c["rvar"], G_, Bg, c["eps"], c["momentum"], relu)
    assert float((yy.double() - ref["y"]).abs().max()) < 1e-5 and float((m.double() - ref["mean"]).abs().max()) < 1e-6
    assert float((i.double() - ref["invstd"]).abs().max()) < 1e-5 and float((rv32.double() - ref["rvar"]).abs().max()) < 1e-6
    gx32, gw32, gb32 = G.bn_bwd_yard(c["x"], yy, gy, c["weight"], m, i, G_, Bg, relu, c["eps"])
    assert float((gx32.double() - bw["gx"]).abs().max()) < 1e-4 and float((gw32.double() - bw["gweight"]).abs().max()) < 1e-3


@pytest.mark.parametrize("shape", GC.POOL_SHAPES)
def test_pool_reference_positions_point_at_atens_gradient(shape):
    gen = torch.Generator().manual_seed(sum(shape))
    x = G.pool_input(*shape, gen)
    planes, H, W = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(planes, Ho, Wo, generator=gen)
    y, gx, pos = G.pool_ref(x, gy)
    assert y.shape == (planes, Ho, Wo) and int(pos.min()) >= 0 and int(pos.max()) <= 8
    if H * W > 16:
        assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).any()) and int((x == 0).sum()) > 1
    # scattering gy to the recorded positions in output order is ATen's gradient
    acc = torch.zeros(planes, H, W)
    for p in range(planes):
        for oy in range(Ho):
            for ox in range(Wo):
                k = int(pos[p, oy, ox])
                iy, ix = 2 * oy - 1 + k // 3, 2 * ox - 1 + k % 3
                assert 0 <= iy < H and 0 <= ix < W
                assert G.bits_equal(x[p, iy, ix].reshape(1), y[p, oy, ox].reshape(1))
                acc[p, iy, ix] += gy[p, oy, ox]
    assert G.bits_equal(acc, gx)


def test_head_references_are_atens_float64_convolution_and_gradients():
    gen = torch.Generator().manual_seed(8)
    p, w, b = torch.randn(2, 16, 7, 9, generator=gen), torch.randn(1, 16, 3, 3, generator=gen) * 0.2, torch.randn(1, generator=gen)
    pr, wr, br = p.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    out = torch.sigmoid(F.conv2d(pr, wr, br))
    assert torch.equal(G.disp_head_ref(p, w, b, torch.float64), out.detach())
    gout = torch.randn(out.shape, generator=gen)
    grads = torch.autograd.grad(out, (pr, wr, br), gout.double())
    mine = G.disp_head_bwd_ref(p, w, out.detach(), gout, torch.float64)
    A = G.disp_head_bwd_ref(p, w, out.detach(), gout, torch.float64, absolute=True)
    for m, g, a in zip(mine, grads, A):
        assert _close64(m, g, a) and bool((a >= m.abs() * (1 - 1e-12)).all())
    A = G.disp_head_ref(p, w, b, torch.float64, absolute=True)
    assert bool((A >= 1.0).all()) and A.shape == out.shape
    x, w2, b2 = torch.randn(2, 8, 5, 6, generator=gen), torch.randn(2, 8, 3, 3, generator=gen), torch.randn(2, generator=gen)
    xr, wr, br = x.double().requires_grad_(True), w2.double().requires_grad_(True), b2.double().requires_grad_(True)
    out = F.conv2d(xr, wr, br, 1, 1)
    assert torch.equal(G.flow_head_ref(x, w2, b2, torch.float64), out.detach())
    gout = torch.randn(out.shape, generator=gen)
    for m, g, a in zip(G.flow_head_bwd_ref(x, w2, gout, torch.float64), torch.autograd.grad(out, (xr, wr, br), gout.double()),
                       G.flow_head_bwd_ref(x, w2, gout, torch.float64, absolute=True)):
        assert _close64(m, g, a)


# --------------------------------------------------------------------------------------------------------- launch rules
def test_launch_rules_on_the_listed_shapes():
    assert G.rule_elu_pad_fwd(8, 0) == "pair" and G.rule_elu_pad_fwd(8, 1) == "scalar" and G.rule_elu_pad_fwd(2, 0) == "scalar" and G.rule_elu_pad_fwd(3, 0) == "scalar"
    assert G.rule_elu_pad_bwd(8, 0, 0, 1) == "quad" and G.rule_elu_pad_bwd(8, 0, 2, 1) == "pair" and G.rule_elu_pad_bwd(8, 0, 2, 0) == "quad"
    assert G.rule_elu_pad_bwd(12, 2, 0, 1) == "pair" and G.rule_elu_pad_bwd(12, 1, 0, 1) == "scalar" and G.rule_elu_pad_bwd(6, 0, 0, 1) == "pair"
    assert G.rule_elu_pad_bwd(4, 0, 0, 1) == "pair" and G.rule_elu_pad_bwd(8, 0, 1, 1) == "scalar" and G.rule_elu_pad_bwd(2, 0, 0, 0) == "scalar"
    assert G.rule_up2_bwd(1, 1, 0) == {"tile32"} and G.rule_up2_bwd(17, 33, 0) == {"tile64"} and G.rule_up2_bwd(5, 65, 0) == {"tile64"}
    assert G.rule_up2_bwd(3, 65, 0) == {"element"} and G.rule_up2_bwd(3, 65, 1) == {"element"}
    assert G.rule_up2_bwd(50, 196, 0) == {"tile64", "tile64-inner"} and G.rule_up2_bwd(50, 196, 1) == {"element", "element-interior"}
    assert G.rule_up2_bwd(33, 65, 0) == {"tile64"} and G.rule_up2_bwd(19, 300, 0) == {"tile64"}      # the operator tests' largest: no inner tile
    assert G.rule_up2_bwd(34, 130, 0) == {"tile64", "tile64-inner"} and G.rule_up2_bwd(33, 130, 0) == {"tile64"} and G.rule_up2_bwd(34, 129, 0) == {"tile64"}
    assert G.up2_bwd_blocks(3, 65, 0) == 1 and G.up2_bwd_blocks(17, 33, 0) == 2 and G.up2_bwd_blocks(17, 33, 1) == 3 and G.up2_bwd_blocks(50, 196, 0) == 16
    assert G.rule_skip(5, 0) == "pair" and G.rule_skip(2, 0) == "pair" and G.rule_skip(196, 0) == "quad" and G.rule_skip(196, 2) == "pair" and G.rule_skip(196, 1) == "scalar"
    assert G.rule_skip(1, 0) == "scalar" and G.rule_up2_fwd(1, 0) == "scalar" and G.rule_up2_fwd(5, 0) == "pair" and G.rule_up2_fwd(5, 1) == "scalar"
    assert G.rule_epilogue_vec(208, [0, 0, 0], [4]) and not G.rule_epilogue_vec(208, [0, 0, 0], [2]) and not G.rule_epilogue_vec(208, [0, 1, 0], [0])
    assert not G.rule_epilogue_vec(63, [0, 0], []) and G.rule_epilogue_vec(52, [0, None, 0], [None, 288])
    assert G.rule_bn(3, 2, 208, [0, 0]) == ("small", 3, 64) and G.rule_bn(1, 4, 256, [0, 0]) == ("small", 1, 64) and G.rule_bn(2, 2, 224, [0, 0]) == ("small", 1, 64)
    assert G.rule_bn(2, 4, 260, [0]) == ("small", 1, 256) and G.rule_bn(3, 4, 1024, [0]) == ("small", 3, 256) and G.rule_bn(2, 4, 1028, [0]) == ("small", 1, 1024)
    assert G.rule_bn(1, 4, 4096, [0]) == ("small", 1, 1024) and G.rule_bn(1, 4, 4100, [0]) == ("three", "vec") and G.rule_bn(1, 5, 256, [0]) == ("three", "vec")
    assert G.rule_bn(2, 4, 1040, [1, 0]) == ("three", "scalar") and G.rule_bn(2, 4, 975, [0]) == ("three", "scalar") and G.rule_bn(4, 3, 4352, [0]) == ("three", "vec")
    for R, B, H, W in GC.HEAD_R_CASES:
        for flow, C in ((False, 16), (True, 8), (True, 136)):
            plan = G.rule_head_fwd(B, C, H, W, flow)
            assert plan == dict(par=False, R=R, ns=2 if W == 63 else 1, nrb=(H + R - 1) // R), (R, B, H, W, plan)
    assert G.rule_head_fwd(12, 16, 64, 208, False)["R"] == 2 and G.rule_head_fwd(12, 16, 256, 832, False)["R"] == 16 and G.rule_head_fwd(12, 16, 128, 416, False)["R"] == 4
    assert G.rule_head_fwd(2, 32, 5, 63, True) == dict(par=True, R=4, ns=2, nrb=2) and G.rule_head_fwd(2, 128, 1, 62, True) == dict(par=True, R=4, ns=1, nrb=1)
    assert not G.rule_head_fwd(2, 24, 5, 63, True)["par"] and not G.rule_head_fwd(2, 136, 5, 63, True)["par"]
    assert G.rule_head_bwd(16, 14, 60, False) == dict(ns=1, nrb=1, nz=1) and G.rule_head_bwd(48, 15, 61, False) == dict(ns=2, nrb=2, nz=3)
    assert G.rule_head_bwd(24, 15, 62, True) == dict(ns=2, nrb=2, nz=3) and G.rule_head_bwd(8, 14, 62, True) == dict(ns=2, nrb=1, nz=1)


def test_the_cases_reach_every_branch_of_the_epilogue():
    for name, variants, rule in (("fwd2", GC.EP_FWD2, GC.ep_fwd2_vec), ("bwd", GC.EP_BWD, GC.ep_bwd_vec), ("bwd2", GC.EP_BWD2, GC.ep_bwd2_vec)):
        reached = {(rule(s[2] * s[3], v), -(-s[2] * s[3] // G.EP_CHUNK)) for s in GC.EP_SHAPES for v in variants}
        assert reached == {(True, 1), (False, 1), (True, 2), (False, 2)}, (name, reached)
        # a strided operand four floats wider stays on the vector kernel, one or two floats wider leaves it
        hw = 208
        assert any(rule(hw, v) and any(x == 4 for x in v[3:-1] if isinstance(x, int)) for v in variants), name
        assert any(not rule(hw, v) and all(o in (0, None) for o in v[:3]) for v in variants), name
    assert {G.rule_epilogue_vec(s[2] * s[3], [o], []) for s in GC.EP_SHAPES for o in (0, 1)} == {True, False}


def test_the_cases_reach_every_branch_of_elu_pad():
    cases = GC.elu_pad_cases()
    assert {(H, W) for H, W, _, _ in cases} == {(H, W) for H in GC.ELU_PAD_H for W in GC.ELU_PAD_W}
    assert {(e, b) for _, _, e, b in cases} == {(0, False), (0, True), (1, False), (1, True)}
    fwd = {(G.rule_elu_pad_fwd(W, oo), W % 2) for _, W, _, _ in cases for _, oo in GC.ELU_PAD_FWD_OFFS}
    assert fwd == {("pair", 0), ("scalar", 0), ("scalar", 1)}                       # the scalar fallback at even W included
    bwd = {(G.rule_elu_pad_bwd(W, go, xo, e), W % 4 == 0 and W >= 8) for _, W, e, _ in cases for xo, _, go in GC.ELU_PAD_BWD_OFFS}
    assert bwd == {("quad", True), ("pair", True), ("scalar", True), ("pair", False), ("scalar", False)}
    assert {o for _, o, _ in GC.ELU_PAD_BWD_OFFS} == {0, 1, 2} and {o for o, _ in GC.ELU_PAD_FWD_OFFS} == {0, 1, 2}    # the unchecked operands


def test_the_cases_reach_every_branch_of_up2_cat_pad():
    reached = set()
    for B, C1, h, w, C2 in GC.UP2_SHAPES:
        for o in GC.UP2_GOUT_OFFS:
            reached |= G.rule_up2_bwd(h, w, o)
    assert reached == {"tile32", "tile64", "tile64-inner", "element", "element-interior"}
    assert "tile64-inner" in G.rule_up2_bwd(50, 196, 0) and G.rule_up2_bwd(3, 65, 0) == {"element"}       # the element kernel on an aligned gout
    assert {G.rule_skip(w, o) for _, _, _, w, C2 in GC.UP2_SHAPES if C2 for o in GC.UP2_GSKIP_OFFS} == {"quad", "pair", "scalar"}
    assert {(G.rule_skip(w, o), w % 2) for _, _, _, w, C2 in GC.UP2_SHAPES if C2 for o in GC.UP2_GSKIP_OFFS} >= {("scalar", 0), ("pair", 0), ("pair", 1)}
    assert {G.rule_up2_fwd(w, o) for _, _, _, w, _ in GC.UP2_SHAPES for o in GC.UP2_OUT_OFFS} == {"pair", "scalar"}
    assert {C2 > 0 for *_, C2 in GC.UP2_SHAPES} == {True, False}


def test_the_cases_reach_every_branch_of_batch_norm():
    for direction in ("fwd", "bwd"):
        reached = set()
        for case in GC.bn_cases():
            for relu in (0, 1):
                for with_res in (False, True):
                    reached.add(GC.bn_rule(case, direction, relu, with_res))
        want = {("small", gb, t) for gb in (1, 3) for t in (64, 256, 1024)} | {("three", "vec"), ("three", "scalar")}
        assert reached == want, (direction, reached)
    small = {(c[0], GC.bn_rule(c, "fwd", 1, False)) for c in GC.bn_cases()}
    assert {(2, ("small", 1, t)) for t in (64, 256, 1024)} <= small                 # G = 2 on the single kernel at all three sizes
    # both sides of every threshold, at the same G
    for g in (1, 2, 3):
        by = {(c[1], c[3] * c[4]): GC.bn_rule(c, "fwd", 1, False) for c in GC.bn_cases() if c[0] == g and c[2] == 2 and c[5] is None}
        assert by[(4, 256)][2] == 64 and by[(4, 260)][2] == 256 and by[(4, 1024)][2] == 256 and by[(4, 1028)][2] == 1024 and by[(4, 4096)][2] == 1024
        assert by[(4, 4100)] == ("three", "vec") and by[(5, 256)] == ("three", "vec") and by[(5, 4096)] == ("three", "vec")
    # every tensor the launchers look at is off alignment once, at hw % 4 == 0
    for name in ("x", "y", "res"):
        assert GC.bn_rule((3, 2, 5, 8, 26, name), "fwd", 1, True) == ("three", "scalar")
    for name in ("x", "y", "gy", "gx", "gres"):
        assert GC.bn_rule((3, 2, 5, 8, 26, name), "bwd", 1, True) == ("three", "scalar")
    assert any(c[3] * c[4] > G.BN_CHUNK and (c[3] * c[4]) % G.BN_CHUNK and GC.bn_rule(c, "fwd", 1, False)[0] == "three" for c in GC.bn_cases())


def test_the_cases_reach_every_branch_of_the_heads():
    fwd = set()
    for R, B, H, W in GC.HEAD_R_CASES:
        for flow, cs in ((False, GC.DISP_C), (True, GC.FLOW_C_SERIAL)):
            for C in cs:
                plan = G.rule_head_fwd(B, C, H, W, flow)
                assert plan["R"] == R and not plan["par"]
                fwd.add((flow, plan["R"], plan["ns"]))
    assert fwd == {(f, r, 1) for f in (False, True) for r in (2, 4, 8, 16)} | {(False, 16, 2), (True, 16, 2)}
    par = {(G.rule_head_fwd(GC.PAR_B, C, H, W, True)["par"], G.rule_head_fwd(GC.PAR_B, C, H, W, True)["nrb"], G.rule_head_fwd(GC.PAR_B, C, H, W, True)["ns"])
           for C in GC.PAR_C for H in GC.PAR_H for W in GC.PAR_W}
    assert par == {(True, 1, 1), (True, 2, 1), (True, 1, 2), (True, 2, 2)}
    for flow, cs in ((False, GC.DISP_BWD_C), (True, GC.FLOW_BWD_C)):
        bwd = {tuple(G.rule_head_bwd(C, H, W, flow).values()) for C in cs for H in GC.BWD_H for W in GC.BWD_W}
        assert bwd == {(ns, nrb, nz) for ns in (1, 2) for nrb in (1, 2) for nz in (1, 3)}


# --------------------------------------------------------------------------------------------------------- decisions near zero
def test_every_decision_of_the_matrices_keeps_its_margin():
    """LeakyReLU / ReLU sign, ELU branch: by construction (the sum is an exactly representable t with |t| >= 2^-10 up to one
    rounding); BN + ReLU: bn_case picks the seed; max pooling: the inputs sit on a grid of 1/8, so unequal candidates differ by
    >= 1/8 and the comparison involves no arithmetic."""
    for shape in GC.EP_SHAPES:
        z, bias = G.epilogue_input(shape, sum(shape))
        assert G.margin_ok(z.double() + bias.double()[None, :, None, None], G.bias_act_A(z, bias))
    for H, W, apply_elu, with_bias in GC.elu_pad_cases():
        x, bias = G.elu_input((GC.ELU_PAD_BC[0], GC.ELU_PAD_BC[1], H, W), with_bias, 100 * H + W)
        assert G.margin_ok(x.double() + (bias.double()[None, :, None, None] if with_bias else 0.0), G.elu_A(x, bias))
    for B, C1, h, w, C2 in GC.UP2_SHAPES:
        for with_bias in (False, True):
            x, bias = G.elu_input((B, C1, h, w), with_bias, h * w + C2)
            assert G.margin_ok(x.double() + (bias.double()[None, :, None, None] if with_bias else 0.0), G.elu_A(x, bias))
    for case in GC.bn_cases():
        for with_res in (False, True):
            c = G.bn_case(*case[:5], 1, with_res, G.bn_seed(case, with_res))
            assert c["seed"] - G.bn_seed(case, with_res) < 40 and G.margin_ok(c["ref"]["pre"], c["ref"]["A_y"])
    for shape in GC.POOL_SHAPES:
        x = G.pool_input(*shape, torch.Generator().manual_seed(sum(shape)))
        fin = x[torch.isfinite(x)]
        assert bool((fin * 8 == torch.round(fin * 8)).all())


# ========================================================================================================= PWC level
# The case matrices of tests/pwc_cases.py against the library's own plan queries (host only: no device is touched) and the three
# restated one-line rules; the float64 references of tests/guarded.py against the oracle.
def _hip_lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib()


def _has(plan, want):
    return all(plan[k] == v for k, v in want.items())


def test_plan_queries_agree_with_hand_computed_plans(monkeypatch):
    """corr_fwd_config / corr_bwd_config worked by hand from csrc/ops_corr.hip (the workload's levels 2 and 3 at the batch of
    training, and three ragged shapes)"""
    for name in ("DFE_CORR_FWD", "DFE_CORR_BWD", "DFE_CORR_DYG"):
        monkeypatch.delenv(name, raising=False)
    lib = _hip_lib()
    # level 2: 52 quads -> 4 tiles of 13; TH 4 keeps 8*16*4 = 512 tiles; NI = 4*13*9 = 468 -> 512 threads; 512 blocks * 512 = 256 K: fine;
    # chunks of 8 channels (9 fit 36 KB); 2 * 8 * (12*15 + 4*13) * 16 bytes
    assert G.corr_plan(lib, (8, 32, 64, 208)) == dict(TH=4, TXQ=13, ntx=4, KS=1, CC=8, DYG=9, PF2=4, threads=512, lds=59392, chunks=4, coarse=0, vec=1)
    # its backward: 4 groups * 8 ch * 16 * 15 quads * 16 B = 120 KB; 8*8*4 blocks * 2 sides = 512; NI = 416 -> 448 threads; 7680 quads / (12*448)
    assert G.corr_plan(lib, (8, 32, 64, 208), sides=2) == dict(TH=8, TXQ=13, ntx=4, NCG=4, ncr=1, IS=1, threads=448, lds=122880, batches=2, vec=1)
    # level 3: 8 groups; NCG 2 is the largest that keeps 8*4*2*4 * 2 = 512 blocks: 60 KB, NI = 208 -> 256 threads
    assert G.corr_plan(lib, (8, 64, 32, 104), sides=2) == dict(TH=8, TXQ=13, ntx=2, NCG=2, ncr=4, IS=1, threads=256, lds=61440, batches=2, vec=1)
    # one pixel: TH 1, 3 displacement rows per block, NI = 3, the split is capped by C = 1; 2 * (3*3 + 1) * 16 bytes
    assert G.corr_plan(lib, (1, 1, 1, 1), vec=0) == dict(TH=1, TXQ=1, ntx=1, KS=1, CC=1, DYG=3, PF2=4, threads=64, lds=320, chunks=1, coarse=1, vec=0)
    # NI = 1*9*3 = 27 -> 18 slots, capped by C = 17: 459 work items; the reduction's 17*36*27*4 bytes exceed the staging buffers
    assert G.corr_plan(lib, (3, 17, 9, 33), vec=0) == dict(TH=1, TXQ=9, ntx=1, KS=17, CC=17, DYG=3, PF2=4, threads=512, lds=66096, chunks=1, coarse=1, vec=0)
    # the 16-byte kernels need W % 4 == 0 whatever the pointers are; a one-sided launch is planned on its own
    assert G.corr_plan(lib, (8, 13, 62, 206), vec=1)["vec"] == 0 and G.corr_plan(lib, (8, 13, 64, 208), vec=0)["vec"] == 0
    assert G.corr_plan(lib, (8, 32, 64, 208), sides=1)["NCG"] == 3
    import ctypes
    buf = (ctypes.c_int * 12)()
    assert lib.dfe_corr_fwd_plan(0, 1, 1, 1, 1, buf) == -2 and lib.dfe_corr_fwd_plan(1, 1, 1, 1, 1, None) == -1
    assert lib.dfe_corr_bwd_plan(1, 1, 1, 1, 3, 1, buf) == -2 and lib.dfe_corr_bwd_plan(1, 1, 1, 1, 1, 1, None) == -1


def test_the_cases_reach_every_plan_of_the_cost_volume(monkeypatch):
    for name in ("DFE_CORR_FWD", "DFE_CORR_BWD", "DFE_CORR_DYG"):
        monkeypatch.delenv(name, raising=False)
    lib = _hip_lib()
    fwd = []
    for shape, family, want in PC.CORR_FWD:
        plan = G.corr_plan(lib, shape, vec=1)
        assert _has(plan, want), (shape, plan, want)
        assert family in G.FAMILIES
        fwd.append((shape, plan))
    assert any(p["coarse"] == 0 and p["vec"] == 1 and p["chunks"] == 2 and s[1] % p["CC"] == p["CC"] - 1 for s, p in fwd)          # fine, 16 bytes, a short last chunk
    assert any(p["coarse"] == 0 and p["vec"] == 0 and s[2] % p["TH"] == 2 and s[3] % 4 == 2 for s, p in fwd)                          # fine, dwords, cut tile and quad
    assert any(p["coarse"] == 1 and p["PF2"] == 10 for s, p in fwd)
    assert any(p["KS"] > 1 and s[1] % p["CC"] and (s[1] % p["CC"]) < p["KS"] for s, p in fwd)                                        # empty slots in the last chunk
    assert any(p["KS"] == s[1] and s[1] > 1 for s, p in fwd)
    assert {min(p["chunks"], 3) for s, p in fwd} == {1, 2, 3} and any(p["chunks"] >= 3 and p["coarse"] == 0 for s, p in fwd)
    assert any(p["ntx"] > 1 for s, p in fwd) and {p["PF2"] for s, p in fwd} == {4, 10} and {p["DYG"] for s, p in fwd} == {3, 9}
    assert any(p["lds"] > 65536 for s, p in fwd)
    assert {(1, 1, 1, 1), (2, 3, 2, 3)} <= {s for s, p in fwd}
    # training's own forward plan at level 2 differs from these only in the channel count
    t = G.corr_plan(lib, (8, 32, 64, 208))
    assert any(all(p[k] == t[k] for k in ("TH", "TXQ", "ntx", "KS", "DYG", "PF2", "threads", "coarse", "vec")) for s, p in fwd)
    both, one = [], []
    for shape, family, want2, want1 in PC.CORR_BWD:
        p2, p1 = G.corr_plan(lib, shape, sides=2), G.corr_plan(lib, shape, sides=1)
        assert _has(p2, want2) and _has(p1, want1), (shape, p2, p1)
        both.append((shape, p2))
        one.append((shape, p1))
    every = both + one
    assert {p["IS"] for s, p in both} == {1, 3, 9} and {p["IS"] for s, p in one} >= {1, 9}
    assert {p["NCG"] for s, p in every} >= {1, 2, 3}
    assert any(p["NCG"] == 3 and p["lds"] > 65536 and s[1] % 8 for s, p in both) and any(p["NCG"] == 2 and s[1] % 8 and p["IS"] == 1 for s, p in every)
    assert {p["vec"] for s, p in both if p["NCG"] == 2 and p["lds"] > 65536 and s[1] % 8} == {0, 1}                # NCG 2 above 64 KB, on either kernel
    assert any(p["batches"] == 3 for s, p in one) and any(p["ncr"] * p["NCG"] > -(-s[1] // 8) for s, p in both)       # a last channel range that is not full
    assert any(p["threads"] & (p["threads"] - 1) for s, p in both)                           # a thread count that is no power of two
    assert any(p["ncr"] > 1 for s, p in both) and any(p["batches"] == 2 for s, p in both) and any(p["batches"] == 1 for s, p in both)
    assert {p["vec"] for s, p in both} == {0, 1} and any(p["NCG"] == 3 and p["vec"] == v for v in (0, 1) for s, p in both)
    assert any(p1 != p2 for (_, p1), (_, p2) in zip(one, both))                              # a one-sided launch picks another plan
    # the alignment shapes are the two fine plans; at W % 4 == 0 one pointer off flips the launcher's rule
    assert [s for s, _, w in PC.CORR_FWD if w.get("coarse") == 0][:2] == PC.ALIGN_SHAPES
    for k in range(3):
        assert not G.rule_corr_vec(208, [int(i == k) for i in range(3)]) and G.rule_corr_vec(208, [0, 0, 0], [81 * 64 * 208])
    assert not G.rule_corr_vec(206, [0, 0, 0]) and not G.rule_corr_vec(208, [0, 0], [2])
    assert set(PC.LEVEL_FWD_VEC_PTRS) < set(PC.LEVEL_FWD_PTRS) and set(PC.LEVEL_BWD_VEC_PTRS) < set(PC.LEVEL_BWD_PTRS)


def test_the_cases_reach_every_branch_of_the_warp_and_the_level():
    lib = _hip_lib()
    assert G.rule_warp_bwd_groups(40, 6, 11) == 16 and G.rule_warp_bwd_groups(32, 6, 11) == 4 and G.rule_warp_bwd_groups(40, 32, 64) == 4 and G.rule_warp_bwd_groups(40, 31, 66) == 16
    assert G.rule_wfg_eligible(8, 512) and not G.rule_wfg_eligible(7, 512) and not G.rule_wfg_eligible(8, 511)
    assert G.rule_map_small(1024) and not G.rule_map_small(1025) and not G.rule_map_small(512, True)
    warp = [s for s, _ in PC.WARP]
    assert {s[1] for s in warp} == {5, 8, 40, 136} and dict(PC.WARP)[(2, 40, 6, 11)] in ("rough", "smooth") and any(G.rule_warp_bwd_groups(*s[1:]) == 16 and s[1] > 16 * 8 for s in warp) and {k for _, k in PC.WARP} | {k for *_, k in PC.LEVEL} == set(G.FLOW_KINDS)
    assert any(s[2] * s[3] < 64 for s in warp) and any(s[2] * s[3] % 64 and s[2] * s[3] > 64 for s in warp) and any(s[2] * s[3] >= 2048 for s in warp)
    assert {G.rule_warp_bwd_groups(*s[1:]) for s in warp} == {4, 16} and G.rule_warp_bwd_groups(40, 32, 65) == 4
    assert {G.rule_wfg_eligible(s[1], s[2] * s[3]) for s in warp} == {True, False}
    level = [s for s, _, _ in PC.LEVEL]
    elig = {(s[1], s[2] * s[3]): G.rule_wfg_eligible(s[1], s[2] * s[3]) for s in level}
    assert elig[(7, 510)] is False and elig[(8, 510)] is False and elig[(7, 512)] is False and elig[(8, 512)] is True
    small = {s[2] * s[3]: G.rule_map_small(s[2] * s[3]) for s in level if s[1] >= 8}
    assert small[1024] is True and small[1056] is False and small[13312] is False
    assert all(G.rule_wfg_eligible(s[1], s[2] * s[3]) for s in PC.LEVEL_SCATTER_ENV) and all(G.rule_map_small(s[2] * s[3]) for s in PC.LEVEL_MAP_LARGE_ENV)
    assert set(PC.LEVEL_SCATTER_ENV) | set(PC.LEVEL_MAP_LARGE_ENV) <= set(level) and set(PC.ALIGN_SHAPES) <= set(level)
    assert {f for _, f, _ in PC.LEVEL} == set(G.FAMILIES)
    assert PC.PILE_TAPS == PC.PILE[2] * PC.PILE[3] > 65536 and G.rule_wfg_eligible(PC.PILE[1], PC.PILE_TAPS)
    # the gather lays header | counters | offsets | entries out inside the scatter's workspace: the same layout as the map's, so
    # dfe_pwc_level_map_bytes is its end.  It fits because C >= 8.
    for s in level + warp + [PC.PILE, (1, 8, 1, 512), (65535, 8, 16, 32), (3, 8, 511, 513)]:
        if G.rule_wfg_eligible(s[1], s[2] * s[3]):
            assert lib.dfe_pwc_level_map_bytes(s[0], s[2], s[3]) <= lib.dfe_scatter_ws_bytes(s[0] * s[1] * s[2] * s[3]), s
    assert lib.dfe_pwc_level_map_bytes(2, 16, 32) > lib.dfe_scatter_ws_bytes(2 * 4 * 16 * 32)          # ... and would not at C = 4


def test_pile_up_flow_puts_more_than_2_16_taps_on_four_targets():
    B, C, H, W = PC.PILE
    taps = G.warp_taps(G.make_flow("collapse", B, H, W, None), 0)
    _, _, cnt = G.warp_gx_ref(taps, torch.ones(B, 1, H, W), 0)
    assert sorted(cnt.flatten().tolist())[-5:] == [0.0] + [float(PC.PILE_TAPS)] * 4
    ys, xs = divmod(int(cnt.flatten().argmax()), W)
    assert 0 < ys < H - 2 and 0 < xs < W - 2                                                           # an interior point


@pytest.mark.parametrize("ac", [0, 1])
def test_warp_restatement_is_the_oracles_warp(ac):
    """the numpy-float32 taps against oracle.warp_flow at the operator tests' tolerance (values 2e-6, the same zeros under the
    mask); the float64 sums over them against the oracle's autograd in float64"""
    from oracle import loss_stack_oracle as O
    gen = torch.Generator().manual_seed(5 + ac)
    for (B, C, H, W), kind in [((2, 5, 7, 9), "rough"), ((1, 8, 5, 26), "smooth"), ((2, 3, 6, 11), "out"), ((1, 2, 12, 20), "collapse"), ((1, 2, 4, 5), "zero")]:
        x, flow = torch.rand(B, C, H, W, generator=gen), G.make_flow(kind, B, H, W, gen)
        gout = torch.randn(B, C, H, W, generator=gen)
        taps = G.warp_taps(flow, ac)
        for um in (0, 1):
            yo = O.warp_flow(x, flow, use_mask=bool(um), align_corners=bool(ac))
            mine = G.warp_fwd_ref(x, taps, um, torch.float32)
            assert float((mine - yo).abs().max()) <= 2e-6 and torch.equal(mine == 0, yo == 0), (kind, um)
            A = G.warp_fwd_ref(x, taps, um, torch.float64, absolute=True)
            assert bool((G.warp_fwd_ref(x, taps, um, torch.float64).abs() <= A * (1 + 1e-12)).all())
        xd, fd = x.double().requires_grad_(True), flow.double().requires_grad_(True)
        O.warp_flow(xd, fd, use_mask=False, align_corners=bool(ac)).backward(gout.double())
        gf = G.warp_gflow_ref(x, taps, gout, 0, ac, None, torch.float64)
        ref, mass, cnt = G.warp_gx_ref(taps, gout, 0)
        # float64 coordinates differ from the fp32 ones by ~1e-6 px: the gradients by that times the image's slope
        assert float((gf - fd.grad).abs().max()) <= 1e-4 * max(1.0, float(fd.grad.abs().max())), kind
        assert float((ref - xd.grad).abs().max()) <= 1e-4 * max(1.0, float(xd.grad.abs().max())), kind
        assert bool((mass >= ref.abs() * (1 - 1e-12)).all()) and float(cnt.max()) <= 4 * H * W


def test_cost_volume_references_are_the_oracles_corr_naive():
    from oracle import loss_stack_oracle as O
    gen = torch.Generator().manual_seed(9)
    for shape in [(2, 3, 2, 3), (1, 5, 6, 11), (1, 1, 1, 1)]:
        B, C, H, W = shape
        f1, f2 = G.make_input(shape, "randn", gen), G.make_input(shape, "randn", gen)
        gout = torch.randn(B, 81, H, W, generator=gen)
        a, b = f1.double().requires_grad_(True), f2.double().requires_grad_(True)
        out = O.corr_naive(a, b)
        out.backward(gout.double())
        A = G.corr_ref(f1, f2, torch.float64, absolute=True)
        assert _close64(G.corr_ref(f1, f2, torch.float64), out.detach(), A)
        g1, g2 = G.corr_bwd_ref(f1, f2, gout, torch.float64)
        A1, A2 = G.corr_bwd_ref(f1, f2, gout, torch.float64, absolute=True)
        assert _close64(g1, a.grad, A1) and _close64(g2, b.grad, A2)
        y1, y2 = G.corr_bwd_ref(f1, f2, gout, torch.float32)
        assert y1.dtype == torch.float32 and float((y1.double() - g1).abs().max()) < 1e-5 and float((y2.double() - g2).abs().max()) < 1e-5
        assert float((G.corr_ref(f1, f2, torch.float32).double() - out.detach()).abs().max()) < 1e-5


def test_the_level_bounds_notice_one_dropped_term():
    """one product missing from one cost-volume sum, one tap missing from one scattered element: both bounds refuse"""
    gen = torch.Generator().manual_seed(4)
    shape = (1, 13, 6, 10)
    f1, f2 = G.make_input(shape, "act", gen), G.make_input(shape, "act", gen)
    y32, r64, A = G.corr_ref(f1, f2, torch.float32), G.corr_ref(f1, f2, torch.float64), G.corr_ref(f1, f2, torch.float64, absolute=True)
    G.check_bound("yardstick against itself", y32, y32, r64, A)
    bad = y32.clone()
    bad[0, 40, 2, 3] -= f1[0, 12, 2, 3] * f2[0, 12, 2, 3] / 13          # displacement (0, 0), the last channel
    with pytest.raises(AssertionError):
        G.check_bound("a dropped product", bad, y32, r64, A)
    flow, gout = G.make_flow("rough", 1, 6, 10, gen), torch.randn(shape, generator=gen)
    taps = G.warp_taps(flow, 0)
    ref, mass, cnt = G.warp_gx_ref(taps, gout, 0)
    gmax = float(gout.abs().max())
    G.check_scatter_bound("float64 against itself", ref.float(), ref, mass, cnt, gmax)
    g5 = gout.reshape(1, 13, 60)[0, 5]
    p = int((torch.from_numpy(taps["inb"][0])[0] * torch.from_numpy(taps["w"][0])[0] * g5.abs()).argmax())    # the heaviest north-west tap
    q = int(taps["idx"][0][0, p])
    bad = ref.clone().reshape(1, 13, 60)
    bad[0, 5, q] -= float(g5[p]) * float(taps["w"][0][0, p])
    assert abs(float(g5[p])) * float(taps["w"][0][0, p]) > 0.1
    with pytest.raises(AssertionError):
        G.check_scatter_bound("a dropped tap", bad.reshape(shape).float(), ref, mass, cnt, gmax)


# ========================================================================================================= fused loss stack
def test_the_cases_reach_every_strip_boundary_and_path_of_the_loss_stack(monkeypatch):
    """dfe_geom_plan (host only) on the matrix of tests/loss_stack_cases.py: strips, row blocks, minimum sizes, pyramid paths,
    adjoint modes, the operand that sizes each of the two shared partial-sum regions, modes and depth terms"""
    for name in ("DFE_PYRAMIDS_GENERIC", "DFE_ADJ_MODE"):
        monkeypatch.delenv(name, raising=False)
    lib = _hip_lib()
    plans = [(c, LC.plan(lib, LC.bare_args(c))) for c in LC.CASES]
    assert all(p["fwd_rows"] == 8 and p["bwd_rows"] == 8 and p["S"] == c[3] and p["dt"] == (c[5] if c[4] != 2 else 0) for c, p in plans)
    assert all(c[1] * c[2] < 10 ** 5 for c in LC.CASES) and len(set(LC.CASES)) == len(LC.CASES)
    every = [(c, sc) for c, p in plans for sc in p["scales"]]
    for c, sc in every:      # the plan's figures are the layout's: strips cover the width, the last one is never empty
        assert sc["fwd_strips"] == -(-sc["W"] // 62) and sc["fwd_last"] == sc["W"] - 62 * (sc["fwd_strips"] - 1) and 1 <= sc["fwd_last"] <= 62
        assert sc["bwd_strips"] == -(-sc["W"] // 60) and sc["bwd_last"] == sc["W"] - 60 * (sc["bwd_strips"] - 1) and 1 <= sc["bwd_last"] <= 60
        assert sc["last_rows"] == sc["H"] - 8 * ((sc["H"] - 1) // 8) and 1 <= sc["last_rows"] <= 8
    # forward strips of 62, backward strips of 60: an exact multiple (more than one strip), a last strip of 1, of 2, a narrow scale
    for strips, last, cols in (("fwd_strips", "fwd_last", 62), ("bwd_strips", "bwd_last", 60)):
        assert any(sc[strips] > 1 and sc[last] == cols for _, sc in every), cols
        assert any(sc[strips] == 1 and sc[last] == cols for _, sc in every), cols
        assert any(sc[strips] > 1 and sc[last] == 1 for _, sc in every), cols
        assert any(sc[strips] > 1 and sc[last] == 2 for _, sc in every), cols
        assert any(sc[strips] == 1 and sc[last] < cols for _, sc in every), cols
    # rows: last blocks of 1, 2, 3 and 8; 1 and 2 where the flow-smoothness backward runs (modes 0 and 2), which walks 3 rows a step
    assert {sc["last_rows"] for _, sc in every} >= {1, 2, 3, 8}
    assert {sc["last_rows"] for c, sc in every if c[4] != 1} >= {1, 2, 3, 8}
    assert any(sc["H"] == 3 for _, sc in every) and any(sc["W"] == 3 for _, sc in every)
    assert any(sc["H"] * sc["W"] < 256 for _, sc in every) and any(sc["H"] * sc["W"] % 256 and sc["H"] * sc["W"] > 256 for _, sc in every)
    # pyramids
    assert any(p["two_level"] == 1 and p["generic_jobs"] == 3 * (c[3] - 3) for c, p in plans)
    assert any(p["two_level"] == 0 and c[3] >= 3 and c[4] != 2 and c[2] % 4 for c, p in plans)                    # W % 4 != 0
    assert any(p["two_level"] == 0 and c[3] < 3 and c[4] != 2 for c, p in plans)                                  # S < 3
    assert any(p["coarse_jobs"] >= 1 and c[3] >= 5 for c, p in plans)
    for c, p in plans:
        assert p["two_level"] == int(c[3] >= 3 and c[4] != 2 and c[1] % 4 == 0 and c[2] % 4 == 0), c
        if p["two_level"]:       # one frame pointer off 16 bytes, in turn: the per-level kernel takes every level
            for f in range(3):
                q = LC.plan(lib, LC.bare_args(c, tuple(4096 + (4 if k == f else 0) for k in range(3))))
                assert q["two_level"] == 0 and q["generic_jobs"] == 3 * (c[3] - 1) and q["total"] == p["total"], (c, f)
            assert LC.plan(lib, LC.bare_args(c, (4096, 8192, 4112)))["two_level"] == 1
    # adjoint of the up-sampling
    assert any(p["adj_mode"] == 1 and p["adj_s0"] == p["S"] and p["S"] > 1 for _, p in plans)                    # mixed, no coarse level
    assert any(p["adj_mode"] == 1 and p["adj_s0"] < p["S"] for _, p in plans)                                    # mixed with one
    assert dict((c[:4], p["adj_s0"]) for c, p in plans)[(2, 24, 124, 4)] == 3
    assert any(p["adj_mode"] == 0 and p["adj_s0"] == 1 and p["adj_nseg"] > 1 and p["S"] > 1 for _, p in plans)    # separable
    # the two regions sized by a maximum: each operand the larger one at least once (modes that run the kernels behind them)
    assert any(p["nblk_total"] > p["fs_units"] for c, p in plans if c[4] != 1) and any(p["nblk_total"] < p["fs_units"] for c, p in plans if c[4] != 1)
    assert any(p["dsm_units"] > p["nblk0"] for c, p in plans if c[4] != 2) and any(p["dsm_units"] < p["nblk0"] for c, p in plans if c[4] != 2)
    assert any(p["nblk_total"] == p["fs_units"] and p["dsm_units"] == p["nblk0"] and c[4] == 0 for c, p in plans)  # ... and neither: no slack
    # modes and depth terms
    assert {c[5] for c in LC.CASES if c[4] == 0} == {0, 1, 2, 3} and {c[5] for c in LC.CASES if c[4] == 1} == {0, 3} and {c[4] for c in LC.CASES} == {0, 1, 2}
    assert any(c[0] == 3 for c in LC.CASES)
    for c, p in plans:
        assert p["total"] == lib.dfe_geom_workspace_floats(ctypes.byref(LC.bare_args(c))), c
    # the environment is honoured as the launchers honour it
    two = next(c for c, p in plans if p["two_level"])
    monkeypatch.setenv("DFE_PYRAMIDS_GENERIC", "1")
    assert LC.plan(lib, LC.bare_args(two))["two_level"] == 0
    monkeypatch.delenv("DFE_PYRAMIDS_GENERIC")
    monkeypatch.setenv("DFE_ADJ_MODE", "separable")
    assert LC.plan(lib, LC.bare_args(two))["adj_mode"] == 0 and LC.plan(lib, LC.bare_args(two))["total"] != dict(plans)[two]["total"]
    monkeypatch.delenv("DFE_ADJ_MODE")
    # errors: as dfe_geom_workspace_floats
    bad = LC.bare_args((1, 8, 24, 3, 0, 0))
    buf = (ctypes.c_int * LC.PLAN_INTS)()
    assert lib.dfe_geom_plan(ctypes.byref(bad), buf) == -2 and lib.dfe_geom_plan(ctypes.byref(bad), None) == -1 and lib.dfe_geom_plan(None, buf) == -1


@pytest.mark.parametrize("shape", sorted(LC.SEEDS))
def test_the_loss_stack_cases_are_margin_checked_and_no_mask_is_constant(shape):
    """what ``strict`` in test_hip_loss_stack.py rests on (as test_api_cpu.py does for STRICT): on the oracle alone, no pixel of
    any scale inside a mask family's noise floor, for both align_corners settings; and each of the eight masks strictly between
    2 % and 98 % set at scale 0"""
    import numpy as np
    from oracle import loss_stack_oracle as O
    from tests import _margins as M
    from tests.golden import make_golden as MG
    B, H, W, S = shape
    assert shape in {c[:4] for c in LC.CASES}
    inp = LC.inputs(shape + (0, 0))
    ang = inp.pose[..., 3:].astype(np.float64)
    for fn in (np.cos, np.sin):      # conditioned poses: the exact value within 0.3 ulp of its nearest float32
        v = fn(ang)
        r = v.astype(np.float32)
        assert (np.abs(v - r.astype(np.float64)) / np.spacing(np.abs(r)).astype(np.float64) < 0.3).all()
    for ac in (False, True):
        within = M.within_counts(M.geom_margins(inp, ac, S))
        assert sum(within.values()) == 0, (shape, ac, within)
        disps, pose, fb, ff = MG.lists_to_t(inp, False)
        _, masks = O.GeomLossOracle(num_scales=S, align_corners=ac).geom_losses(*[MG.T(a) for a in inp.imgs], disps[0], disps[1], disps[2], pose, fb, ff,
                                                                               MG.T(inp.K), MG.T(inp.K_inv))
        for k in ("valid_bwd", "valid_fwd", "occ_bwd", "occ_fwd", "dyna_bwd", "dyna_fwd", "texture_bwd", "texture_fwd"):
            frac = float(masks[k][0].mean())
            assert 0.02 < frac < 0.98, (shape, ac, k, frac)


# ========================================================================================================= geometry, resize, splat, 1x1
# Self-tests of tests/guarded_geom.py and tests/geom_cases.py: every float64 reference agrees with float64 ATen / autograd where ATen
# has the operation, the splat conserves mass, the matrices reach every plane-size class, and no committed inverse_warp2 gradient
# case has an unsafe pixel left.
from tests import geom_cases as GEO         # noqa: E402
from tests import guarded_geom as GG        # noqa: E402

F64 = torch.float64


def _close(a, b, tol=1e-12):
    a, b = a.detach(), b.detach()
    return float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


def test_geom_pose_reference_is_the_oracles_function_in_float64():
    from oracle import loss_stack_oracle as O
    gen = torch.Generator().manual_seed(3)
    vec = (0.3 * torch.randn(9, 6, generator=gen)).double()
    gT, gE = torch.randn(9, 3, 4, generator=gen).double(), torch.randn(9, 3, 3, generator=gen).double()
    T34, E = GG.pose_mats_ref(vec)
    assert _close(T34, O.pose_vec2mat(vec)) and _close(E, O.compute_essential_matrix(vec))
    v = vec.clone().requires_grad_(True)
    want = torch.autograd.grad((O.pose_vec2mat(v) * gT).sum() + (O.compute_essential_matrix(v) * gE).sum(), v)[0]
    assert _close(GG.pose_mats_vjp_ref(vec, gT, gE), want)
    assert _close(GG.pose_mats_vjp_ref(vec, gT, None) + GG.pose_mats_vjp_ref(vec, None, gE), want)
    assert GG.chain_err(want.float(), want) <= 1.0 and GG.chain_err(want * (1 + 8 * G.U24), want) > 4.0


@pytest.mark.parametrize("ac", [False, True])
def test_geom_sampling_reference_is_grid_sample_in_float64(ac):
    """the zero-padded bilinear sample, values and both gradients, and the whole inverse_warp2 / rigid-flow chain against the
    oracle's graph run in float64"""
    from oracle import loss_stack_oracle as O
    B, H, W = 2, 9, 31
    c, unsafe, _ = GG.safe_warp_inputs(B, H, W, 5, "oob", ac)
    assert unsafe == 0
    img, d, rd, p, K = (c[k].double() for k in ("img", "depth", "ref_depth", "pose", "K"))
    gen = torch.Generator().manual_seed(1)
    ix, iy = (torch.rand(B, 40, generator=gen).double() * (W + 3) - 2).requires_grad_(True), (torch.rand(B, 40, generator=gen).double() * (H + 3) - 2).requires_grad_(True)
    im = img.clone().requires_grad_(True)
    got = GG.bilinear_zero_ref(im, ix, iy)
    un = (lambda t, n: 2 * t / (n - 1) - 1) if ac else (lambda t, n: (2 * t + 1) / n - 1)
    want = F.grid_sample(im, torch.stack([un(ix, W), un(iy, H)], 2)[:, None], mode="bilinear", padding_mode="zeros", align_corners=ac)[:, :, 0]
    assert _close(got, want)
    cot = torch.randn(got.shape, generator=gen).double()
    for a, b in zip(torch.autograd.grad(got, [im, ix, iy], cot, retain_graph=True), torch.autograd.grad(want, [im, ix, iy], cot)):
        assert _close(a, b, 1e-10)
    d1, r1, p1 = (t.clone().requires_grad_(True) for t in (d, rd, p))
    d2, r2, p2 = (t.clone().requires_grad_(True) for t in (d, rd, p))
    mine = GG.inverse_warp2_ref(img, d1, r1, p1, K, ac)
    theirs = O.inverse_warp2(img, d2, r2, p2, K, align_corners=ac)        # float64 through the oracle's graph: its K^-1 is fp32-made
    loss = lambda o: (o[0] * c["wi"].double()).sum() + (o[2] * c["wp"].double()).sum() + (o[3] * c["wc"].double()).sum()
    for a, b in zip((mine["img"], mine["valid"], mine["pdepth"], mine["cdepth"]), theirs):
        assert _close(a, b, 1e-5)
    for a, b in zip(torch.autograd.grad(loss((mine["img"], None, mine["pdepth"], mine["cdepth"])), [d1, r1, p1]), torch.autograd.grad(loss(theirs), [d2, r2, p2])):
        assert _close(a, b, 1e-4)
    assert _close(GG.rigid_flow_ref(d, p, K)[0], O.calculate_rigid_flow(d, p, K), 1e-5)


def test_geom_ssim_resize_and_area_references_are_atens_in_float64():
    from oracle import loss_stack_oracle as O
    gen = torch.Generator().manual_seed(2)
    x, y = torch.rand(2, 3, 9, 33, generator=gen).double(), torch.rand(2, 3, 9, 33, generator=gen).double()
    assert _close(GG.ssim_ref(x, y), O.SSIM(x, y), 1e-10)
    pre, gate = GG.ssim_loss_gate(torch.tensor([1.5, 1.0, 0.0, -1.0, -1.5], dtype=F64))
    assert gate.tolist() == [0.0, 0.0, 1.0, 0.0, 0.0] and pre.tolist() == [-0.25, 0.0, 0.5, 1.0, 1.25]
    for (h, w), (H, W) in GEO.RB_CASES + [GEO.RB_REFUSED] + GEO.R0_CASES:
        v = torch.randn(2, h, w, generator=gen).double().requires_grad_(True)
        g = torch.randn(2, H, W, generator=gen).double()
        want = F.interpolate(v[None], (H, W), mode="bilinear", align_corners=False)[0]
        assert _close(GG.resize_bilinear_ref(v.detach(), (H, W), 3.0), want * 3.0)
        assert _close(GG.resize_adjoint_ref(g, (h, w), 3.0), torch.autograd.grad(want, v, g)[0] * 3.0)
        assert bool((GG.resize_adjoint_ref(g, (h, w), -3.0, absolute=True) >= GG.resize_adjoint_ref(g, (h, w), 3.0).abs() - 1e-12).all())
    for (h, w), (H, W) in GEO.R1_CASES:
        v = torch.randn(2, h, w, generator=gen).double()
        assert _close(GG.area_ref(v, (H, W)), F.interpolate(v[None], (H, W), mode="area")[0])
        assert _close(GG.area_ref(v, (H, W), absolute=True), F.adaptive_avg_pool2d(v.abs()[None], (H, W))[0])


def test_geom_conv1x1_references_are_atens_in_float64_and_the_serial_sum_is_serial():
    gen = torch.Generator().manual_seed(4)
    for shape in [(3, 24, 12, 2, 7), (2, 5, 7, 16, 16), (1, 1, 1, 1, 1)]:
        B, Ci, Co, H, W = shape
        x, w, bias, gy, _ = GG.conv1x1_inputs(shape, True, 11)
        assert G.margin_ok(GG.conv1x1_ref(x, w, bias), GG.conv1x1_ref(x, w, bias, absolute=True))
        xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
        want = F.conv2d(xd, wd[:, :, None, None], bias.double())
        assert _close(GG.conv1x1_ref(x, w, bias), want)
        gx, gw = torch.autograd.grad(want, [xd, wd], gy.double())
        assert _close(GG.conv1x1_gx_ref(gy, w), gx) and _close(GG.conv1x1_gw_ref(gy, x), gw)
        for f32, f64, A in ((GG.conv1x1_ref(x, w, bias, torch.float32), GG.conv1x1_ref(x, w, bias), GG.conv1x1_ref(x, w, bias, absolute=True)),
                            (GG.conv1x1_gx_ref(gy, w, torch.float32), GG.conv1x1_gx_ref(gy, w), GG.conv1x1_gx_ref(gy, w, absolute=True)),
                            (GG.conv1x1_gw_ref(gy, x, torch.float32), GG.conv1x1_gw_ref(gy, x), GG.conv1x1_gw_ref(gy, x, absolute=True))):
            assert f32.dtype == torch.float32 and f32.shape == f64.shape == A.shape
            e, zero_ok = G.norm_err(f32, f64, A)
            assert zero_ok and e <= max(Ci, Co, B * H * W) + 1       # a serial sum of n terms: at most n roundings of at most A each


def test_geom_triplet_reference_is_the_half_pixel_resize_with_edge_replication():
    gen = torch.Generator().manual_seed(6)
    for (H0, W0), (H, W) in GEO.TRIPLET_CASES:
        u8 = torch.randint(0, 256, (2, 3 * H0, W0, 3), generator=gen, dtype=torch.uint8)
        got = GG.triplets_ref(u8, [1, 0], H, W)
        assert got.shape == (2, 3, 3 * H, W) and got.dtype == F64 and 0.0 <= float(got.min()) and float(got.max()) <= 1.0
        fr = u8.double().reshape(2, 3, H0, W0, 3).permute(0, 1, 4, 2, 3).reshape(6, 3, H0, W0)        # [b*frame, c, H0, W0]
        if (H, W) == (H0, W0):
            want = fr / 255.0
        elif H <= H0 and W <= W0 or H >= H0 and W >= W0:
            # F.interpolate(align_corners=False) is the same geometry: half-pixel centres, source index clamped at the borders
            want = F.interpolate(fr, (H, W), mode="bilinear", align_corners=False) / 255.0
        want = want.reshape(2, 3, 3, H, W).permute(0, 2, 1, 3, 4).reshape(2, 3, 3 * H, W)
        assert _close(got[1], want[1], 1e-12) and _close(got[0], want[0].flip(-1), 1e-12)
        assert _close(GG.triplets_ref(u8, None, H, W)[0], want[0], 1e-12)
        y32 = GG.triplets_ref(u8, [1, 0], H, W, GG.np.float32)
        # the fp32 source coordinate carries ~4 roundings at its own magnitude (up to 300 here); a value moves by at most that
        # per axis (neighbouring bytes / 255 differ by at most 1)
        assert y32.dtype == torch.float32 and float((y32.double() - got).abs().max()) <= 8 * G.U24 * max(H0, W0)


@pytest.mark.parametrize("kind", GEO.SPLAT_KINDS)
def test_geom_splat_reference_conserves_mass_and_counts_its_taps(kind):
    B, H, W = 3, 9, 31
    flow = GG.splat_flow(kind, B, H, W, torch.Generator().manual_seed(8))
    ref, mass, cnt = GG.splat_ref(flow)
    assert ref.shape == (B, 1, H, W) and torch.equal(ref, mass) and bool((ref >= 0).all())
    t = GG.splat_taps(flow)
    xs, ys = torch.arange(W).float()[None, None, :], torch.arange(H).float()[None, :, None]
    tx, ty = (xs + flow[:, 0]).reshape(B, -1), (ys + flow[:, 1]).reshape(B, -1)
    inside = (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)          # all four taps land (or carry a zero weight)
    per_src = sum(torch.from_numpy(t["w"][k]).double() * torch.from_numpy(t["inb"][k]).double() for k in range(4))
    assert bool(((per_src - 1.0).abs()[inside] <= 4 * G.U24).all()) and bool((per_src <= 1.0 + 4 * G.U24).all())
    assert abs(float(ref.sum()) - float(per_src.sum())) <= 1e-9 * max(1.0, float(per_src.sum()))
    assert float(cnt.sum()) == float(sum(((torch.from_numpy(t["w"][k]) != 0) & torch.from_numpy(t["inb"][k])).sum() for k in range(4)))
    if kind == "zero":
        assert torch.equal(ref, torch.ones_like(ref)) and torch.equal(cnt, torch.ones_like(cnt))
    if kind == "edge":         # half-inside taps: sources that deposit less than 1 but more than 0
        assert bool(((per_src > 0) & (per_src < 1 - 1e-3)).any())
    if kind == "nan":
        assert int((~torch.from_numpy(t["live"])).sum()) >= 1 and bool(torch.isfinite(ref).all())
    if kind == "out":
        assert float(ref[0].sum()) < 0.25 * float(ref[1].sum()) and float(ref.sum()) < 0.2 * B * H * W      # most of the mass leaves the image


def test_geom_case_matrices_reach_every_plane_size_class():
    shapes = GEO.PIXEL_SHAPES + [GEO.TINY_SHAPE]
    assert {GEO.plane_class(h, w) for _, h, w in shapes} == GEO.PLANE_CLASSES
    assert {GEO.plane_class(h, w) for _, h, w in GEO.PIXEL_SHAPES} == GEO.PLANE_CLASSES - {"pixel"}
    assert {c[:3] for c in GEO.warp_grad_cases()} == set(GEO.PIXEL_SHAPES) and {c[3] for c in GEO.warp_grad_cases()} == {"rand", "oob"}
    assert {c[3] for c in GEO.warp_fwd_cases()} == {"rand", "oob", "identity", "clamp"}
    assert {c[:3] for c in GEO.flow_cases()} >= set(shapes)
    assert any(-(-h * w // 256) == 2 and h * w % 256 == 23 for _, h, w in GEO.PIXEL_SHAPES)       # two partial rows per sample, 23 live threads
    assert any(w % 4 for _, h, w in GEO.PIXEL_SHAPES if h * w > 1024)
    # SSIM tiles of 32 x 8: inside one tile, exactly one, one row and one column past it, three tiles across
    assert {(-(-w // 32), -(-h // 8)) for _, _, h, w in GEO.SSIM_SHAPES} == {(1, 1), (2, 2), (3, 1)} and (2, 3, 8, 32) in GEO.SSIM_SHAPES
    # the adjoint's register path: ratio 4 is its limit, one refused case beyond it, one down-sampling case
    lim = lambda i, o: 2 * o[0] <= 8 * i[0] and 2 * o[1] <= 8 * i[1]
    assert all(lim(i, o) for i, o in GEO.RB_CASES) and not lim(*GEO.RB_REFUSED)
    assert any(2 * o[0] == 8 * i[0] and 2 * o[1] == 8 * i[1] for i, o in GEO.RB_CASES) and any(o[0] < i[0] for i, o in GEO.RB_CASES)
    assert {o[0] + o[1] <= 128 for _, o in GEO.R0_CASES} == {True, False} and any(o[0] + o[1] == 128 for _, o in GEO.R0_CASES) and any(o[0] + o[1] == 129 for _, o in GEO.R0_CASES)
    assert any(i[0] % o[0] and i[1] % o[1] for i, o in GEO.R1_CASES) and any(i[0] == 2 * o[0] and i[1] == 2 * o[1] for i, o in GEO.R1_CASES)
    # 1x1: both limits met exactly, both refusals one past them
    assert any(h * w == 256 for _, _, _, h, w in GEO.C1_SHAPES) and any(b * h * w == 4096 for b, _, _, h, w in GEO.C1_SHAPES)
    assert {(h * w, b * h * w > 4096) for b, _, _, h, w in GEO.C1_REFUSED} == {(257, False), (241, True)} and any(b * h * w == 4097 for b, _, _, h, w in GEO.C1_REFUSED)
    assert max(b * d * s for b, d, s in GEO.CAMERA_CASES) > 64 and max(GEO.POSE_N) > 64


_GEO_GRAD = GEO.warp_grad_cases()


@pytest.mark.parametrize("case", _GEO_GRAD, ids=["%dx%dx%d-%s" % c[:4] for c in _GEO_GRAD])
def test_geom_margin_builder_leaves_no_unsafe_pixel(case):
    """the four conditions of tests/guarded_geom.py's warp_unsafe after the depth nudges, for both align_corners settings: the cap
    is zero -- a condition of the case, not a tolerance; and the nudged inputs still exercise what the case is for"""
    B, H, W, kind, seed = case
    for ac in (False, True):
        c, unsafe, before = GG.safe_warp_inputs(B, H, W, seed, kind, ac)
        assert unsafe == 0, (case, ac, before)
        assert not bool(GG.warp_unsafe(c["depth"], c["ref_depth"], c["pose"], c["K"], ac).any())
        r = GG.inverse_warp2_ref(*(c[k].double() for k in ("img", "depth", "ref_depth", "pose", "K")), ac)
        if H * W >= 35:
            assert 0.0 < float(r["valid"].mean()) and (kind != "oob" or float(r["valid"].mean()) < 1.0), (case, ac)
    for c4 in GEO.flow_cases():
        if c4[:3] == (B, H, W):
            assert GG.safe_flow_inputs(*c4[:3], c4[4], c4[3])[1] == 0, c4
    d = GG.mask_inputs(B, H, W, B + H + W)
    assert all(G.margin_ok(v, a) for v, a in d["margins"])
    if H * W >= 35:
        assert all(0.0 < float(d[k].mean()) < 1.0 for k in ("occ_bwd", "occ_fwd", "texture", "dyna"))
