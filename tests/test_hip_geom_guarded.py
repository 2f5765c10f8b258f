"""GPU: the geometry kernels of csrc/ops_basic.hip (cameras, pose matrices, inverse_warp2, rigid flow, SSIM), the mask decisions
(ops_masks.hip) and the forward splat (ops_splat.hip) through the C ABI in guarded, poisoned buffers (tests/guarded.py), at the
plane sizes of tests/geom_cases.py -- a plane that ends inside a block, a second block feeding the pose sums -- with every
pointer rotated through the four dword offsets (the scatter workspaces stay on 16 bytes, as the header demands).

Every call: return code 0, all guard bands intact, every output written, inputs unchanged, scratch of exactly the size the
library's query states, every offset variant bit-equal to the first.  The forwards that restate the reference's fp32 arithmetic
(inverse_warp2's four outputs, the rigid flow, the pose and essential matrices, the masks and the score) equal the fp32 oracle on
the host bit for bit, the masks also the float64 decision.  Chain-rule gradients keep e = max |out - ref64| / (2^-24 max |ref64|)
per sample within 4 max(1, e of fp32 autograd through the oracle on the host) (guarded_geom.check_chain); the two scatters keep
guarded.check_scatter_bound and are bitwise equal on a second run.  No case has a decision within MARGIN of its threshold:
asserted on the float64 reference before anything is launched (tests/guarded_geom.py)."""
import ctypes

import pytest
import torch

from oracle import loss_stack_oracle as O
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


def _ws(n):
    """a scatter workspace of exactly dfe_scatter_ws_bytes(n) bytes on a 16-byte boundary, NaN on entry"""
    lib, _ = _lib()
    nbytes = int(lib.dfe_scatter_ws_bytes(ctypes.c_long(n)))
    assert nbytes == 64 + 8 * n
    return G.Carved((nbytes // 4,), 0)


def _check(tag, bufs, outs, ins=()):
    """bufs: every carve of the call; outs: those that must be written; ins: (carve, the values it was filled with)"""
    torch.cuda.synchronize()
    for i, c in enumerate(bufs):
        assert c is None or c.intact(), (tag, "guard band of buffer %d overwritten" % i)
    for i, c in enumerate(outs):
        assert c.written(), (tag, "output %d has unwritten or non-finite elements" % i)
    for i, (c, t) in enumerate(ins):
        assert G.bits_equal(c.cpu(), t.reshape(c.view.shape)), (tag, "input %d changed" % i)


def _same(tag, first, got):
    """every offset variant returns the bits of the first"""
    for k, (a, b) in enumerate(zip(first, got)):
        assert G.bits_equal(a, b), (tag, "output %d depends on the alignment" % k)


def _cameras(lib, st, pose, K, off, tag):
    """dfe_prepare_cameras(pose [B,6], K, cams, B, 1, 1, {1}) in carved buffers: the carve of the B camera blocks"""
    B, ncf = pose.shape[0], int(lib.dfe_camera_floats())
    pc, kc, cams = _carve(pose, off), _carve(K.reshape(B, 9), (off + 1) % 4), G.Carved((B, ncf), (off + 2) % 4)
    ds = (ctypes.c_float * 1)(1.0)
    assert lib.dfe_prepare_cameras(_p(pc), _p(kc), _p(cams), B, 1, 1, ctypes.cast(ds, ctypes.c_void_p), st) == 0, tag
    _check(tag + " cameras", [pc, kc, cams], [cams], [(pc, pose), (kc, K)])
    return cams


# ========================================================================================================= cameras
@pytest.mark.parametrize("case", GC.CAMERA_CASES)
def test_prepare_cameras_stays_inside_its_blocks(case):
    """the cameras' content is checked through the inverse_warp2 and rigid-flow results they feed (below)"""
    lib, st = _lib()
    B, ndir, nscale = case
    ncf = int(lib.dfe_camera_floats())
    c = GG.warp_inputs(B * ndir, 8, 26, sum(case), "rand")
    ds = (ctypes.c_float * nscale)(*[float(2 ** s) for s in range(nscale)])
    first = None
    for off in GC.OFFS:
        tag = "prepare_cameras %s off %d" % (case, off)
        pc, kc, cams = _carve(c["pose"], off), _carve(c["K"][:B].reshape(B, 9), (off + 1) % 4), G.Carved((B * ndir * nscale, ncf), (off + 3) % 4)
        assert lib.dfe_prepare_cameras(_p(pc), _p(kc), _p(cams), B, ndir, nscale, ctypes.cast(ds, ctypes.c_void_p), st) == 0, tag
        _check(tag, [pc, kc, cams], [cams], [(pc, c["pose"]), (kc, c["K"][:B])])
        first = first or [cams.cpu()]
        _same(tag, first, [cams.cpu()])


# ========================================================================================================= pose matrices
@pytest.mark.parametrize("n", GC.POSE_N)
def test_pose_vec2mat_forward_and_backward(n):
    from unsupervised_depth_opticalflow_egomotion_amd import synthetic
    lib, st = _lib()
    gen = torch.Generator().manual_seed(n)
    vec = torch.from_numpy(synthetic.robust_pose((0.3 * torch.randn(n, 6, generator=gen)).numpy()))
    gT, gE = torch.randn(n, 3, 4, generator=gen), torch.randn(n, 3, 3, generator=gen)
    with O.trig("cr"):
        T_o, E_o = O.pose_vec2mat(vec), O.compute_essential_matrix(vec)
    T64, E64 = GG.pose_mats_ref(vec.double())
    assert float((T64 - T_o.double()).abs().max()) < 1e-6 and float((E64 - E_o.double()).abs().max()) < 1e-6
    for mode in ("both", "T34", "E"):
        for off in GC.OFFS:
            tag = "pose_vec2mat_fwd n %d %s off %d" % (n, mode, off)
            vc = _carve(vec, off)
            tc = G.Carved((n, 3, 4), (off + 1) % 4) if mode != "E" else None
            ec = G.Carved((n, 3, 3), (off + 2) % 4) if mode != "T34" else None
            assert lib.dfe_pose_vec2mat_fwd(_p(vc), _p(tc), _p(ec), n, st) == 0, tag
            _check(tag, [vc, tc, ec], [c for c in (tc, ec) if c], [(vc, vec)])
            assert tc is None or G.bits_equal(tc.cpu(), T_o), (tag, "T34 is not the oracle's")
            assert ec is None or G.bits_equal(ec.cpu(), E_o), (tag, "E is not the oracle's")
    for mode in ("both", "T34", "E"):
        a, b = (gT if mode != "E" else None), (gE if mode != "T34" else None)
        ref64 = GG.pose_mats_vjp_ref(vec, a, b)
        v32 = vec.clone().requires_grad_(True)
        with O.trig("cr"):
            loss = (0.0 if a is None else (O.pose_vec2mat(v32) * a).sum()) + (0.0 if b is None else (O.compute_essential_matrix(v32) * b).sum())
        yard = torch.autograd.grad(loss, v32)[0]
        first = None
        for off in GC.OFFS:
            tag = "pose_vec2mat_bwd n %d %s off %d" % (n, mode, off)
            vc, gv = _carve(vec, off), G.Carved((n, 6), (off + 3) % 4)
            ac, bc = (None if a is None else _carve(a, (off + 1) % 4)), (None if b is None else _carve(b, (off + 2) % 4))
            assert lib.dfe_pose_vec2mat_bwd(_p(vc), _p(ac), _p(bc), _p(gv), n, st) == 0, tag
            _check(tag, [vc, ac, bc, gv], [gv], [(vc, vec)] + ([(ac, a)] if ac else []) + ([(bc, b)] if bc else []))
            if first is None:
                first = [gv.cpu()]
                GG.check_chain("pose_vec2mat_bwd n %d %s gvec" % (n, mode), first[0], yard, ref64)
            _same(tag, first, [gv.cpu()])


# ========================================================================================================= inverse_warp2
def _warp_grads(fn, c, ac, dtype, with_depths):
    """(g_depth, g_pose, g_refdepth or None) of sum(img wi) [+ sum(pdepth wp) + sum(cdepth wc)] by autograd in ``dtype``"""
    t = lambda k: c[k].to(dtype)
    d, rd, p = (t(k).clone().requires_grad_(True) for k in ("depth", "ref_depth", "pose"))
    out = fn(t("img"), d, rd, p, t("K"), ac)
    loss = (out[0] * t("wi")).sum()
    if with_depths:
        loss = loss + (out[2] * t("wp")).sum() + (out[3] * t("wc")).sum()
    g = torch.autograd.grad(loss, [d, p] + ([rd] if with_depths else []))
    return g[0], g[1], (g[2] if with_depths else None)


def _oracle_warp(img, d, rd, p, K, ac):
    with O.trig("cr"):
        return O.inverse_warp2(img, d, rd, p, K, align_corners=ac)


def _ref_warp(img, d, rd, p, K, ac):
    r = GG.inverse_warp2_ref(img, d, rd, p, K, ac)
    return r["img"], r["valid"], r["pdepth"], r["cdepth"]


def _run_warp(lib, st, c, ac, off, tag, backward):
    """forward and the three backward runs at one offset rotation.  (forward outputs, {run: (g_depth, g_pose, g_refdepth)})"""
    B, _, H, W = c["depth"].shape
    npart = int(lib.dfe_pose_partials_floats(B, H, W))
    assert npart == B * -(-H * W // 256) * 12
    cams = _cameras(lib, st, c["pose"], c["K"], off, tag)
    o = lambda k: (off + k) % 4
    ic, dc, rc = _carve(c["img"], o(0)), _carve(c["depth"], o(1)), _carve(c["ref_depth"], o(2))
    oi, ov, op, oc = G.Carved((B, 3, H, W), o(3)), G.Carved((B, 1, H, W), o(0)), G.Carved((B, 1, H, W), o(1)), G.Carved((B, 1, H, W), o(2))
    ins = [(ic, c["img"]), (dc, c["depth"]), (rc, c["ref_depth"])]
    assert lib.dfe_inverse_warp2_fwd(_p(ic), _p(dc), _p(rc), _p(cams), _p(oi), _p(ov), _p(op), _p(oc), B, H, W, int(ac), st) == 0, tag
    _check(tag + " fwd", [ic, dc, rc, cams, oi, ov, op, oc], [oi, ov, op, oc], ins)
    fwd = [t.cpu() for t in (oi, ov, op, oc)]
    o2 = G.Carved((B, 3, H, W), o(1))                                     # the three optional outputs NULL
    assert lib.dfe_inverse_warp2_fwd(_p(ic), _p(dc), None, _p(cams), _p(o2), None, None, None, B, H, W, int(ac), st) == 0, tag
    _check(tag + " fwd image only", [ic, dc, cams, o2], [o2], ins[:2])
    assert G.bits_equal(o2.cpu(), fwd[0]), tag
    grads = {}
    for run in (("img", "all", "all-noref") if backward else ()):
        gi = _carve(c["wi"], o(2))
        gp, gc = (None, None) if run == "img" else (_carve(c["wp"], o(3)), _carve(c["wc"], o(0)))
        gd, gpose, part = G.Carved((B, 1, H, W), o(1)), G.Carved((B, 6), o(2)), G.Carved((npart,), o(3))
        gr, ws = (G.Carved((B, 1, H, W), o(3)), _ws(B * H * W)) if run == "all" else (None, None)
        assert lib.dfe_inverse_warp2_bwd(_p(ic), _p(dc), _p(rc), _p(cams), _p(gi), _p(gp), _p(gc), _p(gd), _p(gr), _p(ws), _p(gpose), _p(part), B, H, W,
                                         int(ac), st) == 0, (tag, run)
        _check("%s bwd %s" % (tag, run), [ic, dc, rc, cams, gi, gp, gc, gd, gr, ws, gpose, part], [gd, gpose, part] + ([gr] if gr else []),
               ins + [(gi, c["wi"])] + ([(gp, c["wp"]), (gc, c["wc"])] if gp else []))
        grads[run] = [gd.cpu(), gpose.cpu()] + ([gr.cpu()] if gr else [])
        if gr:                                                                # the scatter is bitwise reproducible
            gr2, ws2 = G.Carved((B, 1, H, W), o(0)), _ws(B * H * W)
            assert lib.dfe_inverse_warp2_bwd(_p(ic), _p(dc), _p(rc), _p(cams), _p(gi), _p(gp), _p(gc), _p(gd), _p(gr2), _p(ws2), _p(gpose), _p(part), B, H, W,
                                             int(ac), st) == 0, (tag, run)
            _check("%s bwd %s again" % (tag, run), [gr2, ws2, gd, gpose, part], [gr2])
            assert G.bits_equal(gr2.cpu(), grads[run][2]), (tag, "g_refdepth differs on a second run")
    return fwd, grads


_WARP_GRAD = GC.warp_grad_cases()


@pytest.mark.parametrize("case", _WARP_GRAD, ids=["%dx%dx%d-%s" % c[:4] for c in _WARP_GRAD])
@pytest.mark.parametrize("ac", [False, True])
def test_inverse_warp2_forward_and_gradients(case, ac):
    """forward bit-equal to the oracle; g_depth and g_pose of the three backward runs (image cotangent alone; image, projected-
    depth and computed-depth cotangents with g_refdepth; the same with g_refdepth NULL) within 4 max(1, e of fp32 autograd through
    the oracle); g_refdepth within the scatter bound.

    [False-1x2x2-rand] is the case that found project_backward's cancelling sum (gd = gX q0 + gY q1 + gZr q2 = -2.8169 - 0.2235 +
    4.1444 at pixel (0, 1): e = 7.433 against a yardstick of 0.364); the kernel now evaluates the quotient rule's numerator as
    q_i b2 - b_i q2, without the terms that cancel (profiles/geom_guarded_ebound.txt)."""
    lib, st = _lib()
    B, H, W, kind, seed = case
    c, unsafe, _ = GG.safe_warp_inputs(B, H, W, seed, kind, ac)
    assert unsafe == 0, (case, ac, "a coordinate, Z or reference depth sits within the margin of a decision")
    name = "inverse_warp2 %dx%dx%d %s ac %d" % (B, H, W, kind, ac)
    want = [t.detach() for t in _oracle_warp(c["img"], c["depth"], c["ref_depth"], c["pose"], c["K"], ac)]
    first = None
    for off in GC.OFFS:
        tag = "%s off %d" % (name, off)
        fwd, grads = _run_warp(lib, st, c, ac, off, tag, True)
        for got, w, what in zip(fwd, want, ("image", "valid", "projected depth", "computed depth")):
            assert G.bits_equal(got, w), (tag, what + " is not the oracle's")
        flat = [t for run in ("img", "all", "all-noref") for t in grads[run]]
        first = first or flat
        _same(tag, first, flat)
    gimg, gall, gnoref = first[0:2], first[2:5], first[5:7]
    for run, with_depths, got in (("img", False, gimg), ("all", True, gall), ("all-noref", True, gnoref)):
        yd, yp, _ = _warp_grads(_oracle_warp, c, ac, F32, with_depths)
        rd, rp, _ = _warp_grads(_ref_warp, c, ac, F64, with_depths)
        GG.check_chain("%s %s g_depth" % (name, run), got[0], yd, rd)
        GG.check_chain("%s %s g_pose" % (name, run), got[1], yp, rp)
    # g_refdepth: the scatter of g_pdepth (where the interpolated depth is above its clamp) through the kernel's own fp32 taps
    with O.trig("cr"):
        g32, _ = O._rigid_grid(c["depth"], c["pose"], c["K"])
    gn = g32.detach().numpy().reshape(B, H * W, 2)
    taps = GG.taps_from_coords(GG.unnormalize_f32(gn[:, :, 0].copy(), W, ac), GG.unnormalize_f32(gn[:, :, 1].copy(), H, ac), H, W)
    r64 = GG.inverse_warp2_ref(*(c[k].double() for k in ("img", "depth", "ref_depth", "pose", "K")), ac)
    g = torch.where(r64["vraw"] >= GG.Z_MIN, c["wp"].double().reshape(B, H * W), torch.zeros(B, H * W, dtype=F64))
    ref, mass, cnt = GG.scatter_ref(taps, g, H * W)
    sh = (B, 1, H, W)
    G.check_scatter_bound(name + " g_refdepth", gall[2], ref.reshape(sh), mass.reshape(sh), cnt.reshape(sh), float(c["wp"].abs().max()))
    _, _, r_ref = _warp_grads(_ref_warp, c, ac, F64, True)
    assert float((ref.reshape(sh) - r_ref).abs().max()) <= 1e-3 * float(r_ref.abs().max()), (name, "the scatter reference disagrees with float64 autograd")


_WARP_FWD = [c for c in GC.warp_fwd_cases() if c[3] in ("identity", "clamp")]


@pytest.mark.parametrize("case", _WARP_FWD, ids=["%dx%dx%d-%s" % c[:4] for c in _WARP_FWD])
def test_inverse_warp2_identity_and_clamped_poses_forward_and_guard_bands(case):
    """every coordinate an integer (identity) / every Z below 1e-3 (clamp): the forward is the oracle's bit for bit; the backward
    runs for its memory contract alone -- its gradients sit on the decisions and are held to no bound"""
    lib, st = _lib()
    B, H, W, kind, seed = case
    c = GG.warp_inputs(B, H, W, seed, kind)
    for ac in (False, True):
        want = [t.detach() for t in _oracle_warp(c["img"], c["depth"], c["ref_depth"], c["pose"], c["K"], ac)]
        first = None
        for off in GC.OFFS:
            tag = "inverse_warp2 %dx%dx%d %s ac %d off %d" % (B, H, W, kind, ac, off)
            fwd, grads = _run_warp(lib, st, c, ac, off, tag, True)
            for got, w, what in zip(fwd, want, ("image", "valid", "projected depth", "computed depth")):
                assert G.bits_equal(got, w), (tag, what + " is not the oracle's")
            flat = [t for run in ("img", "all", "all-noref") for t in grads[run]]
            first = first or flat
            _same(tag, first, flat)


def test_inverse_warp2_refuses_a_single_row_or_column():
    lib, st = _lib()
    t = torch.ones(1, 3, 1, 4)
    ic, dc, cams = _carve(t), _carve(t[:, :1]), G.Carved((1, int(lib.dfe_camera_floats())))
    out, gd, gp, part = G.Carved((1, 3, 1, 4)), G.Carved((1, 1, 1, 4)), G.Carved((1, 6)), G.Carved((12,))
    for H, W in ((1, 4), (4, 1)):
        assert lib.dfe_inverse_warp2_fwd(_p(ic), _p(dc), None, _p(cams), _p(out), None, None, None, 1, H, W, 0, st) == -2
        assert lib.dfe_inverse_warp2_bwd(_p(ic), _p(dc), None, _p(cams), _p(ic), None, None, _p(gd), None, None, _p(gp), _p(part), 1, H, W, 0, st) == -2
    torch.cuda.synchronize()
    assert all(x.untouched() and x.intact() for x in (out, gd, gp, part))


# ========================================================================================================= rigid flow
_FLOW = GC.flow_cases()


@pytest.mark.parametrize("case", _FLOW, ids=["%dx%dx%d-%s" % c[:4] for c in _FLOW])
def test_rigid_flow_forward_and_gradients(case):
    lib, st = _lib()
    B, H, W, kind, seed = case
    c, unsafe = GG.safe_flow_inputs(B, H, W, seed, kind)
    assert unsafe == 0, (case, "a Z sits within the margin of its clamp")
    name = "rigid_flow %dx%dx%d %s" % (B, H, W, kind)
    npart = int(lib.dfe_pose_partials_floats(B, H, W))
    with O.trig("cr"):
        want = O.calculate_rigid_flow(c["depth"], c["pose"], c["K"])
        d32, p32 = c["depth"].clone().requires_grad_(True), c["pose"].clone().requires_grad_(True)
        yd, yp = torch.autograd.grad((O.calculate_rigid_flow(d32, p32, c["K"]) * c["wf"]).sum(), [d32, p32])
    d64, p64 = c["depth"].double().requires_grad_(True), c["pose"].double().requires_grad_(True)
    rd, rp = torch.autograd.grad((GG.rigid_flow_ref(d64, p64, c["K"].double())[0] * c["wf"].double()).sum(), [d64, p64])
    first = None
    for off in GC.OFFS:
        tag = "%s off %d" % (name, off)
        cams = _cameras(lib, st, c["pose"], c["K"], off, tag)
        dc, out = _carve(c["depth"], (off + 1) % 4), G.Carved((B, 2, H, W), (off + 2) % 4)
        assert lib.dfe_rigid_flow_fwd(_p(dc), _p(cams), _p(out), B, H, W, st) == 0, tag
        _check(tag + " fwd", [dc, cams, out], [out], [(dc, c["depth"])])
        assert G.bits_equal(out.cpu(), want), (tag, "the flow is not the oracle's")
        gc, gd, gp, part = _carve(c["wf"], (off + 3) % 4), G.Carved((B, 1, H, W), off), G.Carved((B, 6), (off + 1) % 4), G.Carved((npart,), (off + 2) % 4)
        assert lib.dfe_rigid_flow_bwd(_p(dc), _p(cams), _p(gc), _p(gd), _p(gp), _p(part), B, H, W, st) == 0, tag
        _check(tag + " bwd", [dc, cams, gc, gd, gp, part], [gd, gp, part], [(dc, c["depth"]), (gc, c["wf"])])
        first = first or [gd.cpu(), gp.cpu()]
        _same(tag, first, [gd.cpu(), gp.cpu()])
    if kind != "clamp":                     # every Z below 1e-3: U = X / 1e-3, gradients of order 1e6 with nothing to compare to
        GG.check_chain(name + " g_depth", first[0], yd, rd)
        GG.check_chain(name + " g_pose", first[1], yp, rp)


# ========================================================================================================= SSIM
@pytest.mark.parametrize("shape", GC.SSIM_SHAPES)
def test_ssim_forward_and_gradients(shape):
    lib, st = _lib()
    B, C, H, W = shape
    x, y, wgt, seed = GG.ssim_inputs(shape, sum(shape))
    s64 = GG.ssim_ref(x.double(), y.double())
    pre, gate = GG.ssim_loss_gate(s64)
    assert bool((pre.abs() >= GG.MARGIN).all()) and bool(((pre - 1.0).abs() >= GG.MARGIN).all())
    gout = (-0.5 * wgt.double() * gate).float()                       # the cotangent of sum(wgt * clamp((1 - SSIM) / 2, 0, 1))
    x32, y32 = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    s32 = O.SSIM(x32, y32)
    yx, yy = torch.autograd.grad((s32 * gout).sum(), [x32, y32])
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    rx, ry = torch.autograd.grad((GG.ssim_ref(x64, y64) * gout.double()).sum(), [x64, y64])
    name = "ssim %s" % (shape,)
    first = None
    for off in GC.OFFS:
        tag = "%s off %d" % (name, off)
        xc, yc, out = _carve(x, off), _carve(y, (off + 1) % 4), G.Carved(shape, (off + 2) % 4)
        assert lib.dfe_ssim_fwd(_p(xc), _p(yc), _p(out), B, C, H, W, st) == 0, tag
        _check(tag + " fwd", [xc, yc, out], [out], [(xc, x), (yc, y)])
        gc, gx, gy = _carve(gout, (off + 3) % 4), G.Carved(shape, off), G.Carved(shape, (off + 1) % 4)
        assert lib.dfe_ssim_bwd(_p(xc), _p(yc), _p(gc), _p(gx), _p(gy), B, C, H, W, st) == 0, tag
        _check(tag + " bwd", [xc, yc, gc, gx, gy], [gx, gy], [(xc, x), (yc, y), (gc, gout)])
        gx1, gy1 = G.Carved(shape, (off + 2) % 4), G.Carved(shape, (off + 3) % 4)
        assert lib.dfe_ssim_bwd(_p(xc), _p(yc), _p(gc), _p(gx1), None, B, C, H, W, st) == 0, tag
        assert lib.dfe_ssim_bwd(_p(xc), _p(yc), _p(gc), None, _p(gy1), B, C, H, W, st) == 0, tag
        _check(tag + " bwd one side", [xc, yc, gc, gx1, gy1], [gx1, gy1])
        got = [out.cpu(), gx.cpu(), gy.cpu()]
        assert G.bits_equal(gx1.cpu(), got[1]) and G.bits_equal(gy1.cpu(), got[2]), (tag, "a single gradient differs from the pair")
        first = first or got
        _same(tag, first, got)
    GG.check_chain(name + " value", first[0], s32.detach(), s64)
    GG.check_chain(name + " gx", first[1], yx, rx)
    GG.check_chain(name + " gy", first[2], yy, ry)


def test_ssim_of_a_constant_image_with_itself_forward_only():
    """x == y constant: the value sits on the clamp of the loss, so only the forward is held to a bound"""
    lib, st = _lib()
    shape = (1, 3, 8, 8)
    x = torch.full(shape, 0.5)
    for off in GC.OFFS:
        xc, out = _carve(x, off), G.Carved(shape, (off + 1) % 4)
        assert lib.dfe_ssim_fwd(_p(xc), _p(xc), _p(out), 1, 3, 8, 8, st) == 0
        _check("ssim const off %d" % off, [xc, out], [out], [(xc, x)])
        GG.check_chain("ssim const off %d" % off, out.cpu(), O.SSIM(x, x), GG.ssim_ref(x.double(), x.double()))


def test_ssim_refuses_more_planes_than_a_grid_dimension():
    lib, st = _lib()
    xc, out, gx = _carve(torch.ones(1, 1, 1, 1)), G.Carved((1, 1, 1, 1)), G.Carved((1, 1, 1, 1))
    assert lib.dfe_ssim_fwd(_p(xc), _p(xc), _p(out), 256, 256, 1, 1, st) == -2
    assert lib.dfe_ssim_bwd(_p(xc), _p(xc), _p(xc), _p(gx), None, 65536, 1, 1, 1, st) == -2
    torch.cuda.synchronize()
    assert out.untouched() and gx.untouched() and out.intact() and gx.intact()


# ========================================================================================================= masks
@pytest.mark.parametrize("shape", GC.PIXEL_SHAPES + [GC.TINY_SHAPE])
def test_mask_decisions_are_the_oracles_and_the_float64_ones(shape):
    lib, st = _lib()
    B, H, W = shape
    alpha, beta = 0.01, 0.5
    d = GG.mask_inputs(B, H, W, sum(shape))
    assert all(G.margin_ok(v, a) for v, a in d["margins"])
    m = O.GeomLossOracle(num_scales=1, flow_consist_alpha=alpha, flow_consist_beta=beta)
    with O.occ_exp("cr"):
        wb, wf, vb, vf = (t[0] for t in m.compute_occ_weight([d["from_l"]], [d["tgt"]], [d["from_r"]]))
    tex = m.compute_texture_mask([d["tgt"]], [d["from_l"]], [d["from_r"]])[0]
    diff = torch.abs(d["rigid"] - d["flow"])
    bound = alpha * (torch.pow(O._l2norm(d["flow"]), 2) + torch.pow(O._l2norm(d["rigid"]), 2)) + beta
    dyn, score = (torch.pow(O._l2norm(diff), 2) < bound).float(), 1.0 / (1e-4 + O._l2norm(diff))
    for off in GC.OFFS:
        tag = "masks %s off %d" % (shape, off)
        o = lambda k: (off + k) % 4
        lc, tc, rc = _carve(d["from_l"], o(0)), _carve(d["tgt"], o(1)), _carve(d["from_r"], o(2))
        outs = [G.Carved((B, 1, H, W), o(k)) for k in (3, 0, 1, 2)]
        assert lib.dfe_occ_masks(_p(lc), _p(tc), _p(rc), *[_p(c) for c in outs], B, H, W, st) == 0, tag
        _check(tag + " occ", [lc, tc, rc] + outs, outs, [(lc, d["from_l"]), (tc, d["tgt"]), (rc, d["from_r"])])
        for got, want, what in zip(outs, (wb, wf, vb, vf), ("occ_bwd", "occ_fwd", "valid_bwd", "valid_fwd")):
            assert G.bits_equal(got.cpu(), want), (tag, what)
        assert G.bits_equal(outs[0].cpu(), d["occ_bwd"]) and G.bits_equal(outs[1].cpu(), d["occ_fwd"]), (tag, "not the float64 decision")
        tx = G.Carved((B, 1, H, W), o(3))
        assert lib.dfe_texture_mask(_p(tc), _p(lc), _p(rc), _p(tx), B, H, W, st) == 0, tag
        _check(tag + " texture", [lc, tc, rc, tx], [tx], [(lc, d["from_l"]), (tc, d["tgt"]), (rc, d["from_r"])])
        assert G.bits_equal(tx.cpu(), tex) and G.bits_equal(tx.cpu(), d["texture"]), tag
        fc, gc, mk, sc, mk2 = _carve(d["flow"], o(1)), _carve(d["rigid"], o(2)), G.Carved((B, 1, H, W), o(3)), G.Carved((B, 1, H, W), o(0)), G.Carved((B, 1, H, W), o(1))
        assert lib.dfe_dynamic_mask(_p(fc), _p(gc), _p(mk), _p(sc), _f(alpha), _f(beta), B, H, W, st) == 0, tag
        assert lib.dfe_dynamic_mask(_p(fc), _p(gc), _p(mk2), None, _f(alpha), _f(beta), B, H, W, st) == 0, tag
        _check(tag + " dynamic", [fc, gc, mk, sc, mk2], [mk, sc, mk2], [(fc, d["flow"]), (gc, d["rigid"])])
        assert G.bits_equal(mk.cpu(), dyn) and G.bits_equal(mk.cpu(), d["dyna"]) and G.bits_equal(mk2.cpu(), dyn), tag
        assert G.bits_equal(sc.cpu(), score), (tag, "score")


# ========================================================================================================= forward splat
@pytest.mark.parametrize("shape", GC.PIXEL_SHAPES)
def test_forward_splat_against_a_float64_scatter(shape):
    lib, st = _lib()
    B, H, W = shape
    n = B * H * W
    for k, kind in enumerate(GC.SPLAT_KINDS):
        flow = GG.splat_flow(kind, B, H, W, torch.Generator().manual_seed(sum(shape) + k))
        ref, mass, cnt = GG.splat_ref(flow)
        first = None
        for off in GC.OFFS:
            tag = "forward_splat %s %s off %d" % (shape, kind, off)
            fc, out, ws = _carve(flow, off), G.Carved((B, 1, H, W), (off + 1) % 4), _ws(n)
            assert lib.dfe_forward_splat_ones(_p(fc), _p(out), _p(ws), B, H, W, 0, st) == 0, tag
            _check(tag, [fc, out, ws], [out])
            assert G.bits_equal(fc.cpu(), flow), (tag, "the flow changed")
            oc, ws2 = G.Carved((B, 1, H, W), (off + 2) % 4), _ws(n)
            assert lib.dfe_forward_splat_ones(_p(fc), _p(oc), _p(ws2), B, H, W, 1, st) == 0, tag
            _check(tag + " clamp01", [fc, oc, ws2], [oc])
            assert G.bits_equal(oc.cpu(), out.cpu().clamp(0.0, 1.0)), (tag, "clamp01 is not clamp(unclamped, 0, 1)")
            first = first or [out.cpu()]
            _same(tag, first, [out.cpu()])
        G.check_scatter_bound("forward_splat %s %s" % (shape, kind), first[0], ref, mass, cnt, 1.0)
        if kind == "nan":                   # the source pixel with the NaN deposits nothing: as if it pointed far outside
            away = torch.where(torch.isnan(flow), torch.full_like(flow, 1e6), flow)
            fc, out, ws = _carve(away), G.Carved((B, 1, H, W)), _ws(n)
            assert lib.dfe_forward_splat_ones(_p(fc), _p(out), _p(ws), B, H, W, 0, st) == 0
            _check("forward_splat away", [fc, out, ws], [out])
            assert G.bits_equal(out.cpu(), first[0]), (shape, "a NaN flow element changed another pixel's deposit")
