"""The PnP operator (pnp.py over csrc/ops_pnp.hip) against the float64 composition of ``GeometrySolvers.pnp`` on the same sets and on
float64 points formed as the operator forms them, on the cases of tests/pnp_cases.py: (B, H, W, k, num, hyp) = (2, 12, 20, 72, 64,
32) without and with noise, (2, 13, 19, 72, 70, 33) and (2, 20, 24, 320, 300, 70) -- num above the scoring kernel's match tile
(PNP_MATCH_TILE = 256: two blocks per plane, the second partly filled) and hyp above its hypothesis tile (PNP_HYP_TILE = 64) and no
multiple of it -- plus the case whose first refinement falls back to all matches.  Every buffer of the raw entry points is carved
out of a guarded one.  The edge cases (PC.EDGE_SEEDS): planes without a single vote (best count 0, winner slot 0, both fall-backs),
rotations of 0.13 to 0.37 rad and of none at all (so3_log's series branch), num = 256 and hyp = 128 (exactly one match tile and
two hypothesis tiles), B = 1 and B = 3.  An edge case is held to max(P_BOUND, 10 x y), y = the composition at 40 iterations
against itself at 20 on that case.

Votes and weights are integers and the cases keep every residual a relative 1e-6 away from the threshold: they must be EQUAL.
``P64``: Levenberg-Marquardt's accept test ``cn < cost`` is decided on rounding noise once the iteration has converged, and the
minimum of a cost known to a relative 1e-16 is located to about its square root, so equality with the composition is not the
contract.  Measured on the device, max |P - P_comp| / max |P_comp| over the planes of all cases is P_MEASURED
(profiles/pnp_ebound.txt, next to the composition's own 20-versus-40-iteration difference); P_BOUND is ten times that.  The
noise-free case recovers the analytic pose to TRUE_MEASURED (what fp32 flows, disparities and camera matrices allow; same file),
asserted at ten times that.  Loss and gradient: the project's written tolerances, 5e-6 relative and 2e-5 of the
gradient's scale."""
import ctypes
import functools

import pytest
import torch

from tests import guarded as G
from tests import pnp_cases as PC

pytestmark = pytest.mark.gpu

P_MEASURED = 1.273e-09
P_BOUND = 10.0 * P_MEASURED
TRUE_MEASURED = 1.212e-07
TRUE_BOUND = 10.0 * TRUE_MEASURED
P = ctypes.c_void_p
WEIGHTS_OF = {1: (0.7,), 2: (0.7, 1.3), 3: (0.7, 1.3, 0.9)}         # a different cotangent per sample


def _i32(carved):
    return carved.view.contiguous().view(torch.int32).cpu()


def raw_ransac(case, sets=None, flow_bwd=None, flow_fwd=None, disp_t=None, offsets=(1, 2, 3, 2), iters=PC.ITERS):
    """dfe_pnp_ransac with the flows, the disparity, the camera matrices, every output and the workspace carved -> dict of CPU
    tensors (``Rh`` [2B,hyp,3,3], ``Th`` [2B,hyp,3]: the hypotheses section of the workspace, bits as the kernel left them);
    guards checked."""
    from unsupervised_depth_opticalflow_egomotion_amd import _lib, pnp
    lib = _lib.get_lib()
    B, H, W, k, num = (case[n] for n in ("B", "H", "W", "k", "num"))
    sets = (case["sets"] if sets is None else sets).cuda().contiguous()
    hyp = sets.shape[1]
    fb = G.Carved((B, 2, H, W), offset_floats=offsets[0], fill=case["flow_bwd"] if flow_bwd is None else flow_bwd)
    ff = G.Carved((B, 2, H, W), offset_floats=offsets[1], fill=case["flow_fwd"] if flow_fwd is None else flow_fwd)
    dt = G.Carved((B, 1, H, W), offset_floats=offsets[2], fill=case["disp_t"] if disp_t is None else disp_t)
    Kc = G.Carved((B, 9), offset_floats=1, fill=case["K"].reshape(B, 9))
    Kic = G.Carved((B, 9), offset_floats=3, fill=case["K_inv"].reshape(B, 9))
    idx, pick = case["idx"].cuda(), case["pick"].cuda()
    P64 = G.Carved((2 * B * 6, 2), offset_floats=offsets[3])          # doubles: 8-byte aligned, not 16
    P32 = G.Carved((2 * B, 6), offset_floats=offsets[2])
    info = G.Carved((2 * B, 4), offset_floats=1)
    sec = pnp.workspace_sections(B, num, hyp)
    assert lib.dfe_pnp_ws_bytes(B, num, hyp) == sec["bytes"]
    ws = G.Carved((sec["bytes"] // 4,), offset_floats=0)
    _lib.check(lib.dfe_pnp_ransac(P(fb.ptr), P(ff.ptr), P(dt.ptr), P(idx.data_ptr()), P(pick.data_ptr()), P(sets.data_ptr()), P(Kc.ptr),
                                  P(Kic.ptr), P(P64.ptr), P(P32.ptr), P(info.ptr), P(ws.ptr), B, H, W, k, num, hyp, iters, PC.THRESH,
                                  _lib.stream_ptr()), "dfe_pnp_ransac")
    torch.cuda.synchronize()
    for c in (fb, ff, dt, Kc, Kic, P64, P32, info, ws):
        assert c.intact()
    words = _i32(ws)
    sl = lambda name, n: words[sec[name] // 4:sec[name] // 4 + n]   # noqa: E731
    Ph = sl("Ph", 2 * 2 * B * hyp * 12).clone().view(torch.float64).reshape(2 * B, hyp, 12)
    return dict(Rh=Ph[:, :, :9].reshape(2 * B, hyp, 3, 3).clone(), Th=Ph[:, :, 9:].clone(), P64=P64.view.contiguous().view(torch.float64).cpu().reshape(2 * B, 6), P32=P32.cpu().reshape(2 * B, 6),
                info=_i32(info).reshape(2 * B, 4), counts=sl("counts", 2 * B * hyp).reshape(2 * B, hyp),
                w1=sl("w1", 2 * B * num).reshape(2 * B, num), w2=sl("w2", 2 * B * num).reshape(2 * B, num),
                written=P32.written() and info.written())


@functools.lru_cache(maxsize=None)
def result(key):
    """(case with its float64 composition, the kernels' outputs): computed once, shared, never changed."""
    case = PC.make_case(key) if key != "fallback" else PC.fallback_case()
    return case, raw_ransac(case)


@functools.lru_cache(maxsize=None)
def edge_result(name):
    """``result`` for a case of PC.EDGE_SEEDS."""
    case = PC.make_edge_case(name)
    return case, raw_ransac(case)


def rel_err(Pd, ref):
    """the largest difference of a plane's pose relative to that pose's scale, over the planes"""
    return float(((Pd - ref).abs().amax(1) / ref.abs().amax(1)).max())


def _equal_decisions(out, c):
    assert out["written"]
    assert torch.equal(out["counts"].long(), c["counts"])                       # every hypothesis, as integers
    assert torch.equal(out["w1"].long(), c["w1"].long()) and torch.equal(out["w2"].long(), c["w2"].long())
    info = out["info"].long()
    assert torch.equal(info[:, 0], c["best"]) and torch.equal(info[:, 1], c["counts"].max(1)[0])
    assert torch.equal(info[:, 2], c["w1"].sum(1).long()) and torch.equal(info[:, 3], c["w2"].sum(1).long())


@pytest.mark.parametrize("key", PC.SHAPES)
def test_votes_sets_and_info_equal_the_composition(key):
    case, out = result(key)
    _equal_decisions(out, case["comp"])
    assert torch.equal(out["info"][:, 1].long(), out["w1"].sum(1).long())       # the consensus is the winner's inlier set (>= 6)


@pytest.mark.parametrize("name", PC.EDGE_SHAPES)
def test_edge_votes_sets_and_info_equal_the_composition(name):
    case, out = edge_result(name)
    c, num = case["comp"], case["num"]
    _equal_decisions(out, c)
    first, second = c["n1raw"] < 6, c["n2raw"] < 6
    info = out["info"].long()
    assert torch.equal(info[~first, 1], out["w1"][~first].sum(1).long())        # a consensus is the winner's inlier set
    if name == "zero":                                                           # no hypothesis gets a vote on planes 0 and 2
        assert first.tolist() == [True, False, True, False] and second.tolist() == [True, False, True, False]
        for plane in (0, 2):
            assert info[plane].tolist() == [0, 0, num, num], (plane, info[plane].tolist())
            assert bool((out["counts"][plane] == 0).all()) and bool((out["w1"][plane] == 1).all()) and bool((out["w2"][plane] == 1).all())
    else:
        assert not bool((first | second).any())


@pytest.mark.parametrize("name", PC.EDGE_SHAPES)
def test_edge_p64_against_the_composition(name):
    case, out = edge_result(name)
    ref = case["comp"]["P"]
    assert bool(torch.isfinite(out["P64"]).all())
    y = rel_err(PC.composition_of(case, case["x"], case["X"], iterations=2 * PC.ITERS)["P"], ref)
    bound = max(P_BOUND, 10.0 * y)
    e = rel_err(out["P64"], ref)
    norms = out["P64"][:, 3:].norm(dim=1)
    print("EBOUND pnp P64 edge %s %s max|dP|/max|P| %.3e; y (the composition at 40 iterations against itself at 20) %.3e bound %.3e; "
          "axis-angle norms %.3e to %.3e" % (name, "x".join(str(int(v)) for v in PC.EDGE_SEEDS[name][0]), e, y, bound,
                                              float(norms.min()), float(norms.max())))
    assert torch.equal(out["P32"], out["P64"].float())                          # rounded once: bit equality
    assert e <= bound, (e, bound)
    if name == "rot0.3":
        assert float(norms.min()) > 0.1 and float(norms.max()) < 0.6
    if name == "rot0":                                                          # the series branch, and the analytic pose
        assert float(norms.max()) < 1e-6
        et = float((out["P64"] - case["P_true"]).abs().max())
        ec = float((case["comp"]["P"] - case["P_true"]).abs().max())
        print("EBOUND pnp noise-free rot 0 max|P - P_true| %.3e (the composition: %.3e) bound %.3e" % (et, ec, TRUE_BOUND))
        assert et <= TRUE_BOUND, (et, TRUE_BOUND)


def test_p64_against_the_composition_and_p32_is_its_rounding():
    worst = 0.0
    for key in PC.SHAPES:
        case, out = result(key)
        ref = case["comp"]["P"]
        assert bool(torch.isfinite(out["P64"]).all())
        e = rel_err(out["P64"], ref)
        yard = rel_err(PC.composition_of(case, case["x"], case["X"], iterations=2 * PC.ITERS)["P"], ref)
        print("EBOUND pnp P64 %s max|dP|/max|P| %.3e; the composition at 40 iterations against itself at 20: %.3e"
              % ("x".join(str(int(v)) for v in key), e, yard))
        worst = max(worst, e)
        assert torch.equal(out["P32"], out["P64"].float())                      # rounded once: bit equality
    print("EBOUND pnp P64 all cases %.3e bound %.3e" % (worst, P_BOUND))
    assert worst <= P_BOUND, (worst, P_BOUND)


def test_the_noise_free_case_recovers_the_analytic_pose():
    case, out = result(PC.SHAPES[0])
    assert not case["noisy"]
    e = float((out["P64"] - case["P_true"]).abs().max())
    ec = float((case["comp"]["P"] - case["P_true"]).abs().max())
    print("EBOUND pnp noise-free max|P - P_true| %.3e (the composition: %.3e) bound %.3e" % (e, ec, TRUE_BOUND))
    assert e <= TRUE_BOUND, (e, TRUE_BOUND)


def test_the_fallback_case_refines_over_all_matches_first():
    case, out = result("fallback")
    c = case["comp"]
    _equal_decisions(out, c)
    few = c["n1raw"] < 6
    assert bool(few.any())
    info = out["info"].long()
    assert bool((info[few, 1] < 6).all()) and bool((info[few, 2] == case["num"]).all()) and bool((out["w1"][few] == 1).all())
    assert bool((info[few, 3] >= 6).all())                                      # the refinement over all matches still converged
    e = rel_err(out["P64"], c["P"])
    print("EBOUND pnp P64 fall-back case max|dP|/max|P| %.3e bound %.3e" % (e, P_BOUND))
    assert e <= P_BOUND, (e, P_BOUND)


def test_tied_counts_go_to_the_lowest_index():
    """Two identical hypotheses: the winner of plane (d = 0, b = 0) is copied to another slot of sample 0's sets; both have the
    maximum count of that plane and the lower slot wins.  The estimate does not move."""
    key = PC.SHAPES[0]
    case, out = result(key)
    best = int(case["comp"]["best"][0])
    slot = 0 if best != 0 else 1
    sets = case["sets"].clone()
    sets[0, slot] = sets[0, best]
    tied = raw_ransac(case, sets=sets)
    assert int(tied["counts"][0, slot]) == int(tied["counts"][0, best]) == int(out["info"][0, 1])
    assert int(tied["info"][0, 0]) == min(slot, best) and int(tied["info"][0, 1]) == int(out["info"][0, 1])
    assert torch.equal(tied["w1"][0], out["w1"][0]) and torch.equal(tied["P64"][0], out["P64"][0])


def _loss_reference(P64, pose, beta, weights, dtype=torch.float64):
    """float64: compute_pnp_loss's expression per direction and sample, fed the given pose estimate; the gradient of
    sum(weights * loss) with respect to the pose vector.  ``dtype`` = float32: the same expression in fp32."""
    import torch.nn.functional as F
    B = pose.shape[0]
    pose = pose.to(dtype).requires_grad_(True)
    loss = 0
    for d in range(2):
        est = P64[d * B:(d + 1) * B].to(dtype)
        term = F.l1_loss(est[:, :3], pose[:, d, :3], reduction="none") + beta * F.l1_loss(est[:, 3:], pose[:, d, 3:], reduction="none")
        loss = loss + term.mean(1)
    (loss * weights.to(dtype)).sum().backward()
    return loss.detach(), pose.grad


@pytest.mark.parametrize("scale", [1.0, 40.0])
def test_loss_and_gradient_against_float64(scale):
    """Two pose scales; element (1, 0, 4) of the pose vector equals ``P32`` exactly: sign(0) = 0, the gradient there is 0."""
    _loss_against_float64(*result(PC.SHAPES[2]), scale, at=1)


@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("name", ["b1", "b3"])
def test_loss_and_gradient_at_one_sample_and_three(name, scale):
    """Element (B - 1, 0, 4) of the pose vector equals ``P32`` exactly, as above."""
    case, out = edge_result(name)
    _loss_against_float64(case, out, scale, at=case["B"] - 1, tag=" " + name)


def _loss_against_float64(case, out, scale, at, tag=""):
    from unsupervised_depth_opticalflow_egomotion_amd import pnp
    B, beta = case["B"], 0.75
    w = torch.tensor(WEIGHTS_OF[B])
    pose = PC.pose_vectors(case, scale=scale)
    pose[at, 0, 4] = out["P32"][0 * B + at, 4]
    l64, g64 = _loss_reference(out["P32"].double(), pose, beta, w)
    assert float(g64[at, 0, 4]) == 0.0
    Pc = G.Carved((2 * B, 6), offset_floats=2, fill=out["P32"])
    p = pose.cuda().requires_grad_(True)
    loss = pnp.PnpLossFn.apply(p, Pc.view, beta)
    (loss * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert Pc.intact()
    el = float(((loss.detach().double().cpu() - l64).abs() / l64.abs()).max())
    eg = float((p.grad.double().cpu() - g64).abs().max() / g64.abs().max())
    print("EBOUND pnp loss%s scale %g: loss %.3e (5e-6)  dpose %.3e (2e-5)" % (tag, scale, el, eg))
    assert el <= 5e-6 and eg <= 2e-5
    assert float(p.grad[at, 0, 4]) == 0.0 and int((p.grad == 0).sum()) == 1


def test_loss_entry_points_in_guarded_buffers():
    _guarded_loss_entry_points([result(key) for key in PC.SHAPES[1:]])


def test_loss_entry_points_in_guarded_buffers_at_one_sample_and_three():
    _guarded_loss_entry_points([edge_result(name) for name in ("b1", "b3")])


def _guarded_loss_entry_points(results):
    from unsupervised_depth_opticalflow_egomotion_amd import _lib
    lib = _lib.get_lib()
    for case, out in results:
        B = case["B"]
        ins = [G.Carved((B, 2, 6), offset_floats=1, fill=PC.pose_vectors(case)), G.Carved((2 * B, 6), offset_floats=3, fill=out["P32"])]
        loss, gloss, gp = G.Carved((B,), offset_floats=1), G.Carved((B,), offset_floats=3, fill=torch.tensor(WEIGHTS_OF[B])), G.Carved((B, 2, 6), offset_floats=2)
        st = _lib.stream_ptr()
        beta = ctypes.c_float(0.5)
        _lib.check(lib.dfe_pnp_loss_fwd(*[P(c.ptr) for c in ins], P(loss.ptr), B, beta, st), "fwd")
        _lib.check(lib.dfe_pnp_loss_bwd(*[P(c.ptr) for c in ins], P(gloss.ptr), P(gp.ptr), B, beta, st), "bwd")
        torch.cuda.synchronize()
        assert all(c.intact() for c in ins + [loss, gloss, gp]) and loss.written() and gp.written()


def test_refusals_come_before_any_launch():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib
    lib = _lib.get_lib()
    out = G.Carved((64,), offset_floats=0)
    odd = G.Carved((64,), offset_floats=1)
    x = torch.zeros(4096, device="cuda")
    p, o, st = P(x.data_ptr()), P(out.ptr), _lib.stream_ptr()

    def call(H, W, k, num, hyp, iters=20, P64=o, ws=o):
        return lib.dfe_pnp_ransac(p, p, p, p, p, p, p, p, P64, o, o, ws, 1, H, W, k, num, hyp, iters, 1.0, st)
    assert call(8, 8, 16, 5, 4) == -2           # num = 5
    assert call(8, 8, 16, 6, 0) == -2           # hyp = 0
    assert call(8, 8, 65, 6, 4) == -2 and call(8, 8, 0, 6, 4) == -2           # k outside [1, H*W]
    assert call(1 << 14, 1 << 14, 16, 6, 4) == -2                             # H*W = 2^28
    assert call(8, 8, 16, 6, 4, iters=0) == -2
    assert call(8, 8, 16, 6, 4, P64=P(odd.ptr)) == -2 and call(8, 8, 16, 6, 4, ws=P(odd.ptr)) == -2      # 4 bytes past 16
    assert call(8, 8, 16, 16385, 4) == -4 and call(8, 8, 16, 6, 4097) == -4
    assert lib.dfe_pnp_ransac(None, p, p, p, p, p, p, p, o, o, o, o, 1, 8, 8, 16, 6, 4, 20, 1.0, st) == -1
    assert lib.dfe_pnp_loss_fwd(p, p, o, 0, ctypes.c_float(1.0), st) == -2
    assert lib.dfe_pnp_loss_bwd(p, p, p, o, 0, ctypes.c_float(1.0), st) == -2
    torch.cuda.synchronize()
    assert out.untouched() and out.intact() and odd.untouched() and odd.intact()


@pytest.mark.parametrize("where", ["flow", "disp"])
def test_a_nan_in_one_sample_leaves_the_other_samples_bits(where):
    """Run once per input: NaN at a sampled pixel of sample 1's backward flow / of its disparity.  The call returns (every loop
    is bounded); sample 0's poses, info and loss keep their bits."""
    from unsupervised_depth_opticalflow_egomotion_amd import pnp
    key = PC.SHAPES[1]
    case, out = result(key)
    B = case["B"]
    pix = int(case["idx"][1, case["pick"][3]])                      # plane d = 0, b = 1, match 3
    fb, dt = case["flow_bwd"].clone(), case["disp_t"].clone()
    if where == "flow":
        fb[1, 0].view(-1)[pix] = float("nan")
    else:
        dt[1, 0].view(-1)[pix] = float("nan")
    bad = raw_ransac(case, flow_bwd=fb, disp_t=dt)
    for plane in (0, 2):                                            # sample 0, both directions
        assert torch.equal(bad["P64"][plane], out["P64"][plane]) and torch.equal(bad["info"][plane], out["info"][plane]), plane
    if where == "flow":                                             # the forward direction of sample 1 did not read the flow
        assert torch.equal(bad["P64"][3], out["P64"][3])
    pose = PC.pose_vectors(case).cuda()
    with torch.no_grad():
        loss = pnp.PnpLossFn.apply(pose, bad["P32"].cuda(), 1.0).cpu()
        good = pnp.PnpLossFn.apply(pose, out["P32"].cuda(), 1.0).cpu()
    assert bool(torch.isfinite(loss[0])) and G.bits_equal(loss[0:1], good[0:1])


def test_two_runs_give_the_same_bits_and_the_wrapper_agrees():
    from unsupervised_depth_opticalflow_egomotion_amd import pnp
    key = PC.SHAPES[3]
    case, out = result(key)
    again = raw_ransac(case, offsets=(3, 0, 1, 0))
    assert torch.equal(again["P64"], out["P64"]) and torch.equal(again["info"], out["info"]) and torch.equal(again["counts"], out["counts"])
    P32, P64, info, ws = pnp.pnp_ransac(case["flow_bwd"].cuda(), case["flow_fwd"].cuda(), case["disp_t"].cuda(), case["idx"].cuda(),
                                        case["pick"].cuda(), case["sets"].cuda(), case["K"].cuda(), case["K_inv"].cuda(),
                                        iters=PC.ITERS, thresh=PC.THRESH, return_ws=True)
    assert torch.equal(P64.cpu(), out["P64"]) and G.bits_equal(P32, out["P32"]) and torch.equal(info.cpu(), out["info"])
    assert ws.numel() == pnp.workspace_sections(case["B"], case["num"], case["hyp"])["bytes"]

    def loss_and_grad():
        p = PC.pose_vectors(case).cuda().requires_grad_(True)
        loss = pnp.PnpLossFn.apply(p, P32, 1.0)
        loss.sum().backward()
        return loss.detach(), p.grad
    (l1, g1), (l2, g2) = loss_and_grad(), loss_and_grad()
    assert G.bits_equal(l1, l2) and G.bits_equal(g1, g2)
    with pytest.raises(ValueError):
        pnp.pnp_ransac(case["flow_bwd"].cuda(), case["flow_fwd"].cuda(), case["disp_t"].cuda(), case["idx"].cuda(),
                       case["pick"].cuda()[:5], case["sets"].cuda(), case["K"].cuda(), case["K_inv"].cuda())


def test_properties_on_the_products_own_sets():
    """``minimal_sets_device(k=6)``'s draw (with replacement: some sets repeat an index; such a hypothesis is ill-defined and CAN
    reach the maximum count -- test_drawn_sets_stage_by_stage holds the kernels to float64 there; this test only looks at the
    outcome): the pose is no further from the analytic one than twice the composition on the same input."""
    from unsupervised_depth_opticalflow_egomotion_amd import pnp
    case = PC.make_case(PC.SHAPES[2])
    B, num = case["B"], case["num"]
    m = PC.solvers()
    sets = m.minimal_sets_device(B, num, torch.device("cuda"), k=6)
    assert tuple(sets.shape) == (B, 256, 6) and any(row.unique().numel() < 6 for row in sets.cpu().reshape(-1, 6))
    _, P64, info = pnp.pnp_ransac(case["flow_bwd"].cuda(), case["flow_fwd"].cuda(), case["disp_t"].cuda(), case["idx"].cuda(),
                                  case["pick"].cuda(), sets, case["K"].cuda(), case["K_inv"].cuda())
    comp = PC.composition_of(case, case["x"], case["X"], sets=sets.cpu())["P"]
    P64 = P64.cpu()
    for p in range(2 * B):
        dist = lambda Q: float((Q[p] - case["P_true"][p]).abs().max())   # noqa: E731
        assert dist(P64) <= 2.0 * dist(comp), (p, dist(P64), dist(comp))
    assert int(info[:, 1].min()) >= 6


# ------------------------------------------------------------------------------------------------ the product's own draws
# ``pick`` and ``sets`` drawn with replacement (PC.build_drawn): a slot whose 6 matches are not 6 distinct pixels, or whose DLT
# system has no isolated null direction, is ill-defined, and the kernel may take another vector of its null space than ``svd``
# does.  So the kernel is held to float64 stage by stage:
#   1  the counts of the well-defined slots equal the composition's;
#   2  an ill-defined slot's own (R, T) is non-finite with count 0, or R is a rotation (R^T R = I, det R = +1) at rounding level:
#      16 x what the reference's own ill-defined hypotheses leave on the same sets;
#   3  every slot's count is the float64 recount from the kernel's own (R, T);
#   4  info, w1, w2 equal PC.continued(case, the kernel's table) and P64 is within the P bound of its pose.
NULL_FACTOR = 16.0


def rotation_bounds(comp, well, tag):
    """(orth_bound, det_bound): NULL_FACTOR x the largest figures (PC.rotation_figures) of the REFERENCE's ill-defined
    hypotheses (``comp``: its composition on the same sets), float64 on the CPU."""
    orth, det = PC.rotation_figures(comp["Rh"])
    ill = ~well
    assert bool(torch.isfinite(orth[ill]).all() and torch.isfinite(det[ill]).all())
    o, d = float(orth[ill].max()), float(det[ill].max())
    print("EBOUND pnp rotation %s reference's ill-defined slots: max|R'R - I| %.3e  |det R - 1| %.3e; bounds %.3e %.3e"
          % (tag, o, d, NULL_FACTOR * o, NULL_FACTOR * d))
    return NULL_FACTOR * o, NULL_FACTOR * d


def check_well_defined_counts(out, comp, well):
    """Stage 1."""
    assert torch.equal(out["counts"].long()[well], comp["counts"][well])


def check_ill_defined_slots(out, comp, well, tag, only=None):
    """Stage 2 on the ill-defined slots (``only``: a further mask)."""
    ob, db = rotation_bounds(comp, well, tag)
    orth, det = PC.rotation_figures(out["Rh"])
    ill = ~well if only is None else (~well & only)
    finite = torch.isfinite(out["Rh"]).all(3).all(2) & torch.isfinite(out["Th"]).all(2)
    dead = ill & ~finite
    assert bool((out["counts"][dead] == 0).all())
    live = ill & finite
    o = float(orth[live].max()) if bool(live.any()) else 0.0
    d = float(det[live].max()) if bool(live.any()) else 0.0
    print("EBOUND pnp rotation %s kernel's ill-defined slots (%d finite, %d not): max|R'R - I| %.3e  |det R - 1| %.3e"
          % (tag, int(live.sum()), int(dead.sum()), o, d))
    assert o <= ob and d <= db, (o, ob, d, db)


def check_scoring(out, cont):
    """Stage 3: every slot's count is the float64 recount from the kernel's own table; a (slot, match) pair within MARGIN of the
    threshold (or with a depth within MARGIN of zero) is left out, and a second such pair makes the case inconclusive."""
    t = PC.THRESH * PC.THRESH
    err, z = cont["err"], cont["zh"]
    near = (torch.isfinite(err) & ((err - t).abs() / t < PC.MARGIN)) | (torch.isfinite(z) & (z.abs() < PC.MARGIN))
    assert int(near.sum()) <= 1, "inconclusive: %d residuals within MARGIN of the threshold" % int(near.sum())
    sure = cont["inl"] & ~near
    got = out["counts"].long()
    assert bool((got >= sure.sum(2)).all() and (got <= sure.sum(2) + near.sum(2)).all())


def check_consensus_and_estimate(case, out, cont, tag):
    """Stage 4."""
    assert PC.conclusive(cont), "inconclusive: margin %.3e, zmargin %.3e, cond %s %s" % (cont["margin"], cont["zmargin"], cont["cond1"].tolist(), cont["cond2"].tolist())
    _equal_decisions(out, cont)
    assert bool(torch.isfinite(out["P64"]).all())
    y = rel_err(PC.continued(case, out["Rh"], out["Th"], iterations=2 * PC.ITERS)["P"], cont["P"])
    bound = max(P_BOUND, 10.0 * y)
    e = rel_err(out["P64"], cont["P"])
    print("EBOUND pnp P64 %s against the composition continued from the kernel's table: max|dP|/max|P| %.3e; y (40 iterations "
          "against 20) %.3e bound %.3e" % (tag, e, y, bound))
    assert e <= bound, (e, bound)
    assert torch.equal(out["P32"], out["P64"].float())


@functools.lru_cache(maxsize=None)
def drawn_result(key):
    """``result`` for a case of PC.DRAWN_SEEDS, with the composition continued from the kernel's own table."""
    case = PC.make_drawn_case(key)
    out = raw_ransac(case)
    return case, out, PC.continued(case, out["Rh"], out["Th"])


def _tag(key):
    return "x".join(str(int(v)) for v in key)


@pytest.mark.parametrize("key", PC.DRAWN_SHAPES)
def test_drawn_sets_stage_by_stage(key):
    case, out, cont = drawn_result(key)
    assert out["written"]
    check_well_defined_counts(out, case["comp"], case["well"])
    check_ill_defined_slots(out, case["comp"], case["well"], "drawn " + _tag(key))
    check_scoring(out, cont)
    check_consensus_and_estimate(case, out, cont, "drawn " + _tag(key))
    # the seed was chosen for a well-defined winner: none of the kernel's ill-defined slots out-polls it, and the estimate is the
    # composition's without those slots (case["ref"]: the same on every host)
    ref = case["ref"]
    assert torch.equal(out["info"].long()[:, 0], ref["best"]) and torch.equal(out["w2"].long(), ref["w2"].long())
    again = PC.continued(case, torch.where(case["well"].view(*case["well"].shape, 1, 1), ref["Rh"], torch.full_like(ref["Rh"], float("nan"))),
                         ref["Th"], iterations=2 * PC.ITERS)
    assert rel_err(out["P64"], ref["P"]) <= max(P_BOUND, 10.0 * rel_err(again["P"], ref["P"]))


def test_a_winner_with_repeated_matches_reaches_both_refinements():
    """The case whose reference winner is ill-defined: stages 2-4 alone.  The kernel's own winner of some plane repeats a match,
    and its consensus goes through both refinements with neither fall-back."""
    case = PC.ill_winner_case()
    out = raw_ransac(case)
    cont = PC.continued(case, out["Rh"], out["Th"])
    check_ill_defined_slots(out, case["comp"], case["well"], "ill-defined winner")
    check_scoring(out, cont)
    check_consensus_and_estimate(case, out, cont, "ill-defined winner")
    best = out["info"].long()[:, 0]
    repeats = ~torch.cat([PC.distinct_pixels(case)] * 2, 0)
    won = torch.gather(repeats, 1, best.view(-1, 1)).squeeze(1)
    assert bool(won.any()), "no plane's winner repeats a match"
    assert bool((cont["n1raw"][won] >= 6).all() and (cont["n2raw"][won] >= 6).all())
    assert torch.equal(out["info"].long()[won, 1], out["w1"][won].sum(1).long())      # the consensus is the winner's own set


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def coincident_result():
    """The hyp = 70 drawn case with six matches moved onto one pixel (PC.coincident_pick), its sets untouched: the baseline of
    the isolation tests."""
    case = dict(PC.make_drawn_case(PC.DRAWN_SHAPES[1]))
    case["pick"] = PC.coincident_pick(case)
    case["x"], case["X"] = PC.points_of(case)
    case["comp"] = PC.composition_of(case, case["x"], case["X"])
    case["well"] = PC.well_defined(case)
    return case, raw_ransac(case)


def _crafted_run(slots, tag):
    """The baseline with ``slots`` of sample 0's sets overwritten by degenerate sets (PC.crafted_sets): every other slot and the
    other sample bit-equal to the baseline's run, the overwritten slots through stages 2 and 3, the outputs through stage 4."""
    case, base = coincident_result()
    B, hyp = case["B"], case["hyp"]
    assert hyp == 70 and B == 2
    sets = PC.crafted_sets(case, slots)
    out = raw_ransac(case, sets=sets)
    touched = torch.zeros(2 * B, hyp, dtype=torch.bool)
    for d in range(2):
        touched[d * B, list(slots)] = True
    well = PC.well_defined(case, sets)
    assert not bool(well[touched].any()) and torch.equal(well[~touched], case["well"][~touched])
    for name in ("Rh", "Th", "counts"):                                                      # no slot's slice leaks into another's
        assert torch.equal(_bits(out[name])[~touched], _bits(base[name])[~touched]), name
    for d in range(2):                                                                       # sample 1: every output
        p = d * B + 1
        for name in ("P64", "P32", "info", "w1", "w2", "counts", "Rh", "Th"):
            assert torch.equal(_bits(out[name][p]), _bits(base[name][p])), (name, p)
    comp = PC.composition_of(case, case["x"], case["X"], sets=sets)
    cont = PC.continued(case, out["Rh"], out["Th"])
    check_ill_defined_slots(out, comp, well, tag, only=touched)
    check_scoring(out, cont)
    check_consensus_and_estimate(case, out, cont, tag)
    return case, base, out


def test_degenerate_sets_stay_inside_their_own_slice():
    """Slots 0, 31, 32, 63, 64 and 69 (the ends of the hypothesis kernel's 32-thread blocks and of the scoring kernel's 64-slot
    LDS round) hold six copies of one index, two indices three times, three indices twice, and six matches of one pixel (six
    coincident points).  No winner is among them: the estimate does not move."""
    case, base, out = _crafted_run(PC.CRAFTED_SLOTS, "crafted slots")
    assert not any(int(b) in PC.CRAFTED_SLOTS for b in base["info"][:, 0])
    for name in ("P64", "P32", "info", "w1", "w2"):
        assert torch.equal(_bits(out[name]), _bits(base[name])), name


def test_a_degenerate_set_in_the_winning_slot_hands_over_to_the_runner_up():
    case, base = coincident_result()
    best = int(base["info"][0, 0])
    slots = PC.CRAFTED_SLOTS[:5] + (best,)
    assert best not in PC.CRAFTED_SLOTS[:5]
    case, base, out = _crafted_run(slots, "crafted winner")
    counts = base["counts"][0].clone()
    counts[list(slots)] = -1
    assert int(out["counts"][0, best]) < int(counts.max())                  # the degenerate set polls less than the runner-up
    assert int(out["info"][0, 0]) == int(counts.argmax()) and int(out["info"][0, 1]) == int(counts.max())


def test_a_nan_match_leaves_its_hypotheses_without_a_vote():
    """Run once: NaN in sample 1's backward flow at the pixel of match 3.  In plane (d = 0, b = 1) every slot whose set holds a
    match of that pixel has a non-finite (R, T) and count 0 (stage 2's other branch), every other slot keeps its (R, T) bit for
    bit and its count is the float64 recount -- the NaN match votes for nobody -- and the other planes keep every count."""
    case, base, _ = drawn_result(PC.DRAWN_SHAPES[0])
    B = case["B"]
    fb = case["flow_bwd"].clone()
    pix = int(case["idx"][1, case["pick"][3]])
    fb[1, 0].view(-1)[pix] = float("nan")
    bad = raw_ransac(case, flow_bwd=fb)
    holds = (case["pick"][case["sets"][1].long()] == case["pick"][3]).any(1)
    assert bool(holds.any()) and not bool(holds.all())
    finite = torch.isfinite(bad["Rh"][1]).all(2).all(1) & torch.isfinite(bad["Th"][1]).all(1)
    assert not bool(finite[holds].any()) and bool((bad["counts"][1, holds] == 0).all())
    for name in ("Rh", "Th"):
        assert torch.equal(_bits(bad[name][1, ~holds]), _bits(base[name][1, ~holds])), name
    x, X = PC.points_of(case, flow_bwd=fb)
    v = PC._continue(x[1:2], X[1:2], case["K"][1], bad["Rh"][1:2], bad["Th"][1:2], votes_only=True)
    t = PC.THRESH * PC.THRESH
    err, z = v["err"][0], v["zh"][0]
    near = (torch.isfinite(err) & ((err - t).abs() / t < PC.MARGIN)) | (torch.isfinite(z) & (z.abs() < PC.MARGIN))
    assert not bool(near.any()), "inconclusive: a residual within MARGIN of the threshold"
    assert torch.equal(bad["counts"][1].long(), v["counts"][0])
    for plane in (0, 2, 3):
        assert torch.equal(bad["counts"][plane], base["counts"][plane]) and torch.equal(_bits(bad["P64"][plane]), _bits(base["P64"][plane]))
