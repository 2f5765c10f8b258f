"""The PnP operator (pnp.py over csrc/ops_pnp.hip) against the float64 composition of ``GeometrySolvers.pnp`` on the same sets and on
float64 points formed as the operator forms them, on the cases of tests/pnp_cases.py: (B, H, W, k, num, hyp) = (2, 12, 20, 72, 64,
32) without and with noise, (2, 13, 19, 72, 70, 33) and (2, 20, 24, 320, 300, 70) -- num above the scoring kernel's match tile
(dfe::ransac::MATCH_TILE = 256: two blocks per plane, the second partly filled) and hyp above its hypothesis tile (HYP_TILE = 64)
and no multiple of it -- plus the case whose first refinement falls back to all matches.  Every buffer of the raw entry points is
carved out of a guarded one (tests/ransac_run.py, which also holds the test bodies shared with tests/test_hip_eight_point.py).
The edge cases (PC.EDGE_SEEDS): planes without a single vote (best count 0, winner slot 0, both fall-backs), rotations of 0.13
to 0.37 rad and of none at all (so3_log's series branch), num = 256 and hyp = 128 (exactly one match tile and two hypothesis
tiles), B = 1 and B = 3.  An edge case is held to max(P_BOUND, 10 x y), y = the composition at 40 iterations
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
from tests import ransac_run as RR
from tests.ransac_run import P, _bits, _equal_decisions, _tag

pytestmark = pytest.mark.gpu

P_MEASURED = 1.273e-09
P_BOUND = 10.0 * P_MEASURED
TRUE_MEASURED = 1.212e-07
TRUE_BOUND = 10.0 * TRUE_MEASURED
WEIGHTS_OF = PC.WEIGHTS_OF


def raw_ransac(case, sets=None, flow_bwd=None, flow_fwd=None, disp_t=None, offsets=(1, 2, 3, 2), iters=PC.ITERS):
    """dfe_pnp_ransac through RR.raw_ransac, the disparity and the camera matrices carved as well -> dict of CPU tensors (``Rh``
    [2B,hyp,3,3], ``Th`` [2B,hyp,3]: the hypotheses section of the workspace, bits as the kernel left them); guards checked."""
    from unsupervised_depth_opticalflow_egomotion_amd import _lib, pnp
    lib = _lib.get_lib()
    B, H, W = case["B"], case["H"], case["W"]
    dt = G.Carved((B, 1, H, W), offset_floats=offsets[2], fill=case["disp_t"] if disp_t is None else disp_t)
    Kc = G.Carved((B, 9), offset_floats=1, fill=case["K"].reshape(B, 9))
    Kic = G.Carved((B, 9), offset_floats=3, fill=case["K_inv"].reshape(B, 9))

    def launch(fb, ff, idx, pick, sets, P64, P32, info, ws, dims):
        assert lib.dfe_pnp_ws_bytes(B, dims[4], dims[5]) == pnp.workspace_sections(B, dims[4], dims[5])["bytes"]
        _lib.check(lib.dfe_pnp_ransac(fb, ff, P(dt.ptr), idx, pick, sets, P(Kc.ptr), P(Kic.ptr), P64, P32, info, ws, *dims, iters,
                                      PC.THRESH, _lib.stream_ptr()), "dfe_pnp_ransac")
    out = RR.raw_ransac(case, launch, pnp.workspace_sections, 6, ("Ph", 12), sets, flow_bwd, flow_fwd, offsets, more=(dt, Kc, Kic))
    Ph = out.pop("table")
    out.update(Rh=Ph[:, :, :9].reshape(2 * B, -1, 3, 3).clone(), Th=Ph[:, :, 9:].clone(), P64=out.pop("est64"), P32=out.pop("est32"))
    return out


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
          "axis-angle norms %.3e to %.3e" % (name, _tag(PC.EDGE_SEEDS[name][0]), e, y, bound,
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
              % (_tag(key), e, yard))
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
    RR.tied_counts_go_to_the_lowest_index(*result(PC.SHAPES[0]), raw_ransac, "P64")


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
    l64, g64 = PC.loss_reference(out["P32"].double(), pose, beta, w)
    assert float(g64[at, 0, 4]) == 0.0
    Pc = G.Carved((2 * B, 6), offset_floats=2, fill=out["P32"])
    p = pose.cuda().requires_grad_(True)
    loss = pnp.PnpLossFn.apply(p, Pc.view, beta)
    (loss * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert Pc.intact()
    el, eg = RR.loss_errors(loss, l64, (p.grad, g64))
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
        st = _lib.stream_ptr()
        beta = ctypes.c_float(0.5)
        RR.guarded_loss_entry_points(B, ins, G.Carved((B, 2, 6), offset_floats=2), WEIGHTS_OF[B],
                                     lambda *a: _lib.check(lib.dfe_pnp_loss_fwd(*a, B, beta, st), "fwd"),
                                     lambda *a: _lib.check(lib.dfe_pnp_loss_bwd(*a, B, beta, st), "bwd"))


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


def stages(case, out, cont, sets, well, tag, only=None):
    """Stages 2 to 4 of a run on ``sets`` (``well``: PC.well_defined of them; ``only``: a further mask for stage 2)."""
    comp = case["comp"] if sets is case["sets"] else PC.composition_of(case, case["x"], case["X"], sets=sets)
    check_ill_defined_slots(out, comp, well, tag, only)
    RR.check_scoring(out, cont["err"], cont["inl"], PC.THRESH, PC.MARGIN, z=cont["zh"])
    check_consensus_and_estimate(case, out, cont, tag)


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


@pytest.mark.parametrize("key", PC.DRAWN_SHAPES)
def test_drawn_sets_stage_by_stage(key):
    case, out, cont = drawn_result(key)
    RR.drawn_sets_stage_by_stage(case, out, cont, stages, key)
    ref = case["ref"]
    again = PC.continued(case, torch.where(case["well"].view(*case["well"].shape, 1, 1), ref["Rh"], torch.full_like(ref["Rh"], float("nan"))),
                         ref["Th"], iterations=2 * PC.ITERS)
    assert rel_err(out["P64"], ref["P"]) <= max(P_BOUND, 10.0 * rel_err(again["P"], ref["P"]))


def test_a_winner_with_repeated_matches_reaches_both_refinements():
    case = PC.ill_winner_case()
    out = raw_ransac(case)
    RR.a_winner_with_repeated_matches(case, out, PC.continued(case, out["Rh"], out["Th"]), stages, 6)


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
    """RR.crafted_run on the coincident baseline."""
    case, base = coincident_result()
    return RR.crafted_run(PC, case, base, raw_ransac, stages, ("Rh", "Th"), ("P64", "P32"), slots, tag)


def test_degenerate_sets_stay_inside_their_own_slice():
    """Slots 0, 31, 32, 63, 64 and 69 (the ends of the hypothesis kernel's 32-thread blocks and of the scoring kernel's 64-slot
    LDS round) hold six copies of one index, two indices three times, three indices twice, and six matches of one pixel (six
    coincident points).  No winner is among them: the estimate does not move."""
    RR.degenerate_sets_stay_inside_their_own_slice(coincident_result()[1], _crafted_run, ("P64", "P32"))


def test_a_degenerate_set_in_the_winning_slot_hands_over_to_the_runner_up():
    RR.a_degenerate_winning_slot_hands_over_to_the_runner_up(coincident_result()[1], _crafted_run)


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
