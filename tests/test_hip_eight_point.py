"""The eight-point operator (eight_point.py over csrc/ops_eight_point.hip) against the float64 composition of
``GeometrySolvers.compute_fundmental_mat`` / ``compute_eight_point_loss`` on the same sets, on the cases of
tests/eight_point_cases.py: (B, H, W, k, num, hyp) = (2, 12, 20, 72, 64, 32) without and with noise, (2, 13, 19, 72, 70, 33) and
(2, 20, 24, 320, 300, 70) -- num above the scoring kernel's match tile (dfe::ransac::MATCH_TILE = 256: two blocks per plane, the
second partly filled) and hyp above its hypothesis tile (HYP_TILE = 64) and no multiple of it.  Every buffer of the raw entry
points is carved out of a guarded one (tests/ransac_run.py, which also holds the test bodies shared with tests/test_hip_pnp.py).
The edge cases (EC.EDGE_SEEDS): both fall-backs of the consensus (fewer than 8 votes: all matches; fewer than 8 inliers of the
first refit: its set is kept), num = 256 and hyp = 128 (exactly one match tile and two hypothesis tiles), B = 1 and B = 3.

Votes and weights are integers and the cases keep every residual a relative 1e-6 away from the threshold: they must be EQUAL.
``F64``: max |F - F_comp| / max |F_comp| over all cases measured on the device is 1.786e-11
(profiles/eight_point_ebound.txt); F_BOUND is 16 x that -- the headroom is for another eigen-iteration path under another
compiler -- and is asserted to lie below the composition's own distance to ``F_true`` on the noisy cases.  Loss and gradient:
the project's written tolerances, 5e-6 relative and 2e-5 of the gradient's scale.  An edge case is held to
max(F_BOUND, 16 x y), y = the float64 composition's own spread on that case between ``eigh`` of the normal matrix and ``svd``
of the design matrix (EC.reference_spread, CPU only; profiles/eight_point_ebound.txt)."""
import functools

import pytest
import torch

from tests import eight_point_cases as EC
from tests import guarded as G
from tests import ransac_run as RR
from tests.ransac_run import P, _bits, _tag

pytestmark = pytest.mark.gpu

F_MEASURED = 1.786e-11
F_BOUND = 16.0 * F_MEASURED
WEIGHTS_OF = EC.WEIGHTS_OF


def raw_ransac(case, sets=None, flow_bwd=None, flow_fwd=None, offsets=(1, 2, 3, 2)):
    """dfe_fundamental_ransac through RR.raw_ransac -> dict of CPU tensors (``Fh``: the hypotheses section of the workspace,
    [2B,hyp,3,3] doubles, bits as the kernel left them); guards checked."""
    from unsupervised_depth_opticalflow_egomotion_amd import _lib, eight_point
    lib = _lib.get_lib()

    def launch(*args):
        B, _, _, _, num, hyp = dims = args[-1]
        assert lib.dfe_eight_point_ws_bytes(B, num, hyp) == eight_point.workspace_sections(B, num, hyp)["bytes"]
        _lib.check(lib.dfe_fundamental_ransac(*args[:-1], *dims, EC.THRESH, _lib.stream_ptr()), "dfe_fundamental_ransac")
    out = RR.raw_ransac(case, launch, eight_point.workspace_sections, 9, ("Fh", 9), sets, flow_bwd, flow_fwd, offsets)
    n, hyp = out["info"].shape[0], out["counts"].shape[1]
    out.update(Fh=out.pop("table").reshape(n, hyp, 3, 3), F64=out.pop("est64").reshape(n, 3, 3), F32=out.pop("est32").reshape(n, 3, 3))
    return out


@functools.lru_cache(maxsize=None)
def result(key):
    """(case with its float64 composition, the kernels' outputs): computed once, shared, never changed."""
    case = EC.make_case(key)
    return case, raw_ransac(case)


@functools.lru_cache(maxsize=None)
def edge_result(name):
    """``result`` for a case of EC.EDGE_SEEDS."""
    case = EC.make_edge_case(name)
    return case, raw_ransac(case)


def rel_err(F, ref):
    return float((F - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("key", EC.SHAPES)
def test_votes_sets_and_info_equal_the_composition(key):
    case, out = result(key)
    RR._equal_decisions(out, case["comp"])
    assert torch.equal(out["info"][:, 1].long(), out["w1"].sum(1).long())       # the consensus is the winner's inlier set (>= 8)


@pytest.mark.parametrize("name", EC.EDGE_SHAPES)
def test_edge_votes_sets_and_info_equal_the_composition(name):
    case, out = edge_result(name)
    c, num = case["comp"], case["num"]
    RR._equal_decisions(out, c)
    info = out["info"].long()
    first, second = c["n1raw"] < 8, c["n2raw"] < 8
    assert torch.equal(info[~first, 1], out["w1"][~first].sum(1).long())        # a consensus is the winner's inlier set
    if EC.EDGE_SEEDS[name][2]:
        assert bool((first | second).any())
    else:
        assert not bool((first | second).any())
    assert bool((info[first, 1] < 8).all()) and bool((info[first, 2] == num).all()) and bool((out["w1"][first] == 1).all())
    assert torch.equal(out["w2"][second], out["w1"][second]) and torch.equal(info[second, 3], info[second, 2])
    if name == "both":
        assert first.tolist() == [True, False, False, False] and second.tolist() == [True, False, False, False]
    if name == "second":
        assert not bool(first.any()) and second.tolist() == [False, False, True, False]


@pytest.mark.parametrize("name", EC.EDGE_SHAPES)
def test_edge_f64_against_the_composition(name):
    case, out = edge_result(name)
    ref = case["comp"]["F"]
    assert bool(torch.isfinite(out["F64"]).all())
    y = EC.reference_spread(case)
    bound = max(F_BOUND, 16.0 * y)
    e = rel_err(out["F64"], ref)
    dist = min(float((ref[p] - case["F_true"][p]).abs().max() / case["F_true"][p].abs().max()) for p in range(ref.shape[0]))
    print("EBOUND eight_point F64 edge %s %s max|dF|/max|F| %.3e; y (eigh against svd, float64) %.3e bound %.3e; the composition's "
          "distance to F_true: min %.3e" % (name, _tag(EC.EDGE_SEEDS[name][0]), e, y, bound, dist))
    assert bound < dist                     # otherwise the case could not tell the estimate from the truth
    assert torch.equal(out["F32"], out["F64"].float())
    assert e <= bound, (e, bound)


def test_f64_against_the_composition_and_f32_is_its_rounding():
    worst, noisy_dist = 0.0, []
    for key in EC.SHAPES:
        case, out = result(key)
        ref = case["comp"]["F"]
        assert bool(torch.isfinite(out["F64"]).all())
        e = rel_err(out["F64"], ref)
        print("EBOUND eight_point F64 %s max|dF|/max|F| %.3e" % (_tag(key), e))
        worst = max(worst, e)
        assert torch.equal(out["F32"], out["F64"].float())                      # rounded once: bit equality
        if case["noisy"]:
            noisy_dist.extend(float((ref[p] - case["F_true"][p]).abs().max() / case["F_true"][p].abs().max()) for p in range(ref.shape[0]))
    print("EBOUND eight_point F64 all cases %.3e bound %.3e; the composition's distance to F_true on the noisy planes: min %.3e"
          % (worst, F_BOUND, min(noisy_dist)))
    assert F_BOUND < min(noisy_dist)        # otherwise the test could not tell the estimate from the truth
    assert worst <= F_BOUND, (worst, F_BOUND)


def test_tied_counts_go_to_the_lowest_index():
    RR.tied_counts_go_to_the_lowest_index(*result(EC.SHAPES[0]), raw_ransac, "F64")


@pytest.mark.parametrize("key", EC.SHAPES[1:3])
def test_properties_on_the_products_own_sets(key):
    """``minimal_sets_device``'s draw (with replacement: some sets repeat an index; such a hypothesis is ill-defined and CAN reach the
    maximum count -- test_drawn_sets_stage_by_stage holds the kernels to float64 there; this test only looks at the outcome):
    F[2,2] = 1, det F at rounding level, and no further from ``F_true`` than twice the composition on the same input."""
    from unsupervised_depth_opticalflow_egomotion_amd import eight_point
    case = EC.make_case(key)
    B, num = case["B"], case["num"]
    m = EC.solvers()
    sets = m.minimal_sets_device(B, num, torch.device("cuda"))
    assert tuple(sets.shape) == (B, 256, 8) and any(row.unique().numel() < 8 for row in sets.cpu().reshape(-1, 8))
    F32, F64, info = eight_point.fundamental_ransac(case["flow_bwd"].cuda(), case["flow_fwd"].cuda(), case["idx"].cuda(),
                                                    case["pick"].cuda(), sets)
    F64 = F64.cpu()
    comp = torch.cat([m.compute_fundmental_mat(case["matches"][:B].double()), m.compute_fundmental_mat(case["matches"][B:].double())], 0)
    assert bool((F64[:, 2, 2] == 1.0).all())
    scale = F64.abs().amax((1, 2))
    assert float((torch.det(F64).abs() / scale ** 3).max()) < 1e-12
    for p in range(2 * B):
        dist = lambda F: float((F[p] - case["F_true"][p]).abs().max())   # noqa: E731
        assert dist(F64) <= 2.0 * dist(comp), (p, dist(F64), dist(comp))
    assert int(info[:, 1].min()) >= 8


@pytest.mark.parametrize("scale", [1.0, 40.0])
def test_loss_and_gradient_against_float64(scale):
    """``scale`` = 40 puts most differences beyond smooth-L1's knee (|d| >= 1), 1 keeps them in the quadratic part."""
    _loss_against_float64(*result(EC.SHAPES[2]), scale)


@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("name", ["b1", "b3"])
def test_loss_and_gradient_at_one_sample_and_three(name, scale):
    _loss_against_float64(*edge_result(name), scale, tag=" " + name)


def _loss_against_float64(case, out, scale, tag=""):
    from unsupervised_depth_opticalflow_egomotion_amd import eight_point, ops
    B = case["B"]
    w = torch.tensor(WEIGHTS_OF[B])
    pose = EC.pose_vectors(case)
    pose[:, :, :3] *= scale
    l64, gpose64, gE64 = EC.loss_reference(out["F64"], case["K"], case["K_inv"], pose, w)
    Kc = G.Carved((B, 3, 3), offset_floats=1, fill=case["K"])
    Kic = G.Carved((B, 3, 3), offset_floats=3, fill=case["K_inv"])
    Fc = G.Carved((2 * B, 3, 3), offset_floats=2, fill=out["F32"])
    p = pose.cuda().requires_grad_(True)
    E = ops.PoseMatsFn.apply(p.reshape(2 * B, 6))[1]
    E.retain_grad()
    loss = eight_point.EightPointLossFn.apply(E, Kc.view, Kic.view, Fc.view)
    (loss * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert Kc.intact() and Kic.intact() and Fc.intact()
    el, eg, ee = RR.loss_errors(loss, l64, (p.grad, gpose64), (E.grad, gE64))
    print("EBOUND eight_point loss%s scale %g: loss %.3e (5e-6)  dpose %.3e  dE %.3e (2e-5)" % (tag, scale, el, eg, ee))
    assert el <= 5e-6 and eg <= 2e-5 and ee <= 2e-5


def test_loss_entry_points_in_guarded_buffers():
    _guarded_loss_entry_points([result(key) for key in EC.SHAPES[1:]])


def test_loss_entry_points_in_guarded_buffers_at_one_sample_and_three():
    _guarded_loss_entry_points([edge_result(name) for name in ("b1", "b3")])


def _guarded_loss_entry_points(results):
    from unsupervised_depth_opticalflow_egomotion_amd import _lib, eight_point, ops
    lib = _lib.get_lib()
    for case, out in results:
        B = case["B"]
        with torch.no_grad():
            E = ops.PoseMatsFn.apply(EC.pose_vectors(case).cuda().reshape(2 * B, 6))[1]
            Kt = eight_point.inverse_transposed(case["K"].cuda())
        ins = [G.Carved((2 * B, 9), offset_floats=1, fill=E), G.Carved((B, 9), offset_floats=2, fill=Kt),
               G.Carved((B, 9), offset_floats=3, fill=case["K_inv"]), G.Carved((2 * B, 9), offset_floats=0, fill=out["F32"])]
        st = _lib.stream_ptr()
        RR.guarded_loss_entry_points(B, ins, G.Carved((2 * B, 9), offset_floats=1), WEIGHTS_OF[B],
                                     lambda *a: _lib.check(lib.dfe_eight_point_loss_fwd(*a, B, st), "fwd"),
                                     lambda *a: _lib.check(lib.dfe_eight_point_loss_bwd(*a, B, st), "bwd"))
        assert float(torch.inverse(case["K"].double().permute(0, 2, 1)).sub(Kt.double().cpu()).abs().max()) < 1e-6


def test_refusals_come_before_any_launch():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib
    lib = _lib.get_lib()
    out = G.Carved((64,), offset_floats=0)
    x = torch.zeros(4096, device="cuda")
    p, o, st = P(x.data_ptr()), P(out.ptr), _lib.stream_ptr()

    def call(H, W, k, num, hyp):
        return lib.dfe_fundamental_ransac(p, p, p, p, p, o, o, o, o, 1, H, W, k, num, hyp, 0.1, st)
    assert call(8, 8, 16, 7, 4) == -2           # num = 7
    assert call(8, 8, 16, 8, 0) == -2           # hyp = 0
    assert call(8, 8, 65, 8, 4) == -2           # k > H*W
    assert call(8, 8, 16, 16385, 4) == -4 and call(8, 8, 16, 8, 4097) == -4
    assert lib.dfe_fundamental_ransac(None, p, p, p, p, o, o, o, o, 1, 8, 8, 16, 8, 4, 0.1, st) == -1
    assert lib.dfe_eight_point_loss_fwd(p, p, p, p, o, 0, st) == -2
    torch.cuda.synchronize()
    assert out.untouched() and out.intact()


def test_a_nan_in_one_samples_flow_poisons_that_sample_only():
    """Run once: NaN at a sampled pixel of sample 1's backward flow.  The call returns (every loop is bounded), sample 1's F of
    that direction and its loss are non-finite, sample 0 is untouched bit for bit."""
    from unsupervised_depth_opticalflow_egomotion_amd import eight_point, ops
    key = EC.SHAPES[1]
    case, out = result(key)
    B, H, W = case["B"], case["H"], case["W"]
    fb = case["flow_bwd"].clone()
    pix = int(case["idx"][1, case["pick"][3]])                      # plane d = 0, b = 1, match 3
    fb[1, 0].view(-1)[pix] = float("nan")
    bad = raw_ransac(case, flow_bwd=fb)
    assert not bool(torch.isfinite(bad["F64"][1]).all())
    for plane in (0, 2, 3):
        assert torch.equal(bad["F64"][plane], out["F64"][plane]), plane
    with torch.no_grad():
        E = ops.PoseMatsFn.apply(EC.pose_vectors(case).cuda().reshape(2 * B, 6))[1]
        loss = eight_point.EightPointLossFn.apply(E, case["K"].cuda(), case["K_inv"].cuda(), bad["F32"].cuda()).cpu()
        good = eight_point.EightPointLossFn.apply(E, case["K"].cuda(), case["K_inv"].cuda(), out["F32"].cuda()).cpu()
    assert not bool(torch.isfinite(loss[1])) and bool(torch.isfinite(loss[0])) and G.bits_equal(loss[0:1], good[0:1])


def test_two_runs_give_the_same_bits_and_the_wrapper_agrees():
    from unsupervised_depth_opticalflow_egomotion_amd import eight_point, ops
    key = EC.SHAPES[3]
    case, out = result(key)
    B = case["B"]
    again = raw_ransac(case, offsets=(3, 0, 1, 0))
    assert torch.equal(again["F64"], out["F64"]) and torch.equal(again["info"], out["info"]) and torch.equal(again["counts"], out["counts"])
    F32, F64, info = eight_point.fundamental_ransac(case["flow_bwd"].cuda(), case["flow_fwd"].cuda(), case["idx"].cuda(),
                                                    case["pick"].cuda(), case["sets"].cuda())
    assert torch.equal(F64.cpu(), out["F64"]) and G.bits_equal(F32, out["F32"]) and torch.equal(info.cpu(), out["info"])

    def loss_and_grad():
        E = ops.PoseMatsFn.apply(EC.pose_vectors(case).cuda().reshape(2 * B, 6))[1].detach().requires_grad_(True)
        loss = eight_point.EightPointLossFn.apply(E, case["K"].cuda(), case["K_inv"].cuda(), F32)
        loss.sum().backward()
        return loss.detach(), E.grad
    (l1, g1), (l2, g2) = loss_and_grad(), loss_and_grad()
    assert G.bits_equal(l1, l2) and G.bits_equal(g1, g2)
    with pytest.raises(ValueError):
        eight_point.fundamental_ransac(case["flow_bwd"].cuda(), case["flow_fwd"].cuda(), case["idx"].cuda(), case["pick"].cuda()[:7],
                                       case["sets"].cuda())


# ------------------------------------------------------------------------------------------------ the product's own draws
# ``pick`` and ``sets`` drawn with replacement (EC.build_drawn): about half the slots of the small shapes are ill-defined (their 8
# matches are not 8 distinct pixels, or the null direction of their normal matrix is not isolated) and the kernel may pick
# another vector of such a slot's null space than ``eigh`` does.  So the kernel is held to float64 stage by stage:
#   1  the counts of the well-defined slots equal the composition's;
#   2  an ill-defined slot's own F_h is non-finite with count 0, or a member of its null space (x2^T F x1 = 0 on its 8 matches,
#      det F = 0) at rounding level: 16 x what the reference's own ill-defined F_h leave on the same sets;
#   3  every slot's count is the float64 recount from the kernel's own F_h;
#   4  info, w1, w2 equal EC.continued(case, the kernel's table) and F64 is within the F bound of its F.
NULL_FACTOR = 16.0          # the factor F_BOUND uses


def null_space_bounds(case, sets, well, tag):
    """(res_bound, det_bound, fit_bound): NULL_FACTOR x the largest figures (EC.null_space_figures) of the REFERENCE's ill-defined
    hypotheses on the same sets, float64 on the CPU -- by either of its routes to the null vector, ``eigh`` of the normal matrix
    (the class's own) and ``svd`` of the design matrix, as EC.reference_spread takes both."""
    ill = ~well
    worst = [0.0, 0.0, 0.0]
    for table in (EC.composition(case["matches"], sets)["Fh"], EC.svd_route_hypotheses(case, sets)):
        figs = EC.null_space_figures(case, table, sets)
        assert all(bool(torch.isfinite(f[ill]).all()) for f in figs)
        worst = [max(w, float(f[ill].max())) for w, f in zip(worst, figs)]
    print("EBOUND eight_point null space %s reference's ill-defined slots: |x2'Fx1|/(max|F| s^2) %.3e  |det F|/max|F|^3 %.3e  "
          "null-space fit %.3e; bounds %.3e %.3e %.3e" % ((tag,) + tuple(worst) + tuple(NULL_FACTOR * w for w in worst)))
    return tuple(NULL_FACTOR * w for w in worst)


def check_ill_defined_slots(case, out, sets, well, tag, only=None):
    """Stage 2 on the ill-defined slots (``only``: a further mask)."""
    bounds = null_space_bounds(case, sets, well, tag)
    figs = EC.null_space_figures(case, out["Fh"], sets)
    ill = ~well if only is None else (~well & only)
    finite = torch.isfinite(out["Fh"]).all(3).all(2)
    dead = ill & ~finite
    assert bool((out["counts"][dead] == 0).all())
    live = ill & finite
    got = tuple(float(f[live].max()) if bool(live.any()) else 0.0 for f in figs)
    print("EBOUND eight_point null space %s kernel's ill-defined slots (%d finite, %d not): |x2'Fx1|/(max|F| s^2) %.3e  "
          "|det F|/max|F|^3 %.3e  null-space fit %.3e" % ((tag, int(live.sum()), int(dead.sum())) + got))
    assert all(g <= b for g, b in zip(got, bounds)), (got, bounds)


def stages(case, out, cont, sets, well, tag, only=None):
    """Stages 2 to 4 of a run on ``sets`` (``well``: EC.well_defined of them; ``only``: a further mask for stage 2)."""
    check_ill_defined_slots(case, out, sets, well, tag, only)
    RR.check_scoring(out, cont["err"], cont["err"] <= EC.THRESH * EC.THRESH, EC.THRESH, EC.MARGIN)
    check_consensus_and_estimate(case, out, cont, tag)


def check_consensus_and_estimate(case, out, cont, tag):
    """Stage 4."""
    assert EC.conclusive(cont), "inconclusive: margin %.3e, gaps %s %s" % (cont["margin"], cont["gap1"].tolist(), cont["gap2"].tolist())
    info = out["info"].long()
    assert torch.equal(info[:, 0], cont["best"]) and torch.equal(info[:, 1], cont["counts"].max(1)[0])
    assert torch.equal(out["w1"].long(), cont["w1"].long()) and torch.equal(out["w2"].long(), cont["w2"].long())
    assert torch.equal(info[:, 2], cont["w1"].sum(1).long()) and torch.equal(info[:, 3], cont["w2"].sum(1).long())
    assert bool(torch.isfinite(out["F64"]).all())
    y = EC.reference_spread(dict(matches=case["matches"], comp=cont))
    bound = max(F_BOUND, 16.0 * y)
    e = rel_err(out["F64"], cont["F"])
    print("EBOUND eight_point F64 %s against the composition continued from the kernel's table: max|dF|/max|F| %.3e; y %.3e "
           "bound %.3e" % (tag, e, y, bound))
    assert e <= bound, (e, bound)
    assert torch.equal(out["F32"], out["F64"].float())


@functools.lru_cache(maxsize=None)
def drawn_result(key):
    """``result`` for a case of EC.DRAWN_SEEDS, with the composition continued from the kernel's own table."""
    case = EC.make_drawn_case(key)
    out = raw_ransac(case)
    return case, out, EC.continued(case, out["Fh"])


@pytest.mark.parametrize("key", EC.DRAWN_SHAPES)
def test_drawn_sets_stage_by_stage(key):
    case, out, cont = drawn_result(key)
    RR.drawn_sets_stage_by_stage(case, out, cont, stages, key)
    ref = case["ref"]
    bound = max(F_BOUND, 16.0 * EC.reference_spread(dict(matches=case["matches"], comp=ref)))
    assert rel_err(out["F64"], ref["F"]) <= bound


def test_a_winner_with_repeated_matches_reaches_both_refits():
    case = EC.ill_winner_case()
    out = raw_ransac(case)
    RR.a_winner_with_repeated_matches(case, out, EC.continued(case, out["Fh"]), stages, 8)


def _crafted_run(slots, tag):
    """RR.crafted_run on the hyp = 70 drawn case, against its unmodified run."""
    case, base, _ = drawn_result(EC.DRAWN_SHAPES[1])
    return RR.crafted_run(EC, case, base, raw_ransac, stages, ("Fh",), ("F64", "F32"), slots, tag)


def test_degenerate_sets_stay_inside_their_own_slice():
    """Slots 0, 31, 32, 63, 64 and 69 (the ends of the hypothesis kernel's 32-thread blocks and of the scoring kernel's 64-slot
    LDS round) hold eight copies of one index, two indices four times, four indices twice.  No winner is among them: the
    estimate does not move."""
    RR.degenerate_sets_stay_inside_their_own_slice(drawn_result(EC.DRAWN_SHAPES[1])[1], _crafted_run, ("F64", "F32"))


def test_a_degenerate_set_in_the_winning_slot_hands_over_to_the_runner_up():
    RR.a_degenerate_winning_slot_hands_over_to_the_runner_up(drawn_result(EC.DRAWN_SHAPES[1])[1], _crafted_run)


def test_a_nan_match_leaves_its_hypotheses_without_a_vote():
    """Run once: NaN in sample 1's backward flow at the pixel of match 3.  In plane (d = 0, b = 1) every slot whose set holds a
    match of that pixel has a non-finite F_h and count 0 (stage 2's other branch), every other slot keeps its F_h bit for bit and
    its count is the float64 recount -- the NaN match votes for nobody -- and the other planes keep every count."""
    from unsupervised_depth_opticalflow_egomotion_amd.geometry_solvers import GeometrySolvers as S
    case, base, _ = drawn_result(EC.DRAWN_SHAPES[0])
    fb = case["flow_bwd"].clone()
    pix = int(case["idx"][1, case["pick"][3]])
    fb[1, 0].view(-1)[pix] = float("nan")
    bad = raw_ransac(case, flow_bwd=fb)
    holds = (case["pick"][case["sets"][1].long()] == case["pick"][3]).any(1)
    assert bool(holds.any()) and not bool(holds.all())
    finite = torch.isfinite(bad["Fh"][1]).all(2).all(1)
    assert not bool(finite[holds].any()) and bool((bad["counts"][1, holds] == 0).all())
    assert torch.equal(_bits(bad["Fh"][1, ~holds]), _bits(base["Fh"][1, ~holds]))
    m = EC.matches_of(case, flow_bwd=fb).double()[1:2]
    err = S._epipolar_residual(bad["Fh"][1:2], m)[0]
    t = EC.THRESH * EC.THRESH
    ok = torch.isfinite(err)
    assert not bool((ok & ((err - t).abs() / t < EC.MARGIN)).any()), "inconclusive: a residual within MARGIN of the threshold"
    assert torch.equal(bad["counts"][1].long(), (ok & (err <= t)).sum(1))
    for plane in (0, 2, 3):
        assert torch.equal(bad["counts"][plane], base["counts"][plane]) and torch.equal(_bits(bad["F64"][plane]), _bits(base["F64"][plane]))
