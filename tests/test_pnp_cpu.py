"""CPU: the PnP term's host side -- the case helper's conditions, the switch's default and round trip, the cached minimal sets of
both sizes, and the new entry points' declarations."""
import ctypes

import pytest
import torch

from tests import pnp_cases as PC
from tests import ransac_cases as RC


def _shape_checks(case, key):
    B, H, W, k, num, hyp, noisy = key
    assert case["idx"].dtype == torch.int32 and tuple(case["idx"].shape) == (2 * B, k)
    assert bool((case["idx"][:, 1:] > case["idx"][:, :-1]).all()) and int(case["idx"].max()) < H * W
    assert case["pick"].dtype == torch.int64 and case["pick"].unique().numel() == num and int(case["pick"].max()) < k
    s = case["sets"]
    assert s.dtype == torch.int32 and tuple(s.shape) == (B, hyp, 6) and int(s.min()) >= 0 and int(s.max()) < num
    assert all(row.unique().numel() == 6 for row in s.reshape(-1, 6))                 # duplicate-free
    assert tuple(case["disp_t"].shape) == (B, 1, H, W) and float(case["disp_t"].min()) >= 2.0 and float(case["disp_t"].max()) <= 20.0
    assert not torch.equal(case["K"][0], case["K"][1])                                # per-sample K
    f = case["figures"]
    assert f["api_equal"] and f["margin"] >= PC.MARGIN and f["zmargin"] >= PC.MARGIN and f["route_free"] and f["same_set"]


@pytest.mark.parametrize("key", PC.SHAPES)
def test_the_cases_meet_their_conditions(key):
    case = PC.make_case(key)                                       # asserts the conditions itself
    _shape_checks(case, key)
    num, noisy = key[4], key[6]
    c = case["comp"]
    assert case["figures"]["consensus"] >= 6
    share = 1.0 - c["w2"].sum(1) / num                              # some matches are left out (the gross outliers), most are kept
    assert float(share.min()) > 0.0 and float(share.max()) < 0.7
    # the refined pose against the analytic one: fp32 inputs without noise, the noise's level with it
    dist = float((c["P"] - case["P_true"]).abs().max())
    assert dist < (2e-2 if noisy else 2e-6), dist


def test_the_fallback_case_needs_the_fallback():
    case = PC.fallback_case()
    _shape_checks(case, PC.FALLBACK[0])
    c = case["comp"]
    few = c["n1raw"] < 6
    assert bool(few.any()) and bool((c["w1"][few] == 1).all()) and bool((c["n2raw"][few] >= 6).all())


def test_the_last_shape_crosses_both_tiles():
    key = PC.SHAPES[-1]
    num, hyp = key[4], key[5]
    assert num > PC.MATCH_TILE and num % PC.MATCH_TILE != 0 and hyp > PC.HYP_TILE and hyp % PC.HYP_TILE != 0


def test_the_switch_is_off_by_default_and_round_trips():
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import DEFAULT_CFG, make_cfg
    assert make_cfg().enable_pnp is False and DEFAULT_CFG["enable_pnp"] is False
    cfg = make_cfg(enable_pnp=True, w_pnp=0.25)
    assert cfg.enable_pnp is True and cfg.w_pnp == 0.25 and cfg.enable_triangle is False and cfg.enable_eight_point is False
    from unsupervised_depth_opticalflow_egomotion_amd.models import Model_geometry
    assert Model_geometry(cfg).enable_pnp is True and Model_geometry(make_cfg()).enable_pnp is False


def test_the_cached_device_sets_of_six_are_the_draw_of_minimal_sets():
    m = PC.solvers()
    m.ransac_iters, m.ransac_seed = 19, 5
    want = m._minimal_sets(3, 50, 6, "cpu")
    got = m.minimal_sets_device(3, 50, torch.device("cpu"), k=6)
    assert got.dtype == torch.int32 and got.is_contiguous() and tuple(got.shape) == (3, 19, 6) and torch.equal(got.long(), want)
    assert m.minimal_sets_device(3, 50, torch.device("cpu"), k=6) is got                 # held, not drawn again
    # the default is the eight-point term's draw, unchanged, and a cache entry of its own
    eight = m.minimal_sets_device(3, 50, torch.device("cpu"))
    assert eight is not got and tuple(eight.shape) == (3, 19, 8) and torch.equal(eight.long(), m._minimal_sets(3, 50, 8, "cpu"))
    assert m.minimal_sets_device(3, 50, torch.device("cpu"), k=8) is eight
    m.ransac_seed = 6                                                                     # another seed, another draw
    other = m.minimal_sets_device(3, 50, torch.device("cpu"), k=6)
    assert other is not got and torch.equal(other.long(), m._minimal_sets(3, 50, 6, "cpu"))


def test_the_header_declares_the_new_entries():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib, pnp
    sigs = _lib.header_signatures()
    I, L, P, D, F = ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_double, ctypes.c_float
    want = {
        "dfe_pnp_ws_bytes": (L, [I, I, I]),
        "dfe_pnp_ransac": (I, [P] * 12 + [I] * 7 + [D, P]),
        "dfe_pnp_loss_fwd": (I, [P] * 3 + [I, F, P]),
        "dfe_pnp_loss_bwd": (I, [P] * 4 + [I, F, P]),
    }
    lib = _lib.get_lib()
    for name, (res, args) in want.items():
        assert sigs[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _lib.header_abi_version() == 4                              # new symbols only
    # the host-only query answers without a device, and the documented sections add up to it
    for B, num, hyp in ((4, 6000, 256), (2, 70, 33), (1, 6, 1)):
        sec = pnp.workspace_sections(B, num, hyp)
        assert lib.dfe_pnp_ws_bytes(B, num, hyp) == sec["bytes"]
        assert all(sec[n] % 16 == 0 for n in sec)
    assert lib.dfe_pnp_ws_bytes(0, 6, 6) == 0


def test_the_new_keyword_leaves_the_existing_cases_bits():
    """``rot`` defaults to the former constant; SHAPES and FALLBACK keep their entries; the generator-only tensors of every
    existing case (the camera matrices: the first draws; idx, pick and sets: the last) carry the checksums taken before the
    keyword existed, and the default equals the explicit 0.02 in every tensor."""
    import inspect
    assert inspect.signature(PC.build).parameters["rot"].default == 0.02
    want = {(2, 12, 20, 72, 64, 32, False): (0, 2477022648), (2, 12, 20, 72, 64, 32, True): (0, 2812100972),
            (2, 13, 19, 72, 70, 33, True): (0, 4139742225), (2, 20, 24, 320, 300, 70, True): (0, 998629082)}
    assert PC.SHAPES == tuple(sorted(want)) and PC.SEEDS == {k: v[0] for k, v in want.items()}
    assert PC.FALLBACK == ((2, 13, 19, 72, 70, 33, True), 1)
    for key, (seed, crc) in want.items():
        case = PC.build(seed, *key)
        assert RC.crc(case, ("K", "idx", "pick", "sets")) == crc, key
        explicit = PC.build(seed, *key, rot=0.02)
        assert all(torch.equal(case[n], explicit[n]) for n in case if torch.is_tensor(case[n]))


@pytest.mark.parametrize("name", PC.EDGE_SHAPES)
def test_the_edge_cases_meet_their_conditions(name):
    (B, H, W, k, num, hyp, noisy), seed, fallback, rot = PC.EDGE_SEEDS[name]
    case = PC.make_edge_case(name)                                  # asserts (a)-(d), and (e) or "some plane falls back"
    f, c = case["figures"], case["comp"]
    assert f["api_equal"] and f["margin"] >= PC.MARGIN and f["zmargin"] >= PC.MARGIN and f["route_free"] and f["same_set"]
    assert PC.well_conditioned(f, fallback) and not PC.well_conditioned(f, not fallback)
    assert case["idx"].dtype == torch.int32 and tuple(case["idx"].shape) == (2 * B, k)
    assert case["pick"].unique().numel() == num and tuple(case["sets"].shape) == (B, hyp, 6)
    assert all(row.unique().numel() == 6 for row in case["sets"].reshape(-1, 6))
    first, second = (c["n1raw"] < 6).tolist(), (c["n2raw"] < 6).tolist()
    norms = c["P"][:, 3:].norm(dim=1)
    y = ((PC.composition_of(case, case["x"], case["X"], iterations=2 * PC.ITERS)["P"] - c["P"]).abs().amax(1) / c["P"].abs().amax(1))
    tiles = "num %d = %g match tiles, hyp %d = %g hypothesis tiles" % (num, num / PC.MATCH_TILE, hyp, hyp / PC.HYP_TILE)
    print("EDGE pnp %s seed %d: n1raw %s n2raw %s; first fall-back on planes %s, second on %s; %s; axis-angle norms %.3e to %.3e; "
          "y per plane %s" % (name, seed, [int(v) for v in c["n1raw"]], [int(v) for v in c["n2raw"]],
                              [p for p, v in enumerate(first) if v], [p for p, v in enumerate(second) if v], tiles,
                              float(norms.min()), float(norms.max()), ["%.2e" % float(v) for v in y]))
    if name == "zero":
        assert first == [True, False, True, False] and second == first
        for plane in (0, 2):                                        # not one vote: argmax of zeros is slot 0
            assert int(c["counts"][plane].max()) == 0 and int(c["best"][plane]) == 0
            assert bool((c["w1"][plane] == 1).all()) and bool((c["w2"][plane] == 1).all())
    else:
        assert f["consensus"] >= 6 and not any(first) and not any(second)
    if name == "rot0.3":
        assert float(norms.min()) > 0.1 and float(norms.max()) < 0.6 and float(case["P_true"][:, 3:].norm(dim=1).max()) > 0.3
    if name == "rot0":                                              # so3_log's series branch (th <= 1e-6)
        assert float(norms.max()) < 1e-6 and float(case["P_true"][:, 3:].abs().max()) == 0.0
        assert float((c["P"] - case["P_true"]).abs().max()) < 2e-6
    if name == "tiles":
        assert num == PC.MATCH_TILE and hyp == 2 * PC.HYP_TILE
    if name in ("b1", "b3"):
        assert B == int(name[1]) and tuple(c["P"].shape) == (2 * B, 6)


@pytest.mark.parametrize("key", PC.DRAWN_SHAPES)
def test_the_drawn_cases_meet_their_conditions(key):
    case = PC.make_drawn_case(key)                                  # asserts the conditions itself
    B, H, W, k, num, hyp, noisy = key
    RC.drawn_layout(6, case, key)
    f, c, well = case["figures"], case["comp"], case["well"]
    assert f["api_equal"] and 4 * f["n_well"] >= hyp and f["n_ill"] >= 4 and f["margin"] >= PC.MARGIN and f["zmargin"] >= PC.MARGIN
    assert f["route_free"] and f["consensus"] >= 6 and f["cond"] >= PC.LM_COND
    # ``winner_well`` and ``lead`` rest on counts that the host's LAPACK decides: printed, not asserted.  What every host agrees on
    # is the composition without the ill-defined slots
    ref = case["ref"]
    top = c["counts"].max(1)[0]
    assert PC.conclusive(ref) and bool(torch.gather(well, 1, ref["best"].view(-1, 1)).all())
    assert torch.equal(ref["counts"][well], c["counts"][well]) and int(ref["counts"][~well].max()) == 0
    print("DRAWN pnp winner well-defined %s lead %d (this host's LAPACK)" % (f["winner_well"].tolist(), f["lead"]))
    print("DRAWN pnp %s seed %d: well-defined slots per plane %s of %d; winner's count %s, best ill-defined count %s; margin %.3e"
          % ("x".join(str(int(v)) for v in key), PC.DRAWN_SEEDS[key], well.sum(1).tolist(), hyp, top.tolist(),
             [int(c["counts"][p][~well[p]].max()) for p in range(2 * B)], f["margin"]))


def test_the_drawn_shapes_are_the_ones_the_slots_need():
    assert PC.DRAWN_SHAPES == ((2, 12, 20, 72, 64, 64, True), (2, 20, 24, 320, 300, 70, True), (3, 13, 19, 72, 70, 33, True))
    num, hyp = PC.DRAWN_SHAPES[1][4], PC.DRAWN_SHAPES[1][5]
    assert max(PC.CRAFTED_SLOTS) == hyp - 1 and {0, 31, 32, 63, 64} < set(PC.CRAFTED_SLOTS) and hyp > PC.HYP_TILE
    assert len(set(PC.COINCIDENT)) == 6 and max(PC.COINCIDENT) < num


def test_the_ill_winner_case_meets_its_conditions():
    case = PC.ill_winner_case()
    key, seed = PC.ILL_WINNER
    RC.drawn_layout(6, case, key)
    f, c, well = case["figures"], case["comp"], case["well"]
    won = ~torch.gather(well, 1, c["best"].view(-1, 1)).squeeze(1)           # this host's LAPACK decides: printed, not asserted
    assert f["consensus"] >= 6 and "ref" not in case
    print("DRAWN pnp ill-defined winner seed %d: planes %s, counts %s" % (seed, won.nonzero().flatten().tolist(), c["counts"].max(1)[0].tolist()))


def test_continued_from_the_references_own_table_is_the_composition():
    """Bit for bit, every entry: ``continued`` is the composition's own code after the table."""
    cases = [PC.make_case(key) for key in PC.SHAPES] + [PC.make_drawn_case(key) for key in PC.DRAWN_SHAPES]
    cases += [PC.ill_winner_case(), PC.fallback_case(), PC.make_edge_case("zero")]     # through both fall-backs as well
    for case in cases:
        c = case["comp"]
        k = PC.continued(case, c["Rh"], c["Th"])
        for name in c:
            a, b = c[name], k[name]
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                                      b.view(torch.int64) if b.dtype == torch.float64 else b), name


def test_continued_follows_the_table_it_is_given():
    """Another table, another winner: with the reference's winning slot of plane 0 made non-finite the runner-up takes over."""
    case = PC.make_drawn_case(PC.DRAWN_SHAPES[0])
    c = case["comp"]
    Rh = c["Rh"].clone()
    best = int(c["best"][0])
    Rh[0, best] = float("nan")
    k = PC.continued(case, Rh, c["Th"])
    counts = c["counts"][0].clone()
    counts[best] = -1
    assert int(k["counts"][0, best]) == 0 and int(k["best"][0]) == int(counts.argmax())
    assert torch.equal(k["P"][1:], c["P"][1:]) and PC.conclusive(PC.continued(case, c["Rh"], c["Th"]))


def test_the_crafted_sets_are_degenerate_and_in_range():
    case = dict(PC.make_drawn_case(PC.DRAWN_SHAPES[1]))
    before = case["pick"]
    case["pick"] = PC.coincident_pick(case)
    assert case["pick"][list(PC.COINCIDENT)].unique().numel() == 1 and int((case["pick"] != before).sum()) <= 5
    sets = PC.crafted_sets(case)
    assert int(sets.min()) >= 0 and int(sets.max()) < case["num"] and torch.equal(sets[1], case["sets"][1])
    assert [sets[0, s].unique().numel() for s in PC.CRAFTED_SLOTS] == [1, 2, 3, 6, 1, 2]
    assert not bool(PC.distinct_pixels(case, sets)[0, list(PC.CRAFTED_SLOTS)].any())   # the fourth kind: six matches, one pixel
    well = PC.well_defined(case, sets)
    B = case["B"]
    assert not bool(well[0, list(PC.CRAFTED_SLOTS)].any()) and not bool(well[B, list(PC.CRAFTED_SLOTS)].any())
    x, X = PC.points_of(case)
    assert float((X[0, list(PC.COINCIDENT)] - X[0, PC.COINCIDENT[0]]).abs().max()) == 0.0          # coincident 3-D points
    comp = PC.composition_of(case, x, X, sets=sets)
    orth, det = PC.rotation_figures(comp["Rh"])                     # the reference itself leaves a rotation there
    assert float(orth[0, list(PC.CRAFTED_SLOTS)].max()) < 1e-12 and float(det[0, list(PC.CRAFTED_SLOTS)].max()) < 1e-12


@pytest.mark.parametrize("B", [2, 3])
def test_the_model_scene_tells_the_plane_and_row_orderings_apart(B):
    """tests/test_hip_pnp_model.py's scene, float64 on the CPU with the analytic pose as the target: exchanging the two directions'
    targets (plane d*B + b read as (1-d)*B + b), or reading the pose's row d*B + b for (b, d), moves some sample's loss by more
    than 100 x the loss tolerance; and the samples' cameras differ, so ``K[0]`` for every sample is not ``K[b]``."""
    WEIGHTS_OF, _loss_reference = PC.WEIGHTS_OF, PC.loss_reference
    case = PC.build(0, B, 12, 20, 72, 64, 64, True)
    w = torch.tensor(WEIGHTS_OF[B])
    pose, target = PC.pose_vectors(case), case["P_true"]
    base = _loss_reference(target, pose, 0.5, w)[0]
    swapped = _loss_reference(torch.cat([target[B:], target[:B]], 0), pose, 0.5, w)[0]
    rows = _loss_reference(target, pose.reshape(2, B, 6).permute(1, 0, 2).contiguous(), 0.5, w)[0]
    assert float(((swapped - base).abs() / base).max()) > 100 * 5e-6 and float(((rows - base).abs() / base).max()) > 100 * 5e-6
    assert all(float((case["K"][b] - case["K"][0]).abs().max()) > 1e-2 for b in range(1, B))
