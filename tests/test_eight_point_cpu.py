"""CPU: the eight-point term's host side -- the case helper's conditions, the switch's default and round trip, the cached minimal
sets, and the new entry points' declarations."""
import ctypes

import pytest
import torch

from tests import eight_point_cases as EC
from tests import ransac_cases as RC


@pytest.mark.parametrize("key", EC.SHAPES)
def test_the_cases_meet_their_conditions(key):
    case = EC.make_case(key)                                       # asserts the conditions itself
    B, H, W, k, num, hyp, noisy = key
    f = case["figures"]
    assert f["api_equal"] and f["margin"] >= EC.MARGIN and f["same_set"] and f["consensus"] >= 8 and f["gap"] >= EC.GAP and f["sep"] >= 1e-7
    assert case["idx"].dtype == torch.int32 and tuple(case["idx"].shape) == (2 * B, k)
    assert bool((case["idx"][:, 1:] > case["idx"][:, :-1]).all()) and int(case["idx"].max()) < H * W
    assert case["pick"].dtype == torch.int64 and case["pick"].unique().numel() == num and int(case["pick"].max()) < k
    s = case["sets"]
    assert s.dtype == torch.int32 and tuple(s.shape) == (B, hyp, 8) and int(s.min()) >= 0 and int(s.max()) < num
    assert all(row.unique().numel() == 8 for row in s.reshape(-1, 8))                 # duplicate-free
    c = case["comp"]
    share = 1.0 - c["w2"].sum(1) / num                              # some matches are left out, most are kept
    assert float(share.min()) > 0.0 and float(share.max()) < 0.7
    assert bool((c["F"][:, 2, 2] == 1.0).all())


def test_the_third_shape_crosses_both_tiles():
    key = EC.SHAPES[-1]
    num, hyp = key[4], key[5]
    assert num > EC.MATCH_TILE and num % EC.MATCH_TILE != 0 and hyp > EC.HYP_TILE and hyp % EC.HYP_TILE != 0


def test_the_switch_is_off_by_default_and_round_trips():
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import DEFAULT_CFG, make_cfg
    assert make_cfg().enable_eight_point is False and DEFAULT_CFG["enable_eight_point"] is False
    cfg = make_cfg(enable_eight_point=True, w_8point=0.25)
    assert cfg.enable_eight_point is True and cfg.w_8point == 0.25 and cfg.enable_triangle is False


def test_the_cached_device_sets_are_the_draw_of_minimal_sets():
    m = EC.solvers()
    m.ransac_iters, m.ransac_seed = 19, 5
    want = m._minimal_sets(3, 50, 8, "cpu")
    got = m.minimal_sets_device(3, 50, torch.device("cpu"))
    assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got.long(), want)
    assert m.minimal_sets_device(3, 50, torch.device("cpu")) is got                      # held, not drawn again
    assert m.minimal_sets_device(3, 51, torch.device("cpu")) is not got
    m.ransac_seed = 6                                                                     # another seed, another draw
    other = m.minimal_sets_device(3, 50, torch.device("cpu"))
    assert other is not got and torch.equal(other.long(), m._minimal_sets(3, 50, 8, "cpu"))


def test_lmeds_is_refused_with_the_switch_on():
    from unsupervised_depth_opticalflow_egomotion_amd._lib import DfeError
    from unsupervised_depth_opticalflow_egomotion_amd.models import Model_geometry
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg
    with pytest.raises(DfeError, match="FM_RANSAC only"):
        Model_geometry(make_cfg(enable_eight_point=True, dataset="nyuv2"))


def test_the_header_declares_the_new_entries():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib, eight_point
    sigs = _lib.header_signatures()
    I, L, P, D = ctypes.c_int, ctypes.c_long, ctypes.c_void_p, ctypes.c_double
    want = {
        "dfe_eight_point_ws_bytes": (L, [I, I, I]),
        "dfe_fundamental_ransac": (I, [P] * 9 + [I] * 6 + [D, P]),
        "dfe_eight_point_loss_fwd": (I, [P] * 5 + [I, P]),
        "dfe_eight_point_loss_bwd": (I, [P] * 6 + [I, P]),
    }
    lib = _lib.get_lib()
    for name, (res, args) in want.items():
        assert sigs[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _lib.header_abi_version() == 4                              # new symbols only
    # the host-only query answers without a device, and the documented sections add up to it
    for B, num, hyp in ((4, 6000, 256), (2, 70, 33), (1, 8, 1)):
        sec = eight_point.workspace_sections(B, num, hyp)
        assert lib.dfe_eight_point_ws_bytes(B, num, hyp) == sec["bytes"]
        assert all(sec[n] % 16 == 0 for n in sec)
    assert lib.dfe_eight_point_ws_bytes(0, 8, 8) == 0


def test_the_existing_tables_and_their_draws_are_unchanged():
    """SHAPES keeps its four keys in their places, and the generator-only tensors of every existing case (the camera matrices:
    the first draws; idx, pick and sets: the last) carry the checksums taken before the edge table existed."""
    want = {(2, 12, 20, 72, 64, 32, False): (0, 2623675490), (2, 12, 20, 72, 64, 32, True): (1, 2804939302),
            (2, 13, 19, 72, 70, 33, True): (0, 3405646239), (2, 20, 24, 320, 300, 70, True): (1, 2126196865)}
    assert EC.SHAPES == tuple(sorted(want)) and EC.SEEDS == {k: v[0] for k, v in want.items()}
    for key, (seed, crc) in want.items():
        assert RC.crc(EC.build(seed, *key), ("K", "idx", "pick", "sets")) == crc, key


@pytest.mark.parametrize("name", EC.EDGE_SHAPES)
def test_the_edge_cases_meet_their_conditions(name):
    (B, H, W, k, num, hyp, noisy), seed, fallback = EC.EDGE_SEEDS[name]
    case = EC.make_edge_case(name)                                  # asserts the conditions itself
    f, c = case["figures"], case["comp"]
    assert f["api_equal"] and f["margin"] >= EC.MARGIN and f["same_set"] and f["gap"] >= EC.GAP and f["sep"] >= 1e-7
    assert EC.well_conditioned(f, fallback) and not EC.well_conditioned(f, not fallback)
    assert case["idx"].dtype == torch.int32 and tuple(case["idx"].shape) == (2 * B, k)
    assert case["pick"].unique().numel() == num and tuple(case["sets"].shape) == (B, hyp, 8)
    assert all(row.unique().numel() == 8 for row in case["sets"].reshape(-1, 8))
    first, second = (c["n1raw"] < 8).tolist(), (c["n2raw"] < 8).tolist()
    tiles = "num %d = %g match tiles, hyp %d = %g hypothesis tiles" % (num, num / EC.MATCH_TILE, hyp, hyp / EC.HYP_TILE)
    print("EDGE eight_point %s seed %d: n1raw %s n2raw %s; first fall-back on planes %s, second on %s; %s; y %.3e"
          % (name, seed, [int(v) for v in c["n1raw"]], [int(v) for v in c["n2raw"]], [p for p, v in enumerate(first) if v],
             [p for p, v in enumerate(second) if v], tiles, EC.reference_spread(case)))
    if name == "both":
        assert first == [True, False, False, False] and second == [True, False, False, False]
        assert bool((c["w1"][0] == 1).all()) and torch.equal(c["w2"][0], c["w1"][0])
    elif name == "second":
        assert first == [False] * 4 and second == [False, False, True, False] and torch.equal(c["w2"][2], c["w1"][2])
        assert not bool((c["w1"][2] == 1).all())                   # the kept set is a proper consensus, not "all matches"
    else:
        assert f["consensus"] >= 8 and not any(first) and not any(second)
    if name == "tiles":
        assert num == EC.MATCH_TILE and hyp == 2 * EC.HYP_TILE
    if name in ("b1", "b3"):
        assert B == int(name[1]) and tuple(c["F"].shape) == (2 * B, 3, 3)
    assert bool((c["F"][:, 2, 2] == 1.0).all())


def test_the_reference_spread_is_rounding_noise_on_the_existing_cases():
    """y of the F bound: ``eigh`` of the normal matrix against ``svd`` of the design matrix, both float64.  On the isolated null
    directions the helper asserts it stays orders below the distance to the truth."""
    for key in EC.SHAPES:
        y = EC.reference_spread(EC.make_case(key))
        assert 0.0 <= y < 1e-9, (key, y)


def _drawn_layout(case, key):
    RC.drawn_layout(8, case, key)
    assert any(row.unique().numel() < 8 for row in case["sets"].reshape(-1, 8))


@pytest.mark.parametrize("key", EC.DRAWN_SHAPES)
def test_the_drawn_cases_meet_their_conditions(key):
    case = EC.make_drawn_case(key)                                  # asserts the conditions itself
    B, H, W, k, num, hyp, noisy = key
    _drawn_layout(case, key)
    f, c, well = case["figures"], case["comp"], case["well"]
    assert f["api_equal"] and 4 * f["n_well"] >= hyp and f["n_ill"] >= 4 and f["margin"] >= EC.MARGIN
    assert f["consensus"] >= 8 and f["gap"] >= EC.GAP and f["sep"] >= 1e-7
    # ``winner_well`` and ``lead`` rest on counts that the host's LAPACK decides: printed, not asserted.  What every host agrees on
    # is the composition without the ill-defined slots
    ref = case["ref"]
    top = c["counts"].max(1)[0]
    assert EC.conclusive(ref) and bool(torch.gather(well, 1, ref["best"].view(-1, 1)).all())
    assert torch.equal(ref["counts"][well], c["counts"][well]) and int(ref["counts"][~well].max()) == 0
    print("DRAWN eight_point winner well-defined %s lead %d (this host's LAPACK)" % (f["winner_well"].tolist(), f["lead"]))
    print("DRAWN eight_point %s seed %d: well-defined slots per plane %s of %d; winner's count %s, best ill-defined count %s; margin %.3e"
          % ("x".join(str(int(v)) for v in key), EC.DRAWN_SEEDS[key], well.sum(1).tolist(), hyp, top.tolist(),
             [int(c["counts"][p][~well[p]].max()) for p in range(2 * B)], f["margin"]))
    assert bool((c["F"][:, 2, 2] == 1.0).all())


def test_the_drawn_shapes_are_the_ones_the_slots_need():
    assert EC.DRAWN_SHAPES == ((2, 12, 20, 72, 64, 64, True), (2, 20, 24, 320, 300, 70, True), (3, 13, 19, 72, 70, 33, True))
    hyp = EC.DRAWN_SHAPES[1][5]
    assert max(EC.CRAFTED_SLOTS) == hyp - 1 and {0, 31, 32, 63, 64} < set(EC.CRAFTED_SLOTS) and hyp > EC.HYP_TILE


def test_the_ill_winner_case_meets_its_conditions():
    case = EC.ill_winner_case()
    key, seed = EC.ILL_WINNER
    _drawn_layout(case, key)
    f, c, well = case["figures"], case["comp"], case["well"]
    won = ~torch.gather(well, 1, c["best"].view(-1, 1)).squeeze(1)           # this host's LAPACK decides: printed, not asserted
    assert f["consensus"] >= 8 and "ref" not in case
    print("DRAWN eight_point ill-defined winner seed %d: planes %s, counts %s" % (seed, won.nonzero().flatten().tolist(), c["counts"].max(1)[0].tolist()))


def test_continued_from_the_references_own_table_is_the_composition():
    """Bit for bit, every entry: ``continued`` is the composition's own code after the table."""
    cases = [EC.make_case(key) for key in EC.SHAPES] + [EC.make_drawn_case(key) for key in EC.DRAWN_SHAPES] + [EC.ill_winner_case()]
    cases += [EC.make_edge_case(name) for name in ("both", "second")]                  # through both fall-backs as well
    for case in cases:
        c = case["comp"]
        k = EC.continued(case, c["Fh"])
        for name in c:
            a, b = c[name], k[name]
            assert a.dtype == b.dtype and torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                                      b.view(torch.int64) if b.dtype == torch.float64 else b), name
        assert k["margin"] <= min(EC.rel_margin(c[n]) for n in ("e1", "e2"))


def test_continued_follows_the_table_it_is_given():
    """Another table, another winner: with the reference's winning slot of plane 0 made non-finite the runner-up takes over, and
    the margin and the isolation figures are those of the new consensus."""
    case = EC.make_drawn_case(EC.DRAWN_SHAPES[0])
    c = case["comp"]
    Fh = c["Fh"].clone()
    best = int(c["best"][0])
    Fh[0, best] = float("nan")
    k = EC.continued(case, Fh)
    counts = c["counts"][0].clone()
    counts[best] = -1
    assert int(k["counts"][0, best]) == 0 and int(k["best"][0]) == int(counts.argmax())
    assert torch.equal(k["F"][1:], c["F"][1:]) and EC.conclusive(EC.continued(case, c["Fh"]))


def test_the_crafted_sets_are_degenerate_and_in_range():
    case = EC.make_drawn_case(EC.DRAWN_SHAPES[1])
    sets = EC.crafted_sets(case)
    assert int(sets.min()) >= 0 and int(sets.max()) < case["num"] and torch.equal(sets[1], case["sets"][1])
    kinds = [sets[0, s].unique().numel() for s in EC.CRAFTED_SLOTS]
    assert kinds == [1, 2, 4, 1, 2, 4]
    well = EC.well_defined(case, sets)
    B = case["B"]
    assert not bool(well[0, list(EC.CRAFTED_SLOTS)].any()) and not bool(well[B, list(EC.CRAFTED_SLOTS)].any())
    other = [s for s in range(case["hyp"]) if s not in EC.CRAFTED_SLOTS]
    assert torch.equal(sets[0, other], case["sets"][0, other]) and torch.equal(well[:, other], case["well"][:, other])
    # the reference itself leaves a valid member of the null space there: finite, det F = 0 at rounding level
    ref = EC.composition(case["matches"], sets)["Fh"]
    res, det, fit = EC.null_space_figures(case, ref, sets)
    assert bool(torch.isfinite(res).all()) and float(det[0, list(EC.CRAFTED_SLOTS)].max()) < 1e-12
    assert float(fit[0, list(EC.CRAFTED_SLOTS)].max()) < 1e-10
    # fit has teeth where res has none: a rank-2 matrix that is no member of the null space (another slot's F_h) is of order 1
    shifted = torch.roll(case["comp"]["Fh"], 1, 1)
    well = case["well"]
    assert float(EC.null_space_figures(case, case["comp"]["Fh"])[2][well].max()) < 1e-10
    assert float(EC.null_space_figures(case, shifted)[2][well].median()) > 1e-3


@pytest.mark.parametrize("B", [2, 3])
def test_the_model_scene_tells_the_plane_and_row_orderings_apart(B):
    """tests/test_hip_eight_point_model.py's scene, float64 on the CPU with the analytic F as the target: exchanging the two
    directions' targets (plane d*B + b read as (1-d)*B + b), or reading E's row d*B + b for (b, d), moves some sample's loss by
    more than 100 x the loss tolerance, at the translation scale 40 the test uses."""
    WEIGHTS_OF, _loss_reference = EC.WEIGHTS_OF, EC.loss_reference
    case = EC.build(0, B, 12, 20, 72, 64, 64, True)
    w = torch.tensor(WEIGHTS_OF[B])
    F = case["F_true"]

    def moves(scale):
        pose = EC.pose_vectors(case)
        pose[:, :, :3] *= scale
        base = _loss_reference(F, case["K"], case["K_inv"], pose, w)[0]
        swapped = _loss_reference(torch.cat([F[B:], F[:B]], 0), case["K"], case["K_inv"], pose, w)[0]
        rows = _loss_reference(F, case["K"], case["K_inv"], pose.reshape(2, B, 6).permute(1, 0, 2).contiguous(), w)[0]
        return float(((swapped - base).abs() / base).max()), float(((rows - base).abs() / base).max())
    swap, rows = moves(40.0)
    assert swap > 100 * 5e-6 and rows > 100 * 5e-6, (swap, rows)
    assert tuple(case["disp_t"].shape) == (B, 1, 12, 20) and float(case["disp_t"].min()) >= 2.0 and float(case["disp_t"].max()) <= 20.0
