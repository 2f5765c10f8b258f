"""CPU: the eight-point epipolar map's switch, header entries, torch composition and the conditions of its cases
(tests/epipolar_cases.py)."""
import ctypes

import pytest
import torch

from tests import eight_point_cases as EC
from tests import epipolar_cases as PC
from tests.guarded import U24


def test_the_switch_is_off_by_default_and_round_trips():
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import DEFAULT_CFG, make_cfg
    assert make_cfg().enable_epipolar_8pf is False and DEFAULT_CFG["enable_epipolar_8pf"] is False
    cfg = make_cfg(enable_epipolar_8pf=True, w_epipolar=0.25)
    assert cfg.enable_epipolar_8pf is True and cfg.w_epipolar == 0.25 and cfg.enable_eight_point is False


def test_lmeds_is_refused_with_the_switch_on():
    from unsupervised_depth_opticalflow_egomotion_amd._lib import DfeError
    from unsupervised_depth_opticalflow_egomotion_amd.models import Model_geometry
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg
    with pytest.raises(DfeError, match="FM_RANSAC only"):
        Model_geometry(make_cfg(enable_epipolar_8pf=True, dataset="nyuv2"))


def test_the_header_declares_the_new_entries():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib
    sigs = _lib.header_signatures()
    I, L, P = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    want = {
        "dfe_epipolar_ws_bytes": (L, [I, I, I]),
        "dfe_epipolar_loss_fwd": (I, [P] * 5 + [I, I, I, P]),
        "dfe_epipolar_loss_bwd": (I, [P] * 6 + [I, I, I, P]),
        "dfe_epipolar_map": (I, [P] * 3 + [I, I, I, P]),
    }
    for name, sig in want.items():
        assert sigs[name] == sig, name
    lib = _lib.get_lib()
    for name in want:
        assert hasattr(lib, name)
    assert _lib.header_abi_version() == 4                              # new symbols only


def test_the_workspace_query_answers_without_a_device():
    """one double per block and plane; a block holds 2048 pixels"""
    from unsupervised_depth_opticalflow_egomotion_amd import _lib
    lib = _lib.get_lib()
    for B, H, W in ((4, 256, 832), (2, 64, 208), (2, 5, 7), (1, 32, 64), (3, 13, 19)):
        assert lib.dfe_epipolar_ws_bytes(B, H, W) == 8 * 2 * B * ((H * W + 2047) // 2048)
    assert lib.dfe_epipolar_ws_bytes(0, 8, 8) == 0 and lib.dfe_epipolar_ws_bytes(2, 0, 8) == 0


def test_a_cpu_tensor_is_refused():
    from unsupervised_depth_opticalflow_egomotion_amd import epipolar
    from unsupervised_depth_opticalflow_egomotion_amd._lib import DfeError
    flow, F = torch.zeros(1, 2, 4, 4), torch.eye(3).repeat(2, 1, 1)
    with pytest.raises(DfeError):
        epipolar.epipolar_map(flow, F[:1])
    with pytest.raises(DfeError):
        epipolar.EpipolarLossFn.apply(flow, flow, F)


@pytest.mark.parametrize("shape", PC.SMALL_SHAPES)
def test_the_composition_in_float64_equals_the_direct_evaluation(shape):
    case = PC.make_case(shape)
    out = PC.solvers(case["F32"].double()).compute_epipolar_map_8pF(None, None, case["flow"].double(), None, None)
    ref = case["ref"]
    assert out.dtype == torch.float64 and tuple(out.shape) == (2 * case["B"], 1, case["H"], case["W"])
    # another association of the same three-term sums: a few roundings of the absolute sum, in float64
    assert bool(((out[:, 0] - ref["dist"]).abs() <= 8 * 2.0 ** -53 * ref["A"]).all())


def test_the_composition_uses_the_fundamental_matrix_of_its_matches():
    """with ``_minimal_sets`` overridden, the map is the direct evaluation under ``compute_fundmental_mat``'s F of the same
    matches, direction by direction"""
    key = (2, 12, 20, 72, 64, 32, True)
    case = EC.make_case(key)
    B = case["B"]
    m = EC.matches_of(case).double()
    s = PC.solvers()
    s.ransac_iters = int(case["sets"].shape[1])
    s._minimal_sets = lambda b, n, k, device: case["sets"].to(device).long()
    for d, flow in enumerate((case["flow_bwd"], case["flow_fwd"])):
        md = m[d * B:(d + 1) * B]
        out = s.compute_epipolar_map_8pF(md, None, flow.double(), case["K"], case["K_inv"])
        Fm = s.compute_fundmental_mat(md)
        assert torch.equal(Fm, case["comp"]["F"][d * B:(d + 1) * B])
        ref = PC.reference(flow.double(), Fm)
        assert bool(((out[:, 0] - ref["dist"]).abs() <= 8 * 2.0 ** -53 * ref["A"]).all())
        # the scene's own robust F: the inliers' distances are small, the map is not the pose's
        assert float(out.median()) < 0.1


@pytest.mark.parametrize("shape", PC.SHAPES)
def test_the_cases_meet_their_conditions(shape):
    """At most 1 % of the pixels near a sign or a threshold, both masks have both values (asserted by the helper), and the case
    tells the plane order apart: exchanging the two directions' planes of F moves some sample's loss by more than 100 x the
    loss bound."""
    case = PC.make_case(shape)
    B, H, W = shape
    n = 2 * B * H * W
    print("epipolar case %s: near a sign %d, near a threshold %d of %d; rigid %.1f %%, inlier %.1f %%; yardstick e %.3f"
          % (shape, round(case["sign_share"] * n), round(case["thres_share"] * n), n, 100 * case["rigid_share"],
             100 * case["inlier_share"], case["e_yard"]))
    assert case["sign_share"] <= PC.MAX_EXCLUDED and case["thres_share"] <= PC.MAX_EXCLUDED
    assert 0 < case["inlier_share"] < case["rigid_share"] < 1
    ones = [1.0] * B
    l64, mA, _, _ = PC.loss_reference(case["ref"], B, ones)
    bound = case["factor"] * U24 * mA + 2 * U24 * l64.abs()
    swapped = PC.loss_reference(PC.reference(case["flow"], torch.cat([case["F32"][B:], case["F32"][:B]], 0)), B, ones)[0]
    assert float(((swapped - l64).abs() / bound).max()) > 100


def test_the_noise_free_scene_sits_on_its_own_epipolar_lines():
    """why the gradient tests do not use it: under its own F about 70 % of its pixels have a sign of s decided by rounding"""
    share = PC.on_line_share()
    assert 0.6 <= share <= 0.8, share
