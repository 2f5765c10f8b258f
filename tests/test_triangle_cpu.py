"""CPU: the triangulation term's host side -- the case helper's conditions, ``triangle_term_torch`` against golden G11 (the
reference's own ``compute_triangulate_loss``), the switch's default, and the new entry points' declarations."""
import os

import numpy as np
import pytest
import torch

from tests import triangle_cases as TC


@pytest.mark.parametrize("key", sorted(TC.SEEDS))
def test_the_cases_meet_their_conditions(key):
    H, W, ac = key
    case = TC.make_case(H, W, ac)                                   # asserts the three conditions itself
    zmin, cmin, dmin = TC.conditions(case, ac)
    assert zmin >= 0.05 and cmin >= 1e-3 and dmin >= 1e-3
    assert case["idx"].dtype == torch.int32 and tuple(case["idx"].shape) == (4, 72)
    assert bool((case["idx"][:, 1:] > case["idx"][:, :-1]).all()) and int(case["idx"].max()) < H * W
    t = case["T34"][:, :, :, 3].norm(dim=-1)
    assert float(t.min()) >= 0.1
    assert all(float(case[n].min()) > 0 for n in ("disp_t", "disp_l", "disp_r"))
    pick = TC.make_pick(case, 150)
    assert pick.unique().numel() < 150 and int(pick.max()) < 72 and pick.dtype == torch.int64


def test_the_float64_reference_differentiates_every_input():
    case = TC.make_case(12, 20, False)
    loss, grads = TC.torch_term(case, TC.make_pick(case, 50), False, torch.float64)
    assert tuple(loss.shape) == (2,) and bool((loss > 0).all())
    for n in TC.GRAD_NAMES:
        assert grads[n].shape == case[n].shape and float(grads[n].abs().max()) > 0, n


@pytest.mark.parametrize("ac", [False, True])
def test_triangle_term_torch_reproduces_golden_g11(golden_dir, ac):
    """``triangle_term_torch`` in float64 on G11's inputs, both directions fed the same matches, pose and second depth: twice the
    reference's ``trian_loss``.  The golden is the reference's fp32 result through a median normalisation; the existing device
    test holds the same quantity to 1e-3 (tests/test_hip_models.py), and so does this."""
    from tests.golden import make_golden as MG
    from unsupervised_depth_opticalflow_egomotion_amd import ops
    g = np.load(os.path.join(golden_dir, "G11_ac%d.npz" % ac))
    c = MG.g11_inputs()
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()   # noqa: E731
    K, match, d1, d2 = D(c["K"]), D(c["match"]), D(c["depth1"]), D(c["depth2"])
    Ki = torch.inverse(K)
    T = Ki.bmm(D(g["P2"]))                                           # P2 = K T34
    T34 = torch.stack([T, T], 1)
    m = TC.bare_model()
    old = ops.get_align_corners()
    ops.set_align_corners(ac)
    try:
        loss = m.triangle_term_torch(d2, d1, d2, T34, None, None, K, Ki, None, None, matches=(match, match))
    finally:
        ops.set_align_corners(old)
    np.testing.assert_allclose(loss.numpy(), 2.0 * g["trian_loss"].astype(np.float64), rtol=1e-3)


def test_the_switch_is_off_by_default():
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import DEFAULT_CFG, make_cfg
    assert make_cfg().enable_triangle is False and DEFAULT_CFG["enable_triangle"] is False
    assert make_cfg(enable_triangle=True).enable_triangle is True


def test_the_header_declares_the_new_entries():
    import ctypes
    from unsupervised_depth_opticalflow_egomotion_amd import _lib
    sigs = _lib.header_signatures()
    I, L, P = ctypes.c_int, ctypes.c_long, ctypes.c_void_p
    want = {
        "dfe_topk_ws_bytes": (L, [I, I, I]),
        "dfe_topk_select": (I, [P, P, P, I, I, I, P]),
        "dfe_triangulate_ws_bytes": (L, [I, I, I, I]),
        "dfe_triangulate_fwd": (I, [P] * 11 + [I] * 6 + [P]),
        "dfe_triangulate_stats": (I, [P, P, P, I, I, P]),
        "dfe_triangulate_bwd": (I, [P] * 15 + [I] * 6 + [P]),
    }
    lib = _lib.get_lib()
    for name, (res, args) in want.items():
        assert sigs[name] == (res, args), name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    # host-only queries answer without a device
    assert lib.dfe_topk_ws_bytes(8, 212992, 63897) == 128 and lib.dfe_topk_ws_bytes(1, 4, 5) == 0
    assert lib.dfe_triangulate_ws_bytes(4, 256, 832, 6000) == 64 + 56 * 4 * 212992 + 32 * 4 * 6000 + 192 * 4 * 24


def _crc(case, names):
    import zlib
    c = 0
    for n in names:
        c = zlib.crc32(case[n].contiguous().numpy().tobytes(), c)
    return c


def test_the_new_keyword_leaves_the_existing_cases_bits():
    """``depth_lo`` defaults to the former constant, and the generator is consumed as before: the camera matrices (the first
    draws) and the idx sets (the last) of every existing case carry the checksums taken before the keyword existed."""
    import inspect
    assert inspect.signature(TC.build).parameters["depth_lo"].default == 2.0
    want = {(12, 20, False): 1262564265, (12, 20, True): 2312075249, (13, 19, False): 47078355, (13, 19, True): 1933281735}
    assert TC.SEEDS == {(12, 20, False): 4, (12, 20, True): 16, (13, 19, False): 3, (13, 19, True): 15}
    for key, seed in TC.SEEDS.items():
        case = TC.build(seed, 2, key[0], key[1], 72)
        assert _crc(case, ("K", "idx")) == want[key], key
        explicit = TC.build(seed, 2, key[0], key[1], 72, depth_lo=2.0)
        assert all(torch.equal(case[n], explicit[n]) for n in case if torch.is_tensor(case[n]))


@pytest.mark.parametrize("key", sorted(TC.SEEDS))
def test_no_existing_case_folds_a_sample_twice(key):
    once, twice = TC.folds(TC.make_case(*key), key[2])
    print("FOLDS %s: %d samples folded once, %d twice or more" % (key, once, twice))
    assert once > 0 and twice == 0


@pytest.mark.parametrize("key", TC.EDGE_SHAPES)
def test_the_edge_cases_meet_their_conditions(key):
    B, H, W, ac, depth_lo = key
    case = TC.make_edge_case(key)                                   # asserts the three conditions itself
    zmin, cmin, dmin = TC.conditions(case, ac)
    assert zmin >= 0.05 and cmin >= 1e-3 and dmin >= 1e-3
    assert case["B"] == B and tuple(case["idx"].shape) == (2 * B, 72) and tuple(case["T34"].shape) == (B, 2, 3, 4)
    assert bool((case["idx"][:, 1:] > case["idx"][:, :-1]).all()) and int(case["idx"].max()) < H * W
    assert all(float(case[n].min()) > 0 for n in ("disp_t", "disp_l", "disp_r"))
    once, twice = TC.folds(case, ac)
    print("FOLDS %s seed %d: %d samples folded once, %d twice or more" % (key, TC.EDGE_SEEDS[key], once, twice))
    if depth_lo < 2.0:
        drawn = TC.folds(case, ac, TC.make_pick(case, 150))[1]
        print("FOLDS %s: %d of them among the 150 draws of the device test" % (key, drawn))
        assert twice >= 1 and drawn >= 1                            # what the case was chosen for
    else:
        assert B in (1, 3)


def test_the_block_edge_counts():
    """257 = one point past a block of 256 threads, 601 = three blocks, partly filled; 51, 257 and 601 are odd, so the lower
    median of rank (num - 1) / 2 is the middle element."""
    for num, blocks in ((51, 1), (257, 2), (601, 3)):
        assert (num + 255) // 256 == blocks and num % 2 == 1 and num % 256 != 0
    case = TC.make_case(12, 20, False)
    assert TC.make_pick(case, 257).unique().numel() <= 72 < 257
