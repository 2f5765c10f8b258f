"""dfe_topk_select (csrc/ops_select.hip) in guarded buffers: the pixel-ordered top-k set of every plane against torch.topk and
against the numpy restatement of its tie rule, at plane sizes that are no multiple of the wave, the block or the ordered pass's
chunk (247: one partial chunk; 4099: one chunk of 4096 and three scores; 8193: three rounds of the ordered pass, a single score
in the third, where the double-buffered wave totals are first reused; 12301: four rounds, 13 scores in the last), k at both ends
and at the training ratio; planes of one repeated value (the largest packed tie count), sets that lie wholly in the first or the
last round, and 1 and 8 planes."""
import ctypes

import numpy as np
import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu

PLANES = 3
SIZES = (247, 4099, 8193, 12301)
ROUND = 4096                    # scores per round of the ordered pass (SEL_THREADS x SEL_ITEMS)


def ks(n):
    return (1, int(0.3 * n), n - 1, n)


def run_select(scores, k, offset=1):
    """scores [planes, n] CPU fp32 -> (idx int32 [planes, k] CPU, record int32 [planes, 4]) from carved buffers; asserts the guards
    are intact and that every output element was written."""
    from unsupervised_depth_opticalflow_egomotion_amd import _lib
    lib = _lib.get_lib()
    planes, n = scores.shape
    src = G.Carved((planes, n), offset_floats=offset, fill=scores)
    out = G.Carved((planes, k), offset_floats=(offset + 2) % 4)
    assert lib.dfe_topk_ws_bytes(planes, n, k) == 16 * planes
    ws = G.Carved((planes, 4), offset_floats=3)
    _lib.check(lib.dfe_topk_select(ctypes.c_void_p(src.ptr), ctypes.c_void_p(out.ptr), ctypes.c_void_p(ws.ptr), planes, n, k,
                                   _lib.stream_ptr()), "dfe_topk_select")
    torch.cuda.synchronize()
    assert src.intact() and out.intact() and ws.intact()
    idx = out.view.view(torch.int32).cpu()
    rec = ws.view.view(torch.int32).cpu()
    assert bool((idx != G.SENTINEL).all()) and bool((rec != G.SENTINEL).all()), "an output element was not written"
    assert bool(((idx >= 0) & (idx < n)).all())
    return idx, rec


def restated(scores, k):
    """sort by (-score, index) in torch.topk's order (NaN above +inf, -0 == +0), take k, sort by index"""
    out = []
    for p in scores.numpy():
        key = np.where(np.isnan(p), np.inf, p.astype(np.float64))
        rank = np.where(np.isnan(p), 1, 0)                   # NaN above +inf
        order = np.lexsort((np.arange(p.size), -key, -rank))
        out.append(np.sort(order[:k]))
    return np.stack(out).astype(np.int32)


def ascending(idx):
    return bool((idx[:, 1:] > idx[:, :-1]).all())


@pytest.mark.parametrize("n", SIZES)
def test_distinct_scores_match_topk(n):
    g = torch.Generator().manual_seed(n)
    scores = torch.randperm(PLANES * n, generator=g).float().view(PLANES, n) / 7.0 - 100.0      # distinct, both signs
    for k in ks(n):
        idx, rec = run_select(scores, k)
        assert ascending(idx)
        want = torch.topk(scores.cuda(), k, dim=1)[1].sort(1)[0].cpu().int()
        assert torch.equal(idx, want), (n, k)
        assert bool((rec[:, 1] + rec[:, 2] == k).all()) and bool((rec[:, 2] == 1).all())


@pytest.mark.parametrize("n", SIZES)
def test_tied_scores_go_to_the_lower_index(n):
    g = torch.Generator().manual_seed(7 * n)
    scores = torch.randint(0, 8, (PLANES, n), generator=g).float() * 0.25 - 0.5              # 8 levels, -0.5 .. 1.25
    scores[0, ::5] = -0.0                                                                      # -0 ties with +0 (level 2)
    for k in ks(n):
        idx, rec = run_select(scores, k)
        assert ascending(idx)
        assert np.array_equal(idx.numpy(), restated(scores, k)), (n, k)
    k = int(0.3 * n)                  # ~n/8 scores per level, 0.3 n falls inside the third: the threshold's tie group is split
    _, rec = run_select(scores, k)
    level = torch.sort(scores, 1, descending=True)[0][:, k - 1]
    split = (scores == level[:, None]).sum(1) > rec[:, 2]          # more scores at the threshold than ties taken
    assert int(split.sum()) >= 2, "no tie group straddles the threshold"


@pytest.mark.parametrize("n", SIZES)
def test_nan_and_infinities_rank_as_topk_ranks_them(n):
    g = torch.Generator().manual_seed(11 * n)
    scores = torch.randn(PLANES, n, generator=g)
    scores[:, 3::41] = float("nan")
    scores[:, 5::37] = float("inf")
    scores[:, 7::43] = float("-inf")
    n_nan = int(torch.isnan(scores[0]).sum())
    for k in ks(n) + (n_nan, n_nan + 2):
        idx, _ = run_select(scores, k)
        assert ascending(idx)
        assert np.array_equal(idx.numpy(), restated(scores, k)), (n, k)
        # the same multiset of values as torch.topk's (which NaN of several it takes is its own business)
        got = torch.gather(scores, 1, idx.long()).sort(1)[0]
        want = torch.topk(scores.cuda(), k, dim=1)[0].sort(1)[0].cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(0.0), want.nan_to_num(0.0)), (n, k)


@pytest.mark.parametrize("n", [ROUND, 12301])
def test_a_plane_of_one_repeated_value_takes_the_first_k(n):
    """Every score ties: nothing lies above the threshold, a full round counts 4096 equal scores in the packed upper half, and
    the set is the first k pixels."""
    value = 0.375
    scores = torch.full((PLANES, n), value)
    key = int(np.float32(value).view(np.uint32)) | 0x80000000            # the order-preserving key of a positive score
    for k in ks(n):
        idx, rec = run_select(scores, k)
        assert torch.equal(idx, torch.arange(k, dtype=torch.int32).expand(PLANES, k)), (n, k)
        want = torch.tensor([key, 0, k, 0], dtype=torch.int64).expand(PLANES, 4)
        assert torch.equal(rec.long() & 0xffffffff, want), (n, k)


@pytest.mark.parametrize("where", ["first", "last"])
def test_a_set_that_lies_wholly_in_one_round(where):
    """n = 12301, four rounds: the k largest scores all in the first round (the three later rounds add nothing and must not
    disturb the positions) or all in the last (every base count stays 0 until then)."""
    n = 12301
    g = torch.Generator().manual_seed(13)
    scores = torch.randperm(PLANES * n, generator=g).float().view(PLANES, n) / 7.0 - 100.0      # distinct, all below 5200
    lo, hi = (0, ROUND) if where == "first" else (3 * ROUND, n)
    for k in (1, 7, hi - lo):
        boosted = scores.clone()
        for p in range(PLANES):
            at = lo + torch.randperm(hi - lo, generator=g)[:k]
            boosted[p, at] += 1.0e4
        idx, rec = run_select(boosted, k)
        assert ascending(idx)
        assert int(idx.min()) >= lo and int(idx.max()) < hi
        want = torch.topk(boosted.cuda(), k, dim=1)[1].sort(1)[0].cpu().int()
        assert torch.equal(idx, want), (where, k)
        assert np.array_equal(idx.numpy(), restated(boosted, k))


@pytest.mark.parametrize("planes", [1, 8])
def test_one_plane_and_eight(planes):
    n = 8193
    g = torch.Generator().manual_seed(17 * planes)
    scores = torch.randint(0, 64, (planes, n), generator=g).float() * 0.25 - 4.0               # ties at every level
    for k in (int(0.3 * n), n - 1):
        idx, rec = run_select(scores, k)
        assert tuple(idx.shape) == (planes, k) and ascending(idx)
        assert np.array_equal(idx.numpy(), restated(scores, k)), (planes, k)
        assert bool((rec[:, 1] + rec[:, 2] == k).all())


def test_two_runs_give_identical_bits():
    g = torch.Generator().manual_seed(5)
    scores = torch.randint(0, 8, (PLANES, 4099), generator=g).float()
    a, ra = run_select(scores, 1229)
    b, rb = run_select(scores, 1229, offset=3)
    assert torch.equal(a, b) and torch.equal(ra, rb)


def test_refusals_come_before_the_launch():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib
    lib = _lib.get_lib()
    out = G.Carved((1, 8))
    src = G.Carved((1, 8), fill=torch.zeros(1, 8))
    ws = G.Carved((1, 4))
    for k in (0, 9):
        assert lib.dfe_topk_select(ctypes.c_void_p(src.ptr), ctypes.c_void_p(out.ptr), ctypes.c_void_p(ws.ptr), 1, 8, k,
                                   _lib.stream_ptr()) == -2
    assert lib.dfe_topk_select(None, ctypes.c_void_p(out.ptr), ctypes.c_void_p(ws.ptr), 1, 8, 4, _lib.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert out.untouched() and ws.untouched()
