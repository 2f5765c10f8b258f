"""The GPU-side scaffolding of the RANSAC terms' tests (tests/test_hip_eight_point.py, tests/test_hip_pnp.py), stated once: a helper,
not a conftest.  Carving the draw's buffers and the workspace out of guarded ones, slicing the workspace by the wrapper's
``workspace_sections``, the decision equalities, and the bodies of the tests that are the same for both terms.  A body takes
the term's runner (``raw_ransac``), its cases module ``M`` (tests/*_cases.py) and ``stages``, the term's own checks of a run
against float64: ``stages(case, out, cont, sets, well, tag, only=None)``."""
import ctypes

import torch

from tests import guarded as G
from tests.ransac_cases import CRAFTED_SLOTS, distinct_pixels

P = ctypes.c_void_p


def _i32(carved):
    return carved.view.contiguous().view(torch.int32).cpu()


def _doubles_written(carved):
    """``Carved.written`` for a buffer of doubles: every double finite and neither of its words the sentinel.  (``written`` reads
    the words as floats, and the low word of a finite double is a NaN or an infinity once in 128 doubles: seen at B = 3.)"""
    words = _i32(carved)
    return bool(torch.isfinite(carved.view.contiguous().view(torch.float64)).all()) and bool((words != G.SENTINEL).all())


def _tag(key):
    return "x".join(str(int(v)) for v in key)


def _bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t.contiguous().view(torch.int32)


def raw_ransac(case, launch, sections, width, table, sets=None, flow_bwd=None, flow_fwd=None, offsets=(1, 2, 3, 2), more=()):
    """A RANSAC entry point with the flows, every output and the workspace carved; guards checked.  ``launch(fb, ff, idx, pick,
    sets, est64, est32, info, ws, (B, H, W, k, num, hyp))`` makes the call on those pointers and checks its status;
    ``sections``: the wrapper's ``workspace_sections(B, num, hyp)``, whose ``table`` = (name, doubles per slot) is the hypothesis
    table; ``width``: the estimate's length per plane; ``more``: the term's further carved inputs, for the guard check.
    -> dict of CPU tensors: ``est64`` / ``est32`` [2B,width], ``info`` [2B,4], ``counts`` [2B,hyp], ``w1`` / ``w2`` [2B,num],
    ``table`` [2B,hyp,doubles] (bits as the kernel left them), ``written``."""
    B, H, W, k, num = (case[n] for n in ("B", "H", "W", "k", "num"))
    sets = (case["sets"] if sets is None else sets).cuda().contiguous()
    hyp = sets.shape[1]
    fb = G.Carved((B, 2, H, W), offset_floats=offsets[0], fill=case["flow_bwd"] if flow_bwd is None else flow_bwd)
    ff = G.Carved((B, 2, H, W), offset_floats=offsets[1], fill=case["flow_fwd"] if flow_fwd is None else flow_fwd)
    idx, pick = case["idx"].cuda(), case["pick"].cuda()
    est64 = G.Carved((2 * B * width, 2), offset_floats=offsets[3])          # doubles: 8-byte aligned, not 16
    est32 = G.Carved((2 * B, width), offset_floats=offsets[2])
    info = G.Carved((2 * B, 4), offset_floats=1)
    sec = sections(B, num, hyp)
    ws = G.Carved((sec["bytes"] // 4,), offset_floats=0)
    launch(P(fb.ptr), P(ff.ptr), P(idx.data_ptr()), P(pick.data_ptr()), P(sets.data_ptr()), P(est64.ptr), P(est32.ptr), P(info.ptr),
           P(ws.ptr), (B, H, W, k, num, hyp))
    torch.cuda.synchronize()
    for c in (fb, ff, est64, est32, info, ws) + tuple(more):
        assert c.intact()
    words = _i32(ws)
    sl = lambda name, n: words[sec[name] // 4:sec[name] // 4 + n]   # noqa: E731
    name, doubles = table
    return dict(table=sl(name, 2 * 2 * B * hyp * doubles).clone().view(torch.float64).reshape(2 * B, hyp, doubles),
                est64=est64.view.contiguous().view(torch.float64).cpu().reshape(2 * B, width), est32=est32.cpu().reshape(2 * B, width),
                info=_i32(info).reshape(2 * B, 4), counts=sl("counts", 2 * B * hyp).reshape(2 * B, hyp),
                w1=sl("w1", 2 * B * num).reshape(2 * B, num), w2=sl("w2", 2 * B * num).reshape(2 * B, num),
                written=_doubles_written(est64) and est32.written() and info.written())


def _equal_decisions(out, c):
    """The integers of a run equal those of a float64 composition ``c``: every count, both weight sets, the four info columns."""
    assert out["written"]
    assert torch.equal(out["counts"].long(), c["counts"])                       # every hypothesis, as integers
    assert torch.equal(out["w1"].long(), c["w1"].long()) and torch.equal(out["w2"].long(), c["w2"].long())
    info = out["info"].long()
    assert torch.equal(info[:, 0], c["best"]) and torch.equal(info[:, 1], c["counts"].max(1)[0])
    assert torch.equal(info[:, 2], c["w1"].sum(1).long()) and torch.equal(info[:, 3], c["w2"].sum(1).long())


def check_well_defined_counts(out, comp, well):
    """Stage 1."""
    assert torch.equal(out["counts"].long()[well], comp["counts"][well])


def check_scoring(out, err, inl, thresh, margin, z=None):
    """Stage 3: every slot's count is the float64 recount (``err``, ``inl`` [2B,hyp,num]) from the kernel's own table; a (slot,
    match) pair within ``margin`` of the threshold (or with a depth ``z`` within ``margin`` of zero) is left out, and a second
    such pair makes the case inconclusive."""
    t = thresh * thresh
    near = torch.isfinite(err) & ((err - t).abs() / t < margin)
    if z is not None:
        near = near | (torch.isfinite(z) & (z.abs() < margin))
    assert int(near.sum()) <= 1, "inconclusive: %d residuals within MARGIN of the threshold" % int(near.sum())
    sure = inl & ~near
    got = out["counts"].long()
    assert bool((got >= sure.sum(2)).all() and (got <= sure.sum(2) + near.sum(2)).all())


def tied_counts_go_to_the_lowest_index(case, out, raw_ransac, est):
    """Two identical hypotheses: the winner of plane (d = 0, b = 0) is copied to another slot of sample 0's sets; both have the
    maximum count of that plane and the lower slot wins.  The estimate ``out[est]`` does not move."""
    best = int(case["comp"]["best"][0])
    slot = 0 if best != 0 else 1
    sets = case["sets"].clone()
    sets[0, slot] = sets[0, best]
    tied = raw_ransac(case, sets=sets)
    assert int(tied["counts"][0, slot]) == int(tied["counts"][0, best]) == int(out["info"][0, 1])
    assert int(tied["info"][0, 0]) == min(slot, best) and int(tied["info"][0, 1]) == int(out["info"][0, 1])
    assert torch.equal(tied["w1"][0], out["w1"][0]) and torch.equal(tied[est][0], out[est][0])


def drawn_sets_stage_by_stage(case, out, cont, stages, key):
    """Stages 1 to 4 on a drawn case, and: the seed was chosen for a well-defined winner, so none of the kernel's ill-defined slots
    out-polls it and the decisions are the composition's without those slots (case["ref"]: the same on every host).  The term
    holds the estimate to ``ref``'s within its own bound."""
    assert out["written"]
    check_well_defined_counts(out, case["comp"], case["well"])
    stages(case, out, cont, case["sets"], case["well"], "drawn " + _tag(key))
    ref = case["ref"]
    assert torch.equal(out["info"].long()[:, 0], ref["best"]) and torch.equal(out["w2"].long(), ref["w2"].long())


def a_winner_with_repeated_matches(case, out, cont, stages, size):
    """The case whose reference winner is ill-defined: stages 2-4 alone.  The kernel's own winner of some plane repeats a match,
    and its consensus (``size`` members at least) goes through both refits with neither fall-back."""
    assert out["written"]
    stages(case, out, cont, case["sets"], case["well"], "ill-defined winner")
    best = out["info"].long()[:, 0]
    repeats = ~torch.cat([distinct_pixels(case)] * 2, 0)
    won = torch.gather(repeats, 1, best.view(-1, 1)).squeeze(1)
    assert bool(won.any()), "no plane's winner repeats a match"
    assert bool((cont["n1raw"][won] >= size).all() and (cont["n2raw"][won] >= size).all())
    assert torch.equal(out["info"].long()[won, 1], out["w1"][won].sum(1).long())      # the consensus is the winner's own set


def crafted_run(M, case, base, raw_ransac, stages, table, estimates, slots, tag):
    """The hyp = 70 case with ``slots`` of sample 0's sets overwritten by degenerate sets (M.crafted_sets): every other slot and
    the other sample bit-equal to the baseline's run ``base``, the overwritten slots through stages 2 and 3, the outputs through
    stage 4.  ``table`` / ``estimates``: the names of the hypothesis table's and the estimate's tensors in a run."""
    B, hyp = case["B"], case["hyp"]
    assert hyp == 70 and B == 2
    sets = M.crafted_sets(case, slots)
    out = raw_ransac(case, sets=sets)
    assert out["written"]
    touched = torch.zeros(2 * B, hyp, dtype=torch.bool)
    for d in range(2):
        touched[d * B, list(slots)] = True
    well = M.well_defined(case, sets)
    assert not bool(well[touched].any()) and torch.equal(well[~touched], case["well"][~touched])
    for name in table + ("counts",):                                                         # no slot's slice leaks into another's
        assert torch.equal(_bits(out[name])[~touched], _bits(base[name])[~touched]), name
    for d in range(2):                                                                       # sample 1: every output
        p = d * B + 1
        for name in estimates + ("info", "w1", "w2", "counts") + table:
            assert torch.equal(_bits(out[name][p]), _bits(base[name][p])), (name, p)
    stages(case, out, M.continued(case, *[out[name] for name in table]), sets, well, tag, only=touched)
    return out


def degenerate_sets_stay_inside_their_own_slice(base, crafted, estimates):
    """``crafted(slots, tag)``: the term's crafted run.  No winner is among CRAFTED_SLOTS: the estimate does not move."""
    out = crafted(CRAFTED_SLOTS, "crafted slots")
    assert not any(int(b) in CRAFTED_SLOTS for b in base["info"][:, 0])
    for name in estimates + ("info", "w1", "w2"):
        assert torch.equal(_bits(out[name]), _bits(base[name])), name


def a_degenerate_winning_slot_hands_over_to_the_runner_up(base, crafted):
    best = int(base["info"][0, 0])
    slots = CRAFTED_SLOTS[:5] + (best,)
    assert best not in CRAFTED_SLOTS[:5]
    out = crafted(slots, "crafted winner")
    counts = base["counts"][0].clone()
    counts[list(slots)] = -1
    assert int(out["counts"][0, best]) < int(counts.max())                  # the degenerate set polls less than the runner-up
    assert int(out["info"][0, 0]) == int(counts.argmax()) and int(out["info"][0, 1]) == int(counts.max())


def guarded_loss_entry_points(B, ins, grad, weights, fwd, bwd):
    """The loss's raw entry points on carved buffers: ``fwd(*ins, loss)`` and ``bwd(*ins, gloss, grad)`` on pointers; every guard
    intact, the loss and the gradient written."""
    loss, gloss = G.Carved((B,), offset_floats=1), G.Carved((B,), offset_floats=3, fill=torch.tensor(weights))
    fwd(*[P(c.ptr) for c in ins], P(loss.ptr))
    bwd(*[P(c.ptr) for c in ins], P(gloss.ptr), P(grad.ptr))
    torch.cuda.synchronize()
    assert all(c.intact() for c in ins + [loss, gloss, grad]) and loss.written() and grad.written()


def loss_errors(loss, l64, *pairs):
    """(the largest relative error of the per-sample loss, the error of each (gradient, its float64) pair over that gradient's
    scale): the figures the loss tests hold to DESIGN section 2's 5e-6 and 2e-5."""
    el = float(((loss.detach().double().cpu() - l64).abs() / l64.abs()).max())
    return (el,) + tuple(float((g.double().cpu() - g64).abs().max() / g64.abs().max()) for g, g64 in pairs)
