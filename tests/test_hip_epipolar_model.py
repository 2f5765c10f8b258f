"""GPU: ``cfg.enable_epipolar_8pf`` end to end on tests/geom_model.py's harness -- Model_geometry.loss_stack with and without the
switch (2 x 64 x 208 loss-stack inputs, no network), the robust F shared with the eight-point term, the lazy masks, and one
256 x 832 step eager and captured in a hipGraph (capture raises on any host read: the no-host-sync proof)."""
import numpy as np
import pytest
import torch

from tests import epipolar_cases as PC
from tests.geom_model import _run_stack, _stack_inputs, _bare, captured_step_equals_the_eager_step, dev
from unsupervised_depth_opticalflow_egomotion_amd.train_step import DEFAULT_CFG, make_cfg, total_loss

pytestmark = pytest.mark.gpu


def test_switch_off_the_pack_is_the_parents_and_on_every_other_key_keeps_its_bits():
    _, _, off = _run_stack(enable_epipolar_8pf=False)
    m, _, on = _run_stack(enable_epipolar_8pf=True)
    # off: the fused stack's own row, and ``rows`` maps loss_epipolar to it
    losses, fused = off.rows
    assert "loss_epipolar" in fused and torch.equal(off["loss_epipolar"].detach(), losses[fused["loss_epipolar"]].detach())
    assert getattr(off["loss_eight_point"], "_dfe_zero_placeholder", False)
    assert list(on) == list(off)
    for k in on:
        if k != "loss_epipolar":
            assert torch.equal(on[k].detach(), off[k].detach()), k
    # on: the same loss tensor, the map without loss_epipolar -- total_loss then takes the term from the dict
    assert torch.equal(on.rows[0], off.rows[0])
    assert on.rows[1] == {k: i for k, i in fused.items() if k != "loss_epipolar"}
    e = on["loss_epipolar"]
    assert tuple(e.shape) == (2,) and e.grad_fn is not None and bool(torch.isfinite(e).all()) and float(e.detach().abs().min()) > 0
    assert not torch.equal(e.detach(), off["loss_epipolar"].detach())          # another F: another term
    assert getattr(on["loss_eight_point"], "_dfe_zero_placeholder", False)     # the eight-point TERM stays off
    F = m.eight_point_F
    assert F.dtype == torch.float64 and tuple(F.shape) == (4, 3, 3) and not F.requires_grad and bool((F[:, 2, 2] == 1.0).all())


def test_the_term_trains_the_scale_0_flows_alone():
    m, x, on = _run_stack(enable_epipolar_8pf=True)
    e = on["loss_epipolar"]
    zero = {a: 0.0 for a in DEFAULT_CFG if a.startswith("w_")}
    zero["w_epipolar"] = 0.5
    cfg = make_cfg(enable_epipolar_8pf=True, **zero)
    total = total_loss(on, cfg)
    assert float(total.detach()) == pytest.approx(0.5 * float(e.detach().mean()), rel=1e-6)
    total.backward()
    torch.cuda.synchronize()
    for t in (x["fb"][0], x["ff"][0]):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0
    # the pose, the disparities and the coarser flows: nothing (the stack's own row is outside the sum, and all other weights
    # are zero: whatever reaches them is exactly zero)
    for t in [x["pose"]] + x["fb"][1:] + x["ff"][1:] + [d for lst in x["disps"] for d in lst]:
        assert t.grad is None or float(t.grad.abs().max()) == 0.0
    # and the term itself, without the rest of the sum, reaches the two flows only
    m2, x2, on2 = _run_stack(enable_epipolar_8pf=True)
    on2["loss_epipolar"].sum().backward()
    torch.cuda.synchronize()
    assert x2["fb"][0].grad is not None and x2["ff"][0].grad is not None
    for t in [x2["pose"]] + x2["fb"][1:] + x2["ff"][1:] + [d for lst in x2["disps"] for d in lst]:
        assert t.grad is None


def test_the_eight_point_term_shares_the_draw_and_the_fundamental_matrix():
    from unsupervised_depth_opticalflow_egomotion_amd import eight_point

    def offset():
        return int(torch.cuda.get_rng_state(dev())[8:16].view(torch.int64))
    m1, _, eight_only = _run_stack(enable_eight_point=True)
    off_eight = offset()
    calls, real = [], eight_point.fundamental_ransac

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    eight_point.fundamental_ransac = counted
    try:
        m2, _, both = _run_stack(enable_eight_point=True, enable_epipolar_8pf=True)
    finally:
        eight_point.fundamental_ransac = real
    off_both = offset()
    assert len(calls) == 1                                           # one robust F per step
    assert torch.equal(both["loss_eight_point"].detach(), eight_only["loss_eight_point"].detach())      # the bits it has alone
    assert torch.equal(m1.eight_point_F, m2.eight_point_F)
    assert torch.equal(m1.triangle_draw[0], m2.triangle_draw[0]) and torch.equal(m1.triangle_draw[1], m2.triangle_draw[1])
    torch.manual_seed(11)
    torch.randint(0, int(0.3 * 64 * 208), [6000], device=dev())
    assert off_both == off_eight == offset()                         # the generator advanced by exactly one draw
    _, _, epi_only = _run_stack(enable_epipolar_8pf=True)
    assert torch.equal(both["loss_epipolar"].detach(), epi_only["loss_epipolar"].detach())


def test_the_term_is_the_operator_under_the_steps_fundamental_matrix():
    """loss_epipolar of the stack against the float64 evaluation under the step's own F (rounded to fp32 as the kernel reads it)"""
    m, x, on = _run_stack(enable_epipolar_8pf=True)
    F32 = m.eight_point_F.float().cpu()
    flow = torch.cat([x["fb"][0].detach(), x["ff"][0].detach()], 0).cpu()
    ref = PC.reference(flow, F32)
    yard = PC.yardstick(flow, F32)
    factor = 4.0 * max(1.0, float(((yard.double() - ref["dist"]).abs() / (PC.U24 * ref["A"])).max()))
    l64, mA, _, _ = PC.loss_reference(ref, 2, (1.0, 1.0))
    err = (on["loss_epipolar"].detach().double().cpu() - l64).abs() / (factor * PC.U24 * mA + 2 * PC.U24 * l64.abs())
    print("EBOUND epipolar_8pf model 2x64x208: loss err/bound %.3f (factor %.3f)" % (float(err.max()), factor))
    assert float(err.max()) <= 1.0


def test_the_lazy_masks_are_get_rigid_mask_of_the_eight_point_map():
    x = _stack_inputs()
    m = _bare(enable_epipolar_8pf=True)
    torch.manual_seed(11)
    _, masks = m.loss_stack(x["imgs"][0], x["imgs"][1], x["imgs"][2], x["disps"][0], x["disps"][1], x["disps"][2], x["pose"], x["fb"],
                            x["ff"], x["K"], x["Ki"])
    rigid, inlier = masks["rigid_fwd_mask"], masks["inlier_fwd_mask"]
    B = 2
    flow = x["ff"][0].detach()[:1].cpu()
    ref = PC.reference(flow, m.eight_point_F[B:B + 1].float().cpu())          # sample 0's forward plane: plane 1*B + 0
    d64, n = ref["dist"], ref["dist"].numel()
    for got, thres in ((rigid, PC.RIGID_THRES), (inlier, PC.INLIER_THRES)):
        assert got.dtype == np.uint8 and got.shape == (1, 64, 208) and set(np.unique(got)) == {0, 255}       # both values
        keep = ~PC.near_threshold(ref, thres)
        assert int((~keep).sum()) <= PC.MAX_EXCLUDED * n
        want = 255 * (d64 < thres).to(torch.uint8)
        assert bool((torch.from_numpy(got)[keep] == want[keep]).all())
    # not the pose's map: with the switch off the masks differ
    m0 = _bare(enable_epipolar_8pf=False)
    torch.manual_seed(11)
    _, masks0 = m0.loss_stack(x["imgs"][0], x["imgs"][1], x["imgs"][2], x["disps"][0], x["disps"][1], x["disps"][2], x["pose"],
                              x["fb"], x["ff"], x["K"], x["Ki"])
    assert not np.array_equal(masks0["rigid_fwd_mask"], rigid)


def test_the_step_with_the_term_is_captured_and_equals_the_eager_step():
    captured_step_equals_the_eager_step("loss_epipolar", enable_epipolar_8pf=True)
