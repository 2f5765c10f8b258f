"""GPU: ``cfg.enable_triangle`` end to end -- Model_geometry.loss_stack with and without the switch, the term against
``triangle_term_torch`` on its own draw, gradients to every input, one eager training step, and the step captured in a hipGraph
(capture raises on any host read: the no-host-sync proof)."""
import numpy as np
import pytest
import torch

from tests.geom_model import _run_stack, dev
from unsupervised_depth_opticalflow_egomotion_amd import convs, ops, synthetic
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
from unsupervised_depth_opticalflow_egomotion_amd.train_step import GraphedTrainStep, make_cfg, make_optimizer, total_loss, train_step

pytestmark = pytest.mark.gpu


def test_the_switch_adds_the_term_and_changes_nothing_else():
    _, _, off = _run_stack(enable_triangle=False)
    m, x, on = _run_stack(enable_triangle=True)
    assert getattr(off["loss_triangle"], "_dfe_zero_placeholder", False) and tuple(off["loss_triangle"].shape) == (2,)
    tri = on["loss_triangle"]
    assert tuple(tri.shape) == (2,) and tri.grad_fn is not None and bool(torch.isfinite(tri).all()) and float(tri.detach().min()) > 0
    assert not getattr(tri, "_dfe_zero_placeholder", False)
    assert list(on) == list(off)
    for k in on:
        if k != "loss_triangle":
            assert torch.equal(on[k].detach(), off[k].detach()), k
    assert torch.equal(on.rows[0], off.rows[0]) and on.rows[1] == off.rows[1]
    # the weighted total takes it through the generic branch
    cfg = make_cfg(enable_triangle=True, w_triangle=0.5)
    assert float(total_loss(on, cfg).detach()) == pytest.approx(float(total_loss(off, cfg).detach()) + 0.5 * float(tri.detach().mean()), rel=1e-5)


def test_the_term_equals_the_torch_composition_on_its_own_draw():
    """Within the operator bound of tests/test_hip_triangulate.py: error against float64 autograd-free ``triangle_term_torch`` on
    the term's own ``idx`` / ``pick``, normalised by the largest float64 magnitude, at most 4 x max(the fp32 composition's, 2^-24)."""
    m, x, on = _run_stack(enable_triangle=True)
    idx, pick = m.triangle_draw
    k = int(0.3 * 64 * 208)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (4, k) and tuple(pick.shape) == (6000,) and pick.dtype == torch.int64
    assert bool((idx[:, 1:] > idx[:, :-1]).all()) and int(pick.min()) >= 0 and int(pick.max()) < k
    with torch.no_grad():
        T34 = ops.PoseMatsFn.apply(x["pose"].detach().reshape(4, 6))[0].view(2, 2, 3, 4)
        args = (x["disps"][0][0], x["disps"][1][0], x["disps"][2][0], T34, x["fb"][0], x["ff"][0], x["K"], x["Ki"])
        yard = m.triangle_term_torch(*[a.detach() for a in args], idx, pick)
        ref = m.triangle_term_torch(*[a.detach().double().cpu() for a in args], idx.cpu(), pick.cpu())
    scale = float(ref.abs().max())
    ek = float((on["loss_triangle"].detach().double().cpu() - ref).abs().max()) / scale
    ey = float((yard.double().cpu() - ref).abs().max()) / scale
    print("EBOUND triangle_term 2x64x208 loss kernel %.3e yardstick %.3e (max |ref| %.3e)" % (ek, ey, scale))
    assert ek <= 4.0 * max(ey, 2.0 ** -24), (ek, ey)


def test_the_terms_gradients_equal_float64_autograd_on_its_own_draw():
    """The same rule for the gradients, at the product's own draw: num = 6000 is 24 blocks of points per plane, k = 3993 pixels, so
    most pixels are drawn more than once.  Reference: float64 autograd on the CPU of ``triangle_term_torch`` behind the oracle's
    ``pose_vec2mat``; yardstick: the fp32 composition on the device behind ``PoseMatsFn``, as the term itself is; a different
    cotangent per sample."""
    from oracle import loss_stack_oracle as O
    m, x, on = _run_stack(enable_triangle=True)
    idx, pick = m.triangle_draw
    assert pick.unique().numel() < idx.shape[1] < pick.numel()
    w = torch.tensor([0.7, 1.3])
    leaves = dict(flow_bwd=x["fb"][0], flow_fwd=x["ff"][0], disp_l=x["disps"][0][0], disp_t=x["disps"][1][0], disp_r=x["disps"][2][0],
                  pose=x["pose"])
    names = list(leaves)
    got = torch.autograd.grad((on["loss_triangle"] * w.cuda()).sum(), [leaves[n] for n in names])

    def composition(dtype, device, pose_mats):
        t = {n: leaves[n].detach().to(device=device, dtype=dtype).requires_grad_(True) for n in names}
        T34 = pose_mats(t["pose"].reshape(4, 6)).view(2, 2, 3, 4)
        loss = m.triangle_term_torch(t["disp_l"], t["disp_t"], t["disp_r"], T34, t["flow_bwd"], t["flow_fwd"],
                                     x["K"].to(device=device, dtype=dtype), x["Ki"].to(device=device, dtype=dtype), idx.to(device),
                                     pick.to(device))
        return torch.autograd.grad((loss * w.to(device=device, dtype=dtype)).sum(), [t[n] for n in names])
    yard = composition(torch.float32, dev(), lambda v: ops.PoseMatsFn.apply(v)[0])
    ref = composition(torch.float64, "cpu", O.pose_vec2mat)
    torch.cuda.synchronize()
    for n, g, y, r in zip(names, got, yard, ref):
        assert g.shape == r.shape and bool(torch.isfinite(g).all()), n
        scale = float(r.abs().max())
        ek = float((g.double().cpu() - r).abs().max()) / scale
        ey = float((y.double().cpu() - r).abs().max()) / scale
        print("EBOUND triangle_term 2x64x208 d%s kernel %.3e yardstick %.3e (max |ref| %.3e)" % (n, ek, ey, scale))
        assert scale > 0 and ek <= 4.0 * max(ey, 2.0 ** -24), (n, ek, ey)


def test_gradients_reach_every_input_and_repeat_bit_for_bit():
    def grads():
        _, x, lp = _run_stack(enable_triangle=True)
        lp["loss_triangle"].sum().backward()
        torch.cuda.synchronize()
        return dict(fb=x["fb"][0].grad, ff=x["ff"][0].grad, disp_l=x["disps"][0][0].grad, disp_t=x["disps"][1][0].grad,
                    disp_r=x["disps"][2][0].grad, pose=x["pose"].grad), lp["loss_triangle"].detach()
    a, la = grads()
    b, lb = grads()
    assert torch.equal(la, lb)
    for k in a:
        assert a[k] is not None and bool(torch.isfinite(a[k]).all()) and float(a[k].abs().max()) > 0, k
        assert torch.equal(a[k], b[k]), k
    assert float(a["pose"][:, 0].abs().max()) > 0 and float(a["pose"][:, 1].abs().max()) > 0        # both directions


def _full(enable, deterministic=False):
    before = convs.DETERMINISTIC
    convs.set_deterministic(deterministic)
    try:
        cfg = make_cfg(num_scales=3, img_hw=(256, 832), mode="geom", enable_triangle=enable, w_triangle=0.001)
        torch.manual_seed(0)
        model = get_model("geom")(cfg).to(dev()).train()
        opt = make_optimizer(model, 1e-4)
        inputs = [torch.from_numpy(a).to(dev()) for a in synthetic.make_triplet_batch(1, 256, 832, 3, seed=1)]
        torch.manual_seed(5)
        loss, lp, _ = train_step(model, opt, inputs, cfg)
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
        return float(loss), lp["loss_triangle"].detach().clone(), grads
    finally:
        convs.set_deterministic(before)


def test_one_eager_training_step_with_the_term():
    l_off, t_off, g_off = _full(False, deterministic=True)
    l_on, t_on, g_on = _full(True, deterministic=True)
    assert np.isfinite(l_on) and tuple(t_on.shape) == (1,) and bool(torch.isfinite(t_on).all())
    assert sorted(g_on) == sorted(g_off)
    for net in ("depth_net", "pose_net", "fpyramid", "pwc_model"):
        names = [n for n in g_on if n.startswith(net + ".")]
        assert names, net
        assert all(bool(torch.isfinite(g_on[n]).all()) for n in names), net
        assert any(not torch.equal(g_on[n], g_off[n]) for n in names), "%s: the term's gradient does not arrive" % net
    l_2, t_2, g_2 = _full(True, deterministic=True)            # deterministic mode: the same bits from the same seed
    assert l_2 == l_on and torch.equal(t_2, t_on)
    assert all(torch.equal(g_2[n], g_on[n]) for n in g_on)


def test_the_step_with_the_term_is_captured_and_replayed():
    cfg = make_cfg(num_scales=3, img_hw=(256, 832), mode="geom", enable_triangle=True, w_triangle=0.001)
    torch.manual_seed(0)
    model = get_model("geom")(cfg).to(dev()).train()
    opt = make_optimizer(model, 1e-4, capturable=True)
    batches = [[torch.from_numpy(a).to(dev()) for a in synthetic.make_triplet_batch(1, 256, 832, 3, seed=s)] for s in (1, 2)]
    g = GraphedTrainStep(model, opt, batches[0], cfg, warmup=1)
    try:
        seen = []
        for inp in (batches[1], batches[0]):
            loss, lp, _ = g(inp)
            torch.cuda.synchronize()
            assert np.isfinite(float(loss)) and bool(torch.isfinite(lp["loss_triangle"]).all()) and float(lp["loss_triangle"]) > 0
            seen.append(float(lp["loss_triangle"]))
        assert seen[0] != seen[1]                  # the new batch and a new draw reach the replay
    finally:
        del g
        torch.cuda.synchronize()
