"""GPU: ``cfg.enable_pnp`` end to end, at the configurations tests/test_hip_eight_point_model.py uses -- Model_geometry.loss_stack with
and without the switch (2 x 64 x 208 loss-stack inputs, no network), the shared draw with all three geometric switches on, and one
256 x 832 step eager and captured in a hipGraph (capture raises on any host read: the no-host-sync proof)."""
import copy

import numpy as np
import pytest
import torch

from unsupervised_depth_opticalflow_egomotion_amd import convs, synthetic
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
from unsupervised_depth_opticalflow_egomotion_amd.train_step import DEFAULT_CFG, GraphedTrainStep, make_cfg, make_optimizer, total_loss, train_step

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _stack_inputs(seed=3):
    inp = synthetic.make_loss_stack_inputs(2, 64, 208, 3, seed=seed)

    def t(a, grad=True):
        x = torch.from_numpy(np.ascontiguousarray(a)).float().to(dev())
        return x.requires_grad_(True) if grad else x
    disps = [[t(a) for a in lst] for lst in inp.disps]
    return dict(imgs=[t(a, False) for a in inp.imgs], disps=disps, pose=t(inp.pose), fb=[t(a) for a in inp.flows_bwd],
                ff=[t(a) for a in inp.flows_fwd], K=t(inp.K, False), Ki=t(inp.K_inv, False))


def _bare(triangle, eight, pnp, beta=1):
    m = get_model("geom").__new__(get_model("geom"))        # the loss stack needs no network
    torch.nn.Module.__init__(m)
    cfg = make_cfg(enable_triangle=triangle, enable_eight_point=eight, enable_pnp=pnp)
    m.dataset, m.num_scales = cfg.dataset, 3
    m.flow_consist_alpha, m.flow_consist_beta = cfg.flow_consist_alpha, cfg.flow_consist_beta
    m.ratio, m.num, m.beta = 0.3, 6000, beta
    m.enable_depth_ssim = m.enable_depth_consis = False
    m.enable_triangle, m.enable_eight_point, m.enable_pnp = triangle, eight, pnp
    return m


def _run_stack(triangle, eight, pnp, seed=3, manual_seed=11, beta=1):
    x = _stack_inputs(seed)
    m = _bare(triangle, eight, pnp, beta)
    torch.manual_seed(manual_seed)
    lp, _ = m.loss_stack(x["imgs"][0], x["imgs"][1], x["imgs"][2], x["disps"][0], x["disps"][1], x["disps"][2], x["pose"], x["fb"],
                         x["ff"], x["K"], x["Ki"])
    torch.cuda.synchronize()
    return m, x, lp


def test_switch_off_the_pack_is_the_parents():
    """Off: the placeholder is still ``_zeros2``'s tagged tensor, and nothing of the pack depends on the new code -- the same
    bits as with the switch on, term by term, for every other key."""
    _, _, off = _run_stack(False, False, False)
    m, _, on = _run_stack(False, False, True)
    assert getattr(off["loss_pnp"], "_dfe_zero_placeholder", False) and tuple(off["loss_pnp"].shape) == (2,)
    assert float(off["loss_pnp"].detach().abs().max()) == 0.0
    assert list(on) == list(off)
    for k in on:
        if k != "loss_pnp":
            assert torch.equal(on[k].detach(), off[k].detach()), k
    assert torch.equal(on.rows[0], off.rows[0]) and on.rows[1] == off.rows[1]
    assert getattr(on["loss_triangle"], "_dfe_zero_placeholder", False) and getattr(on["loss_eight_point"], "_dfe_zero_placeholder", False)


def test_switch_on_the_term_is_finite_and_trains_the_pose_alone():
    m, x, on = _run_stack(False, False, True, beta=0.5)
    e = on["loss_pnp"]
    assert tuple(e.shape) == (2,) and e.grad_fn is not None and bool(torch.isfinite(e).all()) and float(e.detach().abs().min()) > 0
    assert not getattr(e, "_dfe_zero_placeholder", False)
    Pm = m.pnp_pose
    assert Pm.dtype == torch.float64 and tuple(Pm.shape) == (4, 6) and not Pm.requires_grad and bool(torch.isfinite(Pm).all())
    # the term is compute_pnp_loss's expression on the step's poses, beta = cfg.pose_beta
    pose = x["pose"].detach()
    want = sum((Pm[d * 2:(d + 1) * 2, :3].float() - pose[:, d, :3]).abs() + 0.5 * (Pm[d * 2:(d + 1) * 2, 3:].float() - pose[:, d, 3:]).abs()
               for d in range(2)).mean(1)
    assert torch.allclose(e.detach(), want, rtol=5e-6, atol=0)
    # every other weight zero: the total is w_pnp * mean(term), and only the pose receives a gradient
    zero = {a: 0.0 for a in DEFAULT_CFG if a.startswith("w_")}
    zero["w_pnp"] = 0.5
    cfg = make_cfg(enable_pnp=True, **zero)
    total = total_loss(on, cfg)
    assert float(total.detach()) == pytest.approx(0.5 * float(e.detach().mean()), rel=1e-6)
    e.sum().backward()
    torch.cuda.synchronize()
    g = x["pose"].grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g[:, 0].abs().max()) > 0 and float(g[:, 1].abs().max()) > 0
    for t in x["fb"] + x["ff"] + [d for lst in x["disps"] for d in lst]:
        assert t.grad is None                                       # the pose estimate is a constant: depth and flows get nothing


def test_pose_net_parameters_alone_receive_gradient_from_the_term():
    before = convs.DETERMINISTIC
    convs.set_deterministic(True)
    try:
        zero = {a: 0.0 for a in DEFAULT_CFG if a.startswith("w_")}
        zero["w_pnp"] = 0.1
        cfg = make_cfg(num_scales=3, img_hw=(256, 832), mode="geom", enable_pnp=True, **zero)
        torch.manual_seed(0)
        model = get_model("geom")(cfg).to(dev()).train()
        inputs = [torch.from_numpy(a).to(dev()) for a in synthetic.make_triplet_batch(1, 256, 832, 3, seed=1)]
        torch.manual_seed(5)
        lp, _ = model(inputs)
        term = lp["loss_pnp"]
        assert bool(torch.isfinite(term).all()) and float(term.detach().abs().max()) > 0
        names = [n for n, p in model.named_parameters() if p.requires_grad]
        grads = torch.autograd.grad(term.mean(), [p for _, p in model.named_parameters() if p.requires_grad], allow_unused=True)
        torch.cuda.synchronize()
        got = {n for n, g in zip(names, grads) if g is not None}
        assert got and all(n.startswith("pose_net.") for n in got), sorted(n for n in got if not n.startswith("pose_net."))[:4]
        pose_grads = [g for n, g in zip(names, grads) if g is not None]
        assert all(bool(torch.isfinite(g).all()) for g in pose_grads) and any(float(g.abs().max()) > 0 for g in pose_grads)
    finally:
        convs.set_deterministic(before)


def test_all_three_switches_share_one_selection_and_one_draw():
    def offset():
        return int(torch.cuda.get_rng_state(dev())[8:16].view(torch.int64))
    m1, _, two = _run_stack(True, True, False)
    off_two = offset()
    m2, _, three = _run_stack(True, True, True)
    off_three = offset()
    assert torch.equal(three["loss_triangle"].detach(), two["loss_triangle"].detach())              # the same bits
    assert torch.equal(three["loss_eight_point"].detach(), two["loss_eight_point"].detach())
    assert torch.equal(m1.triangle_draw[0], m2.triangle_draw[0]) and torch.equal(m1.triangle_draw[1], m2.triangle_draw[1])
    torch.manual_seed(11)
    torch.randint(0, int(0.3 * 64 * 208), [6000], device=dev())
    assert off_three == off_two == offset()                         # the generator advanced by exactly one draw
    assert float(three["loss_pnp"].detach().abs().min()) > 0
    m3, _, alone = _run_stack(False, False, True)
    assert torch.equal(three["loss_pnp"].detach(), alone["loss_pnp"].detach()) and torch.equal(m2.pnp_pose, m3.pnp_pose)


def test_the_step_with_the_term_is_captured_and_equals_the_eager_step():
    before = convs.DETERMINISTIC
    convs.set_deterministic(True)
    g = None
    try:
        cfg = make_cfg(num_scales=3, img_hw=(256, 832), mode="geom", enable_pnp=True)
        torch.manual_seed(0)
        model = get_model("geom")(cfg).to(dev()).train()
        init = copy.deepcopy(model.state_dict())
        opt = make_optimizer(model, 1e-4, capturable=True)
        batch = [torch.from_numpy(a).to(dev()) for a in synthetic.make_triplet_batch(1, 256, 832, 3, seed=1)]
        g = GraphedTrainStep(model, opt, batch, cfg, warmup=1)
        torch.manual_seed(5)
        loss_g, lp_g, _ = g(batch)
        torch.cuda.synchronize()
        lp_g = {k: v.detach().clone() for k, v in lp_g.items()}
        twin = get_model("geom")(cfg).to(dev()).train()
        twin.load_state_dict(init)
        opt_t = make_optimizer(twin, 1e-4)
        torch.manual_seed(5)
        loss_e, lp_e, _ = train_step(twin, opt_t, batch, cfg)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(lp_g["loss_pnp"]).all()) and float(lp_g["loss_pnp"].abs().min()) > 0
        for k in lp_e:
            assert torch.equal(lp_g[k], lp_e[k].detach()), k
        assert float(loss_g.detach()) == float(loss_e.detach())
    finally:
        del g
        torch.cuda.synchronize()
        convs.set_deterministic(before)
