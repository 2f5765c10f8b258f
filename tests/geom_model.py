"""The harness of the three model-level tests of the geometric terms (tests/test_hip_{triangle,eight_point,pnp}_model.py): a helper,
not a conftest.  ``Model_geometry.loss_stack`` on 2 x 64 x 208 loss-stack inputs without a network, a rigid scene of the terms'
cases on the device, and one 256 x 832 step eager and captured in a hipGraph."""
import copy

import numpy as np
import torch

from unsupervised_depth_opticalflow_egomotion_amd import convs, synthetic
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
from unsupervised_depth_opticalflow_egomotion_amd.train_step import GraphedTrainStep, make_cfg, make_optimizer, train_step


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


def _bare(beta=1, **switches):
    """Model_geometry without its networks (the loss stack needs none), the given ``enable_*`` switches set and no other."""
    m = get_model("geom").__new__(get_model("geom"))
    torch.nn.Module.__init__(m)
    cfg = make_cfg(**switches)
    m.dataset, m.num_scales = cfg.dataset, 3
    m.flow_consist_alpha, m.flow_consist_beta = cfg.flow_consist_alpha, cfg.flow_consist_beta
    m.ratio, m.num, m.beta = 0.3, 6000, beta
    m.enable_depth_ssim = m.enable_depth_consis = False
    for name, on in switches.items():
        setattr(m, name, on)
    return m


def _run_stack(seed=3, manual_seed=11, beta=1, **switches):
    x = _stack_inputs(seed)
    m = _bare(beta, **switches)
    torch.manual_seed(manual_seed)
    lp, _ = m.loss_stack(x["imgs"][0], x["imgs"][1], x["imgs"][2], x["disps"][0], x["disps"][1], x["disps"][2], x["pose"], x["fb"],
                         x["ff"], x["K"], x["Ki"])
    torch.cuda.synchronize()
    return m, x, lp


def _on_device(case, pose):
    g = lambda t: t.to(dev()).contiguous()   # noqa: E731
    return dict(disp=g(case["disp_t"]), fb=g(case["flow_bwd"]), ff=g(case["flow_fwd"]), K=g(case["K"]), Ki=g(case["K_inv"]),
                pose=g(pose).requires_grad_(True))


def captured_step_equals_the_eager_step(term, **switches):
    """One deterministic 256 x 832 step with ``switches`` on, replayed from a hipGraph, against the eager step of a twin model from
    the same weights and seed: ``lp[term]`` finite and nonzero, every term of the pack and the total bit-equal."""
    before = convs.DETERMINISTIC
    convs.set_deterministic(True)
    g = None
    try:
        cfg = make_cfg(num_scales=3, img_hw=(256, 832), mode="geom", **switches)
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
        assert bool(torch.isfinite(lp_g[term]).all()) and float(lp_g[term].abs().min()) > 0
        for k in lp_e:
            assert torch.equal(lp_g[k], lp_e[k].detach()), k
        assert float(loss_g.detach()) == float(loss_e.detach())
    finally:
        del g
        torch.cuda.synchronize()
        convs.set_deterministic(before)
