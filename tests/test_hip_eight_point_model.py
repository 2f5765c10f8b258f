"""GPU: ``cfg.enable_eight_point`` end to end, at the configurations tests/test_hip_triangle_model.py uses -- Model_geometry.loss_stack
with and without the switch (2 x 64 x 208 loss-stack inputs, no network), the shared draw with both geometric switches on, and
one 256 x 832 step eager and captured in a hipGraph (capture raises on any host read: the no-host-sync proof)."""
import numpy as np
import pytest
import torch

from tests import eight_point_cases as EC
from tests.geom_model import _bare, _on_device, _run_stack, captured_step_equals_the_eager_step, dev
from unsupervised_depth_opticalflow_egomotion_amd import convs, synthetic
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
from unsupervised_depth_opticalflow_egomotion_amd.train_step import DEFAULT_CFG, make_cfg, make_optimizer, total_loss, train_step

pytestmark = pytest.mark.gpu


def test_switch_off_the_pack_is_the_parents():
    """Off: the placeholder is still ``_zeros2``'s tagged tensor, and nothing of the pack depends on the new code -- the same
    bits as with the switch on, term by term, for every other key."""
    _, _, off = _run_stack(enable_triangle=False, enable_eight_point=False)
    m, _, on = _run_stack(enable_triangle=False, enable_eight_point=True)
    assert getattr(off["loss_eight_point"], "_dfe_zero_placeholder", False) and tuple(off["loss_eight_point"].shape) == (2,)
    assert float(off["loss_eight_point"].detach().abs().max()) == 0.0
    assert list(on) == list(off)
    for k in on:
        if k != "loss_eight_point":
            assert torch.equal(on[k].detach(), off[k].detach()), k
    assert torch.equal(on.rows[0], off.rows[0]) and on.rows[1] == off.rows[1]
    assert getattr(on["loss_triangle"], "_dfe_zero_placeholder", False)


def test_switch_on_the_term_is_finite_and_trains_the_pose_alone():
    m, x, on = _run_stack(enable_triangle=False, enable_eight_point=True)
    e = on["loss_eight_point"]
    assert tuple(e.shape) == (2,) and e.grad_fn is not None and bool(torch.isfinite(e).all()) and float(e.detach().abs().min()) > 0
    assert not getattr(e, "_dfe_zero_placeholder", False)
    F = m.eight_point_F
    assert F.dtype == torch.float64 and tuple(F.shape) == (4, 3, 3) and not F.requires_grad and bool((F[:, 2, 2] == 1.0).all())
    # every other weight zero: the total is w_8point * mean(term), and only the pose receives a gradient
    zero = {a: 0.0 for a in DEFAULT_CFG if a.startswith("w_")}
    zero["w_8point"] = 0.5
    cfg = make_cfg(enable_eight_point=True, **zero)
    total = total_loss(on, cfg)
    assert float(total.detach()) == pytest.approx(0.5 * float(e.detach().mean()), rel=1e-6)
    e.sum().backward()
    torch.cuda.synchronize()
    g = x["pose"].grad
    assert g is not None and bool(torch.isfinite(g).all()) and float(g[:, 0].abs().max()) > 0 and float(g[:, 1].abs().max()) > 0
    for t in x["fb"] + x["ff"] + [d for lst in x["disps"] for d in lst]:
        assert t.grad is None                                       # F is a constant: the matches get nothing


def test_a_pose_net_parameter_receives_gradient_from_the_term_alone():
    before = convs.DETERMINISTIC
    convs.set_deterministic(True)
    try:
        zero = {a: 0.0 for a in DEFAULT_CFG if a.startswith("w_")}
        zero["w_8point"] = 0.1
        cfg = make_cfg(num_scales=3, img_hw=(256, 832), mode="geom", enable_eight_point=True, **zero)
        torch.manual_seed(0)
        model = get_model("geom")(cfg).to(dev()).train()
        opt = make_optimizer(model, 1e-4)
        inputs = [torch.from_numpy(a).to(dev()) for a in synthetic.make_triplet_batch(1, 256, 832, 3, seed=1)]
        torch.manual_seed(5)
        loss, lp, _ = train_step(model, opt, inputs, cfg)
        torch.cuda.synchronize()
        assert np.isfinite(float(loss)) and float(lp["loss_eight_point"].detach().abs().max()) > 0
        pose_grads = [p.grad for n, p in model.named_parameters() if n.startswith("pose_net.") and p.grad is not None]
        assert pose_grads and all(bool(torch.isfinite(g).all()) for g in pose_grads) and any(float(g.abs().max()) > 0 for g in pose_grads)
    finally:
        convs.set_deterministic(before)


def test_both_switches_share_one_selection_and_one_draw():
    def offset():
        return int(torch.cuda.get_rng_state(dev())[8:16].view(torch.int64))
    m1, _, tri_only = _run_stack(enable_triangle=True, enable_eight_point=False)
    off_tri = offset()
    m2, _, both = _run_stack(enable_triangle=True, enable_eight_point=True)
    off_both = offset()
    assert torch.equal(both["loss_triangle"].detach(), tri_only["loss_triangle"].detach())          # the same bits
    assert torch.equal(m1.triangle_draw[0], m2.triangle_draw[0]) and torch.equal(m1.triangle_draw[1], m2.triangle_draw[1])
    torch.manual_seed(11)
    torch.randint(0, int(0.3 * 64 * 208), [6000], device=dev())
    assert off_both == off_tri == offset()                          # the generator advanced by exactly one draw
    assert float(both["loss_eight_point"].detach().abs().min()) > 0
    _, _, eight_only = _run_stack(enable_triangle=False, enable_eight_point=True)
    assert torch.equal(both["loss_eight_point"].detach(), eight_only["loss_eight_point"].detach())


def test_the_step_with_the_term_is_captured_and_equals_the_eager_step():
    captured_step_equals_the_eager_step("loss_eight_point", enable_eight_point=True)


# ------------------------------------------------------------------------------------------------ the term through models.py
# A rigid scene of tests/eight_point_cases.py (its depth map as the disparity, its flows, a camera matrix per sample) through
# ``geometric_draw`` and ``eight_point_term``: the draw's wiring by bits, the loss and the pose gradient against float64 autograd
# of compute_eight_point_loss's expression on the oracle's [t]x R with the kernel's own F64 as the constant target.  The pose's
# translation is scaled by 40 (as the kernel-level loss test's second scale): at scale 1 every |F_pred - F| lies beyond smooth-L1's
# knee for sample 0 and exchanging the two directions' targets moves its loss by 6e-6 only; at 40 both orderings are visible.
# "Visible": some sample's loss moves by more than 100 x LOSS_TOL (the largest move over the samples; at B = 3 one sample moves by
# 2.7e-4 only under the exchange), which is what a per-sample comparison at LOSS_TOL needs.
LOSS_TOL, GRAD_TOL = 5e-6, 2e-5           # the kernel-level test's (tests/test_hip_eight_point.py)
MODEL_SCENES = ((2, 12, 20), (3, 12, 20))


def _scene(shape):
    B, H, W = shape
    case = EC.build(0, B, H, W, int(0.3 * H * W), 64, 64, True)
    pose = EC.pose_vectors(case)
    pose[:, :, :3] *= 40.0
    m = _bare(enable_triangle=False, enable_eight_point=True)
    m.ratio, m.num, m.ransac_iters = 0.3, 64, 64
    return case, pose, m


@pytest.mark.parametrize("shape", MODEL_SCENES)
def test_the_term_is_the_operator_on_the_models_own_draw(shape):
    """After the same seed, ``geometric_draw`` followed by a direct ``fundamental_ransac`` on ``minimal_sets_device`` gives the bits
    of ``eight_point_term(..., return_F=True)``; the draw is with replacement."""
    from unsupervised_depth_opticalflow_egomotion_amd import eight_point, ops
    case, pose, m = _scene(shape)
    B = case["B"]
    x = _on_device(case, pose)
    torch.manual_seed(7)
    idx, pick = m.geometric_draw(x["disp"], x["pose"], x["fb"], x["ff"], x["K"])
    assert tuple(idx.shape) == (2 * B, 72) and tuple(pick.shape) == (64,) and pick.unique().numel() < 64
    sets = m.minimal_sets_device(B, 64, dev())
    assert tuple(sets.shape) == (B, 64, 8)
    F32, F64, info = eight_point.fundamental_ransac(x["fb"], x["ff"], idx, pick, sets, 0.1)
    direct = eight_point.EightPointLossFn.apply(ops.PoseMatsFn.apply(x["pose"].reshape(2 * B, 6))[1], x["K"], x["Ki"], F32)
    torch.manual_seed(7)
    loss, F64m = m.eight_point_term(x["disp"], x["pose"], x["fb"], x["ff"], x["K"], x["Ki"], return_F=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(F64).all()) and int(info[:, 1].min()) >= 8
    assert torch.equal(F64m.view(torch.int64), F64.view(torch.int64)) and torch.equal(loss.detach().view(torch.int32), direct.detach().view(torch.int32))
    torch.manual_seed(8)                                            # another seed, another draw
    _, other = m.eight_point_term(x["disp"], x["pose"], x["fb"], x["ff"], x["K"], x["Ki"], return_F=True)
    assert not torch.equal(other, F64)


@pytest.mark.parametrize("shape", MODEL_SCENES)
def test_the_term_and_its_pose_gradient_equal_float64_autograd_of_the_reference_expression(shape):
    WEIGHTS_OF, _loss_reference = EC.WEIGHTS_OF, EC.loss_reference
    case, pose, m = _scene(shape)
    B = case["B"]
    x = _on_device(case, pose)
    w = torch.tensor(WEIGHTS_OF[B])
    torch.manual_seed(7)
    loss, F64 = m.eight_point_term(x["disp"], x["pose"], x["fb"], x["ff"], x["K"], x["Ki"], return_F=True)
    (loss * w.to(dev())).sum().backward()
    torch.cuda.synchronize()
    F64 = F64.cpu()
    l64, g64, _ = _loss_reference(F64, case["K"], case["K_inv"], pose, w)
    l32, g32, _ = _loss_reference(F64, case["K"], case["K_inv"], pose, w, dtype=torch.float32)
    fl = float(((l32.double() - l64).abs() / l64.abs()).max())
    fg = float((g32.double() - g64).abs().max() / g64.abs().max())
    el = float(((loss.detach().double().cpu() - l64).abs() / l64.abs()).max())
    eg = float((x["pose"].grad.double().cpu() - g64).abs().max() / g64.abs().max())
    print("EBOUND eight_point model %dx%dx%d: loss %.3e (%g)  dpose %.3e (%g); the reference expression in fp32 on the CPU against "
          "float64: loss %.3e  dpose %.3e" % (shape + (el, LOSS_TOL, eg, GRAD_TOL, fl, fg)))
    assert tuple(loss.shape) == (B,) and el <= LOSS_TOL and eg <= GRAD_TOL
    # the case tells the orderings apart with the kernel's own target: the directions' planes exchanged, or E's row d*B + b
    swapped = _loss_reference(torch.cat([F64[B:], F64[:B]], 0), case["K"], case["K_inv"], pose, w)[0]
    rows = _loss_reference(F64, case["K"], case["K_inv"], pose.reshape(2, B, 6).permute(1, 0, 2).contiguous(), w)[0]
    assert float(((swapped - l64).abs() / l64).max()) > 100 * LOSS_TOL and float(((rows - l64).abs() / l64).max()) > 100 * LOSS_TOL
