"""GPU: ``cfg.enable_pnp`` end to end, at the configurations tests/test_hip_eight_point_model.py uses -- Model_geometry.loss_stack with
and without the switch (2 x 64 x 208 loss-stack inputs, no network), the shared draw with all three geometric switches on, and one
256 x 832 step eager and captured in a hipGraph (capture raises on any host read: the no-host-sync proof)."""
import pytest
import torch

from tests import pnp_cases as PC
from tests.geom_model import _bare, _on_device, _run_stack, captured_step_equals_the_eager_step, dev
from unsupervised_depth_opticalflow_egomotion_amd import convs, synthetic
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
from unsupervised_depth_opticalflow_egomotion_amd.train_step import DEFAULT_CFG, make_cfg, total_loss

pytestmark = pytest.mark.gpu


def test_switch_off_the_pack_is_the_parents():
    """Off: the placeholder is still ``_zeros2``'s tagged tensor, and nothing of the pack depends on the new code -- the same
    bits as with the switch on, term by term, for every other key."""
    _, _, off = _run_stack(enable_triangle=False, enable_eight_point=False, enable_pnp=False)
    m, _, on = _run_stack(enable_triangle=False, enable_eight_point=False, enable_pnp=True)
    assert getattr(off["loss_pnp"], "_dfe_zero_placeholder", False) and tuple(off["loss_pnp"].shape) == (2,)
    assert float(off["loss_pnp"].detach().abs().max()) == 0.0
    assert list(on) == list(off)
    for k in on:
        if k != "loss_pnp":
            assert torch.equal(on[k].detach(), off[k].detach()), k
    assert torch.equal(on.rows[0], off.rows[0]) and on.rows[1] == off.rows[1]
    assert getattr(on["loss_triangle"], "_dfe_zero_placeholder", False) and getattr(on["loss_eight_point"], "_dfe_zero_placeholder", False)


def test_switch_on_the_term_is_finite_and_trains_the_pose_alone():
    m, x, on = _run_stack(enable_triangle=False, enable_eight_point=False, enable_pnp=True, beta=0.5)
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
    m1, _, two = _run_stack(enable_triangle=True, enable_eight_point=True, enable_pnp=False)
    off_two = offset()
    m2, _, three = _run_stack(enable_triangle=True, enable_eight_point=True, enable_pnp=True)
    off_three = offset()
    assert torch.equal(three["loss_triangle"].detach(), two["loss_triangle"].detach())              # the same bits
    assert torch.equal(three["loss_eight_point"].detach(), two["loss_eight_point"].detach())
    assert torch.equal(m1.triangle_draw[0], m2.triangle_draw[0]) and torch.equal(m1.triangle_draw[1], m2.triangle_draw[1])
    torch.manual_seed(11)
    torch.randint(0, int(0.3 * 64 * 208), [6000], device=dev())
    assert off_three == off_two == offset()                         # the generator advanced by exactly one draw
    assert float(three["loss_pnp"].detach().abs().min()) > 0
    m3, _, alone = _run_stack(enable_triangle=False, enable_eight_point=False, enable_pnp=True)
    assert torch.equal(three["loss_pnp"].detach(), alone["loss_pnp"].detach()) and torch.equal(m2.pnp_pose, m3.pnp_pose)


def test_the_step_with_the_term_is_captured_and_equals_the_eager_step():
    captured_step_equals_the_eager_step("loss_pnp", enable_pnp=True)


# ------------------------------------------------------------------------------------------------ the term through models.py
# A rigid scene of tests/pnp_cases.py (its depth map as the disparity, its flows, a camera matrix per sample) through
# ``geometric_draw`` and ``pnp_term``: the draw's wiring by bits -- line 509's ``K[0]`` for every sample included, which a case with
# one K per sample can tell from ``K[b]`` -- the loss and the pose gradient against float64 autograd of compute_pnp_loss's
# expression ((T, axis-angle) against (translation, Euler), beta = 0.5) with the kernel's own P64 as the constant target.
LOSS_TOL, GRAD_TOL = 5e-6, 2e-5           # the kernel-level test's (tests/test_hip_pnp.py)
MODEL_SCENES = ((2, 12, 20), (3, 12, 20))
MODEL_BETA = 0.5


def _scene(shape):
    B, H, W = shape
    case = PC.build(0, B, H, W, int(0.3 * H * W), 64, 64, True)
    m = _bare(enable_triangle=False, enable_eight_point=False, enable_pnp=True, beta=MODEL_BETA)
    m.ratio, m.num, m.ransac_iters = 0.3, 64, 64
    return case, PC.pose_vectors(case), m


@pytest.mark.parametrize("shape", MODEL_SCENES)
def test_the_term_is_the_operator_on_the_models_own_draw_with_the_first_camera(shape):
    """After the same seed, ``geometric_draw`` followed by a direct ``pnp_ransac`` on ``minimal_sets_device(k=6)`` with
    ``K[:1].expand(B, 3, 3)`` gives the bits of ``pnp_term(..., return_pose=True)``; the call with ``K`` itself does not."""
    from unsupervised_depth_opticalflow_egomotion_amd import pnp
    case, pose, m = _scene(shape)
    B = case["B"]
    x = _on_device(case, pose)
    assert not torch.equal(case["K"][0], case["K"][1])
    torch.manual_seed(7)
    idx, pick = m.geometric_draw(x["disp"], x["pose"], x["fb"], x["ff"], x["K"])
    assert tuple(idx.shape) == (2 * B, 72) and tuple(pick.shape) == (64,) and pick.unique().numel() < 64
    sets = m.minimal_sets_device(B, 64, dev(), k=6)
    assert tuple(sets.shape) == (B, 64, 6)
    K0 = x["K"][:1].expand(B, 3, 3).contiguous()
    P32, P64, info = pnp.pnp_ransac(x["fb"], x["ff"], x["disp"], idx, pick, sets, K0, x["Ki"], iters=20, thresh=1.0)
    _, own, _ = pnp.pnp_ransac(x["fb"], x["ff"], x["disp"], idx, pick, sets, x["K"], x["Ki"], iters=20, thresh=1.0)
    direct = pnp.PnpLossFn.apply(x["pose"], P32, MODEL_BETA)
    torch.manual_seed(7)
    loss, P64m = m.pnp_term(x["disp"], x["pose"], x["fb"], x["ff"], x["K"], x["Ki"], return_pose=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(P64).all())
    assert torch.equal(P64m.view(torch.int64), P64.view(torch.int64)) and torch.equal(loss.detach().view(torch.int32), direct.detach().view(torch.int32))
    planes = [d * B + b for d in range(2) for b in range(1, B)]      # every sample but the first sees another camera
    assert not torch.equal(own[planes], P64m[planes]) and torch.equal(own[[0, B]], P64m[[0, B]])
    torch.manual_seed(8)                                            # another seed, another draw
    _, other = m.pnp_term(x["disp"], x["pose"], x["fb"], x["ff"], x["K"], x["Ki"], return_pose=True)
    assert not torch.equal(other, P64)


@pytest.mark.parametrize("shape", MODEL_SCENES)
def test_the_term_and_its_pose_gradient_equal_float64_autograd_of_the_reference_expression(shape):
    WEIGHTS_OF, _loss_reference = PC.WEIGHTS_OF, PC.loss_reference
    case, pose, m = _scene(shape)
    B = case["B"]
    x = _on_device(case, pose)
    w = torch.tensor(WEIGHTS_OF[B])
    torch.manual_seed(7)
    loss, P64 = m.pnp_term(x["disp"], x["pose"], x["fb"], x["ff"], x["K"], x["Ki"], return_pose=True)
    (loss * w.to(dev())).sum().backward()
    torch.cuda.synchronize()
    P64 = P64.cpu()
    l64, g64 = _loss_reference(P64, pose, MODEL_BETA, w)
    l32, g32 = _loss_reference(P64, pose, MODEL_BETA, w, dtype=torch.float32)
    fl = float(((l32.double() - l64).abs() / l64.abs()).max())
    fg = float((g32.double() - g64).abs().max() / g64.abs().max())
    el = float(((loss.detach().double().cpu() - l64).abs() / l64.abs()).max())
    eg = float((x["pose"].grad.double().cpu() - g64).abs().max() / g64.abs().max())
    print("EBOUND pnp model %dx%dx%d: loss %.3e (%g)  dpose %.3e (%g); the reference expression in fp32 on the CPU against float64: "
          "loss %.3e  dpose %.3e" % (shape + (el, LOSS_TOL, eg, GRAD_TOL, fl, fg)))
    assert tuple(loss.shape) == (B,) and el <= LOSS_TOL and eg <= GRAD_TOL
    # the case tells the orderings apart with the kernel's own target: the directions' planes exchanged, or pose row d*B + b
    swapped = _loss_reference(torch.cat([P64[B:], P64[:B]], 0), pose, MODEL_BETA, w)[0]
    rows = _loss_reference(P64, pose.reshape(2, B, 6).permute(1, 0, 2).contiguous(), MODEL_BETA, w)[0]
    assert float(((swapped - l64).abs() / l64).max()) > 100 * LOSS_TOL and float(((rows - l64).abs() / l64).max()) > 100 * LOSS_TOL
