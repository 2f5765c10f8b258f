"""GPU: the deterministic mode end to end (convs.set_deterministic, README "Reproducible").  Under the mode no convolution of a
forward + backward pass of any of the three models reaches ATen / MIOpen; loss pack, every network's outputs and every
parameter's gradient repeat bit for bit across runs, across a churned allocator and across ``net_streams`` 1 and 3; two optimiser
steps repeat; the gradients are those of the default mode's network up to the default mode's own run-to-run noise; the mode's
doors compute the float64 convolution; and ``train.py --deterministic`` prints the same loss lines in two fresh processes."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

from unsupervised_depth_opticalflow_egomotion_amd import convs, synthetic
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg, make_optimizer, total_loss, train_step

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("geom", "depth", "flow")


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def mode_on():
    before = convs.DETERMINISTIC
    convs.set_deterministic(True)
    yield
    convs.set_deterministic(before)


class AtenConvolutions(TorchDispatchMode):
    """counts every ATen convolution operator that is dispatched (as tools/conv_census.py does)"""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func._schema.name
        if name.startswith(("aten::convolution", "aten::miopen_", "aten::_convolution", "aten::cudnn_convolution", "aten::conv")):
            self.seen.append(name)
        return func(*args, **(kwargs or {}))


def _model(mode, streams=1):
    cfg = make_cfg(num_scales=3, img_hw=(256, 832), mode=mode)          # PoseCNN's Linear(14, 14) fixes the frame size
    torch.manual_seed(0)
    model = get_model(mode)(cfg).to(dev()).train()
    model.net_streams = streams
    inputs = [torch.from_numpy(a).to(dev()) for a in synthetic.make_triplet_batch(1, 256, 832, 3, seed=1)]
    return cfg, model, inputs


@pytest.mark.parametrize("mode", MODES)
def test_nothing_reaches_atens_convolutions(mode, mode_on):
    cfg, model, inputs = _model(mode)
    with AtenConvolutions() as seen:
        lp, _ = model(inputs)
        total_loss(lp, cfg).backward()
    torch.cuda.synchronize()
    assert seen.seen == [], sorted(set(seen.seen))
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def _tensors(out, prefix, into):
    if isinstance(out, torch.Tensor):
        into[prefix] = out.detach().clone()
    elif isinstance(out, (tuple, list)):
        for i, o in enumerate(out):
            _tensors(o, "%s.%d" % (prefix, i), into)
    elif isinstance(out, dict):
        for k, o in out.items():
            _tensors(o, "%s.%s" % (prefix, k), into)


def _churn(seed):
    """a few dozen odd-sized tensors allocated and freed, then the cache dropped: the next pass gets other blocks"""
    gen = torch.Generator().manual_seed(seed)
    junk = [torch.empty(int(torch.randint(1 << 8, 1 << 22, (1,), generator=gen)) | 1, device=dev()) for _ in range(40)]
    del junk[::2]
    keep = torch.empty((1 << 20) + 3, device=dev())
    del junk
    torch.cuda.empty_cache()
    return keep


def _pass(mode, streams, churn=None):
    """one forward + backward from the seed: {name: tensor} of the loss pack, of every network's outputs (the disparity lists, the
    flows, the pose vectors: whatever the model's sub-networks return) and of every parameter's gradient"""
    keep = _churn(churn) if churn is not None else None
    cfg, model, inputs = _model(mode, streams)
    got = {}
    calls = {}

    def hook(name):
        def fn(_mod, _inp, out):
            calls[name] = calls.get(name, 0) + 1
            _tensors(out, "out.%s.%d" % (name, calls[name]), got)
        return fn
    for name, m in model.named_children():
        if next(m.parameters(), None) is not None:
            m.register_forward_hook(hook(name))
    lp, _ = model(inputs)
    loss = total_loss(lp, cfg)
    loss.backward()
    torch.cuda.synchronize()
    got["loss"] = loss.detach().clone()
    _tensors(dict(lp), "loss_pack", got)
    n_grads = 0
    for name, p in model.named_parameters():
        if p.grad is not None:
            got["grad." + name] = p.grad.detach().clone()
            n_grads += 1
    assert n_grads > 50 and any(k.startswith("out.") for k in got), sorted(got)[:8]
    del keep
    return got


def _assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b), (what, sorted(set(a) ^ set(b))[:8])
    differ = [k for k in sorted(a) if not torch.equal(a[k], b[k])]
    assert not differ, (what, len(differ), [(k, float((a[k].double() - b[k].double()).abs().max())) for k in differ[:6]])
    assert all(bool(torch.isfinite(v).all()) for v in a.values()), what


@pytest.mark.parametrize("mode", MODES)
def test_the_step_repeats_bit_for_bit(mode, mode_on):
    first = _pass(mode, 1)
    assert any("pose" in k for k in first if k.startswith("out.")) or mode == "flow"
    _assert_same_bits(first, _pass(mode, 1, churn=5), "%s: a churned allocator" % mode)
    _assert_same_bits(first, _pass(mode, 3), "%s: three network streams" % mode)


def test_two_optimiser_steps_repeat(mode_on):
    def two_steps(churn):
        keep = _churn(churn) if churn is not None else None
        cfg, model, inputs = _model("geom")
        opt = make_optimizer(model, 1e-4)
        losses = [train_step(model, opt, inputs, cfg)[0].detach().clone() for _ in range(2)]
        torch.cuda.synchronize()
        del keep
        return dict({"param." + n: p.detach().clone() for n, p in model.named_parameters()}, loss0=losses[0], loss1=losses[1])
    _assert_same_bits(two_steps(None), two_steps(9), "two optimiser steps")


def test_same_network_as_the_default_mode():
    """The yardstick of test_network_streams_do_not_change_results, measured here: 4 x the default mode's own run-to-run difference
    or 1e-3 of the gradient scale, whichever is larger."""
    before = convs.DETERMINISTIC

    def flat(p):
        return torch.cat([p[k].flatten() for k in sorted(p) if k.startswith("grad.")])
    try:
        convs.set_deterministic(False)
        a, a2 = _pass("geom", 1), _pass("geom", 1)
        convs.set_deterministic(True)
        d = _pass("geom", 1)
    finally:
        convs.set_deterministic(before)
    assert [k for k in sorted(a) if k.startswith("grad.")] == [k for k in sorted(d) if k.startswith("grad.")]
    scale, noise, diff = float(flat(a).abs().max()), float((flat(a2) - flat(a)).abs().max()), float((flat(d) - flat(a)).abs().max())
    print("\ndeterministic vs default: grad scale %.3e, default run-to-run %.3e, deterministic vs default %.3e" % (scale, noise, diff))
    assert diff <= max(4.0 * noise, 1e-3 * scale), (diff, noise, scale)
    assert abs(float(d["loss"]) - float(a["loss"])) <= 1e-4 * abs(float(a["loss"]))


# door, x shape, filter shape, (stride, padding, dilation), slope, bias, fuse, the plan
DOORS = {
    "stem_7x7": ("module", (2, 3, 32, 52), (64, 3, 7, 7), (2, 3, 1), None, False, None, ("sconv", "none", "sconv_wgrad")),
    "strided_5x5_fused": ("conv_act", (2, 16, 16, 26), (32, 16, 5, 5), (2, 2, 1), 0.0, True, ("plane", "conv1x1", "sconv_act"), ("sconv_act", "sconv", "sconv_wgrad")),
    "strided_3x3_fused": ("conv_act", (3, 96, 8, 26), (128, 96, 3, 3), (2, 1, 1), 0.1, True, ("plane", "wino_act", "sconv_act"), ("sconv_act", "sconv", "sconv_wgrad")),
    "strided_3x3_unfused": ("conv_act", (1, 32, 7, 9), (64, 32, 3, 3), (2, 1, 1), 0.1, True, ("plane", "wino_act"), ("sconv", "sconv", "sconv_wgrad")),
    "strided_3x3_module": ("module", (2, 64, 10, 14), (128, 64, 3, 3), (2, 1, 1), None, False, None, ("sconv", "sconv", "sconv_wgrad")),
    "shortcut_1x1": ("module", (3, 64, 9, 14), (128, 64, 1, 1), (2, 0, 1), None, False, None, ("conv1x1s2", "sconv", "conv1x1s2")),
    "few_tiles_3x3": ("module", (1, 40, 8, 26), (24, 40, 3, 3), (1, 1, 1), None, True, None, ("wino", "wino", "wino_wgrad")),
    "dilated_16": ("conv_act", (1, 24, 32, 48), (16, 24, 3, 3), (1, 16, 16), 0.1, True, ("plane", "wino_act"), ("wino_act", "wino", "wino_wgrad")),
    "prepadded_small": ("conv3x3_valid", (1, 48, 10, 28), (24, 48, 3, 3), (1, 0, 1), None, False, None, ("wino", "wino", "wino_wgrad")),
}


@pytest.mark.parametrize("case", sorted(DOORS))
def test_the_modes_doors_compute_the_convolution(case, mode_on):
    """every route the mode adds, through its real door, forward and backward against the float64 ``F.conv2d`` graph (5e-5 of the
    reference's maximum, the tolerance of tests/test_hip_conv_route.py), with no ATen convolution on the way"""
    door, xs, ws, (s, p, d), slope, bias, fuse, expected = DOORS[case]
    torch.manual_seed(sum(xs) + sum(ws))
    image = expected[1] == "none"
    x = torch.randn(*xs, device=dev(), requires_grad=not image)
    conv = convs.Conv2d(ws[1], ws[0], ws[2], s, p, d, bias=bias).to(dev())
    w, b = conv.weight, conv.bias
    if door == "module":
        plan = convs.plan(x, w.shape, s, p, d, 1, bias, ctx="module")
        run = lambda: conv(x)                                                                          # noqa: E731
    elif door == "conv_act":
        plan = convs.plan(x, w.shape, s, p, d, 1, True, slope != 1.0, "conv_act", fuse)
        run = lambda: convs.conv_act(x, conv, slope, fuse)                                             # noqa: E731
    else:
        plan = convs.plan(x, w.shape, ctx="prepadded")
        run = lambda: convs.conv3x3_valid(x, w)                                                        # noqa: E731
    assert tuple(plan) == expected
    with AtenConvolutions() as seen:
        y = run()
        g = torch.randn_like(y)
        y.backward(g)
    assert seen.seen == []
    xd, wd = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    bd = b.detach().double().requires_grad_(True) if b is not None else None
    yd = F.conv2d(xd, wd, bd, s, p, d)
    yd = yd if slope is None else F.leaky_relu(yd, slope)
    yd.backward(g.double())
    pairs = [("y", y.detach(), yd.detach()), ("gw", w.grad, wd.grad)] + ([] if image else [("gx", x.grad, xd.grad)]) + ([("gb", b.grad, bd.grad)] if bias else [])
    for name, a, ref in pairs:
        assert float((a.double() - ref).abs().max()) <= 5e-5 * float(ref.abs().max()), (case, name)


def test_a_missing_data_gradient_raises_instead_of_falling_back(mode_on):
    from unsupervised_depth_opticalflow_egomotion_amd._lib import DfeError
    x = torch.randn(1, 9, 32, 52, device=dev(), requires_grad=True)          # a 7x7 stem whose input is NOT an image
    conv = convs.Conv2d(9, 16, 7, 2, 3).to(dev())
    y = conv(x)
    with pytest.raises(DfeError, match="data gradient"):
        y.sum().backward()
    with pytest.raises(DfeError, match="groups 2"):
        convs.conv2d(x[:, :8], torch.randn(16, 4, 3, 3, device=dev()), None, 1, 1, 1, 2)


def test_train_cli_prints_the_same_losses_in_two_processes(tmp_path):
    base = [sys.executable, os.path.join(REPO, "train.py"), "-c", os.path.join(REPO, "config", "kitti_geom.yaml"), "--mode", "geom",
            "--batch_size", "1", "--log_interval", "1", "--save_interval", "1000", "--deterministic", "--num_iterations", "2"]
    env = {k: v for k, v in os.environ.items() if k != "DFE_DETERMINISTIC"}
    runs = []
    for i in range(2):
        out = subprocess.run(base + ["--model_dir", str(tmp_path / ("run%d" % i))], capture_output=True, text=True, cwd=REPO, env=env, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        runs.append([line for line in out.stdout.splitlines() if line.startswith("iter ")])
    assert len(runs[0]) == 2 and runs[0] == runs[1], runs
