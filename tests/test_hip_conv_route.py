"""GPU: what convs.plan names is what runs.  A handful of layers, the smallest that still cross each routing threshold, go through
their real doors (convs.conv2d, convs.conv_act, convs.conv3x3_valid) forward and backward; the ops wrappers are wrapped in call
counters and a TorchDispatchMode (as in tools/conv_census.py) counts aten::convolution / aten::convolution_backward per pass.
The kernels that ran are the plan's, and values and gradients match the float64 ``F.conv2d`` graph to 5e-5 of the reference's
maximum (the tolerance tests/test_hip_sconv.py uses for the same comparison)."""
import pytest
import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

from unsupervised_depth_opticalflow_egomotion_amd import convs, ops

pytestmark = pytest.mark.gpu


class Ran(TorchDispatchMode):
    """the kernel(s) seen per pass: {"fwd": set, "dgrad": set, "wgrad": set}"""

    def __init__(self, monkeypatch):
        super().__init__()
        self.seen = {"fwd": set(), "dgrad": set(), "wgrad": set()}

        def wrap(name, note):
            orig = getattr(ops, name)

            def counted(*a, **kw):
                note(*a, **kw)
                return orig(*a, **kw)
            monkeypatch.setattr(ops, name, counted)

        def wino(x, w, padding=1, transposed=False, dilation=1, bias=None, slope=1.0, out=None, out_off=0, out2=None, out2_off=0):
            fused = bias is not None or float(slope) != 1.0 or out is not None or out2 is not None
            self.seen["dgrad" if transposed else "fwd"].add("wino_act" if fused else "wino")

        def plane_bwd(gy, x, w, want_x=True, want_w=True):
            self.seen["dgrad"].update(["plane"] if want_x else [])
            self.seen["wgrad"].update(["plane"] if want_w else [])
        wrap("wino_conv3x3", wino)
        wrap("wino_wgrad3x3", lambda *a, **kw: self.seen["wgrad"].add("wino_wgrad"))
        wrap("sconv_wgrad", lambda *a, **kw: self.seen["wgrad"].add("sconv_wgrad"))
        wrap("wgrad3x3", lambda *a, **kw: self.seen["wgrad"].add("wgrad3x3"))
        wrap("planeconv_fwd_into", lambda *a, **kw: self.seen["fwd"].add("plane"))
        wrap("planeconv_backward", plane_bwd)
        wrap("conv1x1_small", lambda *a, **kw: [s.add("conv1x1") for s in self.seen.values()])      # one Function: both passes its own

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func._schema.name
        if name == "aten::convolution":
            self.seen["fwd"].add("miopen")
        elif name == "aten::convolution_backward":
            self.seen["dgrad"].update(["miopen"] if args[10][0] else [])
            self.seen["wgrad"].update(["miopen"] if args[10][1] else [])
        return func(*args, **(kwargs or {}))


# door, x shape, filter shape, (stride, padding, dilation), activation slope (conv_act only), switches set for the case, the plan
CASES = {
    "wino_fwd_dgrad": ("conv2d", (2, 16, 32, 64), (16, 16, 3, 3), (1, 1, 1), None, {}, ("wino", "wino", "miopen")),           # 1024 tiles >= 500
    "too_few_tiles": ("conv2d", (2, 16, 8, 16), (16, 16, 3, 3), (1, 1, 1), None, {}, ("miopen", "miopen", "miopen")),          # 64 tiles
    "wino_wgrad": ("conv2d", (2, 32, 32, 64), (32, 32, 3, 3), (1, 1, 1), None, {"WINO_WGRAD_MIN_MACS": 0}, ("wino", "wino", "wino_wgrad")),
    "wgrad_below_the_floor": ("conv2d", (2, 32, 32, 64), (32, 32, 3, 3), (1, 1, 1), None, {}, ("wino", "wino", "miopen")),
    "strided_stem": ("conv2d", (2, 3, 32, 52), (64, 3, 7, 7), (2, 3, 1), None, {}, ("miopen", "miopen", "sconv_wgrad")),
    "small_plane": ("conv_act", (2, 12, 2, 7), (12, 12, 3, 3), (1, 1, 1), 0.0, {}, ("plane", "plane", "plane")),
    "conv1x1_small": ("conv_act", (2, 12, 2, 7), (12, 12, 1, 1), (1, 0, 1), 1.0, {}, ("conv1x1", "conv1x1", "conv1x1")),
    "prepadded_thin_32": ("conv3x3_valid", (1, 32, 66, 210), (16, 32, 3, 3), (1, 0, 1), None, {}, ("wino", "wino", "wino_wgrad")),
    "prepadded_thin_16": ("conv3x3_valid", (1, 16, 66, 210), (16, 16, 3, 3), (1, 0, 1), None, {}, ("wino", "wino", "wgrad3x3")),
    "dilated": ("conv2d", (2, 16, 32, 64), (16, 16, 3, 3), (1, 2, 2), None, {}, ("wino", "wino", "miopen")),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_planned_kernels_are_the_ones_that_run(case, monkeypatch):
    door, xs, ws, (s, p, d), slope, switches, expected = CASES[case]
    for name, value in switches.items():
        monkeypatch.setattr(convs, name, value)
    dev = torch.device("cuda:0")
    torch.manual_seed(sum(xs) + sum(ws))
    x = torch.randn(*xs, device=dev, requires_grad=True)
    conv = torch.nn.Conv2d(ws[1], ws[0], ws[2], s, p, d, bias=door == "conv_act").to(dev)
    w, b = conv.weight, conv.bias
    if door == "conv2d":
        plan = convs.plan(x, w.shape, s, p, d)
        run = lambda: convs.conv2d(x, w, None, s, p, d)                                                # noqa: E731
    elif door == "conv_act":
        plan = convs.plan(x, w.shape, s, p, d, 1, True, slope != 1.0, "conv_act", ("plane", "wino_act", "conv1x1"))
        run = lambda: convs.conv_act(x, conv, slope)                                                   # noqa: E731
    else:
        plan = convs.plan(x, w.shape, ctx="prepadded")
        run = lambda: convs.conv3x3_valid(x, w)                                                        # noqa: E731
    assert tuple(plan) == expected
    with Ran(monkeypatch) as ran:
        y = run()
        g = torch.randn_like(y)
        y.backward(g)
    assert ran.seen == {"fwd": {plan.fwd}, "dgrad": {plan.dgrad}, "wgrad": {plan.wgrad}}
    xd, wd = x.detach().double().requires_grad_(True), w.detach().double().requires_grad_(True)
    bd = b.detach().double().requires_grad_(True) if b is not None else None
    yd = F.conv2d(xd, wd, bd, s, p, d)
    yd = yd if slope is None else F.leaky_relu(yd, slope)
    yd.backward(g.double())
    for a, ref in ((y.detach(), yd.detach()), (x.grad, xd.grad), (w.grad, wd.grad)) + (((b.grad, bd.grad),) if b is not None else ()):
        assert float((a.double() - ref).abs().max()) <= 5e-5 * float(ref.abs().max())
