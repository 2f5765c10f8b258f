"""GPU: the eval-mode BatchNorm kernels (csrc/ops_bn.hip: dfe_bn_fold, dfe_bn_eval_fwd) through the C ABI in guarded, poisoned
buffers (tests/guarded.py): return code 0, guard bands intact, every output element written, inputs unchanged.

dfe_bn_fold equals the double-precision formula rounded once to fp32, bit for bit.  dfe_bn_eval_fwd is held, element by element,
to |y - ref| <= 4 * 2^-24 * (|x s| + |mean s| + |b| + |res|) against the float64 reference act((x - mean) / sqrt(var + eps) * w + b + res)
with s = w / sqrt(var + eps) in float64: one rounding each for s, t, the product and the two adds; ReLU is 1-Lipschitz.  The bound is
derived, not measured.  Shapes: a one-pixel plane, an odd plane (dword path, plane boundaries), H*W % 4 == 0 planes (16-byte path, a
wave's partial chunk), a vector-eligible size behind a misaligned pointer, and more planes than a 16-bit grid dimension holds; each
with and without residual, with and without ReLU, in place and out of place."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu
EPS = 1e-5

# (B, C, H, W), x's offset in floats past a 16-byte boundary
CASES = [((1, 2, 1, 1), 0), ((2, 3, 5, 7), 0), ((3, 16, 4, 13), 0), ((1, 64, 8, 26), 0), ((2, 5, 6, 6), 1), ((70000, 1, 2, 2), 0)]


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib(), L.stream_ptr()


def _p(c):
    return None if c is None else ctypes.c_void_p(c.ptr)


def _inputs(shape):
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(1000 * C + 10 * H + W + B)
    x = 2.0 * torch.randn(shape, generator=gen) + 0.5
    res = torch.randn(shape, generator=gen)
    var = 0.01 + 3.99 * torch.rand(C, generator=gen)
    mean, bias, weight = torch.randn(C, generator=gen), torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)
    weight[::2] *= -1.0                     # both signs
    if C >= 2:
        var[0] = 0.0                        # a dead channel: s = w / sqrt(eps)
        weight[C - 1] = 0.0                 # a zero scale: y = act(b [+ res])
        mean[0], mean[1] = -mean[0].abs(), mean[1].abs()      # both signs whatever the draw
        bias[0], bias[1] = bias[0].abs(), -bias[1].abs()
    return x, res, weight, bias, mean, var


def _fold64(weight, bias, mean, var):
    """(s, t) in float64, as dfe_hip.h states them: eps is the fp32 value the kernel receives"""
    eps = np.float64(np.float32(EPS))
    s = weight.double().numpy() / np.sqrt(var.double().numpy() + eps)
    return s, bias.double().numpy() - mean.double().numpy() * s


def _fold(lib, st, weight, bias, mean, var):
    C = weight.numel()
    wc, bc, mc, vc = (G.Carved((C,), o, fill=t) for o, t in ((1, weight), (2, bias), (3, mean), (0, var)))
    sc, tc = G.Carved((C,), 3), G.Carved((C,), 1)
    assert lib.dfe_bn_fold(_p(wc), _p(bc), _p(mc), _p(vc), ctypes.c_float(EPS), _p(sc), _p(tc), C, st) == 0
    torch.cuda.synchronize()
    for c in (wc, bc, mc, vc, sc, tc):
        assert c.intact()
    assert sc.written() and tc.written()
    for c, t in ((wc, weight), (bc, bias), (mc, mean), (vc, var)):
        assert G.bits_equal(c.cpu(), t)
    return sc, tc


@pytest.mark.parametrize("shape,xoff", CASES, ids=["x".join(map(str, s)) + ("+%d" % o if o else "") for s, o in CASES])
def test_bn_fold_and_eval_in_guarded_buffers(shape, xoff):
    lib, st = _lib()
    B, C, H, W = shape
    x, res, weight, bias, mean, var = _inputs(shape)
    s64, t64 = _fold64(weight, bias, mean, var)
    sc, tc = _fold(lib, st, weight, bias, mean, var)
    # the fold: the double-precision formula, rounded once
    assert np.array_equal(sc.cpu().numpy(), s64.astype(np.float32)), "scale"
    assert np.array_equal(tc.cpu().numpy(), t64.astype(np.float32)), "shift"
    s_b = torch.from_numpy(s64)[None, :, None, None]
    inv = torch.from_numpy(1.0 / np.sqrt(var.double().numpy() + np.float64(np.float32(EPS))))[None, :, None, None]
    bc = lambda t: t.double()[None, :, None, None]      # noqa: E731
    worst = 0.0
    for with_res, relu, in_place in itertools.product((False, True), (0, 1), (False, True)):
        tag = (shape, xoff, with_res, relu, in_place)
        xc = G.Carved(shape, xoff, fill=x)
        rc = G.Carved(shape, 0, fill=res) if with_res else None
        yc = xc if in_place else G.Carved(shape, 0)
        assert lib.dfe_bn_eval_fwd(_p(xc), _p(rc), _p(sc), _p(tc), _p(yc), B, C, H, W, relu, st) == 0, tag
        torch.cuda.synchronize()
        for c in (xc, rc, yc, sc, tc):
            assert c is None or c.intact(), (tag, "a guard band was overwritten")
        assert yc.written(), (tag, "unwritten or non-finite output elements")
        if not in_place:
            assert G.bits_equal(xc.cpu(), x), (tag, "x changed")
        if with_res:
            assert G.bits_equal(rc.cpu(), res), (tag, "residual changed")
        ref = (x.double() - bc(mean)) * inv * bc(weight) + bc(bias)
        bound = (x.double() * s_b).abs() + (bc(mean) * s_b).abs() + bc(bias).abs()
        if with_res:
            ref, bound = ref + res.double(), bound + res.double().abs()
        if relu:
            ref = torch.relu(ref)
        err = (yc.cpu().double() - ref).abs()
        ratio = float((err / (G.U24 * bound).clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= 4.0 * G.U24 * bound).all()), (tag, "max |y - ref| / (2^-24 A) = %.3f > 4" % ratio)
        if relu:
            assert float(yc.cpu().min()) >= 0.0, tag
    print("EBOUND bn_eval %s max |y - ref| / (2^-24 A) = %.3f (bound 4)" % (shape, worst))


def test_bn_eval_refuses_null_and_non_positive_arguments():
    lib, st = _lib()
    x, y, s = G.Carved((1, 2, 2, 2), fill=torch.ones(1, 2, 2, 2)), G.Carved((1, 2, 2, 2)), G.Carved((2,), fill=torch.ones(2))
    assert lib.dfe_bn_eval_fwd(None, None, _p(s), _p(s), _p(y), 1, 2, 2, 2, 0, st) == -1
    assert lib.dfe_bn_eval_fwd(_p(x), None, _p(s), None, _p(y), 1, 2, 2, 2, 0, st) == -1
    assert lib.dfe_bn_eval_fwd(_p(x), None, _p(s), _p(s), None, 1, 2, 2, 2, 0, st) == -1
    assert lib.dfe_bn_eval_fwd(_p(x), None, _p(s), _p(s), _p(y), 1, 0, 2, 2, 0, st) == -2
    assert lib.dfe_bn_eval_fwd(_p(x), None, _p(s), _p(s), _p(y), 1, 2, 2, -1, 0, st) == -2
    assert lib.dfe_bn_fold(_p(s), _p(s), None, _p(s), ctypes.c_float(EPS), _p(s), _p(s), 2, st) == -1
    assert lib.dfe_bn_fold(_p(s), _p(s), _p(s), _p(s), ctypes.c_float(EPS), _p(s), _p(s), 0, st) == -2
    torch.cuda.synchronize()
    assert y.untouched() and y.intact() and x.intact()


def test_ops_bn_eval_matches_the_module_and_runs_in_place():
    """ops.bn_fold / ops.bn_eval on an nn.BatchNorm2d with moved statistics: within the derived bound of the float64 module, and
    ``out=x`` writes x's own storage."""
    from unsupervised_depth_opticalflow_egomotion_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    bn = torch.nn.BatchNorm2d(6).to(dev)
    with torch.no_grad():
        bn.weight.uniform_(-1.5, 1.5), bn.bias.normal_(), bn.running_mean.normal_(), bn.running_var.uniform_(0.01, 4.0)
    bn.eval()
    x, res = torch.randn(2, 6, 5, 8, device=dev), torch.randn(2, 6, 5, 8, device=dev)
    with torch.no_grad():
        scale, shift = ops.bn_fold(bn)
        y = ops.bn_eval(x, scale, shift, residual=res, relu=True)
        bn64 = torch.nn.BatchNorm2d(6).double()
        bn64.load_state_dict({k: v.double().cpu() for k, v in bn.state_dict().items()})
        bn64.eval()
        ref = torch.relu(bn64(x.double().cpu()) + res.double().cpu())
        s = (bn.weight.double() / torch.sqrt(bn.running_var.double() + float(np.float32(bn.eps)))).cpu()[None, :, None, None]
        A = (x.double().cpu() * s).abs() + (bn.running_mean.double().cpu()[None, :, None, None] * s).abs() \
            + bn.bias.double().cpu().abs()[None, :, None, None] + res.double().cpu().abs()
        assert bool(((y.double().cpu() - ref).abs() <= 4.0 * G.U24 * A + 1e-300).all())
        x2 = x.clone()
        y2 = ops.bn_eval(x2, scale, shift, residual=res, relu=True, out=x2)
        assert y2.data_ptr() == x2.data_ptr() and torch.equal(y2, y)
