"""GPU: the kernels of csrc/ops_epipolar.hip -- the dense eight-point epipolar map, its fixed-order mean and the gradient to the
flows -- against the float64 evaluation of tests/epipolar_cases.py, in guarded buffers at float offsets 0 to 3 (the 16-byte path
and the element path), with distinct per-sample cotangents; reproducibility by bits; a poisoned plane; the refusals."""
import ctypes

import pytest
import torch

from tests import eight_point_cases as EC
from tests import epipolar_cases as PC
from tests import guarded as G
from tests.guarded import U24

pytestmark = pytest.mark.gpu


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib(), L.stream_ptr()


def _p(c):
    return None if c is None else ctypes.c_void_p(c.ptr)


def _vector_path(H, W, offs):
    """the launchers' rule, restated: H*W a multiple of four and every flow, map and gradient pointer on 16 bytes"""
    return (H * W) % 4 == 0 and all(o == 0 for o in offs)


class _Buffers:
    """every tensor of the three entry points, carved at the given float offsets"""

    def __init__(self, case, weights, off_in, off_out):
        B, H, W = case["B"], case["H"], case["W"]
        lib, _ = _lib()
        self.fb, self.ff = G.Carved((B, 2, H, W), off_in, fill=case["flow_bwd"]), G.Carved((B, 2, H, W), off_in, fill=case["flow_fwd"])
        self.flow = G.Carved((2 * B, 2, H, W), off_in, fill=case["flow"])
        self.F = G.Carved((2 * B, 9), (off_in + 1) % 4, fill=case["F32"])
        self.gloss = G.Carved((B,), (off_in + 3) % 4, fill=torch.tensor(weights))
        self.dist = G.Carved((2 * B, H, W), off_out)
        self.loss = G.Carved((B,), (off_out + 2) % 4)
        self.ws_bytes = lib.dfe_epipolar_ws_bytes(B, H, W)
        self.ws = G.Carved((self.ws_bytes // 4,), off_out & 2)                 # doubles: on 8 bytes
        self.gb, self.gf = G.Carved((B, 2, H, W), off_out), G.Carved((B, 2, H, W), off_out)
        self.inputs = (self.fb, self.ff, self.flow, self.F, self.gloss)
        self.outputs = (self.dist, self.loss, self.ws, self.gb, self.gf)

    def run(self, case):
        lib, st = _lib()
        B, H, W = case["B"], case["H"], case["W"]
        assert lib.dfe_epipolar_map(_p(self.flow), _p(self.F), _p(self.dist), 2 * B, H, W, st) == 0
        assert lib.dfe_epipolar_loss_fwd(_p(self.fb), _p(self.ff), _p(self.F), _p(self.loss), _p(self.ws), B, H, W, st) == 0
        assert lib.dfe_epipolar_loss_bwd(_p(self.fb), _p(self.ff), _p(self.F), _p(self.gloss), _p(self.gb), _p(self.gf), B, H, W, st) == 0
        torch.cuda.synchronize()
        assert all(c.intact() for c in self.inputs + self.outputs)
        # every output element written: no sentinel word left (the workspace holds doubles, so it is looked at as words)
        assert all(not bool((c.bits[~c.guard] == G.SENTINEL).any()) for c in self.outputs)
        return self.dist.cpu(), self.loss.cpu(), torch.cat([self.gb.cpu(), self.gf.cpu()], 0)


@pytest.mark.parametrize("shape", PC.SHAPES)
def test_map_loss_and_gradient_against_float64_on_both_paths(shape):
    case = PC.make_case(shape)
    B, H, W = shape
    ref, factor = case["ref"], case["factor"]
    weights = EC.WEIGHTS_OF[B]
    l64, mA, g64, unit = PC.loss_reference(ref, B, weights)
    keep = (~PC.near_sign(ref)).unsqueeze(1).expand_as(g64)
    assert float((~keep).double().mean()) <= PC.MAX_EXCLUDED
    first, paths = None, set()
    # all buffers at one offset (0: the 16-byte path where H*W % 4 == 0), then inputs and outputs apart
    for off_in, off_out in ((0, 0), (1, 1), (2, 2), (3, 3), (0, 2), (3, 0)):
        tag = "epipolar %dx%dx%d in+%d out+%d" % (B, H, W, off_in, off_out)
        paths.add(_vector_path(H, W, (off_in, off_out)))
        buf = _Buffers(case, weights, off_in, off_out)
        dist, loss, grad = buf.run(case)
        if first is None:
            first = (dist, loss, grad)
            G.check_bound(tag + " map", dist, case["yard"], ref["dist"], ref["A"])
            el = (loss.double() - l64).abs() / (factor * U24 * mA + 2 * U24 * l64.abs())
            eg = ((grad.double() - g64).abs() / (U24 * unit))[keep]
            print("EBOUND %s loss err/bound %.3f  gradient e %.3f of %.3f (%d of %d elements near a sign left out)"
                  % (tag, float(el.max()), float(eg.max()), factor, int((~keep).sum()), keep.numel()))
            assert bool(torch.isfinite(loss).all()) and float(el.max()) <= 1.0, (tag, loss, l64)
            assert bool(torch.isfinite(grad).all()) and float(eg.max()) <= factor, (tag, float(eg.max()), factor)
            # where s is exactly 0 in fp32 the gradient is 0, never NaN; a distinct cotangent per sample reached its sample
            assert float(grad[:B].abs().amax((1, 2, 3)).min()) > 0 and float(grad[B:].abs().amax((1, 2, 3)).min()) > 0
            again = buf.run(case)                                      # the same buffers once more: the same bits
            assert all(G.bits_equal(a, b) for a, b in zip(first, again)), tag
        else:                                                          # another alignment, another path: the same bits
            assert all(G.bits_equal(a, b) for a, b in zip(first, (dist, loss, grad))), tag
    assert paths == ({True, False} if (H * W) % 4 == 0 else {False})


def test_the_shapes_cover_both_paths_the_tail_and_several_blocks():
    hw = [H * W for _, H, W in PC.SHAPES]
    assert any(n % 4 == 3 for n in hw) and any(n % 4 == 0 for n in hw) and min(hw) < 64
    assert any(n > 3 * 2048 and n % 2048 for n in hw)                 # several blocks per plane, the last partly filled
    assert {B for B, _, _ in PC.SHAPES} == {1, 2, 3}


@pytest.mark.parametrize("poison", ("F", "flow"))
def test_a_poisoned_plane_reaches_its_own_sample_alone(poison):
    """NaN in the forward plane of sample 1 (its F, or one pixel of its flow): that sample's loss is NaN, the other samples keep
    their bits in the loss and in both gradients, and the calls return."""
    shape = (3, 12, 20)
    case = dict(PC.make_case(shape))
    B, H, W = shape
    weights = EC.WEIGHTS_OF[B]
    _, clean_loss, clean_grad = _Buffers(case, weights, 0, 0).run(case)
    if poison == "F":
        case["F32"] = case["F32"].clone()
        case["F32"][B + 1] = float("nan")
    else:
        case["flow_fwd"] = case["flow_fwd"].clone()
        case["flow_fwd"][1, 0, 5, 7] = float("nan")
        case["flow"] = torch.cat([case["flow_bwd"], case["flow_fwd"]], 0)
    lib, st = _lib()
    buf = _Buffers(case, weights, 0, 0)
    assert lib.dfe_epipolar_loss_fwd(_p(buf.fb), _p(buf.ff), _p(buf.F), _p(buf.loss), _p(buf.ws), B, H, W, st) == 0
    assert lib.dfe_epipolar_loss_bwd(_p(buf.fb), _p(buf.ff), _p(buf.F), _p(buf.gloss), _p(buf.gb), _p(buf.gf), B, H, W, st) == 0
    torch.cuda.synchronize()
    loss, gb, gf = buf.loss.cpu(), buf.gb.cpu(), buf.gf.cpu()
    assert bool(torch.isnan(loss[1])) and G.bits_equal(loss[[0, 2]], clean_loss[[0, 2]])
    assert G.bits_equal(gb, clean_grad[:B])                           # the backward planes read other F planes and flows
    assert G.bits_equal(gf[[0, 2]], clean_grad[B:][[0, 2]])
    bad = torch.isnan(gf[1])
    assert bool(bad.all()) if poison == "F" else (bool(bad[:, 5, 7].all()) and int(bad.sum()) == 2)
    assert all(c.intact() for c in buf.inputs + buf.outputs)


def test_the_refusals_come_before_a_launch():
    case = PC.make_case((2, 12, 20))
    B, H, W = 2, 12, 20
    lib, st = _lib()
    buf = _Buffers(case, EC.WEIGHTS_OF[B], 0, 0)
    args = (_p(buf.fb), _p(buf.ff), _p(buf.F), _p(buf.loss), _p(buf.ws))
    assert lib.dfe_epipolar_loss_fwd(None, *args[1:], B, H, W, st) == -1
    assert lib.dfe_epipolar_loss_fwd(*args, 0, H, W, st) == -2 and lib.dfe_epipolar_loss_fwd(*args, B, 0, W, st) == -2
    assert lib.dfe_epipolar_loss_fwd(*args, 16385, H, W, st) == -2 and lib.dfe_epipolar_loss_fwd(*args, B, 1 << 14, 1 << 14, st) == -2
    odd = G.Carved((buf.ws_bytes // 4,), 1)                                # a workspace off its 8 bytes
    assert lib.dfe_epipolar_loss_fwd(*args[:4], _p(odd), B, H, W, st) == -2
    assert lib.dfe_epipolar_loss_bwd(_p(buf.fb), _p(buf.ff), _p(buf.F), None, _p(buf.gb), _p(buf.gf), B, H, W, st) == -1
    assert lib.dfe_epipolar_loss_bwd(_p(buf.fb), _p(buf.ff), _p(buf.F), _p(buf.gloss), _p(buf.gb), _p(buf.gf), B, H, -1, st) == -2
    assert lib.dfe_epipolar_map(_p(buf.flow), _p(buf.F), None, 2 * B, H, W, st) == -1
    assert lib.dfe_epipolar_map(_p(buf.flow), _p(buf.F), _p(buf.dist), 32769, H, W, st) == -2
    torch.cuda.synchronize()
    assert all(c.untouched() for c in (buf.dist, buf.loss, buf.ws, buf.gb, buf.gf, odd))


@pytest.mark.parametrize("shape", ((2, 12, 20), (2, 13, 19)))
def test_the_autograd_function_is_the_entry_points(shape):
    """epipolar.py on plain tensors: the bits of the guarded run; F32 gets no gradient; the map keeps the [P,1,H,W] layout"""
    from unsupervised_depth_opticalflow_egomotion_amd import epipolar
    case = PC.make_case(shape)
    B = shape[0]
    weights = EC.WEIGHTS_OF[B]
    dist, loss, grad = _Buffers(case, weights, 0, 0).run(case)
    dev = G.default_device()
    fb, ff = case["flow_bwd"].to(dev).requires_grad_(True), case["flow_fwd"].to(dev).requires_grad_(True)
    F32 = case["F32"].to(dev).requires_grad_(True)
    out = epipolar.EpipolarLossFn.apply(fb, ff, F32)
    (out * torch.tensor(weights, device=dev)).sum().backward()
    torch.cuda.synchronize()
    assert F32.grad is None and G.bits_equal(out, loss)
    assert G.bits_equal(torch.cat([fb.grad, ff.grad], 0), grad)
    m = epipolar.epipolar_map(case["flow"].to(dev), F32)
    assert tuple(m.shape) == (2 * B, 1) + shape[1:] and G.bits_equal(m[:, 0], dist)
