"""CPU-only checks of the inference path: the header declares the two eval-mode BatchNorm entry points and the binding types them
from their prototypes, their argument checks answer before any launch, ops.bn_fold / ops.bn_eval and InferenceSession refuse host
tensors, autograd inputs and a model in training mode, and the depth decoder's host graph is what it was."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from unsupervised_depth_opticalflow_egomotion_amd import _lib, ops
from unsupervised_depth_opticalflow_egomotion_amd._lib import DfeError

P, I, FL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


def test_header_declares_the_eval_batch_norm_entry_points():
    sigs = _lib.header_signatures()
    assert sigs["dfe_bn_fold"] == (I, [P, P, P, P, FL, P, P, I, P])
    assert sigs["dfe_bn_eval_fwd"] == (I, [P, P, P, P, P, I, I, I, I, I, P])
    lib = _lib.get_lib()
    for name in ("dfe_bn_fold", "dfe_bn_eval_fwd"):
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == sigs[name], name
    assert _lib.header_abi_version() == lib.dfe_abi_version() == 4      # new symbols only: no signature changed


def test_argument_checks_answer_before_any_launch():
    lib, p = _lib.get_lib(), ctypes.c_void_p(16)
    assert lib.dfe_bn_fold(p, p, None, p, 1e-5, p, p, 4, None) == -1
    assert lib.dfe_bn_fold(p, p, p, p, 1e-5, p, None, 4, None) == -1
    assert lib.dfe_bn_fold(p, p, p, p, 1e-5, p, p, 0, None) == -2
    assert lib.dfe_bn_eval_fwd(None, None, p, p, p, 1, 4, 8, 8, 0, None) == -1
    assert lib.dfe_bn_eval_fwd(p, None, None, p, p, 1, 4, 8, 8, 0, None) == -1
    assert lib.dfe_bn_eval_fwd(p, None, p, p, None, 1, 4, 8, 8, 1, None) == -1
    for dims in ((0, 4, 8, 8), (1, 0, 8, 8), (1, 4, -8, 8), (1, 4, 8, 0)):
        assert lib.dfe_bn_eval_fwd(p, None, p, p, p, *dims, 0, None) == -2, dims
    assert lib.dfe_bn_eval_fwd(p, None, p, p, p, 1, 1, 1 << 16, 1 << 15, 0, None) == -2      # H * W = 2^31
    assert lib.dfe_bn_eval_fwd(p, None, p, p, p, 1 << 15, 1 << 15, 1, 1, 0, None) == -2      # 2^30 units of work


def test_bn_ops_refuse_host_tensors_and_autograd_inputs():
    bn = torch.nn.BatchNorm2d(3).eval()
    x, s = torch.randn(1, 3, 4, 4), torch.ones(3)
    with torch.no_grad():
        with pytest.raises(DfeError):
            ops.bn_eval(x, s, s)
        with pytest.raises(DfeError):
            ops.bn_fold(bn)
    with pytest.raises(DfeError, match="forward-only"):
        ops.bn_eval(x.clone().requires_grad_(), s, s)
    with pytest.raises(DfeError, match="forward-only"):
        ops.bn_fold(bn)          # grad mode on, weight requires grad
    with torch.no_grad(), pytest.raises(DfeError):
        ops.bn_eval(x[0], s, s)
    with torch.no_grad(), pytest.raises(DfeError, match="fp32"):
        ops.bn_eval(x, s.to(torch.int32), s)          # a table of another dtype would be read as floats


def test_inference_session_refuses_host_and_training_models():
    from unsupervised_depth_opticalflow_egomotion_amd.inference import InferenceSession
    from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg
    model = get_model("depth")(make_cfg(mode="depth"))
    with pytest.raises(ValueError, match="training mode"):
        InferenceSession(model)
    with pytest.raises(DfeError, match="HIP device"):
        InferenceSession(model.eval())
    with pytest.raises(ValueError):
        InferenceSession(torch.nn.Linear(2, 2).eval())


def test_depth_decoder_host_graph_is_unchanged():
    """forward_aten against the module graph written out here; forward() of host tensors is forward_aten; forward_fused's new
    ``scales`` argument defaults to every head."""
    import inspect
    from unsupervised_depth_opticalflow_egomotion_amd.networks.depth_model import DepthDecoder
    torch.manual_seed(5)
    enc = [64, 64, 128, 256, 512]
    dec = DepthDecoder(enc, scales=range(3)).eval()
    feats = [torch.randn(1, c, 64 >> i, 96 >> i) for i, c in enumerate(enc)]
    with torch.no_grad():
        got, x, want = dec.forward_aten(feats), feats[-1], {}
        for scale in range(4, -1, -1):
            a, b = dec.upconvs[4 - scale]
            x = F.elu(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), a.conv.conv.weight, a.conv.conv.bias))
            x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
            if scale > 0:
                x = torch.cat([x, feats[scale - 1]], 1)
            x = F.elu(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), b.conv.conv.weight, b.conv.conv.bias))
            if scale < 3:
                h = dec.dispconvs[scale].conv
                want[scale] = torch.sigmoid(F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), h.weight, h.bias))
        assert sorted(got) == [0, 1, 2]
        for k in want:
            assert torch.equal(got[k], want[k]), k
        fwd = dec(feats)
        assert all(torch.equal(fwd[k], got[k]) for k in got)
    assert inspect.signature(DepthDecoder.forward_fused).parameters["scales"].default is None
    assert list(inspect.signature(DepthDecoder.forward_aten).parameters) == ["self", "feats"]
