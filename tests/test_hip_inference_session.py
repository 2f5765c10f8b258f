"""GPU: inference.InferenceSession on the joint model at 128x448 (the smallest frame the flow net accepts; the pose net's
Linear(14, 14) layers fix its frame at 256x832), B = 1 and 2.

* the model's own eval call returns the same bits before, during and after a session's life (the session leaves nothing behind);
* depth, flow and pose from a session are no farther from a float64 host reference (the same model, ``.double()``, through its
  ATen branch; the flow net's warp / correlation, which have no host path, are the oracle's) than twice the plain eval call's
  distance: max|session - f64| <= 2 max|plain - f64| + 1e-7 scale.  2 = a re-ordered rounding chain over ~20 layers; a wrong eps,
  swapped mean / var or a dropped residual move the output by orders of magnitude more.  The BatchNorm buffers and affine
  parameters are moved away from (0, 1) / (1, 0) first: with fresh ones the fold is nearly the identity;
* graph replay returns the eager session's bits (deterministic mode: the convolutions on fixed-order kernels);
* weights written in place between two calls of a graph session: the tables are folded again, the call is captured again and the
  result is a fresh eager session's -- also when another model's filters were registered with the Winograd cache in between;
* a session ``infer_depth`` launches one disparity head; ``test.py --session graph`` prints the tables it prints without the flag."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from unsupervised_depth_opticalflow_egomotion_amd import convs, ops, synthetic
from unsupervised_depth_opticalflow_egomotion_amd.inference import InferenceSession
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
from unsupervised_depth_opticalflow_egomotion_amd.networks import PWC_tf
from unsupervised_depth_opticalflow_egomotion_amd.networks.resnet import FrameBatchNorm2d
from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 128, 448
PH, PW = 256, 832


def dev():
    return torch.device("cuda:0")


def _frames(B, h, w, seed):
    im = torch.from_numpy(synthetic.make_triplet_batch(B, h, w, 3, seed=seed)[0])
    return [im[:, :, k * h:(k + 1) * h].contiguous() for k in range(3)]


def _build(seed=0):
    torch.manual_seed(seed)
    model = get_model("geom")(make_cfg()).to(dev())
    gen = torch.Generator().manual_seed(seed + 17)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, FrameBatchNorm2d):
                m.weight.copy_((0.6 + 0.8 * torch.rand(m.weight.shape, generator=gen)).to(dev()))
                m.bias.copy_((0.2 * torch.randn(m.bias.shape, generator=gen)).to(dev()))
        model.train()
        for k in range(6):          # running statistics: 1 - 0.9^6 = 47 % of the way to the activations' own
            model.depth_net(_frames(2, H, W, 50 + k)[1].to(dev()))
    return model.eval()


class _Deterministic:
    def __enter__(self):
        self.was = convs.DETERMINISTIC
        convs.set_deterministic(True)

    def __exit__(self, *exc):
        convs.set_deterministic(self.was)


@pytest.fixture(scope="module", autouse=True)
def _leave_the_process_as_found():
    """The models of this module register ~150 filters with the process-wide Winograd cache, which keeps a dead model's transformed
    filters (hundreds of MB) until its next refresh, and the sessions' graphs leave their memory pools in the allocator's cache.
    Hand both back when the module ends, so that the tests after it start from the allocator state they start from alone."""
    yield
    import gc
    gc.collect()
    torch.cuda.synchronize()
    ops.wino_weights.refresh()          # prunes the entries of dead parameters
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def world():
    from oracle import loss_stack_oracle as O

    class HostPWC(PWC_tf):          # the product's warp / correlation have no host path: the oracle's (checker only)
        def warp(self, x, flow):
            return O.warp_flow(x, flow, use_mask=False)

        def corr_naive(self, a, b, d=4):
            return O.corr_naive(a, b, d)
    model = _build()
    host = copy.deepcopy(model).cpu()
    pw = HostPWC()
    pw.load_state_dict(host.pwc_model.state_dict())
    pw.corr = pw.corr_naive
    host.pwc_model = pw
    host = host.double().eval()
    fl, ft, fr = _frames(2, H, W, 7)
    pose_in = torch.cat(_frames(2, PH, PW, 8), 1)
    with torch.no_grad():
        ref = {"depth": host.infer_depth(ft.double()), "flow": host.inference_flow(ft.double(), fr.double()),
               "pose": host.infer_pose(pose_in.double())}
    return {"model": model, "img": ft.to(dev()), "img_r": fr.to(dev()), "pose_in": pose_in.to(dev()), "ref": ref}


def _eq(a, b):
    return np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def test_plain_eval_call_keeps_its_bits_around_a_session(world):
    """deterministic mode, so that the three plain calls can be compared for equality at all (MIOpen's solver choice follows the
    workspace the allocator hands it); the BatchNorm layers take the ATen branch in each of them"""
    model, img = world["model"], world["img"]
    with _Deterministic(), torch.no_grad():
        before = model.infer_depth(img)
        for graph in (False, True):
            session = InferenceSession(model, graph=graph)
            mine = session.infer_depth(img)
            during = model.infer_depth(img)
            assert not _eq(mine, before)            # another rounding chain: the session did run its own kernels
            assert float((mine - before).abs().max()) <= 1e-4 * float(before.abs().max())
            assert all(m.folded is None and "folded" not in m.__dict__ for m in model.modules() if isinstance(m, FrameBatchNorm2d))
            del session
            after = model.infer_depth(img)
            assert _eq(before, during) and _eq(before, after), graph


@pytest.mark.parametrize("B", [1, 2])
def test_session_is_no_farther_from_float64_than_the_plain_call(world, B):
    model, ref = world["model"], world["ref"]
    session = InferenceSession(model)
    calls = {"depth": ("infer_depth", (world["img"][:B],), ref["depth"][:B]),
             "flow": ("inference_flow", (world["img"][:B], world["img_r"][:B]), ref["flow"][:B]),
             "pose": ("infer_pose", (world["pose_in"][:B],), ref["pose"][:B])}
    with torch.no_grad():
        for what, (name, args, want) in calls.items():
            plain = getattr(model, name)(*[a.contiguous() for a in args])
            mine = getattr(session, name)(*[a.contiguous() for a in args])
            assert mine.shape == plain.shape == want.shape and mine.dtype == torch.float32
            scale = float(want.abs().max())
            d_plain = float((plain.double().cpu() - want).abs().max())
            d_mine = float((mine.double().cpu() - want).abs().max())
            print("F64DIST %s B=%d: session %.3e plain eval %.3e (scale %.3e)" % (what, B, d_mine, d_plain, scale))
            assert d_mine <= 2.0 * d_plain + 1e-7 * scale, (what, B, d_mine, d_plain, scale)
    assert session.stats() == {"folds": 1, "captures": 0, "replays": 0}


def test_graph_replay_returns_the_eager_sessions_bits(world):
    model = world["model"]
    with _Deterministic():
        eager, graph = InferenceSession(model), InferenceSession(model, graph=True)
        calls = [("infer_depth", (world["img"][:B].contiguous(),)) for B in (1, 2)]
        calls += [("inference_flow", (world["img"][:B].contiguous(), world["img_r"][:B].contiguous())) for B in (1, 2)]
        calls += [("infer_pose", (world["pose_in"][:B].contiguous(),)) for B in (1, 2)]
        for name, args in calls:
            want = getattr(eager, name)(*args)
            for _ in range(2):          # the capturing call and a pure replay
                assert _eq(getattr(graph, name)(*args), want), (name, args[0].shape)
        other = world["img"][:1].flip(3).contiguous()          # new values through the static input buffers
        assert _eq(graph.infer_depth(other), eager.infer_depth(other))
        st = graph.stats()
        assert st["captures"] == len(calls) and st["replays"] == 2 * len(calls) + 1 and st["folds"] == 1
        assert eager.stats()["captures"] == eager.stats()["replays"] == 0
        # a capture belongs to the mode and convention it was made under: under another one the call is captured again
        flipped = not ops.get_align_corners()
        ops.set_align_corners(flipped)
        try:
            pose_in = world["pose_in"][:1].contiguous()
            assert _eq(graph.infer_pose(pose_in), eager.infer_pose(pose_in))
        finally:
            ops.set_align_corners(not flipped)
        assert graph.stats()["captures"] == len(calls) + 1 and graph.stats()["folds"] == 1


@pytest.mark.parametrize("second_model", [False, True], ids=["alone", "another model registers"])
def test_weights_written_between_calls_are_followed(second_model):
    model = _build(seed=3)
    img = _frames(1, H, W, 9)[1].to(dev())
    block = model.depth_net.encoder.encoder.layer1[0]
    with _Deterministic():
        session = InferenceSession(model, graph=True)
        first = session.infer_depth(img)
        assert session.stats() == {"folds": 1, "captures": 1, "replays": 1}
        assert convs.plan(torch.empty(1, 64, H // 4, W // 4, device=dev()), block.conv1.weight.shape, 1, 1, ctx="module").fwd == "wino"
        if second_model:        # the Winograd cache rebuilds its device tables at the next refresh (train_step.GraphedTrainStep's note)
            other = convs.Conv2d(32, 32, 3, 1, 1).to(dev())
            with torch.no_grad():
                other(torch.randn(1, 32, 16, 24, device=dev()))
            assert ops.wino_weights.members is None
        with torch.no_grad():
            for p in (block.conv1.weight, block.bn1.weight, block.bn1.running_var):
                p.mul_(1.01)
        second = session.infer_depth(img)
        assert session.stats() == {"folds": 2, "captures": 2, "replays": 2}
        fresh = InferenceSession(model).infer_depth(img)
        assert _eq(second, fresh) and not _eq(second, first)
        assert _eq(session.infer_depth(img), fresh)          # and a pure replay of the new capture
        assert session.stats() == {"folds": 2, "captures": 2, "replays": 3}


def test_depth_and_flow_models_get_the_methods_they_have(world):
    img, img_r, pose_in = world["img"][:1].contiguous(), world["img_r"][:1].contiguous(), world["pose_in"]
    with _Deterministic(), torch.no_grad():
        torch.manual_seed(1)
        flow_model = get_model("flow")(make_cfg(mode="flow")).to(dev()).eval()
        for graph in (False, True):
            s = InferenceSession(flow_model, graph=graph)
            assert hasattr(s, "inference_flow") and not hasattr(s, "infer_depth") and not hasattr(s, "infer_pose")
            assert _eq(s.inference_flow(img, img_r), flow_model.inference_flow(img, img_r))      # no BatchNorm: the same kernels
            assert s.stats()["folds"] == 1 and s.stats()["replays"] == int(graph)
        depth_model = get_model("depth")(make_cfg(mode="depth")).to(dev()).eval()
        for graph in (False, True):
            s = InferenceSession(depth_model, graph=graph)
            assert hasattr(s, "infer_depth") and hasattr(s, "infer_pose") and not hasattr(s, "inference_flow")
            assert _eq(s.infer_pose(pose_in), depth_model.infer_pose(pose_in))
            mine, plain = s.infer_depth(img), depth_model.infer_depth(img)
            # two fp32 rounding chains of the same ~40 layers (each within ~1e-6 of float64, see above); a wrong fold is O(1)
            assert mine.shape == plain.shape and float((mine - plain).abs().max()) <= 1e-4 * float(plain.abs().max())
    with pytest.raises(ValueError, match="training mode"):
        InferenceSession(depth_model.train())
    s = InferenceSession(depth_model.eval())
    depth_model.train()
    with pytest.raises(ValueError, match="training mode"):
        s.infer_depth(img)
    depth_model.eval()
    with pytest.raises(Exception, match="HIP device"):
        s.infer_depth(img.cpu())


def test_session_depth_launches_one_disparity_head(world, monkeypatch):
    calls = []
    real = ops.disp_head
    monkeypatch.setattr(ops, "disp_head", lambda *a: (calls.append(1), real(*a))[1])
    with torch.no_grad():
        world["model"].infer_depth(world["img"])
        assert len(calls) == 3
        del calls[:]
        InferenceSession(world["model"]).infer_depth(world["img"])
    assert len(calls) == 1


def test_test_py_session_graph_prints_the_same_tables(tmp_path):
    """``test.py --task demo`` on one seeded checkpoint, without the flag and with ``--session graph``: exit 0, the same metric keys
    (white space normalised), and every printed metric within one unit of its last printed digit (%.4f).  The two processes differ
    by a rounding chain (~1e-7 of an output) and by the default mode's MIOpen run-to-run rounding; a metric that sits on a rounding
    boundary of its fourth decimal may print one unit apart, never more."""
    ckpt = str(tmp_path / "last.pth")
    torch.manual_seed(0)
    sd = get_model("geom")(make_cfg()).state_dict()
    torch.save({"iteration": 1, "model_state_dict": {"module." + k: v for k, v in sd.items()}, "optimizer_state_dict": {}}, ckpt)
    base = [sys.executable, os.path.join(REPO, "test.py"), "-c", os.path.join(REPO, "config", "kitti_geom.yaml"), "--mode", "geom",
            "--task", "demo", "--pretrained_model", ckpt]
    number = r"-?(?:\d+\.\d+|nan|inf)"
    keys, values = [], []
    for extra in ([], ["--session", "graph"]):
        out = subprocess.run(base + extra, capture_output=True, text=True, cwd=REPO, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        assert "Model Loaded." in out.stdout and "[EVAL] [synthetic flow]" in out.stdout and "[EVAL] [synthetic depth]" in out.stdout
        tables = out.stdout[out.stdout.index("[EVAL]"):]
        keys.append(re.sub(number, "#", tables).replace(",", " ").split())
        values.append([float(v) for v in re.findall(number, tables)])
    assert keys[0] == keys[1] and "abs_rel" in keys[0] and "epe" in keys[0]
    assert len(values[0]) == len(values[1]) == 4 + 7, values
    print("TESTPY plain %s\nTESTPY graph %s" % (values[0], values[1]))
    for a, b in zip(*values):
        assert np.isfinite(a) and np.isfinite(b) and abs(a - b) <= 1.0001e-4, (values[0], values[1])
