"""CPU-only checks: the C-ABI library loads and exports every symbol include/dfe_hip.h declares, the host
API mirrors the reference (state-dict keys, get_model, config weights), the product path refuses CPU
tensors instead of falling back, and the 2-process (gloo) data-parallel path reproduces the single-process
gradient."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests.golden import make_golden as MG

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_header_symbol():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib
    names = _lib.header_symbols()
    assert len(names) >= 24 and "dfe_geom_loss_fwd" in names and "dfe_warp_flow_bwd" in names
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), n
    assert _lib.get_lib().dfe_abi_version() == _lib.header_abi_version() >= 2
    # every argument and return type is read from the prototype (tests/test_binding_cpu.py pins them): nothing is left untyped
    assert all(getattr(_lib.get_lib(), n).argtypes is not None for n in names) and set(names) == set(_lib.header_signatures())


def test_error_strings_and_argument_checks_without_gpu():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib, loss_stack
    lib = _lib.get_lib()
    assert lib.dfe_error_string(-2) == b"a dimension is out of range"
    # argument validation happens before any launch, so these calls are safe without a GPU
    assert lib.dfe_warp_flow_fwd(None, None, None, 1, 1, 8, 8, 0, 0, None) == -1
    assert lib.dfe_corr_fwd(ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 1, 4, 8, 8, 3, None) == -4
    a = loss_stack.GeomArgs()
    a.B, a.H, a.W, a.num_scales = 4, 256, 832, 3
    assert lib.dfe_geom_workspace_floats(ctypes.byref(a)) > 0
    a.num_scales = 9
    assert lib.dfe_geom_workspace_floats(ctypes.byref(a)) == -2
    a.num_scales, a.mode = 3, 3      # modes 0 (geom), 1 (depth), 2 (flow) exist
    assert lib.dfe_geom_workspace_floats(ctypes.byref(a)) == -4
    # net-glue entry points: NULL / dimension checks, scratch sizes
    P = ctypes.c_void_p(16)
    assert lib.dfe_bias_act_fwd(None, None, 1, 1, 8, 8, 0.1, None) == -1
    assert lib.dfe_bias_act_fwd(P, None, 0, 1, 8, 8, 0.1, None) == -2
    assert lib.dfe_bias_act_bwd(P, P, 10, P, None, None, 1, 4, 8, 8, 0.1, None) == -2      # batch stride < C*H*W
    assert lib.dfe_bias_act_partials_floats(4, 16, 64, 208) == 4 * 16 * 7                  # ceil(13312 / 2048) blocks per plane
    assert lib.dfe_elu_pad_fwd(P, None, P, 1, 1, 1, 5, 1, None) == -2                      # 1-pixel planes cannot be reflected
    assert lib.dfe_elu_pad_bwd(None, None, P, P, None, None, 1, 1, 4, 4, 1, None) == -1    # ELU backward needs x
    assert lib.dfe_elu_up2_cat_pad_fwd(P, None, None, P, 1, 2, 3, 4, 4, None) == -1        # C2 > 0 without a skip tensor
    assert lib.dfe_elu_up2_cat_pad_bwd(P, None, P, None, None, None, None, 1, 2, 0, 4, 4, None) == -1
    assert lib.dfe_glue_partials_floats(2, 3, 16, 16) == 2 * 3 * 1
    assert lib.dfe_bn_partials_floats(3, 4, 64, 64, 208) == 3 * 4 * 64 * 7 * 3
    assert lib.dfe_bn_fwd(P, None, P, P, None, None, P, P, P, P, 1, 1, 4, 1, 1, 1e-5, 0.1, 0, None) == -2   # one value per channel
    assert lib.dfe_bn_fwd(P, None, P, P, None, None, None, P, P, P, 1, 2, 4, 8, 8, 1e-5, 0.1, 0, None) == -1
    assert lib.dfe_bn_bwd(P, None, P, P, P, P, P, None, None, None, P, P, 1, 2, 4, 8, 8, 1, None) == -1       # ReLU mask needs y
    assert lib.dfe_geom_timed_collect(None, None) == -1
    # small-plane convolutions (ops_planeconv.hip): the host-side shape logic runs without a GPU
    assert lib.dfe_planeconv_supported(8, 81, 128, 4, 13) == 1 and lib.dfe_planeconv_supported(8, 211, 128, 8, 26) == 1
    assert lib.dfe_planeconv_supported(8, 64, 64, 64, 208) == 0          # > 4096 pixels per sample: MIOpen's
    assert lib.dfe_planeconv_supported(1, 4, 4, 1, 4000) == 0            # one very wide row does not fit the staging budget
    assert lib.dfe_planeconv_supported(0, 4, 4, 4, 4) == 0
    for (B, Ci, Co, H, W) in [(8, 81, 128, 4, 13), (8, 256, 96, 8, 26), (4, 12, 12, 2, 7), (1, 1, 1, 1, 1)]:
        ws = lib.dfe_planeconv_ws_floats(B, Ci, Co, H, W)
        assert ws >= max(B * Co * H * W, B * Ci * H * W, Co * Ci * 9), (B, Ci, Co, H, W, ws)   # one partial plane of each pass at least
    assert lib.dfe_planeconv_ws_floats(8, 64, 64, 64, 208) == 0
    assert lib.dfe_planeconv_fwd(None, P, None, 0.1, P, 0, None, 0, P, 1, 4, 4, 4, 4, None) == -1
    assert lib.dfe_planeconv_fwd(P, P, None, 0.1, P, 10, None, 0, P, 1, 4, 4, 4, 4, None) == -2      # batch stride < Co*H*W
    assert lib.dfe_planeconv_dgrad(P, P, P, P, 8, 64, 64, 64, 208, None) == -4                        # unsupported: larger plane
    assert lib.dfe_planeconv_wgrad(P, P, None, P, 1, 4, 4, 4, 4, None) == -1
    # fused Winograd convolution (ops_wino.hip) and the tiny 1x1 convolutions: argument checks and scratch sizes
    assert lib.dfe_wino_weight_floats(64, 64) == 64 * 64 * 16 and lib.dfe_wino_weight_floats(5, 33) == 64 * 5 * 16
    assert lib.dfe_wino_weight_floats(0, 4) == 0
    assert lib.dfe_wino_conv3x3(None, P, P, 0, P, 1 << 20, 1, 4, 4, 8, 8, 1, 0, None) == -1
    assert lib.dfe_wino_conv3x3(P, P, P, 4 * 8 * 8, P, 1 << 20, 1, 4, 4, 8, 8, 3, 0, None) == -4  # padding 0, 1 or 2
    assert lib.dfe_wino_conv3x3(P, P, P, 10, P, 1 << 20, 1, 4, 4, 8, 8, 1, 0, None) == -2        # batch stride < Co*Ho*Wo
    assert lib.dfe_wino_conv3x3(P, P, P, 4 * 8 * 8, ctypes.c_void_p(20), 1 << 20, 1, 4, 4, 8, 8, 1, 0, None) == -4   # scratch not 16-byte aligned
    assert lib.dfe_wino_conv3x3(P, P, P, 4 * 8 * 8, P, 10, 1, 4, 4, 8, 8, 1, 0, None) == -5     # scratch smaller than the transformed filters
    assert lib.dfe_wino_scratch_floats(12, 512, 512, 8, 26, 1) > lib.dfe_wino_weight_floats(512, 512)      # small plane: channel splits
    assert lib.dfe_wino_scratch_floats(8, 128, 128, 64, 208, 1) == lib.dfe_wino_weight_floats(128, 128)   # large plane: none
    assert lib.dfe_wino_conv3x3_dilated(P, P, P, 4 * 8 * 9, P, 1, 4, 4, 8, 9, 2, 0, None) == -4  # W not a multiple of the dilation
    assert lib.dfe_wino_conv3x3(P, P, P, 1 << 40, P, 1 << 30, 64, 256, 4, 512, 512, 1, 0, None) == -2   # 32-bit offsets: B*Ci*H*W < 2^30
    assert lib.dfe_wino_wgrad_floats(8, 128, 128, 64, 208, 1) > 0 and lib.dfe_wino_wgrad_floats(8, 128, 128, 64, 208, 2) == 0
    assert lib.dfe_wino_wgrad3x3(P, 4 * 8 * 8, None, 0, P, P, 1, 4, 4, 8, 8, 1, None) == -1
    assert lib.dfe_wino_wgrad3x3(P, 4 * 8 * 8, P, 4 * 8 * 8, P, P, 1, 4, 4, 8, 8, 2, None) == -4 and lib.dfe_wino_wgrad_floats(1, 4, 4, 8, 8, 1) > 0
    assert lib.dfe_wino_conv3x3_u_act(P, None, None, 1.0, P, 4 * 8 * 8, None, 0, None, 0, 1, 4, 4, 8, 8, 1, 1, None) == -1
    # strided weight gradient (csrc/ops_sconv.hip): the planner runs on the host
    assert lib.dfe_sconv_wgrad_floats(12, 3, 64, 256, 832, 7, 2, 3) == 768 * 64 * 3 * 49          # one round of three blocks per CU, one slab
    assert lib.dfe_sconv_wgrad_floats(4, 9, 16, 256, 832, 7, 2, 3) > 0 and lib.dfe_sconv_wgrad_floats(4, 16, 32, 128, 416, 5, 2, 2) > 0
    assert lib.dfe_sconv_wgrad_floats(12, 16, 32, 128, 416, 3, 2, 1) > 0 and lib.dfe_sconv_wgrad_floats(1, 20, 40, 9, 9, 3, 1, 1) > 0
    assert lib.dfe_sconv_wgrad_floats(1, 64, 64, 16, 16, 5, 2, 2) == 0 and lib.dfe_sconv_wgrad_floats(1, 8, 8, 16, 16, 3, 3, 1) == 0
    assert lib.dfe_sconv_wgrad_floats(1, 8, 8, 16, 16, 8, 2, 4) == 0 and lib.dfe_sconv_wgrad_floats(0, 8, 8, 16, 16, 3, 2, 1) == 0
    assert lib.dfe_sconv_wgrad(P, 4 * 8 * 8, None, 0, P, P, 1, 4, 4, 8, 8, 3, 2, 1, None) == -1
    assert lib.dfe_sconv_wgrad(P, 4 * 8 * 8, P, 4 * 4 * 4, P, P, 1, 4, 4, 8, 8, 9, 2, 4, None) == -4
    assert lib.dfe_sconv_wgrad(P, 1, P, 4 * 4 * 4, P, P, 1, 4, 4, 8, 8, 3, 2, 1, None) == -2                # batch stride smaller than a sample
    assert lib.dfe_sconv_tune(0, 0) == 0
    # transformed filters kept across calls: blocks per filter, argument checks
    assert lib.dfe_wino_transform_blocks(64, 64) == 16 and lib.dfe_wino_transform_blocks(5, 33) == 2 and lib.dfe_wino_transform_blocks(0, 3) == 0
    assert lib.dfe_wino_transform_weights_multi(None, P, 4, None) == -1 and lib.dfe_wino_transform_weights_multi(P, P, 0, None) == -2
    assert lib.dfe_wino_conv3x3_u(P, None, P, 4 * 8 * 8, None, 0, 1, 4, 4, 8, 8, 1, 1, None) == -1
    assert lib.dfe_wino_conv3x3_u(P, P, P, 4 * 8 * 8, ctypes.c_void_p(20), 64, 1, 4, 4, 8, 8, 1, 1, None) == -4    # partial sums not 16-byte aligned
    assert lib.dfe_wino_conv3x3_u(P, P, P, 4 * 8 * 9, None, 0, 1, 4, 4, 8, 9, 1, 2, None) == -4    # W not a multiple of the dilation
    assert lib.dfe_wino_conv3x3(P, None, P, 4 * 8 * 8, P, 1 << 20, 1, 4, 4, 8, 8, 1, 0, None) == -1
    assert lib.dfe_conv1x1_small_supported(4, 256, 12, 2, 7) == 1 and lib.dfe_conv1x1_small_supported(4, 16, 16, 64, 208) == 0
    assert lib.dfe_conv1x1_small_fwd(P, None, None, 1.0, P, 4, 12, 12, 2, 7, None) == -1


def test_no_cpu_fallback():
    from unsupervised_depth_opticalflow_egomotion_amd._lib import DfeError
    from unsupervised_depth_opticalflow_egomotion_amd.structures import warp_flow, inverse_warp2
    from unsupervised_depth_opticalflow_egomotion_amd.pytorch_ssim import SSIM
    with pytest.raises(DfeError):
        warp_flow(torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 8, 8))
    with pytest.raises(DfeError):
        SSIM(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    with pytest.raises(AssertionError):
        inverse_warp2(torch.zeros(1, 3, 8, 8), torch.zeros(1, 8, 8), torch.zeros(1, 1, 8, 8), torch.zeros(1, 6), torch.eye(3)[None])


def test_product_never_imports_the_oracle():
    import subprocess, sys
    code = ("import sys; sys.path.insert(0, %r); import unsupervised_depth_opticalflow_egomotion_amd.models, "
            "unsupervised_depth_opticalflow_egomotion_amd.loss_stack, unsupervised_depth_opticalflow_egomotion_amd.ddp; "
            "assert not any(m.startswith('oracle') for m in sys.modules), 'oracle imported by the product'") % REPO
    subprocess.run([sys.executable, "-c", code], check=True)


def test_state_dict_keys_match_reference(golden_dir):
    from core.networks import get_model
    g = np.load(os.path.join(golden_dir, "G7_ac0.npz"))
    m = get_model("geom")(MG.g7_cfg())
    sd = m.state_dict()
    assert list(sd.keys()) == list(g["state_keys"])
    assert [str(tuple(v.shape)) for v in sd.values()] == list(g["state_shapes"])
    assert sum(p.numel() for p in m.parameters()) == 21571085
    for name in ("depth_net", "pose_net", "fpyramid", "pwc_model"):
        assert hasattr(m, name)
    with pytest.raises(ValueError):
        get_model("pose")


def test_config_weights_and_lazy_pack():
    from core.config import generate_loss_weights_dict
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg
    from unsupervised_depth_opticalflow_egomotion_amd.models import LazyPack, LOSS_ORDER_GEOM
    w = generate_loss_weights_dict(make_cfg())
    assert set(w) == set(LOSS_ORDER_GEOM) and w["loss_flow_smooth"] == 10.0 and w["loss_eight_point"] == 0.1
    calls = []
    lp = LazyPack({"a": lambda: calls.append(1) or 5, "b": lambda: 7})
    assert list(lp.keys()) == ["a", "b"] and not calls
    assert lp["a"] == 5 and lp["a"] == 5 and len(calls) == 1
    assert dict(lp.items()) == {"a": 5, "b": 7}


def test_synthetic_dataset_contract():
    from unsupervised_depth_opticalflow_egomotion_amd.synthetic import SyntheticTriplets, make_loss_stack_inputs
    ds = SyntheticTriplets(4, (64, 192), 3)
    img, k, ki = ds[1]
    assert img.shape == (3, 192, 192) and k.shape == (3, 3, 3) and ki.shape == (3, 3, 3)
    assert float(img.min()) >= 0 and float(img.max()) <= 1
    np.testing.assert_allclose((k[1] @ ki[1]).numpy(), np.eye(3), atol=1e-4)
    np.testing.assert_allclose(k[1, 0].numpy(), k[0, 0].numpy() / 2)
    a, b = make_loss_stack_inputs(1, 32, 96, 3, seed=9), make_loss_stack_inputs(1, 32, 96, 3, seed=9)
    assert np.array_equal(a.flows_fwd[0], b.flows_fwd[0]) and len(a.flows_fwd) == 4


def test_profiler_keeps_the_reference_interface(capsys):
    """profiling.Profiler = core/visualize/profiler.py's report_process / report_all / reset (no GPU needed); ranges are free
    when profiling is off."""
    from unsupervised_depth_opticalflow_egomotion_amd import profiling
    assert not profiling.enabled()
    with profiling.range("section"):
        pass
    pr = profiling.Profiler()
    pr.report_process("load")
    pr.report_all("whole")
    out = capsys.readouterr().out
    assert "load\t: " in out and "whole\t: " in out
    quiet = profiling.Profiler(silent=True)
    assert quiet.report_process("x") is None and quiet.report_all("y") is None
    quiet.reset(silent=False)
    assert quiet.silent is False


def _tile_pixel_host(p, W, H, TW, float_path):
    """csrc/loss_stack_exact.h tile_pixel<TW> restated with numpy: the reciprocal-multiply estimate in float32 exactly as the
    device evaluates it + the integer fix-up (float_path), or the integer-division overload."""
    p = p.astype(np.uint32)
    Wu, TR = np.uint32(W), np.uint32(64 // TW)
    LG = {8: 3, 16: 4, 32: 5}[TW]

    def quot(num, den):
        if not float_path:
            return num // np.uint32(den)
        if den == TR * Wu:
            r = np.float32(np.float32(1.0) / np.float32(W)) * np.float32(np.float32(1.0) / np.float32(TR))
            q = ((num.astype(np.float32) + np.float32(0.5)) * r).astype(np.uint32)
        elif den == Wu:
            q = ((num.astype(np.float32) + np.float32(0.5)) * np.float32(np.float32(1.0) / np.float32(W))).astype(np.uint32)
        else:
            q = ((num.astype(np.float32) + np.float32(0.5)) / np.float32(den)).astype(np.uint32)
        lo = q * np.uint32(den)
        return np.where(num < lo, q - 1, np.where(num - lo >= np.uint32(den), q + 1, q)).astype(np.uint32)
    g = quot(p, TR * Wu)
    q = p - g * TR * Wu
    WT = Wu & ~np.uint32(TW - 1)
    inside = g < np.uint32(H) // TR
    full = q < TR * WT
    px_t = np.uint32(TW) * (q >> np.uint32(6)) + (q & np.uint32(TW - 1))
    py_t = TR * g + ((q & np.uint32(63)) >> np.uint32(LG))
    wr = max(int(Wu - WT), 1)
    e = np.where(full, 0, q - TR * WT).astype(np.uint32)
    r = quot(e, np.uint32(wr))
    px_e, py_e = WT + e - r * np.uint32(wr), TR * g + r
    py_r = quot(p, Wu)
    px_r = p - py_r * Wu
    px = np.where(inside, np.where(full, px_t, px_e), px_r)
    py = np.where(inside, np.where(full, py_t, py_e), py_r)
    return px.astype(np.int64), py.astype(np.int64)


@pytest.mark.parametrize("hw", [(256, 832), (128, 416), (64, 208), (375, 1242), (187, 621), (93, 310), (46, 155), (23, 77), (11, 38),
                                (130, 418), (7, 9), (4, 16), (1, 1), (3, 1000), (1024, 4096)])
def test_tile_pixel_is_a_bijection_for_the_kitti_pyramids(hw):
    """the pointwise kernels' pixel order (a wave = a 16 x 4 tile) must visit every pixel exactly once.  Both
    overloads (reciprocal multiply + integer fix-up; integer divisions), every tile width, every level of the 832x256 and the
    1242x375 six-scale pyramids, ragged and large (2^22 pixels: beyond the float estimate's own margin) sizes."""
    H, W = hw
    p = np.arange(H * W, dtype=np.int64)
    for TW in (8, 16, 32):
        ref = None
        for float_path in (True, False):
            px, py = _tile_pixel_host(p, W, H, TW, float_path)
            assert px.min() >= 0 and px.max() < W and py.min() >= 0 and py.max() < H
            lin = py * W + px
            assert np.array_equal(np.sort(lin), p), (hw, TW, float_path)
            ref = lin if ref is None else ref
            assert np.array_equal(lin, ref)          # the two overloads are the same map


# ---------------------------------------------------------------------------------- 2-process gloo DDP
class _TinyNets(torch.nn.Module):
    """Small stand-in for the networks: disparities at 3 scales and a 2x6 pose from the stacked frames."""

    def __init__(self):
        super().__init__()
        self.c = torch.nn.Conv2d(3, 4, 3, padding=1)
        self.d = torch.nn.ModuleList([torch.nn.Conv2d(4, 1, 3, padding=1) for _ in range(3)])
        self.p = torch.nn.Linear(4, 12)

    def forward(self, img):
        f = torch.relu(self.c(img))
        disps = [torch.sigmoid(self.d[s](torch.nn.functional.avg_pool2d(f, 2 ** s) if s else f)) for s in range(3)]
        pose = 0.01 * self.p(f.mean((2, 3))).view(-1, 2, 6)
        return disps, pose


def _ddp_loss(model, batch):
    from oracle import loss_stack_oracle as O
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import total_loss, make_cfg
    il, it, ir, K = batch
    m = model.module if hasattr(model, "module") else model
    dl, _ = m(il); dr, _ = m(ir)
    dt, pose = model(it)
    lp, _ = O.GeomLossOracle(3).depth_losses(il, it, ir, dl, dt, dr, pose, K)
    return total_loss(lp, make_cfg())


def _make_batch(n):
    from unsupervised_depth_opticalflow_egomotion_amd import synthetic
    inp = synthetic.make_loss_stack_inputs(n, 32, 96, 3, seed=321)
    return [torch.from_numpy(a) for a in inp.imgs] + [torch.from_numpy(inp.K)]


def _ddp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    from unsupervised_depth_opticalflow_egomotion_amd import ddp
    torch.set_num_threads(2)
    ddp.init_process_group("gloo")
    torch.manual_seed(0)
    model = ddp.wrap(_TinyNets())
    full = _make_batch(4)
    idx = ddp.shard_indices(4, world, rank)
    shard = [t[idx] for t in full]
    _ddp_loss(model, shard).backward()
    if hasattr(model, "reduce_gradients"):       # strategy "flat": one all-reduce after backward ("torch": DDP reduced during it)
        model.reduce_gradients()
    grads = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    if rank == 0:
        torch.save(grads, out)
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("strategy", ["flat", "torch"])
def test_two_process_gloo_matches_single_process(tmp_path, strategy, monkeypatch):
    """ddp.wrap's two strategies (the flat all-reduce after backward, round 4's default; torch's DistributedDataParallel)."""
    import torch.multiprocessing as mp
    monkeypatch.setenv("DFE_DP_STRATEGY", strategy)      # inherited by the spawned ranks
    out = str(tmp_path / "g.pt")
    port = 29500 + (os.getpid() % 2000) + (7 if strategy == "torch" else 0)
    mp.spawn(_ddp_worker, args=(2, port, out), nprocs=2, join=True)
    g2 = torch.load(out)
    torch.manual_seed(0)
    model = _TinyNets()
    _ddp_loss(model, _make_batch(4)).backward()
    g1 = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    # every loss term is a per-sample (B,) vector with per-sample normalisers and .mean() over the batch, so
    # equal shards + gradient averaging reproduce the single-process gradient
    np.testing.assert_allclose(g2.numpy(), g1.numpy(), rtol=2e-5, atol=1e-7)


class _ThreeBranches(torch.nn.Module):
    """Three independent branches under the joint model's names (depth_net / pose_net / fpyramid + pwc_model)."""

    def __init__(self):
        super().__init__()
        mk = lambda: torch.nn.Sequential(torch.nn.Linear(6, 8), torch.nn.Tanh(), torch.nn.Linear(8, 1))
        self.depth_net, self.pose_net, self.fpyramid, self.pwc_model = mk(), mk(), mk(), torch.nn.Linear(1, 1)

    def forward(self, x, use=("depth", "pose", "flow")):
        out = x.new_zeros(x.shape[0], 1)
        if "flow" in use:
            out = out + self.pwc_model(self.fpyramid(x))
        if "pose" in use:
            out = out + 2.0 * self.pose_net(x)
        if "depth" in use:
            out = out + 3.0 * self.depth_net(x)
        return out


def _branch_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    from unsupervised_depth_opticalflow_egomotion_amd import ddp
    torch.set_num_threads(1)
    ddp.init_process_group("gloo")
    torch.manual_seed(0)
    net = _ThreeBranches()
    model = ddp.wrap(net)
    assert type(model).__name__ == "FlatAllReduce" and model.branches == ["depth_net", "pose_net", "flow"]
    torch.manual_seed(5)
    x = torch.randn(8, 6)
    xs = x[ddp.shard_indices(8, world, rank)]
    res = {}

    def grads():
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}
    # step 1: calibration (no trigger yet: everything is reduced in reduce_gradients); step 2: the three messages leave from backward
    for step in (1, 2):
        net.zero_grad()
        model(xs).pow(2).mean().backward()
        model.reduce_gradients()
        res["step%d" % step] = grads()
    res["early_hits"] = model.early_hits
    res["order"], res["triggers"] = list(model._order), dict(model.triggers)
    res["in_flat"] = all(model._flat.data_ptr() <= p.grad.data_ptr() < model._flat.data_ptr() + 4 * model._flat.numel()
                         for p in net.parameters())
    res["bytes"] = model.message_bytes()
    # a gradient that changes after its branch's message left (second backward pass before the step): reduced again
    net.zero_grad()
    model(xs).pow(2).mean().backward()
    model(xs).abs().mean().backward()
    model.reduce_gradients()
    res["two_backwards"] = grads()
    # ranks whose sets of parameters with gradients differ: rank 1 runs without the pose branch, nobody runs the flow branch
    net.zero_grad()
    model(xs, use=("depth", "pose") if rank == 0 else ("depth",)).pow(2).mean().backward()
    model.reduce_gradients()
    res["partial"] = grads()
    # a rank without any gradient still joins the collectives
    net.zero_grad()
    if rank == 0:
        model(xs).pow(2).mean().backward()
    model.reduce_gradients()
    res["one_rank"] = grads()
    torch.save(res, out + str(rank))
    torch.distributed.destroy_process_group()


def test_branch_overlapped_reducer_two_ranks(tmp_path, monkeypatch):
    """ddp.FlatAllReduce (round 5): one all-reduce per network branch, issued from backward by ONE hook per branch.  Two gloo
    ranks: gradients equal the single-process ones; from step 2 on all three messages leave during backward; a second
    backward pass before the step is detected and reduced again; ranks with different sets of gradients neither hang nor
    diverge (a gradient on any rank -> the averaged gradient on every rank; none anywhere -> None)."""
    import torch.multiprocessing as mp
    monkeypatch.setenv("DFE_DP_STRATEGY", "flat")
    out = str(tmp_path / "b.pt")
    mp.spawn(_branch_worker, args=(2, 29500 + (os.getpid() % 2000) + 19, out), nprocs=2, join=True)
    r0, r1 = torch.load(out + "0"), torch.load(out + "1")
    torch.manual_seed(0)
    net = _ThreeBranches()
    torch.manual_seed(5)
    x = torch.randn(8, 6)

    def single(loss_fns, use=("depth", "pose", "flow")):
        net.zero_grad()
        for f in loss_fns:
            # equal shards + averaging = the mean over the two shards' losses
            sum(f(net(x[i::2], use)) for i in (0, 1)).mul(0.5).backward()
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}
    sq, ab = (lambda y: y.pow(2).mean()), (lambda y: y.abs().mean())
    ref = single([sq])
    for r in (r0, r1):
        for key in ("step1", "step2"):
            for n in ref:
                np.testing.assert_allclose(r[key][n].numpy(), ref[n].numpy(), rtol=1e-5, atol=1e-7, err_msg=key + n)
        assert r["early_hits"] >= 3 and r["in_flat"] and sorted(r["order"]) == ["depth_net", "flow", "pose_net"]
        assert r["bytes"] == {"depth_net": 4 * (65 + 4), "pose_net": 4 * (65 + 4), "flow": 4 * (67 + 6)}
        # the trigger of a branch = its FIRST layer's weight or bias (the last gradient backward produces there)
        assert r["triggers"]["depth_net"].startswith("depth_net.0.") and r["triggers"]["flow"].startswith("fpyramid.0.")
    assert r0["order"] == r1["order"]
    ref2 = single([sq, ab])
    for r in (r0, r1):
        for n in ref2:
            np.testing.assert_allclose(r["two_backwards"][n].numpy(), ref2[n].numpy(), rtol=1e-5, atol=1e-7, err_msg="two " + n)
    # partial: depth from both ranks; pose only from rank 0 (averaged with rank 1's zeros); flow from nobody
    net.zero_grad()
    (0.5 * (sq(net(x[0::2], ("depth", "pose"))) + sq(net(x[1::2], ("depth",))))).backward()
    for r in (r0, r1):
        for n, p in net.named_parameters():
            if n.startswith(("fpyramid", "pwc_model")):
                assert r["partial"][n] is None, n
            else:
                np.testing.assert_allclose(r["partial"][n].numpy(), p.grad.numpy(), rtol=1e-5, atol=1e-7, err_msg="partial " + n)
    net.zero_grad()
    (0.5 * sq(net(x[0::2]))).backward()
    for r in (r0, r1):
        for n, p in net.named_parameters():
            np.testing.assert_allclose(r["one_rank"][n].numpy(), p.grad.numpy(), rtol=1e-5, atol=1e-7, err_msg="one " + n)


def _diverging_first_step_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank), LOCAL_RANK=str(rank))
    from unsupervised_depth_opticalflow_egomotion_amd import ddp
    torch.set_num_threads(1)
    ddp.init_process_group("gloo")
    torch.manual_seed(0)
    net = _ThreeBranches()
    model = ddp.wrap(net)
    torch.manual_seed(5)
    x = torch.randn(8, 6)
    xs = x[ddp.shard_indices(8, world, rank)]
    res = {"armed_after": []}

    def grads():
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}
    # step 1: rank 1 runs WITHOUT the pose branch; step 2: rank 0 has no gradient at all; step 3: both complete -> the ranks
    # agree and arm; step 4: the messages leave from backward in the agreed order
    plans = [(("depth", "pose", "flow"), ("depth", "flow")), (None, ("depth", "pose", "flow")),
             (("depth", "pose", "flow"),) * 2, (("depth", "pose", "flow"),) * 2]
    for step, plan in enumerate(plans, 1):
        net.zero_grad()
        if plan[rank] is not None:
            model(xs, use=plan[rank]).pow(2).mean().backward()
        model.reduce_gradients()
        res["step%d" % step] = grads()
        res["armed_after"].append(model._order is not None)
    res["order"], res["calibration_steps"], res["early_hits"] = list(model._order), model.calibration_steps, model.early_hits
    # a backward pass whose optimiser step is skipped, then zero_grad + a new backward pass: the early messages of the
    # skipped pass must not be handed out as this pass's gradients
    net.zero_grad()
    model(xs).abs().mean().backward()
    net.zero_grad()
    model(xs).pow(2).mean().backward()
    model.reduce_gradients()
    res["after_skip"] = grads()
    torch.save(res, out + str(rank))
    torch.distributed.destroy_process_group()


def test_reducer_first_backward_differs_between_ranks(tmp_path, monkeypatch):
    """VERDICT r05 item 7 / ADVICE r05 (medium): the issue order of the per-branch all-reduces is a cross-rank agreement.  A
    rank whose FIRST backward pass lacks a branch (or has no gradient at all) keeps every rank in calibration -- static
    order, identical message sizes -- instead of arming a local order the other rank does not share (which aborted gloo
    with a size mismatch and would hang RCCL)."""
    import torch.multiprocessing as mp
    monkeypatch.setenv("DFE_DP_STRATEGY", "flat")
    out = str(tmp_path / "d.pt")
    mp.spawn(_diverging_first_step_worker, args=(2, 29500 + (os.getpid() % 2000) + 23, out), nprocs=2, join=True)
    r0, r1 = torch.load(out + "0"), torch.load(out + "1")
    torch.manual_seed(0)
    net = _ThreeBranches()
    torch.manual_seed(5)
    x = torch.randn(8, 6)
    sq = lambda y: y.pow(2).mean()

    def single(use0, use1):
        net.zero_grad()
        parts = [sq(net(x[i::2], u)) for i, u in ((0, use0), (1, use1)) if u is not None]
        (0.5 * sum(parts)).backward()
        return {n: (None if p.grad is None else p.grad.clone()) for n, p in net.named_parameters()}
    full = ("depth", "pose", "flow")
    refs = {"step1": single(full, ("depth", "flow")), "step2": single(None, full), "step3": single(full, full),
            "step4": single(full, full), "after_skip": single(full, full)}
    for r in (r0, r1):
        assert r["armed_after"] == [False, False, True, True] and r["calibration_steps"] == 3
        assert r["early_hits"] >= 3
        for key, ref in refs.items():
            for n in ref:
                assert r[key][n] is not None, (key, n)
                np.testing.assert_allclose(r[key][n].numpy(), ref[n].numpy(), rtol=1e-5, atol=1e-7, err_msg=key + " " + n)
    assert r0["order"] == r1["order"] and sorted(r0["order"]) == ["depth_net", "flow", "pose_net"]


class _RealDepthNets(torch.nn.Module):
    """The product's own Depth_Model (ResNet-18 encoder incl. the never-used fc, grouped BatchNorm, fused-decoder
    modules on their host path) under a ``depth_net.`` prefix like Model_depth, plus a learnable pose."""

    def __init__(self):
        super().__init__()
        from unsupervised_depth_opticalflow_egomotion_amd.networks import Depth_Model
        self.depth_net = Depth_Model(3)
        self.pose = torch.nn.Parameter(0.01 * torch.randn(2, 6))

    def forward(self, il, it, ir):
        dl, dt, dr = self.depth_net.forward_frames([il, it, ir])
        return dl, dt, dr, self.pose.unsqueeze(0).expand(il.shape[0], 2, 6)


def _real_loss(model, batch):
    from oracle import loss_stack_oracle as O
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import total_loss, make_cfg
    il, it, ir, K = batch
    dl, dt, dr, pose = model(il, it, ir)
    lp, _ = O.GeomLossOracle(3).depth_losses(il, it, ir, dl, dt, dr, pose, K)
    return total_loss(lp, make_cfg())


def _real_batch(n):
    from unsupervised_depth_opticalflow_egomotion_amd import synthetic
    inp = synthetic.make_loss_stack_inputs(n, 64, 192, 3, seed=654)
    return [torch.from_numpy(a) for a in inp.imgs] + [torch.from_numpy(inp.K)]


def _real_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE=str(world), RANK=str(rank),
                      LOCAL_RANK=str(rank))
    from unsupervised_depth_opticalflow_egomotion_amd import ddp
    torch.set_num_threads(2)
    ddp.init_process_group("gloo")
    torch.manual_seed(0)
    net = _RealDepthNets()
    net.eval()                        # BatchNorm on running statistics: sharding-invariant, so gradients can be compared
    model = ddp.wrap(net)
    flat = os.environ.get("DFE_DP_STRATEGY", "flat") == "flat"
    assert type(model).__name__ == ("FlatAllReduce" if flat else "DistributedDataParallel")
    full = _real_batch(2)
    idx = ddp.shard_indices(2, world, rank)
    _real_loss(model, [t[idx] for t in full]).backward()
    if flat:
        model.reduce_gradients()
        assert model.ignored == ["depth_net.encoder.encoder.fc.bias", "depth_net.encoder.encoder.fc.weight"]
    named = dict(net.named_parameters())
    fc = [n for n in named if ".fc." in n]
    assert len(fc) == 2 and all(named[n].grad is None and named[n].requires_grad for n in fc)   # ignored, not frozen
    grads = torch.cat([p.grad.reshape(-1) for n, p in named.items() if n not in fc])
    # one train-mode step under DDP as well (per-replica grouped BatchNorm statistics, buffers broadcast)
    net.train()
    net.zero_grad()
    _real_loss(model, [t[idx] for t in full]).backward()
    if flat:
        model.reduce_gradients()
        assert all(p.grad.data_ptr() >= model._flat.data_ptr() and p.grad.data_ptr() < model._flat.data_ptr() + 4 * model._flat.numel()
                   for n, p in named.items() if n not in fc)          # the reduced gradients are views of the flat buffer
    assert all(torch.isfinite(p.grad).all() for n, p in named.items() if n not in fc)
    if rank == 0:
        torch.save(grads, out)
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize("strategy", ["flat", "torch"])
def test_two_process_gloo_real_depth_nets(tmp_path, strategy, monkeypatch):
    """world_size 2 over gloo with the PRODUCT's networks (not a stand-in): both data-parallel strategies reproduce the
    single-process gradient, and the never-used ``encoder.fc`` parameters are excluded from the reduction while staying in
    the optimizer's parameter list (reference optimizer-state compatibility, train.py:85-87)."""
    import torch.multiprocessing as mp
    from unsupervised_depth_opticalflow_egomotion_amd import ddp
    monkeypatch.setenv("DFE_DP_STRATEGY", strategy)
    out = str(tmp_path / "g.pt")
    port = 31500 + (os.getpid() % 2000) + (7 if strategy == "torch" else 0)
    mp.spawn(_real_worker, args=(2, port, out), nprocs=2, join=True)
    g2 = torch.load(out)
    torch.manual_seed(0)
    net = _RealDepthNets()
    net.eval()
    _real_loss(net, _real_batch(2)).backward()
    fc = set(ddp.unused_parameter_names(net))
    assert fc == {"depth_net.encoder.encoder.fc.weight", "depth_net.encoder.encoder.fc.bias"}
    g1 = torch.cat([p.grad.reshape(-1) for n, p in net.named_parameters() if n not in fc])
    scale = float(g1.abs().max())
    assert float((g2 - g1).abs().max()) <= 2e-5 * scale + 1e-7
    # optimizer parameter group = every parameter, in order, like the reference's Adam (fc included)
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=1e-4)
    assert len(opt.param_groups[0]["params"]) == len(list(net.parameters()))
    ref_like = torch.optim.Adam(list(net.parameters()), lr=1e-4).state_dict()
    opt.load_state_dict(ref_like)     # a reference-layout optimizer state loads (same group size and indexing)


def test_strict_seeds_are_margin_checked():
    """The seeds the GPU parity tests demand EXACT mask equality on have no pixel inside any mask's fp32 noise floor
    (tests/_margins.py), in both align_corners modes; robust_pose makes cos / sin unambiguous."""
    from tests import _margins as M
    from unsupervised_depth_opticalflow_egomotion_amd import synthetic
    strict = {(2, 32, 96): 932, (2, 64, 208): 77, (2, 128, 448): 600, (1, 256, 832): 1219}   # = test_hip_loss_stack.STRICT
    for (b, h, w), seed in strict.items():
        inp = synthetic.make_loss_stack_inputs(b, h, w, 3, seed=seed)
        ang = inp.pose[..., 3:].astype(np.float64)
        for fn in (np.cos, np.sin):      # exact value within 0.3 ulp of its nearest float32
            v = fn(ang)
            r = v.astype(np.float32)
            assert (np.abs(v - r.astype(np.float64)) / np.spacing(np.abs(r)).astype(np.float64) < 0.3).all()
        for ac in (False, True):
            within = M.within_counts(M.geom_margins(inp, ac, 3))
            assert sum(within.values()) == 0, ((b, h, w), seed, ac, within)


def test_evaluation_metrics_match_the_reference_formulas():
    """Device-side eval_flow_avg / eval_depth against the numpy restatement of
    evaluate_flow.py:85-174 and evaluate_depth.py:13-52, same signatures and return formats (run on CPU tensors here)."""
    from oracle import eval_oracle as EO
    from core.evaluation import eval_flow_avg, eval_depth
    r = np.random.default_rng(5)
    cfg = types.SimpleNamespace(img_hw=(64, 208))
    gts, nocs, preds, moves = [], [], [], []
    for _ in range(3):
        H, W = 93, 310
        gt = np.concatenate([6 * r.standard_normal((H, W, 2)), (r.random((H, W, 1)) > 0.3)], 2).astype(np.float32)
        noc = (gt[:, :, 2] * (r.random((H, W)) > 0.2)).astype(np.float32)
        gts.append(gt); nocs.append(noc); moves.append((r.random((H, W)) > 0.7).astype(np.float32))
        preds.append((2 * r.standard_normal((64, 208, 2))).astype(np.float32))
    ref = EO.eval_flow_avg(gts, nocs, preds, cfg.img_hw, moves)
    out = eval_flow_avg(gts, nocs, [torch.from_numpy(p) for p in preds], cfg, moving_masks=moves)
    vals = [float(v) for v in out.strip().split("\n")[1].split(",")]
    # table order: epe, noc, occ, move, static, move_rate, static_rate, err_rate
    np.testing.assert_allclose(vals, [ref[0], ref[1], ref[2], ref[4], ref[5], ref[6], ref[7], ref[3]], atol=6e-5, rtol=1e-4)
    out4 = eval_flow_avg(gts, nocs, preds, cfg)
    assert out4.split("\n")[0].split(",")[-1].strip() == "err_rate" and len(out4.strip().split("\n")[1].split(",")) == 4
    gtd = [np.where(r.random((375, 1242)) > 0.9, r.uniform(1, 90, (375, 1242)), 0).astype(np.float32) for _ in range(2)]
    prd = [r.uniform(0.5, 60, (375, 1242)).astype(np.float32) for _ in range(2)]
    np.testing.assert_allclose(eval_depth(gtd, [torch.from_numpy(p) for p in prd]), EO.eval_depth(gtd, prd), rtol=2e-5)


def test_evaluation_metrics_vs_reference_golden(golden_dir):
    """core.evaluation (the product's eval_flow_avg / eval_depth, here on CPU tensors) against golden G10 -- the tables the
    reference's own evaluate_flow / evaluate_depth printed for the same inputs."""
    from core.evaluation import eval_flow_avg, eval_depth
    from tests.golden import make_golden as MG
    g = np.load(os.path.join(golden_dir, "G10.npz"))
    c = MG.g10_inputs()
    cfg = types.SimpleNamespace(img_hw=c["hw"])
    vals = lambda t: [float(v) for v in str(t).strip().split("\n")[1].split(",")]   # noqa: E731
    out = eval_flow_avg(c["gt_flows"], c["nocs"], [torch.from_numpy(p) for p in c["preds"]], cfg, moving_masks=c["movs"])
    assert out.split("\n")[0] == str(g["flow_table_moving"]).split("\n")[0]          # same header line
    np.testing.assert_allclose(vals(out), vals(g["flow_table_moving"]), atol=1.01e-4)
    out = eval_flow_avg(c["gt_flows"], c["nocs"], c["preds"], cfg)
    np.testing.assert_allclose(vals(out), vals(g["flow_table"]), atol=1.01e-4)
    np.testing.assert_allclose(eval_depth(c["gt_depths"], [torch.from_numpy(p) for p in c["pred_depths"]]), g["depth_metrics"], rtol=2e-5)


def test_kitti_png_codec_and_readers(tmp_path):
    """kitti_io: the own PNG codec (16-bit RGB is what KITTI's flow ground truth uses and PIL truncates) against PIL on
    what PIL can write, every row filter type on hand-encoded files, and the flow / mask / calibration readers."""
    import struct, zlib
    from PIL import Image
    from unsupervised_depth_opticalflow_egomotion_amd import kitti_io as K
    r = np.random.default_rng(0)
    yy, xx = np.mgrid[0:60, 0:90]
    smooth = ((np.sin(xx / 9.0) + np.cos(yy / 7.0)) * 60 + 128).astype(np.uint8)
    for name, arr in (("noise8", (r.random((37, 53, 3)) * 255).astype(np.uint8)), ("smooth8", np.stack([smooth, smooth // 2, 255 - smooth], 2)),
                      ("grey16", (np.sin(xx / 30.0) * 20000 + 30000).astype(np.uint16)), ("grey8", smooth)):
        Image.fromarray(arr).save(str(tmp_path / (name + ".png")), optimize=True)      # PIL picks row filters adaptively
        assert np.array_equal(K.read_png(str(tmp_path / (name + ".png"))), arr), name

    def encode16(img, ftypes):
        h, w, ch = img.shape
        bpp, stride = ch * 2, w * ch * 2
        raw = img.astype(">u2").tobytes()
        prev, out = np.zeros(stride, np.int32), b""
        for y in range(h):
            row = np.frombuffer(raw[y * stride:(y + 1) * stride], np.uint8).astype(np.int32)
            left = np.concatenate([np.zeros(bpp, np.int32), row[:-bpp]])
            ul = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]])
            ft = ftypes[y % len(ftypes)]
            p = left + prev - ul
            pa, pb, pc = abs(p - left), abs(p - prev), abs(p - ul)
            pred = [0, left, prev, (left + prev) >> 1, np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))][ft]
            out += bytes([ft]) + ((row - pred) & 255).astype(np.uint8).tobytes()
            prev = row
        ck = lambda k, b: struct.pack(">I", len(b)) + k + b + struct.pack(">I", zlib.crc32(k + b) & 0xFFFFFFFF)   # noqa: E731
        return b"\x89PNG\r\n\x1a\n" + ck(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0)) + ck(b"IDAT", zlib.compress(out)) + ck(b"IEND", b"")
    img = (r.random((23, 31, 3)) * 65535).astype(np.uint16)
    for fts in ([0], [1], [2], [3], [4], [0, 1, 2, 3, 4], [4, 3, 1]):
        (tmp_path / "e.png").write_bytes(encode16(img, fts))
        assert np.array_equal(K.read_png(str(tmp_path / "e.png")), img), fts
    K.write_png(str(tmp_path / "w.png"), img)
    assert np.array_equal(K.read_png(str(tmp_path / "w.png")), img)
    flow = r.normal(0, 20, (20, 30, 2))
    valid = r.random((20, 30)) > 0.3
    K.write_flow_png(str(tmp_path / "f.png"), flow, valid)
    back = K.read_flow_png(str(tmp_path / "f.png"))
    assert np.array_equal(back[:, :, 2] > 0, valid) and np.abs(back[:, :, :2] - flow * valid[:, :, None]).max() <= 1 / 64
    (tmp_path / "c.txt").write_text("calib_time: 09-Jan-2012 13:57:47\nP_rect_02: 7.2e+02 0 6.1e+02 4.4e+01 0 7.2e+02 1.7e+02 2.1e-01 0 0 1 2.7e-03\n")
    assert np.allclose(K.load_intrinsics_raw(str(tmp_path / "c.txt")), [[720, 0, 610], [0, 720, 170], [0, 0, 1]])
    up = K.resize_bilinear_u8(np.arange(12, dtype=np.uint8).reshape(3, 4), (6, 8))
    ref = torch.nn.functional.interpolate(torch.arange(12.).reshape(1, 1, 3, 4), (6, 8), mode="bilinear", align_corners=False)[0, 0].numpy()
    assert np.allclose(up, ref, atol=1e-5)
    gt = np.stack([np.eye(3, 4)] * 3); gt[1, 0, 3] = 1.0; gt[2, 0, 3] = 2.0
    ate, re = K.compute_pose_error(gt, gt * np.array([1, 1, 1, 0.5]))
    assert ate < 1e-12 and re < 1e-12          # the ATE is invariant to the prediction's scale


@pytest.mark.parametrize("ac", [False, True])
def test_triangulation_family_vs_reference_golden(golden_dir, ac):
    """geometry_solvers: mid-point triangulation, reprojection, depth registration, affine / scale
    fits, triangulation loss, top-ratio and random match sampling against golden G11 -- the reference's own methods
    (model_geometry.py:427-470, 569-683) called unbound on a bare object.  Pure torch: runs on the host here."""
    from tests.golden import make_golden as MG
    from unsupervised_depth_opticalflow_egomotion_amd import ops
    from unsupervised_depth_opticalflow_egomotion_amd.geometry_solvers import GeometrySolvers
    from unsupervised_depth_opticalflow_egomotion_amd.loss_terms import LossTerms

    class M(LossTerms, GeometrySolvers):
        ratio, num = 0.3, 50
    g = np.load(os.path.join(golden_dir, "G11_ac%d.npz" % ac))
    c = MG.g11_inputs()
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float()   # noqa: E731
    m = M()
    K, match = T(c["K"]), T(c["match"])
    Ki = torch.inverse(K)
    P1 = K.bmm(torch.cat([torch.eye(3), torch.zeros(3, 1)], -1).unsqueeze(0).repeat(K.shape[0], 1, 1))
    P2 = T(g["P2"])
    close = lambda a, b, tol=2e-5: np.testing.assert_allclose(a.detach().numpy(), b, rtol=tol, atol=tol * max(1.0, float(np.abs(b).max())))   # noqa: E731
    old = ops.get_align_corners()
    ops.set_align_corners(ac)
    try:
        pts = m.midpoint_triangulate(match, K, Ki, P1, P2)
        close(pts, g["points"], 1e-4)
        c1, z1 = m.reproject(P1, T(g["points"]))
        c2, z2 = m.reproject(P2, T(g["points"]))
        close(c1, g["coord1"], 1e-4); close(z1, g["depth1"]); close(c2, g["coord2"], 1e-4); close(z2, g["depth2"])
        d1 = T(c["depth1"])
        r1, i1 = m.register_depth(d1, T(g["coord1"]), T(g["depth1"]))
        close(r1, g["reg_pred1"], 1e-4); close(i1, g["reg_inter1"], 1e-4)
        a, b = m.affine_adapt(T(g["reg_inter1"]), T(g["depth1"]).abs() + 0.5, use_translation=True)
        close(a, g["affine_a"], 1e-3); close(b, g["affine_b"], 1e-3)
        close(m.scale_adapt(T(g["reg_inter1"]), T(g["depth1"]).abs() + 0.5), g["scale_a"], 1e-4)
        loss = m.get_trian_loss(T(g["depth1"]), T(g["reg_inter1"]))
        assert loss.shape == (2,)
        flow, score = T(c["flow"]), T(c["score"])
        bsz, _, h, w = flow.shape
        grid = m.meshgrid(bsz, h, w)
        full = torch.cat([grid, grid + flow], 1).view(bsz, 4, -1)
        tm, td, ts = m.top_ratio_sample(full, d1.view(bsz, 1, -1), score.view(bsz, 1, -1), 0.3)
        assert np.array_equal(tm.numpy(), g["top_match"]) and np.array_equal(td.numpy(), g["top_depth"]) and np.array_equal(ts.numpy(), g["top_score"])
        torch.manual_seed(1111)
        sm, sd = m.sample_match(flow, d1, score)
        assert np.array_equal(sm.numpy(), g["sample_match"]) and np.array_equal(sd.numpy(), g["sample_depth"])
    finally:
        ops.set_align_corners(old)


def test_eight_point_properties():
    """compute_fundmental_mat (normalised eight-point, batched; stands in for cv2.findFundamentalMat, which is absent and
    random): exact recovery of a known F from noise-free matches, rank 2, F[2,2] = 1, invariance to the order of the
    matches, graceful least squares under noise."""
    from unsupervised_depth_opticalflow_egomotion_amd.geometry_solvers import GeometrySolvers
    r = np.random.default_rng(3)
    b, n = 3, 64
    K = np.array([[480.0, 0, 416], [0, 490, 128], [0, 0, 1]])
    Fs, ms = [], []
    for i in range(b):
        ang = 0.05 * r.standard_normal(3)
        cx, sx, cy, sy, cz, sz = np.cos(ang[0]), np.sin(ang[0]), np.cos(ang[1]), np.sin(ang[1]), np.cos(ang[2]), np.sin(ang[2])
        R = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
        t = np.array([0.5, 0.05, 0.1]) + 0.05 * r.standard_normal(3)
        X = np.stack([r.uniform(-4, 4, n), r.uniform(-1.5, 1.5, n), r.uniform(4, 30, n)])
        x1 = K @ X
        x2 = K @ (R @ X + t[:, None])
        ms.append(np.concatenate([x1[:2] / x1[2], x2[:2] / x2[2]], 0))
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        Fm = np.linalg.inv(K).T @ tx @ R @ np.linalg.inv(K)
        Fs.append(Fm / Fm[2, 2])
    m = torch.from_numpy(np.stack(ms)).float()
    est = GeometrySolvers().compute_fundmental_mat(m).double().numpy()
    for i in range(b):
        assert abs(est[i][2, 2] - 1.0) < 1e-6 and abs(np.linalg.det(est[i])) < 1e-9 * np.abs(est[i]).max() ** 3 + 1e-18
        np.testing.assert_allclose(est[i], Fs[i], rtol=2e-3, atol=2e-3 * np.abs(Fs[i]).max())
        x1 = np.concatenate([ms[i][:2], np.ones((1, n))]); x2 = np.concatenate([ms[i][2:], np.ones((1, n))])
        res = np.abs(np.sum(x2 * (est[i] @ x1), 0)) / (np.linalg.norm((est[i] @ x1)[:2], axis=0) + 1e-12)
        assert res.max() < 5e-2                                  # epipolar distance in pixels (float32 matches)
    perm = torch.randperm(n)
    np.testing.assert_allclose(GeometrySolvers().compute_fundmental_mat(m[:, :, perm]).numpy(), est, rtol=1e-3, atol=1e-5)
    noisy = GeometrySolvers().compute_fundmental_mat(m + 0.2 * torch.randn_like(m)).numpy()
    assert np.isfinite(noisy).all()


def test_kitti_pose_snippets_are_rgb_like_the_reference_loader(tmp_path):
    """The reference's odometry loader reads frames with imageio (RGB, core/dataset/kitti_pose.py:6,18) while its flow and
    depth loaders use cv2 (BGR): KITTIPoseSnippets must hand infer_pose RGB frames."""
    from PIL import Image
    from unsupervised_depth_opticalflow_egomotion_amd import kitti_io
    root = tmp_path / "odom"
    (root / "sequences" / "09" / "image_2").mkdir(parents=True)
    (root / "poses").mkdir()
    rgb = np.zeros((4, 6, 3), np.uint8)
    rgb[..., 0], rgb[..., 1], rgb[..., 2] = 200, 100, 50
    for i in range(3):
        Image.fromarray(rgb).save(str(root / "sequences" / "09" / "image_2" / ("%06d.png" % i)))
    eye = np.hstack([np.eye(3), np.zeros((3, 1))]).reshape(-1)
    np.savetxt(str(root / "poses" / "09.txt"), np.stack([eye, eye, eye]))
    ds = kitti_io.KITTIPoseSnippets(str(root), ["09"], 3)
    assert len(ds) == 1
    img = ds[0]["imgs"][0]
    assert img.dtype == np.uint8 and tuple(img[0, 0]) == (200, 100, 50)                       # R, G, B
    assert tuple(kitti_io.read_image_bgr(str(root / "sequences" / "09" / "image_2" / "000000.png"))[0, 0]) == (50, 100, 200)


def test_ransac_solvers_reject_gross_outliers():
    """The robust half of SURVEY 8(f) rank 4 (model_geometry.py:473-566: cv2.findFundamentalMat(FM_RANSAC, 0.1, 0.99) /
    FM_LMEDS, cv2.solvePnPRansac(reprojectionError=1)): with 30 % gross outliers among the matches the batched RANSAC
    recovers F and the pose within 1e-2; the all-match least squares of round 3 does not."""
    from unsupervised_depth_opticalflow_egomotion_amd.geometry_solvers import GeometrySolvers as GS
    r = np.random.default_rng(5)
    b, n = 2, 400
    K = torch.tensor([[480.0, 0, 416], [0, 490, 128], [0, 0, 1]], dtype=torch.float64)
    w = torch.from_numpy(0.06 * r.standard_normal((b, 3)))
    T = torch.from_numpy(np.array([[0.5, 0.05, 0.1]]) + 0.1 * r.standard_normal((b, 3)))
    R = GS._so3_exp(w)
    X = torch.from_numpy(np.stack([r.uniform(-4, 4, (b, n)), r.uniform(-1.5, 1.5, (b, n)), r.uniform(4, 30, (b, n))], 2))
    Y = X.bmm(R.transpose(1, 2)) + T.unsqueeze(1)
    proj = lambda P: torch.stack([480 * P[:, :, 0] / P[:, :, 2] + 416, 490 * P[:, :, 1] / P[:, :, 2] + 128], 2)   # noqa: E731
    x1, x2 = proj(X), proj(Y) + torch.from_numpy(0.02 * r.standard_normal((b, n, 2)))
    no = int(0.3 * n)
    x2[:, :no] += torch.from_numpy(r.uniform(-60, 60, (b, no, 2)))
    matches = torch.cat([x1.transpose(1, 2), x2.transpose(1, 2)], 1).float()
    tx = torch.zeros(b, 3, 3, dtype=torch.float64)
    tx[:, 0, 1], tx[:, 0, 2], tx[:, 1, 0], tx[:, 1, 2], tx[:, 2, 0], tx[:, 2, 1] = -T[:, 2], T[:, 1], T[:, 2], -T[:, 0], -T[:, 1], T[:, 0]
    Ft = torch.inverse(K).t().unsqueeze(0).matmul(tx.bmm(R)).matmul(torch.inverse(K).unsqueeze(0))
    Ft = Ft / Ft[:, 2:3, 2:3]
    rel = lambda A: float(((A.double() - Ft).abs().amax((1, 2)) / Ft.abs().amax((1, 2))).max())   # noqa: E731
    m = GS()
    assert rel(m.compute_fundmental_mat(matches)) <= 1e-2
    assert rel(m.compute_fundmental_mat(matches, robust=False)) > 2e-2
    m.dataset = "nyuv2"                    # cv2.FM_LMEDS
    assert rel(m.compute_fundmental_mat(matches)) <= 1e-2
    est = GS().pnp(x2.float(), X.float(), K.float())
    assert float((est[:, :3].double() - T).abs().max()) <= 1e-2 and float((est[:, 3:].double() - w).abs().max()) <= 1e-2
    lsq = GS().pnp(x2.float(), X.float(), K.float(), robust=False)
    assert max(float((lsq[:, :3].double() - T).abs().max()), float((lsq[:, 3:].double() - w).abs().max())) > 2e-2
    assert torch.equal(est, GS().pnp(x2.float(), X.float(), K.float()))      # seeded draw: reproducible


def test_pnp_properties():
    """pnp (batched Levenberg-Marquardt on SE(3); stands in for cv2.solvePnPRansac + solvePnP): exact recovery of a known
    pose from noise-free 3-D / 2-D correspondences, from the identity and from a perturbed start, in the reference's
    (T, axis-angle) output convention; small noise moves the answer by a comparable amount."""
    from unsupervised_depth_opticalflow_egomotion_amd.geometry_solvers import GeometrySolvers as GS
    r = np.random.default_rng(8)
    b, n = 3, 120
    K = torch.tensor([[480.0, 0, 416], [0, 490, 128], [0, 0, 1]])
    w = torch.from_numpy(0.08 * r.standard_normal((b, 3))).float()
    T = torch.from_numpy(np.array([[0.5, 0.05, 0.1]]) + 0.1 * r.standard_normal((b, 3))).float()
    R = GS._so3_exp(w.double())
    X = torch.from_numpy(np.stack([r.uniform(-4, 4, (b, n)), r.uniform(-1.5, 1.5, (b, n)), r.uniform(4, 30, (b, n))], 2))
    Y = X.bmm(R.transpose(1, 2)) + T.double().unsqueeze(1)
    x = torch.stack([480 * Y[:, :, 0] / Y[:, :, 2] + 416, 490 * Y[:, :, 1] / Y[:, :, 2] + 128], 2)
    np.testing.assert_allclose(GS._so3_log(R).numpy(), w.double().numpy(), atol=1e-9)
    est = GS().pnp(x.float(), X.float(), K)
    np.testing.assert_allclose(est[:, :3].numpy(), T.numpy(), atol=2e-3)
    np.testing.assert_allclose(est[:, 3:].numpy(), w.numpy(), atol=5e-4)
    ini = torch.cat([w + 0.02, T + 0.1], 1)                      # the reference reads ini_pose as (axis-angle, T)
    est2 = GS().pnp(x.float(), X.float(), K, ini_pose=ini)
    np.testing.assert_allclose(est2.numpy(), est.numpy(), atol=2e-3)
    noisy = GS().pnp((x + 0.3 * torch.randn_like(x)).float(), X.float(), K)
    assert float((noisy - est).abs().max()) < 0.05
    # compute_pnp_loss: zero when the pose vector equals the solved (T, axis-angle)
    class M(GS):
        beta = 1
    Ki = torch.inverse(K).unsqueeze(0).repeat(b, 1, 1)
    x1 = torch.stack([480 * X[:, :, 0] / X[:, :, 2] + 416, 490 * X[:, :, 1] / X[:, :, 2] + 128], 1).float()
    matches = torch.cat([x1, x.float().transpose(1, 2)], 1)
    loss = M().compute_pnp_loss(X[:, :, 2].float().unsqueeze(1), matches, est, K.unsqueeze(0).repeat(b, 1, 1), Ki)
    assert loss.shape == (b, 3) and float(loss.max()) < 5e-3


def test_miopen_tuned_databases_are_activated_before_the_first_convolution(tmp_path):
    """miopen_tuning.activate(): the shipped user databases (text files keyed by architecture / CU count / MIOpen build) are
    copied to a per-user directory and MIOPEN_USER_DB_PATH points there -- unless the caller chose a path or switched it
    off.  Run in fresh interpreters: the decision is taken once per process, at the import of convs."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import os; from unsupervised_depth_opticalflow_egomotion_amd import convs, miopen_tuning as m; "
            "p = os.environ.get('MIOPEN_USER_DB_PATH'); print(m.status(), p, sorted(os.listdir(p)) if p and os.path.isdir(p) else None)")

    def run(extra):
        env = {k: v for k, v in os.environ.items() if k not in ("MIOPEN_USER_DB_PATH", "DFE_MIOPEN_DB")}
        env.update(extra, PYTHONPATH=root, TMPDIR=str(tmp_path))
        return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, cwd=root, timeout=300).stdout.strip()

    shipped = sorted(f for f in os.listdir(os.path.join(root, "unsupervised_depth_opticalflow_egomotion_amd", "miopen_db")) if f.endswith(".txt"))
    assert len(shipped) == 2 and all(f.startswith("gfx950") for f in shipped)
    out = run({})
    # no GPU in this process: the running MIOpen's key cannot be read, and status() says so instead of claiming "tuned"
    assert out.startswith("tuned-unverified " + str(tmp_path)) and all(f in out for f in shipped), out
    assert run({"DFE_MIOPEN_DB": "0"}).startswith("default None")
    mine = tmp_path / "mine"; mine.mkdir()
    assert run({"MIOPEN_USER_DB_PATH": str(mine)}).startswith("env " + str(mine))


def test_miopen_db_status_reports_tuned_only_for_a_matching_key(monkeypatch, tmp_path):
    """status() says 'tuned' only when a shipped file is keyed '<arch><CUs hex>.HIP.<version tag>' of the MIOpen that runs;
    a directory name alone ('dfe_miopen_db_*') is not a measurement."""
    from unsupervised_depth_opticalflow_egomotion_amd import miopen_tuning as m
    keys = m.shipped_keys()
    assert len(keys) == 1 and next(iter(keys)).startswith("gfx950100.HIP.")
    monkeypatch.setitem(m._state, "path", str(tmp_path / "dfe_miopen_db_0_abc"))
    monkeypatch.setattr(m, "running_key", lambda: next(iter(keys)))
    assert m.status() == "tuned"
    monkeypatch.setattr(m, "running_key", lambda: "gfx950100.HIP.9_9_9_20990101-1-1-gdeadbeef")
    assert m.status() == "tuned-unmatched"
    monkeypatch.setattr(m, "running_key", lambda: "gfx94298.HIP." + next(iter(keys)).split(".HIP.")[1])
    assert m.status() == "tuned-unmatched"
    monkeypatch.setattr(m, "running_key", lambda: None)
    assert m.status() == "tuned-unverified"
    monkeypatch.setitem(m._state, "path", str(tmp_path / "mine"))
    assert m.status() == "env"


def test_winograd_dispatch_rule_is_shape_logic_only(monkeypatch):
    """convs.plan's forward field (which 3x3 layers take dfe_wino_conv3x3) is pure shape logic: CPU tensors never qualify, and on
    a fake device tensor the thresholds, the paddings and the dilation rule decide."""
    from unsupervised_depth_opticalflow_egomotion_amd import convs

    class FakeCuda:
        is_cuda, dtype = True, torch.float32

        def __init__(self, *shape):
            self.shape = shape

        def dim(self):
            return len(self.shape)

        def numel(self):
            n = 1
            for s in self.shape:
                n *= s
            return n

    def el(x, w_shape, cin, stride, padding, dilation, groups=1):      # (the plan reads the channel count off the filter's shape)
        return convs.plan(x, w_shape, stride, padding, dilation, groups).fwd == "wino"
    assert not el(torch.zeros(8, 64, 64, 208), (64, 64, 3, 3), 64, (1, 1), (1, 1), (1, 1))          # CPU tensor
    x = FakeCuda(8, 128, 64, 208)
    assert el(x, (128, 128, 3, 3), 128, (1, 1), (1, 1), (1, 1)) and el(x, (96, 128, 3, 3), 128, (1, 1), (0, 0), (1, 1))
    assert not el(x, (128, 128, 3, 3), 128, (2, 2), (1, 1), (1, 1))                                   # stride 2
    assert not el(x, (128, 128, 5, 5), 128, (1, 1), (2, 2), (1, 1))                                   # 5x5
    assert not el(x, (128, 128, 3, 3), 128, (1, 1), (2, 2), (1, 1))                                   # padding 2 without dilation
    assert el(x, (128, 128, 3, 3), 128, (1, 1), (4, 4), (4, 4)) and el(x, (128, 128, 3, 3), 128, (1, 1), (16, 16), (16, 16))
    assert not el(x, (128, 128, 3, 3), 128, (1, 1), (3, 3), (3, 3))                                   # 64 is no multiple of 3
    assert not el(x, (128, 128, 3, 3), 128, (1, 1), (1, 1), (1, 1), groups=2)
    assert not el(FakeCuda(8, 8, 64, 208), (16, 8, 3, 3), 8, (1, 1), (1, 1), (1, 1))                  # too few reduction channels
    assert el(FakeCuda(12, 16, 256, 832), (16, 16, 3, 3), 16, (1, 1), (1, 1), (1, 1))                 # the decoder's 16 -> 16 layers qualify
    assert not el(FakeCuda(8, 128, 4, 13), (128, 128, 3, 3), 128, (1, 1), (1, 1), (1, 1))             # 8 * 2 * 7 tiles: the small-plane kernels' job
    assert not el(FakeCuda(64, 512, 128, 416), (64, 512, 3, 3), 512, (1, 1), (1, 1), (1, 1))          # > 2^30 elements: 32-bit offsets
    monkeypatch.setattr(convs, "WINO_MIN_TILES", 0)
    assert not el(x, (128, 128, 3, 3), 128, (1, 1), (1, 1), (1, 1))                                   # switched off


def test_conv_routes_match_the_recorded_table(monkeypatch):
    """convs.plan against tests/golden/conv_routes.json: the forward / data-gradient / weight-gradient kernel of every convolution
    the three models issue in one training step at 256x832, 3 scales (modes geom, depth, flow at per-GPU batches 1, 4, 8), as the
    call sites of the commit named in the fixture chose them -- under the default switches and with each switch flipped alone.  A
    changed threshold or a reordered rule moves layers between MIOpen and this build's kernels without failing any value test;
    it fails here.  No entry is left out."""
    import json
    from unsupervised_depth_opticalflow_egomotion_amd import convs
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_routes.json")) as fh:
        doc = json.load(fh)
    entries, default = doc["entries"], doc["routes"]["default"]
    assert len(default) == len(entries) and sorted(set(i for ids in doc["modes"].values() for i in ids)) == list(range(len(entries)))
    assert sorted(doc["modes"]) == sorted("%s/%d" % (m, b) for m in ("geom", "depth", "flow") for b in (1, 4, 8))

    def route(e):
        kw = {"plane": route(entries[e["first"]]).fwd == "plane"} if "first" in e else {}     # a dense block decides once
        return convs.plan((True, torch.float32, tuple(e["x"])), e["w"], e["stride"], e["padding"], e["dilation"], e["groups"], e["bias"],
                          e["act"], e["ctx"], tuple(e.get("fuse", ())), **kw)
    assert set(doc["routes"]) == {"default", "WINO_MIN_TILES=0", "WINO_DILATED=0", "WINO_WGRAD=0", "SCONV=0", "PLANECONV_MAX_HW=0",
                                  "WINO_EPILOGUE=0", "FLOW_HEAD=0", "PHASE_MIN_DILATION=2"}
    checked = 0
    for setting, diff in doc["routes"].items():
        want = list(default)
        with monkeypatch.context() as mp:
            if setting != "default":
                for i, v in diff.items():
                    want[int(i)] = v
                name, value = setting.split("=")
                mp.setattr(convs, name, type(getattr(convs, name))(int(value)))
            got = ["/".join(route(e)) for e in entries]
        wrong = [(setting, i, entries[i], got[i], want[i]) for i in range(len(entries)) if got[i] != want[i]]
        assert not wrong, wrong[:5]
        checked += len(got)
    assert checked == 9 * len(entries)
    # the table is not trivially MIOpen: under the default switches every kernel of this build has a layer -- except the
    # phase-image path, which the default DFE_WINO_DILATED=1 leaves empty at these shapes (the Winograd kernel takes all four
    # dilated layers first); it is seen with that switch off
    fwd, dgrad, wgrad = (set(r.split("/")[k] for r in default) for k in range(3))
    assert {"miopen", "wino", "wino_act", "plane", "conv1x1", "flow_head"} <= fwd and "wino" in dgrad
    assert {"wino_wgrad", "sconv_wgrad", "wgrad3x3"} <= wgrad
    assert "phase" not in fwd and any(v.startswith("phase/") for v in doc["routes"]["WINO_DILATED=0"].values())
    # host tensors never reach the library or a kernel of this build, whatever the door
    for ctx in ("conv2d", "module", "conv_act", "raw", "dense", "dense_head", "prepadded"):
        assert convs.plan(torch.zeros(1, 16, 8, 8), (16, 16, 3, 3), 1, 1, bias=True, act=True, ctx=ctx, fuse=("plane", "wino_act", "conv1x1")) == convs.MIOPEN


def test_ops_is_the_leaf_and_nothing_imports_it_inside_a_function():
    """ops.py knows nothing of convs; no module of the package imports ops or convs inside a function (the package's own lazy
    ``set_align_corners`` attribute aside, which must not pull torch in when the package is imported)."""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unsupervised_depth_opticalflow_egomotion_amd")
    with open(os.path.join(root, "ops.py")) as fh:
        assert "convs" not in fh.read()
    late = []
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py") and (d, f) != (root, "__init__.py"):
                with open(os.path.join(d, f)) as fh:
                    late += [(f, line.strip()) for line in fh if re.match(r"\s+(from \.+ import .*\b(ops|convs)\b|from \.+(ops|convs) import)", line)]
    assert not late, late


def test_wino_weight_cache_host_logic_without_a_gpu():
    """ops.WinoWeightCache never holds host tensors (there is no CPU path to cache for) and refresh() with nothing registered
    is a no-op that does not touch the device; DFE_WINO_CACHE=0 turns lookups off."""
    import torch
    from unsupervised_depth_opticalflow_egomotion_amd import ops

    cache = ops.WinoWeightCache()
    w = torch.nn.Parameter(torch.randn(8, 8, 3, 3))
    assert cache.lookup(w, False) is None and cache.lookup(w, True) is None and not cache.entries
    cache.refresh()
    cache.invalidate()
    assert cache.table is None and cache.hits == 0
    cache.enabled = False
    assert cache.lookup(w, False) is None and cache.misses == 0


@pytest.mark.parametrize("ac", [False, True])
def test_legacy_inverse_warp_signatures_vs_reference_golden(golden_dir, ac):
    """VERDICT r05 "missing" 3: the legacy signatures of inverse_warp.py (:30-107,148-224,305-352) -- tensor expressions, so
    they run on the host here -- against golden G12 (the reference's own functions).  The Euler rotation itself is the HIP
    operator: its matrices come from the golden here, the GPU test covers ``inverse_warp(rotation_mode='euler')``."""
    from tests.golden import make_golden as MG
    from unsupervised_depth_opticalflow_egomotion_amd.structures import inverse_warp as iw
    g = np.load(os.path.join(golden_dir, "G12_ac%d.npz" % ac))
    c = MG.g12_inputs()
    T = lambda a, grad=False: torch.from_numpy(np.ascontiguousarray(a)).float().requires_grad_(grad)   # noqa: E731
    K, pose = T(c["K"]), T(c["pose"])
    np.testing.assert_allclose(iw.quat2mat(pose[:, 3:]).numpy(), g["quat2mat"], rtol=0, atol=1e-7)
    pm = iw.pose_vec2mat(pose, "quat")
    np.testing.assert_allclose(pm.numpy(), g["pose_mat_quat"], rtol=0, atol=1e-7)
    with pytest.raises(ValueError):
        iw.pose_vec2mat(pose, "axis-angle")
    cam = iw.pixel2cam(T(c["depth"]), K.inverse())
    assert np.array_equal(cam.numpy(), g["pixel2cam"])
    proj = K @ pm
    cam_g = T(g["pixel2cam"])
    # the three projections on the quaternion matrices reproduce the reference's expressions bit for bit when fed its inputs
    ref_proj = K @ T(g["pose_mat_quat"])
    for name, fn in (("cam2pixel", iw.cam2pixel), ("cam2pixel_change_shape", iw.cam2pixel_change_shape)):
        mine = fn(cam_g, ref_proj[:, :, :3], ref_proj[:, :, -1:])
        assert mine.shape == g[name].shape
    assert np.array_equal(iw.skewsymmetric(pose[:, :3]).numpy(), g["skew"])
    assert np.array_equal(iw.meshgrid(5, 7).numpy(), g["meshgrid"])
    d, p = T(c["depth"], True), T(c["pose"], True)
    y, valid = iw.inverse_warp(T(c["img"]), d, p, K, rotation_mode="quat", align_corners=ac)
    (y * T(c["wgt"])).sum().backward()
    np.testing.assert_allclose(y.detach().numpy(), g["iw_quat_img"], rtol=0, atol=2e-6)
    assert np.array_equal(np.packbits(valid.numpy().astype(np.uint8).reshape(-1)), g["iw_quat_valid"])
    np.testing.assert_allclose(d.grad.numpy(), g["iw_quat_gdepth"], rtol=1e-4, atol=1e-4 * np.abs(g["iw_quat_gdepth"]).max())
    np.testing.assert_allclose(p.grad.numpy(), g["iw_quat_gpose"], rtol=1e-4, atol=1e-4 * np.abs(g["iw_quat_gpose"]).max())
    # cam2pixel / cam2pixel2 / change_shape on the golden's own Euler projection (K @ [R|t] recovered from G12's grid is not
    # stored; the Euler matrix comes from the oracle's restatement, itself pinned by G2)
    from oracle import loss_stack_oracle as O
    proj_e = K @ O.pose_vec2mat(pose)
    np.testing.assert_allclose(iw.cam2pixel(cam, proj_e[:, :, :3], proj_e[:, :, -1:]).numpy(), g["cam2pixel"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(iw.cam2pixel_change_shape(cam, proj_e[:, :, :3], proj_e[:, :, -1:]).numpy(),
                               g["cam2pixel_change_shape"], rtol=0, atol=1e-4)
    g2, z2 = iw.cam2pixel2(cam, proj_e[:, :, :3], proj_e[:, :, -1:], "zeros")
    np.testing.assert_allclose(g2.numpy(), g["cam2pixel2_grid"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(z2.numpy(), g["cam2pixel2_z"], rtol=0, atol=2e-6)
    assert np.array_equal(g2.numpy() == 2.0, g["cam2pixel2_grid"] == 2.0)


def test_occupancy_critical_kernels_keep_their_resources():
    """Round 6 lost 3 ms of step time to FOUR BYTES of static LDS in k_wino_fwd16 (two blocks per CU -> one: +45 % on every
    Winograd layer; EXPERIMENT_LOG round-6 appendix) -- nothing a parity test can see.  This reads the resource metadata of the
    built library (tools/kernel_meta.py: the code objects' AMDGPU notes, no GPU needed) and holds the matrix kernels to what
    their launch configuration assumes: no static LDS beside the dynamic buffers, at most 256 registers (two waves per SIMD),
    no register spills to memory, no scratch; the per-sample prepare kernels are the only ones allowed scratch.

    The last loop holds the deterministic mode's kernels to the same (no spills, no scratch, vgpr <= 256, agpr == 0): the twelve
    k_sconv_fwd / k_sconv_dgrad kernels sit at 250 / 243 VGPRs at the most, and the two 1x1 stride-2 kernels carry
    amdgpu_waves_per_eu(2) so that their MFMA accumulators stay out of the AGPRs (53 and 86 VGPRs; 76 + 24 and 104 + 20 without)."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels()
    assert len(ks) > 150
    by = lambda sub: [k for k in ks if sub in k["name"]]      # noqa: E731
    wino, wgrad = by("k_wino_fwd16"), by("k_wino_wgrad2")
    assert len(wino) == 8 and len(wgrad) >= 8
    for k in wino + wgrad + by("k_sconv_wgrad") + by("11k_planeconvI"):
        assert k["lds"] == 0, (k["name"], "static LDS in a kernel whose occupancy is sized by its dynamic LDS")
        assert k["vgpr"] + k["agpr"] <= 512 // 2 or "planeconv" in k["name"] or "sconv" in k["name"], k
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0, k
    for k in wino + wgrad:
        assert k["vgpr"] <= 256 and k["agpr"] == 0, k
    allowed_scratch = ("k_prepare_cameras", "k_pose_mats_bwd", "k_geom_prepare")
    for k in ks:
        if k["scratch"] > 0 or k["vgpr_spill"] > 0:
            assert any(a in k["name"] for a in allowed_scratch), k
    # the pointwise kernels of the loss stack: at least five waves per SIMD
    for k in by("k_geom_point_fwdILb0E") + by("k_geom_point_bwdILb0E"):
        assert k["vgpr"] <= 96, k
    # the rolling SSIM backward: 4 736 waves at the headline shape; at 97+ registers the chip holds 4 096 and the launch runs a
    # second, 16 %-full round (51 us instead of 39: profiles/r06_ssim_bwd_experiment.md)
    ssim_bwd = by("k_geom_ssim_bwd_roll")
    assert len(ssim_bwd) == 1 and ssim_bwd[0]["vgpr"] <= 96 and ssim_bwd[0]["scratch"] == 0, ssim_bwd
    # the deterministic mode's passes on the shared staging layer (csrc/dfe_mfma_stage.h): k_sconv_fwd / _dgrad sit at the
    # 256-register limit of two waves per SIMD
    det = by("k_sconv_fwd") + by("k_sconv_dgrad") + by("k_conv1x1s2_fwd") + by("k_conv1x1s2_wgrad")
    assert len(det) == 6 + 6 + 1 + 1
    for k in det:
        assert k["vgpr_spill"] == 0 and k["scratch"] == 0, k
        assert k["vgpr"] <= 256 and k["agpr"] == 0, k


def test_conv_planners_answer_as_recorded():
    """The host-only planners of csrc/ops_sconv.hip, ops_wino_wgrad.hip and ops_conv1x1s2.hip -- workspace floats and support
    per shape -- against tests/golden/conv_ws_floats.json, exactly: the shape lists of the kernels' GPU tests and of
    tools/sconv_bench.py and shapes some or all planners refuse.  The file holds the answers of the library built from the commit
    before the planners moved onto shared helpers (split_round, sc_tile_plan), never this tree's:
        DFE_HIP_LIB=<that build>/libdfe_hip.so python tools/conv_ws_floats.py > tests/golden/conv_ws_floats.json"""
    import json
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import conv_ws_floats
    from unsupervised_depth_opticalflow_egomotion_amd._lib import get_lib
    with open(os.path.join(REPO, "tests", "golden", "conv_ws_floats.json")) as fh:
        rows = json.load(fh)
    assert len(rows) >= 90
    # the recorded shapes are still the lists' shapes, and the refused ones answer 0 wherever they did
    assert [tuple(r["shape"]) for r in rows] == list(dict.fromkeys(s for _, s in conv_ws_floats.shapes()))
    assert sum(1 for r in rows for k, v in r.items() if k not in ("from", "shape") and v == 0) >= 100
    lib = get_lib()
    for r in rows:
        got = conv_ws_floats.answers(lib, tuple(r["shape"]))
        assert got == {k: r[k] for k in got}, (r["from"], r["shape"], got)


def test_bench_dump_outputs_float32_whole_or_a_fixed_sample(tmp_path):
    """bench.dump_outputs (bench.py --dump-outputs): every output as <name>.npy in float32; when they do not fit in the limit
    together, the small ones stay whole and the largest are cut to one common number of elements, the same seeded sample on
    every call, in index order."""
    import bench
    r = np.random.default_rng(0)
    outs = {"loss": torch.tensor(1.5, dtype=torch.float64), "mask": r.integers(0, 2, (64, 80)).astype(np.uint8),
            "big": torch.from_numpy(r.standard_normal(300_000)), "bigger": r.standard_normal((2, 400_000))}
    bench.dump_outputs(outs, str(tmp_path / "whole"))
    for k, v in outs.items():
        got = np.load(str(tmp_path / "whole" / (k + ".npy")))
        assert got.dtype == np.float32 and got.shape == tuple(np.shape(v))
        np.testing.assert_array_equal(got, np.asarray(v, dtype=np.float32))
    limit = 1_000_000
    for sub in ("a", "b"):
        bench.dump_outputs(outs, str(tmp_path / sub), limit=limit)
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == sorted(k + ".npy" for k in outs)
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= limit
    for f in files:
        np.testing.assert_array_equal(np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f)))
    assert np.load(str(tmp_path / "a" / "mask.npy")).shape == (64, 80)
    big, bigger = np.load(str(tmp_path / "a" / "big.npy")), np.load(str(tmp_path / "a" / "bigger.npy"))
    assert big.ndim == 1 and big.shape == bigger.shape and 100_000 < big.size < 300_000
    src = np.asarray(outs["big"], dtype=np.float32)
    pos = np.array([np.flatnonzero(src == x)[0] for x in big[:200]])
    assert (np.diff(pos) > 0).all()


def test_hw_queue_limit_is_raised_only_when_it_can_take_effect(monkeypatch):
    """The package raises GPU_MAX_HW_QUEUES to 8 at import (three network streams + a process group's streams need more than the
    runtime's 4 queues); a value the user exported wins, and models._side_streams only drops the high stream priorities under a
    process group when >= 8 queues are in effect."""
    import unsupervised_depth_opticalflow_egomotion_amd as pkg
    monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
    assert not pkg._kfd_is_open()                                                       # no GPU here: the runtime never starts
    assert pkg._hw_queue_limit() == 8 and os.environ["GPU_MAX_HW_QUEUES"] == "8"
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "4")
    assert pkg._hw_queue_limit() == 4 and os.environ["GPU_MAX_HW_QUEUES"] == "4"
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "16")
    assert pkg._hw_queue_limit() == 16
    # the runtime already started: only the environment the process was started with counts, and nothing is written
    monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
    monkeypatch.setattr(pkg, "_initial_env", lambda name: None)
    assert pkg._hw_queue_limit(started=True) == 4 and "GPU_MAX_HW_QUEUES" not in os.environ
    monkeypatch.setenv("GPU_MAX_HW_QUEUES", "8")                                        # set too late by the script itself
    assert pkg._hw_queue_limit(started=True) == 4
    monkeypatch.setattr(pkg, "_initial_env", lambda name: "8")                          # exported in the shell
    assert pkg._hw_queue_limit(started=True) == 8
    monkeypatch.undo()
    assert pkg._initial_env("PATH") == os.environ["PATH"] and pkg._initial_env("DFE_NO_SUCH_VARIABLE") is None
    monkeypatch.setattr(torch.cuda, "is_initialized", lambda: True)
    monkeypatch.setattr(pkg, "_initial_env", lambda name: None)
    assert pkg._hw_queue_limit() == 4

    from unsupervised_depth_opticalflow_egomotion_amd import models
    made = []
    monkeypatch.setattr(torch.cuda, "Stream", lambda dev, priority=0: made.append(priority) or ("stream", priority))
    monkeypatch.delenv("DFE_STREAM_PRIORITIES", raising=False)
    for pg, queues, want in ((False, 4, (0, 0)), (True, 4, (-1, -1)), (True, 8, (0, 0)), (False, 8, (0, 0))):
        monkeypatch.setattr(models, "_SIDE_STREAMS", {})
        monkeypatch.setattr(pkg, "HW_QUEUES", queues)
        monkeypatch.setattr(torch.distributed, "is_initialized", lambda pg=pg: pg)
        got = models._side_streams(torch.device("cuda", 0))
        assert (got[0][1], got[1][1]) == want, (pg, queues, got)
    monkeypatch.setenv("DFE_STREAM_PRIORITIES", "-1,0")
    monkeypatch.setattr(models, "_SIDE_STREAMS", {})
    got = models._side_streams(torch.device("cuda", 0))
    assert (got[0][1], got[1][1]) == (-1, 0)


def test_fused_adam_keeps_its_own_capturable_across_load_state_dict():
    """The optimiser's checkpoint contract: eager, --graph and torch.optim.Adam checkpoints are interchangeable and
    the mode comes from the constructor, never from the checkpoint.  torch's load_state_dict overwrites every group key with
    the checkpoint's, ``capturable`` included, and moves ``step`` to the parameter's device when the checkpoint says capturable;
    FusedAdam keeps its own flag, still takes lr / betas / eps from the checkpoint, and keeps every count a float32 host scalar.
    Construction, loading and saving need no GPU (only step() does)."""
    import copy
    from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
    torch.manual_seed(0)
    shapes = [(5,), (3, 4), (1,)]
    src = [torch.randn(s, requires_grad=True) for s in shapes]
    ref = torch.optim.Adam([dict(params=src[:2]), dict(params=src[2:], lr=3e-4, betas=(0.8, 0.99), eps=1e-6)], lr=2e-3)
    for _ in range(3):
        for p in src:
            p.grad = torch.randn_like(p)
        ref.step()
    plain = ref.state_dict()
    assert all(g["capturable"] is False for g in plain["param_groups"])
    flagged = copy.deepcopy(plain)
    for g in flagged["param_groups"]:
        g["capturable"] = True
    for ckpt, mine in ((plain, True), (flagged, False), (plain, False), (flagged, True)):
        ps = [torch.zeros(s, requires_grad=True) for s in shapes]
        opt = FusedAdam([dict(params=ps[:2]), dict(params=ps[2:])], lr=1.0, betas=(0.1, 0.2), eps=0.5, capturable=mine)
        opt.load_state_dict(copy.deepcopy(ckpt))
        assert [g["capturable"] for g in opt.param_groups] == [mine, mine]
        assert [(g["lr"], tuple(g["betas"]), g["eps"]) for g in opt.param_groups] == [(2e-3, (0.9, 0.999), 1e-8), (3e-4, (0.8, 0.99), 1e-6)]
        for p, q in zip(ps, src):
            st = opt.state[p]
            assert st["step"].device.type == "cpu" and st["step"].dtype == torch.float32 and st["step"].dim() == 0
            assert float(st["step"]) == 3.0
            assert torch.equal(st["exp_avg"], ref.state[q]["exp_avg"]) and torch.equal(st["exp_avg_sq"], ref.state[q]["exp_avg_sq"])
        out = opt.state_dict()
        assert [g["capturable"] for g in out["param_groups"]] == [mine, mine]
        assert all(float(out["state"][i]["step"]) == 3.0 for i in range(3))
        back = torch.optim.Adam([dict(params=ps[:2]), dict(params=ps[2:])], lr=1.0)       # and torch reads it back
        back.load_state_dict(out)
        assert all(torch.equal(back.state[p]["exp_avg"], ref.state[q]["exp_avg"]) for p, q in zip(ps, src))
