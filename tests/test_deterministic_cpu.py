"""CPU-only checks of the deterministic mode (convs.set_deterministic / DFE_DETERMINISTIC): the plan of every convolution a
training step issues (tests/golden/conv_routes.json) names no MIOpen pass, switching the mode off again restores the recorded
routes, a layer no kernel of this build takes is refused by ``plan`` itself, and the host-only planners of the mode's kernels
(dfe_sconv_fwd / _dgrad, dfe_conv1x1s2_fwd / _wgrad) accept and refuse what their launchers document -- every refusal before a
launch, so none of this needs a device."""
import ctypes
import json
import os

import pytest
import torch

from unsupervised_depth_opticalflow_egomotion_amd import _lib, convs

HERE = os.path.dirname(os.path.abspath(__file__))


def _table():
    with open(os.path.join(HERE, "golden", "conv_routes.json")) as fh:
        return json.load(fh)


def _routes(entries):
    def route(e):      # the call test_conv_routes_match_the_recorded_table rebuilds
        kw = {"plane": route(entries[e["first"]]).fwd == "plane"} if "first" in e else {}
        return convs.plan((True, torch.float32, tuple(e["x"])), e["w"], e["stride"], e["padding"], e["dilation"], e["groups"], e["bias"],
                          e["act"], e["ctx"], tuple(e.get("fuse", ())), **kw)
    return [route(e) for e in entries]


@pytest.fixture
def mode():
    """the mode switched on for one test and restored afterwards, whatever the test did"""
    before = convs.DETERMINISTIC
    convs.set_deterministic(True)
    yield
    convs.set_deterministic(before)


def test_no_recorded_layer_is_planned_on_miopen(mode):
    doc = _table()
    entries = doc["entries"]
    plans = _routes(entries)
    assert len(plans) == len(entries) >= 255
    image = lambda e: e["x"][1] in (3, 9) and tuple(e["x"][2:]) == (256, 832)      # noqa: E731  (no gradient is ever asked for the image)
    for e, p in zip(entries, plans):
        assert p.fwd != "miopen" and p.wgrad != "miopen", (e, p)
        assert p.dgrad != "miopen" or image(e), (e, p)
        if p.dgrad == "none":            # the one pass without a kernel: the 7x7 stems' data gradient
            assert image(e) and e["w"][2] == 7, (e, p)
    # every family of the mode has a layer, and the layers that were this build's already stay where they are
    fwd, dgrad, wgrad = (set(getattr(p, k) for p in plans) for k in ("fwd", "dgrad", "wgrad"))
    assert {"sconv", "conv1x1s2", "wino", "wino_act", "plane", "conv1x1", "flow_head"} <= fwd
    assert {"sconv", "wino", "none"} <= dgrad and {"sconv_wgrad", "conv1x1s2", "wino_wgrad", "wgrad3x3"} <= wgrad
    for e, p, was in zip(entries, plans, doc["routes"]["default"]):
        was_fwd, _, was_wgrad = was.split("/")
        assert "/".join(p) == was or was_fwd not in ("plane", "conv1x1", "flow_head"), (e, p, was)
        assert p.wgrad == "wgrad3x3" or was_wgrad != "wgrad3x3", (e, p, was)
    # the stride-2 layers: all three passes, whatever the input width (SCONV_WGRAD_MAX_CI does not limit), the 1x1 shortcuts included
    for e, p in zip(entries, plans):
        if e["stride"] in (2, [2, 2]):
            k = e["w"][2]
            assert p.fwd in (("conv1x1s2",) if k == 1 else ("sconv", "sconv_act")), (e, p)
            assert p.wgrad == ("conv1x1s2" if k == 1 else "sconv_wgrad") and p.dgrad == ("none" if k == 7 else "sconv"), (e, p)
        if e["dilation"] in (8, 16, [8, 8], [16, 16]):          # their weight gradients run on the phase images
            assert p.wgrad == "wino_wgrad", (e, p)


def test_the_fused_strided_epilogue_is_planned_where_the_caller_admits_it(mode):
    x = (True, torch.float32, (4, 16, 128, 416))
    assert convs.plan(x, (32, 16, 5, 5), 2, 2, bias=True, act=True, ctx="conv_act", fuse=("plane", "conv1x1", "sconv_act")).fwd == "sconv_act"
    assert convs.plan(x, (32, 16, 5, 5), 2, 2, bias=True, act=True, ctx="conv_act", fuse=("plane", "conv1x1")).fwd == "sconv"
    assert convs.plan(x, (32, 16, 5, 5), 2, 2, bias=False, act=True, ctx="conv_act", fuse=("sconv_act",)).fwd == "sconv"
    convs.set_deterministic(False)
    assert convs.plan(x, (32, 16, 5, 5), 2, 2, bias=True, act=True, ctx="conv_act", fuse=("plane", "conv1x1", "sconv_act")).fwd == "miopen"


def test_switching_the_mode_off_restores_the_recorded_routes():
    doc = _table()
    entries, default = doc["entries"], doc["routes"]["default"]
    before = convs.DETERMINISTIC
    try:
        convs.set_deterministic(False)
        assert ["/".join(p) for p in _routes(entries)] == default
        convs.set_deterministic(True)
        assert ["/".join(p) for p in _routes(entries)] != default
        convs.set_deterministic(False)
        got = ["/".join(p) for p in _routes(entries)]           # a memo key without the mode would hand back the mode's plans
        assert got == default, [(i, g, d) for i, (g, d) in enumerate(zip(got, default)) if g != d][:5]
    finally:
        convs.set_deterministic(before)


def test_the_environment_variable_sets_the_mode():
    import subprocess
    import sys
    code = "from unsupervised_depth_opticalflow_egomotion_amd import convs; print(int(convs.DETERMINISTIC))"
    for value, want in (("1", "1"), ("0", "0"), (None, "0")):
        env = {k: v for k, v in os.environ.items() if k != "DFE_DETERMINISTIC"}
        if value is not None:
            env["DFE_DETERMINISTIC"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(HERE), env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip().splitlines()[-1] == want, (value, out.stdout, out.stderr)


def test_unsupported_layers_are_refused_by_plan(mode):
    x32 = (True, torch.float32, (2, 16, 32, 32))
    with pytest.raises(_lib.DfeError, match=r"groups 2"):
        convs.plan(x32, (16, 8, 3, 3), 1, 1, 1, 2)
    with pytest.raises(_lib.DfeError, match=r"not fp32"):
        convs.plan((True, torch.float64, (2, 16, 32, 32)), (16, 16, 3, 3), 1, 1)
    for ctx in ("conv2d", "module", "raw", "prepadded", "conv_act", "dense"):
        with pytest.raises(_lib.DfeError, match=r"\(2, 16, 32, 32\).*\(16, 16, 5, 5\)"):          # 5x5 stride 1: outside every family; the layer is named
            convs.plan(x32, (16, 16, 5, 5), 1, 2, ctx=ctx)
    with pytest.raises(_lib.DfeError):
        convs.plan(x32, (16, 16, 3, 3), 2, 0)                   # stride 2 without the k // 2 padding
    with pytest.raises(_lib.DfeError):
        convs.plan(x32, (16, 16, 1, 1), 1, 0)                   # 1x1 stride 1 on a plane too large for the tiny-plane kernel
    with pytest.raises(_lib.DfeError):
        convs.plan((True, torch.float32, (2, 16, 30, 32)), (16, 16, 3, 3), 1, 4, 4)       # dilation 4 does not divide H
    # host tensors stay ATen's, as without the mode
    assert convs.plan(torch.zeros(1, 16, 8, 8), (16, 16, 5, 5), 1, 2) == convs.MIOPEN
    assert convs.plan(torch.zeros(1, 16, 8, 8, dtype=torch.float64), (16, 8, 3, 3), 1, 1, 1, 2) == convs.MIOPEN
    # without the mode the same layers are MIOpen's, silently
    convs.set_deterministic(False)
    assert convs.plan(x32, (16, 8, 3, 3), 1, 1, 1, 2) == convs.MIOPEN and convs.plan(x32, (16, 16, 5, 5), 1, 2) == convs.MIOPEN


def test_planners_accept_and_refuse_what_the_launchers_document():
    lib = _lib.get_lib()
    P, Q = ctypes.c_void_p(16), ctypes.c_void_p(20)
    L = ctypes.c_long
    # ---- dfe_sconv_fwd: K in {3, 5, 7}; a sample of x has at least 4 floats
    for (B, Ci, Co, H, W, K) in [(12, 3, 64, 256, 832, 7), (4, 9, 16, 256, 832, 7), (4, 16, 32, 128, 416, 5), (1, 256, 256, 4, 13, 3), (3, 128, 196, 8, 26, 3),
                                 (1, 3, 16, 3, 5, 3), (1, 1, 1, 2, 2, 3)]:
        assert lib.dfe_sconv_fwd_floats(B, Ci, Co, H, W, K) > 0, (B, Ci, Co, H, W, K)
    for (B, Ci, Co, H, W, K) in [(1, 16, 16, 8, 8, 1), (1, 16, 16, 8, 8, 2), (1, 16, 16, 8, 8, 9), (0, 16, 16, 8, 8, 3), (1, 3, 8, 1, 1, 3), (1, 1, 8, 1, 3, 3)]:
        assert lib.dfe_sconv_fwd_floats(B, Ci, Co, H, W, K) == 0, (B, Ci, Co, H, W, K)
    # thin layers split their input channels over blocks: the workspace then holds the partial outputs too
    packed = lambda Ci, Co, K: (Ci + 3) // 4 * 4 * K * K * ((Co + 63) // 64 * 64) + 64      # noqa: E731
    assert lib.dfe_sconv_fwd_floats(12, 3, 64, 256, 832, 7) == packed(3, 64, 7)
    assert lib.dfe_sconv_fwd_floats(1, 256, 256, 4, 13, 3) > packed(256, 256, 3) + 2 * 256 * 2 * 7
    fwd = lambda x, xbs, w, y, ybs, ws, *dims: lib.dfe_sconv_fwd(x, L(xbs), w, None, 1.0, y, L(ybs), ws, *dims, None)      # noqa: E731
    assert fwd(None, 4 * 64, P, P, 4 * 16, P, 1, 4, 4, 8, 8, 3) == -1 and fwd(P, 4 * 64, P, P, 4 * 16, None, 1, 4, 4, 8, 8, 3) == -1
    assert fwd(P, 4 * 64, P, P, 4 * 16, P, 1, 4, 4, 8, 8, 4) == -4 and fwd(P, 3, P, P, 8, P, 1, 3, 8, 1, 1, 3) == -4
    assert fwd(P, 4 * 64 - 1, P, P, 4 * 16, P, 1, 4, 4, 8, 8, 3) == -2 and fwd(P, 4 * 64, P, P, 4 * 16 - 1, P, 1, 4, 4, 8, 8, 3) == -2
    assert fwd(P, 4 * 64, P, P, 4 * 16, Q, 1, 4, 4, 8, 8, 3) == -4                      # the workspace 4 bytes off 16
    assert fwd(P, 4 * 64, P, P, 4 * 16, P, 0, 4, 4, 8, 8, 3) == -2
    # ---- dfe_sconv_dgrad: K in {1, 3, 5}; a sample of gy has at least 4 floats
    for (B, Ci, Co, H, W, K) in [(4, 16, 32, 128, 416, 5), (1, 256, 256, 4, 13, 3), (3, 128, 196, 8, 26, 3), (3, 64, 128, 64, 208, 1), (1, 3, 16, 3, 5, 3),
                                 (12, 3, 16, 256, 832, 3)]:
        assert lib.dfe_sconv_dgrad_floats(B, Ci, Co, H, W, K) > 0, (B, Ci, Co, H, W, K)
    for (B, Ci, Co, H, W, K) in [(1, 3, 64, 256, 832, 7), (1, 16, 16, 8, 8, 2), (1, 16, 16, 8, 8, 0), (1, 16, 16, 0, 8, 3), (2, 8, 3, 1, 1, 3), (1, 8, 1, 5, 1, 1)]:
        assert lib.dfe_sconv_dgrad_floats(B, Ci, Co, H, W, K) == 0, (B, Ci, Co, H, W, K)
    dg = lambda gy, gbs, w, gx, xbs, ws, *dims: lib.dfe_sconv_dgrad(gy, L(gbs), w, gx, L(xbs), ws, *dims, None)      # noqa: E731
    assert dg(None, 4 * 16, P, P, 4 * 64, P, 1, 4, 4, 8, 8, 3) == -1 and dg(P, 4 * 16, P, None, 4 * 64, P, 1, 4, 4, 8, 8, 3) == -1
    assert dg(P, 4 * 16, P, P, 4 * 64, P, 1, 4, 4, 8, 8, 7) == -4 and dg(P, 3, P, P, 8, P, 2, 8, 3, 1, 1, 3) == -4
    assert dg(P, 4 * 16 - 1, P, P, 4 * 64, P, 1, 4, 4, 8, 8, 3) == -2 and dg(P, 4 * 16, P, P, 4 * 64 - 1, P, 1, 4, 4, 8, 8, 3) == -2
    assert dg(P, 4 * 16, P, P, 4 * 64, Q, 1, 4, 4, 8, 8, 3) == -4
    # ---- dfe_conv1x1s2_*: any channel count and plane; only the 32-bit element numbers limit
    for (B, Ci, Co, H, W) in [(3, 64, 128, 64, 208), (24, 256, 512, 16, 52), (1, 1, 1, 1, 1), (3, 64, 128, 5, 7), (1, 7, 130, 6, 8)]:
        assert lib.dfe_conv1x1s2_supported(B, Ci, Co, H, W) == 1 and lib.dfe_conv1x1s2_wgrad_floats(B, Ci, Co, H, W) >= Co * Ci, (B, Ci, Co, H, W)
    for (B, Ci, Co, H, W) in [(0, 64, 128, 8, 8), (1, 0, 128, 8, 8), (1, 64, 128, 8, 0), (1, 4, 4, 1 << 15, 1 << 14), (1 << 12, 4, 4, 1 << 10, 1 << 10)]:
        assert lib.dfe_conv1x1s2_supported(B, Ci, Co, H, W) == 0 and lib.dfe_conv1x1s2_wgrad_floats(B, Ci, Co, H, W) == 0, (B, Ci, Co, H, W)
    # one resident round of blocks: 512 over the (64 x 64) output tiles, never more splits than 32-pixel chunks
    assert lib.dfe_conv1x1s2_wgrad_floats(3, 64, 128, 64, 208) == 156 * 128 * 64           # 9984 pixels = 312 chunks, 2 tiles: 256 splits wanted, 2 chunks each
    assert lib.dfe_conv1x1s2_wgrad_floats(24, 256, 512, 16, 52) == 16 * 512 * 256          # 32 tiles: 16 splits
    assert lib.dfe_conv1x1s2_wgrad_floats(1, 64, 128, 5, 7) == 128 * 64                    # 12 pixels: one chunk, one split
    f1 = lambda x, xbs, w, y, ybs, *dims: lib.dfe_conv1x1s2_fwd(x, L(xbs), w, y, L(ybs), *dims, None)      # noqa: E731
    assert f1(None, 4 * 64, P, P, 4 * 16, 1, 4, 4, 8, 8) == -1 and f1(P, 4 * 64, None, P, 4 * 16, 1, 4, 4, 8, 8) == -1 and f1(P, 4 * 64, P, None, 4 * 16, 1, 4, 4, 8, 8) == -1
    assert f1(P, 4 * 64 - 1, P, P, 4 * 16, 1, 4, 4, 8, 8) == -2 and f1(P, 4 * 64, P, P, 4 * 16 - 1, 1, 4, 4, 8, 8) == -2 and f1(P, 4 * 64, P, P, 4 * 16, 1, 4, 0, 8, 8) == -2
    assert f1(P, 1 << 40, P, P, 1 << 40, 1, 4, 4, 1 << 15, 1 << 14) == -4
    w1 = lambda x, xbs, gy, gbs, gw, ws, *dims: lib.dfe_conv1x1s2_wgrad(x, L(xbs), gy, L(gbs), gw, ws, *dims, None)      # noqa: E731
    assert w1(P, 4 * 64, None, 4 * 16, P, P, 1, 4, 4, 8, 8) == -1 and w1(P, 4 * 64, P, 4 * 16, P, None, 1, 4, 4, 8, 8) == -1
    assert w1(P, 4 * 64 - 1, P, 4 * 16, P, P, 1, 4, 4, 8, 8) == -2 and w1(P, 4 * 64, P, 4 * 16 - 1, P, P, 1, 4, 4, 8, 8) == -2
    assert w1(P, 1 << 40, P, 1 << 40, P, P, 1, 4, 4, 1 << 15, 1 << 14) == -4
    # the wrappers' queries agree with the library's
    from unsupervised_depth_opticalflow_egomotion_amd import ops
    assert ops.sconv_fwd_supported((4, 16, 128, 416), 32, 5) and not ops.sconv_fwd_supported((4, 16, 128, 416), 32, 1)
    assert ops.sconv_dgrad_supported((3, 64, 64, 208), 128, 1) and not ops.sconv_dgrad_supported((3, 3, 256, 832), 64, 7)
    assert ops.conv1x1s2_supported((3, 64, 64, 208), 128) and not ops.conv1x1s2_supported((0, 64, 64, 208), 128)
