"""The device-resident training set on the GPU: dfe_resize_strips_u8 (the store's bytes) and dfe_gather_triplets_u8 (a batch in
one launch) in guarded, sentinel-filled carves against the OpenCV restatement and the gather's formula in numpy;
prepared_data.ResidentTrainSet against prepared_data.PreparedFeeder bit for bit, from a build and from its cache; a replayed
graph fed through ``out=``; train.py --data_source resident.  Every comparison is equality: the path is integer arithmetic plus
a table lookup."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cv2_linear_u8 as CV
from tests import guarded as G
from tests import resident_tree as RT
from unsupervised_depth_opticalflow_egomotion_amd import _lib, convs, ops, prepared_data
from unsupervised_depth_opticalflow_egomotion_amd._lib import DfeError

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = RT.LUT
HW = (64, 208)


def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _lut():
    return torch.from_numpy(LUT).to(dev())


# ================================================================================================ the store's bytes
def _pack(strips, align=256):
    offs, pos = [], 0
    for s in strips:
        offs.append(pos)
        pos += (s.size + align - 1) // align * align
    buf = np.zeros(pos, np.uint8)
    for s, o in zip(strips, offs):
        buf[o:o + s.size] = s.reshape(-1)
    return buf, offs


@pytest.mark.parametrize("rgb", [0, 1])
@pytest.mark.parametrize("shape,hw", [((40, 60), (64, 128)),       # generic INTER_LINEAR
                                      ((32, 64), (16, 32)),        # exact 1/2: INTER_AREA
                                      ((16, 32), (16, 32))])       # same size: copy
def test_store_bytes_equal_the_restatement(shape, hw, rgb):
    h0, w0 = shape
    rng = np.random.default_rng(h0 * w0 + rgb)
    strips = [rng.integers(0, 256, (3 * h0, w0, 3), dtype=np.uint8) for _ in range(2)]
    buf, offs = _pack(strips)
    raw = torch.from_numpy(buf).to(dev())
    F = 8
    slot = np.array([[5, -1, 0], [2, 7, -1]], np.int64)            # two frames are 'stored already'; slots 1, 3, 4, 6 get nothing
    store = G.CarvedBytes((F, 3, hw[0], hw[1]))
    ops.resize_strips_u8(raw, [shape, shape], hw, slot, store.view, offs, rgb=bool(rgb))
    torch.cuda.synchronize()
    assert store.intact()
    got = store.cpu().numpy()
    for b in range(2):
        for f in range(3):
            frame = strips[b][f * h0:(f + 1) * h0]
            want = CV.resize_linear_u8(frame[:, :, ::-1] if rgb else frame, hw).transpose(2, 0, 1)      # B, G, R planes
            if slot[b, f] >= 0:
                assert np.array_equal(got[slot[b, f]], want), (b, f)
    for s in (1, 3, 4, 6):
        assert (got[s] == G.BYTE_SENTINEL).all(), s
    # the looked-up floats of the prepare kernel are the table at these bytes: one statement of the arithmetic
    full = G.CarvedBytes((6, 3, hw[0], hw[1]))
    ops.resize_strips_u8(raw, [shape, shape], hw, np.arange(6).reshape(2, 3), full.view, offs, rgb=bool(rgb))
    img = ops.prepare_triplets_u8(raw, [shape, shape], hw, None, offs, rgb=bool(rgb))
    torch.cuda.synchronize()
    assert full.intact()
    img, st = img.cpu().numpy(), full.cpu().numpy()
    for b in range(2):
        for f in range(3):
            assert np.array_equal(img[b, :, f * hw[0]:(f + 1) * hw[0]], LUT[st[3 * b + f]])
            if slot[b, f] >= 0:
                assert np.array_equal(st[3 * b + f], got[slot[b, f]])


def test_resize_refusals_come_before_the_library():
    raw = torch.zeros(9 * 4 * 4, dtype=torch.uint8, device=dev())
    store = G.CarvedBytes((2, 3, 4, 4))
    for bad in ([[0, 1, 2]], [[0, -2, 1]], [[0, 1]]):
        with pytest.raises(ValueError):
            ops.resize_strips_u8(raw, [(4, 4)], (4, 4), bad, store.view)
    with pytest.raises(ValueError):
        ops.resize_strips_u8(raw, [(4, 4)], (4, 4), [[0, 1, -1]], store.view, offsets=[1])
    with pytest.raises(DfeError):
        ops.resize_strips_u8(raw.cpu(), [(4, 4)], (4, 4), [[0, 1, -1]], store.view)
    with pytest.raises(ValueError):
        ops.resize_strips_u8(raw, [(4, 4)], (4, 4), [[0, 1, -1]], store.view.float())
    torch.cuda.synchronize()
    assert store.untouched() and store.intact()
    lib = _lib.get_lib()
    p = ctypes.c_void_p(raw.data_ptr())          # F <= 0: refused before the pointers are looked at
    assert lib.dfe_resize_strips_u8(p, p, p, p, p, ctypes.c_void_p(store.ptr), 0, 1, 4, 4, 0, 0, None) == -2
    torch.cuda.synchronize()
    assert store.untouched()


# ================================================================================================ the gather
F_, N_, S_ = 7, 5, 3
TRI = np.array([[0, 1, 2], [1, 2, 3], [2, 3, 4], [4, 5, 6], [6, 0, 3]], np.int32)       # triplets sharing frames
GATHER_HW = [(6, 16),     # one vector group per row: the flipped load address is 0
             (4, 48),     # three groups, the middle one mirrors onto itself
             (8, 32),
             (5, 19),     # element path, frames not 16-byte aligned
             (3, 1)]


def _batch(B):
    """(idx, flip) lists of B samples; for B >= 3 with a repeated index, indices 0 and N-1 and both flips"""
    if B == 1:
        return None
    idx = [(3 * j + (j // 5)) % N_ for j in range(B)]
    idx[0], idx[1], idx[2] = 0, N_ - 1, 0
    flip = [(j * 7 // 3) % 2 for j in range(B)]
    flip[0], flip[1] = 1, 0
    if B > 64:
        idx[64], flip[64] = 3, 1                  # the second launch's first sample
    return idx, flip


def _gather_case(H, W, idx, flip, store_off, out_off, seed):
    rng = np.random.default_rng(seed)
    store_np = rng.integers(0, 256, (F_, 3, H, W), dtype=np.uint8)
    ktab_np = rng.standard_normal((N_, 2, S_, 3, 3)).astype(np.float32)
    store = G.CarvedBytes((F_, 3, H, W), offset_bytes=store_off)
    store.view.copy_(torch.from_numpy(store_np))
    B = len(idx)
    out, K, Ki = G.Carved((B, 3, 3 * H, W), out_off), G.Carved((B, S_, 3, 3), out_off), G.Carved((B, S_, 3, 3))
    assert out.view.is_contiguous() and store.view.is_contiguous()
    res = ops.gather_triplets_u8((store.view, torch.from_numpy(TRI).to(dev()), torch.from_numpy(ktab_np).to(dev()), _lut()), idx, flip,
                                 out=[out.view, K.view, Ki.view])
    torch.cuda.synchronize()
    assert [t.data_ptr() for t in res] == [out.ptr, K.ptr, Ki.ptr]
    want = RT.gather_reference(store_np, TRI, ktab_np, idx, flip)
    tag = (H, W, B, store_off, out_off)
    assert out.intact() and K.intact() and Ki.intact() and store.intact(), tag
    assert np.array_equal(store.cpu().numpy(), store_np), tag
    for c, w in zip((out, K, Ki), want):
        assert G.bits_equal(c.cpu(), torch.from_numpy(w)), tag
    return out.cpu().numpy()


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("H,W", GATHER_HW)
def test_gather_in_guarded_carves(H, W, B):
    if B == 1:      # one sample cannot repeat an index: both ends of the table and both flips over two launches
        cases = [([0], [1]), ([N_ - 1], [0]), ([2], None)]
    else:
        idx, flip = _batch(B)
        assert len(idx) == len(flip) == B and len(set(idx)) < B and 0 in idx and N_ - 1 in idx and set(flip) == {0, 1}
        assert all(0 <= i < N_ for i in idx)
        cases = [(idx, flip)]
    seed = 1000 * H + 10 * W + B
    for idx, flip in cases:
        ref = _gather_case(H, W, idx, flip, 0, 0, seed)
        assert np.isin(ref, LUT).all()
        # out and store one to three elements off 16-byte alignment: the element path, the same bits
        for store_off, out_off in ((1, 0), (0, 1), (2, 2), (3, 3)):
            assert np.array_equal(_gather_case(H, W, idx, flip, store_off, out_off, seed), ref)


def test_gather_fresh_outputs_and_a_slot_outside_the_store():
    """Without ``out`` the three tensors are fresh; a slot >= F (or < 0) in tri is never dereferenced: its rows are lut[0]."""
    H, W = 4, 32
    rng = np.random.default_rng(3)
    store_np = rng.integers(1, 256, (F_, 3, H, W), dtype=np.uint8)          # no zero byte: lut[0] marks the refused frame
    tri = TRI.copy()
    tri[1] = [F_, -1, 2]
    store = G.CarvedBytes((F_, 3, H, W))
    store.view.copy_(torch.from_numpy(store_np))
    ktab = torch.zeros(N_, 2, S_, 3, 3, device=dev())
    tensors = (store.view, torch.from_numpy(tri).to(dev()), ktab, _lut())
    a = ops.gather_triplets_u8(tensors, [1, 0], [0, 1])
    b = ops.gather_triplets_u8(tensors, [1, 0], [0, 1])
    torch.cuda.synchronize()
    assert a[0].data_ptr() != b[0].data_ptr() and a[0].shape == (2, 3, 3 * H, W) and a[1].shape == a[2].shape == (2, S_, 3, 3)
    img = a[0].cpu().numpy()
    assert (img[0, :, :2 * H] == 0).all() and np.array_equal(img[0, :, 2 * H:], LUT[store_np[2]])
    assert np.array_equal(img[1, :, :H], LUT[store_np[0][:, :, ::-1]]) and store.intact()


def test_gather_refusals_come_before_any_launch():
    H, W = 4, 16
    store = torch.zeros(F_, 3, H, W, dtype=torch.uint8, device=dev())
    tri, ktab, lut = torch.from_numpy(TRI).to(dev()), torch.zeros(N_, 2, S_, 3, 3, device=dev()), _lut()
    out, K, Ki = G.Carved((2, 3, 3 * H, W)), G.Carved((2, S_, 3, 3)), G.Carved((2, S_, 3, 3))
    dst = [out.view, K.view, Ki.view]
    t = (store, tri, ktab, lut)
    for idx, flip in (([-1, 0], None), ([0, N_], None), ([0, 1], [1]), ([0, 1], [0, 1, 0]), ([], None)):
        with pytest.raises(ValueError):
            ops.gather_triplets_u8(t, idx, flip, out=dst)
    with pytest.raises(DfeError):
        ops.gather_triplets_u8((store.cpu(), tri, ktab, lut), [0, 1], out=dst)
    with pytest.raises(DfeError):
        ops.gather_triplets_u8(t, [0, 1], out=[out.view.cpu(), K.view, Ki.view])
    for bad in ((store.int(), tri, ktab, lut), (store, tri.long(), ktab, lut), (store, tri, ktab.double(), lut), (store, tri, ktab, lut[:100])):
        with pytest.raises(ValueError):
            ops.gather_triplets_u8(bad, [0, 1], out=dst)
    wide = G.Carved((2, 3, 3 * H, 2 * W))
    with pytest.raises(ValueError, match="contiguous"):
        ops.gather_triplets_u8(t, [0, 1], out=[wide.view[:, :, :, ::2], K.view, Ki.view])
    with pytest.raises(ValueError):
        ops.gather_triplets_u8(t, [0, 1], out=[out.view, K.view])
    with pytest.raises(ValueError):
        ops.gather_triplets_u8(t, [0, 1, 2], out=dst)                     # three samples into outputs of two
    # the library's own check is on the host too: a bad index returns DFE_ERR_DIMS and no kernel has run
    lib = _lib.get_lib()
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    for bad in ((0, N_), (-1, 0)):
        rc = lib.dfe_gather_triplets_u8(p(store), F_, p(tri), p(ktab), N_, p(lut), (ctypes.c_int * 2)(*bad), None, p(out.view), p(K.view),
                                        p(Ki.view), 2, S_, H, W, None)
        assert rc == -2
    torch.cuda.synchronize()
    assert out.untouched() and K.untouched() and Ki.untouched() and out.intact()


# ================================================================================================ the set against the feeder
@pytest.fixture(scope="module")
def shared(tmp_path_factory):
    """The shared-frame tree (10 strips, two raw sizes), its source, a set built from it (and written to a cache) and the six
    batches of B = 3 it yields, computed once."""
    root = str(tmp_path_factory.mktemp("resident") / "tree")
    os.makedirs(root)
    _, frames = RT.build_shared_tree(root, n=10, seed=3)
    cache = os.path.join(os.path.dirname(root), "cache")
    src = prepared_data.PreparedKITTI(root, 3, HW)
    rset = prepared_data.ResidentTrainSet(src, HW, dev(), num_workers=2, cache_dir=cache, reserve_mb=64)
    return dict(root=root, cache=cache, src=src, set=rset, frames=frames, batches=_collect(rset.batches(3, 6), 6))


def _collect(it, n):
    out = []
    for _ in range(n):
        img, k, ki = next(it)
        out.append((img.cpu().numpy(), k.cpu().numpy(), ki.cpu().numpy()))
    with pytest.raises(StopIteration):
        next(it)
    return out


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))


def test_set_store_and_tables(shared):
    s = shared["set"]
    want = np.stack([RT.stored_frame(fr, HW) for fl in shared["frames"] for fr in fl])
    assert s.F == 14 < 3 * s.N == 30 and not s.from_cache
    assert np.array_equal(s.tensors[0].cpu().numpy(), want)
    assert np.array_equal(s.tensors[1].cpu().numpy(), s.tri) and np.array_equal(s.tensors[3].cpu().numpy(), LUT)
    assert s.nbytes == prepared_data.resident_bytes(14, 10, 3, HW)


def test_set_equals_the_feeder_bit_for_bit(shared):
    src = shared["src"]
    flips = [src.sample(i)[1] for k in range(6) for i in prepared_data.batch_indices(k, 3)]
    assert set(flips) == {False, True}
    feeder = _collect(prepared_data.PreparedFeeder(src, 3, HW, dev(), 6, num_workers=0), 6)
    assert _same(shared["batches"], feeder)
    for j, idx in enumerate(prepared_data.batch_indices(0, 3)):
        i, flip = src.sample(idx)
        assert np.array_equal(shared["batches"][0][0][j], CV.prepare_triplet_reference(src.decode(i), HW, flip, rgb=True))
        assert np.array_equal(shared["batches"][0][1][j], src.intrinsics(i)[0])
        assert np.array_equal(shared["batches"][0][2][j], src.intrinsics(i)[1])


def test_set_equals_the_feeder_on_a_rank_shard(shared):
    src = shared["src"]
    flips = [src.sample(i)[1] for k in range(6) for i in prepared_data.batch_indices(k, 3, 2, 1)]
    assert set(flips) == {False, True}
    got = _collect(shared["set"].batches(3, 6, world=2, rank=1), 6)
    feeder = _collect(prepared_data.PreparedFeeder(src, 3, HW, dev(), 6, num_workers=0, world=2, rank=1), 6)
    assert _same(got, feeder) and not _same(got, shared["batches"])


def test_set_loaded_from_the_cache_yields_the_same_batches(shared, monkeypatch):
    def boom(self, i, out=None):
        raise AssertionError("decode called")
    monkeypatch.setattr(prepared_data.PreparedKITTI, "decode", boom)
    src = prepared_data.PreparedKITTI(shared["root"], 3, HW)
    again = prepared_data.ResidentTrainSet(src, HW, dev(), num_workers=2, cache_dir=shared["cache"], reserve_mb=64)
    assert again.from_cache and again.decoded == 0 and again.F == shared["set"].F
    assert torch.equal(again.tensors[0], shared["set"].tensors[0])
    assert _same(_collect(again.batches(3, 6), 6), shared["batches"])


def test_set_refuses_a_device_that_is_too_full(shared):
    free = torch.cuda.mem_get_info(dev())[0]
    with pytest.raises(DfeError, match="--data_source prepared"):
        prepared_data.ResidentTrainSet(shared["src"], HW, dev(), reserve_mb=free / (1 << 20))


# ================================================================================================ a replayed graph fed through out=
def test_graph_is_fed_in_place(shared):
    """Two identical seeded models in the deterministic mode, each with its own GraphedTrainStep: one is handed fresh tensors
    (the copy path), the other's static inputs are written by the gather itself.  Equal loss bits over three steps; the static
    inputs stay where they are and hold batch k before replay k.
    The frames are 256x832, not the tree's 64x208: Model_depth's PoseCNN ends in Linear(14, 14) over a 2x7 plane, which only that
    size (seven halvings of it) yields -- at 64x208 the model cannot be run at all.  The set is the same tree resized to it."""
    from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import GraphedTrainStep, make_cfg, make_optimizer
    before = convs.DETERMINISTIC
    convs.set_deterministic(True)
    try:
        hw = (256, 832)
        cfg = make_cfg(num_scales=3, img_hw=hw, mode="depth")
        src = prepared_data.PreparedKITTI(shared["root"], 3, hw)
        rset = prepared_data.ResidentTrainSet(src, hw, dev(), reserve_mb=64).batches(2, 4)
        assert rset.F == 14
        first = rset.fetch(0)
        steps = []
        for _ in range(2):
            torch.manual_seed(11)
            model = get_model("depth")(cfg).to(dev()).train()
            opt = make_optimizer(model, 1e-4, capturable=True)
            steps.append(GraphedTrainStep(model, opt, first, cfg, warmup=1))
        copied, fed = steps
        ptrs = [t.data_ptr() for t in fed.static_inputs]
        for k in range(3):
            fresh = rset.fetch(k)
            assert all(a.data_ptr() != b.data_ptr() for a, b in zip(fresh, copied.static_inputs))
            l_c = copied(fresh)[0].detach().clone()
            inputs = rset.fetch(k, out=fed.static_inputs)
            assert [t.data_ptr() for t in inputs] == ptrs == [t.data_ptr() for t in fed.static_inputs]
            assert all(torch.equal(a, b) for a, b in zip(fed.static_inputs, fresh))          # batch k's bits, before replay k
            l_f = fed(inputs)[0].detach().clone()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(l_c).all()) and G.bits_equal(l_c.reshape(-1), l_f.reshape(-1)), (k, float(l_c), float(l_f))
        assert not torch.equal(rset.fetch(0)[0], rset.fetch(1)[0])
    finally:
        convs.set_deterministic(before)


# ================================================================================================ train.py
def test_train_resident_source(shared, tmp_path):
    """train.py --data_source resident: exits 0, logs every iteration, writes last.pth in the reference's format."""
    cmd = [sys.executable, os.path.join(REPO, "train.py"), "-c", os.path.join(REPO, "config", "kitti_geom.yaml"),
           "--data_source", "resident", "--prepared_base_dir", shared["root"], "--mode", "depth", "--batch_size", "2",
           "--num_iterations", "3", "--num_workers", "2", "--log_interval", "1", "--save_interval", "3",
           "--model_dir", str(tmp_path / "models")]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "A total of 10 image pairs found" in out.stdout and "iter      2 total" in out.stdout, out.stdout[-2000:]
    assert "resident set: 14 frames" in out.stdout, out.stdout[-2000:]
    ck = torch.load(os.path.join(str(tmp_path / "models"), "depth", "last.pth"), map_location="cpu")
    assert set(ck.keys()) == {"iteration", "model_state_dict", "optimizer_state_dict"} and ck["iteration"] == 3
