"""dfe_prepare_triplets_u8 (ops.prepare_triplets_u8) against the OpenCV 8-bit resize restatement (tests/cv2_linear_u8.py),
equality of the fp32 output; the prefetching feeder (prepared_data.PreparedFeeder) against its serial path; train.py on a
prepared tree."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import cv2_linear_u8 as CV
from tests import prepared_tree
from unsupervised_depth_opticalflow_egomotion_amd import ops, prepared_data

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LUT = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


def dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _pack(strips, align=256):
    """Strips at 256-byte aligned offsets of one uint8 buffer (what the feeder's ring slots hold)."""
    offs, pos = [], 0
    for s in strips:
        offs.append(pos)
        pos += (s.size + align - 1) // align * align
    buf = np.zeros(pos, np.uint8)
    for s, o in zip(strips, offs):
        buf[o:o + s.size] = s.reshape(-1)
    return buf, offs


def _run(strips, hw, flips, rgb):
    buf, offs = _pack(strips)
    sizes = [(s.shape[0] // 3, s.shape[1]) for s in strips]
    out = ops.prepare_triplets_u8(torch.from_numpy(buf).to(dev()), sizes, hw, flips, offs, rgb=rgb)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(strips, hw, flips, rgb):
    got = _run(strips, hw, flips, rgb)
    assert got.shape == (len(strips), 3, 3 * hw[0], hw[1])
    for b, s in enumerate(strips):
        want = CV.prepare_triplet_reference(s, hw, flips[b], rgb)
        assert np.array_equal(got[b], want), (b, s.shape, hw, flips[b], rgb)
    return got


@pytest.mark.parametrize("rgb", [0, 1])
def test_u8_kernel_mixed_kitti_sizes(rgb):
    """375x1242, 370x1224 and 376x1241 strips in one batch to 256x832, flips on and off."""
    rng = np.random.default_rng(7 + rgb)
    strips = [prepared_tree.strip(rng, h, w) for h, w in ((375, 1242), (370, 1224), (376, 1241))]
    got = _check(strips, (256, 832), [1, 0, 1] if rgb else [0, 1, 0], rgb)
    assert np.isin(got, LUT).all()


@pytest.mark.parametrize("shape,hw", [((40, 60), (64, 128)),          # non-integer upscale
                                      ((512, 1664), (256, 832)),      # exact 1/2: INTER_AREA
                                      ((50, 190), (32, 95)),          # 285 bytes a row: 280 vector + 5 scalar
                                      ((37, 124), (32, 97)),          # 291 bytes: 288 vector + 3 scalar
                                      ((64, 128), (64, 128))])        # same size: copy
def test_u8_kernel_geometries(shape, hw):
    rng = np.random.default_rng(shape[0] * shape[1])
    strips = [rng.integers(0, 256, (3 * shape[0], shape[1], 3), dtype=np.uint8) for _ in range(2)]
    _check(strips, hw, [0, 1], 0)
    _check(strips, hw, [1, 0], 1)


def test_u8_kernel_constant_frames_on_lattice():
    """A constant strip of every value k: the output equals the restatement and sits on the float32(k / 255.0) lattice."""
    strips = [np.full((3 * 13, 29, 3), k, np.uint8) for k in range(256)]
    got = _check(strips, (8, 19), [k & 1 for k in range(256)], 0)
    assert np.isin(got, LUT).all()
    for k in (0, 1, 128, 254, 255):
        assert np.isin(got[k], LUT[max(k - 1, 0):k + 2]).all()


def test_u8_kernel_refuses_out_of_range_offsets():
    buf = torch.zeros(9 * 10 * 10, dtype=torch.uint8, device=dev())
    with pytest.raises(ValueError):
        ops.prepare_triplets_u8(buf, [(10, 10)], (5, 5), offsets=[1])


def _tree(tmp_path, n=10):
    root = str(tmp_path)
    prepared_tree.build_tree(root, n=n, seed=3)
    return root


def _collect(feeder, n):
    out = []
    for _ in range(n):
        img, k, ki = next(feeder)
        out.append((img.cpu().numpy(), k.cpu().numpy(), ki.cpu().numpy()))
    with pytest.raises(StopIteration):
        next(feeder)
    return out


def test_feeder_workers_equal_serial_path(tmp_path):
    """3 workers, ring depth 2 (slot reuse forced) over 8 batches: the same bits as num_workers=0, batches in idx order, and
    batch 0 equals the restatement on the decoded strips with the reader's flips and intrinsics."""
    root = _tree(tmp_path)
    src = prepared_data.PreparedKITTI(root, 3, (64, 208))
    serial = _collect(prepared_data.PreparedFeeder(src, 2, (64, 208), dev(), 8, num_workers=0), 8)
    par = _collect(prepared_data.PreparedFeeder(src, 2, (64, 208), dev(), 8, num_workers=3, depth=2), 8)
    for a, b in zip(serial, par):
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    for k in (0, 5):
        for j, idx in enumerate(prepared_data.batch_indices(k, 2)):
            i, flip = src.sample(idx)
            want = CV.prepare_triplet_reference(src.decode(i), (64, 208), flip, rgb=True)
            assert np.array_equal(serial[k][0][j], want)
            assert np.array_equal(serial[k][1][j], src.intrinsics(i)[0]) and np.array_equal(serial[k][2][j], src.intrinsics(i)[1])


def test_feeder_current_stream_path_equal(tmp_path):
    root = _tree(tmp_path)
    src = prepared_data.PreparedKITTI(root, 3, (64, 208))
    a = _collect(prepared_data.PreparedFeeder(src, 2, (64, 208), dev(), 3, num_workers=2), 3)
    b = _collect(prepared_data.PreparedFeeder(src, 2, (64, 208), dev(), 3, num_workers=2, side_stream=False), 3)
    assert all(np.array_equal(x, y) for p, q in zip(a, b) for x, y in zip(p, q))


class _Failing:
    """A source that fails on one data-list entry."""

    def __init__(self, src, bad):
        self.src, self.bad = src, bad
        self.headers, self.max_strip_bytes = src.headers, src.max_strip_bytes

    def __getattr__(self, name):
        return getattr(self.src, name)

    def decode(self, i, out=None):
        if i == self.bad:
            raise OSError("corrupt strip %d" % i)
        return self.src.decode(i, out)


def test_feeder_worker_exception_surfaces(tmp_path):
    root = _tree(tmp_path)
    src = prepared_data.PreparedKITTI(root, 3, (64, 208))
    bad = src.sample(prepared_data.batch_indices(2, 2)[1])[0]
    first_bad = min(k for k in range(6) if any(src.sample(i)[0] == bad for i in prepared_data.batch_indices(k, 2)))
    f = prepared_data.PreparedFeeder(_Failing(src, bad), 2, (64, 208), dev(), 6, num_workers=3)
    with pytest.raises(OSError, match="corrupt strip"):
        for _ in range(first_bad + 1):
            next(f)
    f.close()
    assert not f.threads


def test_train_prepared_source(tmp_path):
    """train.py --data_source prepared: exits 0, logs every iteration, writes last.pth in the reference's format."""
    root = _tree(tmp_path / "tree")
    cmd = [sys.executable, os.path.join(REPO, "train.py"), "-c", os.path.join(REPO, "config", "kitti_geom.yaml"),
           "--data_source", "prepared", "--prepared_base_dir", root, "--mode", "depth", "--batch_size", "2",
           "--num_iterations", "3", "--num_workers", "2", "--log_interval", "1", "--save_interval", "3",
           "--model_dir", str(tmp_path / "models")]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "A total of 10 image pairs found" in out.stdout and "iter      2 total" in out.stdout, out.stdout[-2000:]
    ck = torch.load(os.path.join(str(tmp_path / "models"), "depth", "last.pth"), map_location="cpu")
    assert set(ck.keys()) == {"iteration", "model_state_dict", "optimizer_state_dict"} and ck["iteration"] == 3
