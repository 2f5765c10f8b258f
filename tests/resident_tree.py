"""Helpers of tests/test_resident_cpu.py and tests/test_hip_resident.py (not a conftest: imported explicitly).

``build_shared_tree``: a miniature prepared tree whose consecutive strips SHARE frames the way a real drive's do -- strip i of a
drive is frames i, i+1, i+2 of the drive's frame list (a sliding window) -- with one drive per raw size.  ``NumpyStore``: the
device steps of ``prepared_data.ResidentTrainSet`` restated in numpy on the OpenCV restatement (tests/cv2_linear_u8.py), so that
the set's host half (plan, budget, cache, iteration) runs without a device."""
import os

import numpy as np

from tests import cv2_linear_u8 as CV
from tests import prepared_tree
from unsupervised_depth_opticalflow_egomotion_amd import kitti_io

LUT = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
SENTINEL = 0xA5


def build_shared_tree(root, n=10, sizes=prepared_tree.SMALL_SIZES, seed=0, n_calib=3):
    """Write n strips, n // len(sizes) (+1) per drive, drive d at raw size sizes[d]; returns (train.txt lines, frames) with
    frames[d] the drive's frame list (uint8 [h, w, 3], R, G, B as written): strip j of drive d is frames[d][j:j + 3]."""
    rng = np.random.default_rng(seed)
    calibs = []
    for k in range(n_calib):
        rel = os.path.join("calib", "c%d" % k, "calib_cam_to_cam.txt")
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        with open(os.path.join(root, rel), "w") as fh:
            fh.write(prepared_tree.calib_text(rng, k))
        calibs.append(rel)
    counts = [n // len(sizes) + (1 if d < n % len(sizes) else 0) for d in range(len(sizes))]
    lines, frames = [], []
    for d, ((h, w), cnt) in enumerate(zip(sizes, counts)):
        os.makedirs(os.path.join(root, "drive%d" % d), exist_ok=True)
        fl = [prepared_tree.strip(rng, h, w)[:h].copy() for _ in range(cnt + 2)]
        frames.append(fl)
        for j in range(cnt):
            rel = os.path.join("drive%d" % d, "%010d.png" % j)
            kitti_io.write_png(os.path.join(root, rel), np.concatenate(fl[j:j + 3], 0))
            lines.append("%s %s" % (rel, calibs[len(lines) % n_calib]))
    with open(os.path.join(root, "train.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return lines, frames


def stored_frame(frame_rgb, hw):
    """What the store holds of a decoded (R, G, B) frame: the restatement's resize in B, G, R planes, uint8 [3, H, W]."""
    return CV.resize_linear_u8(np.asarray(frame_rgb)[:, :, ::-1], hw).transpose(2, 0, 1).copy()


def gather_reference(store, tri, ktab, idx, flip):
    """out[b][c][f*H + y][x] = lut[store[tri[idx[b]][f]][c][y][flip ? W-1-x : x]] and the K rows, in numpy."""
    F, _, H, W = store.shape
    out = np.empty((len(idx), 3, 3 * H, W), np.float32)
    for b, i in enumerate(idx):
        for f in range(3):
            fr = store[tri[i, f]]
            out[b, :, f * H:(f + 1) * H] = LUT[fr[:, :, ::-1] if flip is not None and flip[b] else fr]
    return out, ktab[idx, 0].copy(), ktab[idx, 1].copy()


class NumpyStore:
    """prepared_data._HipStore's interface on the host."""

    def __init__(self):
        self.resize_calls = 0

    def alloc(self, F, img_hw):
        return np.full((F, 3, img_hw[0], img_hw[1]), SENTINEL, np.uint8)

    def resize(self, store, raw, sizes, offsets, slot, img_hw):
        self.resize_calls += 1
        for b, ((h0, w0), o) in enumerate(zip(sizes, offsets)):
            strip = raw[o:o + 9 * h0 * w0].reshape(3 * h0, w0, 3)
            for f in range(3):
                if slot[b, f] >= 0:
                    store[slot[b, f]] = stored_frame(strip[f * h0:(f + 1) * h0], img_hw)

    def load(self, store, frames):
        store[...] = frames

    def save(self, store, fh):
        fh.write(store.tobytes())

    def finish(self, store, tri, ktab, sizes, img_hw):
        return store, np.asarray(tri), np.asarray(ktab), LUT

    def gather(self, tensors, idx, flip, out):
        store, tri, ktab, _ = tensors
        res = gather_reference(store, tri, ktab, idx, flip)
        if out is None:
            return list(res)
        for dst, src in zip(out, res):
            dst[...] = src
        return list(out)
