"""Seeded miniature prepared KITTI trees: what ``KITTI_RAW.prepare_data_mp`` leaves behind and ``KITTI_Prepared`` reads
(core/dataset/kitti_prepared.py:22-33,101-108) -- ``train.txt`` lines ``<image> <calib>`` relative to the tree, stacked-triplet
PNG strips [3*h, w, 3] and ``calib_cam_to_cam.txt`` files whose LAST line holds the 3x4 projection the reader uses.

Used by tests/test_prepared_cpu.py, tests/test_hip_prepared_feed.py, tests/golden/make_golden_prepared.py and
tools/feed_bench.py."""
import os

import numpy as np

from unsupervised_depth_opticalflow_egomotion_amd import kitti_io

SMALL_SIZES = ((30, 100), (27, 90))            # two raw frame sizes (h, w), 3*h rows per strip
KITTI_SIZES = ((375, 1242), (370, 1224), (374, 1238), (376, 1241))


def strip(rng, h, w):
    """A smooth-ish uint8 [3*h, w, 3] strip (a panning texture plus noise) -- PNG-compressible like a real frame."""
    base = rng.integers(0, 256, (h // 4 + 2, (w + 32) // 4 + 2, 3)).astype(np.float32)
    big = np.repeat(np.repeat(base, 4, 0), 4, 1)[:h, :w + 32]
    frames = [big[:, 8 * f:8 * f + w] for f in range(3)]
    im = np.concatenate(frames, 0) + rng.normal(0, 6, (3 * h, w, 3))
    return np.clip(np.rint(im), 0, 255).astype(np.uint8)


def calib_text(rng, k):
    """A calib_cam_to_cam.txt-like file: a few lines, the last one ``P_rect_03: <12 values>`` with distinct intrinsics."""
    f = 700.0 + 7.25 * k + float(rng.integers(0, 50))
    cx, cy = 600.0 + 1.5 * k, 170.0 + 0.75 * k
    p2 = [f, 0.0, cx, 44.85, 0.0, f, cy, 0.2163, 0.0, 0.0, 1.0, 0.002745]
    p3 = [f + 0.5, 0.0, cx + 0.25, -337.2, 0.0, f + 0.5, cy - 0.125, 2.369, 0.0, 0.0, 1.0, 0.004915]
    lines = ["calib_time: 09-Jan-2012 13:57:47", "corner_dist: 9.950000e-02",
             "P_rect_02: " + " ".join("%.6e" % v for v in p2),
             "P_rect_03: " + " ".join("%.6e" % v for v in p3)]
    return "\n".join(lines) + "\n"


def build_tree(root, n=8, sizes=SMALL_SIZES, seed=0, n_calib=3):
    """Write ``n`` strips cycling through ``sizes`` and ``n_calib`` calib files under ``root``; return the train.txt lines."""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "drive"), exist_ok=True)
    calibs = []
    for k in range(n_calib):
        rel = os.path.join("calib", "c%d" % k, "calib_cam_to_cam.txt")
        os.makedirs(os.path.dirname(os.path.join(root, rel)), exist_ok=True)
        with open(os.path.join(root, rel), "w") as fh:
            fh.write(calib_text(rng, k))
        calibs.append(rel)
    lines = []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        rel = os.path.join("drive", "%010d.png" % i)
        kitti_io.write_png(os.path.join(root, rel), strip(rng, h, w))
        lines.append("%s %s" % (rel, calibs[i % n_calib]))
    with open(os.path.join(root, "train.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    return lines
