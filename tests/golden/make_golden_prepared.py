#!/usr/bin/env python3
"""Generate tests/golden/G13_prepared.npz by RUNNING THE REAL REFERENCE ``KITTI_Prepared`` (core/dataset/kitti_prepared.py).

Runs only in the build container, where the reference checkout exists; tests read only the saved arrays.  The tree comes from
tests/prepared_tree.py (seed 13, two raw sizes, three calib files with distinct last lines).  ``cv2`` is a recording stub, as
in make_golden.py: ``imread`` records the path and returns the PIL-decoded strip in B, G, R order, ``flip`` records that it was
called, ``resize`` returns zeros of the requested shape -- the image arithmetic is not what this fixture pins.  Saved for
idx 0..63 of a dataset built as the reference's train.py builds it (num_iterations not None): the data-list index
``KITTI_Prepared.__getitem__`` read (from the recorded path), the flip bit, K_ms and K_inv_ms.

Usage:  python tests/golden/make_golden_prepared.py"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, REPO)

from tests import prepared_tree  # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd import kitti_io  # noqa: E402

N_IDX, NUM_SCALES, IMG_HW, N_SAMPLES, SEED = 64, 3, (256, 832), 10, 13


def install_cv2_stub(log):
    cv2 = types.ModuleType("cv2")

    def imread(path):
        log.append(("imread", path))
        return kitti_io.read_image_bgr(path)

    def flip(img, code):
        log.append(("flip", code))
        return img

    def resize(img, dsize):
        return np.zeros((dsize[1], dsize[0]) + img.shape[2:], img.dtype)
    cv2.imread, cv2.flip, cv2.resize = imread, flip, resize
    sys.modules["cv2"] = cv2


def main():
    log = []
    install_cv2_stub(log)
    # the module file alone: core/dataset/__init__.py imports every dataset (imageio, ...), which this fixture does not need
    import importlib.util
    spec = importlib.util.spec_from_file_location("kitti_prepared", os.path.join(REF, "core", "dataset", "kitti_prepared.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    KITTI_Prepared = mod.KITTI_Prepared
    with tempfile.TemporaryDirectory() as root:
        lines = prepared_tree.build_tree(root, n=N_SAMPLES, seed=SEED)
        images = [os.path.join(root, ln.split()[0]) for ln in lines]
        ds = KITTI_Prepared(root, num_scales=NUM_SCALES, img_hw=IMG_HW, num_iterations=N_IDX)
        index, flips, kms, kinvs = [], [], [], []
        for idx in range(N_IDX):
            del log[:]
            _, k, ki = ds[idx]
            index.append(images.index([p for what, p in log if what == "imread"][0]))
            flips.append(int(any(what == "flip" for what, _ in log)))
            kms.append(k.numpy())
            kinvs.append(ki.numpy())
    out = os.path.join(HERE, "G13_prepared.npz")
    np.savez_compressed(out, index=np.array(index, np.int64), flip=np.array(flips, np.uint8), K_ms=np.stack(kms),
                        K_inv_ms=np.stack(kinvs), n_samples=N_SAMPLES, seed=SEED, img_hw=np.array(IMG_HW),
                        num_scales=NUM_SCALES)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
