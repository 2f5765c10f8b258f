"""Helpers of the device-evaluation tests (test_eval_device_cpu.py, test_hip_eval_device.py).  Not a conftest: imported explicitly.

* ``mini_tree``: miniature KITTI-shaped trees written with ``kitti_io``'s own writers -- 3 flow pairs per year and 3 Eigen frames,
  ground truth at two sizes around 40 x 136 -- and a config namespace naming them.
* ``flow_case`` / ``depth_case``: synthetic ground truth and predictions for the kernel tests, CONDITIONED: every pixel whose
  float64 decision lies within a relative ``BAND`` of its threshold is moved (never dropped), and ``*_near`` counts what is left.
  BAND = 1e-4 is about a hundred fp32 roundings of these chains (each a handful of operations of 6e-8)."""
import os
import types

import numpy as np

BAND = 1e-4
GT_SIZES = ((37, 61), (40, 64), (33, 130), (48, 70), (37, 61))      # within one batch; widths no multiple of 4 or 64 but one
PRED_SIZES = ((16, 32), (24, 40))                                     # no integer ratio to any of the above
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0


# ------------------------------------------------------------------------------------------------ float64 restatements
def resize64(img, out_hw):
    """oracle.eval_oracle.resize_linear without its final rounding to fp32 (for decision margins)"""
    h, w = img.shape[:2]
    H, W = out_hw
    ys = np.clip((np.arange(H) + 0.5) * (h / H) - 0.5, 0, None)
    xs = np.clip((np.arange(W) + 0.5) * (w / W) - 0.5, 0, None)
    y0 = np.minimum(np.floor(ys).astype(int), h - 1); x0 = np.minimum(np.floor(xs).astype(int), w - 1)
    y1 = np.minimum(y0 + 1, h - 1); x1 = np.minimum(x0 + 1, w - 1)
    shape = (-1, 1) + (1,) * (img.ndim - 2)
    wy = (ys - y0).reshape(shape); wx = (xs - x0).reshape((1, -1) + (1,) * (img.ndim - 2))
    im = img.astype(np.float64)
    top = im[y0][:, x0] * (1 - wx) + im[y0][:, x1] * wx
    bot = im[y1][:, x0] * (1 - wx) + im[y1][:, x1] * wx
    return top * (1 - wy) + bot * wy


def _near(value, threshold):
    return np.abs(value - threshold) <= BAND * abs(threshold)


def flow_near(gt, pred, pred_hw):
    """pixels of one sample whose outlier decisions (epe against 3, epe / mag against 0.05) lie inside the band, in float64"""
    H, W = gt.shape[:2]
    p = pred.astype(np.float64).copy()
    p[:, :, 0] = p[:, :, 0] / pred_hw[1] * W
    p[:, :, 1] = p[:, :, 1] / pred_hw[0] * H
    flo = resize64(p, (H, W))
    g = gt.astype(np.float64)
    epe = np.sqrt(((flo - g[:, :, :2]) ** 2).sum(2))
    mag = np.maximum(np.sqrt((g[:, :, :2] ** 2).sum(2)), 1e-10)
    return _near(epe, 3.0) | _near(epe / mag, 0.05)


def depth_near(gt, disp):
    """pixels of one sample whose decisions (gt against min / max, max(gt / pred, pred / gt) against 1.25^k) lie inside the band"""
    from unsupervised_depth_opticalflow_egomotion_amd.eval_device import crop_box
    H, W = gt.shape
    g = gt.astype(np.float64)
    near = _near(g, MIN_DEPTH) | _near(g, MAX_DEPTH)
    pred = 1.0 / (resize64(disp, (H, W)) + 1e-4)
    y0, y1, x0, x1 = crop_box(H, W)
    mask = (g > MIN_DEPTH) & (g < MAX_DEPTH)
    crop = np.zeros_like(mask); crop[y0:y1, x0:x1] = True
    mask &= crop
    if mask.any():
        pm = pred * (np.median(g[mask]) / np.median(pred[mask]))
        pm = np.clip(pm, MIN_DEPTH, MAX_DEPTH)
        th = np.maximum(np.clip(g, MIN_DEPTH, MAX_DEPTH) / pm, pm / np.clip(g, MIN_DEPTH, MAX_DEPTH))
        for k in (1, 2, 3):
            near |= mask & _near(th, 1.25 ** k)
    return near, mask


# ------------------------------------------------------------------------------------------------ kernel-test inputs
def flow_case(pred_hw, seed=0, sizes=GT_SIZES):
    """(gt_flows [H,W,3] fp32, noc masks, moving masks, preds [h,w,2] fp32).  Sample 1 has noc == valid (the occ denominator is 0
    and clamped to 1), sample 0 a pixel with noc = 1 and valid = 0, every sample valid pixels of zero ground-truth flow (the
    1e-10 clamp of the magnitude)."""
    r = np.random.default_rng(seed)
    gts, nocs, movs, preds = [], [], [], []
    for i, (H, W) in enumerate(sizes):
        uv = (4 * r.standard_normal((H, W, 2))).astype(np.float32)
        uv[r.random((H, W)) < 0.05] = 0.0
        valid = (r.random((H, W)) > 0.3).astype(np.float32)
        noc = valid * (r.random((H, W)) > 0.2)
        if i == 1:
            noc = valid.copy()
        if i == 0:
            valid[3, 5], noc[3, 5] = 0.0, 1.0
        valid[2, 2], uv[2, 2] = 1.0, 0.0
        pred = (2 * r.standard_normal(tuple(pred_hw) + (2,))).astype(np.float32)
        gt = np.concatenate([uv, valid[:, :, None]], 2).astype(np.float32)
        for _ in range(20):                                   # move, never drop: the ground truth of a pixel is its own
            near = flow_near(gt, pred, pred_hw)
            if not near.any():
                break
            bump = (0.37 + 0.2 * r.random(int(near.sum()))).astype(np.float32)
            gt[near, 0] += bump
        gts.append(gt); nocs.append(noc.astype(np.float32)); preds.append(pred)
        movs.append((r.random((H, W)) > 0.6).astype(np.float32))
    return gts, nocs, movs, preds


def depth_case(pred_hw, kind, seed=0, sizes=GT_SIZES):
    """(gt depths [H,W] fp32, disps [h,w] fp32).  Masked counts: sample 0 odd, 1 even, 2 exactly one, 3 exactly two, 4 dense.
    ``kind``: 'uniform' disparities, 'constant' (every pred equal: the select sees ties) or 'span' (1e-3 ... 1, log-uniform: the
    digits of every radix pass differ).  ``pred_hw`` None: each disparity at its ground truth's size (the resize is the identity)."""
    from unsupervised_depth_opticalflow_egomotion_amd.eval_device import crop_box
    r = np.random.default_rng(seed)
    gts, disps = [], []
    for i, (H, W) in enumerate(sizes):
        hw = (H, W) if pred_hw is None else tuple(pred_hw)
        if kind == "constant":
            disp = np.full(hw, 0.3, np.float32)
        elif kind == "span":
            disp = np.exp(r.uniform(np.log(1e-3), 0.0, hw)).astype(np.float32)
        else:
            disp = r.uniform(0.05, 1.0, hw).astype(np.float32)
        y0, y1, x0, x1 = crop_box(H, W)
        gt = np.where(r.random((H, W)) > (0.3 if i == 4 else 0.8), r.uniform(2, 60, (H, W)), 0).astype(np.float32)
        gt[r.random((H, W)) > 0.97] = 90.0                    # beyond max_depth, some inside the crop
        gt[r.random((H, W)) > 0.97] = 5e-4                    # below min_depth
        inside = np.zeros((H, W), bool); inside[y0:y1, x0:x1] = True
        if i in (2, 3):
            gt[inside] = 0
            gt[y0 + 1, x0 + 3] = 7.5
            if i == 3:
                gt[y1 - 1, x1 - 1] = 31.0
        for _ in range(40):
            near, mask = depth_near(gt, disp)
            want_odd = {0: True, 1: False}.get(i)
            if want_odd is not None and (int(mask.sum()) % 2 == 1) != want_odd:
                ys, xs = np.nonzero(mask)
                gt[ys[0], xs[0]] = 0
                continue
            if not near.any():
                break
            gt[near] = (gt[near] * (1.013 + 0.01 * r.random(int(near.sum())))).astype(np.float32)
        gts.append(gt); disps.append(disp)
    return gts, disps


# ------------------------------------------------------------------------------------------------ miniature trees
def mini_tree(root, img_hw=(64, 128), sizes=((40, 136), (38, 132), (40, 136)), seed=7):
    """flow2012 / flow2015 (image_2, flow_occ, flow_noc, obj_map, calib_cam_to_cam) and raw + eigen under ``root``; returns a config
    namespace naming them (``img_hw``, ``gt_2012_dir``, ``gt_2015_dir``, ``raw_base_dir``, ``eigen_dir``)."""
    from PIL import Image
    from unsupervised_depth_opticalflow_egomotion_amd import kitti_io as K, synthetic
    r = np.random.default_rng(seed)

    def image(s, hw):
        a = synthetic.smooth_texture(np.random.default_rng(s), (1, 3) + tuple(hw))[0]
        return (np.clip(a, 0, 1) * 255).astype(np.uint8).transpose(1, 2, 0)
    calib = "P_rect_02: 2.3e+02 0 2.0e+02 0 0 2.3e+02 6.0e+01 0 0 0 1 0\nP2: 2.3e+02 0 2.0e+02 0 0 2.3e+02 6.0e+01 0 0 0 1 0\n"
    for year in (2012, 2015):
        d = os.path.join(root, "flow%d" % year)
        for sub in ("image_2", "flow_occ", "flow_noc", "obj_map", "calib_cam_to_cam"):
            os.makedirs(os.path.join(d, sub), exist_ok=True)
        for i, hw in enumerate(sizes):
            stem = "%06d" % i
            Image.fromarray(image(100 * year + 10 * i, hw)).save(os.path.join(d, "image_2", stem + "_10.png"))
            Image.fromarray(image(100 * year + 10 * i + 1, hw)).save(os.path.join(d, "image_2", stem + "_11.png"))
            flow = r.normal(0, 4, hw + (2,))
            valid = r.random(hw) > 0.4
            K.write_flow_png(os.path.join(d, "flow_occ", stem + "_10.png"), flow, valid)
            K.write_flow_png(os.path.join(d, "flow_noc", stem + "_10.png"), flow, valid & (r.random(hw) > 0.2))
            if year == 2015:
                Image.fromarray(((r.random(hw) > 0.7) * 3).astype(np.uint8)).save(os.path.join(d, "obj_map", stem + "_10.png"))
            with open(os.path.join(d, "calib_cam_to_cam", stem + ".txt"), "w") as fh:
                fh.write(calib)
    raw, eig = os.path.join(root, "raw"), os.path.join(root, "eigen")
    os.makedirs(os.path.join(raw, "2011_09_26/drive_0001/image_02/data"), exist_ok=True)
    os.makedirs(eig, exist_ok=True)
    lines, gts = [], np.empty(len(sizes), object)
    for i, hw in enumerate(sizes):
        Image.fromarray(image(50 + i, hw)).save(os.path.join(raw, "2011_09_26/drive_0001/image_02/data/%010d.png" % i))
        lines.append("2011_09_26/drive_0001 %010d l" % i)
        g = r.uniform(2, 60, hw).astype(np.float32)
        g[r.random(hw) > 0.4] = 0
        gts[i] = g
    with open(os.path.join(eig, "test_files.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    np.savez(os.path.join(eig, "gt_depths.npz"), data=gts)
    return types.SimpleNamespace(img_hw=tuple(img_hw), gt_2012_dir=os.path.join(root, "flow2012"),
                                 gt_2015_dir=os.path.join(root, "flow2015"), raw_base_dir=raw, eigen_dir=eig,
                                 config_file="mini", mode="geom", result_dir=None)
