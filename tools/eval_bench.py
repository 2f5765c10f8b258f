#!/usr/bin/env python3
"""One KITTI evaluation during training: eval_device.Evaluator.run() against the per-image path of test.py's tasks.

  python tools/eval_bench.py [--flow 200] [--depth 100] [--batch 4] [--rounds 2] [--session eager]

A synthetic set at KITTI's sizes -- ``--flow`` pairs with 375 x 1242 ground truth (valid / noc / moving masks) and ``--depth``
frames with sparse 375 x 1242 depth, 256 x 832 network inputs, a Model_geometry with seeded random weights -- is evaluated two ways
on the same arrays:
  fused      one ``Evaluator.run()`` over device-resident sets (flow 2015 + Eigen depth): batched inference through an
             InferenceSession, the metric kernels behind each batch, one host transfer per task;
  per-image  the bodies of test.py's ``test_kitti_flow`` / ``test_eigen_depth`` without their file reads: each prepared input
             uploaded and run at B = 1 through the model's own methods, then ``core.evaluation.eval_flow_avg`` / ``eval_depth``.
Neither includes reading or resizing PNGs (the per-image path of test.py pays that on every call as well; the sets pay it once).
Each figure is the host time of the whole evaluation, ending in its host transfer, after one untimed run of each; the two are
timed in turn ``--rounds`` times and every round is printed.  The tables of both are printed for comparison.

The tool sets no time limit of its own: run it under ``timeout``.  profiles/eval_device.txt is its output."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from core.evaluation import eval_depth, eval_flow_avg                                    # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd import eval_device                     # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model                # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg             # noqa: E402

GT_HW, IMG_HW, DISTINCT = (375, 1242), (256, 832), 8


def synthetic_arrays(n_flow, n_depth, seed=0):
    r = np.random.default_rng(seed)
    H, W = GT_HW
    flows, nocs, movs, depths = [], [], [], []
    for _ in range(DISTINCT):           # a few distinct samples, repeated: the work does not depend on the values
        valid = (r.random((H, W)) > 0.3).astype(np.float32)
        flows.append(np.concatenate([8 * r.standard_normal((H, W, 2)).astype(np.float32), valid[:, :, None]], 2))
        nocs.append(valid * (r.random((H, W)) > 0.2))
        movs.append((r.random((H, W)) > 0.7).astype(np.float32))
        depths.append(np.where(r.random((H, W)) > 0.95, r.uniform(1, 90, (H, W)), 0).astype(np.float32))   # LiDAR-sparse
    pick = lambda lst, n: [lst[i % DISTINCT] for i in range(n)]      # noqa: E731
    gen = torch.Generator().manual_seed(seed)
    pairs = torch.rand((n_flow, 3, 2 * IMG_HW[0], IMG_HW[1]), generator=gen)
    frames = torch.rand((n_depth, 3) + IMG_HW, generator=gen)
    return pick(flows, n_flow), pick(nocs, n_flow), pick(movs, n_flow), pick(depths, n_depth), pairs, frames


def per_image(model, cfg, dev, flows, nocs, movs, depths, pairs, frames):
    h = IMG_HW[0]
    preds = []
    with torch.no_grad():
        for i in range(len(flows)):
            img = pairs[i][None].to(dev)
            flow = model.inference_flow(img[:, :, :h].contiguous(), img[:, :, h:].contiguous())
            preds.append(flow[0].permute(1, 2, 0).contiguous())
        table = eval_flow_avg(flows, nocs, preds, cfg, moving_masks=movs)
        pred_depths = []
        for i in range(len(depths)):
            disp = model.infer_depth(frames[i][None].to(dev))
            disp = torch.nn.functional.interpolate(disp, GT_HW, mode="bilinear", align_corners=False)[0, 0]
            pred_depths.append(1.0 / (disp + 1e-4))
        return table, eval_depth(depths, pred_depths)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--flow", type=int, default=200)
    ap.add_argument("--depth", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--session", choices=("eager", "graph"), default="eager")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_bench.py needs a HIP device: a timing from anywhere else says nothing")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cfg = make_cfg(img_hw=IMG_HW, mode="geom")
    model = get_model("geom")(cfg).to(dev).eval()
    flows, nocs, movs, depths, pairs, frames = synthetic_arrays(args.flow, args.depth)
    t0 = time.perf_counter()
    fset = eval_device.FlowEvalSet(flows, nocs, movs, pairs, dev, "synthetic_2015")
    dset = eval_device.DepthEvalSet(depths, frames, dev)
    torch.cuda.synchronize()
    build = time.perf_counter() - t0
    ev = eval_device.Evaluator(model, cfg, flow_2015=fset, depth=dset, batch=args.batch, session=args.session)
    print("# %s; %d flow pairs + %d depth frames, ground truth %dx%d, inputs %dx%d, batch %d, session %s"
          % (torch.cuda.get_device_name(0), args.flow, args.depth, GT_HW[0], GT_HW[1], IMG_HW[0], IMG_HW[1], args.batch, args.session))
    print("# sets packed and uploaded once: %.2f s (from arrays; no PNG is read here)" % build)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, out
    run_fused = ev.run
    run_image = lambda: per_image(model, cfg, dev, flows, nocs, movs, depths, pairs, frames)      # noqa: E731
    timed(run_fused), timed(run_image)                                # warm-up: every shape, every library's algorithm choice
    for r in range(args.rounds):
        order = (("fused", run_fused), ("per-image", run_image))[::1 if r % 2 == 0 else -1]
        for name, fn in order:
            secs, out = timed(fn)
            print("round %d  %-9s  %8.3f s" % (r, name, secs), flush=True)
            if name == "fused":
                fused = out
            else:
                image = out
    print("fused     2015:\n%sfused     depth: %s" % (fused["eval_2015_res"], ["%.4f" % v for v in fused["eval_eigen_res"]]))
    print("per-image 2015:\n%sper-image depth: %s" % (image[0], ["%.4f" % v for v in image[1]]))


if __name__ == "__main__":
    main()
