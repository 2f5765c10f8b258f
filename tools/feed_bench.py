#!/usr/bin/env python3
"""What feeding the training loop from a prepared KITTI tree costs (prepared_data.PreparedFeeder), next to bench.py's resident
batch.  Writes a seeded miniature prepared tree of KITTI-sized PNG strips (tests/prepared_tree.py; 375x1242, 370x1224, 374x1238,
376x1241 frames) to a temp dir and times the same loop body -- ``inputs = <source>; train_step(model, opt, inputs, cfg)`` -- as

  (a) resident   one batch kept in HBM and replayed (what bench.py measures)
  (b) memory     the feeder over strips decoded up front (no PNG decode: the feeder's own ring / upload / prepare overhead),
                 with the upload + prepare on the feeder's side stream and, for comparison, on the training stream
  (c) png        the feeder over the PNG tree, --workers decode threads each
  (d) resident set  prepared_data.ResidentTrainSet over the same tree: every frame resized once into HBM, a batch is one gather
                 launch (its build seconds, decode throughput and the host time of fetch() are reported)

per line: ms/step (device-synchronised wall time over --steps after --warmup), frame-pairs/s (2B per step), the host time a step
spends blocked in next() (wait) and the host time to enqueue the step (train_step's return) per step.  Also PIL's decode time
of one strip on one thread and per strip with 6 threads.  ``--repeat R`` alternates lines (a), (c) at the first --workers count
and (d) R times within the process (run-to-run spread on one clock); ``--graph`` also runs (a) and (d) through
train_step.GraphedTrainStep ((d) writes the graph's static inputs in place).  One process; run each GPU invocation under
``timeout -k 10``:

  timeout -k 10 600 python tools/feed_bench.py --batch 4 --steps 40 --warmup 8 --workers 0,6,12
"""
import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import prepared_tree  # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd import prepared_data  # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model  # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd.train_step import GraphedTrainStep, make_cfg, make_optimizer, train_step  # noqa: E402


def decode_times(src, threads):
    n = src.count()
    t = time.perf_counter()
    for i in range(n):
        src.decode(i)
    one = (time.perf_counter() - t) / n
    with ThreadPoolExecutor(threads) as ex:
        t = time.perf_counter()
        list(ex.map(src.decode, range(n)))
        many = (time.perf_counter() - t) / n
    return one * 1e3, many * 1e3


def timed(model, opt, cfg, get_inputs, warmup, steps, batch, step=None):
    """``step(inputs)``: what runs the step (default: the eager train_step)"""
    if step is None:
        step = lambda inputs: train_step(model, opt, inputs, cfg)      # noqa: E731
    for _ in range(warmup):
        step(get_inputs())
    torch.cuda.synchronize()
    wait = enq = 0.0
    t0 = time.perf_counter()
    for _ in range(steps):
        a = time.perf_counter()
        inputs = get_inputs()
        b = time.perf_counter()
        step(inputs)
        c = time.perf_counter()
        wait += b - a
        enq += c - b
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"ms_per_step": round(dt * 1e3, 3), "frame_pairs_per_s": round(2 * batch / dt, 2),
            "next_wait_ms": round(wait / steps * 1e3, 3), "enqueue_ms": round(enq / steps * 1e3, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--mode", default="geom")
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=832)
    ap.add_argument("--strips", type=int, default=16, help="PNG strips in the miniature tree")
    ap.add_argument("--workers", default="0,6,12", help="decode thread counts for line (c)")
    ap.add_argument("--repeat", type=int, default=1, help="alternate lines (a), (c) and (d) this many times")
    ap.add_argument("--graph", action="store_true", help="also run lines (a) and (d) through GraphedTrainStep")
    ap.add_argument("--json", default=None, help="also write the results here")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    hw, B = (args.height, args.width), args.batch
    res = {"config": vars(args), "lines": []}
    with tempfile.TemporaryDirectory() as root:
        t = time.perf_counter()
        prepared_tree.build_tree(root, n=args.strips, sizes=prepared_tree.KITTI_SIZES, seed=0)
        print("tree: %d strips written in %.1f s" % (args.strips, time.perf_counter() - t), flush=True)
        src = prepared_data.PreparedKITTI(root, 3, hw)
        one, six = decode_times(src, 6)
        res["pil_decode_ms_per_strip"] = {"threads_1": round(one, 2), "threads_6": round(six, 2)}
        print("PIL decode of one %dx%d strip: %.1f ms on 1 thread, %.1f ms per strip on 6 threads"
              % (src.headers[0][0], src.headers[0][1], one, six), flush=True)
        mem = prepared_data.InMemoryStrips(src)
        cfg = make_cfg(num_scales=3, img_hw=hw, mode=args.mode)
        torch.manual_seed(1234)
        model = get_model(args.mode)(cfg).to(dev)
        model.train()
        opt = make_optimizer(model, cfg.lr)
        n = args.warmup + args.steps

        def feeder_line(name, source, workers, side=True):
            f = prepared_data.PreparedFeeder(source, B, hw, dev, n, num_workers=workers, side_stream=side)
            try:
                r = timed(model, opt, cfg, lambda: next(f), args.warmup, args.steps, B)
            finally:
                f.close()
            r.update(line=name, workers=workers, side_stream=side)
            res["lines"].append(r)
            print(json.dumps(r), flush=True)
            return r

        first = prepared_data.PreparedFeeder(mem, B, hw, dev, 1)
        resident = next(first)
        first.close()
        def line(name, r, **extra):
            r.update(line=name, **extra)
            res["lines"].append(r)
            print(json.dumps(r), flush=True)
            return r

        t = time.perf_counter()
        rset = prepared_data.ResidentTrainSet(src, hw, dev, num_workers=6)
        built = time.perf_counter() - t
        res["resident_set"] = {"frames": rset.F, "bytes": rset.nbytes, "build_s": round(built, 3), "strips_decoded": rset.decoded,
                               "decode_strips_per_s": round(rset.decoded / built, 1)}
        print("resident set: %d frames, %d bytes, built in %.2f s (%d strip decodes on 6 threads, two passes: %.1f strips/s)"
              % (rset.F, rset.nbytes, built, rset.decoded, rset.decoded / built), flush=True)

        def resident_line(name="d_resident_set", step=None, out=None):
            rset.batches(B, n)
            k = [0]

            def fetch():
                k[0] += 1
                return rset.fetch(k[0] - 1, out=out)
            # next_wait_ms is fetch()'s host time here: the draw of the batch plus one launch
            return line(name, timed(model, opt, cfg, fetch, args.warmup, args.steps, B, step))

        workers = [int(x) for x in args.workers.split(",") if x != ""]
        a = line("a_resident", timed(model, opt, cfg, lambda: resident, args.warmup, args.steps, B))
        b = feeder_line("b_memory", mem, 6)
        feeder_line("b_memory", mem, 6, side=False)
        for w in workers:
            feeder_line("c_png", src, w)
        resident_line()
        for _ in range(args.repeat - 1):              # (a), (c), (d) alternated: the spread of each on one clock
            line("a_resident", timed(model, opt, cfg, lambda: resident, args.warmup, args.steps, B))
            if workers:
                feeder_line("c_png", src, workers[0])
            resident_line()
        if args.graph:
            # a capturable optimiser of its own (the step count on the device); the weights it trains are the same model's
            gopt = make_optimizer(model, cfg.lr, capturable=True)
            graphed = GraphedTrainStep(model, gopt, resident, cfg)
            for _ in range(args.repeat):
                # (a): the static inputs hold the batch already -- graphed(None) replays without a copy
                line("a_resident_graph", timed(model, gopt, cfg, lambda: None, args.warmup, args.steps, B, graphed))
                resident_line("d_resident_set_graph", graphed, graphed.static_inputs)
        res["b_over_a_throughput"] = round(b["frame_pairs_per_s"] / a["frame_pairs_per_s"], 4)
        res["b_over_a_enqueue"] = round(b["enqueue_ms"] / a["enqueue_ms"], 4)
        print("(b)/(a): throughput %.4f, enqueue %.4f" % (res["b_over_a_throughput"], res["b_over_a_enqueue"]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
