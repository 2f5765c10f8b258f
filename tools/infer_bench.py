#!/usr/bin/env python3
"""The three inference entry points of the joint model, plain eval call against inference.InferenceSession (eager, graph replay).

  python tools/infer_bench.py [--methods infer_depth,inference_flow,infer_pose] [--batches 1,4] [--calls 60] [--rounds 3]
  python tools/infer_bench.py --count-launches          # a run of its own: the profiler slows the host

Per (method, batch) at 256x832 the three configurations are timed in turn, ``--rounds`` times, the order rotating (A/B/C, B/C/A,
...) so that a drift of the box hits them alike.  One timed window = ``--calls`` calls after ``--warmup`` calls, the device
synchronised before and after the whole window:
  ms/call   the median over the window's calls of the device-event time from one call's start to the next one's (events are
            recorded in stream order without a host wait, so a host-bound call shows its enqueue period here);
  wall      the window's host time over its calls (includes the final synchronise);
  enqueue   the host time until the last call has returned, over the calls -- what the host spends per call.
The table shows the median of the rounds.  ``--count-launches`` counts the device kernels of one call with torch.profiler.

The tool sets no time limit of its own.  Run every GPU step as a process of its own under ``timeout``, and stop at the first that
fails -- how profiles/inference_session.txt was made:

  for m in infer_depth inference_flow infer_pose; do timeout -k 10 240 python tools/infer_bench.py --methods $m --calls 300 || break; done
  for m in infer_depth inference_flow infer_pose; do timeout -k 10 240 python tools/infer_bench.py --methods $m --count-launches || break; done"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unsupervised_depth_opticalflow_egomotion_amd import synthetic                      # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd.inference import InferenceSession     # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd.models import get_model               # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg            # noqa: E402

H, W = 256, 832
CONFIGS = ("plain", "eager", "graph")


def inputs_of(method, B, dev):
    im = torch.from_numpy(synthetic.make_triplet_batch(B, H, W, 3, seed=11)[0]).to(dev)
    l, t, r = (im[:, :, k * H:(k + 1) * H].contiguous() for k in range(3))
    return {"infer_depth": (t,), "inference_flow": (t, r), "infer_pose": (torch.cat([l, t, r], 1),)}[method]


def window(fn, calls):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(calls + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        ev[i].record()
        fn()
    ev[calls].record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    per = [ev[i].elapsed_time(ev[i + 1]) for i in range(calls)]
    return statistics.median(per), (t2 - t0) * 1e3 / calls, (t1 - t0) * 1e3 / calls


def count_launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sum(1 for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()), len(names)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--methods", default="infer_depth,inference_flow,infer_pose")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--count-launches", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("infer_bench.py needs a HIP device: a timing from anywhere else says nothing")
    if args.calls < 50 and not args.count_launches:
        raise SystemExit("--calls must be at least 50")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = get_model("geom")(make_cfg()).to(dev).eval()
    sessions = {"eager": InferenceSession(model), "graph": InferenceSession(model, graph=True)}
    print("# %s, %dx%d, %d calls per window after %d warm-up calls, %d rounds (median shown)"
          % (torch.cuda.get_device_name(0), H, W, args.calls, args.warmup, args.rounds))
    print("%-15s %2s %-6s %9s %9s %9s" % ("method", "B", "config", "ms/call", "wall", "enqueue") if not args.count_launches else
          "%-15s %2s %-6s %9s %9s" % ("method", "B", "config", "kernels", "+copies"))
    for method in args.methods.split(","):
        for B in (int(b) for b in args.batches.split(",")):
            x = inputs_of(method, B, dev)
            fns = {"plain": lambda: getattr(model, method)(*x)}
            fns.update({k: (lambda s=s: getattr(s, method)(*x)) for k, s in sessions.items()})
            with torch.no_grad():
                for c in CONFIGS:
                    for _ in range(args.warmup):
                        fns[c]()
                torch.cuda.synchronize()
                if args.count_launches:
                    for c in CONFIGS:
                        k, n = count_launches(fns[c])
                        print("%-15s %2d %-6s %9d %9d" % (method, B, c, k, n - k), flush=True)
                    continue
                res = {c: [] for c in CONFIGS}
                for r in range(args.rounds):
                    for c in CONFIGS[r % 3:] + CONFIGS[:r % 3]:
                        res[c].append(window(fns[c], args.calls))
            for c in CONFIGS:
                med = [statistics.median(v[i] for v in res[c]) for i in range(3)]
                spread = max(v[0] for v in res[c]) - min(v[0] for v in res[c])
                print("%-15s %2d %-6s %9.3f %9.3f %9.3f   (ms/call over the rounds: +-%.3f)" % (method, B, c, med[0], med[1], med[2], spread / 2),
                      flush=True)
    print("# session stats: %s" % {k: s.stats() for k, s in sessions.items()})


if __name__ == "__main__":
    main()
