#!/usr/bin/env python3
"""train.py --graph and --resume through the prepared source (--data_source prepared), each against an eager run on the same
batches, on a miniature tree of KITTI-sized strips (tests/prepared_tree.py).  train.py seeds nothing, so the graph pair starts
from one checkpoint (loaded as --flow_pretrained_model / --depth_pretrained_model in geom mode); the resume pair runs with
--lr 0, so the resumed iterations 2-3 (idx restarts at 0: batches 0-1) must log what iterations 0-1 of the first run logged.
Tolerance: one unit of the printed fourth decimal.  Exit 0 when both agree.  Needs a HIP device:

  timeout -k 10 500 python tools/prepared_train_check.py geom
"""
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import prepared_tree  # noqa: E402

tmp = TREE = None


def run(args, tag):
    """One train.py process on the tree; {iteration: [total, term, ...]} of its logged lines."""
    cmd = [sys.executable, os.path.join(REPO, "train.py"), "-c", os.path.join(REPO, "config", "kitti_geom.yaml"),
           "--data_source", "prepared", "--prepared_base_dir", TREE, "--batch_size", "2", "--num_workers", "2",
           "--log_interval", "1"] + args
    print("$ python " + " ".join(cmd[1:]).replace(REPO + os.sep, "").replace(tmp, "$TMP"), flush=True)
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=REPO, timeout=300)
    print("[%s] exit %d" % (tag, out.returncode), flush=True)
    if out.returncode != 0:
        print(out.stderr[-3000:])
        sys.exit(1)
    lines = [l for l in out.stdout.splitlines() if l.startswith("iter")]
    for l in lines:
        print("  " + l)
    return {int(l.split()[1]): [float(l.split()[3])] + [float(t.rsplit(":", 1)[1]) for t in l.split("|")[1].split()] for l in lines}


def cmp(a, b, pairs, tag, tol=1e-4):
    worst = 0.0
    for ia, ib in pairs:
        x, y = a[ia], b[ib]
        worst = max(worst, max(abs(p - q) for p, q in zip(x, y)))
    ok = worst <= tol + 1e-9
    print("[%s] max |difference| of the logged total and terms (printed to 4 decimals) %.4g, tolerance %g (one printed unit): %s"
          % (tag, worst, tol, "OK" if ok else "FAIL"), flush=True)
    return ok


def main():
    global tmp, TREE
    tmp = tempfile.mkdtemp()
    TREE = os.path.join(tmp, "tree")
    prepared_tree.build_tree(TREE, n=12, sizes=prepared_tree.KITTI_SIZES, seed=5)
    mode = sys.argv[1] if len(sys.argv) > 1 else "geom"
    # one checkpoint gives both processes the same initial weights (train.py seeds nothing): geom loads it as flow + depth model
    run(["--mode", mode, "--num_iterations", "1", "--save_interval", "1", "--model_dir", os.path.join(tmp, "init")], "init")
    ck = os.path.join(tmp, "init", mode, "last.pth")
    pre = ["--flow_pretrained_model", ck, "--depth_pretrained_model", ck]
    eager = run(["--mode", mode, "--num_iterations", "4", "--save_interval", "100", "--model_dir", os.path.join(tmp, "e")] + pre, "eager")
    graph = run(["--mode", mode, "--num_iterations", "4", "--save_interval", "100", "--graph", "--model_dir", os.path.join(tmp, "g")] + pre, "graph")
    ok1 = cmp(eager, graph, [(i, i) for i in range(4)], "graph vs eager, iters 0-3, same initial weights and batches")
    # --resume: lr 0 keeps the weights at their initial values, so the resumed iterations 2-3 (idx restarts at 0, batches 0-1)
    # must log what iterations 0-1 of a fresh eager run logged
    e0 = run(["--mode", mode, "--num_iterations", "2", "--save_interval", "2", "--lr", "0", "--model_dir", os.path.join(tmp, "r")], "eager lr0")
    res = run(["--mode", mode, "--num_iterations", "4", "--save_interval", "2", "--lr", "0", "--resume", "--model_dir", os.path.join(tmp, "r")], "resume lr0")
    ok2 = cmp(e0, res, [(0, 2), (1, 3)], "resume (iters 2-3) vs eager (iters 0-1), same batches")
    shutil.rmtree(tmp)
    sys.exit(0 if ok1 and ok2 else 2)


if __name__ == "__main__":
    main()
