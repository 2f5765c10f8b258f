#!/usr/bin/env python3
"""What a geometric term costs in the training step (B = 4, 256x832, geom mode, one GPU).

  python tools/geom_term_bench.py --term {triangle,eight_point,pnp,epipolar_8pf} [--steps 60] [--warmup 10] [--rounds 3] [--graph] [--kernels]

Three configurations of the same model and batch, timed in turn, ``--rounds`` times, the order rotating so that a drift of the
box hits them alike (as profiles/deterministic_mode.txt alternates its pairs):
  off     the step with the term's switch off (the switch changes nothing while it is off);
  fused   the step with the fused term (Model_geometry.<term>_term: selection, the term's kernels, the loss launch);
  torch   the step with the composition the tree had before the kernels, fed by the same matches:
          triangle     ``triangle_term_torch`` fed by ``GeometrySolvers.sample_match``, host sync included; eager only: it cannot
                       be captured, and ``--graph`` does not try;
          eight_point  ``compute_eight_point_loss`` per direction (the same selection and draw, gathered in torch): its minimal
                       sets drawn on the host and uploaded every call, ``eigh`` / ``svd`` over 2 x B x 256 hypotheses,
                       ``torch.inverse``;
          pnp          ``compute_pnp_loss`` per direction: ``svd`` over 2 x B x 256 systems of 12x12, a [B,256,num,3] float64
                       temporary per direction, 30 rounds of ``torch.linalg.solve`` (which raises on a singular system: the
                       composition is then left out with a line);
          epipolar_8pf ``compute_epipolar_map_8pF`` per direction on the step's matches (``compute_fundmental_mat`` as for
                       eight_point, then the dense map in torch: a bmm over [b,3,H*W] and a dozen elementwise kernels with
                       their autograd) and ``compute_epipolar_loss``; the fused RANSAC is not run beside it.
``--graph`` times off / fused as GraphedTrainStep replays, and tries the composition too: if its capture is refused the line
says so.  One window = ``--steps`` steps after ``--warmup``, the device synchronised before and after; ms/step is the window's
wall time over its steps.  The requirement is (fused - off) below (torch - off) by more than the run-to-run spread of off; the
script prints the medians, the spreads and that verdict.  ``--kernels`` (a run of its own: the profiler slows the host) prints
the device time of the term's launches in one fused step; for epipolar_8pf also the achieved bytes/s of the two dense kernels
against their shape-derived byte counts, and the part of the term that is dfe_fundamental_ransac (k_ep_*; paid once when
``enable_eight_point`` is on as well).

The tool sets no time limit of its own: run it under ``timeout``, each mode as a process of its own.  It replaces
tools/triangle_bench.py, tools/eight_point_bench.py and tools/pnp_bench.py, which profiles/*_term.txt cite."""
import argparse
import os
import re
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unsupervised_depth_opticalflow_egomotion_amd import ops, synthetic                                   # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd.models import Model_geometry                            # noqa: E402
from unsupervised_depth_opticalflow_egomotion_amd.train_step import (GraphedTrainStep, make_cfg,          # noqa: E402
                                                                     make_optimizer, train_step)

B, H, W = 4, 256, 832


def step_matches(self, disp_t0, pose, flow_bwd0, flow_fwd0, K, draw):
    """Per direction (d, match [b,4,num], pix [b,num]): the step's own selection and draw, gathered in torch."""
    idx, pick = draw if draw is not None else self.geometric_draw(disp_t0, pose, flow_bwd0, flow_fwd0, K)
    b, _, h, w = flow_bwd0.shape
    for d, flow in enumerate((flow_bwd0, flow_fwd0)):
        pix = idx[d * b:(d + 1) * b].long()[:, pick]
        x, y = (pix % w).float(), torch.div(pix, w, rounding_mode="floor").float()
        uv = torch.gather(flow.detach().reshape(b, 2, h * w), 2, pix.unsqueeze(1).expand(-1, 2, -1))
        yield d, torch.stack([x, y, x + uv[:, 0], y + uv[:, 1]], 1), pix


class TriangleComposition(Model_geometry):
    """The term as the parent tree could have switched it on: sample_match (topk, a count read back to the host, a host-side
    randint) and compute_triangulate_loss, per direction."""

    def triangle_term(self, disp_l0, disp_t0, disp_r0, pose, flow_bwd0, flow_fwd0, K, K_inv, return_draw=False):
        loss = None
        for d, (flow, src) in enumerate(((flow_bwd0, disp_l0), (flow_fwd0, disp_r0))):
            with torch.no_grad():
                rigid = ops.RigidFlowFn.apply(disp_t0, pose[:, d].contiguous(), K)
                _, score = ops.dynamic_mask(flow, rigid, self.flow_consist_alpha, self.flow_consist_beta)
            match, _ = self.sample_match(flow, disp_t0, score)
            term = self.compute_triangulate_loss(match, pose[:, d].contiguous(), K, K_inv, [disp_t0], [src])
            loss = term if loss is None else loss + term
        return (loss, None, None) if return_draw else loss


class EightPointComposition(Model_geometry):
    """The term as the parent tree could have switched it on: compute_eight_point_loss per direction on the step's matches."""

    def step_fundamental(self, flow_bwd0, flow_fwd0, idx, pick):          # the fused RANSAC is not run beside the composition
        return None, torch.zeros(2 * flow_bwd0.shape[0], 3, 3, dtype=torch.float64, device=flow_bwd0.device)

    def eight_point_term(self, disp_t0, pose, flow_bwd0, flow_fwd0, K, K_inv, draw=None, return_F=False, F=None):
        b = flow_bwd0.shape[0]
        loss = None
        draw = draw if draw is not None else getattr(self, "triangle_draw", None)
        for d, match, _ in step_matches(self, disp_t0, pose, flow_bwd0, flow_fwd0, K, draw):
            term = self.compute_eight_point_loss(match, pose[:, d].contiguous(), K, K_inv).reshape(1).expand(b)
            loss = term if loss is None else loss + term
        return (loss, torch.zeros(2 * b, 3, 3, dtype=torch.float64, device=flow_bwd0.device)) if return_F else loss


class PnpComposition(Model_geometry):
    """The term as the parent tree could have switched it on: compute_pnp_loss per direction on the step's matches."""

    def pnp_term(self, disp_t0, pose, flow_bwd0, flow_fwd0, K, K_inv, draw=None, return_pose=False):
        b, _, h, w = flow_bwd0.shape
        loss = None
        for d, match, pix in step_matches(self, disp_t0, pose, flow_bwd0, flow_fwd0, K, draw):
            depth = torch.gather(disp_t0.detach().reshape(b, 1, h * w), 2, pix.unsqueeze(1))
            term = self.compute_pnp_loss(depth, match, pose[:, d].contiguous(), K, K_inv).mean(1)
            loss = term if loss is None else loss + term
        return (loss, torch.zeros(2 * b, 6, dtype=torch.float64, device=flow_bwd0.device)) if return_pose else loss


class EpipolarComposition(Model_geometry):
    """The term in plain torch: compute_epipolar_map_8pF per direction on the step's matches, then the plain mean."""

    def step_fundamental(self, flow_bwd0, flow_fwd0, idx, pick):
        return None, torch.zeros(2 * flow_bwd0.shape[0], 3, 3, dtype=torch.float64, device=flow_bwd0.device)

    def epipolar_8pf_term(self, disp_t0, pose, flow_bwd0, flow_fwd0, K, draw=None, F=None):
        loss = None
        draw = draw if draw is not None else getattr(self, "triangle_draw", None)
        for d, match, _ in step_matches(self, disp_t0, pose, flow_bwd0, flow_fwd0, K, draw):
            dist = self.compute_epipolar_map_8pF(match, pose[:, d].contiguous(), (flow_bwd0, flow_fwd0)[d], K, None)
            term = self.compute_epipolar_loss(dist, None)
            loss = term if loss is None else loss + term
        return loss


def epipolar_bytes():
    """Shape-derived traffic of the two dense kernels at (B, H, W): the forward pass reads two flow planes per plane and writes one
    double per block; the backward pass reads them again and writes two gradient planes per plane."""
    planes = 2 * B * 2 * H * W * 4
    return {"k_epi_loss_part": planes, "k_epi_bwd": 2 * planes}


# term -> (the switch and what goes with it, the torch composition, the fused kernels' names, whether --graph tries the composition)
TERMS = {
    "triangle": (dict(enable_triangle=True, w_triangle=0.001), TriangleComposition, r"k_tri_\w+|k_topk_select", False),
    "eight_point": (dict(enable_eight_point=True), EightPointComposition, r"k_ep_\w+|k_topk_select", True),
    "pnp": (dict(enable_pnp=True), PnpComposition, r"k_pnp_\w+|k_topk_select", True),
    "epipolar_8pf": (dict(enable_epipolar_8pf=True), EpipolarComposition, r"k_epi_\w+|k_ep_\w+|k_topk_select", True),
}


def build(term, kind, graph):
    switches, composition = TERMS[term][:2]
    switches = {k: (v if k.startswith("w_") else kind != "off") for k, v in switches.items()}
    cfg = make_cfg(num_scales=3, img_hw=(H, W), mode="geom", **switches)
    torch.manual_seed(0)
    model = (composition if kind == "torch" else Model_geometry)(cfg).cuda().train()
    opt = make_optimizer(model, 1e-4, capturable=graph)
    inputs = [torch.from_numpy(a).cuda() for a in synthetic.make_triplet_batch(B, H, W, 3, seed=1)]
    if graph:
        g = GraphedTrainStep(model, opt, inputs, cfg, warmup=3)
        return lambda: g(inputs)
    return lambda: train_step(model, opt, inputs, cfg)


def window(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def kernel_times(fn, pattern):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    rows = {}
    for e in prof.events():
        m = re.search(pattern, e.name)
        if e.device_type == torch.autograd.DeviceType.CUDA and m:
            rows.setdefault(m.group(0), []).append(e.device_time if hasattr(e, "device_time") else e.cuda_time)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--term", choices=sorted(TERMS), required=True)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geom_term_bench.py needs a HIP device: a timing from anywhere else says nothing")
    pattern, torch_under_graph = TERMS[args.term][2:]
    kinds = ("off", "fused") if args.kernels or (args.graph and not torch_under_graph) else ("off", "fused", "torch")
    fns = {}
    for k in kinds:
        try:
            fns[k] = build(args.term, k, args.graph)
        except Exception as e:                                    # noqa: BLE001  (the composition under capture)
            if k != "torch" or not args.graph:
                raise
            print("torch  cannot be captured: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:160]))
    for k in tuple(fns):
        try:
            for _ in range(args.warmup):
                fns[k]()
            torch.cuda.synchronize()
        except Exception as e:                                    # noqa: BLE001  (torch.linalg.solve raises on a singular system)
            if k != "torch":
                raise
            del fns[k]
            print("torch  failed in its warm-up and is left out: %s: %s" % (type(e).__name__, str(e).splitlines()[0][:160]))
    kinds = tuple(k for k in kinds if k in fns)
    print("# %s, B = %d, %dx%d, geom, %s, %d steps per window after %d warm-up steps, %d rounds"
          % (torch.cuda.get_device_name(0), B, H, W, "graph replay" if args.graph else "eager", args.steps, args.warmup, args.rounds))
    if args.kernels:
        times = kernel_times(fns["fused"], pattern)
        for name, us in sorted(times.items()):
            print("kernel %-22s launches %d  device time %8.1f us" % (name, len(us), sum(us)))
        if args.term == "epipolar_8pf":
            for name, nbytes in epipolar_bytes().items():
                us = sum(times[name])
                print("dense  %-22s %.2f MB by shape in %.1f us = %.2f TB/s" % (name, nbytes / 1e6, us, nbytes / us / 1e6))
            ransac = sum(sum(v) for k, v in times.items() if k.startswith("k_ep_"))
            dense = sum(sum(v) for k, v in times.items() if k.startswith("k_epi_"))
            print("term   dfe_fundamental_ransac (k_ep_*) %.1f us; the map's kernels (k_epi_*) %.1f us; selection (k_topk_select) "
                  "%.1f us" % (ransac, dense, sum(times.get("k_topk_select", []))))
        return
    res = {k: [] for k in kinds}
    for r in range(args.rounds):
        order = kinds[r % len(kinds):] + kinds[:r % len(kinds)]
        for k in order:
            res[k].append(window(fns[k], args.steps))
            print("round %d %-6s ms_per_step %8.4f" % (r + 1, k, res[k][-1]), flush=True)
    med = {k: statistics.median(v) for k, v in res.items()}
    for k in kinds:
        print("median %-6s %8.4f ms (%.4f .. %.4f)" % (k, med[k], min(res[k]), max(res[k])))
    spread = max(res["off"]) - min(res["off"])
    print("fused - off = %+.4f ms; run-to-run spread of off = %.4f ms" % (med["fused"] - med["off"], spread))
    if "torch" in med:
        gain = (med["torch"] - med["off"]) - (med["fused"] - med["off"])
        print("torch - off = %+.4f ms; (torch - off) - (fused - off) = %.4f ms: %s" % (
            med["torch"] - med["off"], gain, "above the spread" if gain > spread else "NOT above the spread"))


if __name__ == "__main__":
    main()
