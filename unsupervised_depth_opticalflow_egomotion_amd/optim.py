"""The optimiser of the reference's training loop -- ``torch.optim.Adam(model.parameters(), lr)`` (train.py:85-87) -- as
one HIP launch per step (csrc/ops_adam.hip).

``FusedAdam`` keeps ``torch.optim.Adam``'s hyper-parameters, update rule and state layout (``step``, ``exp_avg``,
``exp_avg_sq`` per parameter; the same ``param_groups`` keys), so a checkpoint written by one loads into the other
(train.py:90-94 resumes from ``optimizer.state_dict()``).  What changes is how the update reaches the GPU: ATen's fused
multi-tensor kernel takes its pointer tables as kernel arguments -- six launches of ~48 us for this model's ~250 tensors,
on the serial tail of the step -- here the tables are device tensors (the gradient pointers are refreshed each step, the
rest is built once) and one launch updates everything.

Two options the reference does not have, both off by default, run inside the step on the device: global-norm gradient
clipping (``max_grad_norm``) and skipping a step whose gradients are not finite (``skip_nonfinite``); see ``FusedAdam``.

fp32 parameters on one HIP device, dense gradients, no weight decay / amsgrad / maximize (the reference uses none);
anything else raises."""
import ctypes

import torch

from . import ops
from ._lib import check, get_lib, stream_ptr


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, capturable=False, max_grad_norm=None,
                 skip_nonfinite=False):
        """``capturable``: the step count lives on the device (dfe_adam_step_dev), so that a whole training step -- this
        ``step()`` included -- can be captured in a hipGraph and replayed (train_step.GraphedTrainStep, train.py --graph);
        ``state_dict()`` reads the count back.  All parameters of a group must then step together.

        The gradient guard (both off by default; with both off ``step()`` is what it always was), decided on the device
        inside ``step()`` -- behind a data-parallel reducer's step pre-hook, capturable in a hipGraph, no host read:
        ``max_grad_norm`` (a float > 0): ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` -- ONE 2-norm over every
        parameter that has a gradient, across param groups; c = min(1, max_norm / (norm + 1e-6)) and the update uses
        g * c.  The gradients themselves are never written: ``p.grad`` read after the step is the UNCLIPPED gradient.
        ``skip_nonfinite``: a step with a NaN or +-inf gradient element is not applied -- every parameter and moment keeps
        its bits, the step count does not advance, ``guard_stats()["skipped_steps"]`` goes up by one (GradScaler's
        behaviour without the scaling).  With clipping on and ``skip_nonfinite`` off such a step goes through torch's
        formula unchanged: c = 0 for an inf norm, NaN for a NaN norm.
        Both are attributes of the optimiser, not keys of ``param_groups`` or of ``state_dict()`` (which stays
        torch.optim.Adam's): like ``capturable`` they say how this process steps.  With either on, the step count of every
        group lives on the device (the host cannot know whether it advanced) and all parameters of a group must step
        together."""
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (0.0 < max_grad_norm < float("inf")):
                raise ValueError("max_grad_norm must be a finite float above 0 or None, got %r" % max_grad_norm)
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False, foreach=None,
                        capturable=bool(capturable), differentiable=False, fused=None)
        super().__init__(params, defaults)
        self._plans = {}
        self._dev_count = {}          # capturable groups: group index -> (step count [1] float64, coefficients [2] float32) on the device
        # what a captured step (hipGraph) reads by ADDRESS: plans (table, block map, its own pinned pointer table) and the
        # device counts.  Held for the optimiser's lifetime, so that a replay can never read freed memory; ``capture_epoch``
        # moves whenever they stop being the live ones (load_state_dict) and GraphedTrainStep refuses to replay across that.
        self._captured = []
        self.capture_epoch = 0
        self._guard_rec = None        # the guard's device record (32 bytes as 4 float64: include/dfe_hip.h), made by the first guarded step

    MAX_PLANS = 8

    def state_dict(self):
        """As torch.optim.Adam's.  Inside this optimiser the parameters of a group share ONE step-count tensor (one
        increment per step instead of ~250); a checkpoint must not carry that sharing -- torch.optim.Adam increments
        every parameter's count, i.e. a shared one once per parameter -- so every entry gets its own copy here."""
        for gi, (count, _) in self._dev_count.items():      # capturable: the count advanced on the device (graph replays)
            t = float(count.cpu()[0])
            for p in self.param_groups[gi]["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    st["step"] = torch.tensor(t, dtype=torch.float32)
        sd = super().state_dict()
        sd["state"] = {k: ({**v, "step": v["step"].clone()} if "step" in v else v) for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        """As torch.optim.Adam's, except that ``capturable`` stays what the constructor was given: it says how THIS
        process steps (train.py --graph or not), not what the moments are, and a checkpoint written in either mode -- or by
        the reference's torch.optim.Adam -- loads into either.  torch would overwrite the flag with the checkpoint's along
        with lr / betas / eps (which are still taken from it), and, where the checkpoint says capturable, move every
        ``step`` to the device; here the counts always live on the host as float32 scalars (step() reads them per
        parameter; the device count of a capturable group is seeded from them)."""
        mine = [bool(g["capturable"]) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, c in zip(self.param_groups, mine):
            g["capturable"] = c
        for st in self.state.values():
            if "step" in st:
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
        self._plans = {}                       # the moment tensors were replaced
        self._dev_count = {}                   # re-seeded from the loaded counts at the next step
        if self._captured:
            self.capture_epoch += 1            # a graph captured before this point updates the OLD moments: re-capture

    def _fingerprint(self, params):
        """Cheap check that the cached parameter / moment pointers are still the live ones."""
        a, b = params[0], params[-1]
        return (a.data_ptr(), b.data_ptr(), self.state[a]["exp_avg"].data_ptr(), self.state[b]["exp_avg_sq"].data_ptr())

    # ------------------------------------------------------------------ tables
    def _plan(self, gi, params):
        """Static part of the launch for one param group and one set of parameters that have gradients."""
        key = (gi, tuple(id(p) for p in params))
        plan = self._plans.get(key)
        if plan is not None and plan["fingerprint"] == self._fingerprint(params):
            return plan
        lib = get_lib()
        chunk = lib.dfe_adam_chunk()
        dev = params[0].device
        rows, blocks = [], []
        for t, p in enumerate(params):
            st = self.state[p]
            rows.append([p.data_ptr(), 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()])
            blocks += [[t, c] for c in range((p.numel() + chunk - 1) // chunk)]
        # the pointer table reaches the device through a small ring of pinned buffers (an un-pinned source would make the
        # copy synchronise the stream, i.e. stall the host once per step); a buffer is reused only after its copy ran
        plan = {"host": torch.tensor(rows, dtype=torch.int64),
                "pinned": [torch.empty(len(rows), 5, dtype=torch.int64).pin_memory() for _ in range(4)],
                # the captured step's own source buffer (see step()): allocated here, pinning memory is not capturable
                "graph_pinned": torch.empty(len(rows), 5, dtype=torch.int64).pin_memory(),
                "events": [None] * 4, "turn": 0,
                "table": torch.empty(len(rows), 5, dtype=torch.int64, device=dev),
                "blockmap": torch.tensor(blocks, dtype=torch.int32).to(dev), "nblocks": len(blocks),
                "fingerprint": self._fingerprint(params)}
        # a group normally has ONE live plan; parameters that got their first gradient at different steps need one per
        # distinct count.  Plans are keyed by (group, parameter ids) only -- never by the count, which changes every
        # step -- and a group keeps at most MAX_PLANS of them (oldest dropped: pinned buffers, table, block map).
        mine = [k for k in self._plans if k[0] == gi]
        for k in mine[:max(0, len(mine) - (self.MAX_PLANS - 1))]:
            del self._plans[k]
        self._plans[key] = plan
        return plan

    def _collect(self, group):
        """The parameters of ``group`` that have a gradient and those gradients (contiguous), state created where missing."""
        if group.get("weight_decay", 0) or group.get("amsgrad") or group.get("maximize"):
            raise NotImplementedError("FusedAdam implements the reference's plain Adam (no weight decay / amsgrad / maximize)")
        params = [p for p in group["params"] if p.grad is not None]
        grads = []
        for p in params:
            g = p.grad
            if (g.is_sparse or g.dtype != torch.float32 or p.dtype != torch.float32 or not p.is_cuda or p.device != params[0].device
                    or not p.is_contiguous()):
                raise NotImplementedError("FusedAdam needs dense fp32 parameters and gradients on one HIP device")
            grads.append(g if g.is_contiguous() else g.contiguous())
            st = self.state[p]
            if not st:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return params, grads

    def _upload(self, plan, grads, capturing):
        """This step's gradient pointers into the plan's device table."""
        host = plan["host"]
        host[:, 1] = torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64)
        if capturing:
            # the graph's copy node re-reads its source on every replay: a pinned buffer of its OWN, outside the ring
            # the eager steps cycle through (an eager step after the capture would otherwise leave its gradient
            # pointers where the next replay picks them up)
            plan["graph_pinned"].copy_(host)
            plan["table"].copy_(plan["graph_pinned"], non_blocking=True)
            self._captured.append(plan)
        else:
            k = plan["turn"]
            plan["turn"] = (k + 1) % len(plan["pinned"])
            if plan["events"][k] is not None:
                plan["events"][k].synchronize()
            plan["pinned"][k].copy_(host)
            plan["table"].copy_(plan["pinned"][k], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            plan["events"][k] = ev

    def _count_on_device(self, gi, t0, dev, capturing):
        dc = self._dev_count.get(gi)
        if dc is None:      # seeded from the host count once; from then on the device count is the truth
            dc = self._dev_count[gi] = (torch.full((1,), t0, dtype=torch.float64, device=dev),
                                        torch.zeros(2, dtype=torch.float32, device=dev))
        if capturing:
            self._captured.append(dc)
        return dc

    def _advance_host_count(self, group, ps, t):
        first = self.state[ps[0]]["step"]
        shared = all(self.state[p]["step"] is first for p in ps)
        if shared:
            # torch.optim.Adam counts per parameter: one that holds the shared tensor but sits this launch out
            # (no gradient this step) keeps its count on a copy of its own
            if len(ps) != len(group["params"]):
                inside = {id(p) for p in ps}
                for q in group["params"]:
                    sq = self.state.get(q)
                    if sq and sq.get("step") is first and id(q) not in inside:
                        sq["step"] = first.clone()
            first += 1.0                    # one CPU tensor shared by the launch's parameters
        else:
            new = torch.tensor(t, dtype=torch.float32)
            for p in ps:
                self.state[p]["step"] = new

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.max_grad_norm is not None or self.skip_nonfinite:
            self._step_guarded()
            ops.wino_weights.refresh()      # after a skipped step too: the parameters did not change, the rebuild is harmless
            return loss
        lib = get_lib()
        for gi, group in enumerate(self.param_groups):
            params, grads = self._collect(group)
            if not params:
                continue
            dev = params[0].device
            # parameters of a group that stepped together share their count: one launch per distinct count
            by_step = {}
            for p, g in zip(params, grads):
                by_step.setdefault(float(self.state[p]["step"]), []).append((p, g))
            for t0, pg in by_step.items():
                ps = [p for p, _ in pg]
                plan = self._plan(gi, ps)
                capturing = torch.cuda.is_current_stream_capturing()
                self._upload(plan, [g for _, g in pg], capturing)
                t = t0 + 1.0
                b1, b2 = group["betas"]
                if group.get("capturable"):
                    if len(by_step) != 1:
                        raise NotImplementedError("FusedAdam(capturable=True): all parameters of a group must step together")
                    dc = self._count_on_device(gi, t0, dev, capturing)
                    check(lib.dfe_adam_step_dev(ctypes.c_void_p(plan["table"].data_ptr()), ctypes.c_void_p(plan["blockmap"].data_ptr()),
                                                plan["nblocks"], float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                                ctypes.c_void_p(dc[0].data_ptr()), ctypes.c_void_p(dc[1].data_ptr()), stream_ptr()),
                          "dfe_adam_step_dev")
                else:
                    check(lib.dfe_adam_step(ctypes.c_void_p(plan["table"].data_ptr()), ctypes.c_void_p(plan["blockmap"].data_ptr()),
                                            plan["nblocks"], float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                            1.0 - b1 ** t, 1.0 - b2 ** t, stream_ptr()), "dfe_adam_step")
                self._advance_host_count(group, ps, t)
        # the parameters changed behind autograd's back (raw pointers, no version bump): the Winograd kernel's cached
        # transformed filters are rebuilt here, in one launch on this stream, right behind the update
        ops.wino_weights.refresh()
        return loss

    # ------------------------------------------------------------------ the guarded step
    def _step_guarded(self):
        """dfe_grad_guard over ONE table that holds every group's parameters (one global norm, one upload), then one
        dfe_adam_step_guarded per group on its rows of that table.  The finisher advances the first group's device count;
        every further group's advances in a one-thread launch of its own that reads the same decision."""
        lib = get_lib()
        live = []                                           # (group index, group, parameters, count before the step)
        params, grads = [], []
        for gi, group in enumerate(self.param_groups):
            ps, gs = self._collect(group)
            if not ps:
                continue
            if len({float(self.state[p]["step"]) for p in ps}) != 1:
                raise NotImplementedError("FusedAdam(max_grad_norm / skip_nonfinite): all parameters of a group must step together")
            live.append((gi, group, ps, float(self.state[ps[0]]["step"])))
            params += ps
            grads += gs
        if not params:
            return
        dev = params[0].device
        if any(p.device != dev for p in params):
            raise NotImplementedError("FusedAdam needs dense fp32 parameters and gradients on one HIP device")
        plan = self._plan(-1, params)                       # key -1: the table across the groups
        guard = plan.get("guard")
        if guard is None:
            chunk = lib.dfe_adam_chunk()
            per_group, row = [], 0
            for gi, _, ps, _ in live:
                blocks = [[t, c] for t, p in enumerate(ps) for c in range((p.numel() + chunk - 1) // chunk)]
                per_group.append((gi, row, torch.tensor(blocks, dtype=torch.int32).to(dev), len(blocks)))
                row += len(ps)
            guard = plan["guard"] = {"groups": per_group,
                                     "ws": torch.empty((lib.dfe_grad_guard_ws_bytes(plan["nblocks"]) + 7) // 8, dtype=torch.float64, device=dev)}
        if [g[0] for g in guard["groups"]] != [l[0] for l in live]:
            raise NotImplementedError("FusedAdam(max_grad_norm / skip_nonfinite): all parameters of a group must step together")
        if self._guard_rec is None:
            assert lib.dfe_grad_guard_record_bytes() == 32
            self._guard_rec = torch.zeros(4, dtype=torch.float64, device=dev)
        capturing = torch.cuda.is_current_stream_capturing()
        self._upload(plan, grads, capturing)
        if capturing:
            self._captured.append(self._guard_rec)
        rec = ctypes.c_void_p(self._guard_rec.data_ptr())
        counts = [self._count_on_device(gi, t0, dev, capturing) for gi, _, _, t0 in live]
        for k, ((gi, group, ps, t0), dc) in enumerate(zip(live, counts)):
            b1, b2 = group["betas"]
            if k == 0:
                check(lib.dfe_grad_guard(ctypes.c_void_p(plan["table"].data_ptr()), ctypes.c_void_p(plan["blockmap"].data_ptr()),
                                         plan["nblocks"], float(self.max_grad_norm or 0.0), int(self.skip_nonfinite), float(group["lr"]),
                                         float(b1), float(b2), ctypes.c_void_p(guard["ws"].data_ptr()), ctypes.c_void_p(dc[0].data_ptr()),
                                         ctypes.c_void_p(dc[1].data_ptr()), rec, stream_ptr()), "dfe_grad_guard")
            else:
                check(lib.dfe_adam_tick_guarded(float(group["lr"]), float(b1), float(b2), ctypes.c_void_p(dc[0].data_ptr()),
                                                ctypes.c_void_p(dc[1].data_ptr()), rec, stream_ptr()), "dfe_adam_tick_guarded")
        for (gi, group, ps, t0), dc, (_, row, blockmap, nblocks) in zip(live, counts, guard["groups"]):
            b1, b2 = group["betas"]
            check(lib.dfe_adam_step_guarded(ctypes.c_void_p(plan["table"].data_ptr() + 40 * row), ctypes.c_void_p(blockmap.data_ptr()),
                                            nblocks, float(b1), float(b2), float(group["eps"]), ctypes.c_void_p(dc[1].data_ptr()), rec,
                                            stream_ptr()), "dfe_adam_step_guarded")
            # the host's count runs ahead of the device's after a skipped step: state_dict() reads the device's back
            self._advance_host_count(group, ps, t0 + 1.0)

    def guard_stats(self):
        """``{"grad_norm", "clip_coef", "finite", "skipped_steps"}`` of the last guarded step (``skipped_steps`` since the
        optimiser was made).  One 32-byte device-to-host copy that synchronises: call it at log intervals only."""
        if self.max_grad_norm is None and not self.skip_nonfinite:
            raise ValueError("FusedAdam.guard_stats(): neither max_grad_norm nor skip_nonfinite is on")
        if self._guard_rec is None:
            return {"grad_norm": 0.0, "clip_coef": 1.0, "finite": True, "skipped_steps": 0}
        rec = self._guard_rec.cpu().numpy()
        return {"grad_norm": float(rec[0]), "clip_coef": float(rec.view("float32")[4]), "finite": bool(rec.view("int32")[5]),
                "skipped_steps": int(rec[1])}
