"""``InferenceSession``: the models' inference entry points (``infer_depth`` / ``inference_flow`` / ``infer_pose``) as a forward-only
path that stays on this build's kernels in eval mode, computes only what it returns and can be replayed from a hipGraph.

* Inside a session call every ``FrameBatchNorm2d`` of the depth encoder is ONE streaming pass ``act(x * scale[c] + shift[c] [+ residual])``
  in place over the convolution's output (``ops.bn_eval``) with the running statistics folded into per-channel tables
  (``ops.bn_fold``), where the plain eval call runs ATen's batch norm, a residual add and a ReLU.  The tables are installed on the
  layers for the length of the call only and removed again: ``model.infer_depth(...)`` called directly keeps its ATen branch and
  runs the kernels it ran before (the same bits in the deterministic mode; in the default mode MIOpen's convolutions repeat to
  rounding only, with or without a session).
* ``infer_depth`` launches the scale-0 disparity head alone (``DepthDecoder.forward_fused(scales=(0,))``).
* ``graph=True``: per (method, input shapes, deterministic mode, align_corners) the call is warmed up eagerly on a side stream,
  captured once on a single stream and replayed: inputs are copied into static buffers, the results returned as clones of the
  static outputs.

Weights may change between calls.  The session records the autograd version counter of every parameter and buffer of the nets it
runs; when any of them moved it folds the BatchNorm tables again IN PLACE (same device buffers), refreshes the Winograd filter cache,
drops every captured graph and captures again on the next call.  A captured Winograd launch reads the cache's transformed filters
(the U buffers) by address, and the cache re-transforms on a version miss and may allocate new buffers when a parameter is
registered again: the session holds a reference to every U buffer that existed when a graph was captured for as long as that graph
lives, and never replays across a version change.  (The cache's device tables, which train_step.GraphedTrainStep holds, are read by
``refresh`` alone, which no inference graph captures.)

Writers that bypass the version counters -- ``optim.FusedAdam`` and a replayed ``GraphedTrainStep`` write through raw pointers:
* the convolution weights need nothing: a replay reads them by address, and ``FusedAdam.step`` re-transforms the cached U buffers
  in place, so a ``Model_flow`` session (no BatchNorm, no folded table) replays on fresh data after any optimiser step;
* the folded BatchNorm tables do: an eager training step of a model with a depth encoder is seen (its BatchNorm layers bump
  ``num_batches_tracked``), a replayed ``GraphedTrainStep`` or ``p.data`` surgery is not -- call ``session.invalidate()`` after it.

Measured against the plain eval call: profiles/inference_session.txt (tools/infer_bench.py)."""
import functools

import torch

from . import convs, ops
from ._lib import DfeError
from .networks.resnet import FrameBatchNorm2d

METHODS = ("infer_depth", "inference_flow", "infer_pose")
_NETS = ("depth_net", "pose_net", "fpyramid", "pwc_model")


class _Captured:
    """One captured call: the graph, its static inputs and outputs, and the Winograd cache buffers its launches read by address."""

    def __init__(self, graph, inputs, outputs, held):
        self.graph, self.inputs, self.outputs, self.held = graph, inputs, outputs, held


class InferenceSession:
    """``InferenceSession(model, graph=False, warmup=2)`` for a ``Model_geometry`` / ``Model_depth`` / ``Model_flow`` in eval mode on a
    HIP device.  It has the inference methods the model has, with their signatures and return values; everything runs under
    ``torch.no_grad()``.  ``stats()``: how many times the tables were folded, calls captured and graphs replayed."""

    def __init__(self, model, graph=False, warmup=2):
        nets = [getattr(model, n) for n in _NETS if isinstance(getattr(model, n, None), torch.nn.Module)]
        if not nets or not any(hasattr(model, m) for m in METHODS):
            raise ValueError("InferenceSession: %s has none of the networks / methods %s" % (type(model).__name__, ", ".join(METHODS)))
        if model.training:
            raise ValueError("InferenceSession: the model is in training mode; call model.eval() first")
        tracked = [t for net in nets for t in list(net.parameters()) + list(net.buffers())]
        if not all(t.is_cuda for t in tracked):
            raise DfeError("InferenceSession: the model must be on a HIP device (there is no CPU fallback in the product path)")
        if graph and not ops.wino_weights.enabled:
            raise DfeError("InferenceSession(graph=True) needs the Winograd filter cache (DFE_WINO_CACHE=0 is set): without it the fused "
                           "Winograd layers transform their filters per call through a host copy, which cannot be captured")
        self.model, self.graph, self.warmup = model, bool(graph), max(int(warmup), 1)
        self._tracked = tracked
        depth_net = getattr(model, "depth_net", None)
        self._bns = [m for m in depth_net.encoder.modules() if isinstance(m, FrameBatchNorm2d)] if depth_net is not None else []
        self._tables = [None] * len(self._bns)
        self._versions = None
        self._graphs = {}
        self._stats = {"folds": 0, "captures": 0, "replays": 0}

    def __getattr__(self, name):
        if name in METHODS and hasattr(self.__dict__.get("model"), name):
            return functools.partial(self._call, name)
        raise AttributeError("%s has no attribute %r" % (type(self).__name__, name))

    def stats(self):
        return dict(self._stats)

    def invalidate(self):
        """Call after a write to the model that bumps no version counter (optim.FusedAdam.step, a replayed GraphedTrainStep,
        ``p.data`` surgery): the next call folds and captures again."""
        self._versions = None

    # ---- the state a call depends on
    def _sync(self):
        versions = [t._version for t in self._tracked]
        if versions == self._versions:
            return
        if self._graphs:               # no replay is in flight when its graph and the graph's memory pool are released
            torch.cuda.synchronize()
        self._graphs.clear()           # before anything they read is rewritten; captured again on the next call of each method
        for i, m in enumerate(self._bns):
            self._tables[i] = ops.bn_fold(m, out=self._tables[i])
        self._stats["folds"] += 1
        # in-place writes made every registered filter's cache entry miss; one launch re-transforms them (filters first seen later are
        # transformed per call until the next refresh -- a capture refreshes once more behind its warm-up)
        ops.wino_weights.invalidate()
        ops.wino_weights.refresh()
        self._versions = versions

    # ---- one call
    def _run(self, name, args):
        if name != "infer_depth":
            return getattr(self.model, name)(*args)
        net = self.model.depth_net
        for m, t in zip(self._bns, self._tables):
            m.folded = t
        try:
            disp = net.decoder.forward_fused(net.encoder(args[0]), scales=(0,))[0]
        finally:
            for m in self._bns:
                m.__dict__.pop("folded", None)      # back to the class attribute: nothing is left on the layer
        return self.model.disp2depth(disp)

    def _capture(self, name, args):
        inputs = [a.clone() for a in args]
        main = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(main)
        with torch.cuda.stream(side):      # allocator, MIOpen's solver choice, the Winograd cache's registrations
            for _ in range(self.warmup):
                self._run(name, inputs)
        main.wait_stream(side)
        torch.cuda.synchronize()
        ops.wino_weights.refresh()         # every filter the warm-up registered is cached now: no capture-time transform (it copies from the host)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):      # one stream: the inference methods have no parallel branches
            outputs = self._run(name, inputs)
        held = [e["U"] for e in ops.wino_weights.entries.values()]      # what the captured Winograd launches read by address
        self._stats["captures"] += 1
        return _Captured(graph, inputs, outputs, held)

    def _call(self, name, *args):
        if self.model.training:
            raise ValueError("InferenceSession.%s: the model is in training mode; call model.eval() first" % name)
        for a in args:
            if not isinstance(a, torch.Tensor) or not a.is_cuda:
                raise DfeError("InferenceSession.%s takes tensors on a HIP device (there is no CPU fallback in the product path)" % name)
        with torch.no_grad():
            self._sync()
            if not self.graph:
                return self._run(name, args)
            # the kernels a capture recorded follow the deterministic mode, the warps the grid_sample convention
            key = (name, convs.DETERMINISTIC, ops.get_align_corners()) + tuple((tuple(a.shape), a.dtype) for a in args)
            cap = self._graphs.get(key)
            if cap is None:
                cap = self._graphs[key] = self._capture(name, args)
            for dst, src in zip(cap.inputs, args):
                dst.copy_(src, non_blocking=True)
            cap.graph.replay()
            self._stats["replays"] += 1
            return cap.outputs.clone()           # each of the three methods returns one tensor
