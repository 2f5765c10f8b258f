"""KITTI evaluation from device-resident sets: what ``train.py`` runs every ``--test_interval`` iterations and ``test.py
--fused_eval`` runs once.

``FlowEvalSet`` / ``DepthEvalSet`` hold a task's prepared network inputs and its ground truth on the device for their whole life:
KITTI's frames differ in size (370-376 x 1224-1242), so the ground truth lies in planes padded to ``[N, Hmax, Wmax]`` (``Wmax`` a
multiple of 4: the kernels read it 16 bytes at a time) beside an int table of each sample's ``H, W`` -- for depth also the Eigen
crop box ``y0, y1, x0, x1``, computed as evaluate_depth.py does (float64 products truncated by ``astype(int32)``).  A flow set
holds ``u`` and ``v`` as fp32 planes and ``valid`` / ``noc`` / ``moving`` as bits of one byte plane; a depth set one fp32 plane.
The files are read and the inputs prepared exactly as ``test.py``'s per-image tasks do (``kitti_io.KITTIFlowPairs``,
``load_gt_flow_kitti``, ``load_gt_mask``, ``read_image_bgr``, ``resize_bilinear_u8``, ``/ 255``): the nets see the same bits.

``Evaluator.run()`` runs ``inference_flow`` / ``infer_depth`` over each set in batches through an ``inference.InferenceSession``
and enqueues the metric kernels (``dfe_eval_flow`` / ``dfe_eval_depth``, csrc/ops_eval.hip) behind each batch on the current
stream: a batch of predictions at the training size becomes the reference's per-sample sums with no host read, and each task is
read back once, at its end.  ``eval_flow_records`` / ``flow_table`` / ``eval_depth_records`` are the launchers alone, for callers
that hold predictions already.

What is pinned: the metric arithmetic against ``oracle/eval_oracle.py`` (tests/test_hip_eval_device.py).  What is not: the
reference resizes the network inputs and the predictions with cv2, which does not exist here; ``kitti_io.resize_bilinear_u8``
and the kernels' resize state its published definition (as ``test.py`` already does)."""
import ctypes
import os

import numpy as np
import torch

from . import kitti_io
from ._lib import DfeError, check, get_lib, stream_ptr

FLAG_VALID, FLAG_NOC, FLAG_MOVING = 1, 2, 4
TASKS_BY_MODE = {"flow": ("flow_2012", "flow_2015"), "depth": ("depth",), "geom": ("flow_2012", "flow_2015", "depth")}
RESULT_KEYS = {"flow_2012": "eval_2012_res", "flow_2015": "eval_2015_res", "depth": "eval_eigen_res"}
MIN_DEPTH, MAX_DEPTH = 1e-3, 80.0


def tasks_for_mode(mode):
    """The reference's tasks by training mode (train.py:142-155): flow -> 2012 + 2015, depth -> Eigen, geom -> all three."""
    if mode not in TASKS_BY_MODE:
        raise ValueError("Mode {} not found.".format(mode))
    return TASKS_BY_MODE[mode]


def crop_box(h, w):
    """evaluate_depth.py:27-28: the Eigen crop ``(y0, y1, x0, x1)`` of an ``h x w`` frame."""
    c = np.array([0.40810811 * h, 0.99189189 * h, 0.03594771 * w, 0.96405229 * w]).astype(np.int32)
    return int(c[0]), int(c[1]), int(c[2]), int(c[3])


def _binary(a, what, i):
    a = np.asarray(a)
    if not np.all((a == 0) | (a == 1)):
        raise ValueError("sample %d: the %s mask holds values other than 0 and 1" % (i, what))
    return a.astype(np.uint8)


def pack_flags(valid, noc, moving=None, sample=0):
    """{0,1} masks -> one byte plane: bit 0 valid, bit 1 noc, bit 2 moving."""
    f = _binary(valid, "valid", sample) * FLAG_VALID + _binary(noc, "noc", sample) * FLAG_NOC
    if moving is not None:
        f = f + _binary(moving, "moving", sample) * FLAG_MOVING
    return f.astype(np.uint8)


def unpack_flags(flags):
    f = np.asarray(flags)
    return tuple(((f & bit) != 0).astype(np.float32) for bit in (FLAG_VALID, FLAG_NOC, FLAG_MOVING))


def pad_planes(planes, dtype):
    """2-D arrays of differing sizes -> (``[N, Hmax, Wmax]`` zero-padded with ``Wmax`` a multiple of 4, ``[N, 2]`` int32 sizes)."""
    dims = np.array([p.shape for p in planes], np.int32).reshape(len(planes), 2)
    hmax, wmax = int(dims[:, 0].max()), (int(dims[:, 1].max()) + 3) // 4 * 4
    out = np.zeros((len(planes), hmax, wmax), dtype)
    for i, p in enumerate(planes):
        out[i, :p.shape[0], :p.shape[1]] = p
    return out, dims


def unpad_planes(padded, dims):
    return [np.asarray(padded[i, :h, :w]) for i, (h, w) in enumerate(np.asarray(dims)[:, :2])]


def pack_flow_gt(gt_flows, noc_masks, moving_masks=None):
    """``[H,W,3]`` (u, v, valid) maps + noc (+ moving) masks -> the host arrays of a flow set."""
    if len(gt_flows) == 0 or len(noc_masks) != len(gt_flows) or (moving_masks is not None and len(moving_masks) != len(gt_flows)):
        raise ValueError("a flow set needs as many noc (and moving) masks as ground-truth maps, and at least one")
    u, dims = pad_planes([np.asarray(g)[:, :, 0] for g in gt_flows], np.float32)
    v, _ = pad_planes([np.asarray(g)[:, :, 1] for g in gt_flows], np.float32)
    flags, _ = pad_planes([pack_flags(np.asarray(g)[:, :, 2], noc_masks[i], None if moving_masks is None else moving_masks[i], i)
                           for i, g in enumerate(gt_flows)], np.uint8)
    return {"u": u, "v": v, "flags": flags, "dims": dims}


def pack_depth_gt(gt_depths, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, names=None):
    """``[H,W]`` depth maps -> the host arrays of a depth set; a sample with nothing inside (min, max) and the crop raises."""
    if len(gt_depths) == 0:
        raise ValueError("a depth set needs at least one ground-truth map")
    gt, hw = pad_planes([np.asarray(g) for g in gt_depths], np.float32)
    dims = np.zeros((len(gt_depths), 6), np.int32)
    for i, (h, w) in enumerate(hw):
        y0, y1, x0, x1 = crop_box(int(h), int(w))
        dims[i] = (h, w, y0, y1, x0, x1)
        g = gt[i, y0:y1, x0:x1]
        if not np.any((g > np.float32(min_depth)) & (g < np.float32(max_depth))):
            raise ValueError("depth sample %s has no ground truth inside (%g, %g) and the crop box: its mask is empty"
                             % (names[i] if names is not None else i, min_depth, max_depth))
    return {"gt": gt, "dims": dims}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _count(dirname, suffix):
    return len([f for f in os.listdir(dirname) if f.endswith(suffix)]) if os.path.isdir(dirname) else 0


class FlowEvalSet:
    """``FlowEvalSet(gt_flows, noc_masks, moving_masks=None, inputs=None, device=None)``: ``inputs`` [N,3,2h,w], the two frames of
    each pair stacked along H as ``kitti_io.KITTIFlowPairs`` gives them (None: a set of ground truth alone, for the launchers)."""

    def __init__(self, gt_flows, noc_masks, moving_masks=None, inputs=None, device=None, name="flow"):
        host = pack_flow_gt(gt_flows, noc_masks, moving_masks)
        self.name, self.n, self.has_moving = name, len(gt_flows), moving_masks is not None
        self.hmax, self.wmax = host["u"].shape[1:]
        self.device = torch.device(device if device is not None else "cpu")
        self.u, self.v, self.flags, self.dims = (_dev(host[k], self.device) for k in ("u", "v", "flags", "dims"))
        if inputs is not None and len(inputs) != self.n:
            raise ValueError("%d inputs for %d ground-truth maps" % (len(inputs), self.n))
        self.inputs = None if inputs is None else torch.as_tensor(inputs).float().to(self.device).contiguous()

    def __len__(self):
        return self.n

    @classmethod
    def from_kitti(cls, gt_dir, img_hw, year, device=None):
        """The pairs and ground truth ``test.py --task kitti_flow_<year>`` reads (test.py:21-87), prepared once."""
        num = _count(os.path.join(gt_dir, "flow_occ"), "_10.png")
        if num == 0:
            raise FileNotFoundError("no flow_occ/*_10.png under %s" % gt_dir)
        gt_flows, noc_masks = kitti_io.load_gt_flow_kitti(gt_dir, "kitti_%d" % year, num)
        moving = kitti_io.load_gt_mask(gt_dir, num) if year == 2015 and os.path.isdir(os.path.join(gt_dir, "obj_map")) else None
        pairs = kitti_io.KITTIFlowPairs(gt_dir, img_hw, num, year)
        return cls(gt_flows, noc_masks, moving, torch.stack([pairs[i][0] for i in range(num)]), device, "kitti_%d" % year)


class DepthEvalSet:
    """``DepthEvalSet(gt_depths, inputs=None, device=None)``: ``inputs`` [N,3,h,w] prepared frames."""

    def __init__(self, gt_depths, inputs=None, device=None, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, names=None, name="eigen"):
        host = pack_depth_gt(gt_depths, min_depth, max_depth, names)
        self.name, self.n, self.min_depth, self.max_depth = name, len(gt_depths), float(min_depth), float(max_depth)
        self.hmax, self.wmax = host["gt"].shape[1:]
        self.device = torch.device(device if device is not None else "cpu")
        self.gt, self.dims = _dev(host["gt"], self.device), _dev(host["dims"], self.device)
        if inputs is not None and len(inputs) != self.n:
            raise ValueError("%d inputs for %d ground-truth maps" % (len(inputs), self.n))
        self.inputs = None if inputs is None else torch.as_tensor(inputs).float().to(self.device).contiguous()

    def __len__(self):
        return self.n

    @classmethod
    def from_eigen(cls, raw_base_dir, eigen_dir, img_hw, device=None):
        """The Eigen split ``test.py --task kitti_depth`` reads (test.py:104-135), prepared once."""
        listing, gt_file = os.path.join(eigen_dir, "test_files.txt"), os.path.join(eigen_dir, "gt_depths.npz")
        for f in (listing, gt_file):
            if not os.path.exists(f):
                raise FileNotFoundError("kitti_depth needs %s (Eigen split files of the reference's ./data/eigen)" % f)
        with open(listing) as fh:
            names = [ln.strip().split(" ") for ln in fh if ln.strip()]
        gt_depths = list(np.load(gt_file, allow_pickle=True)["data"])
        frames = []
        for path1, idx, _ in names:
            img = kitti_io.read_image_bgr(os.path.join(raw_base_dir, path1, "image_02/data/" + str(idx) + ".png"))
            frames.append(torch.from_numpy(kitti_io.resize_bilinear_u8(img, img_hw) / 255.0).float().permute(2, 0, 1))
        return cls(gt_depths, torch.stack(frames), device, names=["%s %s" % (n[0], n[1]) for n in names])


# ------------------------------------------------------------------------------------------------ the launchers
def _p(t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise DfeError("the evaluation kernels take tensors on a HIP device (there is no CPU fallback in the product path)")
    return ctypes.c_void_p(t.data_ptr())


def _pred(pred, channels):
    if not isinstance(pred, torch.Tensor) or pred.dim() != 4 or pred.shape[1] != channels or pred.dtype != torch.float32:
        raise DfeError("expected an fp32 prediction [n,%d,h,w]" % channels)
    return pred.contiguous()


def _nbytes(t):
    return t.numel() * t.element_size()


def _buffers(n, rec, ws_bytes, records, ws, device):
    if records is None:
        records = torch.empty((n, rec), dtype=torch.float64, device=device)
    elif _nbytes(records) < n * rec * 8 or not records.is_contiguous():
        raise DfeError("records: %d contiguous bytes needed" % (n * rec * 8))
    if ws is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    return records, ws


def eval_flow_records(fset, pred, first=0, records=None, ws=None):
    """``pred`` [n,2,h,w] for the set rows ``first .. first+n-1`` -> their records [n, 16] float64 (layout: include/dfe_hip.h),
    enqueued on the current stream.  ``records`` / ``ws``: the caller's buffers (any dtype; sizes in bytes as the header states)."""
    lib = get_lib()
    pred = _pred(pred, 2)
    n, _, h, w = pred.shape
    records, ws = _buffers(n, lib.dfe_eval_flow_record_doubles(), lib.dfe_eval_flow_ws_bytes(n), records, ws, pred.device)
    check(lib.dfe_eval_flow(_p(pred), n, h, w, _p(fset.u), _p(fset.v), _p(fset.flags), _p(fset.dims), fset.n, fset.hmax, fset.wmax,
                            int(first), _p(ws), _nbytes(ws), _p(records), stream_ptr()), "dfe_eval_flow")
    return records


def flow_table(records, has_moving, n=None):
    """The records of a whole task -> the eight table values [8] float64 on the device: epe, epe_noc, epe_occ, err_rate, epe_move,
    epe_static, move_err_rate, static_err_rate (``evaluation.eval_flow_avg``'s accumulator divided by the count)."""
    lib = get_lib()
    n = int(n if n is not None else _nbytes(records) // (8 * lib.dfe_eval_flow_record_doubles()))
    table = torch.empty(8, dtype=torch.float64, device=records.device)
    check(lib.dfe_eval_flow_finish(_p(records), n, int(bool(has_moving)), _p(table), stream_ptr()), "dfe_eval_flow_finish")
    return table


def eval_depth_records(dset, disp, first=0, records=None, ws=None):
    """``disp`` [n,1,h,w] (what ``infer_depth`` returns) for the set rows ``first .. first+n-1`` -> their records [n, 10] float64:
    abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3, median(gt[mask]), median(pred[mask]), the masked count."""
    lib = get_lib()
    disp = _pred(disp, 1)
    n, _, h, w = disp.shape
    records, ws = _buffers(n, lib.dfe_eval_depth_record_doubles(), lib.dfe_eval_depth_ws_bytes(n, dset.hmax, dset.wmax), records, ws,
                           disp.device)
    check(lib.dfe_eval_depth(_p(disp), n, h, w, _p(dset.gt), _p(dset.dims), dset.n, dset.hmax, dset.wmax, int(first), dset.min_depth,
                             dset.max_depth, _p(ws), _nbytes(ws), _p(records), stream_ptr()), "dfe_eval_depth")
    return records


def format_flow_table(values, has_moving):
    """``evaluation.eval_flow_avg``'s table string from its eight accumulated values."""
    error, error_noc, error_occ, error_rate, error_move, error_static, move_rate, static_rate = values
    if has_moving:
        result = "{:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10}, {:>10} \n".format(
            "epe", "epe_noc", "epe_occ", "epe_move", "epe_static", "move_err_rate", "static_err_rate", "err_rate")
        result += "{:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f}, {:10.4f} \n".format(
            error, error_noc, error_occ, error_move, error_static, move_rate, static_rate, error_rate)
        return result
    result = "{:>10}, {:>10}, {:>10}, {:>10} \n".format("epe", "epe_noc", "epe_occ", "err_rate")
    result += "{:10.4f}, {:10.4f}, {:10.4f}, {:10.4f} \n".format(error, error_noc, error_occ, error_rate)
    return result


# ------------------------------------------------------------------------------------------------ the evaluator
class Evaluator:
    """``Evaluator(model, cfg, flow_2012=None, flow_2015=None, depth=None, batch=4, session="eager")``; ``run()`` returns
    ``{"eval_2012_res": str, "eval_2015_res": str, "eval_eigen_res": [7 floats]}`` for the sets it was given, the strings formatted
    as ``evaluation.eval_flow_avg`` formats them.  ``session``: "eager" or "graph" (``InferenceSession(graph=True)``)."""

    def __init__(self, model, cfg, flow_2012=None, flow_2015=None, depth=None, batch=4, session="eager"):
        if session not in ("eager", "graph"):
            raise ValueError("session must be 'eager' or 'graph'")
        self.sets = {k: s for k, s in (("flow_2012", flow_2012), ("flow_2015", flow_2015), ("depth", depth)) if s is not None}
        if not self.sets:
            raise ValueError("Evaluator: no evaluation set given")
        for task, s in self.sets.items():
            method = "infer_depth" if task == "depth" else "inference_flow"
            if not hasattr(model, method):
                raise ValueError("Evaluator: %s has no %s for the task %s" % (type(model).__name__, method, task))
            if s.inputs is None or not s.inputs.is_cuda:
                raise DfeError("Evaluator: the set %s needs prepared inputs on a HIP device" % s.name)
        self.model, self.cfg, self.batch, self.graph = model, cfg, max(int(batch), 1), session == "graph"
        self._session = None
        self._buffers = {}

    def _scratch(self, task, n_total, rec, ws_bytes, device):
        key = (task, n_total, rec, ws_bytes)
        if key not in self._buffers:
            self._buffers[key] = (torch.empty((n_total, rec), dtype=torch.float64, device=device),
                                  torch.empty(ws_bytes, dtype=torch.uint8, device=device))
        return self._buffers[key]

    def _run_flow(self, session, task):
        lib, s = get_lib(), self.sets[task]
        h = s.inputs.shape[2] // 2
        records, ws = self._scratch(task, s.n, lib.dfe_eval_flow_record_doubles(), lib.dfe_eval_flow_ws_bytes(min(self.batch, s.n)),
                                    s.inputs.device)
        for first in range(0, s.n, self.batch):
            pairs = s.inputs[first:first + self.batch]           # the tail batch is smaller
            flow = session.inference_flow(pairs[:, :, :h].contiguous(), pairs[:, :, h:].contiguous())
            eval_flow_records(s, flow, first, records[first:first + len(pairs)], ws)
        values = flow_table(records, s.has_moving, s.n).cpu().tolist()       # the task's one host transfer
        return format_flow_table(values, s.has_moving)

    def _run_depth(self, session):
        lib, s = get_lib(), self.sets["depth"]
        records, ws = self._scratch("depth", s.n, lib.dfe_eval_depth_record_doubles(),
                                    lib.dfe_eval_depth_ws_bytes(min(self.batch, s.n), s.hmax, s.wmax), s.inputs.device)
        for first in range(0, s.n, self.batch):
            x = s.inputs[first:first + self.batch]
            eval_depth_records(s, session.infer_depth(x), first, records[first:first + len(x)], ws)
        rows = records.cpu().numpy()[:, :7]                                  # the task's one host transfer
        return [float(v) for v in rows.astype(np.float32).mean(0)]           # evaluate_depth.py: the mean of the fp32 rows

    def run(self):
        from .inference import InferenceSession
        modes = [(m, m.training) for m in self.model.modules()]
        self.model.eval()
        try:
            if self._session is None:
                self._session = InferenceSession(self.model, graph=self.graph)
            # FusedAdam and a replayed GraphedTrainStep write weights and BatchNorm statistics through raw pointers
            self._session.invalidate()
            out = {}
            with torch.no_grad():
                for task in ("flow_2012", "flow_2015", "depth"):
                    if task in self.sets:
                        out[RESULT_KEYS[task]] = self._run_depth(self._session) if task == "depth" else self._run_flow(self._session, task)
            return out
        finally:
            for m, was in modes:
                m.training = was
