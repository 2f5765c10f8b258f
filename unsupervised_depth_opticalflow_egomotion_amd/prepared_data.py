"""Training on the reference's prepared KITTI tree (``KITTI_RAW.prepare_data_mp``'s output, read by ``KITTI_Prepared``,
core/dataset/kitti_prepared.py:10-152, train.py:100-125) with a prefetching feeder.

``PreparedKITTI`` is KITTI_Prepared's non-image half, exactly: the ``train.txt`` list, the sample map, the flip draw and the
intrinsics.  The image half -- cv2.imread, the per-frame 8-bit cv2.resize, cv2.flip, / 255 -- runs on the device for a whole batch
(``ops.prepare_triplets_u8``).  ``PreparedFeeder`` decodes PNG strips on host threads into a ring of pinned slots, uploads them on a
side stream into a device ring, runs the prepare kernel there and hands each batch to the training stream through events, so
batch k+1 is decoded, uploaded and prepared while step k runs.

Sample order.  The training loop asks for idx = (it - start) * B * world + rank * B + j (train.py), i.e. idx runs sequentially
per rank.  The reference's DataLoader shuffles (unseeded) which idx comes when, but every idx already maps to a random sample
and flip: ``RandomState(idx).randint(count)`` then the next draw ``rand() > 0.5`` (kitti_prepared.py:38-42,78,139-140), so
the sequential order draws from the same distribution.  A local RandomState per idx gives the global-RNG sequence the
reference gets from ``np.random.seed(idx)`` and is safe in threads."""
from __future__ import annotations

import os
import queue
import struct
import threading
import warnings

import numpy as np
import torch

from . import ops

_PNG_SIG = b"\x89PNG\r\n\x1a\n"
_CHANNELS = {0: 1, 2: 3, 6: 4}          # colour types accepted: 8-bit grey, RGB, RGBA


def png_header(path):
    """(height, width, channels) from a PNG's IHDR; ValueError for anything but 8-bit grey / RGB / RGBA (how cv2.imread
    converts the others is not restated here)."""
    with open(path, "rb") as fh:
        head = fh.read(33)
    if len(head) < 33 or head[:8] != _PNG_SIG or head[12:16] != b"IHDR":
        raise ValueError("%s is not a PNG file" % path)
    w, h, depth, ctype = struct.unpack(">IIBB", head[16:26])
    if depth != 8 or ctype not in _CHANNELS:
        raise ValueError("%s: unsupported PNG (bit depth %d, colour type %d); the prepared tree must hold 8-bit grey, RGB or "
                         "RGBA strips" % (path, depth, ctype))
    return h, w, _CHANNELS[ctype]


def _pil():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


class PreparedKITTI:
    """KITTI_Prepared (kitti_prepared.py:10-152) without the image arithmetic.  At start-up only the IHDR of every listed strip is
    read: that validates the tree and sizes the feeder's pinned ring exactly."""

    def __init__(self, data_dir, num_scales=3, img_hw=(256, 832)):
        self.data_dir, self.num_scales, self.img_hw = data_dir, int(num_scales), (int(img_hw[0]), int(img_hw[1]))
        info = os.path.join(data_dir, "train.txt")
        if not os.path.isfile(info):
            raise FileNotFoundError("%s not found: --prepared_base_dir must point at a tree prepared by the reference's "
                                    "KITTI_RAW.prepare_data_mp (preparing one from raw KITTI is not part of this package)" % info)
        self.data_list = []
        with open(info) as fh:
            for line in fh.readlines():                       # kitti_prepared.py:22-33
                k = line.strip("\n").split()
                self.data_list.append((os.path.join(data_dir, k[0]), os.path.join(data_dir, k[1])))
        if not self.data_list:
            raise ValueError("%s lists no samples" % info)
        self.headers = [png_header(img) for img, _ in self.data_list]
        self.max_strip_bytes = max(3 * h * w for h, w, _ in self.headers)
        self._K = {}
        self._pil = _pil()
        if self._pil is None:
            warnings.warn("PIL is not installed: prepared strips are decoded by kitti_io.read_png (same bytes, slower)")

    def count(self):
        return len(self.data_list)

    def sample(self, idx):
        """(data-list index, flip) of training idx: np.random.seed(idx); randint(count); rand() > 0.5."""
        rs = np.random.RandomState(int(idx))
        i = int(rs.randint(self.count()))
        return i, bool(rs.rand() > 0.5)

    def frame_hw(self, i):
        """img_hw_orig = (int(h / 3), w) of entry i (kitti_prepared.py:144)."""
        h, w, _ = self.headers[i]
        return int(h / 3), w

    @staticmethod
    def read_cam_intrinsic(fname):
        """The calib file's LAST line, split on single spaces after the key (kitti_prepared.py:101-108): P_rect_03 in a real
        calib_cam_to_cam.txt."""
        with open(fname) as fh:
            lines = fh.readlines()
        data = [float(k) for k in lines[-1].strip("\n").split(" ")[1:]]
        return np.array(data).reshape(3, 4)[:3, :3]

    def intrinsics(self, i):
        """(K_ms, K_inv_ms) float32 [S, 3, 3] of entry i (kitti_prepared.py:110-130,146-148), cached per entry."""
        k = self._K.get(i)
        if k is None:
            K = self.read_cam_intrinsic(self.data_list[i][1])
            ks, kis = ops.rescale_intrinsics(K, self.frame_hw(i), self.img_hw, self.num_scales)
            k = self._K[i] = (ks.numpy(), kis.numpy())
        return k

    def decode(self, i, out=None):
        """Entry i's strip as uint8 [h, w, 3] in R, G, B order (PIL's convert("RGB"); the prepare kernel writes cv2.imread's
        B, G, R).  ``out``: a uint8 array of h*w*3 bytes to decode into."""
        path = self.data_list[i][0]
        h, w, ch = self.headers[i]
        if self._pil is not None:
            with self._pil.open(path) as im:
                if (im.height, im.width) != (h, w):
                    raise ValueError("%s changed size since start-up" % path)
                a = np.asarray(im.convert("RGB"))
        else:
            from . import kitti_io
            a = kitti_io.read_png(path)
            if a.dtype != np.uint8:
                raise ValueError("%s: not an 8-bit PNG" % path)
            if a.ndim == 2:
                a = np.repeat(a[:, :, None], 3, 2)
            a = a[:, :, :3]
        if out is None:
            return np.ascontiguousarray(a)
        out.reshape(h, w, 3)[...] = a
        return out


class InMemoryStrips:
    """A source whose strips are decoded once up front (``decode`` copies them out): measures the feeder's own overhead without
    PNG decode (tools/feed_bench.py).  Same sample map, intrinsics and bytes as the wrapped PreparedKITTI."""

    def __init__(self, src):
        self.src = src
        self.headers, self.max_strip_bytes = src.headers, src.max_strip_bytes
        self.strips = [src.decode(i) for i in range(src.count())]

    def count(self):
        return self.src.count()

    def sample(self, idx):
        return self.src.sample(idx)

    def frame_hw(self, i):
        return self.src.frame_hw(i)

    def intrinsics(self, i):
        return self.src.intrinsics(i)

    def decode(self, i, out=None):
        if out is None:
            return self.strips[i].copy()
        out.reshape(self.strips[i].shape)[...] = self.strips[i]
        return out


def batch_indices(k, batch_size, world=1, rank=0):
    """Training idx of batch k on ``rank``: k * B * world + rank * B + j (train.py's per-rank shard)."""
    base = int(k) * batch_size * world + rank * batch_size
    return [base + j for j in range(batch_size)]


class _Slot:
    """One pinned host slot: the batch's B dfe_u8_desc descriptors (first ``hdr`` bytes), its packed strips (256-byte aligned,
    at hdr + j * stride) and its K / K_inv pair -- one copy for the bytes, one for the intrinsics."""

    def __init__(self, capacity, batch_size, num_scales):
        self.raw = torch.empty(capacity, dtype=torch.uint8).pin_memory()
        self.raw_np = self.raw.numpy()
        self.desc = self.raw_np[:32 * batch_size].view(np.dtype(ops.U8_DESC))
        self.K = torch.empty(2, batch_size, num_scales, 3, 3).pin_memory()
        self.K_np = self.K.numpy()
        self.batch, self.done = -1, 0
        self.copied = None       # event recorded after this slot's upload: refill only once it has completed


class PreparedFeeder:
    """Iterator of training inputs ``[images fp32 [B,3,3H,W], K_ms [B,S,3,3], K_inv_ms [B,S,3,3]]`` on ``device`` for batches
    0 .. num_batches-1 of ``batch_indices``.

    ``num_workers`` host threads decode strips into ``depth`` pinned slots (default num_workers + 2; allocated once); batch k uses
    slot k % depth, refilled only after the event recorded behind its upload has completed.  A worker also draws the sample and
    flip and writes the sample's kernel descriptor, so the training thread only enqueues: the upload (into one of two device raw
    slots, allocated once) and the prepare kernel run on a side stream, and the training stream waits on an event.  A device slot
    is rewritten only behind the prepare that read it (same stream, and an event the upload waits on).  The outputs are fresh
    tensors (models.py keeps a lazy closure over images[0] past the step).  Batches come out in idx order for any worker count;
    ``num_workers=0`` decodes in the calling thread (same bits).  A worker's exception is re-raised by the next ``next()``.
    ``side_stream=False`` uploads and prepares on the consumer's current stream (slower: tools/feed_bench.py)."""

    def __init__(self, source, batch_size, img_hw, device, num_batches, num_workers=0, depth=None, world=1, rank=0,
                 side_stream=True):
        self.src, self.B, self.hw, self.device = source, int(batch_size), (int(img_hw[0]), int(img_hw[1])), torch.device(device)
        self.n, self.world, self.rank = int(num_batches), int(world), int(rank)
        self.workers_n = max(int(num_workers), 0)
        self.depth = int(depth) if depth is not None else self.workers_n + 2
        if self.depth < 1:
            raise ValueError("PreparedFeeder: depth must be >= 1")
        self.hdr = (32 * self.B + 255) // 256 * 256
        self.stride = (source.max_strip_bytes + 255) // 256 * 256
        self.capacity = self.hdr + self.stride * self.B
        # every raw size of the tree: the kernel's tables are uploaded once, here
        self.tab_index, self.tables = ops.u8_tables([source.frame_hw(i) for i in range(source.count())], self.hw, self.device)
        num_scales = source.intrinsics(0)[0].shape[0]
        self.slots = [_Slot(self.capacity, self.B, num_scales) for _ in range(self.depth)]
        self.dev_raw = [torch.empty(self.capacity, dtype=torch.uint8, device=self.device) for _ in range(2)]
        self.dev_free = [None, None]          # event recorded after the prepare that read device slot d
        self.stream = torch.cuda.Stream(self.device) if side_stream else None
        self.k = 0                            # next batch next() returns
        self.issued = {}                      # batch -> (outputs, ready event)
        self.error = None
        self.cv = threading.Condition()
        self.tasks = queue.Queue()
        self.threads = []
        self.closed = False
        for k in range(min(self.depth, self.n)):
            self._submit(k)
        for t in range(self.workers_n):
            th = threading.Thread(target=self._worker, name="prepared-feeder-%d" % t, daemon=True)
            th.start()
            self.threads.append(th)

    # ---------------------------------------------------------------------------------------------------- host side
    def _submit(self, k):
        slot = self.slots[k % self.depth]
        slot.batch, slot.done = k, 0
        if self.workers_n:
            for j in range(self.B):
                self.tasks.put((k, j))

    def _fill(self, k, j):
        """Sample j of batch k: the sample map and flip draw, the descriptor, the decoded strip and the intrinsics."""
        slot = self.slots[k % self.depth]
        ev = slot.copied
        if ev is not None:
            ev.synchronize()                   # the previous batch's upload from this slot has run
        i, flip = self.src.sample(batch_indices(k, self.B, self.world, self.rank)[j])
        h, w, _ = self.src.headers[i]
        h0, w0 = self.src.frame_hw(i)
        o = self.hdr + j * self.stride
        xt, yt = self.tab_index[(h0, w0)]
        slot.desc[j] = (o, h0, w0, xt, yt, int(flip), 0)
        self.src.decode(i, slot.raw_np[o:o + 3 * h * w])
        ks, kis = self.src.intrinsics(i)
        slot.K_np[0, j] = ks
        slot.K_np[1, j] = kis

    def _worker(self):
        while True:
            task = self.tasks.get()
            if task is None or self.closed:
                return
            k, j = task
            try:
                self._fill(k, j)
            except BaseException as e:            # surfaces in the training thread on the next next()
                with self.cv:
                    if self.error is None:
                        self.error = e
                    self.cv.notify_all()
                return
            with self.cv:
                self.slots[k % self.depth].done += 1
                self.cv.notify_all()

    def _wait_filled(self, k):
        slot = self.slots[k % self.depth]
        if not self.workers_n:
            for j in range(self.B):
                self._fill(k, j)
            return slot
        with self.cv:
            while self.error is None and not (slot.batch == k and slot.done == self.B):
                self.cv.wait(0.5)
                if self.error is None and not any(t.is_alive() for t in self.threads):
                    self.error = RuntimeError("PreparedFeeder: every worker thread has exited")
            if self.error is not None:
                raise self.error
        return slot

    # ---------------------------------------------------------------------------------------------------- device side
    def _issue(self, k):
        slot = self.slots[k % self.depth]
        d = k % 2
        consumer = torch.cuda.current_stream(self.device)
        s = self.stream or consumer
        last = slot.desc[self.B - 1]
        n = int(last["offset"]) + 9 * int(last["h0"]) * int(last["w0"])
        with torch.cuda.stream(s):
            if self.dev_free[d] is not None:
                s.wait_event(self.dev_free[d])       # the prepare that read device slot d has completed
            raw = self.dev_raw[d]
            raw[:n].copy_(slot.raw[:n], non_blocking=True)
            K = slot.K.to(self.device, non_blocking=True)
            slot.copied = torch.cuda.Event()
            slot.copied.record(s)
            img = ops.prepare_triplets_u8_desc(raw, raw[:32 * self.B], self.B, self.hw, self.tables, rgb=True)
            ev = torch.cuda.Event()
            ev.record(s)
            self.dev_free[d] = ev
        if self.stream is not None:
            img.record_stream(consumer)
            K.record_stream(consumer)
        self.issued[k] = ([img, K[0], K[1]], ev)
        if k + self.depth < self.n:
            self._submit(k + self.depth)

    def _ready(self, k):
        slot = self.slots[k % self.depth]
        with self.cv:
            return slot.batch == k and slot.done == self.B and self.error is None

    def __iter__(self):
        return self

    def __len__(self):
        return self.n

    def __next__(self):
        if self.k >= self.n:
            self.close()
            raise StopIteration
        if self.error is not None:
            raise self.error
        k = self.k
        if k not in self.issued:
            self._wait_filled(k)
            self._issue(k)
        # batch k+1 goes up now if its strips are already decoded (it overlaps step k on the side stream)
        if self.workers_n and k + 1 < self.n and k + 1 not in self.issued and self._ready(k + 1):
            self._issue(k + 1)
        inputs, ev = self.issued.pop(k)
        if self.stream is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
        self.k += 1
        return inputs

    def close(self):
        """Stop the workers (idempotent).  Tasks still queued are dropped."""
        if self.closed:
            return
        self.closed = True
        for _ in self.threads:
            self.tasks.put(None)
        for th in self.threads:
            th.join()
        self.threads = []
        if self.stream is not None:
            self.stream.synchronize()          # the device ring is not released under a running upload / prepare

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
