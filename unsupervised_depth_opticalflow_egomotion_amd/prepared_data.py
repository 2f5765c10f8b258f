"""Training on the reference's prepared KITTI tree (``KITTI_RAW.prepare_data_mp``'s output, read by ``KITTI_Prepared``,
core/dataset/kitti_prepared.py:10-152, train.py:100-125) with a prefetching feeder.

``PreparedKITTI`` is KITTI_Prepared's non-image half, exactly: the ``train.txt`` list, the sample map, the flip draw and the
intrinsics.  The image half -- cv2.imread, the per-frame 8-bit cv2.resize, cv2.flip, / 255 -- runs on the device for a whole batch
(``ops.prepare_triplets_u8``).  ``PreparedFeeder`` decodes PNG strips on host threads into a ring of pinned slots, uploads them on a
side stream into a device ring, runs the prepare kernel there and hands each batch to the training stream through events, so
batch k+1 is decoded, uploaded and prepared while step k runs.  ``ResidentTrainSet`` is the same source for a tree that fits in
device memory: the resized 8-bit frames are computed once and kept there, and a batch is one gather launch (same bits).

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


# ------------------------------------------------------------------------------------------------ the device-resident set
RESIDENT_FORMAT = 1                     # meta.json's version: bumped when a cached file's layout changes
RESIDENT_FILES = ("frames.u8", "tri.i32", "K.f32")
MAX_BUILD_THREADS = 16                  # decode threads of the build, whatever num_workers asks for (never sized by the machine)
# What the training step itself needs next to the set, in MB: the measured peak allocation of a B = 8 geom step at 256x832
# (torch.cuda.max_memory_allocated = 8 516 459 520 bytes, profiles/resident_set.txt) times 1.5 -- the allocator's cached blocks
# (10 393 485 312 bytes reserved in the same run), MIOpen workspaces, a graph's private pool -- rounded up to a GB: 13 GB.
RESIDENT_RESERVE_MB = 13312
_CHUNK_BYTES = 64 << 20                 # decoded strips uploaded per resize launch / store bytes per pinned cache chunk


def resident_bytes(F, N, S, img_hw):
    """Device bytes of a resident set: F frames uint8 [3, H, W], the int32 [N, 3] triplet table, the fp32 [N, 2, S, 3, 3]
    intrinsics table and the 256-float lut."""
    H, W = int(img_hw[0]), int(img_hw[1])
    return int(F) * 3 * H * W + int(N) * 3 * 4 + int(N) * 2 * int(S) * 9 * 4 + 256 * 4


def frame_keys(strip, h0, w0):
    """The dedup keys of a decoded strip's three frames: (h0, w0, blake2b-128 of the frame's decoded RGB bytes)."""
    import hashlib
    rows = np.asarray(strip, np.uint8).reshape(-1, w0, 3)
    return [(h0, w0, hashlib.blake2b(rows[f * h0:(f + 1) * h0].tobytes(), digest_size=16).digest()) for f in range(3)]


def _ordered_map(fn, items, num_workers):
    """fn over items in order, on up to min(num_workers, MAX_BUILD_THREADS) threads a chunk at a time (a chunk's results are
    held, never the whole list's); 0 workers: in the calling thread."""
    items = list(items)
    workers = min(max(int(num_workers), 0), MAX_BUILD_THREADS)
    if not workers:
        for it in items:
            yield fn(it)
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(workers) as ex:           # joined on exit: no thread outlives the build
        for a in range(0, len(items), 4 * workers):
            for r in ex.map(fn, items[a:a + 4 * workers]):
                yield r


def plan_frames(source, num_workers=0):
    """The host half of the build: decode every strip once, key its frames and give each distinct frame a slot, in data-list
    order on the calling thread (the layout is the same for any worker count).  Returns (tri int32 [N, 3]: the slots of
    triplet i's frames; slot int64 [N, 3]: the same where triplet i is the FIRST holder of the frame, else -1; F)."""
    n = source.count()
    tri, slot, seen = np.empty((n, 3), np.int32), np.full((n, 3), -1, np.int64), {}

    def keys(i):
        return frame_keys(source.decode(i), *source.frame_hw(i))
    for i, ks in enumerate(_ordered_map(keys, range(n), num_workers)):
        for f, k in enumerate(ks):
            s = seen.get(k)
            if s is None:
                s = seen[k] = len(seen)
                slot[i, f] = s
            tri[i, f] = s
    return tri, slot, len(seen)


def intrinsics_table(source):
    """fp32 [N, 2, S, 3, 3]: K_ms then K_inv_ms of every data-list entry."""
    return np.stack([np.stack(source.intrinsics(i)) for i in range(source.count())]).astype(np.float32)


def cache_key(source):
    """SHA-256 over train.txt's bytes and every strip's (size, mtime_ns, IHDR triple)."""
    import hashlib
    h = hashlib.sha256()
    with open(os.path.join(source.data_dir, "train.txt"), "rb") as fh:
        h.update(fh.read())
    for (img, _), hdr in zip(source.data_list, source.headers):
        st = os.stat(img)
        h.update(struct.pack("<qq3i", st.st_size, st.st_mtime_ns, *hdr))
    return h.hexdigest()


def cache_open(cache_dir, key, N, S, img_hw):
    """(frames memmap uint8 [F, 3, H, W], tri, ktab) of a complete cache whose meta.json matches, else None: a missing or
    short file, another key, size, scale count or format all mean 'absent' (temporary files of an interrupted write are
    never looked at: meta.json is written last)."""
    import json
    H, W = int(img_hw[0]), int(img_hw[1])
    try:
        with open(os.path.join(cache_dir, "meta.json")) as fh:
            meta = json.load(fh)
        want = {"format": RESIDENT_FORMAT, "img_hw": [H, W], "num_scales": int(S), "N": int(N), "key": key}
        if any(meta.get(k) != v for k, v in want.items()):
            return None
        F = int(meta["F"])
        sizes = (F * 3 * H * W, N * 12, N * 2 * S * 36)
        if F < 1 or any(os.path.getsize(os.path.join(cache_dir, f)) != s for f, s in zip(RESIDENT_FILES, sizes)):
            return None
        frames = np.memmap(os.path.join(cache_dir, "frames.u8"), np.uint8, "r", shape=(F, 3, H, W))
        tri = np.fromfile(os.path.join(cache_dir, "tri.i32"), np.int32).reshape(N, 3)
        ktab = np.fromfile(os.path.join(cache_dir, "K.f32"), np.float32).reshape(N, 2, S, 3, 3)
    except (OSError, ValueError, KeyError, TypeError):
        return None
    if tri.size and (tri.min() < 0 or tri.max() >= F):
        return None
    return frames, tri, ktab


def cache_write(cache_dir, key, img_hw, write_frames, F, tri, ktab):
    """Write the cache: every file under a temporary name renamed into place, meta.json last (and removed first, so that a
    half-overwritten directory is never taken for a cache).  ``write_frames(fh)`` streams the store's bytes."""
    import json
    os.makedirs(cache_dir, exist_ok=True)
    meta_path = os.path.join(cache_dir, "meta.json")
    if os.path.exists(meta_path):
        os.remove(meta_path)

    def put(name, writer):
        tmp = os.path.join(cache_dir, name + ".tmp")
        with open(tmp, "wb") as fh:
            writer(fh)
        os.replace(tmp, os.path.join(cache_dir, name))
    put("frames.u8", write_frames)
    put("tri.i32", lambda fh: fh.write(np.ascontiguousarray(tri, np.int32).tobytes()))
    put("K.f32", lambda fh: fh.write(np.ascontiguousarray(ktab, np.float32).tobytes()))
    meta = {"format": RESIDENT_FORMAT, "img_hw": [int(img_hw[0]), int(img_hw[1])], "num_scales": int(ktab.shape[2]), "F": int(F),
            "N": int(tri.shape[0]), "key": key}
    put("meta.json", lambda fh: fh.write(json.dumps(meta, indent=1).encode()))


class _HipStore:
    """The device steps of ResidentTrainSet (injectable: the host half -- plan, budget, cache -- is tested without a device)."""

    def __init__(self, device):
        self.device = torch.device(device)

    def alloc(self, F, img_hw):
        return torch.empty(F, 3, int(img_hw[0]), int(img_hw[1]), dtype=torch.uint8, device=self.device)

    def resize(self, store, raw, sizes, offsets, slot, img_hw):
        """raw: packed decoded strips (host uint8, R, G, B) -> the frames of ``slot`` >= 0 in store"""
        ops.resize_strips_u8(torch.from_numpy(raw).to(self.device), sizes, img_hw, slot, store, offsets, rgb=True)

    def load(self, store, frames):
        """host frames (a memmap) -> store, through one pinned chunk"""
        flat, src = store.view(-1), frames.reshape(-1)
        pin = torch.empty(min(_CHUNK_BYTES, flat.numel()), dtype=torch.uint8).pin_memory()
        for a in range(0, flat.numel(), pin.numel()):
            n = min(pin.numel(), flat.numel() - a)
            pin.numpy()[:n] = src[a:a + n]
            flat[a:a + n].copy_(pin[:n])                  # blocking: the chunk is free again when it returns

    def save(self, store, fh):
        flat = store.view(-1)
        for a in range(0, flat.numel(), _CHUNK_BYTES):
            fh.write(flat[a:a + _CHUNK_BYTES].cpu().numpy().tobytes())

    def finish(self, store, tri, ktab, sizes, img_hw):
        """the set's tensors for ``gather``: (store, tri, ktab, lut)"""
        lut = ops.u8_tables(sizes, img_hw, self.device)[1][2]
        return (store, torch.from_numpy(np.ascontiguousarray(tri, np.int32)).to(self.device),
                torch.from_numpy(np.ascontiguousarray(ktab, np.float32)).to(self.device), lut)

    def gather(self, tensors, idx, flip, out):
        return ops.gather_triplets_u8(tensors, idx, flip, out)


class ResidentTrainSet:
    """The prepared tree's training set kept in device memory: every distinct frame resized ONCE to its 8-bit ``img_hw`` bytes
    (dfe_resize_strips_u8, the image half of ``PreparedFeeder`` up to the byte), a batch made by one gather launch
    (dfe_gather_triplets_u8: frame slots -> flip -> lut -> CHW) with no decode, no host-to-device copy and no thread.  The bits
    are ``PreparedFeeder``'s.  Built over a ``PreparedKITTI``: the sample map, the flip draw and the intrinsics stay its.

    Build: strips are decoded on up to ``num_workers`` threads (at most 16), keyed per frame by (h0, w0, blake2b-128 of the decoded
    RGB bytes) and given slots in data-list order on the building thread -- consecutive strips of a drive share two frames, so a
    set holds about a third of its triplets' frames; then decoded again a chunk at a time, uploaded and resized into the store
    (the number of frames must be known before the store is allocated, and the decoded set does not fit in host memory).
    Before allocating, ``resident_bytes`` + ``reserve_mb`` (what the step needs) is compared with the device's free memory; a set
    that does not fit raises DfeError.  EVERY RANK HOLDS THE WHOLE SET: the sample map draws over the whole list.
    ``cache_dir``: frames.u8 / tri.i32 / K.f32 / meta.json; a cache whose key matches the tree is loaded through np.memmap in
    pinned chunks and nothing is decoded; anything else rebuilds and overwrites (``write_cache=False``: rebuilds only -- the
    ranks of a job other than the first, which would write the same files at the same time).

    ``batches(B, n, world, rank)`` then iterates like ``PreparedFeeder`` (same ``batch_indices``); ``fetch(k, out=None)`` launches
    batch k's gather on the CURRENT stream and returns [images, K_ms, K_inv_ms]: fresh tensors (models.py keeps a closure over
    images[0]), or the tensors of ``out`` (a captured graph's static inputs)."""

    def __init__(self, source, img_hw, device, num_workers=0, cache_dir=None, reserve_mb=RESIDENT_RESERVE_MB, device_ops=None,
                 write_cache=True):
        import time
        t0 = time.perf_counter()
        self.src, self.hw, self.device = source, (int(img_hw[0]), int(img_hw[1])), device
        self.dev = device_ops if device_ops is not None else _HipStore(device)
        self.N = source.count()
        self.S = int(source.intrinsics(0)[0].shape[0])
        self.decoded = 0                               # strips decoded by this build (0: loaded from the cache)
        key = cache_key(source) if cache_dir else None
        cached = cache_open(cache_dir, key, self.N, self.S, self.hw) if cache_dir else None
        sizes = sorted(set(source.frame_hw(i) for i in range(self.N)))
        if cached is not None:
            frames, self.tri, self.ktab = cached
            self.F = int(frames.shape[0])
            store = self._alloc(reserve_mb)
            self.dev.load(store, frames)
            del frames
        else:
            self.tri, slot, self.F = plan_frames(source, num_workers)
            self.decoded += self.N
            self.ktab = intrinsics_table(source)
            store = self._alloc(reserve_mb)
            self._fill(store, slot, num_workers)
            if cache_dir and write_cache:
                cache_write(cache_dir, key, self.hw, lambda fh: self.dev.save(store, fh), self.F, self.tri, self.ktab)
        self.from_cache = cached is not None
        self.tensors = self.dev.finish(store, self.tri, self.ktab, sizes, self.hw)
        self.nbytes = resident_bytes(self.F, self.N, self.S, self.hw)
        self.build_seconds = time.perf_counter() - t0
        self.B = self.n = None
        self.world, self.rank, self.k = 1, 0, 0

    def _alloc(self, reserve_mb):
        need, reserve = resident_bytes(self.F, self.N, self.S, self.hw), int(float(reserve_mb) * (1 << 20))
        free = int(torch.cuda.mem_get_info(self.device)[0])
        if need + reserve > free:
            raise ops.DfeError("ResidentTrainSet: the set needs %d bytes (%d frames of %dx%d for %d triplets) plus a reserve of %d "
                               "bytes for the training step, but only %d bytes are free on %s: train with --data_source prepared "
                               "instead (it streams the tree from the host)"
                               % (need, self.F, self.hw[0], self.hw[1], self.N, reserve, free, self.device))
        return self.dev.alloc(self.F, self.hw)

    def _fill(self, store, slot, num_workers):
        """Second pass: the strips that hold a frame's first occurrence, decoded into packed chunks and resized into the store."""
        todo = [i for i in range(self.N) if (slot[i] >= 0).any()]
        stride = (self.src.max_strip_bytes + 255) // 256 * 256
        per = max(_CHUNK_BYTES // stride, 1)
        for a in range(0, len(todo), per):
            part = todo[a:a + per]
            raw = np.zeros(len(part) * stride, np.uint8)

            def fill(j):
                h, w, _ = self.src.headers[part[j]]
                self.src.decode(part[j], raw[j * stride:j * stride + 3 * h * w])
            for _ in _ordered_map(fill, range(len(part)), num_workers):
                pass
            self.decoded += len(part)
            self.dev.resize(store, raw, [self.src.frame_hw(i) for i in part], [j * stride for j in range(len(part))],
                            slot[part], self.hw)

    # ---------------------------------------------------------------------------------------------------- batches
    def batches(self, batch_size, num_batches, world=1, rank=0):
        """Iterate batches 0 .. num_batches-1 of ``batch_indices(k, batch_size, world, rank)``; returns self."""
        self.B, self.n, self.world, self.rank, self.k = int(batch_size), int(num_batches), int(world), int(rank), 0
        return self

    def draw(self, k):
        """(data-list entries, flips) of batch k: ``source.sample`` of its training indices, on the host."""
        if self.B is None:
            raise ValueError("ResidentTrainSet: call batches(batch_size, num_batches, world, rank) first")
        picks = [self.src.sample(i) for i in batch_indices(k, self.B, self.world, self.rank)]
        return [p[0] for p in picks], [p[1] for p in picks]

    def fetch(self, k, out=None):
        idx, flip = self.draw(k)
        return self.dev.gather(self.tensors, idx, flip, out)

    def __iter__(self):
        return self

    def __len__(self):
        return self.n

    def __next__(self):
        if self.n is None or self.k >= self.n:
            raise StopIteration
        self.k += 1
        return self.fetch(self.k - 1)

    def close(self):
        """Nothing runs behind the set (no thread, no side stream): kept for PreparedFeeder's interface."""


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
