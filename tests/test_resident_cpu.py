"""The host half of the device-resident training set (prepared_data.ResidentTrainSet): the size function and the budget
refusal, frame dedup and slot assignment, the on-disk cache, the command line and the header's two new prototypes.  The set's
device steps are injected (tests/resident_tree.NumpyStore); every comparison is equality."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import cv2_linear_u8 as CV
from tests import resident_tree as RT
from unsupervised_depth_opticalflow_egomotion_amd import _lib, prepared_data
from unsupervised_depth_opticalflow_egomotion_amd._lib import DfeError

HW = (16, 32)
GB = 1 << 30


@pytest.fixture()
def plenty(monkeypatch):
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (64 * GB, 64 * GB))


@pytest.fixture()
def tree(tmp_path):
    root = str(tmp_path / "tree")
    os.makedirs(root)
    lines, frames = RT.build_shared_tree(root, n=10, seed=5)
    return root, lines, frames


def _set(root, workers=0, cache=None, **kw):
    src = prepared_data.PreparedKITTI(root, 3, HW)
    return prepared_data.ResidentTrainSet(src, HW, "cpu", num_workers=workers, cache_dir=cache, device_ops=RT.NumpyStore(), **kw)


# ------------------------------------------------------------------------------------------------ sizes and the budget
def test_resident_bytes_by_hand():
    # one 256x832 frame is 3 * 256 * 832 = 638976 bytes; a triplet row 12 bytes; an intrinsics row 2 * 3 * 9 * 4 = 216; lut 1024
    assert prepared_data.resident_bytes(1, 1, 3, (256, 832)) == 638976 + 12 + 216 + 1024
    assert prepared_data.resident_bytes(7, 5, 3, (4, 48)) == 7 * 576 + 5 * 12 + 5 * 216 + 1024
    assert prepared_data.resident_bytes(45000, 45000, 4, (256, 832)) == 45000 * 638976 + 45000 * 12 + 45000 * 288 + 1024
    assert prepared_data.resident_bytes(0, 0, 1, (1, 1)) == 1024


def test_budget_refusal_names_both_sizes(tree, monkeypatch):
    root = tree[0]
    free = 3 * (1 << 20)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (free, 64 * GB))
    src = prepared_data.PreparedKITTI(root, 3, HW)
    _, _, F = prepared_data.plan_frames(src)
    need = prepared_data.resident_bytes(F, 10, 3, HW)
    assert need < free                                   # the set alone would fit: the reserve is what refuses it
    with pytest.raises(DfeError) as e:
        _set(root, reserve_mb=4)
    msg = str(e.value)
    assert str(need) in msg and str(free) in msg and str(4 << 20) in msg and "--data_source prepared" in msg
    assert _set(root, reserve_mb=2).F == F               # 2 MB + the set fits into 3 MB


def test_default_reserve_is_the_measured_one():
    """profiles/resident_set.txt records the B = 8 peak behind the default; the default covers it."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resident_set.txt")) as fh:
        m = re.search(r"max_memory_allocated[^\n]*?(\d+) bytes", fh.read())
    assert m is not None and prepared_data.RESIDENT_RESERVE_MB * (1 << 20) >= int(m.group(1))


# ------------------------------------------------------------------------------------------------ dedup and slots
def test_tree_shares_frames(tree):
    root, lines, frames = tree
    src = prepared_data.PreparedKITTI(root, 3, HW)
    assert len(lines) == 10 and len(set(src.frame_hw(i) for i in range(10))) == 2
    a, b = src.decode(0), src.decode(1)
    h0 = src.frame_hw(0)[0]
    assert np.array_equal(a[h0:], b[:2 * h0]) and not np.array_equal(a[:h0], b[:h0])


def test_plan_dedups_and_maps_every_triplet_to_its_frames(tree):
    root, _, frames = tree
    src = prepared_data.PreparedKITTI(root, 3, HW)
    tri, slot, F = prepared_data.plan_frames(src, 0)
    assert F == sum(len(fl) for fl in frames) == 14 and F < 3 * src.count()
    assert tri.dtype == np.int32 and slot.dtype == np.int64 and tri.shape == slot.shape == (10, 3)
    # slots in data-list order: first occurrences count up, everything else is -1
    firsts = slot[slot >= 0]
    assert np.array_equal(firsts, np.arange(F))
    assert np.array_equal(tri[slot >= 0], firsts) and (slot[0] == [0, 1, 2]).all() and (slot[1] == [-1, -1, 3]).all()
    # every triplet's slots hold its own frames
    owner = {}
    for i in range(10):
        strip, (h0, w0) = src.decode(i), src.frame_hw(i)
        for f in range(3):
            fr = strip[f * h0:(f + 1) * h0].tobytes()
            assert owner.setdefault(int(tri[i, f]), (h0, w0, fr)) == (h0, w0, fr)
    assert len(owner) == F and len(set(owner.values())) == F


def test_equal_bytes_at_two_raw_sizes_are_two_frames():
    a = np.arange(2 * 6 * 3, dtype=np.uint8).reshape(2 * 3, 2, 3)          # [3*h0, w0, 3] with (h0, w0) = (2, 2)
    ka, kb = prepared_data.frame_keys(a, 2, 2), prepared_data.frame_keys(a.reshape(3, 4, 3), 1, 4)
    assert len(set(ka)) == 3 and len(ka[0][2]) == 16 and not set(ka) & set(kb)


def test_layout_equal_for_any_worker_count(tree, plenty):
    root = tree[0]
    a, b = _set(root, 0), _set(root, 3)
    assert a.F == b.F and np.array_equal(a.tri, b.tri) and np.array_equal(a.tensors[0], b.tensors[0])
    assert np.array_equal(a.ktab, b.ktab) and a.ktab.shape == (10, 2, 3, 3, 3)
    assert not (a.tensors[0] == RT.SENTINEL).all(axis=(1, 2, 3)).any()      # every slot was written


def test_store_holds_the_resized_frames_and_fetch_follows_the_feeder_indices(tree, plenty):
    root, _, frames = tree
    s = _set(root, 2)
    want = [RT.stored_frame(fr, HW) for fl in frames for fr in fl]         # data-list order = drive by drive, frame by frame
    assert np.array_equal(s.tensors[0], np.stack(want))
    s.batches(3, 4, world=2, rank=1)
    assert len(s) == 4
    got = list(s)
    assert len(got) == 4
    for k, (img, K, Ki) in enumerate(got):
        picks = [s.src.sample(i) for i in prepared_data.batch_indices(k, 3, 2, 1)]
        for j, (i, flip) in enumerate(picks):
            assert np.array_equal(K[j], s.src.intrinsics(i)[0]) and np.array_equal(Ki[j], s.src.intrinsics(i)[1])
            assert np.array_equal(img[j], CV.prepare_triplet_reference(s.src.decode(i), HW, flip, rgb=True))
    with pytest.raises(StopIteration):
        next(s)
    s.close()


def test_build_threads_are_capped_and_joined(tree, plenty):
    import threading
    before = threading.active_count()
    s = _set(tree[0], 64)
    assert prepared_data.MAX_BUILD_THREADS == 16 and threading.active_count() <= before and s.decoded >= 10


# ------------------------------------------------------------------------------------------------ cache
def _no_decode(monkeypatch):
    def boom(self, i, out=None):
        raise AssertionError("decode called")
    monkeypatch.setattr(prepared_data.PreparedKITTI, "decode", boom)


def test_cache_reload_decodes_nothing(tree, plenty, tmp_path, monkeypatch):
    root, cache = tree[0], str(tmp_path / "cache")
    a = _set(root, 0, cache)
    assert not a.from_cache and sorted(os.listdir(cache)) == ["K.f32", "frames.u8", "meta.json", "tri.i32"]
    with open(os.path.join(cache, "meta.json")) as fh:
        meta = json.load(fh)
    assert meta == {"format": prepared_data.RESIDENT_FORMAT, "img_hw": list(HW), "num_scales": 3, "F": a.F, "N": 10,
                    "key": prepared_data.cache_key(a.src)} and len(meta["key"]) == 64
    _no_decode(monkeypatch)
    b = _set(root, 0, cache)
    assert b.from_cache and b.decoded == 0 and b.F == a.F
    assert np.array_equal(a.tensors[0], b.tensors[0]) and np.array_equal(a.tri, b.tri) and np.array_equal(a.ktab, b.ktab)
    assert a.tri.dtype == b.tri.dtype and a.ktab.dtype == b.ktab.dtype


def test_cache_rebuilds_when_the_list_grows(tree, plenty, tmp_path):
    root, cache = tree[0], str(tmp_path / "cache")
    a = _set(root, 0, cache)
    with open(os.path.join(root, "train.txt")) as fh:
        first = fh.readline()
    with open(os.path.join(root, "train.txt"), "a") as fh:
        fh.write(first)
    b = _set(root, 0, cache)
    assert not b.from_cache and b.N == 11 and b.F == a.F and np.array_equal(b.tri[10], b.tri[0])
    assert _set(root, 0, cache).from_cache                                  # ... and overwrote the cache


def test_cache_rebuilds_when_a_strip_changes(tree, plenty, tmp_path):
    root, cache = tree[0], str(tmp_path / "cache")
    a = _set(root, 0, cache)
    path = a.src.data_list[3][0]
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    assert not _set(root, 0, cache).from_cache


def test_cache_without_meta_is_absent(tree, plenty, tmp_path):
    root, cache = tree[0], str(tmp_path / "cache")
    a = _set(root, 0, cache)
    os.remove(os.path.join(cache, "meta.json"))
    b = _set(root, 0, cache)
    assert not b.from_cache and np.array_equal(a.tensors[0], b.tensors[0]) and os.path.exists(os.path.join(cache, "meta.json"))


def test_interrupted_write_is_absent(tree, plenty, tmp_path):
    """Temporary files and even finished data files, but no meta.json: nothing is read from the directory."""
    root, cache = tree[0], str(tmp_path / "cache")
    os.makedirs(cache)
    for name in ("frames.u8.tmp", "tri.i32", "K.f32.tmp", "meta.json.tmp"):
        with open(os.path.join(cache, name), "wb") as fh:
            fh.write(b"\x00" * 100)
    src = prepared_data.PreparedKITTI(root, 3, HW)
    assert prepared_data.cache_open(cache, prepared_data.cache_key(src), 10, 3, HW) is None
    s = _set(root, 0, cache)
    assert not s.from_cache and _set(root, 0, cache).from_cache
    assert sorted(os.listdir(cache)) == ["K.f32", "frames.u8", "meta.json", "tri.i32"]      # every temporary name was renamed


def test_a_rank_that_must_not_write_builds_and_leaves_the_directory_alone(tree, plenty, tmp_path):
    root, cache = tree[0], str(tmp_path / "cache")
    s = _set(root, 0, cache, write_cache=False)
    assert not s.from_cache and not os.path.exists(cache)
    a = _set(root, 0, cache)
    assert _set(root, 0, cache, write_cache=False).from_cache and np.array_equal(a.tensors[0], s.tensors[0])


def test_cache_of_another_size_or_a_short_file_is_absent(tree, plenty, tmp_path):
    root, cache = tree[0], str(tmp_path / "cache")
    a = _set(root, 0, cache)
    key = prepared_data.cache_key(a.src)
    assert prepared_data.cache_open(cache, key, 10, 3, HW) is not None
    assert prepared_data.cache_open(cache, key, 10, 3, (16, 48)) is None
    assert prepared_data.cache_open(cache, key, 10, 4, HW) is None
    assert prepared_data.cache_open(cache, "0" * 64, 10, 3, HW) is None
    with open(os.path.join(cache, "frames.u8"), "r+b") as fh:
        fh.truncate(100)
    assert prepared_data.cache_open(cache, key, 10, 3, HW) is None


# ------------------------------------------------------------------------------------------------ CLI and header
def test_cli_accepts_resident_and_keeps_yaml_cache():
    import train
    ap = train.build_parser()
    assert ap.parse_args(["--data_source", "resident"]).data_source == "resident"
    yaml_cfg = {"img_hw": [256, 832], "data_source": "resident", "resident_cache": "/data/cache", "resident_reserve_mb": 100}
    unset = train.merge_cfg(ap.parse_args([]), yaml_cfg)
    assert unset["data_source"] == "resident" and unset["resident_cache"] == "/data/cache" and unset["resident_reserve_mb"] == 100
    given = train.merge_cfg(ap.parse_args(["--resident_cache", "/x", "--data_source", "prepared"]), yaml_cfg)
    assert given["resident_cache"] == "/x" and given["data_source"] == "prepared"
    assert "resident_cache" in train.KEEP_YAML_WHEN_UNSET
    with pytest.raises(SystemExit):
        ap.parse_args(["--data_source", "elsewhere"])


def test_header_declares_and_binds_both_symbols():
    import ctypes
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    sigs = _lib.header_signatures()
    p, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert sigs["dfe_resize_strips_u8"] == (i, [p, p, p, p, p, p, l, i, i, i, i, i, p])
    assert sigs["dfe_gather_triplets_u8"] == (i, [p, l, p, p, i, p, p, p, p, p, p, i, i, i, i, p])
    assert re.search(r"idx_host\s*:\s*HOST pointer", text) and re.search(r"flip_host\s*:\s*HOST pointer", text)
    assert _lib.header_abi_version() == 4
