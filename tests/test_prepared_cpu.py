"""The prepared-tree reader (prepared_data.PreparedKITTI) against the real reference KITTI_Prepared (golden G13), the
OpenCV 8-bit resize restatement (tests/cv2_linear_u8.py) and the device kernel's table format (ops.resize_u8_tables), on
the CPU."""
import os

import numpy as np
import pytest
import torch

from tests import cv2_linear_u8 as CV
from tests import prepared_tree
from unsupervised_depth_opticalflow_egomotion_amd import kitti_io, ops, prepared_data

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def g13_tree(tmp_path_factory):
    g = np.load(os.path.join(HERE, "golden", "G13_prepared.npz"))
    root = str(tmp_path_factory.mktemp("g13"))
    prepared_tree.build_tree(root, n=int(g["n_samples"]), seed=int(g["seed"]))
    return root, g


def test_reader_matches_reference_kitti_prepared(g13_tree):
    """Sample map, flip draw and per-scale intrinsics equal what the reference's KITTI_Prepared returned (bit for bit)."""
    root, g = g13_tree
    src = prepared_data.PreparedKITTI(root, int(g["num_scales"]), tuple(g["img_hw"]))
    assert src.count() == int(g["n_samples"])
    for idx in range(len(g["index"])):
        i, flip = src.sample(idx)
        assert i == int(g["index"][idx]) and int(flip) == int(g["flip"][idx]), idx
        ks, kis = src.intrinsics(i)
        assert ks.dtype == np.float32 and np.array_equal(ks, g["K_ms"][idx]), idx
        assert np.array_equal(kis, g["K_inv_ms"][idx]), idx


def test_reader_leaves_global_rng_alone(g13_tree):
    root, g = g13_tree
    src = prepared_data.PreparedKITTI(root, 3, (256, 832))
    np.random.seed(5)
    a = np.random.rand()
    np.random.seed(5)
    src.sample(7)
    assert np.random.rand() == a


def test_pil_bytes_equal_kitti_io(g13_tree):
    pytest.importorskip("PIL")
    root, _ = g13_tree
    src = prepared_data.PreparedKITTI(root, 3, (256, 832))
    for i in range(src.count()):
        a = src.decode(i)
        b = kitti_io.read_png(src.data_list[i][0])
        assert a.dtype == np.uint8 and np.array_equal(a, b)
        out = np.zeros(a.size, np.uint8)
        src.decode(i, out)
        assert np.array_equal(out.reshape(a.shape), a)


def test_header_sizes_ring(g13_tree):
    root, _ = g13_tree
    src = prepared_data.PreparedKITTI(root, 3, (256, 832))
    assert sorted(set(src.frame_hw(i) for i in range(src.count()))) == sorted(prepared_tree.SMALL_SIZES)
    assert src.max_strip_bytes == max(9 * h * w for h, w in prepared_tree.SMALL_SIZES)


def test_restatement_identity_copy():
    img = np.random.default_rng(0).integers(0, 256, (20, 33, 3), dtype=np.uint8)
    assert np.array_equal(CV.resize_linear_u8(img, (20, 33)), img)


def test_restatement_half_is_area_rule():
    img = np.random.default_rng(1).integers(0, 256, (16, 24, 3), dtype=np.uint8)
    s = img.astype(np.int32)
    want = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(CV.resize_linear_u8(img, (8, 12)), want)


@pytest.mark.parametrize("n_out,n_in", [(832, 1242), (256, 375), (64, 40), (128, 60), (832, 1224), (7, 5), (100, 333)])
def test_restatement_coefficient_sums(n_out, n_in):
    for clamp in (True, False):
        _, c0, c1 = CV._axis(n_out, n_in, clamp)
        assert set(np.add(c0, c1).tolist()) <= {2047, 2048, 2049}
        s, t0, t1 = ops._cv_linear_axis(n_out, n_in, clamp)
        assert np.array_equal(t0, c0) and np.array_equal(t1, c1) and np.array_equal(s, CV._axis(n_out, n_in, clamp)[0])


def _emulate_kernel(strip, hw, flip, rgb):
    """dfe_prepare_triplets_u8's integer arithmetic in numpy on ops.resize_u8_tables / resize_u8_vector_bytes."""
    H, W = hw
    h0, w0 = strip.shape[0] // 3, strip.shape[1]
    xt, yt = ops.resize_u8_tables(h0, w0, H, W)
    nvec = ops.resize_u8_vector_bytes(W)
    x = np.arange(W)
    xs = W - 1 - x if flip else x
    x0 = xt[xs, 0]
    x1 = np.minimum(x0 + 1, w0 - 1)
    a0, a1 = (xt[xs, 1] & 0xFFFF)[None, :, None], (xt[xs, 1] >> 16)[None, :, None]
    y0, y1 = yt[:, 0], yt[:, 1]
    b0, b1 = (yt[:, 2] & 0xFFFF)[:, None, None], (yt[:, 2] >> 16)[:, None, None]
    byte = (3 * xs[:, None] + np.arange(3)[None, :])[None]
    lut = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)
    out = []
    for f in range(3):
        fr = strip[f * h0:(f + 1) * h0].astype(np.int64)
        if rgb:
            fr = fr[:, :, ::-1]
        h0r = fr[y0][:, x0] * a0 + fr[y0][:, x1] * a1
        h1r = fr[y1][:, x0] * a0 + fr[y1][:, x1] * a1
        vec = (((b0 * (h0r >> 4)) >> 16) + ((b1 * (h1r >> 4)) >> 16) + 2) >> 2
        sca = (h0r * b0 + h1r * b1 + (1 << 21)) >> 22
        out.append(lut[np.clip(np.where(byte < nvec, vec, sca), 0, 255)])
    return np.concatenate(out, 0).transpose(2, 0, 1)


@pytest.mark.parametrize("h0,w0,hw,flip,rgb", [(37, 124, (32, 96), 0, 0), (40, 60, (64, 128), 1, 0), (24, 46, (12, 23), 0, 1),
                                               (30, 100, (30, 100), 1, 1), (13, 21, (7, 5), 1, 0), (27, 90, (8, 11), 0, 0)])
def test_kernel_tables_match_restatement(h0, w0, hw, flip, rgb):
    """The kernel's table format (ops.resize_u8_tables) evaluated in numpy equals the literal two-pass restatement: linear
    down / up scales, the exact 1/2 (area), a same-size copy, widths with a scalar tail (3 * 5, 3 * 11 bytes), flips, RGB."""
    strip = np.random.default_rng(h0 * w0).integers(0, 256, (3 * h0, w0, 3), dtype=np.uint8)
    got = _emulate_kernel(strip, hw, flip, rgb)
    want = CV.prepare_triplet_reference(strip, hw, flip, rgb)
    assert np.array_equal(got, want)


def test_vector_split():
    assert ops.resize_u8_vector_bytes(832) == 2496 == CV.vector_bytes(2496)
    for w in range(1, 70):
        assert ops.resize_u8_vector_bytes(w) == CV.vector_bytes(3 * w)
    assert CV.vector_bytes(8) == 0 and CV.vector_bytes(15) == 8 and CV.vector_bytes(33) == 32 and CV.vector_bytes(27) == 24


def test_ddp_shard_indices():
    B, world = 4, 3
    seen = []
    for k in range(5):
        for rank in range(world):
            ids = prepared_data.batch_indices(k, B, world, rank)
            assert ids == [(k * B * world) + rank * B + j for j in range(B)]
            seen += ids
    assert seen == list(range(5 * B * world))


def test_missing_train_txt(tmp_path):
    with pytest.raises(FileNotFoundError, match="train.txt"):
        prepared_data.PreparedKITTI(str(tmp_path))


def test_sixteen_bit_png_rejected(tmp_path):
    prepared_tree.build_tree(str(tmp_path), n=2)
    kitti_io.write_png(str(tmp_path / "drive" / ("%010d.png" % 1)), np.zeros((90, 100, 3), np.uint16))
    with pytest.raises(ValueError, match="bit depth 16"):
        prepared_data.PreparedKITTI(str(tmp_path))


def test_palette_and_grey_alpha_rejected(tmp_path):
    prepared_tree.build_tree(str(tmp_path), n=2)
    kitti_io.write_png(str(tmp_path / "drive" / ("%010d.png" % 0)), np.zeros((90, 100, 2), np.uint8))
    with pytest.raises(ValueError, match="colour type 4"):
        prepared_data.PreparedKITTI(str(tmp_path))


def test_prepare_u8_refuses_cpu_tensors():
    with pytest.raises(ops._lib.DfeError):
        ops.prepare_triplets_u8(torch.zeros(3 * 4 * 5 * 3, dtype=torch.uint8), [(4, 5)], (4, 5))
