"""An independent numpy restatement of ``cv2.resize(img, (W, H))`` (INTER_LINEAR) on a uint8 [h0, w0, cn] image, as OpenCV
4.1.1's modules/imgproc/src/resize.cpp computes it, used to check ``dfe_prepare_triplets_u8`` (tests/test_hip_prepared_feed.py).

Unlike ops.resize_u8_tables it runs OpenCV's passes literally: the coordinate set-up of ``resizeGeneric_``'s caller
(xofs / ialpha per destination column, yofs / ibeta per destination row), ``HResizeLinear`` into int32 rows of ``w * cn``
values (right-edge columns ``S[sx] * 2048``), then per destination row ``VResizeLinear`` with ``VResizeLinearVec_32s8u``'s rule on
the bytes its vector loop covers and ``FixedPtCast<int, uchar, 22>`` on the rest.  ``cv::resize`` copies a same-size image;
``cv::hal::resize`` turns INTER_LINEAR at an exact 1/2 on both axes into INTER_AREA (``resizeAreaFast_``).

No cv2 exists where this was written: this is a reading of that file, not pinned against cv2's output."""
import numpy as np

COEF_BITS = 11
COEF_SCALE = 1 << COEF_BITS


def _floor_f32(v):
    """cvFloor(float)."""
    i = int(v)
    return i - (1 if i > v else 0)


def _sat_short(v):
    """saturate_cast<short>(float): round half to even, then saturate."""
    return int(min(max(np.rint(np.float32(v)), -32768), 32767))


def _axis(dsize, ssize, clamp):
    inv_scale = float(dsize) / float(ssize)
    scale = 1.0 / inv_scale
    ofs, c0, c1 = [], [], []
    for d in range(dsize):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = _floor_f32(f)
        f = np.float32(f - np.float32(s))
        if clamp:
            if s < 0:
                f, s = np.float32(0), 0
            if s >= ssize - 1:
                f, s = np.float32(0), ssize - 1
        ofs.append(s)
        c0.append(_sat_short(np.float32(np.float32(1.0) - f) * np.float32(COEF_SCALE)))
        c1.append(_sat_short(f * np.float32(COEF_SCALE)))
    return ofs, c0, c1


def vector_bytes(n):
    """Bytes of an n-byte row VResizeLinearVec_32s8u covers (16 per step, then one 8-byte step when more than 8 remain)."""
    x = 16 * (n // 16)
    return x + 8 if n - x > 8 else x


def resize_linear_u8(img, out_hw):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    h0, w0, cn = img.shape
    H, W = int(out_hw[0]), int(out_hw[1])
    if (h0, w0) == (H, W):
        return img.copy()
    if w0 == 2 * W and h0 == 2 * H:
        s = img.astype(np.int32)
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    xofs, a0, a1 = _axis(W, w0, True)
    yofs, b0, b1 = _axis(H, h0, False)
    # HResizeLinear: xmax = the first column whose sx + 1 >= w0 (sx monotone); from there on D = S[sx] * ONE
    xmax = next((d for d, s in enumerate(xofs) if s + 1 >= w0), W)
    src = img.astype(np.int64)
    sx = np.array(xofs)
    A0, A1 = np.array(a0)[:xmax, None], np.array(a1)[:xmax, None]

    def hresize(row):        # columns [0, xmax): S[sx]*a0 + S[sx+1]*a1; [xmax, W): S[sx]*ONE
        S = src[row]
        D = np.empty((W, cn), np.int64)
        D[:xmax] = S[sx[:xmax]] * A0 + S[sx[:xmax] + 1] * A1
        D[xmax:] = S[sx[xmax:]] * COEF_SCALE
        return D.reshape(-1)

    n = W * cn
    nv = vector_bytes(n)
    out = np.empty((H, n), np.uint8)
    rows = {}
    for dy in range(H):
        r0 = min(max(yofs[dy], 0), h0 - 1)
        r1 = min(max(yofs[dy] + 1, 0), h0 - 1)
        for r in (r0, r1):
            if r not in rows:
                rows[r] = hresize(r)
        S0, S1 = rows[r0], rows[r1]
        B0, B1 = b0[dy], b1[dy]
        vec = (((B0 * (S0[:nv] >> 4)) >> 16) + ((B1 * (S1[:nv] >> 4)) >> 16) + 2) >> 2
        sca = (S0[nv:] * B0 + S1[nv:] * B1 + (1 << 21)) >> 22
        out[dy] = np.clip(np.concatenate([vec, sca]), 0, 255).astype(np.uint8)
    return out.reshape(H, W, cn)


def prepare_triplet_reference(strip, img_hw, flip, rgb=False):
    """KITTI_Prepared.preprocess_img (kitti_prepared.py:63-90) on one uint8 [3*h0', w0, 3] strip in cv2.imread's channel order
    (``rgb``: the strip holds R, G, B and is reordered first): fp32 [3, 3*H, W], values float32(u / 255.0)."""
    img = np.asarray(strip, np.uint8)
    if rgb:
        img = img[:, :, ::-1]
    h0 = img.shape[0] // 3
    frames = [resize_linear_u8(img[f * h0:(f + 1) * h0], img_hw) for f in range(3)]
    u = np.concatenate(frames, 0)
    if flip:
        u = u[:, ::-1]
    return (u.astype(np.float64) / 255.0).astype(np.float32).transpose(2, 0, 1).copy()
