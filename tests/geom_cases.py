"""The case matrices of test_hip_geom_guarded.py, test_hip_resize_guarded.py and the conv1x1_small part of
test_hip_planeconv_guarded.py, kept apart from the GPU tests so that test_guarded_cpu.py can assert on the host that they reach
every plane-size class and that every committed inverse_warp2 gradient case is free of unsafe pixels (tests/guarded_geom.py).
Offsets are in floats past a 16-byte boundary.  Not a conftest: imported explicitly."""
OFFS = [0, 1, 2, 3]

# one thread per pixel, 256-thread blocks: (B, H, W)
PIXEL_SHAPES = [(1, 2, 2),       # the smallest plane inverse_warp2 accepts
                (2, 5, 7),       # less than one wave
                (2, 16, 16),     # exactly one block
                (3, 9, 31),      # 279 pixels: the second block has 23 live threads, k_pose_finalize adds two partial rows per sample
                (2, 17, 70)]     # five blocks, W % 4 != 0
TINY_SHAPE = (2, 1, 1)           # masks and rigid flow only


def plane_class(H, W):
    hw = H * W
    if hw == 1:
        return "pixel"
    if hw == 4:
        return "smallest"
    if hw < 64:
        return "sub-wave"
    if hw == 256:
        return "one-block"
    if hw < 512:
        return "partial-second-block"
    return "many-blocks"


PLANE_CLASSES = {"pixel", "smallest", "sub-wave", "one-block", "partial-second-block", "many-blocks"}

# inverse_warp2: gradient cases (B, H, W, pose kind, seed), seeds fixed on the host before any kernel ran: 300 + 7 * shape index +
# pose index (16x16 "oob": 331), each with no unsafe pixel left after the depth nudges for BOTH align_corners settings
# (test_guarded_cpu.py asserts the zero).  Forward / guard-band cases: every pose kind.
WARP_POSES_GRAD = ["rand", "oob"]
WARP_POSES_FWD = ["rand", "oob", "identity", "clamp"]
WARP_SEEDS = {(2, 16, 16, "oob"): 331}          # (B, H, W, pose kind) -> seed, where it is not the formula's


def _seed(shape, kind):
    return WARP_SEEDS.get(shape + (kind,), 300 + 7 * PIXEL_SHAPES.index(shape) + WARP_POSES_FWD.index(kind))


def warp_grad_cases():
    return [(s + (k, _seed(s, k))) for s in PIXEL_SHAPES for k in WARP_POSES_GRAD]


def warp_fwd_cases():
    return [(s + (k, _seed(s, k))) for s in PIXEL_SHAPES for k in WARP_POSES_FWD]


def flow_cases():
    return [(s + (k, _seed(s, k))) for s in PIXEL_SHAPES for k in WARP_POSES_GRAD] + [TINY_SHAPE + ("rand", 399), (2, 5, 7, "clamp", 398)]


# SSIM, 32 x 8 tiles: (B, C, H, W)
SSIM_SHAPES = [(1, 1, 1, 1), (2, 3, 8, 32), (1, 3, 9, 33), (2, 2, 3, 70)]

# dfe_resize_bilinear_fwd / _bwd: (in, out); the last is refused by the backward (one axis beyond ratio 4)
RB_PLANES = 3
RB_CASES = [((4, 13), (8, 26)), ((5, 7), (20, 28)), ((6, 20), (23, 77)), ((8, 26), (8, 26)), ((8, 26), (4, 13))]
RB_REFUSED = ((3, 5), (13, 5))
RB_MULTS = [1.0, 2.0, 4.0]
# dfe_resize mode 0 on both sides of ATen's kernel switch (output H + W <= 128 / > 128), at the switch itself, down-sampling
R0_CASES = [((4, 13), (8, 26)), ((14, 50), (28, 100)), ((14, 50), (29, 100)), ((20, 50), (40, 100)), ((9, 31), (4, 15)), ((1, 1), (3, 2))]
# mode 1: non-divisible, the exact halves, up-sampling, identity
R1_CASES = [((7, 9), (3, 4)), ((8, 26), (4, 13)), ((17, 70), (8, 35)), ((3, 4), (7, 9)), ((5, 7), (5, 7))]

# dfe_conv1x1_small: (B, Ci, Co, H, W)
C1_SHAPES = [(4, 256, 12, 2, 7), (3, 24, 12, 2, 7), (3, 12, 12, 2, 7), (1, 1, 1, 1, 1), (2, 5, 7, 16, 16), (16, 3, 2, 16, 16)]
C1_SLOPES = [0.1, 0.0, 1.0]
C1_REFUSED = [(1, 2, 3, 1, 257), (17, 2, 3, 1, 241)]          # H*W = 257; B*H*W = 4097

POSE_N = [1, 7, 65]
CAMERA_CASES = [(1, 1, 1), (3, 2, 3), (5, 2, 7)]              # (B, ndir, nscale): 70 cameras are past one 64-thread block

SPLAT_KINDS = ["smooth", "rough", "out", "zero", "collapse", "edge", "nan"]

# dfe_prepare_triplets: (H0, W0) -> (H, W)
TRIPLET_CASES = [((6, 10), (6, 10)), ((10, 14), (5, 7)), ((7, 9), (12, 20)), ((5, 300), (3, 90))]
TRIPLET_B = 3
TRIPLET_FLIPS = [1, 0, 1]
