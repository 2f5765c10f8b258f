"""The case matrices of test_hip_glue_guarded.py and test_hip_head_guarded.py, kept apart from the GPU tests so that
test_guarded_cpu.py can assert on the host which launcher branch every case takes (tests/guarded.py: rule_*) and that each
matrix reaches all of them.  Offsets are in floats past a 16-byte boundary; ``x`` suffixes are floats added to a dense batch
stride.  Not a conftest: imported explicitly."""
from tests import guarded as G

# ------------------------------------------------------------------------------------------------------- epilogue
# hw = 208 (vector), 52 (vector, one partial float4 row), 63 (odd: scalar only), 1, and 41 * 60 = 2460 > EP_CHUNK: two chunks,
# the second 412 elements
EP_SHAPES = [(2, 5, 8, 26), (3, 4, 4, 13), (2, 3, 7, 9), (1, 2, 1, 1), (2, 2, 41, 60)]
EP_SLOPES = [0.1, 0.0, 1.0]
# dfe_bias_act_fwd2: (z, dst1, dst2 offsets; dst1, dst2 stride extras; mode)  mode: two / one (dst2 NULL) / inplace (dst1 == z)
# / slices (dst1 and dst2 = channel slices [0,C) and [C,2C) of one buffer whose offset is dst1's and stride extra dst1's)
EP_FWD2 = [(0, 0, 0, 0, 0, "two"), (1, 0, 0, 0, 0, "two"), (0, 1, 0, 0, 0, "two"), (0, 0, 1, 0, 0, "two"), (1, 1, 1, 0, 0, "two"),
           (0, 0, 0, 1, 0, "two"), (0, 0, 0, 2, 0, "two"), (0, 0, 0, 4, 0, "two"), (0, 0, 0, 0, 1, "two"), (0, 0, 0, 0, 2, "two"),
           (0, 0, 0, 0, 4, "two"), (0, 0, 0, 0, 0, "one"), (0, 1, 0, 0, 0, "one"), (0, 0, 0, 4, 0, "one"), (0, 0, 0, 0, 0, "inplace"),
           (1, 1, 0, 0, 0, "inplace"), (0, 0, 0, 4, 0, "slices"), (0, 0, 0, 1, 0, "slices"), (0, 3, 3, 0, 0, "slices")]
# dfe_bias_act_bwd: (y, gy, gz offsets; gy stride extra; gbias: "gbias" / "none" (no partials either))
EP_BWD = [(0, 0, 0, 0, "gbias"), (1, 0, 0, 0, "gbias"), (0, 1, 0, 0, "gbias"), (0, 0, 1, 0, "gbias"), (1, 1, 1, 0, "gbias"),
          (0, 0, 0, 1, "gbias"), (0, 0, 0, 2, "gbias"), (0, 0, 0, 4, "gbias"), (0, 0, 0, 0, "none"), (0, 2, 0, 4, "none")]
# dfe_bias_act_bwd2: (y, g1, g2, gz offsets (g2 None: NULL); y, g1, g2 stride extras; gbias)
EP_BWD2 = [(0, 0, 0, 0, 0, 0, 0, "gbias"), (1, 0, 0, 0, 0, 0, 0, "gbias"), (0, 1, 0, 0, 0, 0, 0, "gbias"), (0, 0, 1, 0, 0, 0, 0, "gbias"),
           (0, 0, 0, 1, 0, 0, 0, "gbias"), (1, 1, 1, 1, 0, 0, 0, "gbias"),
           (0, 0, 0, 0, 1, 0, 0, "gbias"), (0, 0, 0, 0, 2, 0, 0, "gbias"), (0, 0, 0, 0, 4, 0, 0, "gbias"),
           (0, 0, 0, 0, 0, 1, 0, "gbias"), (0, 0, 0, 0, 0, 2, 0, "gbias"), (0, 0, 0, 0, 0, 4, 0, "gbias"),
           (0, 0, 0, 0, 0, 0, 1, "gbias"), (0, 0, 0, 0, 0, 0, 2, "gbias"), (0, 0, 0, 0, 0, 0, 4, "gbias"),
           (0, 0, None, 0, 0, 0, 0, "gbias"), (0, 0, None, 0, 4, 4, 0, "none"), (0, 1, None, 0, 0, 0, 0, "gbias")]
EP_FINAL_N = [1, 3, 8]


def ep_fwd2_vec(hw, v):
    zo, o1, o2, x1, x2, mode = v
    if mode == "inplace":
        return G.rule_epilogue_vec(hw, [zo], [])
    if mode == "one":
        return G.rule_epilogue_vec(hw, [zo, o1], [x1])          # C * hw is a multiple of 4 whenever hw is
    if mode == "slices":
        return G.rule_epilogue_vec(hw, [zo, o1], [x1])          # the second slice starts C * hw floats later
    return G.rule_epilogue_vec(hw, [zo, o1, o2], [x1, x2])


def ep_bwd_vec(hw, v):
    return G.rule_epilogue_vec(hw, list(v[:3]), [v[3]])


def ep_bwd2_vec(hw, v):
    return G.rule_epilogue_vec(hw, list(v[:4]), [v[4], v[5], v[6] if v[2] is not None else None])


# ------------------------------------------------------------------------------------------------------- elu_pad
ELU_PAD_H = [2, 3, 4, 7]
ELU_PAD_W = [2, 3, 4, 6, 8, 12]
ELU_PAD_BC = (2, 3)
# forward: (x offset (unchecked), out offset); backward: (x, gout (unchecked), gx offsets)
ELU_PAD_FWD_OFFS = [(0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (1, 1)]
ELU_PAD_BWD_OFFS = [(0, 0, 0), (0, 1, 0), (0, 2, 0), (1, 0, 0), (2, 0, 0), (0, 0, 1), (0, 0, 2), (2, 1, 2), (1, 1, 1)]


def elu_pad_cases():
    """(H, W, apply_elu, with_bias): both switches over the matrix, every (H, W)"""
    out = []
    for H in ELU_PAD_H:
        for W in ELU_PAD_W:
            k = len(out)
            out.append((H, W, 1 - k % 2, (k // 2) % 2 == 0))
            out.append((H, W, k % 2, (k // 2) % 2 == 1))
    return out


# ------------------------------------------------------------------------------------------------------- elu_up2_cat_pad
# (B, C1, h, w, C2)
UP2_SHAPES = [(1, 2, 1, 1, 1), (2, 3, 2, 2, 0), (1, 2, 3, 5, 2),
              (1, 1, 17, 33, 1),      # two row tiles, the second one row high; TW = 64, one column tile
              (1, 2, 5, 65, 0),       # two column tiles, the second one column wide
              (2, 1, 3, 65, 1),       # tiles (2) > blocks (1): the element kernel with an aligned gout
              (1, 2, 50, 196, 1)]     # 4 x 4 tiles of 16 x 64: the middle four are clear of the plane's ring
UP2_GOUT_OFFS = [0, 1]
UP2_GSKIP_OFFS = [0, 1, 2]
UP2_OUT_OFFS = [0, 1]


# ------------------------------------------------------------------------------------------------------- batch norm
# (G, Bg, C, H, W, offsets) -- offsets: None (all aligned) or the name of the one tensor that sits one float off
BN_TENSORS_FWD = ("x", "y", "res")
BN_TENSORS_BWD = ("x", "y", "gy", "gx", "gres")


def bn_cases():
    out = [(3, 2, 5, 8, 26, None), (1, 4, 3, 16, 16, None), (2, 2, 4, 8, 28, None), (2, 4, 3, 16, 65, "x"), (2, 4, 3, 15, 65, None)]    # hw = 975: scalar by size
    for hw_shape in [(16, 16), (10, 26), (32, 32), (4, 257), (64, 64), (50, 82)]:        # hw = 256, 260, 1024, 1028, 4096, 4100
        for g in (1, 2, 3):
            for bg in (4, 5):
                out.append((g, bg, 2, hw_shape[0], hw_shape[1], None))
    out.append((1, 5, 2, 50, 52, None))         # hw = 2600 > BN_CHUNK at Bg = 5: three kernels, two chunks, the second 552 long
    out.append((1, 2, 3, 1, 1, None))           # Bg * hw == 2
    for name in ("x", "y", "res", "gy", "gx", "gres"):
        out.append((3, 2, 5, 8, 26, name))      # hw % 4 == 0 with one pointer off: the three-kernel scalar path
    return out


def bn_rule(case, direction, relu, with_res):
    """rule_bn of a case: the launcher looks at x, y, residual (forward) / x, gy, gx, y if relu, gres (backward)"""
    G_, Bg, C, H, W, off = case
    o = lambda name: 1 if off == name else 0
    if direction == "fwd":
        offs = [o("x"), o("y"), o("res") if with_res else None]
    else:
        offs = [o("x"), o("gy"), o("gx"), o("y") if relu else None, o("gres")]
    return G.rule_bn(G_, Bg, H * W, offs)


# ------------------------------------------------------------------------------------------------------- max pooling
POOL_SHAPES = [(6, 1, 1), (3, 2, 9), (4, 8, 9), (2, 37, 131), (1, 2, 130)]
POOL_OFFS = [0, 1, 2, 3]

# ------------------------------------------------------------------------------------------------------- heads
# forward R plan of k_head_fwd, (B, H, W) with ns = 1 and a second / last row block one row high where R = 16:
# R is halved from 16 while B * ns * ceil(H / R) < 2048: B = 1024 -> 2 * 1024 = 2048 at R = 16; 700 -> 1400, then 3 * 700 = 2100 at
# R = 8; 512 -> 1024, 1536, then 5 * 512 = 2560 at R = 4; 2 -> R = 2.  Two strips: 512 * 2 * 2 = 2048 at R = 16.
HEAD_R_CASES = [(16, 1024, 17, 3), (8, 700, 17, 3), (4, 512, 17, 3), (2, 2, 17, 3), (16, 512, 17, 63)]
DISP_C = [16]
FLOW_C_SERIAL = [8, 136]
# k_head_fwd_par (flow head, 32 <= C <= 128)
PAR_C = [32, 128]
PAR_H = [1, 4, 5]
PAR_W = [5, 62, 63]
PAR_B = 2
# backward: W + 2 crosses the 62-column strip at W = 60 / 61, H + 2 the 16-row block at H = 14 / 15; nz = 1 and 3
BWD_W = [60, 61, 62]
BWD_H = [14, 15]
BWD_B = 2
DISP_BWD_C = [16, 48]
FLOW_BWD_C = [8, 24]
