"""Case matrix of the fused loss stack's guarded tests (test_hip_loss_stack_guarded.py) and of the oracle comparison at the same
shapes (test_hip_loss_stack.py::test_*_at_the_strip_boundaries).  test_guarded_cpu.py asks the library's own plan query
(dfe_geom_plan, include/dfe_hip.h) what each case runs and asserts that together they reach every strip boundary, row remainder,
pyramid path, adjoint mode and workspace-sizing operand named there, and re-derives on the host that no pixel of any case lies
inside a mask family's noise floor and that no mask is constant.

A case is (B, H, W, S, mode, depth_terms): mode 0 = Model_geometry, 1 = Model_depth, 2 = Model_flow; depth_terms = DFE_DEPTH_TERM_*
bits.  Inputs: synthetic.make_loss_stack_inputs(B, H, W, S, seed=SEEDS[(B, H, W, S)]) with conditioned poses (tests/conftest.py).
Strips hold 62 (forward) / 60 (backward) valid columns, row blocks 8 rows."""
import ctypes
import functools

CASES = [
    (2, 24, 124, 4, 0, 0),    # W_0 = 2 x 62, W_1 = 62; H_3 = 3; two-level pyramid; mixed adjoint with a coarse level (adj_s0 = 3)
    (1, 33, 126, 3, 0, 3),    # last forward strip of 2 columns (W_1 = 63: of 1); last row block of 1 row; separable adjoint
    (1, 25, 122, 3, 0, 1),    # last backward strip of 2 columns (W_1 = 61: of 1); depth SSIM alone
    (2, 17, 121, 2, 0, 2),    # last backward strip of 1 column; S < 3: the per-level pyramid kernel; consistency alone
    (1, 40, 125, 3, 1, 0),    # last forward strip of 1 column; W % 4 != 0: the per-level pyramid kernel; Model_depth
    (1, 36, 120, 3, 1, 3),    # W_0 = 2 x 60, W_1 = 60; mixed adjoint without a coarse level; Model_depth with both terms
    (1, 36, 120, 3, 2, 0),    # Model_flow; H_1 = 18: a last row block of 2 rows under the flow-smoothness backward
    (1, 70, 100, 5, 0, 0),    # S = 5 at a non-divisible size: box means on k_geom_area_coarse
    (3, 64, 12, 3, 0, 0),     # tall and narrow: the other operand sizes both partial-sum regions; W_2 = 3; odd batch
    (1, 17, 126, 2, 0, 0),    # both operands equal, of both regions (11 = 11 and 9 = 9): a region one unit short has no slack to hide in
]

# margin-checked seeds per (B, H, W, S), valid for both align_corners settings (test_guarded_cpu.py re-derives this)
SEEDS = {(2, 24, 124, 4): 1, (1, 33, 126, 3): 1, (1, 25, 122, 3): 1, (2, 17, 121, 2): 1, (1, 40, 125, 3): 1, (1, 36, 120, 3): 1,
         (1, 70, 100, 5): 1, (3, 64, 12, 3): 1, (1, 17, 126, 2): 1}

PLAN_HEAD = ("S", "two_level", "generic_jobs", "coarse_jobs", "adj_mode", "adj_s0", "adj_nseg", "nblk_total", "fs_units", "dsm_units",
             "nblk0", "dt", "total_lo", "total_hi", "fwd_rows", "bwd_rows")
PLAN_SCALE = ("H", "W", "fwd_strips", "fwd_last", "bwd_strips", "bwd_last", "last_rows")
PLAN_INTS = 16 + 7 * 8


def case_id(case):
    return "B%d_%dx%d_S%d_mode%d_dt%d" % case


def inputs(case):
    """the LossStackInputs of a case's shape (made once per shape; read-only)"""
    return _inputs(tuple(case[:4]))


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    from unsupervised_depth_opticalflow_egomotion_amd import synthetic
    B, H, W, S = shape
    return synthetic.make_loss_stack_inputs(B, H, W, S, seed=SEEDS[shape])


def bare_args(case, img_ptrs=(0, 0, 0)):
    """a dfe_geom_args with the dimensions of ``case`` and no pointer but the three frame pointers (integers: the plan query
    looks at their alignment and follows none)"""
    from unsupervised_depth_opticalflow_egomotion_amd.loss_stack import GeomArgs
    a = GeomArgs()
    a.B, a.H, a.W, a.num_scales, a.mode, a.depth_terms = case
    for f in range(3):
        a.img[f] = img_ptrs[f] or None
    return a


def plan(lib, args):
    """dfe_geom_plan as a dict: the head's names, ``total`` and ``scales`` (a list of dicts of PLAN_SCALE)"""
    buf = (ctypes.c_int * PLAN_INTS)()
    rc = lib.dfe_geom_plan(ctypes.byref(args), buf)
    assert rc == 0, rc
    p = dict(zip(PLAN_HEAD, buf))
    p["total"] = p["total_lo"] + (p["total_hi"] << 31)
    p["scales"] = [dict(zip(PLAN_SCALE, buf[16 + 7 * s:23 + 7 * s])) for s in range(p["S"])]
    return p
