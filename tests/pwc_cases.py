"""Case matrices of the guarded PWC-level tests (test_hip_corr_guarded.py, test_hip_warp_guarded.py,
test_hip_pwc_level_guarded.py).  test_guarded_cpu.py asks the library's own plan queries (dfe_corr_fwd_plan / dfe_corr_bwd_plan)
and the restated one-line rules of tests/guarded.py what each shape runs, and asserts that together they reach every plan named
below; the GPU tests repeat the assertion for the case they run.  Shapes are [B, C, H, W]."""

# ---- cost volume, forward: (shape, family, what the plan query must answer for it)
CORR_FWD = [
    ((8, 13, 64, 208), "randn", dict(coarse=0, PF2=4, DYG=9, KS=1, TH=4, threads=512, chunks=2, CC=7, vec=1, ntx=4)),     # fine, 16-byte kernel; 6 of 7 channels in the second chunk
    ((8, 13, 62, 206), "act", dict(coarse=0, PF2=4, DYG=9, KS=1, TH=4, chunks=2, vec=0, ntx=4)),                          # fine, dword kernel; a bottom tile of 2 rows, a right quad of 2 columns
    ((8, 20, 62, 206), "sparse", dict(coarse=0, PF2=4, chunks=3, vec=0)),                                                  # fine, three chunks: the first buffer is reused
    ((2, 24, 130, 20), "randn", dict(coarse=1, PF2=10, chunks=3, KS=1)),                                                   # coarse, 10 staged quads
    ((1, 33, 40, 132), "act", dict(coarse=1, KS=15, CC=15, chunks=3, ntx=3, DYG=3)),                                       # channel split, 3 of 15 slots used in the last chunk
    ((3, 17, 9, 33), "sparse", dict(coarse=1, KS=17, CC=17, chunks=1)),                                                    # KS = C
    ((1, 1, 1, 1), "randn", dict(chunks=1, KS=1, threads=64)),
    ((2, 3, 2, 3), "randn", dict(chunks=1, KS=3)),
]

# ---- cost volume, backward: (shape, family, plan with both gradients, plan with one)
CORR_BWD = [
    ((8, 20, 64, 208), "randn", dict(TH=8, NCG=3, IS=1, threads=320, lds=92160, batches=2, ncr=1, vec=1), dict(NCG=2, ncr=2, IS=1, batches=2)),
    ((8, 20, 62, 206), "act", dict(TH=8, NCG=3, IS=1, threads=320, lds=92160, batches=2, vec=0), dict(NCG=2, ncr=2, IS=1)),
    ((8, 20, 128, 64), "act", dict(TH=8, TXQ=16, NCG=2, ncr=2, IS=1, threads=256, lds=73728, batches=2, vec=1), dict(TH=4, NCG=2, batches=3)),     # NCG 2 above 64 KB; the second channel range holds one group
    ((8, 20, 128, 62), "randn", dict(TH=8, TXQ=16, NCG=2, ncr=2, IS=1, threads=256, lds=73728, batches=2, vec=0), dict(TH=4, NCG=2, batches=3)),  # ... on the dword kernel
    ((8, 13, 64, 50), "sparse", dict(IS=3, TH=4, ncr=2, vec=0), dict(IS=9, TH=2)),
    ((2, 24, 130, 20), "randn", dict(IS=9, NCG=2, ncr=2, vec=1), dict(IS=9)),
    ((3, 17, 9, 33), "act", dict(IS=9, ncr=3, vec=0), dict(IS=9)),
    ((1, 1, 1, 1), "randn", dict(IS=9), dict(IS=9)),
    ((2, 3, 2, 3), "act", dict(IS=9), dict(IS=9)),
]

# ---- the two fine-plan shapes at which every pointer is moved one float off a 16-byte boundary in turn
ALIGN_SHAPES = [(8, 13, 64, 208), (8, 13, 62, 206)]
CORR_FWD_PTRS = ("f1", "f2", "out")
CORR_BWD_PTRS = ("f1", "f2", "gout", "g1", "g2")
# the pointers launch_corr_fwd / launch_corr_bwd look at inside the level (the others reach the warp kernels only, which
# never use more than dword accesses)
LEVEL_FWD_PTRS = ("c1", "c2", "flow", "warped", "x")
LEVEL_FWD_VEC_PTRS = ("c1", "flow", "warped", "x")
LEVEL_BWD_PTRS = ("c1", "c2", "flow", "warped", "gx", "g_warped", "g_c1", "g_c2", "g_flow")
LEVEL_BWD_VEC_PTRS = ("c1", "warped", "gx", "g_warped", "g_c1")

# ---- feature warp: (shape, flow kind); every case runs use_mask 0 / 1, both align_corners modes, gflow alone, gx alone and both
WARP = [
    ((2, 5, 7, 9), "rough"),            # H*W = 63 < 64, C < 8: one partial wave, the scatter
    ((1, 8, 5, 26), "smooth"),          # H*W = 130: not a multiple of 64
    ((2, 40, 6, 11), "rough"),          # C = 40 > 32 on a small plane: 16 channel groups, five of them with a chunk
    ((1, 136, 6, 11), "smooth"),        # ... and 17 chunks: every one of the 16 groups adds to the sum, the first walks two
    ((1, 40, 32, 65), "rough"),         # H*W = 2080 >= 2048: 4 groups at C = 40, the gather
    ((1, 8, 32, 64), "collapse"),       # H*W = 2048 exactly
    ((2, 5, 3, 1), "zero"),             # a single column
    ((2, 8, 20, 40), "out"),            # sample 0 wholly out of view, sample 1 partly: masked and unmasked zeros beside live pixels
]

# ---- level: (shape, family, flow kind)
LEVEL = [
    ((8, 13, 64, 208), "randn", "smooth"),       # the fine plans of training's batch, 16-byte kernels, gather, map in three launches
    ((8, 13, 62, 206), "act", "rough"),          # the same plans on the dword kernels
    ((2, 7, 15, 34), "randn", "rough"),          # C = 7, H*W = 510: scatter
    ((2, 8, 15, 34), "sparse", "smooth"),        # C = 8, H*W = 510: scatter (plane too small), map in one launch
    ((2, 7, 16, 32), "act", "out"),              # C = 7, H*W = 512: scatter (too few channels)
    ((2, 8, 16, 32), "randn", "rough"),          # C = 8, H*W = 512: the first gather
    ((2, 8, 32, 32), "act", "collapse"),         # H*W = 1024: the last map in one launch
    ((2, 8, 32, 33), "randn", "zero"),           # H*W = 1056: the first map in three
]
LEVEL_SCATTER_ENV = [(2, 8, 16, 32), (2, 8, 32, 33)]        # DFE_WARP_SCATTER=1 where the gather is eligible
LEVEL_MAP_LARGE_ENV = [(2, 8, 16, 32), (2, 8, 32, 32)]      # DFE_WFG_MAP_LARGE=1 where the map would be built in one launch

# ---- pile-up: every pixel sampled at one interior point -> H*W taps on each of four targets, above the 2^16 a double adds exactly
PILE = (1, 8, 258, 256)
PILE_TAPS = 258 * 256


def level_seed(shape):
    return 7 * shape[0] + 11 * shape[1] + 13 * shape[2] + 17 * shape[3]
