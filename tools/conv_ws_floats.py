#!/usr/bin/env python3
"""The planners of the NCHW matrix-core convolutions (csrc/ops_sconv.hip, ops_wino_wgrad.hip, ops_conv1x1s2.hip) as the library
answers them: workspace floats and support per shape, host code only (no GPU).  tests/golden/conv_ws_floats.json is this
script's output from the library of the commit BEFORE a change to those planners, and tests/test_api_cpu.py holds the tree to it:

    DFE_HIP_LIB=<that build>/libdfe_hip.so python tools/conv_ws_floats.py > tests/golden/conv_ws_floats.json

Every shape is put to all six entry points, whichever list it comes from: the lists of the kernels' GPU tests, of
tools/sconv_bench.py, and shapes no planner takes (the answer 0 is pinned too).
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

# (B, Ci, Co, H, W, K, stride, P) that no planner takes, or only some: empty and negative sizes, filters and strides outside the
# kernels, tensors below the loaders' four floats, sample sizes at the 32-bit limit
UNSUPPORTED = [(0, 16, 16, 8, 8, 3, 2, 1), (1, 0, 16, 8, 8, 3, 2, 1), (1, 16, 0, 8, 8, 3, 2, 1), (1, 16, 16, 0, 8, 3, 2, 1), (1, 16, 16, 8, -1, 3, 2, 1),
               (1, 16, 16, 8, 8, 9, 2, 4), (1, 16, 16, 8, 8, 4, 2, 2), (1, 16, 16, 8, 8, 3, 3, 1), (1, 16, 16, 8, 8, 3, 2, -1), (1, 32, 32, 8, 8, 7, 2, 3),
               (1, 1, 1, 1, 3, 3, 2, 1), (1, 1, 1, 1, 1, 1, 2, 0), (1, 64, 64, 2, 2, 5, 1, 0), (1, 20, 8, 6, 6, 5, 2, 2), (1, 16, 16, 8, 8, 3, 1, 2),
               (1, 1, 1, 32768, 32768, 1, 2, 0), (1, 40000, 40000, 2, 2, 1, 2, 0)]


def shapes():
    """[(origin, (B, Ci, Co, H, W, K, stride, P))]: 5-tuples are the 1x1 stride-2 layers, 6-tuples (.., K) the stride-2 passes with
    P = K // 2, the Winograd list's 6-tuples (.., P) 3x3 stride 1"""
    from tests import test_hip_sconv_passes_guarded as PG, test_hip_conv_wgrad_guarded as WG, test_hip_sconv as SC
    import sconv_bench as SB
    out = []
    for mod, names in ((PG, ("FWD_SHAPES", "FWD_SPLIT_RULE", "DGRAD_SHAPES", "DGRAD_SPLIT_RULE", "C1_SHAPES")),
                       (WG, ("WINO_SHAPES", "SCONV_SHAPES", "THIN_SHAPES")), (SC, ("SHAPES",)), (SB, ("LAYERS", "ONE_BY_ONE", "CHECKS"))):
        for name in names:
            for s in getattr(mod, name):
                s = tuple(int(v) for v in s)
                if len(s) == 5:
                    s = s + (1, 2, 0)
                elif len(s) == 6:
                    s = s[:5] + ((3, 1, s[5]) if name == "WINO_SHAPES" else (s[5], 2, s[5] // 2))
                assert len(s) == 8, (name, s)
                out.append(("%s.%s" % (mod.__name__.split(".")[-1], name), s))
    return out + [("unsupported", s) for s in UNSUPPORTED]


def answers(lib, shape):
    """the six entry points on one (B, Ci, Co, H, W, K, stride, P), under the default tuning"""
    B, ci, co, H, W, K, S, P = shape
    lib.dfe_sconv_tune(0, 0)
    lib.dfe_wino_wgrad_tune(0, 768, 512, 12)
    return {"sconv_wgrad_floats": lib.dfe_sconv_wgrad_floats(B, ci, co, H, W, K, S, P), "sconv_fwd_floats": lib.dfe_sconv_fwd_floats(B, ci, co, H, W, K),
            "sconv_dgrad_floats": lib.dfe_sconv_dgrad_floats(B, ci, co, H, W, K), "wino_wgrad_floats": lib.dfe_wino_wgrad_floats(B, ci, co, H, W, P),
            "conv1x1s2_wgrad_floats": lib.dfe_conv1x1s2_wgrad_floats(B, ci, co, H, W), "conv1x1s2_supported": lib.dfe_conv1x1s2_supported(B, ci, co, H, W)}


def table():
    from unsupervised_depth_opticalflow_egomotion_amd._lib import get_lib
    lib = get_lib()
    rows, seen = [], set()
    for origin, s in shapes():
        if s not in seen:
            seen.add(s)
            rows.append({"from": origin, "shape": list(s), **answers(lib, s)})
    return rows


if __name__ == "__main__":
    print("[\n" + ",\n".join(json.dumps(r) for r in table()) + "\n]")
