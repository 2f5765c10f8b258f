"""How often a minimal set drawn with replacement is ill-defined at the model's own scale, and how often such a hypothesis wins:
CPU only, the float64 compositions of tests/eight_point_cases.py and tests/pnp_cases.py on ``build_drawn`` at 64x208 with
k = int(0.3 * 64 * 208), num = 6000, hyp = 256, B = 2, seeds 0..15.  Writes profiles/ransac_degenerate_sets.txt.

    python tools/ransac_degenerate_sets.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import eight_point_cases as EC  # noqa: E402
from tests import pnp_cases as PC  # noqa: E402

B, H, W, NUM, HYP, SEEDS = 2, 64, 208, 6000, 256, 16
K = int(0.3 * H * W)


def figures(mod, seed):
    case = mod.build_drawn(seed, B, H, W, K, NUM, HYP, True)
    well = mod.well_defined(case)
    repeats = ~torch.cat([mod.distinct_pixels(case)] * 2, 0)
    if mod is EC:
        counts = EC.composition(EC.matches_of(case), case["sets"])["counts"]
    else:
        counts = PC.composition_of(case)["counts"]
    best = counts.argmax(1)
    top = counts.max(1)[0]
    ill_top = torch.where(well, torch.full_like(counts, -1), counts).max(1)[0]
    wins = ~torch.gather(well, 1, best.view(-1, 1)).squeeze(1)
    return dict(ill=(~well).sum(1), repeats=repeats.sum(1), wins=wins, ties=(ill_top == top) & ~wins, top=top, ill_top=ill_top)


def main():
    lines = ["Minimal sets drawn with replacement at the model's own scale: build_drawn(seed, B = %d, H = %d, W = %d, k = %d, num = %d,"
             % (B, H, W, K, NUM),
             "hyp = %d, noisy), seeds 0..%d, float64 compositions on the CPU (tools/ransac_degenerate_sets.py).  A slot is ill-defined when"
             % (HYP, SEEDS - 1),
             "its matches are not pairwise distinct pixels (\"repeats\") or the null direction of its normal matrix is not isolated",
             "(tests/*_cases.py well_defined).  Per seed, over the %d planes: ill-defined slots (min-max), of which with a repeated pixel" % (2 * B),
             "(min-max); planes whose float64 winner is ill-defined; planes where an ill-defined slot ties a well-defined winner's count;",
             "the winner's count and the best ill-defined count (of the first plane).", ""]
    for name, mod, size in (("eight-point", EC, 8), ("pnp", PC, 6)):
        lines.append("%s (sets of %d)" % (name, size))
        lines.append("   seed  ill-defined  repeats  wins  ties  top/ill-top (plane 0)")
        tot = dict(ill=0, repeats=0, wins=0, ties=0)
        for seed in range(SEEDS):
            f = figures(mod, seed)
            lines.append("   %4d  %4d-%-4d   %3d-%-3d   %d/%d   %d/%d   %d/%d" % (
                seed, int(f["ill"].min()), int(f["ill"].max()), int(f["repeats"].min()), int(f["repeats"].max()), int(f["wins"].sum()), 2 * B,
                int(f["ties"].sum()), 2 * B, int(f["top"][0]), int(f["ill_top"][0])))
            for k in tot:
                tot[k] += float(f[k].sum())
            print(lines[-1], flush=True)
        planes = SEEDS * 2 * B
        lines.append("   mean per plane: %.1f of %d slots ill-defined (%.1f with a repeated pixel); an ill-defined slot wins %d of %d planes "
                     "and ties the winner on %d more" % (tot["ill"] / planes, HYP, tot["repeats"] / planes, int(tot["wins"]), planes, int(tot["ties"])))
        lines.append("")
    with open(os.path.join(ROOT, "profiles", "ransac_degenerate_sets.txt"), "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines[-12:]))


if __name__ == "__main__":
    main()
