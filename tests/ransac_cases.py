"""What a case of the RANSAC terms' tests is, stated once for tests/eight_point_cases.py and tests/pnp_cases.py: a helper, not a
conftest.

A case is a tiny two-view problem: a smooth non-planar depth in [2, 20], per sample its own ``K``, per sample and direction a
pose with a long baseline (|t| about 1.5) and a small rotation, the exact rigid flow of that depth, 30 % of the pixels with their
flow replaced by gross outliers (3 to 8 px off, either sign, both axes), optionally 0.02 px of Gaussian noise on the rest; a
pixel-ordered ``idx``, a seeded duplicate-free ``pick`` (so that no two matches of a plane coincide) and seeded duplicate-free
``sets`` of the term's minimal size.  A DRAWN case has ``pick`` and ``sets`` drawn with replacement, as the product draws them.

The term modules keep what belongs to the term: the seed tables, the thresholds, the float64 composition, the conditions a seed
is chosen by and the figures of its solver.  The functions here take those pieces as arguments."""
import zlib

import numpy as np
import torch

from tests.triangle_cases import _rotation, _smooth

MARGIN = 1e-6
NOISE_PX = 0.02
OUTLIER_SHARE = 0.3
# the scoring kernel's tiles (dfe::ransac in csrc/dfe_ransac.h): MATCH_TILE matches per block, HYP_TILE hypotheses per LDS round
MATCH_TILE, HYP_TILE = 256, 64
# Steering the search for a drawn case only, NOT asserted: the reference's winner leads every ill-defined slot's count by LEAD.
# Those counts rest on vectors that the host's LAPACK picks by rounding (one host polls 8 below the winner where another polls
# 6), so LEAD is twice the 8 first asked for
LEAD = 16
# the slots the isolation tests overwrite: the first and last thread of the hypothesis kernel's first two blocks (32 threads
# each), the first thread of the third and the last slot; 63 / 64 are also the end of the scoring kernel's first LDS round and
# the start of its second
CRAFTED_SLOTS = (0, 31, 32, 63, 64, 69)
WEIGHTS_OF = {1: (0.7,), 2: (0.7, 1.3), 3: (0.7, 1.3, 0.9)}         # the loss tests' cotangents: a different one per sample


def solvers(sets=None):
    """GeometrySolvers with ``_minimal_sets`` overridden on the instance to return ``sets`` [B,hyp,size]."""
    from unsupervised_depth_opticalflow_egomotion_amd.geometry_solvers import GeometrySolvers
    m = GeometrySolvers()
    if sets is not None:
        m.ransac_iters = int(sets.shape[1])
        m._minimal_sets = lambda b, n, k, device: sets.to(device).long()
    return m


def scene(seed, B, H, W, k, num, hyp, noisy, set_size, rot=0.02):
    """(case, K [B,3,3], pose [2,B,3,4]): the tensors every case has (no conditions checked; fp32 values, as the operators take
    them; ``disp_t``: the depth map the flows were rendered from) and, in float64 as numpy arrays, the camera matrices and the
    poses (R | t) of direction d, sample b.  The seed tables hold for this order of draws alone: ``sets`` is the last one, so
    ``set_size`` changes nothing before it, and ``rot`` -- the range of each of the three rotation angles -- enters as the range
    of one ``uniform``."""
    rng = np.random.default_rng(seed)
    K = np.zeros((B, 3, 3))
    flows = np.zeros((2, B, 2, H, W))
    pose = np.zeros((2, B, 3, 4))
    depths = np.zeros((B, 1, H, W))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for b in range(B):
        f = 0.9 * W * rng.uniform(0.95, 1.05)
        K[b] = [[f, 0, (W - 1) / 2.0 + rng.uniform(-0.5, 0.5)], [0, f * rng.uniform(0.97, 1.03), (H - 1) / 2.0 + rng.uniform(-0.5, 0.5)],
                [0, 0, 1]]
        depth = _smooth(rng, H, W, 2.0, 20.0)
        depths[b, 0] = depth
        Ki = np.linalg.inv(K[b])
        X = depth[None] * np.einsum("ij,jhw->ihw", Ki, np.stack([xs, ys, np.ones_like(xs)]))
        for d in range(2):
            sign = rng.choice([-1.0, 1.0], 2)
            t = np.array([sign[0] * rng.uniform(1.0, 1.4), sign[1] * rng.uniform(0.7, 1.0), rng.uniform(-0.3, 0.3)])
            R = _rotation(rng.uniform(-rot, rot, 3))
            pose[d, b, :, :3], pose[d, b, :, 3] = R, t
            p = np.einsum("ij,jhw->ihw", K[b] @ R, X) + (K[b] @ t)[:, None, None]
            u, v = p[0] / p[2] - xs, p[1] / p[2] - ys
            if noisy:
                u = u + NOISE_PX * rng.standard_normal((H, W))
                v = v + NOISE_PX * rng.standard_normal((H, W))
            out = rng.random((H, W)) < OUTLIER_SHARE
            u = np.where(out, u + rng.choice([-1.0, 1.0], (H, W)) * rng.uniform(3.0, 8.0, (H, W)), u)
            v = np.where(out, v + rng.choice([-1.0, 1.0], (H, W)) * rng.uniform(3.0, 8.0, (H, W)), v)
            flows[d, b, 0], flows[d, b, 1] = u, v
    idx = np.stack([np.sort(rng.choice(H * W, k, replace=False)) for _ in range(2 * B)]).astype(np.int32)
    pick = rng.permutation(k)[:num].astype(np.int64)
    sets = np.stack([np.stack([rng.choice(num, set_size, replace=False) for _ in range(hyp)]) for _ in range(B)]).astype(np.int32)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a.astype(np.float32)))   # noqa: E731
    K32 = f32(K)
    case = dict(B=B, H=H, W=W, k=k, num=num, hyp=hyp, noisy=noisy, seed=seed, K=K32, K_inv=torch.inverse(K32.double()).float(),
                flow_bwd=f32(flows[0]), flow_fwd=f32(flows[1]), disp_t=f32(depths), idx=torch.from_numpy(idx),
                pick=torch.from_numpy(pick), sets=torch.from_numpy(sets))
    return case, K, pose


def gathered(case, flow_bwd=None, flow_fwd=None):
    """Per direction (pix [B,num] int64, x, y, u, v [B,num] fp32): pixel idx[p][pick[j]], its coordinates and its flow -- what
    sample_match gathers."""
    B, H, W = case["B"], case["H"], case["W"]
    for d, flow in enumerate((case["flow_bwd"] if flow_bwd is None else flow_bwd, case["flow_fwd"] if flow_fwd is None else flow_fwd)):
        pix = case["idx"][d * B:(d + 1) * B].long()[:, case["pick"]]
        x, y = (pix % W).float(), torch.div(pix, W, rounding_mode="floor").float()
        uv = torch.gather(flow.reshape(B, 2, H * W), 2, pix.unsqueeze(1).expand(-1, 2, -1))
        yield pix, x, y, uv[:, 0], uv[:, 1]


def per_direction(fn, B, *planes):
    """``fn`` on each direction's B planes of the tensors ``planes`` [2B,...] on its own, the two dicts it returns concatenated.
    A batched ``eigh`` / ``svd`` / ``bmm`` may round differently at another batch size (seen at B = 1 and B = 3 on another
    host), the class is called with one direction at a time, and the equality with its result that the cases assert is one of
    bits."""
    halves = [fn(*[t[d * B:(d + 1) * B] for t in planes]) for d in range(2)]
    return {k: torch.cat([h[k] for h in halves], 0) for k in halves[0]}


def rel_margin(e, keep=None, *, thresh):
    """The smallest relative distance of a finite residual to the threshold (inf if there is none); ``keep``: a mask."""
    t = thresh * thresh
    e = e if keep is None else e[keep]
    e = e[torch.isfinite(e)]
    return float(((e - t).abs() / t).min()) if e.numel() else float("inf")


def same_set(inl, counts, best):
    """Every hypothesis that reaches the maximum count has the winner's inlier set: inl [p,hyp,n] bool."""
    top = counts == counts.max(1, keepdim=True)[0]
    win = torch.gather(inl, 1, best.view(-1, 1, 1).expand(-1, 1, inl.shape[2]))
    return bool(((inl == win) | ~top.unsqueeze(2)).all())


def consensus(c):
    """The smallest consensus of a composition, before the fall-backs."""
    return int(min(c["n1raw"].min(), c["n2raw"].min()))


def build_drawn(build, set_size, seed, B, H, W, k, num, hyp, noisy):
    """``build`` with ``pick`` drawn with replacement from a generator seeded with ``seed`` (``Model_geometry.geometric_draw``)
    and ``sets`` the class's own ``_minimal_sets(B, num, set_size, "cpu")`` at ``ransac_iters = hyp`` (a function of the shape
    alone)."""
    case = build(seed, B, H, W, k, num, hyp, noisy)
    g = torch.Generator().manual_seed(seed)
    case["pick"] = torch.randint(0, k, (num,), generator=g)
    m = solvers()
    m.ransac_iters = hyp
    case["sets"] = m._minimal_sets(B, num, set_size, "cpu").to(torch.int32)
    return case


def distinct_pixels(case, sets=None):
    """bool [B,hyp]: the matches of the set are distinct pixels (``idx`` is duplicate-free, so of either direction's plane)."""
    sets = case["sets"] if sets is None else sets
    px = case["pick"][sets.long()].sort(2)[0]
    return (px[:, :, 1:] != px[:, :, :-1]).all(2)


def drawn_figures(well, c):
    """The figures of a drawn case that both terms take from ``well`` [2B,hyp] and the composition ``c``.  ``winner_well`` and
    ``lead`` rest on the counts of ill-defined slots, which the host's LAPACK decides: they steer the search and are printed,
    never asserted."""
    top = c["counts"].max(1)[0]
    ill_top = torch.where(well, torch.full_like(c["counts"], -10 ** 6), c["counts"]).max(1)[0]
    return dict(n_well=int(well.sum(1).min()), n_ill=int((~well).sum(1).min()), lead=int((top - ill_top).min()),
                winner_well=torch.gather(well, 1, c["best"].view(-1, 1)).squeeze(1), consensus=consensus(c))


def drawn_accept(ok, f, ill_winner):
    """``ok`` (the term's own conditions) and: the reference's winner is well-defined on every plane and leads by LEAD, or, for
    the ill-winner case, is ill-defined on some plane."""
    if ill_winner:
        return bool(ok) and not bool(f["winner_well"].all())
    return bool(ok) and bool(f["winner_well"].all()) and f["lead"] >= LEAD


def find_seed(build, conditions, accept, start=0, tries=2000):
    """The first seed from ``start`` for which ``accept(conditions(case), case)`` holds, case = ``build(seed)`` (run once on the
    CPU; the result goes into the term's tables)."""
    for seed in range(start, start + tries):
        case = build(seed)
        if accept(conditions(case), case):
            return seed
    raise RuntimeError("no seed found")


def checked(case, f, carried, checks):
    """Asserts the term's ``checks`` -- (condition, message) pairs over the figures ``f`` -- and stores the ``carried`` entries of
    ``f`` in the case, the rest under ``figures``.  The case is cached and shared from here on: nothing may write into it."""
    for ok, message in checks:
        assert ok, message
    case.update({k: f[k] for k in carried}, figures={k: v for k, v in f.items() if k not in carried})
    return case


def case_checks(f, api):
    """What both terms assert of a case that is not drawn."""
    return [(f["api_equal"], "the restated composition is not %s" % api),
            (f["margin"] >= MARGIN, "a residual within a relative %g of the threshold (%g)" % (MARGIN, f["margin"])),
            (f["same_set"], "two hypotheses reach the maximum count with different inlier sets")]


def drawn_checks(f, case, set_size, api):
    """What both terms assert of a drawn case: only what does not depend on the host -- the figures of the well-defined slots
    and of the refits."""
    return [(f["api_equal"], "the restated composition is not %s" % api),
            (4 * f["n_well"] >= case["hyp"] and f["n_ill"] >= 4, "a plane with %d well-defined, %d ill-defined slots" % (f["n_well"], f["n_ill"])),
            (f["margin"] >= MARGIN, "a residual within a relative %g of the threshold (%g)" % (MARGIN, f["margin"])),
            (f["consensus"] >= set_size, "a consensus of %d" % f["consensus"])]


def without_ill_defined(continued, case, well, first, *rest):
    """The composition with the ill-defined slots refused a vote: the term's ``continued`` from the reference's table (``first``,
    ``rest``: its tensors) with those slots of ``first`` made non-finite.  Nothing in it rests on a vector that rounding picked,
    so it is the same on every host, and it is what the kernel must arrive at whenever none of its own ill-defined slots
    out-polls the winner."""
    first = first.clone()
    first[~well] = float("nan")
    return continued(case, first, *rest)


def pose_vectors(case, seed=0, scale=1.0):
    """A pose [B,2,6] near nothing in particular (the loss tests need a generic one, not the true one)."""
    g = torch.Generator().manual_seed(77 + seed)
    p = torch.randn(case["B"], 2, 6, generator=g) * 0.1
    p[:, :, :3] += torch.tensor([1.0, 0.5, 0.1])
    return p * scale


def crc(case, names):
    c = 0
    for n in names:
        c = zlib.crc32(case[n].contiguous().numpy().tobytes(), c)
    return c


def drawn_layout(set_size, case, key):
    """What a drawn case with sets of ``set_size`` looks like, whatever its seed."""
    B, H, W, k, num, hyp, noisy = key
    assert case["pick"].dtype == torch.int64 and tuple(case["pick"].shape) == (num,) and int(case["pick"].min()) >= 0 and int(case["pick"].max()) < k
    assert case["pick"].unique().numel() < num                                         # drawn with replacement: some pixel repeats
    s = case["sets"]
    assert s.dtype == torch.int32 and tuple(s.shape) == (B, hyp, set_size) and int(s.min()) >= 0 and int(s.max()) < num
    m = solvers()
    m.ransac_iters = hyp
    assert torch.equal(s.long(), m._minimal_sets(B, num, set_size, "cpu"))              # the class's own draw
    well = case["well"]
    assert well.dtype == torch.bool and tuple(well.shape) == (2 * B, hyp)
    assert not bool((well & ~torch.cat([distinct_pixels(case)] * 2, 0)).any())       # a repeated pixel is never well-defined


def checksums(every_tensor=False):
    """{"<term>/<table>/<case>": {name: CRC32 or integers}} of every named case of both terms, from ``build`` / ``build_drawn`` and
    the tables alone.  The tensors that numpy's generator and an fp32 cast decide (K, the flows, disp_t, idx, pick, sets, and the
    pose -- F_true's T34, P_true -- rounded to fp32: its float64 bits hold cos / sin of the host's libm), and for the cases that
    are not drawn the integer decisions of the float64 composition, which the cases keep a relative MARGIN from the threshold:
    the same on every host, recorded in tests/golden/ransac_case_checksums.json.  ``every_tensor``: the float64 bits of every
    tensor of the case as well (K_inv, F_true, P_true go through LAPACK and libm) -- for two trees on one host."""
    from tests import eight_point_cases as EC
    from tests import pnp_cases as PC
    _crc = lambda t: zlib.crc32(t.contiguous().numpy().tobytes())   # noqa: E731
    out = {}
    for term, M in (("eight_point", EC), ("pnp", PC)):
        named = [("SEEDS/%s" % "x".join(str(int(v)) for v in key), M.build, (seed,) + key, {}) for key, seed in sorted(M.SEEDS.items())]
        for name, entry in sorted(M.EDGE_SEEDS.items()):
            named.append(("EDGE_SEEDS/" + name, M.build, (entry[1],) + entry[0], dict(rot=entry[3]) if len(entry) > 3 else {}))
        if hasattr(M, "FALLBACK"):
            named.append(("FALLBACK", M.build, (M.FALLBACK[1],) + M.FALLBACK[0], {}))
        named += [("DRAWN_SEEDS/%s" % "x".join(str(int(v)) for v in key), M.build_drawn, (seed,) + key, {}) for key, seed in sorted(M.DRAWN_SEEDS.items())]
        named.append(("ILL_WINNER", M.build_drawn, (M.ILL_WINNER[1],) + M.ILL_WINNER[0], {}))
        for name, build, args, kw in named:
            case = build(*args, **kw)
            pose = case["T34"] if "T34" in case else case["P_true"]
            rec = {n: _crc(case[n]) for n in ("K", "flow_bwd", "flow_fwd", "disp_t", "idx", "pick", "sets")}
            rec["pose"] = _crc(pose.float())
            if build is M.build:
                c = EC.composition(EC.matches_of(case), case["sets"]) if M is EC else PC.composition_of(case)
                rec.update(best=c["best"].tolist(), counts=_crc(c["counts"]), w1=c["w1"].sum(1).long().tolist(), w2=c["w2"].sum(1).long().tolist())
            if every_tensor:
                rec.update({n + "/bits": _crc(v) for n, v in sorted(case.items()) if hasattr(v, "numpy")})
            out["%s/%s" % (term, name)] = rec
    return out
