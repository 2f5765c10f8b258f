"""GPU: the gradient guard of the optimiser step (csrc/ops_adam.hip: k_grad_sumsq, k_grad_guard_finish, k_adam_step_guarded;
optim.FusedAdam(max_grad_norm=, skip_nonfinite=); train_step.GraphedTrainStep's handling of its record).

Kernel level, through the C ABI on carved tensors with guard bands (test_hip_optim.Launch's way): the norm against numpy
float64 within the counted bound, the coefficient against torch's formula, the clipped update through test_hip_optim.check_step
with g' = g * c32 as its input, c == 1 as a bit-exact no-op against dfe_adam_step_dev, a planted NaN / +-inf leaving every
p, m, v and the count alone, the workspace's exact extent, refused arguments.  Optimiser level: five steps against a float64
CPU twin that runs torch.nn.utils.clip_grad_norm_ and torch.optim.Adam, a skipped step in the counts, capture / replay
against an eager twin, and a whole deterministic training step of the flow model that skips."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.test_hip_optim import HYPER, SENTINEL, U, Carved, Launch, _inputs, _lib, check_step, chunk, dev

pytestmark = pytest.mark.gpu

G1 = "g_off_by_one"                   # only g is off 16 bytes, by ONE float: the scalar path for g alone
ALIGNS = {
    "aligned": lambda i: (0, 0, 0, 0),
    "g_off": lambda i: (0, 1 + i % 3, 0, 0),
    "p_off": lambda i: (1 + i % 3, 0, 0, 0),
    "all_off": lambda i: (1 + i % 3, 1 + (i + 1) % 3, 1 + (i + 2) % 3, 1 + i % 3),
    G1: lambda i: (0, 1, 0, 0),
}
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def ns():
    """a lone element, a partial float4, under a chunk, a chunk less one, a full chunk, one past it, two chunks and a tail"""
    c = chunk()
    return [1, 3, 1023, c - 1, c, c + 1, 2 * c + 5]


def _sentinel_floats(n):
    return np.full(n, SENTINEL, dtype=np.int32).view(np.float32)


class GLaunch(Launch):
    """test_hip_optim.Launch with this file's alignments, optional gradients of its own, a carved workspace and a carved record."""

    def __init__(self, sizes, align, grads=None, t0=0.0):
        self.ns = list(sizes)
        self.inputs = []
        for i, n in enumerate(self.ns):
            p, g, m, v = _inputs(n)
            self.inputs.append((p, g if grads is None else np.ascontiguousarray(grads[i], dtype=np.float32), m, v))
        self.t = [[Carved(x, o) for x, o in zip(quad, ALIGNS[align](i))] for i, quad in enumerate(self.inputs)]
        c = chunk()
        rows = [[q.view.data_ptr() for q in quad] + [n] for quad, n in zip(self.t, self.ns)]
        blocks = [[i, k] for i, n in enumerate(self.ns) for k in range((n + c - 1) // c)]
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev())
        self.blockmap = torch.tensor(blocks, dtype=torch.int32).to(dev())
        self.nblocks = len(blocks)
        lib = _lib().get_lib()
        self.ws_bytes = int(lib.dfe_grad_guard_ws_bytes(self.nblocks))
        assert self.ws_bytes % 4 == 0 and int(lib.dfe_grad_guard_record_bytes()) == 32
        self.ws = Carved(_sentinel_floats(self.ws_bytes // 4), 0)             # the view IS the ws_bytes the library asks for
        self.rec = Carved(np.zeros(8, dtype=np.float32), 0)
        self.count = torch.full((1,), float(t0), dtype=torch.float64, device=dev())
        self.coef = torch.zeros(2, dtype=torch.float32, device=dev())

    def guard(self, max_norm, skip, lr=LR, b1=B1, b2=B2):
        L = _lib()
        L.check(L.get_lib().dfe_grad_guard(*self.args(), float(max_norm), int(skip), lr, b1, b2, ctypes.c_void_p(self.ws.view.data_ptr()),
                                           ctypes.c_void_p(self.count.data_ptr()), ctypes.c_void_p(self.coef.data_ptr()),
                                           ctypes.c_void_p(self.rec.view.data_ptr()), L.stream_ptr()), "dfe_grad_guard")
        torch.cuda.synchronize()

    def update(self, b1=B1, b2=B2, eps=EPS):
        L = _lib()
        L.check(L.get_lib().dfe_adam_step_guarded(*self.args(), b1, b2, eps, ctypes.c_void_p(self.coef.data_ptr()),
                                                  ctypes.c_void_p(self.rec.view.data_ptr()), L.stream_ptr()), "dfe_adam_step_guarded")
        torch.cuda.synchronize()

    def record(self):
        raw = self.rec.numpy().copy()
        return {"norm": float(raw.view(np.float64)[0]), "skipped": float(raw.view(np.float64)[1]), "c": raw[4:5].copy()[0],
                "finite": int(raw.view(np.int32)[5]), "skip": int(raw.view(np.int32)[6]), "bits": raw.view(np.int32).copy()}

    def ref_norm(self):
        """sqrt of the correctly rounded sum of the exact squares: float64 of the same fp32 inputs"""
        sq = np.concatenate([q[1].astype(np.float64) ** 2 for q in self.inputs])
        return math.sqrt(math.fsum(sq))

    def n_elements(self):
        return sum(self.ns)

    def bits(self, which):                      # which: 0 p, 1 g, 2 m, 3 v
        return [quad[which].numpy().view(np.int32).copy() for quad in self.t]

    def intact(self):
        return all(q.guards_intact() for quad in self.t for q in quad) and self.ws.guards_intact() and self.rec.guards_intact()

    def grads_untouched(self):
        return all(np.array_equal(b, q[1].view(np.int32)) for b, q in zip(self.bits(1), self.inputs))


def _randn_grads(scale, seed=5):
    r = np.random.default_rng(seed)
    return [(r.standard_normal(n) * scale).astype(np.float32) for n in ns()]


# ------------------------------------------------------------------ 1 norm

@pytest.mark.parametrize("scale", [1.0, 1e25], ids=["randn", "randn_1e25"])
@pytest.mark.parametrize("align", list(ALIGNS))
def test_norm_vs_float64(align, scale):
    """|norm - ref| <= (N + 2) 2^-53 ref, N the launch's element count: every fp32 square is exact in double (24 x 24 bits fit
    in 53), a sum of N non-negative terms carries a relative error of at most (N - 1) 2^-53 in ANY order of addition, the square
    root rounds once more (and halves the relative error of its argument, which is left uncounted), and the reference -- the
    correctly rounded sum, then one square root -- is itself within 2 roundings.  randn 1e25 squares to 1e50: inf if anything
    squares or adds in fp32.  Two runs leave identical bits in the whole record."""
    launch = GLaunch(ns(), align, _randn_grads(scale))
    launch.guard(0.0, 1)
    rec = launch.record()
    ref, n = launch.ref_norm(), launch.n_elements()
    err = abs(rec["norm"] - ref) / ref
    print("\ngrad guard norm %s x%g: norm %.17g ref %.17g, error %.2f x 2^-53 [bound %d]" % (align, scale, rec["norm"], ref, err * 2.0 ** 53, n + 2))
    assert math.isfinite(rec["norm"]) and err <= (n + 2) * 2.0 ** -53
    assert rec["finite"] == 1 and rec["skip"] == 0 and rec["skipped"] == 0.0 and float(launch.count.cpu()[0]) == 1.0
    again = GLaunch(ns(), align, _randn_grads(scale))
    again.guard(0.0, 1)
    assert np.array_equal(rec["bits"], again.record()["bits"])
    assert launch.intact() and launch.grads_untouched()


# ------------------------------------------------------------------ 2 coefficient

@pytest.mark.parametrize("align", ["aligned", G1])
def test_coefficient(align):
    """c32 within one fp32 ulp of float32(min(1, max_norm / (ref + 1e-6))); exactly 1.0f with max_norm above the norm and with
    clipping off."""
    launch = GLaunch(ns(), align, _randn_grads(1.0))
    ref = launch.ref_norm()
    for frac in (0.37, 1e-3, 0.999):
        max_norm = frac * ref
        launch.guard(max_norm, 0)
        want = np.float32(min(1.0, max_norm / (ref + 1e-6)))
        got = launch.record()["c"]
        assert got.dtype == np.float32 and abs(float(got) - float(want)) <= float(np.spacing(want)), (frac, got, want)
        assert float(got) < 1.0
    launch.guard(1.5 * ref, 0)
    assert launch.record()["c"].view(np.int32) == np.float32(1.0).view(np.int32)
    launch.guard(0.0, 0)
    assert launch.record()["c"].view(np.int32) == np.float32(1.0).view(np.int32)
    assert float(launch.count.cpu()[0]) == 5.0 and launch.intact()


# ------------------------------------------------------------------ 3 clipped update

@pytest.mark.parametrize("hyper", HYPER, ids=lambda h: "lr%g-b%g-%g-eps%g-t%d" % h)
@pytest.mark.parametrize("align", list(ALIGNS))
def test_clipped_update_vs_float64(align, hyper):
    """The guarded update is Adam on g' = fl32(g * c32): with c32 read back and g' formed in numpy fp32, test_hip_optim.check_step's
    counted bounds hold unchanged (g' is the kernel's own input by definition).  The device gradient keeps the uploaded bits."""
    lr, b1, b2, eps, t = hyper
    launch = GLaunch(ns(), align, t0=t - 1)
    launch.guard(0.37 * launch.ref_norm(), 1, lr, b1, b2)
    rec = launch.record()
    c32 = rec["c"]
    assert rec["skip"] == 0 and 0.3 < float(c32) < 0.4 and float(launch.count.cpu()[0]) == t
    launch.update(b1, b2, eps)
    assert launch.intact() and launch.grads_untouched()
    worst = np.zeros(3)
    for i, (quad, (p, g, m, v)) in enumerate(zip(launch.t, launch.inputs)):
        with np.errstate(under="ignore"):
            g1 = g * c32
        assert g1.dtype == np.float32
        after = [quad[0].numpy(), g1, quad[2].numpy(), quad[3].numpy()]
        worst = np.maximum(worst, check_step([p, g1, m, v], after, lr, b1, b2, eps, t, "%s tensor %d" % (align, i)))
    print("\nclipped update %s %s: c %.6f, worst m %.2f u(|m|+|g|) [4], v %.2f u v [6], p %.2f u |U| [8]" % ((align, hyper, float(c32)) + tuple(worst)))


# ------------------------------------------------------------------ 4 c == 1

@pytest.mark.parametrize("align", list(ALIGNS))
def test_c_equal_one_is_the_unguarded_step(align):
    t0 = 9
    a, b = GLaunch(ns(), align, t0=t0), GLaunch(ns(), align, t0=t0)
    a.guard(1e38, 1)
    assert a.record()["c"].view(np.int32) == np.float32(1.0).view(np.int32)
    a.update()
    b.step_dev(LR, B1, B2, EPS, b.count, b.coef)
    assert float(a.count.cpu()[0]) == float(b.count.cpu()[0]) == t0 + 1
    assert torch.equal(a.coef, b.coef)
    for which in (0, 2, 3):
        assert all(np.array_equal(x, y) for x, y in zip(a.bits(which), b.bits(which))), which
    assert a.intact() and a.grads_untouched()


# ------------------------------------------------------------------ 5 non-finite

def _plants():
    c = chunk()
    last = len(ns()) - 1
    return {"first": ("aligned", 0, 0), "last": ("aligned", last, ns()[last] - 1), "chunk_end": ("aligned", 4, c - 1),
            "scalar_path": (G1, last, c + 7)}


@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")], ids=["nan", "pinf", "ninf"])
@pytest.mark.parametrize("where", ["first", "last", "chunk_end", "scalar_path"])
def test_nonfinite_step_is_skipped(where, value):
    align, ti, ei = _plants()[where]
    assert ns()[4] == chunk()
    clean = [_inputs(n)[1] for n in ns()]
    bad = [g.copy() for g in clean]
    bad[ti][ei] = value
    t0 = 4
    launch = GLaunch(ns(), align, bad, t0=t0)
    before = [launch.bits(w) for w in (0, 2, 3)]
    launch.guard(1.0, 1)
    launch.update()
    rec = launch.record()
    assert rec["finite"] == 0 and rec["skip"] == 1
    for b, w in zip(before, (0, 2, 3)):
        assert all(np.array_equal(x, y) for x, y in zip(b, launch.bits(w))), "a skipped step wrote tensor kind %d" % w
    assert float(launch.count.cpu()[0]) == t0 and rec["skipped"] == 1.0
    assert launch.intact()
    # clean gradients next: the step a first call makes from the same state
    launch.t[ti][1].view.copy_(torch.from_numpy(clean[ti].copy()))
    launch.guard(1.0, 1)
    launch.update()
    fresh = GLaunch(ns(), align, clean, t0=t0)
    fresh.guard(1.0, 1)
    fresh.update()
    ra, rb = launch.record(), fresh.record()
    assert ra["skipped"] == 1.0 and rb["skipped"] == 0.0 and ra["finite"] == rb["finite"] == 1
    assert ra["norm"] == rb["norm"] and ra["c"].view(np.int32) == rb["c"].view(np.int32) and ra["skip"] == rb["skip"] == 0
    assert float(launch.count.cpu()[0]) == float(fresh.count.cpu()[0]) == t0 + 1 and torch.equal(launch.coef, fresh.coef)
    for w in (0, 2, 3):
        assert all(np.array_equal(x, y) for x, y in zip(launch.bits(w), fresh.bits(w))), w
    # the same plant with nothing to stop it: runs, stays inside its views (no assertion on the values)
    loose = GLaunch(ns(), align, bad, t0=t0)
    loose.guard(0.0, 0)
    loose.update()
    rl = loose.record()
    assert rl["finite"] == 0 and rl["skip"] == 0 and float(loose.count.cpu()[0]) == t0 + 1
    assert loose.intact() and loose.grads_untouched()


# ------------------------------------------------------------------ 6 workspace, 7 arguments

@pytest.mark.parametrize("align", ["aligned", G1])
def test_workspace_extent(align):
    """dfe_grad_guard_ws_bytes is the exact extent written: every 32-bit word of it changes from the fill pattern (a double partial
    whose low word IS the pattern would be a 2^-32 coincidence; the flags are 0 / 1), no word outside it or around the record does."""
    launch = GLaunch(ns(), align)
    assert launch.ws_bytes == 12 * launch.nblocks and launch.ws.n * 4 == launch.ws_bytes
    launch.guard(1.0, 1)
    words = launch.ws.numpy().view(np.int32)
    assert (words != SENTINEL).all(), np.nonzero(words == SENTINEL)[0][:8]
    flags = words[2 * launch.nblocks:]
    assert (flags == 0).all()
    partial = launch.ws.numpy()[:2 * launch.nblocks].view(np.float64)
    assert (partial >= 0).all() and abs(math.sqrt(math.fsum(partial)) - launch.ref_norm()) <= 1e-12 * launch.ref_norm()
    assert launch.intact()
    assert _lib().get_lib().dfe_grad_guard_ws_bytes(0) == 0


def test_guard_arguments_are_checked():
    """NULL table / block map / ws / step_count / coef / record and an empty grid are refused before anything is launched."""
    L = _lib()
    lib = L.get_lib()
    launch = GLaunch([5, chunk() + 1], "aligned")
    tb, bm, nb = launch.args()
    ws, cnt, coef, rec = (ctypes.c_void_p(x.data_ptr()) for x in (launch.ws.view, launch.count, launch.coef, launch.rec.view))
    s = L.stream_ptr()
    for a in ((None, bm, nb, 1.0, 1, LR, B1, B2, ws, cnt, coef, rec), (tb, None, nb, 1.0, 1, LR, B1, B2, ws, cnt, coef, rec),
              (tb, bm, nb, 1.0, 1, LR, B1, B2, None, cnt, coef, rec), (tb, bm, nb, 1.0, 1, LR, B1, B2, ws, None, coef, rec),
              (tb, bm, nb, 1.0, 1, LR, B1, B2, ws, cnt, None, rec), (tb, bm, nb, 1.0, 1, LR, B1, B2, ws, cnt, coef, None),
              (tb, bm, 0, 1.0, 1, LR, B1, B2, ws, cnt, coef, rec), (tb, bm, -3, 1.0, 1, LR, B1, B2, ws, cnt, coef, rec)):
        assert lib.dfe_grad_guard(*a, s) != 0, a
    for a in ((None, bm, nb, B1, B2, EPS, coef, rec), (tb, None, nb, B1, B2, EPS, coef, rec), (tb, bm, nb, B1, B2, EPS, None, rec),
              (tb, bm, nb, B1, B2, EPS, coef, None), (tb, bm, 0, B1, B2, EPS, coef, rec), (tb, bm, -1, B1, B2, EPS, coef, rec)):
        assert lib.dfe_adam_step_guarded(*a, s) != 0, a
    assert lib.dfe_adam_tick_guarded(LR, B1, B2, None, coef, rec, s) != 0 and lib.dfe_adam_tick_guarded(LR, B1, B2, cnt, coef, None, s) != 0
    torch.cuda.synchronize()
    assert (launch.ws.numpy().view(np.int32) == SENTINEL).all() and (launch.rec.numpy() == 0).all()
    assert float(launch.count.cpu()[0]) == 0.0 and (launch.coef.cpu().numpy() == 0).all()
    assert all(np.array_equal(q.numpy(), x) for quad, inp in zip(launch.t, launch.inputs) for q, x in zip(quad, inp))
    assert launch.intact()


# ------------------------------------------------------------------ 8 trajectory

T_STEPS, T_LR = 5, 1e-3
T_SCALES = [0.3, 3.0, 0.5, 2.0, 0.1]          # times randn: with max_norm = sqrt(N) the steps clip at ~ 1, 1/3, 1, 1/2, 1
T_GROUPS = [dict(lr=T_LR, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6)]


def _t_shapes():
    c = chunk()
    return [[(1,), (3,), (255,), (c - 1,), (c + 1,), (17, 9)], [(1023,), (c,), (2 * c + 5,), (64, 65)]]


def _t_data():
    r = np.random.default_rng(2024)
    p0 = [[r.standard_normal(s).astype(np.float32) for s in grp] for grp in _t_shapes()]
    grads = [[[(r.standard_normal(s) * T_SCALES[it]).astype(np.float32) for s in grp] for grp in _t_shapes()] for it in range(T_STEPS)]
    return p0, grads, math.sqrt(sum(int(np.prod(s)) for grp in _t_shapes() for s in grp))


def _twin64(p0, grads, max_norm):
    """float64 on the CPU: torch.nn.utils.clip_grad_norm_ (or nothing), then torch.optim.Adam.  Returns [group][tensor] (p, m, v),
    the clip coefficients it used and the per-tensor sums the bound below needs."""
    params = [[torch.from_numpy(x).double().requires_grad_(True) for x in grp] for grp in p0]
    opt = torch.optim.Adam([dict(params=ps, **T_GROUPS[gi]) for gi, ps in enumerate(params)], foreach=False)
    coefs = []
    for it in range(T_STEPS):
        for gi, ps in enumerate(params):
            for k, p in enumerate(ps):
                p.grad = torch.from_numpy(grads[it][gi][k]).double()
        if max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_([p for ps in params for p in ps], max_norm))
            coefs.append(min(1.0, max_norm / (norm + 1e-6)))
        opt.step()
    return [[(p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()) for p in ps] for ps in params], coefs


def _fused_run(p0, grads, **guard):
    from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
    params = [[torch.from_numpy(x).to(dev()).requires_grad_(True) for x in grp] for grp in p0]
    opt = FusedAdam([dict(params=ps, **T_GROUPS[gi]) for gi, ps in enumerate(params)], **guard)
    stats = []
    for it in range(T_STEPS):
        for gi, ps in enumerate(params):
            for k, p in enumerate(ps):
                p.grad = torch.from_numpy(grads[it][gi][k]).to(dev())
        opt.step()
        if guard:
            stats.append(opt.guard_stats())
    torch.cuda.synchronize()
    return params, opt, stats


def _errors(params, opt, ref):
    worst = np.zeros(3)
    for gi, ps in enumerate(params):
        for k, p in enumerate(ps):
            got = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
            for j in range(3):
                worst[j] = max(worst[j], np.abs(got[j].cpu().numpy().astype(np.float64) - ref[gi][k][j]).max() / np.abs(ref[gi][k][j]).max())
    return worst


def test_clipped_trajectory_vs_float64():
    """Five steps, two param groups, ten tensors, ONE norm across the groups.  The guarded run is measured against the float64
    twin that clips (torch.nn.utils.clip_grad_norm_, torch.optim.Adam), the unguarded run against the float64 twin that does not;
    errors per tensor relative to its largest reference value, the worst tensor counts, as in
    test_hip_optim.test_fused_adam_trajectory_vs_float64, whose tolerance this is: 2 x the yardstick's error + 4 u -- the
    yardstick being the unguarded run (the same kernel arithmetic on gradients of the same size) -- plus what the guard adds:
    g' = fl32(g fl32(c)) carries two more roundings, |g' - g c| <= 2 u |g c| (the device's double norm is within 1e-11 of the
    twin's).  exp_avg is a weighted sum of the g': + 2 u sum_k w_k max|g_k c_k| / max|m_ref|; exp_avg_sq is a sum of non-negative
    g'^2 terms: + 4 u; a step's update lr/c1 m / (sqrt(v)/sqrt(c2) + eps) moves by at most 2 u of its size through m and 2 u
    through sqrt(v), and its size is at most 1.12 lr while t <= 5 (Cauchy-Schwarz over the two sets of weights, whose ratio
    stays under 1.25): + 5 steps x 5 u lr / max|p_ref|."""
    p0, grads, max_norm = _t_data()
    ref_c, coefs = _twin64(p0, grads, max_norm)
    ref_u, _ = _twin64(p0, grads, None)
    assert [c < 1.0 for c in coefs] == [False, True, False, True, False], coefs
    params_u, opt_u, _ = _fused_run(p0, grads)
    params_g, opt_g, stats = _fused_run(p0, grads, max_grad_norm=max_norm)
    for st, c in zip(stats, coefs):
        assert st["finite"] and st["skipped_steps"] == 0
        assert abs(st["clip_coef"] - c) <= 2.0 ** -23 * c and (st["clip_coef"] == 1.0) == (c == 1.0), (st, c)
    err_u, err_g = _errors(params_u, opt_u, ref_u), _errors(params_g, opt_g, ref_c)
    extra = np.zeros(3)
    for gi, grp in enumerate(ref_c):
        b1 = T_GROUPS[gi]["betas"][0]
        for k, (p, m, v) in enumerate(grp):
            wsum = sum((1.0 - b1) * b1 ** (T_STEPS - 1 - it) * coefs[it] * float(np.abs(grads[it][gi][k]).max()) for it in range(T_STEPS))
            extra = np.maximum(extra, [T_STEPS * 5.0 * U * T_GROUPS[gi]["lr"] / np.abs(p).max(), 2.0 * U * wsum / np.abs(m).max(), 4.0 * U])
    print("\nclipped trajectory: error to float64 in u, guarded p %.2f m %.2f v %.2f; unguarded p %.2f m %.2f v %.2f; the guard's "
          "own roundings allow p %.3f m %.2f v %.2f" % (tuple(err_g / U) + tuple(err_u / U) + tuple(extra / U)))
    for j, name in enumerate(("parameter", "exp_avg", "exp_avg_sq")):
        assert err_g[j] <= 2.0 * err_u[j] + 4.0 * U + extra[j], (name, err_g[j] / U, err_u[j] / U, extra[j] / U)
    sd = opt_g.state_dict()
    assert len(sd["state"]) == 10 and all(float(st["step"]) == T_STEPS for st in sd["state"].values())
    assert set(sd["param_groups"][0]) == set(opt_u.state_dict()["param_groups"][0])         # the layout stays torch.optim.Adam's
    assert all(torch.equal(a.grad, torch.from_numpy(g).to(dev())) for a, g in zip(params_g[0], grads[-1][0]))    # unclipped


def test_a_nonfinite_step_does_not_count():
    """Step 3 of 5 gets an inf from a gradient hook: afterwards every count reads 4 and one step is recorded as skipped; the
    parameters and moments are those of the four clean steps alone."""
    from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
    p0, grads, _ = _t_data()
    flat0 = [x for grp in p0 for x in grp]

    def run(hooked):
        params = [torch.from_numpy(x).to(dev()).requires_grad_(True) for x in flat0]
        opt = FusedAdam([dict(params=params[:6]), dict(params=params[6:], lr=3e-4)], lr=T_LR, skip_nonfinite=True)
        calls = [0]

        def hook(g):
            calls[0] += 1
            if calls[0] == 3:
                g = g.clone()
                g.view(-1)[-1] = float("inf")
            return g
        if hooked:
            params[8].register_hook(hook)
        for it in range(T_STEPS):
            if not hooked and it == 2:
                continue
            xs = [torch.from_numpy(g).to(dev()) for grp in grads[it] for g in grp]
            opt.zero_grad(set_to_none=True)
            sum((p * x).sum() for p, x in zip(params, xs)).backward()
            opt.step()
        torch.cuda.synchronize()
        return params, opt
    params, opt = run(True)
    twin, opt_t = run(False)
    sd = opt.state_dict()
    assert all(float(st["step"]) == T_STEPS - 1 for st in sd["state"].values()) and len(sd["state"]) == 10
    stats = opt.guard_stats()
    assert stats["skipped_steps"] == 1 and stats["finite"] and stats["clip_coef"] == 1.0
    assert opt_t.guard_stats()["skipped_steps"] == 0
    for p, q in zip(params, twin):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(opt.state[p]["exp_avg"], opt_t.state[q]["exp_avg"]) and torch.equal(opt.state[p]["exp_avg_sq"], opt_t.state[q]["exp_avg_sq"])
    # the checkpoint is torch.optim.Adam's
    other = torch.optim.Adam([dict(params=[q.detach().clone().requires_grad_(True) for q in twin[:6]]),
                              dict(params=[q.detach().clone().requires_grad_(True) for q in twin[6:]])], lr=T_LR)
    other.load_state_dict(sd)
    assert all(float(st["step"]) == T_STEPS - 1 for st in other.state.values())


def test_make_optimizer_refuses_the_guard_without_fused_adam(monkeypatch):
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_optimizer
    model = torch.nn.Linear(3, 2).to(dev())
    monkeypatch.setenv("DFE_FUSED_ADAM", "0")
    with pytest.raises(L.DfeError, match="DFE_FUSED_ADAM=0"):
        make_optimizer(model, 1e-3, skip_nonfinite=True)
    assert isinstance(make_optimizer(model, 1e-3), torch.optim.Adam)
    monkeypatch.delenv("DFE_FUSED_ADAM")
    monkeypatch.setenv("DFE_CLIP_GRAD_NORM", "2.5")
    monkeypatch.setenv("DFE_SKIP_NONFINITE", "1")
    opt = make_optimizer(model, 1e-3)
    assert isinstance(opt, FusedAdam) and opt.max_grad_norm == 2.5 and opt.skip_nonfinite is True


# ------------------------------------------------------------------ 9 graph

def test_captured_guarded_step_equals_eager():
    """The optimiser-only step captured once and replayed three times on rewritten static gradients, the second time with an inf:
    parameters, moments, count and record equal an eager guarded twin's bit for bit; two steps counted, one skipped."""
    from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
    p0, grads, max_norm = _t_data()
    flat0 = [x for grp in p0 for x in grp]
    feeds = [[torch.from_numpy(g).to(dev()) for grp in grads[it] for g in grp] for it in (1, 2, 3)]
    feeds[1][3][-1] = float("inf")

    def make():
        params = [torch.from_numpy(x).to(dev()).requires_grad_(True) for x in flat0]
        opt = FusedAdam([dict(params=params[:6]), dict(params=params[6:], lr=3e-4, betas=(0.8, 0.99))], lr=T_LR, capturable=True,
                        max_grad_norm=max_norm, skip_nonfinite=True)
        static = [torch.from_numpy(g).to(dev()) for grp in grads[0] for g in grp]
        for p, g in zip(params, static):
            p.grad = g
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            opt.step()                  # warm-up: state, plan, device counts and the record exist before the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        with torch.no_grad():           # ... and back to the start, in place
            for p, x in zip(params, flat0):
                p.copy_(torch.from_numpy(x))
                opt.state[p]["exp_avg"].zero_()
                opt.state[p]["exp_avg_sq"].zero_()
                opt.state[p]["step"].zero_()
            for dc in opt._dev_count.values():
                dc[0].zero_()
            opt._guard_rec.zero_()
        torch.cuda.synchronize()
        return params, opt, static
    params, opt, static = make()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    twin, opt_t, static_t = make()
    for feed in feeds:
        for s, st, x in zip(static, static_t, feed):
            s.copy_(x)
            st.copy_(x)
        graph.replay()
        opt_t.step()
        torch.cuda.synchronize()
        assert torch.equal(opt._guard_rec.view(torch.int32), opt_t._guard_rec.view(torch.int32))
    for p, q in zip(params, twin):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(opt.state[p]["exp_avg"], opt_t.state[q]["exp_avg"]) and torch.equal(opt.state[p]["exp_avg_sq"], opt_t.state[q]["exp_avg_sq"])
    assert len(opt._dev_count) == 2
    for gi in opt._dev_count:
        assert float(opt._dev_count[gi][0].cpu()[0]) == 2.0 == float(opt_t._dev_count[gi][0].cpu()[0])
        assert torch.equal(opt._dev_count[gi][1], opt_t._dev_count[gi][1])
    stats = opt.guard_stats()
    assert stats["skipped_steps"] == 1 and stats["finite"] and stats["clip_coef"] < 1.0, stats
    assert all(float(st["step"]) == 2.0 for st in opt.state_dict()["state"].values())
    assert float((params[0].detach().cpu() - torch.from_numpy(flat0[0])).abs().max()) > 0.5 * T_LR       # ... of parameters that moved
    del graph
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 10 whole step

def _flow_model():
    from unsupervised_depth_opticalflow_egomotion_amd import synthetic
    from unsupervised_depth_opticalflow_egomotion_amd.models import get_model
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg
    cfg = make_cfg(num_scales=3, img_hw=(256, 832), mode="flow")
    torch.manual_seed(0)
    model = get_model("flow")(cfg).to(dev()).train()
    inputs = [torch.from_numpy(a).to(dev()) for a in synthetic.make_triplet_batch(1, 256, 832, 3, seed=1)]
    return cfg, model, inputs


def _state_of(model, opt):
    sd = opt.state_dict()["state"]
    out = {"param." + n: p.detach().clone() for n, p in model.named_parameters()}
    for i, st in sd.items():
        for k, v in st.items():
            out["state.%d.%s" % (i, k)] = v.detach().clone()
    return out


def _same_bits(a, b):
    assert sorted(a) == sorted(b)
    differ = [k for k in sorted(a) if not torch.equal(a[k], b[k])]
    assert not differ, (len(differ), differ[:6])


def test_whole_step_skips_and_resumes_bit_for_bit():
    """train_step of the flow model in the deterministic mode with skip_nonfinite: a parameter hook makes one gradient element inf
    on step 2.  Parameters and optimiser state after step 2 are those after step 1; step 3 is the step 2 of a twin that never
    had the hook."""
    from unsupervised_depth_opticalflow_egomotion_amd import convs
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_optimizer, train_step
    before = convs.DETERMINISTIC
    convs.set_deterministic(True)
    try:
        def run(hooked, steps):
            cfg, model, inputs = _flow_model()
            opt = make_optimizer(model, 1e-4, skip_nonfinite=True)
            calls = [0]

            def hook(g):
                calls[0] += 1
                if calls[0] == 2:
                    g = g.contiguous().clone()
                    g.view(-1)[g.numel() // 2] = float("inf")
                return g
            if hooked:
                [p for p in model.parameters() if p.requires_grad][7].register_hook(hook)
            states = []
            for _ in range(steps):
                train_step(model, opt, inputs, cfg)
                torch.cuda.synchronize()
                states.append(_state_of(model, opt))
            return states, opt.guard_stats()
        states, stats = run(True, 3)
        twin, stats_t = run(False, 2)
    finally:
        convs.set_deterministic(before)
    assert stats["skipped_steps"] == 1 and stats_t["skipped_steps"] == 0 and stats["finite"]
    assert any(k.endswith(".step") for k in states[0]) and all(float(v) == 1.0 for k, v in states[1].items() if k.endswith(".step"))
    _same_bits(states[0], twin[0])
    _same_bits(states[1], states[0])
    _same_bits(states[2], twin[1])
    assert any(not torch.equal(states[2][k], states[0][k]) for k in states[0] if k.startswith("param."))


def test_graphed_step_warmup_leaves_no_skipped_steps():
    """GraphedTrainStep's warm-up steps all skip here (a hook plants an inf in every backward): constructing it must leave the
    record as it found it -- no skipped step, no count."""
    from tests.test_hip_optim import _batch, _toy
    from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import GraphedTrainStep, make_cfg
    model = _toy()
    opt = FusedAdam(list(model.parameters()), lr=1e-3, capturable=True, max_grad_norm=1.0, skip_nonfinite=True)

    def hook(g):
        g = g.clone()
        g[:1].fill_(float("inf"))       # (a fill kernel: ``g[0] = inf`` copies a host scalar, which a capture refuses)
        return g
    list(model.parameters())[2].register_hook(hook)
    before = [p.detach().clone() for p in model.parameters()]
    g = GraphedTrainStep(model, opt, _batch(0), make_cfg(), warmup=3, restore=True)
    try:
        torch.cuda.synchronize()
        stats = opt.guard_stats()
        assert stats["skipped_steps"] == 0, stats
        assert all(float(st["step"]) == 0.0 for st in opt.state_dict()["state"].values())
        g(_batch(1))
        torch.cuda.synchronize()
        stats = opt.guard_stats()
        assert stats["skipped_steps"] == 1 and not stats["finite"]
        assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
        opt.skip_nonfinite = False
        with pytest.raises(RuntimeError, match="guard"):
            g(_batch(1))
    finally:
        del g
        torch.cuda.synchronize()
