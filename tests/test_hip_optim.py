"""GPU: the optimiser (csrc/ops_adam.hip, optim.FusedAdam, train_step.GraphedTrainStep's use of it) pinned to float64.

A  one launch of dfe_adam_step through the C ABI against the float64 recurrence: sizes around the chunk edge, every
   combination of 16-byte aligned / misaligned p, g, m, v (the scalar path: ddp.FlatAllReduce hands over gradient views
   that start at any float), guard bands around every view, six hyper-parameter rows, gradients whose square overflows;
B  dfe_adam_step_dev: the count and the two coefficients formed on the device;
C  FusedAdam over 50 steps, two param groups, a scheduler's lr change, against float64, held to torch.optim.Adam's own
   error on the same gradients;
D  capture / replay / resume on a toy module whose gradient IS its input: the moments of a replayed run are bit-equal to
   an eager run's, so a frozen or reset bias correction (percents of lr per step) has nowhere to hide; every direction
   of the checkpoint matrix eager <-> graph <-> torch.optim.Adam.

u = 2^-24 is fp32's unit roundoff throughout; the library is built with -ffp-contract=off (no fused multiply-add), so
every fp32 operation of the kernel rounds once and the bounds below are counted from its expression tree."""
import copy
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -149                    # the smallest fp32 subnormal: a result rounded in the subnormal range is off by <= TINY / 2
SENTINEL = -559038737                 # 0xDEADBEEF as int32: -6.2598534e18 as a float, a value no update produces
PAD = 8                               # guard floats on each side of a view

ALIGN = {                             # float offsets of (p, g, m, v) from a 16-byte aligned base, for tensor number i
    "aligned": lambda i: (0, 0, 0, 0),
    "g_off": lambda i: (0, 1 + i % 3, 0, 0),                  # the ddp.FlatAllReduce case
    "p_off": lambda i: (1 + i % 3, 0, 0, 0),
    "all_off": lambda i: (1 + i % 3, 1 + (i + 1) % 3, 1 + (i + 2) % 3, 1 + i % 3),
}
HYPER = [                             # lr, beta1, beta2, eps, t
    (1e-3, 0.9, 0.999, 1e-8, 1),
    (1e-3, 0.9, 0.999, 1e-8, 1000),
    (1e-4, 0.9, 0.999, 1e-8, 100000),
    (1e-2, 0.5, 0.9, 1e-3, 3),
    (1e-3, 0.0, 0.999, 1e-8, 2),
    (1e-3, 0.9, 0.0, 1e-8, 2),
]


def dev():
    return torch.device("cuda:0")


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L


def chunk():
    return int(_lib().get_lib().dfe_adam_chunk())


def sizes():
    """1, 3, 255, 1023, 4095, 4096, 4097, 8192, 8192 + 5 -- and the same edges of whatever the library's chunk is."""
    c = chunk()
    return sorted({1, 3, 255, 1023, 4095, 4096, 4097, 8192, 8192 + 5, c - 1, c, c + 1, 2 * c, 2 * c + 5})


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """fp32 p, g, m, v of one tensor (read-only, shared by every test): p = N(0,1) 10^[-3,2]; g = N(0,1) 10^[-12,7] with
    a run of exact zeros; m of g's magnitude, either sign; v of g^2's magnitude; from 255 elements on, five gradients of
    1e25 (g^2 overflows fp32), the last element among them."""
    r = np.random.default_rng(1000 + n)
    p = r.standard_normal(n) * 10.0 ** r.uniform(-3, 2, n)
    mag = 10.0 ** r.uniform(-12, 7, n)
    g = r.standard_normal(n) * mag
    m = r.standard_normal(n) * mag
    v = r.chisquare(1, n) * mag * mag
    if n >= 3:
        a = n // 3
        g[a:a + max(1, n // 8)] = 0.0
    if n >= 255:
        big = np.array([0, 129, n // 2, n - 2, n - 1])
        g[big] = 1e25
        m[big] = r.standard_normal(5) * 1e25
        v[big] = r.chisquare(1, 5) * 1e30
    out = tuple(np.ascontiguousarray(x, dtype=np.float32) for x in (p, g, m, v))
    for x in out:
        x.setflags(write=False)
    assert np.isfinite(np.stack(out)).all() and (out[3] >= 0).all()
    return out


class Carved:
    """``values`` as a view that starts ``off`` floats past a 16-byte boundary, inside a buffer pre-filled with SENTINEL."""

    def __init__(self, values, off):
        n = len(values)
        self.buf = torch.empty(n + 2 * PAD + 3, dtype=torch.float32, device=dev())
        assert self.buf.data_ptr() % 16 == 0
        self.buf.view(torch.int32).fill_(SENTINEL)
        self.lo, self.n = PAD + off, n
        self.view = self.buf[self.lo:self.lo + n]
        self.view.copy_(torch.from_numpy(values.copy()))         # (the cached inputs are read-only arrays)
        assert self.view.data_ptr() % 16 == 4 * off

    def guards_intact(self):
        bits = self.buf.view(torch.int32)
        return bool((bits[:self.lo] == SENTINEL).all()) and bool((bits[self.lo + self.n:] == SENTINEL).all())

    def numpy(self):
        return self.view.cpu().numpy()


class Launch:
    """The tensors of one launch, carved, with the table and block map built the way FusedAdam._plan builds them."""

    def __init__(self, ns, align):
        self.ns = list(ns)
        self.t = [[Carved(x, o) for x, o in zip(_inputs(n), ALIGN[align](i))] for i, n in enumerate(self.ns)]
        c = chunk()
        rows = [[q.view.data_ptr() for q in quad] + [n] for quad, n in zip(self.t, self.ns)]
        blocks = [[i, k] for i, n in enumerate(self.ns) for k in range((n + c - 1) // c)]
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev())
        self.blockmap = torch.tensor(blocks, dtype=torch.int32).to(dev())
        self.nblocks = len(blocks)

    def args(self):
        return ctypes.c_void_p(self.table.data_ptr()), ctypes.c_void_p(self.blockmap.data_ptr()), self.nblocks

    def step(self, lr, b1, b2, eps, t):
        L = _lib()
        L.check(L.get_lib().dfe_adam_step(*self.args(), lr, b1, b2, eps, 1.0 - b1 ** t, 1.0 - b2 ** t, L.stream_ptr()),
                "dfe_adam_step")
        torch.cuda.synchronize()

    def step_dev(self, lr, b1, b2, eps, count, coef):
        L = _lib()
        L.check(L.get_lib().dfe_adam_step_dev(*self.args(), lr, b1, b2, eps, ctypes.c_void_p(count.data_ptr()),
                                              ctypes.c_void_p(coef.data_ptr()), L.stream_ptr()), "dfe_adam_step_dev")
        torch.cuda.synchronize()

    def check(self, lr, b1, b2, eps, t, what=""):
        worst = np.zeros(3)
        for i, (quad, n) in enumerate(zip(self.t, self.ns)):
            assert all(q.guards_intact() for q in quad), "%s tensor %d (n = %d): a guard float was written" % (what, i, n)
            worst = np.maximum(worst, check_step(_inputs(n), [q.numpy() for q in quad], lr, b1, b2, eps, t,
                                                 "%s tensor %d (n = %d)" % (what, i, n)))
        return worst


def check_step(before, after, lr, b1, b2, eps, t, what=""):
    """One Adam step ``before`` -> ``after`` (fp32 p, g, m, v each) against the float64 recurrence of the same fp32 inputs
    and the true double hyper-parameters.  Returns the worst error of m, v, p in units of its bound's u-coefficient."""
    P, G, M, V = (np.asarray(x, dtype=np.float64) for x in before)
    p1, g1, m1, v1 = (np.asarray(x) for x in after)
    assert all(x.dtype == np.float32 for x in (p1, g1, m1, v1))
    assert np.array_equal(g1.view(np.int32), np.asarray(before[1]).view(np.int32)), what + ": the gradient was written"
    pk, mk, vk = p1.astype(np.float64), m1.astype(np.float64), v1.astype(np.float64)
    M1 = M + (1.0 - b1) * (G - M)
    V1 = b2 * V + (1.0 - b2) * G * G
    # m = m + fl(1-b1) * (g - m): the subtraction rounds once (<= u |g - m|), fl(1-b1) and the product once each on a term
    # of size (1-b1) |g - m|, the sum once (<= u |m'|, and |m'| <= max(|m|, |g|) up to those roundings): (3 (1-b1) + 1) u (|m| + |g|)
    bound_m = 4.0 * U * (np.abs(M) + np.abs(G))
    err_m = np.abs(mk - M1)
    assert (err_m <= bound_m).all(), "%s: exp_avg off by %.2f u (|m| + |g|), bound 4" % (what, np.max(err_m / np.maximum(bound_m / 4, 1e-300)))
    # v = fl(b2) * v + fl(1-b2) * g * g: two roundings on the first term, three on the second, one for the sum; both terms
    # are >= 0, so the relative errors do not amplify: (1 + u)^4 - 1 < 6 u; a result in the subnormal range adds <= TINY
    with np.errstate(over="ignore"):
        over = np.isinf(V1.astype(np.float32))
    assert (vk[over] == np.inf).all(), what + ": exp_avg_sq must overflow to +inf where float32(float64 result) does"
    fin = ~over
    bound_v = 6.0 * U * V1[fin] + TINY
    err_v = np.abs(vk[fin] - V1[fin])
    assert (err_v <= bound_v).all(), "%s: exp_avg_sq off by %.2f u v, bound 6" % (what, np.max((err_v - TINY) / np.maximum(U * V1[fin], 1e-300)))
    # p = p - step_size * m / (sqrtf(v) / c2s + eps) from the kernel's OWN m', v' (a cancellation in m stays out of this bound):
    # step_size, c2s, eps are rounded once each, then sqrtf, the division by c2s, the sum with eps, step_size * m and the final
    # division round once each: 8 roundings on the update U; the subtraction rounds once: u |P1|
    with np.errstate(divide="ignore"):
        upd = (lr / (1.0 - b1 ** t)) * mk / (np.sqrt(vk) / math.sqrt(1.0 - b2 ** t) + eps)
    P1 = P - upd
    bound_p = U * np.abs(P1) + 8.0 * U * np.abs(upd) + TINY
    err_p = np.abs(pk - P1)
    assert np.isfinite(pk).all(), what + ": a parameter is not finite"
    assert (err_p <= bound_p).all(), "%s: parameter off by %.2f (in units of u |U|), bound 8" % (
        what, np.max((err_p - U * np.abs(P1) - TINY) / np.maximum(U * np.abs(upd), 1e-300)))
    # where g^2 overflowed the denominator is inf and the update exactly 0: p unchanged (to the one rounding of p - 0)
    assert (np.abs(pk[over] - P[over]) <= U * np.abs(P[over])).all(), what + ": an overflowed gradient moved its parameter"
    with np.errstate(divide="ignore", invalid="ignore"):
        wm = np.max(np.where(bound_m > 0, err_m / (bound_m / 4.0), 0.0))
        wv = np.max(np.where(V1[fin] > 0, (err_v - TINY) / (U * V1[fin]), 0.0)) if fin.any() else 0.0
        wp = np.max(np.where(np.abs(upd) > 0, (err_p - U * np.abs(P1) - TINY) / (U * np.abs(upd)), 0.0))
    return np.array([wm, wv, wp])


# ------------------------------------------------------------------ A

@pytest.mark.parametrize("hyper", HYPER, ids=lambda h: "lr%g-b%g-%g-eps%g-t%d" % h)
@pytest.mark.parametrize("align", list(ALIGN))
def test_adam_kernel_one_step_vs_float64(align, hyper):
    """dfe_adam_step on nine tensors in one launch (every size of ``sizes()``), within the counted fp32 bounds of
    ``check_step`` and without touching a float outside its views.  Emulating the kernel's fp32 arithmetic in numpy over
    these value ranges gives a worst case of 2.0 u (m), 2.4 u (v), 4.2 u (p) against the bounds' 4, 6, 8."""
    launch = Launch(sizes(), align)
    launch.step(*hyper)
    worst = launch.check(*hyper, what="%s %s" % (align, hyper))
    print("\nadam one step %s %s: worst m %.2f u(|m|+|g|) [4], v %.2f u v [6], p %.2f u |U| [8]" % ((align, hyper) + tuple(worst)))


def test_adam_kernel_arguments_are_checked():
    """NULL tables, an empty grid and non-positive bias corrections are refused before anything is launched."""
    L = _lib()
    lib = L.get_lib()
    launch = Launch([5], "aligned")
    a = launch.args()
    assert lib.dfe_adam_step(None, a[1], 1, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, L.stream_ptr()) != 0
    assert lib.dfe_adam_step(a[0], a[1], 0, 1e-3, 0.9, 0.999, 1e-8, 0.1, 0.001, L.stream_ptr()) != 0
    assert lib.dfe_adam_step(a[0], a[1], 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.001, L.stream_ptr()) != 0
    assert lib.dfe_adam_step_dev(a[0], a[1], 1, 1e-3, 0.9, 0.999, 1e-8, None, None, L.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert all(np.array_equal(q.numpy(), x) for q, x in zip(launch.t[0], _inputs(5)))


# ------------------------------------------------------------------ B

@pytest.mark.parametrize("t0", [0, 1, 9, 999, 99999])
def test_adam_device_count_and_coefficients(t0):
    """dfe_adam_step_dev: the count advances by exactly one per call without the host touching it, the coefficients it forms
    are the host's doubles rounded to fp32 (to 1 ulp: the device's double pow need not match the host's last bit), and the
    update is the one dfe_adam_step makes from the same state at the same t -- m and v bit for bit (they do not depend on the
    coefficients), p within the bound of A."""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    c = chunk()
    ns = [3, 1023, c, c + 1, 2 * c + 5]
    host, devc = Launch(ns, "g_off"), Launch(ns, "g_off")
    t = t0 + 1
    host.step(lr, b1, b2, eps, t)
    count = torch.full((1,), float(t0), dtype=torch.float64, device=dev())
    coef = torch.zeros(2, dtype=torch.float32, device=dev())
    devc.step_dev(lr, b1, b2, eps, count, coef)
    assert float(count.cpu()[0]) == t
    got = coef.cpu().numpy()
    want = np.array([lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)]).astype(np.float32)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64)).all(), (got, want)
    for qh, qd in zip(host.t, devc.t):
        assert torch.equal(qh[2].view.view(torch.int32), qd[2].view.view(torch.int32))      # exp_avg
        assert torch.equal(qh[3].view.view(torch.int32), qd[3].view.view(torch.int32))      # exp_avg_sq
    worst = devc.check(lr, b1, b2, eps, t, what="device count %d" % t0)
    print("\nadam device count t0 = %d: coef %s (host %s), worst p %.2f u |U| [8]" % (t0, got, want, worst[2]))
    for _ in range(3):
        devc.step_dev(lr, b1, b2, eps, count, coef)
    assert float(count.cpu()[0]) == t0 + 4
    t = t0 + 4
    want = np.array([lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)]).astype(np.float32)
    got = coef.cpu().numpy()
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(want).astype(np.float64)).all(), (got, want)
    assert all(q.guards_intact() for quad in devc.t for q in quad)


# ------------------------------------------------------------------ C

STEPS, LR_CHANGE_AT = 50, 25
GROUPS = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8), dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-6)]


def _traj_shapes():
    c = chunk()
    return [[(1,), (3,), (255,), (c - 1,), (c + 1,), (2 * c + 5,)],          # group 0: gradients are views of one flat buffer
            [(1023,), (c,), (2 * c,), (64, 65)]]                             # group 1: the last one gets a transposed gradient


def _lr_at(gi, it):
    return GROUPS[gi]["lr"] * (0.5 if (gi == 0 and it >= LR_CHANGE_AT) else 1.0)


@functools.lru_cache(maxsize=None)
def _trajectory():
    """Initial parameters, the 50 gradients per parameter (fp32, on the host), the float64 trajectory's end state and
    torch.optim.Adam(foreach=False, fused=False)'s on the device from the same gradients: computed once."""
    r = np.random.default_rng(77)
    shapes = _traj_shapes()
    p0 = [[r.standard_normal(s).astype(np.float32) for s in grp] for grp in shapes]
    scale = [[10.0 ** r.uniform(-3, 1) for _ in grp] for grp in shapes]
    grads = [[[(r.standard_normal(s) * scale[gi][k] * 10.0 ** r.uniform(-1, 1)).astype(np.float32) for k, s in enumerate(grp)]
              for gi, grp in enumerate(shapes)] for _ in range(STEPS)]
    ref = []
    for gi, grp in enumerate(shapes):
        (b1, b2), eps = GROUPS[gi]["betas"], GROUPS[gi]["eps"]
        out = []
        for k in range(len(grp)):
            P, M, V = p0[gi][k].astype(np.float64), 0.0, 0.0
            for it in range(STEPS):
                G, t = grads[it][gi][k].astype(np.float64), it + 1
                M = M + (1.0 - b1) * (G - M)
                V = b2 * V + (1.0 - b2) * G * G
                P = P - (_lr_at(gi, it) / (1.0 - b1 ** t)) * M / (np.sqrt(V) / math.sqrt(1.0 - b2 ** t) + eps)
            out.append((P, M, V))
        ref.append(out)
    params = [[torch.from_numpy(x).to(dev()).requires_grad_(True) for x in grp] for grp in p0]
    opt = torch.optim.Adam([dict(params=ps, **GROUPS[gi]) for gi, ps in enumerate(params)], foreach=False, fused=False)
    for it in range(STEPS):
        opt.param_groups[0]["lr"] = _lr_at(0, it)
        for gi, ps in enumerate(params):
            for k, p in enumerate(ps):
                p.grad = torch.from_numpy(grads[it][gi][k]).to(dev())
        opt.step()
    torch.cuda.synchronize()
    return p0, grads, ref, _traj_errors(params, opt, ref)


def _traj_errors(params, opt, ref):
    """Worst error to float64 over all tensors, each tensor's error relative to its own largest reference value:
    [parameter, exp_avg, exp_avg_sq]."""
    worst = np.zeros(3)
    for gi, ps in enumerate(params):
        for k, p in enumerate(ps):
            got = (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])
            for j in range(3):
                e = np.abs(got[j].cpu().numpy().astype(np.float64) - ref[gi][k][j]).max() / np.abs(ref[gi][k][j]).max()
                worst[j] = max(worst[j], e)
    return worst


@pytest.mark.parametrize("capturable", [False, True], ids=["host_count", "device_count"])
def test_fused_adam_trajectory_vs_float64(capturable):
    """FusedAdam, 50 steps, two param groups with different lr / betas / eps, group 0's lr halved at step 25 as a scheduler
    would, gradients handed over as views at odd float offsets of one flat buffer (group 0) and as a transposed matrix
    (group 1's last parameter); ``capturable=True`` runs the same through one device count per group.

    Its error to the float64 recurrence is held to torch.optim.Adam(foreach=False, fused=False)'s on the same device and
    gradients: both are fp32 evaluations of one recurrence that differ in association only, so their errors are random walks
    of one size; 2 x torch's error + 4 u of the tensor's scale.  Errors are per tensor relative to its largest reference
    value, the worst tensor counts.  Measured on an MI355X, FusedAdam / torch.optim.Adam in u (the same figures for both
    values of ``capturable``): parameter 6.32 / 6.32 (ratio 1.00), exp_avg 4.11 / 2.61 (1.58), exp_avg_sq 11.13 / 12.00 (0.93);
    EXPERIMENT_LOG.md, "FusedAdam against float64"."""
    from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
    p0, grads, ref, err_torch = _trajectory()
    params = [[torch.from_numpy(x).to(dev()).requires_grad_(True) for x in grp] for grp in p0]
    opt = FusedAdam([dict(params=ps, **GROUPS[gi]) for gi, ps in enumerate(params)], capturable=capturable)
    # group 0's flat gradient buffer: every view starts at an ODD float offset (4 bytes past an 8-byte boundary)
    offs, off = [], 1
    for p in params[0]:
        offs.append(off)
        off += p.numel()
        off += 1 - off % 2
    flat = torch.zeros(off, device=dev())
    views = [flat[o:o + p.numel()].view_as(p) for o, p in zip(offs, params[0])]
    assert all(v.data_ptr() % 8 == 4 for v in views)
    for it in range(STEPS):
        opt.param_groups[0]["lr"] = _lr_at(0, it)
        for k, p in enumerate(params[0]):
            views[k].copy_(torch.from_numpy(grads[it][0][k]))
            p.grad = views[k]
        for k, p in enumerate(params[1]):
            g = torch.from_numpy(grads[it][1][k]).to(dev())
            if k == len(params[1]) - 1:
                g = g.t().contiguous().t()
                assert not g.is_contiguous()
            p.grad = g
        opt.step()
    torch.cuda.synchronize()
    assert all(g["capturable"] is capturable for g in opt.param_groups)
    err = _traj_errors(params, opt, ref)
    print("\nfused adam trajectory (capturable=%s): error to float64 in u, FusedAdam p %.2f m %.2f v %.2f; torch.optim.Adam "
          "p %.2f m %.2f v %.2f; ratios %s" % ((capturable,) + tuple(err / U) + tuple(err_torch / U) + (np.round(err / err_torch, 3),)))
    for j, name in enumerate(("parameter", "exp_avg", "exp_avg_sq")):
        assert err[j] <= 2.0 * err_torch[j] + 4.0 * U, (name, err[j] / U, err_torch[j] / U)
    sd = opt.state_dict()
    n = sum(len(ps) for ps in params)
    assert len(sd["state"]) == n and all(float(sd["state"][i]["step"]) == STEPS for i in range(n))
    assert all(not st["step"].is_cuda for st in opt.state.values())
    # the checkpoint loads into torch.optim.Adam and comes back out of it unchanged
    twins = [[p.detach().clone().requires_grad_(True) for p in ps] for ps in params]
    ot = torch.optim.Adam([dict(params=ps, **GROUPS[gi]) for gi, ps in enumerate(twins)], foreach=False, fused=False)
    ot.load_state_dict(copy.deepcopy(sd))
    back = ot.state_dict()
    for i in range(n):
        assert float(back["state"][i]["step"]) == STEPS
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][key], sd["state"][i][key])
    assert [g["lr"] for g in ot.param_groups] == [_lr_at(0, STEPS - 1), _lr_at(1, STEPS - 1)]
    for ps in twins:
        for p in ps:
            p.grad = torch.ones_like(p)
    ot.step()                                       # and torch steps from it: count 51
    torch.cuda.synchronize()
    assert all(float(st["step"]) == STEPS + 1 for st in ot.state.values())
    assert all(bool(torch.isfinite(p).all()) for ps in twins for p in ps)


# ------------------------------------------------------------------ D

N_EAGER, K = 7, 4
LR = 1e-3


class Toy(torch.nn.Module):
    """loss = sum_i (w_i * x_i).sum(): dloss/dw_i = x_i, whatever w is -- no atomics, nothing that depends on the
    parameters, so a replayed step and an eager step see the SAME gradient bits."""

    def __init__(self, init):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in init])

    def forward(self, inputs):
        loss = (self.w[0] * inputs[0]).sum()
        for w, x in zip(list(self.w)[1:], inputs[1:]):
            loss = loss + (w * x).sum()
        return {"loss_depth_pixel": loss}, {}


@functools.lru_cache(maxsize=None)
def _toy_data():
    c = chunk()
    ns = [1, 3, c - 1, c, c + 1, 2 * c + 5]
    gen = torch.Generator().manual_seed(11)
    init = [torch.randn(n, generator=gen) for n in ns]
    # N_EAGER + 2 K batches, every one different (and of a different size: Adam's moments must follow)
    batches = [[torch.randn(n, generator=gen) * 10.0 ** ((i % 5) - 2) for n in ns] for i in range(N_EAGER + 2 * K)]
    return init, batches


def _toy(init=None, model_state=None):
    m = Toy(_toy_data()[0] if init is None else init).to(dev())
    if model_state is not None:
        m.load_state_dict(model_state)
    return m


def _batch(i):
    return [t.to(dev()) for t in _toy_data()[1][i]]


def _eager(model, opt, first, count):
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import make_cfg, train_step
    cfg = make_cfg()
    for i in range(first, first + count):
        train_step(model, opt, _batch(i), cfg)
    torch.cuda.synchronize()


def _fused(model, capturable):
    from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
    return FusedAdam(list(model.parameters()), lr=LR, capturable=capturable)


def _moments(model, opt):
    return [(opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in model.parameters()]


@functools.lru_cache(maxsize=None)
def _checkpoints():
    """The checkpoints the matrix starts from, each (model state, optimiser state, step count, next batch):
    ``fused``: N eager FusedAdam steps; ``torch``: the same with torch.optim.Adam; ``graph``: ``fused`` loaded into a capturable
    FusedAdam and advanced by K replays (written by ``test_resume_matrix[fused]``'s own code path, see ``_resume``)."""
    out = {}
    for name in ("fused", "torch"):
        model = _toy()
        opt = _fused(model, False) if name == "fused" else torch.optim.Adam(list(model.parameters()), lr=LR)
        _eager(model, opt, 0, N_EAGER)
        out[name] = (copy.deepcopy(model.state_dict()), copy.deepcopy(opt.state_dict()), N_EAGER, N_EAGER)
    model, opt = _resume(out["fused"], graph=True, check=False)
    out["graph"] = (copy.deepcopy(model.state_dict()), copy.deepcopy(opt.state_dict()), N_EAGER + K, N_EAGER + K)
    assert all(g["capturable"] is True for g in out["graph"][1]["param_groups"])
    return out


def _steps_of(opt):
    sd = opt.state_dict()
    return [float(sd["state"][i]["step"]) for i in range(len(sd["state"]))]


def _resume(ckpt, graph, check=True):
    """Load ``ckpt`` into a fresh model + FusedAdam(capturable=graph), run K steps on the next K batches (replays of a
    GraphedTrainStep, or eager steps) and, with ``check``, hold every step of the way against an eager
    FusedAdam(capturable=False) twin started from the same checkpoint."""
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import GraphedTrainStep, make_cfg
    model_state, opt_state, n0, first = ckpt
    model = _toy(model_state=model_state)
    opt = _fused(model, graph)
    opt.load_state_dict(copy.deepcopy(opt_state))
    assert all(g["capturable"] is graph for g in opt.param_groups)
    assert all(not st["step"].is_cuda and st["step"].dtype == torch.float32 for st in opt.state.values())
    assert _steps_of(opt) == [float(n0)] * len(list(model.parameters()))
    if graph:
        before = [p.detach().clone() for p in model.parameters()]
        g = GraphedTrainStep(model, opt, _batch(0), make_cfg(), warmup=3, restore=True)
        try:
            torch.cuda.synchronize()
            assert _steps_of(opt) == [float(n0)] * len(before)              # constructing it trains nothing and counts nothing
            assert all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
            for i in range(first, first + K):
                g(_batch(i))
            torch.cuda.synchronize()
        finally:
            del g
            torch.cuda.synchronize()
    else:
        _eager(model, opt, first, K)
    assert _steps_of(opt) == [float(n0 + K)] * len(list(model.parameters()))
    assert all(g["capturable"] is graph for g in opt.param_groups)
    assert all(not st["step"].is_cuda for st in opt.state.values())
    if check:
        twin = _toy(model_state=model_state)
        opt_t = _fused(twin, False)
        opt_t.load_state_dict(copy.deepcopy(opt_state))
        _eager(twin, opt_t, first, K)
        assert _steps_of(opt_t) == [float(n0 + K)] * len(list(twin.parameters()))
        for (m, v), (mt, vt) in zip(_moments(model, opt), _moments(twin, opt_t)):
            assert torch.equal(m, mt) and torch.equal(v, vt)                 # the same gradients through the same arithmetic
        for p, pt, p_start in zip(model.parameters(), twin.parameters(), model_state.values()):
            # the device's coefficients may differ from the host's by 1 ulp: <= 1 ulp of p per step; 2 x that
            assert float((p - pt).abs().max()) <= K * 2.0 ** -22 * float(pt.abs().max())
            assert float((pt.detach() - p_start.to(dev())).abs().max()) > 0.5 * LR      # ... of parameters that did move
    return model, opt


@pytest.mark.parametrize("source,graph", [("fused", True), ("torch", True), ("graph", True), ("graph", False)],
                         ids=["eager_to_graph", "torch_adam_to_graph", "graph_to_graph", "graph_to_eager"])
def test_resume_matrix(source, graph):
    """Checkpoints are interchangeable between the eager step, the graphed step and torch.optim.Adam, and the mode is the
    constructor's, never the checkpoint's: N = 7 eager steps (or N + K, for a checkpoint written after replays), then K = 4
    steps on K different batches.  Right after the GraphedTrainStep is built the count is still N; after the K steps it is
    N + K; the moments are bit-equal to an eager twin's from the same checkpoint and the parameters within K 2^-22 max|p|
    (a bias correction frozen at the captured step, or restarted at t = 1, moves p by percents of lr = 1e-3 per step); the
    live groups keep the constructor's ``capturable`` and every ``step`` stays a host tensor."""
    model, opt = _resume(_checkpoints()[source], graph)
    if source != "torch":
        # ... and equal to ONE eager FusedAdam run from scratch over the same batches (no checkpoint in between)
        n = _checkpoints()[source][2] + K
        chain = _toy()
        opt_c = _fused(chain, False)
        _eager(chain, opt_c, 0, n)
        for (m, v), (mc, vc) in zip(_moments(model, opt), _moments(chain, opt_c)):
            assert torch.equal(m, mc) and torch.equal(v, vc)
        for p, pc in zip(model.parameters(), chain.parameters()):
            assert float((p - pc).abs().max()) <= n * 2.0 ** -22 * float(pc.abs().max())


@pytest.mark.parametrize("kind", ["fused", "torch"])
def test_graphed_step_refuses_a_non_capturable_optimiser(kind):
    """A non-capturable Adam takes its bias corrections as kernel arguments: captured, they would stay those of the captured
    step.  GraphedTrainStep says so before it runs a warm-up step or captures anything."""
    from unsupervised_depth_opticalflow_egomotion_amd.train_step import GraphedTrainStep, make_cfg
    model = _toy()
    opt = _fused(model, False) if kind == "fused" else torch.optim.Adam(list(model.parameters()), lr=LR)
    before = [p.detach().clone() for p in model.parameters()]
    with pytest.raises(ValueError, match="capturable"):
        GraphedTrainStep(model, opt, _batch(0), make_cfg())
    torch.cuda.synchronize()
    assert not torch.cuda.is_current_stream_capturing()
    assert len(opt.state) == 0 and all(torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    # one capturable group among several is not enough
    if kind == "fused":
        from unsupervised_depth_opticalflow_egomotion_amd.optim import FusedAdam
        ps = list(model.parameters())
        mixed = FusedAdam([dict(params=ps[:2]), dict(params=ps[2:], capturable=False)], lr=LR, capturable=True)
        with pytest.raises(ValueError, match="capturable"):
            GraphedTrainStep(model, mixed, _batch(0), make_cfg())
        assert len(mixed.state) == 0
