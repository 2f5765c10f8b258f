"""Helpers of the guarded geometry / resize / splat / 1x1 tests (test_hip_geom_guarded.py, test_hip_resize_guarded.py, the
conv1x1_small part of test_hip_planeconv_guarded.py; cases: tests/geom_cases.py; self-tests in test_guarded_cpu.py).  Not a
conftest: imported explicitly.

Float64 references written plainly for these tests -- NOT oracle/loss_stack_oracle.py, which restates the fp32 arithmetic on
purpose and stays the fp32 yardstick and the side of every bit-equality check: the pose matrices, the pinhole projection ->
normalised grid -> zero-padded bilinear sample (differentiated by float64 autograd), the box SSIM, the bilinear resize and its
exact adjoint, the area resize, the forward splat, the 1x1 convolution, the triplet preparation.  Next to them the input
builders that keep every decision of a case MARGIN away from its threshold: asserted on the host before anything is launched.

The bound of a chain-rule gradient (no simple per-element absolute sum): e = max |out - ref64| / (2^-24 max |ref64|) per sample,
held to 4 max(1, e of fp32 autograd through the oracle on the host, same inputs)."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import guarded as G

F32, F64 = torch.float32, torch.float64
U24, MARGIN = G.U24, G.MARGIN
NUDGE = 1.0 + 2.0 ** -7
Z_MIN = 1e-3


# --------------------------------------------------------------------------------------------------------- pose matrices
def euler_ref(ang):
    """R = Rx Ry Rz of ang [n,3], in ang's dtype"""
    rx, ry, rz = ang[:, 0], ang[:, 1], ang[:, 2]
    o, z = torch.ones_like(rx), torch.zeros_like(rx)
    m = lambda *v: torch.stack(v, 1).reshape(-1, 3, 3)
    X = m(o, z, z, z, torch.cos(rx), -torch.sin(rx), z, torch.sin(rx), torch.cos(rx))
    Y = m(torch.cos(ry), z, torch.sin(ry), z, o, z, -torch.sin(ry), z, torch.cos(ry))
    Z = m(torch.cos(rz), -torch.sin(rz), z, torch.sin(rz), torch.cos(rz), z, z, z, o)
    return X @ Y @ Z


def pose_mats_ref(vec):
    """(T34 [n,3,4] = [R | t], E [n,3,3] = [t]x R) of vec [n,6] = (t, euler angles)"""
    R, t = euler_ref(vec[:, 3:]), vec[:, :3]
    z = torch.zeros_like(t[:, 0])
    S = torch.stack([z, -t[:, 2], t[:, 1], t[:, 2], z, -t[:, 0], -t[:, 1], t[:, 0], z], 1).reshape(-1, 3, 3)
    return torch.cat([R, t[:, :, None]], 2), S @ R


def pose_mats_vjp_ref(vec, gT34, gE):
    """float64 vector-Jacobian product: gvec [n,6] (gT34 / gE may be None)"""
    v = vec.double().clone().requires_grad_(True)
    T34, E = pose_mats_ref(v)
    loss = 0.0
    if gT34 is not None:
        loss = loss + (T34 * gT34.double()).sum()
    if gE is not None:
        loss = loss + (E * gE.double()).sum()
    return torch.autograd.grad(loss, v)[0]


def chain_err(out, ref64):
    """per sample (dim 0): max |out - ref64| / (2^-24 max |ref64|); a sample whose reference is all zero must be all zero"""
    out, ref64 = out.detach().double().cpu().flatten(1), ref64.detach().double().flatten(1)
    num, den = (out - ref64).abs().amax(1), ref64.abs().amax(1)
    zero = den == 0
    assert bool((num[zero] == 0).all()), "non-zero output where the reference is identically zero"
    e = num / (U24 * den.clamp_min(1e-300))
    return float(e[~zero].max()) if bool((~zero).any()) else 0.0


def check_chain(tag, out, yard, ref64):
    assert out.shape == ref64.shape == yard.shape, (tag, out.shape, yard.shape, ref64.shape)
    assert bool(torch.isfinite(out).all()), tag
    ek, ey = chain_err(out, ref64), chain_err(yard, ref64)
    print("EBOUND %s kernel %.3f yardstick %.3f" % (tag, ek, ey))
    assert ek <= 4.0 * max(1.0, ey), (tag, ek, ey)
    return ek, ey


# --------------------------------------------------------------------------------------------------------- projection and sampling
def unnormalize_ref(g, size, ac):
    return (g + 1.0) * ((size - 1) / 2.0) if ac else (g + 1.0) * (size / 2.0) - 0.5


def bilinear_zero_ref(img, ix, iy):
    """img [B,C,H,W] sampled at pixel coordinates ix, iy [B,N] with zero padding -> [B,C,N]; differentiable in img, ix, iy"""
    B, C, H, W = img.shape
    x0, y0 = torch.floor(ix.detach()), torch.floor(iy.detach())
    wx, wy = ix - x0, iy - y0
    flat = img.reshape(B, C, H * W)
    out = 0.0
    for dy, dx, w in ((0, 0, (1 - wy) * (1 - wx)), (0, 1, (1 - wy) * wx), (1, 0, wy * (1 - wx)), (1, 1, wy * wx)):
        xx, yy = x0 + dx, y0 + dy
        inb = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= H - 1)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long()
        out = out + flat.gather(2, idx[:, None, :].expand(B, C, -1)) * (w * inb.to(img.dtype))[:, None, :]
    return out


def project_ref(depth, pose, K):
    """float64 pinhole projection of every pixel: (X, Y, Zraw, absZ) [B,HW]; absZ = the absolute sum behind Zraw"""
    B, _, H, W = depth.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    pix = torch.stack([xs, ys, torch.ones_like(xs)]).reshape(1, 3, H * W)
    cam = (torch.linalg.inv(K) @ pix) * depth.reshape(B, 1, H * W)
    T34, _ = pose_mats_ref(pose)
    P = K @ T34
    p = P[:, :, :3] @ cam + P[:, :, 3:]
    absz = (P[:, 2:3, :3].abs() @ cam.abs() + P[:, 2:3, 3:].abs())[:, 0]
    return p[:, 0], p[:, 1], p[:, 2], absz.detach()


def inverse_warp2_ref(img, depth, ref_depth, pose, K, ac):
    """float64 inverse_warp2 on float64 (possibly requires_grad) tensors.  dict: img [B,3,H,W], valid, pdepth, cdepth [B,1,H,W]
    and what the safety conditions look at: ix, iy (pixel coordinates after the zero-padding overwrite), xn, yn (normalised,
    before it), live_x, live_y, zraw, absz, vraw (interpolated reference depth before its clamp), all [B,HW]"""
    B, _, H, W = depth.shape
    X, Y, zraw, absz = project_ref(depth, pose, K)
    Z = torch.where(zraw >= Z_MIN, zraw, torch.full_like(zraw, Z_MIN))
    xn, yn = 2.0 * (X / Z) / (W - 1) - 1.0, 2.0 * (Y / Z) / (H - 1) - 1.0
    live_x, live_y = (xn.detach().abs() <= 1.0), (yn.detach().abs() <= 1.0)
    gx, gy = torch.where(live_x, xn, torch.full_like(xn, 2.0)), torch.where(live_y, yn, torch.full_like(yn, 2.0))
    ix, iy = unnormalize_ref(gx, W, ac), unnormalize_ref(gy, H, ac)
    vraw = bilinear_zero_ref(ref_depth, ix, iy)[:, 0]
    pd = torch.where(vraw >= Z_MIN, vraw, torch.full_like(vraw, Z_MIN))
    valid = (torch.maximum(gx.detach().abs(), gy.detach().abs()) <= 1.0).to(F64)
    sh = (B, 1, H, W)
    return dict(img=bilinear_zero_ref(img, ix, iy).reshape(B, -1, H, W), valid=valid.reshape(sh), pdepth=pd.reshape(sh), cdepth=Z.reshape(sh),
                ix=ix.detach(), iy=iy.detach(), xn=xn.detach(), yn=yn.detach(), live_x=live_x, live_y=live_y, zraw=zraw.detach(), absz=absz,
                vraw=vraw.detach())


def rigid_flow_ref(depth, pose, K):
    """float64 calculate_rigid_flow: (flow [B,2,H,W], zraw, absz [B,HW])"""
    B, _, H, W = depth.shape
    X, Y, zraw, absz = project_ref(depth, pose, K)
    Z = torch.where(zraw >= Z_MIN, zraw, torch.full_like(zraw, Z_MIN))
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F64), torch.arange(W, dtype=F64), indexing="ij")
    fl = torch.stack([(X / Z).reshape(B, H, W) - xs, (Y / Z).reshape(B, H, W) - ys], 1)
    return fl, zraw.detach(), absz


def warp_unsafe(depth, ref_depth, pose, K, ac):
    """[B,HW] bool: the pixels of an inverse_warp2 case that break one of the four conditions (float64 reference):
    an in-range coordinate within MARGIN max(H, W) pixels of an integer; a normalised coordinate within that of +-1; the
    pre-clamp Z within MARGIN (of its absolute sum) of 1e-3; the interpolated reference depth within MARGIN (relative) of 1e-3"""
    B, _, H, W = depth.shape
    r = inverse_warp2_ref(torch.zeros(B, 3, H, W, dtype=F64), depth.double(), ref_depth.double(), pose.double(), K.double(), ac)
    tol = MARGIN * max(H, W)
    frac = lambda c: (c - torch.round(c)).abs()
    bad = (r["live_x"] & (frac(r["ix"]) < tol)) | (r["live_y"] & (frac(r["iy"]) < tol))
    bad |= ((r["xn"].abs() - 1.0).abs() < tol) | ((r["yn"].abs() - 1.0).abs() < tol)
    bad |= (r["zraw"] - Z_MIN).abs() < MARGIN * torch.maximum(r["absz"], torch.full_like(r["absz"], Z_MIN))
    bad |= (r["vraw"] - Z_MIN).abs() < MARGIN * torch.maximum(r["vraw"].abs(), torch.full_like(r["vraw"], Z_MIN))
    return bad


def flow_unsafe(depth, pose, K):
    """the rigid flow's one decision: the pre-clamp Z"""
    _, zraw, absz = rigid_flow_ref(depth.double(), pose.double(), K.double())
    return (zraw - Z_MIN).abs() < MARGIN * torch.maximum(absz, torch.full_like(absz, Z_MIN))


def warp_inputs(B, H, W, seed, pose_kind):
    """tests/golden/make_golden.py's g2_inputs for any batch: dict of CPU fp32 tensors img, depth, ref_depth, pose (through
    synthetic.robust_pose: cos and sin unambiguous), K, and the cotangents wi [B,3,H,W], wp, wc [B,1,H,W], wf [B,2,H,W]"""
    from tests.golden import make_golden as MG
    from unsupervised_depth_opticalflow_egomotion_amd import synthetic
    r = MG.rng(seed)
    u = lambda *s: torch.from_numpy(r.random(s).astype(np.float32))
    n = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32))
    img, depth, ref_depth = u(B, 3, H, W), 0.1 + 0.9 * u(B, 1, H, W), 0.1 + 0.9 * u(B, 1, H, W)
    pose = (0.05 * r.standard_normal((B, 6))).astype(np.float32)
    if pose_kind == "identity":
        pose[:] = 0
    elif pose_kind == "oob":
        pose[:, 0], pose[:, 4] = 0.6, 0.3
    elif pose_kind == "clamp":
        pose[:, 2] = -2.0
    else:
        assert pose_kind == "rand"
    pose = torch.from_numpy(synthetic.robust_pose(pose))
    K = torch.from_numpy(MG.kmat(B, max(H, 2), max(W, 2)))
    return dict(img=img, depth=depth, ref_depth=ref_depth, pose=pose, K=K, wi=n(B, 3, H, W), wp=n(B, 1, H, W), wc=n(B, 1, H, W), wf=n(B, 2, H, W))


def safe_warp_inputs(B, H, W, seed, pose_kind, ac, rounds=4):
    """(inputs, unsafe pixels left, unsafe pixels before the nudges): the depth of an offending pixel is multiplied by 1 + 2^-7
    and the conditions are checked again, ``rounds`` times at the most.  A committed gradient case leaves zero."""
    c = warp_inputs(B, H, W, seed, pose_kind)
    first = None
    for _ in range(rounds + 1):
        bad = warp_unsafe(c["depth"], c["ref_depth"], c["pose"], c["K"], ac)
        first = int(bad.sum()) if first is None else first
        if not bool(bad.any()):
            break
        c["depth"] = torch.where(bad.reshape(c["depth"].shape), c["depth"] * NUDGE, c["depth"])
    return c, int(bad.sum()), first


def safe_flow_inputs(B, H, W, seed, pose_kind, rounds=4):
    c = warp_inputs(B, H, W, seed, pose_kind)
    for _ in range(rounds + 1):
        bad = flow_unsafe(c["depth"], c["pose"], c["K"])
        if not bool(bad.any()):
            break
        c["depth"] = torch.where(bad.reshape(c["depth"].shape), c["depth"] * NUDGE, c["depth"])
    return c, int(bad.sum())


def taps_from_coords(ix, iy, H, W):
    """make_tap (csrc/dfe_device.h) in numpy float32 on fp32 pixel coordinates [B,N]: G.warp_taps's dict (w, inb, idx)"""
    f32 = np.float32
    assert ix.dtype == f32 and iy.dtype == f32
    xw, yn = np.floor(ix), np.floor(iy)
    w, n = ix - xw, iy - yn
    e, s = f32(1.0) - w, f32(1.0) - n
    wts = [s * e, s * w, n * e, n * w]
    xin0, xin1 = (xw > -1) & (xw < W), (xw + 1 > -1) & (xw + 1 < W)
    yin0, yin1 = (yn > -1) & (yn < H), (yn + 1 > -1) & (yn + 1 < H)
    inb = [xin0 & yin0, xin1 & yin0, xin0 & yin1, xin1 & yin1]
    x0, y0 = np.clip(xw, -2, W + 1).astype(np.int64), np.clip(yn, -2, H + 1).astype(np.int64)
    idx = [np.where(inb[k], (y0 + k // 2) * W + x0 + k % 2, 0) for k in range(4)]
    assert all(t.dtype == f32 for t in wts)
    return dict(w=wts, inb=inb, idx=idx)


def unnormalize_f32(g, size, ac):
    """unnormalize (csrc/dfe_device.h) on a numpy float32 grid: the one FMA is evaluated in float64 and rounded once"""
    f32 = np.float32
    g1 = g + f32(1.0)
    if ac:
        return g1 * (f32(size - 1) / f32(2.0))
    return (g1.astype(np.float64) * (size / 2.0) - 0.5).astype(f32)


def scatter_ref(taps, g, HW):
    """float64 scatter of the contributions g * w (weights exact fp32 inputs), g [B,N] float64: (ref, mass, count) [B,HW]"""
    B = g.shape[0]
    ref, mass, cnt = (torch.zeros(B, HW, dtype=F64) for _ in range(3))
    for k in range(4):
        w = torch.from_numpy(taps["w"][k]).double() * torch.from_numpy(taps["inb"][k]).double()
        idx = torch.from_numpy(taps["idx"][k])
        for b in range(B):
            ref[b].index_add_(0, idx[b], g[b] * w[b])
            mass[b].index_add_(0, idx[b], g[b].abs() * w[b])
            cnt[b].index_add_(0, idx[b], ((w[b] != 0) & (g[b] != 0)).double())
    return ref, mass, cnt


# --------------------------------------------------------------------------------------------------------- SSIM
def ssim_ref(x, y):
    """3x3 zero-padded box SSIM (divisor always 9), in the inputs' dtype"""
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ones = torch.ones(1, 1, 3, 3, dtype=x.dtype)
    B, C, H, W = x.shape
    box = lambda t: F.conv2d(t.reshape(B * C, 1, H, W), ones, padding=1).reshape(B, C, H, W) / 9.0
    mx, my = box(x), box(y)
    vx, vy, cov = box(x * x) - mx * mx, box(y * y) - my * my, box(x * y) - mx * my
    return ((2 * mx * my + c1) * (2 * cov + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def ssim_loss_gate(s64):
    """the reference's clamp((1 - SSIM) / 2, 0, 1): (pre-clamp value, whether gradient passes)"""
    pre = (1.0 - s64) / 2.0
    return pre, ((pre > 0) & (pre < 1)).to(F64)


def ssim_inputs(shape, seed):
    """x, y in [0,1], y = x + noise; a cotangent; every pre-clamp loss value MARGIN away from 0 and 1 (first seed that does)"""
    for s in range(seed, seed + 40):
        gen = torch.Generator().manual_seed(s)
        x = torch.rand(shape, generator=gen)
        y = (x + 0.1 * torch.randn(shape, generator=gen)).clamp(0, 1)
        wgt = torch.randn(shape, generator=gen)
        pre, _ = ssim_loss_gate(ssim_ref(x.double(), y.double()))
        if bool((pre.abs() >= MARGIN).all()) and bool(((pre - 1.0).abs() >= MARGIN).all()):
            return x, y, wgt, s
    raise AssertionError("no seed keeps the clamp margin")


# --------------------------------------------------------------------------------------------------------- resize
def resize_matrix(n_in, n_out, dtype=F64):
    """[n_out, n_in]: the weights of the bilinear resize with align_corners=False along one axis (the ratio exact)"""
    M = torch.zeros(n_out, n_in, dtype=dtype)
    for o in range(n_out):
        src = max((o + 0.5) * n_in / n_out - 0.5, 0.0)
        i0 = min(int(src), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = src - i0
        M[o, i0] += 1.0 - l1
        M[o, i1] += l1
    return M


def resize_bilinear_ref(x, out_hw, mult=1.0):
    """float64 [P,h,w] -> [P,H,W]: Wy x Wx^T * mult"""
    Wy, Wx = resize_matrix(x.shape[1], out_hw[0]), resize_matrix(x.shape[2], out_hw[1])
    return torch.einsum("oh,phw,qw->poq", Wy, x.double(), Wx) * mult


def resize_adjoint_ref(g, in_hw, mult=1.0, absolute=False):
    """the exact adjoint, float64: gin [P,h,w] = Wy^T g Wx * mult; absolute: sum |w| |g| |mult|"""
    Wy, Wx = resize_matrix(in_hw[0], g.shape[1]), resize_matrix(in_hw[1], g.shape[2])
    g = g.double().abs() if absolute else g.double()
    return torch.einsum("oh,poq,qw->phw", Wy, g, Wx) * (abs(mult) if absolute else mult)


def area_ref(x, out_hw, absolute=False):
    """adaptive average: the mean over [floor(o in / out), ceil((o + 1) in / out)); float64 [P,h,w] -> [P,H,W]"""
    P, h, w = x.shape
    x = x.double().abs() if absolute else x.double()
    out = torch.empty(P, out_hw[0], out_hw[1], dtype=F64)
    for oy in range(out_hw[0]):
        ys, ye = (oy * h) // out_hw[0], -((-(oy + 1) * h) // out_hw[0])
        for ox in range(out_hw[1]):
            xs, xe = (ox * w) // out_hw[1], -((-(ox + 1) * w) // out_hw[1])
            out[:, oy, ox] = x[:, ys:ye, xs:xe].sum((1, 2)) / ((ye - ys) * (xe - xs))
    return out


# --------------------------------------------------------------------------------------------------------- forward splat
def splat_taps(flow):
    """k_forward_splat_ones's targets and weights in numpy float32, operation by operation: tx = x + u, ty = y + v rounded in
    fp32 as the kernel rounds them; G.warp_taps's dict (w, inb, idx), a NaN or fully outside target has no tap"""
    f32 = np.float32
    fl = flow.numpy().astype(f32)
    B, _, H, W = fl.shape
    with np.errstate(invalid="ignore"):
        tx = (np.arange(W, dtype=f32)[None, None, :] + fl[:, 0]).reshape(B, H * W)
        ty = (np.arange(H, dtype=f32)[None, :, None] + fl[:, 1]).reshape(B, H * W)
        live = (tx > -1) & (tx < W) & (ty > -1) & (ty < H)
        tx, ty = np.where(live, tx, f32(0)), np.where(live, ty, f32(0))
        xf, yf = np.floor(tx), np.floor(ty)
        wx, wy = tx - xf, ty - yf
        ex, ey = f32(1.0) - wx, f32(1.0) - wy
        wts = [ex * ey, wx * ey, ex * wy, wx * wy]
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    xa, xb, ya, yb = x0 >= 0, x0 + 1 < W, y0 >= 0, y0 + 1 < H
    inb = [live & xa & ya, live & xb & ya, live & xa & yb, live & xb & yb]
    idx = [np.where(inb[k], (y0 + k // 2) * W + x0 + k % 2, 0) for k in range(4)]
    assert all(t.dtype == f32 for t in wts)
    return dict(w=wts, inb=inb, idx=idx, live=live)


def splat_ref(flow):
    """float64 scatter-add of the four weights of every source pixel: (ref, mass, count) [B,1,H,W]; mass == ref (weights >= 0)"""
    B, _, H, W = flow.shape
    ref, mass, cnt = scatter_ref(splat_taps(flow), torch.ones(B, H * W, dtype=F64), H * W)
    sh = (B, 1, H, W)
    return ref.reshape(sh), mass.reshape(sh), cnt.reshape(sh)


def splat_flow(kind, B, H, W, gen):
    """G.FLOW_KINDS, 'edge' (targets in (-1, 0) and (W-1, W) / (H-1, H): half-inside taps) and 'nan' (one NaN element in an
    otherwise smooth flow)"""
    if kind in G.FLOW_KINDS:
        return G.make_flow(kind, B, H, W, gen)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=F32), torch.arange(W, dtype=F32), indexing="ij")
    if kind == "edge":
        f = torch.zeros(B, 2, H, W)
        tx = torch.where(xs % 2 == 0, torch.full_like(xs, -0.25), torch.full_like(xs, W - 0.75)) - 0.125 * (ys % 3)
        ty = torch.where(ys % 2 == 0, torch.full_like(ys, -0.5), torch.full_like(ys, H - 0.5)) - 0.0625 * (xs % 5)
        f[0::2, 0] = tx - xs                      # even samples: the left and right borders
        f[1::2, 1] = ty - ys                      # odd samples: the top and bottom borders
        if B == 1:
            f[0, 1] = ty - ys
        return f
    assert kind == "nan"
    f = G.make_flow("smooth", B, H, W, gen)
    f[B - 1, 1, H // 2, W // 2] = float("nan")
    return f


# --------------------------------------------------------------------------------------------------------- 1x1 convolution
def conv1x1_ref(x, w, bias, dtype=F64, absolute=False):
    """pre-activation sum_k x[b,k,p] w[n,k] + bias[n]; float32: the serial sum in channel order, one product and one addition
    rounded at a time; absolute: sum |x||w| + |b|"""
    if absolute:
        x, w, bias, dtype = x.abs(), w.abs(), (None if bias is None else bias.abs()), F64
    x, w = x.to(dtype), w.to(dtype)
    if dtype == F64:
        s = torch.einsum("bkhw,nk->bnhw", x, w)
    else:
        s = torch.zeros(x.shape[0], w.shape[0], x.shape[2], x.shape[3], dtype=dtype)
        for k in range(x.shape[1]):
            s = s + x[:, k, None] * w[None, :, k, None, None]
    return s if bias is None else s + bias.to(dtype)[None, :, None, None]


def conv1x1_gx_ref(gy, w, dtype=F64, absolute=False):
    """gx[b,k,p] = sum_n gy[b,n,p] w[n,k]"""
    if absolute:
        gy, w, dtype = gy.abs(), w.abs(), F64
    return conv1x1_ref(gy, w.t(), None, dtype)


def conv1x1_gw_ref(gy, x, dtype=F64, absolute=False):
    """gw[n,k] = sum_{b,p} gy[b,n,p] x[b,k,p]; float32: serial over (b, p)"""
    if absolute:
        gy, x, dtype = gy.abs(), x.abs(), F64
    gy, x = gy.to(dtype).flatten(2), x.to(dtype).flatten(2)
    if dtype == F64:
        return torch.einsum("bnp,bkp->nk", gy, x)
    s = torch.zeros(gy.shape[1], x.shape[1], dtype=dtype)
    for b in range(gy.shape[0]):
        for p in range(gy.shape[2]):
            s = s + gy[b, :, p, None] * x[b, None, :, p]
    return s


def conv1x1_inputs(shape, with_bias, seed):
    """(x, w, bias, gy) with every pre-activation MARGIN (of its absolute sum) away from zero: the first seed that does"""
    B, Ci, Co, H, W = shape
    for s in range(seed, seed + 40):
        gen = torch.Generator().manual_seed(s)
        x, gy = torch.randn(B, Ci, H, W, generator=gen), torch.randn(B, Co, H, W, generator=gen)
        w = torch.randn(Co, Ci, generator=gen) / Ci ** 0.5
        bias = torch.randn(Co, generator=gen) * 0.5 if with_bias else None
        if G.margin_ok(conv1x1_ref(x, w, bias), conv1x1_ref(x, w, bias, absolute=True)):
            return x, w, bias, gy, s
    raise AssertionError("no seed keeps the activation margin")


# --------------------------------------------------------------------------------------------------------- triplets
def triplets_ref(u8, flip, H, W, dtype=np.float64):
    """uint8 [B, 3*H0, W0, 3] -> [B, 3, 3*H, W]: per frame the bilinear resize with half-pixel centres and edge replication, flip
    of the resized frame, / 255, HWC -> CHW; every operation in ``dtype`` (float32: the kernel's expression)"""
    a = u8.numpy().astype(dtype)
    B, H3, W0, _ = a.shape
    H0 = H3 // 3
    t = dtype
    fy = np.clip((np.arange(H, dtype=t) + t(0.5)) * (t(H0) / t(H)) - t(0.5), 0, H0 - 1).astype(t)
    fx = np.clip((np.arange(W, dtype=t) + t(0.5)) * (t(W0) / t(W)) - t(0.5), 0, W0 - 1).astype(t)
    y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
    y1, x1 = np.minimum(y0 + 1, H0 - 1), np.minimum(x0 + 1, W0 - 1)
    wy, wx = (fy - y0).astype(t)[None, :, None, None], (fx - x0).astype(t)[None, None, :, None]
    out = np.empty((B, 3, 3 * H, W), t)
    for f in range(3):
        fr = a[:, f * H0:(f + 1) * H0]
        top = fr[:, y0][:, :, x0] + (fr[:, y0][:, :, x1] - fr[:, y0][:, :, x0]) * wx
        bot = fr[:, y1][:, :, x0] + (fr[:, y1][:, :, x1] - fr[:, y1][:, :, x0]) * wx
        v = ((top + (bot - top) * wy) * (t(1.0) / t(255.0))).astype(t)          # [B,H,W,3]
        for b in range(B):
            vb = v[b, :, ::-1] if (flip is not None and int(flip[b])) else v[b]
            out[b, :, f * H:(f + 1) * H] = vb.transpose(2, 0, 1)
    return torch.from_numpy(out)


# --------------------------------------------------------------------------------------------------------- masks
def mask_inputs(B, H, W, seed):
    """images in [0,1] and flows whose three families of decisions keep MARGIN in float64 (first seed that does).  dict: tgt,
    from_l, from_r (a few pixels of the warps all zero: the validity bits), flow, rigid, and the float64 decisions"""
    for s in range(seed, seed + 40):
        gen = torch.Generator().manual_seed(s)
        tgt, l, r = (torch.rand(B, 3, H, W, generator=gen) for _ in range(3))
        l[0, :, 0, 0] = 0.0
        r[B - 1, :, H - 1, W - 1] = 0.0
        flow, rigid = torch.randn(B, 2, H, W, generator=gen) * 4.0, torch.randn(B, 2, H, W, generator=gen) * 4.0
        d = mask_decisions(tgt, l, r, flow, rigid, 0.01, 0.5)
        if all(G.margin_ok(v, a) for v, a in d["margins"]):
            d.update(tgt=tgt, from_l=l, from_r=r, flow=flow, rigid=rigid, seed=s)
            return d
    raise AssertionError("no seed keeps the mask margins")


def mask_decisions(tgt, l, r, flow, rigid, alpha, beta):
    """float64: occ_bwd, occ_fwd, texture (img = tgt, warped = l, source = r), dyna [B,1,H,W] and (left - right, absolute sum) of
    every decision"""
    t, l, r, fl, rg = (v.double() for v in (tgt, l, r, flow, rigid))
    dl, dr = (t - l).abs().mean(1, True), (t - r).abs().mean(1, True)
    wgt = 1.0 - torch.softmax(torch.cat([dl, dr], 1), 1)
    n2 = lambda v: (torch.sqrt((v * v).sum(1, keepdim=True)) + 1e-12) ** 2
    nd, bound = n2((rg - fl).abs()), alpha * (n2(fl) + n2(rg)) + beta
    one = torch.ones_like(dl)
    return dict(occ_bwd=(wgt[:, 0:1] > 0.48).float(), occ_fwd=(wgt[:, 1:2] > 0.48).float(), texture=(dl < dr).float(), dyna=(nd < bound).float(),
                margins=[(wgt[:, 0:1] - 0.48, one), (wgt[:, 1:2] - 0.48, one), (dl - dr, dl + dr), (nd - bound, nd + bound)])
