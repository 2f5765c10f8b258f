"""GPU: the fused loss stack (dfe_geom_loss_fwd / dfe_geom_loss_bwd of csrc/loss_stack_fwd.hip and loss_stack_bwd.hip) through the C
ABI in guarded, poisoned buffers (tests/guarded.py) on the cases of tests/loss_stack_cases.py: scale widths at the boundaries of the
62- and 60-column strips, last row blocks of 1, 2, 3 and 8 rows, 3-row and 3-column scales, every pyramid and adjoint path, both
operands of the two partial-sum regions that are sized by a maximum, the three modes and the depth-term settings
(test_guarded_cpu.py asserts that coverage through dfe_geom_plan).

The baseline run of a case: every input, losses, grad_losses and every gradient is a carve; the workspace is a carve of exactly
dfe_geom_workspace_floats floats on 16 bytes whose payload holds the NaN sentinel.  After forward and backward every guard is
intact, every input unchanged, losses and gradients written and finite, and losses, mask pack and gradients are bit-equal to the run
of the same inputs through geom_loss_stack / depth_loss_stack / flow_loss_stack on plain tensors -- which
test_hip_loss_stack.py::test_fused_stack_at_the_strip_boundaries pins to the oracle.  Every further check is bit-equality with that
baseline under a change that must not matter: pointers off 16 bytes, other workspace contents, a workspace another case used before,
a second backward, NULL gradient outputs.  No test runs the kernels on a misaligned or short workspace: both are refused."""
import ctypes
import functools

import pytest
import torch

from tests import guarded as G
from tests import loss_stack_cases as LC

pytestmark = pytest.mark.gpu
NLOSS = 10
CASE_IDS = [LC.case_id(c) for c in LC.CASES]
# (X, Y): Y runs in the workspace X ran in before; another shape, mode and depth-term setting
REUSE = [((1, 33, 126, 3, 0, 3), (1, 40, 125, 3, 1, 0)), ((1, 36, 120, 3, 2, 0), (2, 17, 121, 2, 0, 2)), ((1, 40, 125, 3, 1, 0), (1, 25, 122, 3, 0, 1)),
         ((2, 24, 124, 4, 0, 0), (1, 36, 120, 3, 1, 3)), ((1, 33, 126, 3, 0, 3), (1, 36, 120, 3, 2, 0)), ((1, 36, 120, 3, 1, 3), (3, 64, 12, 3, 0, 0)),
         ((1, 40, 125, 3, 1, 0), (1, 33, 126, 3, 0, 3))]


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib(), L.stream_ptr()


def _clean_env(monkeypatch):
    for name in ("DFE_PYRAMIDS_GENERIC", "DFE_ADJ_MODE"):
        monkeypatch.delenv(name, raising=False)


def _ac(case):
    return LC.CASES.index(case) % 2


# --------------------------------------------------------------------------------------------------------- names and groups
def _input_names(case):
    B, H, W, S, mode, dt = case
    names = ["img%d" % f for f in range(3)]
    if mode != 2:
        names += ["disp%d_%d" % (f, s) for f in range(3) for s in range(S)] + ["pose", "K"] + (["K_inv"] if mode == 0 else [])
    if mode != 1:
        names += ["flow%d_%d" % (d, s) for d in range(2) for s in range(S)]
    return names


def _families(case):
    """the gradient outputs of a mode, by family: {family: [(name, shape)]}"""
    B, H, W, S, mode, dt = case
    hw = [(int(H / 2 ** s), int(W / 2 ** s)) for s in range(S)]
    fam = {}
    if mode != 2:
        for f in range(3):
            fam["grad_disp%d" % f] = [("grad_disp%d_%d" % (f, s), (B, 1) + hw[s]) for s in range(S)]
    if mode != 1:
        for d in range(2):
            fam["grad_flow%d" % d] = [("grad_flow%d_%d" % (d, s), (B, 2) + hw[s]) for s in range(S)]
    if mode != 2:
        fam["grad_pose"] = [("grad_pose", (B, 2, 6))]
    return fam


def _group(name):
    if name.startswith("img"):
        return "frames"
    if name in ("pose", "K", "K_inv"):
        return "cam"
    if name.startswith("grad_disp") or name.startswith("grad_flow"):
        return name.rsplit("_", 1)[0]
    if name.startswith("disp") or name.startswith("flow"):
        return name[:4]
    return name                      # losses, grad_losses, grad_pose


def _groups(case):
    return sorted({_group(n) for n in _input_names(case)} | {"losses", "grad_losses"} | set(_families(case)))


def _offsets(names, moved):
    """floats past a 16-byte boundary: the members of the moved group take 1, 2, 3, 1, ... in turn, everything else 0"""
    off, k = {}, 0
    for n in names:
        off[n] = 0
        if moved is not None and _group(n) == moved:
            off[n] = 1 + k % 3
            k += 1
    return off


@functools.lru_cache(maxsize=None)
def _tensors(case):
    """the inputs of a case on the device (read-only), and its grad_losses"""
    inp = LC.inputs(case)
    B, H, W, S, mode, dt = case
    cuda = lambda a: torch.from_numpy(a).float().contiguous().cuda()
    t = {"img%d" % f: cuda(inp.imgs[f]) for f in range(3)}
    t.update({"disp%d_%d" % (f, s): cuda(inp.disps[f][s]) for f in range(3) for s in range(S)})
    t.update({"flow0_%d" % s: cuda(inp.flows_bwd[s]) for s in range(S)})
    t.update({"flow1_%d" % s: cuda(inp.flows_fwd[s]) for s in range(S)})
    t.update(pose=cuda(inp.pose), K=cuda(inp.K), K_inv=cuda(inp.K_inv))
    gen = torch.Generator().manual_seed(sum(case))
    t["grad_losses"] = (0.5 + torch.rand(NLOSS, B, generator=gen)).cuda()
    return t


def _fill_args(case, ac, bufs, ws, ws_floats=None):
    from unsupervised_depth_opticalflow_egomotion_amd.loss_stack import GeomArgs
    B, H, W, S, mode, dt = case
    a = GeomArgs()
    a.B, a.H, a.W, a.num_scales, a.align_corners, a.mode, a.depth_terms = B, H, W, S, ac, mode, dt
    a.alpha, a.beta = (0.01, 0.5) if mode == 0 else (0.0, 0.0)      # as the wrappers pass them
    p = lambda n: bufs[n].ptr if n in bufs else None
    for f in range(3):
        a.img[f] = p("img%d" % f)
        for s in range(S):
            a.disp[f][s] = p("disp%d_%d" % (f, s))
            a.grad_disp[f][s] = p("grad_disp%d_%d" % (f, s))
    for d in range(2):
        for s in range(S):
            a.flow[d][s] = p("flow%d_%d" % (d, s))
            a.grad_flow[d][s] = p("grad_flow%d_%d" % (d, s))
    a.pose, a.K, a.K_inv = p("pose"), p("K"), p("K_inv")
    a.losses, a.grad_losses, a.grad_pose = p("losses"), p("grad_losses"), p("grad_pose")
    a.workspace, a.workspace_floats = ws.ptr, ws.span if ws_floats is None else ws_floats
    return a


def _total(lib, case):
    n = int(lib.dfe_geom_workspace_floats(ctypes.byref(LC.bare_args(case))))
    assert n > 0 and n % 4 == 0, (case, n)
    return n


def _settle(tag, bufs, ws, outs, ins):
    torch.cuda.synchronize()
    assert ws.intact(), (tag, "guard of the workspace overwritten")
    for name, c in bufs.items():
        assert c.intact(), (tag, "guard of %s overwritten" % name)
    for name in outs:
        assert bufs[name].written(), (tag, "%s has unwritten or non-finite elements" % name)
    for name, t in ins.items():
        assert G.bits_equal_dev(bufs[name].view, t), (tag, "input %s changed" % name)


def _forward(lib, st, case, ac, moved=None, ws=None, ws_fill=None):
    """dict(bufs, ws, case, ac): bufs holds the input carves and ``losses``"""
    t = _tensors(case)
    names = _input_names(case)
    off = _offsets(names + ["losses"], moved)
    bufs = {n: G.Carved(t[n].shape, off[n], fill=t[n]) for n in names}
    bufs["losses"] = G.Carved((NLOSS, case[0]), off["losses"])
    if ws is None:
        ws = G.Carved((_total(lib, case),), 0)
    if ws_fill is not None:
        ws.view.fill_(ws_fill)
    args = _fill_args(case, ac, bufs, ws)
    tag = "geom_loss_fwd %s ac %d moved %s fill %s" % (LC.case_id(case), ac, moved, ws_fill)
    rc = lib.dfe_geom_loss_fwd(ctypes.byref(args), st)
    assert rc == 0, (tag, rc)
    _settle(tag, bufs, ws, ("losses",), {n: t[n] for n in names})
    return dict(bufs=bufs, ws=ws, case=case, ac=ac, args=args)


def _backward(lib, st, fw, moved=None, want=None):
    """dict of carves: grad_losses and the gradients of the families in ``want`` (None: all); the others are NULL"""
    case, ac = fw["case"], fw["ac"]
    t = _tensors(case)
    fam = _families(case)
    want = set(fam) if want is None else set(want)
    assert want <= set(fam)
    outs = [(n, shape) for f in sorted(want) for n, shape in fam[f]]
    off = _offsets(["grad_losses"] + [n for n, _ in outs], moved)
    grads = {n: G.Carved(shape, off[n]) for n, shape in outs}
    grads["grad_losses"] = G.Carved((NLOSS, case[0]), off["grad_losses"], fill=t["grad_losses"])
    bufs = dict(fw["bufs"])
    bufs.update(grads)
    args = _fill_args(case, ac, bufs, fw["ws"])
    tag = "geom_loss_bwd %s ac %d moved %s want %s" % (LC.case_id(case), ac, moved, sorted(want))
    rc = lib.dfe_geom_loss_bwd(ctypes.byref(args), st)
    assert rc == 0, (tag, rc)
    ins = {n: t[n] for n in _input_names(case)}
    ins["grad_losses"] = t["grad_losses"]
    _settle(tag, bufs, fw["ws"], [n for n, _ in outs], ins)
    return grads


def _same(tag, a, b, names):
    for n in names:
        assert G.bits_equal_dev(a[n].view, b[n].view), (tag, n, "differs")


def _grad_names(case, want=None):
    fam = _families(case)
    return [n for f in sorted(fam if want is None else want) for n, _ in fam[f]]


def _mask_bytes(lib, fw):
    """the mask pack of a forward's workspace (a copy); mode 2 has soft weights instead and leaves the pack unwritten"""
    B, H, W, S = fw["case"][:4]
    off = int(lib.dfe_geom_maskpack_offset_bytes(ctypes.byref(fw["args"]), 0))
    n = B * sum(int(H / 2 ** s) * int(W / 2 ** s) for s in range(S))
    assert off > 0 and off % 4 == 0 and off + n <= 4 * fw["ws"].span
    return fw["ws"].view.view(torch.uint8)[off:off + (n if fw["case"][4] != 2 else 0)].clone()


def _run(lib, st, case, ac, **kw):
    fw = _forward(lib, st, case, ac, **kw)
    mask = _mask_bytes(lib, fw)
    gr = _backward(lib, st, fw, moved=kw.get("moved"))
    out = dict(gr)
    out["losses"] = fw["bufs"]["losses"]
    return fw, out, mask


def _plain(case, ac):
    """the same inputs through the product's wrappers on plain tensors: (losses [10, B], {gradient name: tensor}, mask info)"""
    from unsupervised_depth_opticalflow_egomotion_amd import loss_stack as LS
    B, H, W, S, mode, dt = case
    t = _tensors(case)
    leaf = lambda n: t[n].clone().requires_grad_(True)
    imgs = [t["img%d" % f].clone() for f in range(3)]
    disps = [[leaf("disp%d_%d" % (f, s)) for s in range(S)] for f in range(3)] if mode != 2 else None
    flows = [[leaf("flow%d_%d" % (d, s)) for s in range(S)] for d in range(2)] if mode != 1 else None
    pose = leaf("pose") if mode != 2 else None
    terms = dict(enable_depth_ssim=bool(dt & 1), enable_depth_consis=bool(dt & 2))
    mask = None
    if mode == 0:
        lp, handle = LS.geom_loss_stack(*imgs, disps[0], disps[1], disps[2], pose, flows[0], flows[1], t["K"].clone(), t["K_inv"].clone(), num_scales=S,
                                        align_corners=bool(ac), return_masks="lazy", **terms)
        mask = handle[0]
    elif mode == 1:
        lp, mask = LS.depth_loss_stack(*imgs, disps[0], disps[1], disps[2], pose, t["K"].clone(), num_scales=S, align_corners=bool(ac), return_masks=True, **terms)
    else:
        lp = LS.flow_loss_stack(*imgs, flows[0], flows[1], num_scales=S, align_corners=bool(ac))
    losses = lp.rows[0]
    assert tuple(losses.shape) == (NLOSS, B)
    (losses * t["grad_losses"]).sum().backward()           # d total / d losses is grad_losses, bit for bit
    torch.cuda.synchronize()
    grads = {}
    if mode != 2:
        grads.update({"grad_disp%d_%d" % (f, s): disps[f][s].grad for f in range(3) for s in range(S)})
        grads["grad_pose"] = pose.grad
    if mode != 1:
        grads.update({"grad_flow%d_%d" % (d, s): flows[d][s].grad for d in range(2) for s in range(S)})
    return losses.detach(), grads, mask


@functools.lru_cache(maxsize=None)
def _baseline(case):
    """(forward state, outputs, mask-pack bytes) of the guarded run whose workspace holds the NaN sentinel, already compared
    with the plain run"""
    lib, st = _lib()
    ac = _ac(case)
    B, H, W, S, mode, dt = case
    assert _total(lib, case) == LC.plan(lib, LC.bare_args(case))["total"]
    fw, out, mask = _run(lib, st, case, ac)
    assert fw["ws"].span == _total(lib, case) and fw["ws"].ptr % 16 == 0
    tag = "baseline %s ac %d against the plain run" % (LC.case_id(case), ac)
    losses, grads, pmask = _plain(case, ac)
    assert G.bits_equal_dev(out["losses"].view, losses), (tag, "losses", out["losses"].cpu(), losses)
    assert set(grads) == set(_grad_names(case))
    for n, g in grads.items():
        assert g is not None and G.bits_equal_dev(out[n].view, g), (tag, n)
    if mode == 0:          # the whole mask pack, byte for byte
        off = int(lib.dfe_geom_maskpack_offset_bytes(ctypes.byref(fw["args"]), 0))
        assert torch.equal(mask, pmask.view(torch.uint8)[off:off + mask.numel()]), (tag, "mask pack")
    elif mode == 1:        # the four masks Model_depth decodes
        from unsupervised_depth_opticalflow_egomotion_amd.loss_stack import decode_masks
        mine = decode_masks(fw["ws"].view, B, H, W, S)
        for theirs, name in (("valid_to_l", "valid_bwd"), ("valid_to_r", "valid_fwd"), ("texture_bwd", "texture_bwd"), ("texture_fwd", "texture_fwd")):
            for s in range(S):
                assert torch.equal(mine[name][s], pmask[theirs][s]), (tag, theirs, s)
    return fw, out, mask


def _outputs(case):
    return ["losses"] + _grad_names(case)


# --------------------------------------------------------------------------------------------------------- the tests
@pytest.mark.parametrize("case", LC.CASES, ids=CASE_IDS)
def test_baseline_in_guarded_buffers_is_the_plain_run(case, monkeypatch):
    _clean_env(monkeypatch)
    lib, st = _lib()
    fw, out, mask = _baseline(case)
    p = LC.plan(lib, fw["args"])
    B, H, W, S, mode, dt = case
    assert p["two_level"] == int(S >= 3 and mode != 2 and H % 4 == 0 and W % 4 == 0) and p["dt"] == (dt if mode != 2 else 0), p
    assert torch.equal(_mask_bytes(lib, fw), mask), "the backward changed the mask pack"


@pytest.mark.parametrize("case", LC.CASES, ids=CASE_IDS)
def test_every_pointer_group_off_16_bytes_in_turn(case, monkeypatch):
    """frames, disparities, flows, pose / K / K_inv, losses, grad_losses and each gradient family 1, 2 and 3 floats past a
    16-byte boundary: the bits of the aligned run.  Moving the frames takes the per-level pyramid kernel (the plan says so)."""
    _clean_env(monkeypatch)
    lib, st = _lib()
    ac = _ac(case)
    base_fw, base, base_mask = _baseline(case)
    two = LC.plan(lib, base_fw["args"])["two_level"]
    forward_groups = {_group(n) for n in _input_names(case)} | {"losses"}
    for moved in _groups(case):
        tag = "%s moved %s" % (LC.case_id(case), moved)
        if moved in forward_groups:
            fw, out, mask = _run(lib, st, case, ac, moved=moved)
            assert any(c.ptr % 16 for c in fw["bufs"].values()), tag
            p = LC.plan(lib, fw["args"])
            assert p["two_level"] == (0 if moved == "frames" else two) and p["total"] == base_fw["ws"].span, (tag, p)
            assert torch.equal(mask, base_mask), (tag, "mask pack")
        else:
            out = _backward(lib, st, base_fw, moved=moved)
            assert any(c.ptr % 16 for c in out.values()), tag
            out["losses"] = base["losses"]
        _same(tag, out, base, _outputs(case))


@pytest.mark.parametrize("case", LC.CASES, ids=CASE_IDS)
def test_workspace_contents_on_entry_do_not_matter(case, monkeypatch):
    """the baseline's workspace held the NaN sentinel; zeros and a large finite value give the same bits (a region read before it
    is written shows up as a NaN or as a difference)"""
    _clean_env(monkeypatch)
    lib, st = _lib()
    base_fw, base, base_mask = _baseline(case)
    assert base_fw["ws"].span > 0
    for fill in (0.0, 1.0e30):
        fw, out, mask = _run(lib, st, case, _ac(case), ws_fill=fill)
        tag = "%s workspace prefilled with %r" % (LC.case_id(case), fill)
        _same(tag, out, base, _outputs(case))
        assert torch.equal(mask, base_mask), (tag, "mask pack")


@pytest.mark.parametrize("pair", REUSE, ids=lambda p: LC.case_id(p[0]) + "-then-" + LC.case_id(p[1]))
def test_workspace_reused_by_a_case_of_another_shape_and_mode(pair, monkeypatch):
    _clean_env(monkeypatch)
    lib, st = _lib()
    X, Y = pair
    assert X in LC.CASES and Y in LC.CASES and X[1:3] != Y[1:3] and X[4] != Y[4] and X[5] != Y[5]
    ws = G.Carved((max(_total(lib, X), _total(lib, Y)),), 0)
    _run(lib, st, X, _ac(X), ws=ws)
    fw, out, mask = _run(lib, st, Y, _ac(Y), ws=ws)
    base_fw, base, base_mask = _baseline(Y)
    tag = "%s after %s in one workspace" % (LC.case_id(Y), LC.case_id(X))
    _same(tag, out, base, _outputs(Y))
    assert torch.equal(mask, base_mask), (tag, "mask pack")


@pytest.mark.parametrize("case", LC.CASES, ids=CASE_IDS)
def test_backward_twice_on_one_forward_and_the_mask_pack_survives(case, monkeypatch):
    _clean_env(monkeypatch)
    lib, st = _lib()
    fw = _forward(lib, st, case, _ac(case))
    before = _mask_bytes(lib, fw)
    first = _backward(lib, st, fw)
    assert torch.equal(_mask_bytes(lib, fw), before), "the backward changed the mask pack"
    second = _backward(lib, st, fw)
    assert torch.equal(_mask_bytes(lib, fw), before), "the second backward changed the mask pack"
    _same("%s second backward" % LC.case_id(case), second, first, _grad_names(case))
    _same("%s against the baseline" % LC.case_id(case), first, _baseline(case)[1], _grad_names(case))


@pytest.mark.parametrize("case", LC.CASES, ids=CASE_IDS)
def test_null_gradient_outputs_are_skipped(case, monkeypatch):
    """every family alone (grad_disp of one frame, grad_flow of one direction, grad_pose), grad_pose NULL alone, and with the
    consistency term the source frames' disparity gradients without the target's and the reverse: what is requested has the bits
    of the full run.  (Every store through G.gdisp, G.gflow and gpose of loss_stack_bwd.hip is behind a NULL test: read before
    this test first ran.)"""
    _clean_env(monkeypatch)
    lib, st = _lib()
    B, H, W, S, mode, dt = case
    base_fw, base, _ = _baseline(case)
    fam = sorted(_families(case))
    wants = [{f} for f in fam]
    if "grad_pose" in fam:
        wants.append(set(fam) - {"grad_pose"})
    if mode != 2 and dt & 2:
        wants += [{"grad_disp1"}, {"grad_disp0", "grad_disp2"}, {"grad_disp1", "grad_pose"}, {"grad_disp0", "grad_disp2", "grad_pose"}]
    for want in wants:
        out = _backward(lib, st, base_fw, want=want)
        assert set(out) == set(_grad_names(case, want)) | {"grad_losses"}
        _same("%s gradients %s alone" % (LC.case_id(case), sorted(want)), out, base, _grad_names(case, want))


def test_short_or_misaligned_workspace_is_refused_before_any_launch(monkeypatch):
    """workspace_floats one below the total: DFE_ERR_WORKSPACE; a workspace 1, 2 or 3 floats off 16 bytes: DFE_ERR_DIMS; from both
    entry points, with the workspace and every output untouched"""
    _clean_env(monkeypatch)
    lib, st = _lib()
    for case in (LC.CASES[0], LC.CASES[5], LC.CASES[6]):
        t = _tensors(case)
        total = _total(lib, case)
        bufs = {n: G.Carved(t[n].shape, 0, fill=t[n]) for n in _input_names(case) + ["grad_losses"]}
        outs = {n: G.Carved(shape, 0) for f in _families(case).values() for n, shape in f}
        outs["losses"] = G.Carved((NLOSS, case[0]), 0)
        bufs.update(outs)
        spaces = [(G.Carved((total,), 0), total - 1, -5)] + [(G.Carved((total,), k), total, -2) for k in (1, 2, 3)]
        for ws, floats, code in spaces:
            args = _fill_args(case, 0, bufs, ws, floats)
            assert lib.dfe_geom_loss_fwd(ctypes.byref(args), st) == code, (case, floats, ws.ptr % 16)
            assert lib.dfe_geom_loss_bwd(ctypes.byref(args), st) == code, (case, floats, ws.ptr % 16)
        torch.cuda.synchronize()
        for ws, _, _ in spaces:
            assert ws.untouched() and ws.intact()
        for n, c in outs.items():
            assert c.untouched() and c.intact(), n
        for n in _input_names(case) + ["grad_losses"]:
            assert bufs[n].intact() and G.bits_equal_dev(bufs[n].view, t[n]), n
