"""GPU: the weight-gradient kernels (csrc/ops_wino_wgrad.hip, ops_sconv.hip, ops_wgrad.hip) through the C ABI in guarded,
poisoned buffers (tests/guarded.py): x and gy as dword-aligned, batch-strided views at every float offset, gweight and the
split-partial workspace (exactly the size the library reports under the tune setting in force) poisoned with NaN, results
bit-equal across offsets and strides, and the per-element bound e = |out - ref64| / (2^-24 A) against a plain fp32
implementation of the same algorithm on zero-mean, activation-like and sparse inputs."""
import ctypes

import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu

# (x offset, gy offset, x batch stride - dense, gy batch stride - dense)
BASE = (0, 0, 0, 0)
VARIANTS = [(1, 0, 0, 0), (0, 1, 0, 0), (2, 3, 1, 2), (3, 2, 2, 3), (1, 1, 3, 1), (0, 0, 2, 2), (3, 3, 0, 0), (2, 2, 1, 1)]


def _lib():
    from unsupervised_depth_opticalflow_egomotion_amd import _lib as L
    return L.get_lib(), L.stream_ptr()


def _p(c):
    return ctypes.c_void_p(c.ptr)


def _l(v):
    return ctypes.c_long(int(v))


def _run(call, nws, x_cpu, gy_cpu, gw_shape, variant, tag):
    """x, gy, gweight and ws carved per ``variant``; call(x, xbs, gy, gbs, gw, ws) -> rc; returns gweight on the CPU"""
    xo, go, xbe, gbe = variant
    assert nws > 0, tag
    x = G.Carved(tuple(x_cpu.shape), xo, x_cpu[0].numel() + xbe, fill=x_cpu)
    gy = G.Carved(tuple(gy_cpu.shape), go, gy_cpu[0].numel() + gbe, fill=gy_cpu)
    gw = G.Carved(gw_shape, go)
    ws = G.Carved((nws,), xo)
    rc = call(x, gy, gw, ws)
    assert rc == 0, (tag, variant, rc)
    torch.cuda.synchronize()
    for name, c in (("x", x), ("gy", gy), ("gweight", gw), ("ws", ws)):
        assert c.intact(), (tag, variant, "guard or gap of %s overwritten" % name)
    assert gw.written(), (tag, variant, "gweight elements unwritten or not finite")
    assert torch.equal(x.cpu(), x_cpu) and torch.equal(gy.cpu(), gy_cpu), (tag, variant, "an input changed")
    return gw.cpu()


# ---------------------------------------------------------------------------------------------------- dfe_wino_wgrad3x3
# (B, Ci, Co, H, W, P)
WINO_SHAPES = [(1, 1, 1, 3, 3, 0),            # one tile; gy is a single float
               (2, 5, 3, 3, 3, 1),
               (1, 33, 17, 5, 27, 1),         # 14 tile columns: the second chunk partial
               (2, 40, 70, 4, 50, 0),         # 24 tile columns
               (1, 130, 64, 6, 10, 1)]        # the 64 x 32 block by shape
TUNES = ((0, 12), (11, 12), (11, 8), (21, 12), (21, 8), (12, 8))


@pytest.mark.parametrize("shape", WINO_SHAPES)
def test_wino_wgrad_guarded(shape):
    B, Ci, Co, H, W, P = shape
    lib, st = _lib()
    Ho, Wo = H + 2 * P - 2, W + 2 * P - 2
    cases = []
    for family in G.FAMILIES:
        gen = torch.Generator().manual_seed(sum(shape) + G.FAMILIES.index(family))
        x, gy = G.make_input((B, Ci, H, W), family, gen), G.make_input((B, Co, Ho, Wo), family, gen)
        cases.append((family, x, gy, G.conv_wgrad_ref(gy, x, 3, 1, P, 1, torch.float64), G.wino_wgrad(x, gy, P, torch.float32),
                      G.wino_wgrad(x, gy, P, torch.float64, absolute=True)))

    def call(x, gy, gw, ws):
        return lib.dfe_wino_wgrad3x3(_p(x), _l(x.batch_stride), _p(gy), _l(gy.batch_stride), _p(gw), _p(ws), B, Ci, Co, H, W, P, st)

    try:
        for tile, chunk in TUNES:
            assert lib.dfe_wino_wgrad_tune(tile, 0, 0, chunk) == 0
            nws = int(lib.dfe_wino_wgrad_floats(B, Ci, Co, H, W, P))          # the size follows the setting
            for family, x, gy, ref, yard, Sw in cases:
                tag = "wino_wgrad %s %s tile %d chunk %d" % (family, shape, tile, chunk)
                base = _run(call, nws, x, gy, (Co, Ci, 3, 3), BASE, tag)
                G.check_bound(tag, base, yard, ref, Sw)
                if family == "act":
                    for v in VARIANTS:
                        assert torch.equal(_run(call, nws, x, gy, (Co, Ci, 3, 3), v, tag), base), (tag, v, "gweight depends on the alignment")
    finally:
        lib.dfe_wino_wgrad_tune(0, 0, 0, 12)


# ---------------------------------------------------------------------------------------------------- dfe_sconv_wgrad
# (B, Ci, Co, H, W, K, stride, P)
SCONV_SHAPES = [(1, 3, 5, 6, 6, 3, 2, 1), (2, 9, 10, 17, 23, 7, 2, 3), (1, 16, 32, 21, 27, 5, 2, 2), (1, 4, 4, 1, 1, 3, 2, 1), (2, 33, 17, 7, 9, 3, 2, 1),
                (1, 17, 20, 5, 130, 3, 2, 1)]
SCONV_TUNES = ((0, 0), (96, 0), (2048, 1))


@pytest.mark.parametrize("shape", SCONV_SHAPES)
def test_sconv_wgrad_guarded(shape):
    B, Ci, Co, H, W, K, S, P = shape
    lib, st = _lib()
    Ho, Wo = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
    cases = []
    for family in G.FAMILIES:
        gen = torch.Generator().manual_seed(sum(shape) + G.FAMILIES.index(family))
        x, gy = G.make_input((B, Ci, H, W), family, gen), G.make_input((B, Co, Ho, Wo), family, gen)
        cases.append((family, x, gy, G.conv_wgrad_ref(gy, x, K, S, P, 1, torch.float64), G.conv_wgrad_ref(gy, x, K, S, P, 1, torch.float32),
                      G.conv_wgrad_ref(gy.abs(), x.abs(), K, S, P, 1, torch.float64)))

    def call(x, gy, gw, ws):
        return lib.dfe_sconv_wgrad(_p(x), _l(x.batch_stride), _p(gy), _l(gy.batch_stride), _p(gw), _p(ws), B, Ci, Co, H, W, K, S, P, st)

    try:
        for blocks, rows in SCONV_TUNES:
            assert lib.dfe_sconv_tune(blocks, rows) == 0
            nws = int(lib.dfe_sconv_wgrad_floats(B, Ci, Co, H, W, K, S, P))
            for family, x, gy, ref, yard, A in cases:
                tag = "sconv_wgrad %s %s blocks %d rows %d" % (family, shape, blocks, rows)
                base = _run(call, nws, x, gy, (Co, Ci, K, K), BASE, tag)
                G.check_bound(tag, base, yard, ref, A)
                if family == "act":
                    for v in VARIANTS:
                        assert torch.equal(_run(call, nws, x, gy, (Co, Ci, K, K), v, tag), base), (tag, v, "gweight depends on the alignment")
    finally:
        lib.dfe_sconv_tune(0, 0)


def test_tiny_views_are_refused_or_safe():
    """The staging loads fetch 16 bytes from a safe address when their slot lies outside the image.  dfe_sconv_wgrad takes a
    sample's base for it and therefore refuses samples of fewer than 4 floats (0 workspace floats, DFE_ERR_UNSUPPORTED, nothing
    written); dfe_wino_wgrad3x3 takes its own workspace (at least 9 floats) and accepts any view (test_wino_wgrad_guarded runs
    a one-float gy)."""
    lib, st = _lib()
    for (B, Ci, Co, H, W, K, S, P) in [(2, 3, 4, 1, 1, 3, 2, 1), (1, 4, 3, 1, 1, 3, 2, 1), (3, 1, 8, 3, 1, 3, 2, 1)]:
        assert lib.dfe_sconv_wgrad_floats(B, Ci, Co, H, W, K, S, P) == 0
        Ho, Wo = (H + 2 * P - K) // S + 1, (W + 2 * P - K) // S + 1
        x, gy = G.Carved((B, Ci, H, W), 0, fill=torch.ones(B, Ci, H, W)), G.Carved((B, Co, Ho, Wo), 0, fill=torch.ones(B, Co, Ho, Wo))
        gw, ws = G.Carved((Co, Ci, K, K), 0), G.Carved((64,), 0)
        assert lib.dfe_sconv_wgrad(_p(x), _l(Ci * H * W), _p(gy), _l(Co * Ho * Wo), _p(gw), _p(ws), B, Ci, Co, H, W, K, S, P, st) == -4
        torch.cuda.synchronize()
        assert gw.untouched() and ws.untouched() and gw.intact() and ws.intact()
    assert lib.dfe_wino_wgrad_floats(1, 1, 1, 1, 1, 1) >= 9 and lib.dfe_wino_wgrad_floats(1, 1, 1, 3, 3, 0) >= 9


# ---------------------------------------------------------------------------------------------------- dfe_wgrad3x3_fwd
# (B, Ci, Co, H, W): pre-padded input p [B,Ci,H+2,W+2]
THIN_SHAPES = [(2, 16, 16, 8, 32), (1, 32, 16, 5, 16), (2, 48, 32, 7, 48)]


@pytest.mark.parametrize("shape", THIN_SHAPES)
def test_wgrad3x3_thin_guarded(shape):
    B, Ci, Co, H, W = shape
    lib, st = _lib()
    nws = int(lib.dfe_wgrad3x3_partials_floats(B, Ci, Co, H, W))
    assert nws > 0
    for family in G.FAMILIES:
        gen = torch.Generator().manual_seed(sum(shape) + G.FAMILIES.index(family))
        p_cpu, gy_cpu = G.make_input((B, Ci, H + 2, W + 2), family, gen), G.make_input((B, Co, H, W), family, gen)
        tag = "wgrad3x3_thin %s %s" % (family, shape)
        p, gy = G.Carved(p_cpu.shape, 0, fill=p_cpu), G.Carved(gy_cpu.shape, 0, fill=gy_cpu)
        gw, ws = G.Carved((Co, Ci, 3, 3), 1), G.Carved((nws,), 1)
        assert lib.dfe_wgrad3x3_fwd(_p(p), _p(gy), _p(gw), _p(ws), B, Ci, Co, H, W, st) == 0
        torch.cuda.synchronize()
        assert p.intact() and gy.intact() and gw.intact() and ws.intact() and gw.written(), tag
        G.check_bound(tag, gw.cpu(), G.conv_wgrad_ref(gy_cpu, p_cpu, 3, 1, 0, 1, torch.float32), G.conv_wgrad_ref(gy_cpu, p_cpu, 3, 1, 0, 1, torch.float64),
                      G.conv_wgrad_ref(gy_cpu.abs(), p_cpu.abs(), 3, 1, 0, 1, torch.float64))
        p2 = G.Carved(p_cpu.shape, 2, fill=p_cpu)                  # 8-byte aligned p is within the contract
        gw2, ws2 = G.Carved((Co, Ci, 3, 3), 0), G.Carved((nws,), 0)
        assert lib.dfe_wgrad3x3_fwd(_p(p2), _p(gy), _p(gw2), _p(ws2), B, Ci, Co, H, W, st) == 0
        torch.cuda.synchronize()
        assert p2.intact() and gw2.intact() and ws2.intact() and torch.equal(gw2.cpu(), gw.cpu()), tag
    # outside the contract: p 4 bytes off 8, gy 4 / 8 / 12 bytes off 16 -> DFE_ERR_UNSUPPORTED, nothing written
    for po, go in ((1, 0), (3, 0), (0, 1), (0, 2), (0, 3)):
        p, gy = G.Carved(p_cpu.shape, po, fill=p_cpu), G.Carved(gy_cpu.shape, go, fill=gy_cpu)
        gw, ws = G.Carved((Co, Ci, 3, 3), 0), G.Carved((nws,), 0)
        assert lib.dfe_wgrad3x3_fwd(_p(p), _p(gy), _p(gw), _p(ws), B, Ci, Co, H, W, st) == -4, (po, go)
        torch.cuda.synchronize()
        assert gw.untouched() and ws.untouched() and gw.intact() and ws.intact(), (po, go)
