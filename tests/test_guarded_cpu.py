"""CPU: self-tests of tests/guarded.py -- the guard bands notice a write one float before a view, one float after it and into a
batch gap (and nothing else), and the plain-torch Winograd emulations that serve as the fp32 yardstick compute, in float64, what
aten's float64 convolution / weight gradient computes."""
import pytest
import torch

from tests import guarded as G

CPU = torch.device("cpu")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("gap", [0, 1, 5])
def test_carved_guards_notice_stray_writes(off, gap):
    shape, dense = (3, 2, 3, 5), 30
    vals = torch.arange(90, dtype=torch.float32).reshape(shape)
    c = G.Carved(shape, off, dense + gap, fill=vals, device=CPU)
    flat = c.bits.view(torch.float32)
    assert c.view.data_ptr() % 16 == 4 * off and c.view.stride() == (dense + gap, 15, 5, 1)
    assert c.lo >= 64 and c.bits.numel() - (c.lo + c.span) >= 64
    assert c.intact() and c.written() and torch.equal(c.cpu(), vals)
    c.view[1, 1, 2, 4] = -1.0                  # inside the view: allowed
    c.view[2, 1, 2, 4] = -2.0                  # the view's last element
    c.view[0, 0, 0, 0] = -3.0                  # ... and its first
    assert c.intact()
    for pos in [c.lo - 1, c.lo + c.span] + ([c.lo + dense, c.lo + 2 * (dense + gap) - 1] if gap else []):
        old = c.bits[pos].clone()
        flat[pos] = 0.0
        assert not c.intact(), pos
        c.bits[pos] = old
        assert c.intact()
    flat[0] = 1.0                              # the far end of the guard band
    assert not c.intact()


def test_carved_poisoned_payload_and_one_dimensional_views():
    c = G.Carved((7,), 3, device=CPU)
    assert c.intact() and c.untouched() and not c.written() and bool(torch.isnan(c.view).all())
    c.view[:6] = 1.0
    assert not c.written() and not c.untouched()                 # one element nobody wrote
    c.view[6] = float("inf")
    assert not c.written()
    c.view[6] = 0.0
    assert c.written() and c.intact()
    g = G.Carved((2, 4), 0, 6, device=CPU)                       # the gap stays NaN when the payload is filled
    g.view.fill_(2.0)
    assert g.intact() and int(torch.isnan(g.bits.view(torch.float32)[g.lo:g.lo + g.span]).sum()) == 2


def test_sparse_family_has_zero_blocks_and_a_zero_channel():
    gen = torch.Generator().manual_seed(1)
    x = G.make_input((2, 6, 9, 10), "sparse", gen)
    assert float(x[0, :, 0:4, 0:4].abs().max()) == 0.0 and float(x[1, :, 8:, 8:].abs().max()) == 0.0 and float(x[:, 3].abs().max()) == 0.0
    assert float(x.min()) == 0.0 and float(x.max()) > 0.0
    assert float(G.make_input((1, 2, 4, 4), "act", gen).min()) >= 1.0


# (B, Ci, Co, H, W, P, dilation)
EMU_SHAPES = [(1, 512, 4, 6, 6, 1, 1), (2, 5, 3, 3, 3, 0, 1), (2, 6, 17, 3, 4, 0, 1), (1, 4, 33, 1, 2, 1, 1), (2, 12, 20, 7, 9, 1, 1), (2, 8, 8, 6, 8, 2, 1),
              (1, 7, 40, 5, 5, 2, 1), (2, 9, 20, 6, 12, 1, 3), (1, 8, 8, 4, 4, 1, 2)]


@pytest.mark.parametrize("shape", EMU_SHAPES)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_winograd_emulation_in_float64_is_atens_convolution(shape, family):
    """|emulation64 - aten64| <= (Ci + 32) 2^-53 S_w per element (float64 roundings of Ci products and the transforms, each
    bounded by the Winograd-domain absolute sum), forward and data-gradient form."""
    B, Ci, Co, H, W, P, d = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = G.make_input((B, Ci, H, W), family, gen)
    for transposed in (False, True):
        w = G.make_weight(Ci, Co, 3, gen) if transposed else G.make_weight(Co, Ci, 3, gen)
        ref = G.wino_conv_ref64(x, w, P, d, transposed)
        emu = G.wino_conv(x, w, P, d, transposed, torch.float64)
        Sw = G.wino_conv(x, w, P, d, transposed, torch.float64, absolute=True)
        assert emu.shape == ref.shape == Sw.shape
        assert bool(((emu - ref).abs() <= (Ci + 32) * 2.0 ** -53 * Sw).all()), float((emu - ref).abs().max())
        assert float((G.wino_conv(x, w, P, d, transposed, torch.float32).double() - ref).abs().max()) <= 1e-4 * max(1.0, float(ref.abs().max()))


WG_EMU_SHAPES = [(1, 1, 1, 3, 3, 0), (2, 5, 3, 3, 3, 1), (1, 33, 17, 5, 27, 1), (2, 40, 70, 4, 50, 0), (1, 130, 64, 6, 10, 1)]


@pytest.mark.parametrize("shape", WG_EMU_SHAPES)
@pytest.mark.parametrize("family", G.FAMILIES)
def test_winograd_wgrad_emulation_in_float64_is_atens_weight_gradient(shape, family):
    B, Ci, Co, H, W, P = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x = G.make_input((B, Ci, H, W), family, gen)
    gy = G.make_input((B, Co, H + 2 * P - 2, W + 2 * P - 2), family, gen)
    ref = G.conv_wgrad_ref(gy, x, 3, 1, P, 1, torch.float64)
    emu = G.wino_wgrad(x, gy, P, torch.float64)
    Sw = G.wino_wgrad(x, gy, P, torch.float64, absolute=True)
    ntiles = B * ((H + 2 * P - 1) // 2) * ((W + 2 * P - 1) // 2)
    assert emu.shape == ref.shape == Sw.shape == (Co, Ci, 3, 3)
    assert bool(((emu - ref).abs() <= (ntiles + 32) * 2.0 ** -53 * Sw).all()), float((emu - ref).abs().max())
