"""nearest x2 upsample + 3x3 convolution (pad 1) as four 2x2 phase convolutions of the low-resolution map — the identity the
phase kernels (csrc/lean.h / wide.h PHASE) rest on, and the weight layout they read (packing.pack_conv_up4), on the CPU.

Output pixel (2i + a, 2j + b) reads low-resolution rows {i - 1 + a, i + a} and columns {j - 1 + b, j + b} (zero outside the
map) with the 3x3 taps summed over the duplicates the upsample makes: V[a][b][r][s] = sum_{dy in S_a(r)} sum_{dx in S_b(s)} W[dy][dx],
S_0 = ({0}, {1, 2}), S_1 = ({0, 1}, {2}).  Reference: Upsample.forward of openaimodel.py:99-101 / model.py:64-68."""
import torch
import torch.nn.functional as F

import udifftext_amd  # noqa: F401
from sgm.modules import hipnn as H
from udifftext_amd import packing

F64 = torch.float64


def _reference(x, w):
    """x [B, H, W, C], w [N, C, 3, 3] -> [B, 2H, 2W, N]: interpolate(nearest, x2) + conv2d(pad 1)"""
    up = F.interpolate(x.permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    return F.conv2d(up, w, padding=1).permute(0, 2, 3, 1)


def _phase_reconstruction(x, v):
    """x [B, H, W, C], v [4, N, 2, 2, C] (phase 2a + b, taps r, s) -> [B, 2H, 2W, N] by the identity, zero outside the map"""
    B, Hh, Ww, C = x.shape
    N = v.shape[1]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))                         # low-resolution rows / columns -1 and H / W are zero
    out = torch.zeros((B, 2 * Hh, 2 * Ww, N), dtype=x.dtype)
    for a in range(2):
        for b in range(2):
            acc = torch.zeros((B, Hh, Ww, N), dtype=x.dtype)
            for r in range(2):
                for s in range(2):
                    # low-resolution pixel (i - 1 + a + r, j - 1 + b + s) = padded index (i + a + r, j + b + s)
                    acc += xp[:, a + r:a + r + Hh, b + s:b + s + Ww, :] @ v[2 * a + b, :, r, s, :].t()
            out[:, a::2, b::2, :] = acc
    return out


def _unrounded_sums(w):
    N, C = w.shape[:2]
    v = torch.zeros((4, N, 2, 2, C), dtype=w.dtype)
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for s in range(2):
                    v[2 * a + b, :, r, s, :] = sum(w[:, :, dy, dx] for dy in packing.UP4_TAPS[a][r] for dx in packing.UP4_TAPS[b][s])
    return v


def _case():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 5, 6, 4), generator=g, dtype=F64)
    w = torch.randn((7, 4, 3, 3), generator=g, dtype=F64)
    return x, w


def test_phase_reconstruction_equals_interpolate_conv_in_fp64():
    x, w = _case()
    got, ref = _phase_reconstruction(x, _unrounded_sums(w)), _reference(x, w)
    assert got.shape == ref.shape == (2, 10, 12, 7)
    assert (got - ref).abs().max().item() <= 1e-12


def test_border_only_input_gives_the_same_result():
    x, w = _case()
    edge = torch.zeros_like(x)
    edge[:, 0], edge[:, -1], edge[:, :, 0], edge[:, :, -1] = x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1]
    assert edge[:, 1:-1, 1:-1].abs().max().item() == 0 and edge.abs().max().item() > 0
    got, ref = _phase_reconstruction(edge, _unrounded_sums(w)), _reference(edge, w)
    assert (got - ref).abs().max().item() <= 1e-12


def test_pack_conv_up4_column_order_padding_and_rounding():
    g = torch.Generator().manual_seed(6)
    N, C = 7, 4
    w = torch.randn((N, C, 3, 3), generator=g)
    p = packing.pack_conv_up4(w, n_pad_to=4)
    Np, Cp = 8, 64
    assert p.dtype == torch.bfloat16 and p.shape == (4, Np, 4 * Cp) and p.is_contiguous()
    v = p.reshape(4, Np, 2, 2, Cp)
    assert v[:, N:].abs().max().item() == 0 and v[..., C:].abs().max().item() == 0        # padded rows / channels are zero
    # k = (2r + s) * Cpad + c, phase 2a + b; fp32 sums of the bf16-ROUNDED taps, rounded once
    want = _unrounded_sums(w.bfloat16().float()).bfloat16()
    assert torch.equal(v[:, :N, :, :, :C], want)
    for ph, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        for k4, (r, s) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            col = p[ph, 2, k4 * Cp + 3]
            taps = [w.bfloat16().float()[2, 3, dy, dx] for dy in packing.UP4_TAPS[a][r] for dx in packing.UP4_TAPS[b][s]]
            assert col == sum(taps).bfloat16()
    # a single tap survives untouched: phase (0, 0) tap (0, 0) is W[0][0], phase (1, 1) tap (1, 1) is W[2][2]
    assert torch.equal(v[0, :N, 0, 0, :C], w[:, :, 0, 0].bfloat16()) and torch.equal(v[3, :N, 1, 1, :C], w[:, :, 2, 2].bfloat16())
    # the rounded layout reproduces the convolution with the bf16 3x3 weights to the one extra rounding (2^-9 per summed weight)
    x = torch.randn((1, 4, 4, C), generator=g, dtype=F64)
    got = _phase_reconstruction(x, v[:, :N, :, :, :C].to(F64))
    ref = _reference(x, w.bfloat16().to(F64))
    assert ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item() < 2 ** -8
    # output-channel padding follows n_pad_to (64 when the consumer is a GEMM)
    assert packing.pack_conv_up4(w, n_pad_to=64).shape == (4, 64, 4 * Cp)


def test_up4_layout_is_cached_and_rebuilt_when_the_weight_version_changes():
    conv = H.Conv2d(4, 7, 3, padding=1)
    first = conv.packed_up4()
    assert conv.packed_up4() is first and H.has_layout(conv, "up4")
    plain = conv.packed()
    with torch.no_grad():
        conv.weight.mul_(2.0)                                  # a training step: _version + 1
    second = conv.packed_up4()
    assert second is not first
    assert torch.equal(second, packing.pack_conv_up4(conv.weight, conv.n_pad))
    assert not torch.equal(second, first)
    assert conv.packed() is not plain                          # the 3x3 pack follows the same key
    assert conv.packed_up4() is second
