"""Memory footprint of the LPIPS kernels (csrc/lpips.hip) as cases of tests/test_footprint_gpu.py's table: udt_conv2d_f32,
udt_maxpool3s2_f32, udt_lpips_input_f32, udt_lpips_layer_f32 with its size query.

The cases are appended to that module's ``CASES`` when this module is imported, as tests/test_char_maps_footprint_gpu.py does it, and
run here through the table's own ``_run_case``: every operand a strided channels-last view (pixel stride ld > C) inside a NaN-poisoned
arena, every output guarded and pre-filled with the sentinel, the layer's scratch of EXACTLY the stated size between two guards, against
compact buffers, bit-equal.  A tap of the convolution that read a pixel's ld gap, a neighbouring image or a packed-weight row beyond
Cout would bring a NaN into an output, which is asserted absent on top of the bitwise comparison.
"""
import pytest
import torch

import test_footprint_gpu as table
from test_footprint_gpu import F32, U8, _mods, _rand, env  # noqa: F401  (env: the table's fixture)

pytestmark = pytest.mark.gpu

CONV, POOL, INPUT, LAYER, LAYER_Q = ("udt_conv2d_f32", "udt_maxpool3s2_f32", "udt_lpips_input_f32", "udt_lpips_layer_f32",
                                     "udt_lpips_layer_scratch_bytes")
OWN = []


def case(name, covers):
    def deco(fn):
        if name not in [c[0] for c in table.CASES]:           # (a re-import must not register twice)
            table.case(name, covers)(fn)
        OWN.append((name, fn))
        return fn
    return deco


def _conv_case(N, H, W, Cin, Cout, ks, stride, pad, relu, seed):
    def fn(b):
        O, L, lib, P = _mods()
        x = b.inp(_rand((N, H, W, Cin), seed), ld=Cin + 5, name="x")
        w = b.inp(P.pack_conv_f32(_rand((Cout, Cin, ks, ks), seed + 1, (Cin * ks * ks) ** -0.5)), name="w packed")
        bias = b.inp(_rand((Cout,), seed + 2), name="bias")
        Ho, Wo = O.conv_out_hw(H, W, ks, stride, (pad, pad))
        out = b.out((N, Ho, Wo, Cout), F32, ld=Cout + 3, name="out")
        O.conv2d_f32(x, w, bias, Cout, ks, stride, pad, relu=relu, out=out)
        assert not bool(torch.isnan(out).any()), "a tap read poison: an ld gap, a guard, or a weight row that is not there"
        return {"out": out}
    return fn


case("conv2d_f32 11x11 / 4 pad 2, 2x27x31x3 -> 37 channels (partial row and column tiles), ld_x 8, ld_out 40", [CONV])(
    _conv_case(2, 27, 31, 3, 37, 11, 4, 2, True, 901))
case("conv2d_f32 3x3 pad 1, 1x13x11x192 -> 70 channels (two row tiles, two column tiles), no ReLU", [CONV])(
    _conv_case(1, 13, 11, 192, 70, 3, 1, 1, False, 904))


@case("maxpool3s2_f32 2x7x8x5 -> 3x3 (floor drops a column), ld_x 9, ld_out 7", [POOL])
def _pool_case(b):
    O, L, lib, P = _mods()
    x = b.inp(_rand((2, 7, 8, 5), 911, 1.0, -3.0), ld=9, name="x")
    out = b.out((2, 3, 3, 5), F32, ld=7, name="out")
    O.maxpool3s2_f32(x, out=out)
    assert not bool(torch.isnan(out).any())
    return {"out": out}


@case("lpips_input_f32 2 pairs of 3x5x7 -> [4, 5, 7, 3], ld_out 8", [INPUT])
def _input_case(b):
    O, L, lib, P = _mods()
    g = torch.Generator().manual_seed(921)
    samples = b.inp(torch.rand((2, 3, 5, 7), generator=g), name="samples")
    images = b.inp(torch.rand((2, 3, 5, 7), generator=g) * 2.0 - 1.0, name="images")
    shift, scale = b.inp(torch.tensor([-.030, -.088, -.188]), name="shift"), b.inp(torch.tensor([.458, .448, .450]), name="scale")
    assert samples.is_contiguous() and images.is_contiguous()
    out = b.out((4, 5, 7, 3), F32, ld=8, name="out")
    O.lpips_input(samples, images, shift, scale, quantise=True, out=out)
    assert not bool(torch.isnan(out).any())
    return {"out": out}


def _layer_case(N, h, w, C, accumulate, seed):
    def fn(b):
        O, L, lib, P = _mods()
        feats = b.inp(_rand((2 * N, h, w, C), seed).clamp_min(0.0), ld=C + 6, name="feats")
        lin = b.inp(_rand((C,), seed + 1).abs(), name="lin")
        out = b.inout(_rand((N,), seed + 2), name="out") if accumulate else b.out((N,), F32, name="out")
        need = lib.udt_lpips_layer_scratch_bytes(N, h * w)
        assert need == N * ((h * w + 63) // 64) * 4
        scratch = b.scratch(need, name="layer partials", dtype=U8)
        O.lpips_layer(feats, lin, out, accumulate, scratch=scratch)
        assert not bool(torch.isnan(out).any()), "a pixel read poison"
        assert lib.udt_lpips_layer_f32(feats.data_ptr(), lin.data_ptr(), out.data_ptr(), N, h * w, C, feats.stride(2), 0,
                                       scratch.data_ptr(), need - 1, O._stream()) == -3          # UDT_ERR_WORKSPACE: one byte less is refused
        return {"out": out}
    return fn


case("lpips_layer_f32 3 pairs, 9x15 pixels (3 partials per pair, the last of 7 pixels), C 70, overwrite", [LAYER, LAYER_Q])(
    _layer_case(3, 9, 15, 70, False, 931))
case("lpips_layer_f32 2 pairs, 3x5 pixels, C 384, accumulate into out", [LAYER, LAYER_Q])(_layer_case(2, 3, 5, 384, True, 934))


@pytest.mark.parametrize("idx", range(len(OWN)), ids=[c[0] for c in OWN])
def test_lpips_footprint(env, idx):
    name, fn = OWN[idx]
    table._run_case(name, fn, env.dev)
