"""Memory footprint of the FID kernels (csrc/fid.hip) as cases of tests/test_footprint_gpu.py's table: udt_conv2d_rect_f32,
udt_pool3_f32, udt_fid_input_f32, udt_mean_pixels_f32, udt_moments_accum_f64.

The cases are appended to that module's ``CASES`` when this module is imported, as tests/test_lpips_footprint_gpu.py does it, and run
here through the table's own ``_run_case``: every operand a strided channels-last view (pixel stride ld > C) inside a NaN-poisoned
arena, every output guarded and pre-filled with the sentinel, against compact buffers, bit-equal.  None of these entry points takes
scratch.  The fp64 accumulators of the moments are handed out as fp32 arenas of twice the width and viewed as float64 (the arena
helpers know 1-, 2- and 4-byte elements): the guards on both sides hold the sentinel all the same.
"""
import pytest
import torch

import test_footprint_gpu as table
from test_footprint_gpu import F32, _mods, _rand, env  # noqa: F401  (env: the table's fixture)

pytestmark = pytest.mark.gpu

CONV, POOL, INPUT, MEAN, MOMENTS = ("udt_conv2d_rect_f32", "udt_pool3_f32", "udt_fid_input_f32", "udt_mean_pixels_f32",
                                    "udt_moments_accum_f64")
OWN = []


def case(name, covers):
    def deco(fn):
        if name not in [c[0] for c in table.CASES]:           # (a re-import must not register twice)
            table.case(name, covers)(fn)
        OWN.append((name, fn))
        return fn
    return deco


def _conv_case(N, H, W, Cin, Cout, kernel, stride, pad, relu, seed):
    def fn(b):
        O, L, lib, P = _mods()
        x = b.inp(_rand((N, H, W, Cin), seed), ld=Cin + 5, name="x")
        w = b.inp(P.pack_conv_f32(_rand((Cout, Cin, *kernel), seed + 1, (Cin * kernel[0] * kernel[1]) ** -0.5)), name="w packed")
        bias = b.inp(_rand((Cout,), seed + 2), name="bias")
        Ho, Wo = (H + 2 * pad[0] - kernel[0]) // stride + 1, (W + 2 * pad[1] - kernel[1]) // stride + 1
        out = b.out((N, Ho, Wo, Cout), F32, ld=Cout + 3, name="out")
        O.conv2d_rect_f32(x, w, bias, Cout, kernel, stride, pad, relu=relu, out=out)
        assert not bool(torch.isnan(out).any()), "a tap read poison: an ld gap, a guard, or a weight row that is not there"
        return {"out": out}
    return fn


case("conv2d_rect_f32 1x7 pad (0, 3), 2x5x9x5 -> 37 channels (K 35), ld_x 10, ld_out 40", [CONV])(
    _conv_case(2, 5, 9, 5, 37, (1, 7), 1, (0, 3), True, 941))
case("conv2d_rect_f32 7x1 pad (3, 0), 1x13x11x24 -> 70 channels (two row tiles, two column tiles), no ReLU", [CONV])(
    _conv_case(1, 13, 11, 24, 70, (7, 1), 1, (3, 0), False, 944))
case("conv2d_rect_f32 3x1 pad (1, 0) / 2 on 2x7x6x16 -> 5 channels", [CONV])(_conv_case(2, 7, 6, 16, 5, (3, 1), 2, (1, 0), True, 947))


def _pool_case(N, H, W, C, stride, pad, average, seed):
    def fn(b):
        O, L, lib, P = _mods()
        x = b.inp(_rand((N, H, W, C), seed, 1.0, -3.0), ld=C + 4, name="x")
        Ho, Wo = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
        out = b.out((N, Ho, Wo, C), F32, ld=C + 2, name="out")
        O.pool3_f32(x, stride, pad, average, out=out)
        assert not bool(torch.isnan(out).any()), "a tap read poison: the padding, an ld gap or a neighbouring image"
        return {"out": out}
    return fn


case("pool3_f32 average, stride 1, pad 1, 2x5x4x7, ld_x 11, ld_out 9", [POOL])(_pool_case(2, 5, 4, 7, 1, 1, True, 951))
case("pool3_f32 max, stride 1, pad 1, 2x1x1x5 (every tap but one is padding)", [POOL])(_pool_case(2, 1, 1, 5, 1, 1, False, 952))
case("pool3_f32 max, stride 2, pad 0, 2x7x8x5 (floor drops a column)", [POOL])(_pool_case(2, 7, 8, 5, 2, 0, False, 953))


@case("fid_input_f32 2 pairs of 3x5x7 -> [4, 299, 299, 3], ld_out 8", [INPUT])
def _input_case(b):
    O, L, lib, P = _mods()
    g = torch.Generator().manual_seed(961)
    samples = b.inp(torch.rand((2, 3, 5, 7), generator=g), name="samples")
    images = b.inp(torch.rand((2, 3, 5, 7), generator=g) * 2.0 - 1.0, name="images")
    assert samples.is_contiguous() and images.is_contiguous()
    out = b.out((4, 299, 299, 3), F32, ld=8, name="out")
    O.fid_input(samples, images, quantise=True, out=out)
    assert not bool(torch.isnan(out).any())
    return {"out": out}


@case("mean_pixels_f32 3x2x3x70 -> [3, 70], ld_x 75, ld_out 72", [MEAN])
def _mean_case(b):
    O, L, lib, P = _mods()
    x = b.inp(_rand((3, 2, 3, 70), 971), ld=75, name="x")
    out = b.out((3, 70), F32, ld=72, name="out")
    O.mean_pixels_f32(x, out=out)
    assert not bool(torch.isnan(out).any())
    return {"out": out}


@case("moments_accum_f64 n 5, D 17 (partial tiles on both axes), ld 23, accumulated into", [MOMENTS])
def _moments_case(b):
    O, L, lib, P = _mods()
    n, D = 5, 17
    x = b.inp(_rand((n, D), 981), ld=23, name="x")
    # the fp64 accumulators, with previous contents: fp32 arenas of twice the width, viewed as float64
    total32 = b.inout(_rand((D,), 982).double().view(torch.float32), name="sum")
    outer32 = b.inout(_rand((D, D), 983).double().view(torch.float32), name="outer")
    assert total32.is_contiguous() and outer32.is_contiguous() and total32.data_ptr() % 8 == 0 and outer32.data_ptr() % 8 == 0
    total, outer = total32.view(torch.float64), outer32.view(torch.float64)
    assert tuple(total.shape) == (D,) and tuple(outer.shape) == (D, D)
    O.moments_accum_f64(x, total, outer)
    assert not bool(torch.isnan(total).any()) and not bool(torch.isnan(outer).any()), "a row read poison: the ld gap or a guard"
    return {"sum": total32, "outer": outer32}


@pytest.mark.parametrize("idx", range(len(OWN)), ids=[c[0] for c in OWN])
def test_fid_footprint(env, idx):
    name, fn = OWN[idx]
    table._run_case(name, fn, env.dev)
