"""The FID kernels (csrc/fid.hip) and udifftext_amd.fid_inception.FID on the GPU against the float64 restatement of tests/fid_ref.py.

Convolution, average pool, input stage, global mean and moments are held PER ELEMENT to the bounds derived there from the kernels'
stated roundings; the max-pools are bit-equal; exact-integer moments are EQUAL; every case prints its largest err / bound.

Blocks and the whole network: no bound can be derived simply, so it is measured — the restatement is run in fp32 on the CPU on the
test's own inputs, its largest distance from the float64 run relative to the float64 run's largest magnitude is taken, and the GPU is
allowed 8 times that (its summation order differs, its BatchNorm is folded, and fp32 CPU kernels vary).  Measured values on the inputs
below (synthetic weights) are in the two tests' docstrings and in profiles/fid.txt.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import evaluate_standin as S
import fid_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
HUGE = 1e30


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib, ops, packing
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)

    class Env:
        pass
    Env.O, Env.L, Env.lib, Env.P, Env.dev = ops, lib, lib.load(), packing, cuda
    return Env


def _rand(shape, seed, scale=1.0, shift=0.0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale + shift


def _nhwc(x, dev):
    return x.permute(0, 2, 3, 1).contiguous().to(dev)


def _nchw(y):
    return y.permute(0, 3, 1, 2).double().cpu()


# ------------------------------------------------------------------------------------------------ rectangular convolution
# name -> (x shape NCHW, Cout, (kh, kw), stride, (pad_h, pad_w))
CONV_CASES = {
    "1x7 p(0,3) on 2x5x5x9 -> 37 (K 35)": ((2, 5, 5, 9), 37, (1, 7), 1, (0, 3)),
    "7x1 p(3,0) on 2x5x5x9 -> 37": ((2, 5, 5, 9), 37, (7, 1), 1, (3, 0)),
    "1x7 p(0,3) on W 3 < kw": ((2, 5, 4, 3), 37, (1, 7), 1, (0, 3)),
    "7x1 p(3,0) on H 3 < kh": ((2, 5, 3, 4), 37, (7, 1), 1, (3, 0)),
    "1x3 p(0,1) on 1x448x3x3 -> 70": ((1, 448, 3, 3), 70, (1, 3), 1, (0, 1)),
    "3x1 p(1,0) on 1x448x3x3 -> 70": ((1, 448, 3, 3), 70, (3, 1), 1, (1, 0)),
    "3x3 / 2 on 2x16x17x17 -> 8x8": ((2, 16, 17, 17), 33, (3, 3), 2, (0, 0)),
    "5x5 p2 on 1x48x4x6": ((1, 48, 4, 6), 64, (5, 5), 1, (2, 2)),
    "1x1 on 3x80x1x1": ((3, 80, 1, 1), 192, (1, 1), 1, (0, 0)),
    "1x1 on 2x192x13x11 -> 70 (three row tiles, two column tiles)": ((2, 192, 13, 11), 70, (1, 1), 1, (0, 0)),
}


def _conv_run(env, x, w, b, stride, pad, relu):
    Cout, _, kh, kw = w.shape
    out = env.O.conv2d_rect_f32(_nhwc(x, env.dev), env.P.pack_conv_f32(w).to(env.dev), None if b is None else b.to(env.dev), Cout, (kh, kw),
                                stride, pad, relu=relu)
    ref, bound = R.conv(x, w, b, stride, pad, relu)
    got = _nchw(out)
    assert got.shape == ref.shape
    return got, ref, bound


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_rect_conv_against_float64_per_element(env, name, relu):
    shape, Cout, kernel, stride, pad = CONV_CASES[name]
    seed = 500 + list(CONV_CASES).index(name) * 3
    x = _rand(shape, seed)
    w = _rand((Cout, shape[1], *kernel), seed + 1, (shape[1] * kernel[0] * kernel[1]) ** -0.5)
    b = _rand((Cout,), seed + 2, 0.5)
    got, ref, bound = _conv_run(env, x, w, b, stride, pad, relu)
    err = (got - ref).abs()
    print(f"rect conv {name} {'relu' if relu else 'linear'}: out {tuple(ref.shape)}, max err/bound {float((err / bound).max()):.3f}")
    assert bool((bound > 0).all()) and bool((err <= bound).all())
    if relu:
        assert bool((got >= 0).all()) and bool((got == 0).any()) and bool((got > 0).any())


def test_rect_conv_huge_right_column_and_huge_top_row_stay_where_they_are(env):
    """1x7: the right-most input column holds +-1e6 — an output whose window does not reach it still meets its own (small) bound; a
    tap that wrapped from the left edge of a row into the end of the previous one would read it.  7x1: the same with the top ROW of
    every image — a tap above the first row that wrapped into the image before it (or below the last into the next) would read it."""
    x = _rand((2, 5, 6, 20), 570)
    x[..., -1] = torch.where(_rand((2, 5, 6), 571) > 0, 1e6, -1e6)
    w, b = _rand((37, 5, 1, 7), 572, 35 ** -0.5), _rand((37,), 573, 0.5)
    got, ref, bound = _conv_run(env, x, w, b, 1, (0, 3), False)
    err = (got - ref).abs()
    left = bound[..., :16]                     # (only the windows of output columns 16 .. 19, columns ox - 3 .. ox + 3, reach input column 19)
    assert float(left.max()) < 1e-3 and float(bound[..., 16:].min()) > 1e-2
    print(f"rect conv huge column: max err/bound {float((err / bound).max()):.3f}; left outputs' largest bound {float(left.max()):.2e}")
    assert bool((err <= bound).all())
    x = _rand((2, 5, 20, 6), 575)
    x[:, :, 0, :] = torch.where(_rand((2, 5, 6), 576) > 0, 1e6, -1e6)
    w = _rand((37, 5, 7, 1), 577, 35 ** -0.5)
    got, ref, bound = _conv_run(env, x, w, b, 1, (3, 0), False)
    err = (got - ref).abs()
    below = bound[..., 4:, :]                  # (only output rows 0 .. 3 reach input row 0; the last rows' windows end in padding)
    assert float(below.max()) < 1e-3 and float(bound[..., :4, :].min()) > 1e-2
    print(f"rect conv huge row: max err/bound {float((err / bound).max()):.3f}; lower outputs' largest bound {float(below.max()):.2e}")
    assert bool((err <= bound).all())


def test_rect_conv_reads_and_writes_channel_slices(env):
    """x is channels 3 .. 7 of a 15-wide map whose other channels hold 1e30, out is channels 4 .. 40 of a 50-wide map of sentinels"""
    x, w, b = _rand((2, 5, 5, 9), 580), _rand((37, 5, 1, 7), 581, 35 ** -0.5), _rand((37,), 582, 0.5)
    wide_x = torch.full((2, 5, 9, 15), HUGE, device=env.dev)
    wide_x[..., 3:8] = _nhwc(x, env.dev)
    wide_o = torch.full((2, 5, 9, 50), SENTINEL, device=env.dev)
    env.O.conv2d_rect_f32(wide_x[..., 3:8], env.P.pack_conv_f32(w).to(env.dev), b.to(env.dev), 37, (1, 7), 1, (0, 3), relu=False,
                          out=wide_o[..., 4:41])
    ref, bound = R.conv(x, w, b, 1, (0, 3), False)
    assert bool(((_nchw(wide_o[..., 4:41]) - ref).abs() <= bound).all())
    assert bool((wide_o[..., :4] == SENTINEL).all()) and bool((wide_o[..., 41:] == SENTINEL).all())
    dense = env.O.conv2d_rect_f32(_nhwc(x, env.dev), env.P.pack_conv_f32(w).to(env.dev), b.to(env.dev), 37, (1, 7), 1, (0, 3))
    assert torch.equal(dense, wide_o[..., 4:41])                # the same bits for every ld


def test_rect_conv_refusals_write_nothing_and_square_calls_equal_conv2d_f32(env):
    x, w, b = _rand((1, 3, 9, 9), 590), _rand((5, 3, 3, 3), 591, 27 ** -0.5), _rand((5,), 592, 0.5)
    xd, wd, bd = _nhwc(x, env.dev), env.P.pack_conv_f32(w).to(env.dev), b.to(env.dev)
    out = torch.full((1, 9, 9, 5), SENTINEL, device=env.dev)
    st = env.O._stream()
    names = ("x", "w", "bias", "out", "N", "H", "W", "Cin", "ld_x", "Cout", "ld_out", "kh", "kw", "stride", "pad_h", "pad_w", "relu", "stream")
    base = dict(x=xd.data_ptr(), w=wd.data_ptr(), bias=None, out=out.data_ptr(), N=1, H=9, W=9, Cin=3, ld_x=3, Cout=5, ld_out=5, kh=3, kw=3,
                stride=1, pad_h=1, pad_w=1, relu=0, stream=st)
    call = lambda **k: env.lib.udt_conv2d_rect_f32(*[{**base, **k}[a] for a in names])
    for bad in (dict(kh=12), dict(kw=0), dict(pad_w=3), dict(pad_h=3), dict(pad_w=-1), dict(ld_out=4), dict(ld_x=2), dict(stride=5),
                dict(H=2, kh=7, pad_h=0), dict(W=2, kw=7, pad_w=0), dict(N=0)):
        assert call(**bad) == -1, bad                          # UDT_ERR_BAD_SHAPE
    assert call(w=None) == -2 and call(out=None) == -2         # UDT_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError):
        env.O.conv2d_rect_f32(xd, wd, None, 5, (3, 3), 1, (3, 1))
    # square geometry: the same kernel, the same bits as udt_conv2d_f32
    for shape, Cout, ks, stride, pad in (((2, 3, 35, 43), 37, 11, 4, 2), ((2, 64, 12, 12), 70, 3, 1, 1), ((1, 48, 4, 6), 64, 5, 1, 2)):
        x, w, b = _rand(shape, 593), _rand((Cout, shape[1], ks, ks), 594, (shape[1] * ks * ks) ** -0.5), _rand((Cout,), 595, 0.5)
        xd, wd, bd = _nhwc(x, env.dev), env.P.pack_conv_f32(w).to(env.dev), b.to(env.dev)
        a = env.O.conv2d_f32(xd, wd, bd, Cout, ks, stride, pad, relu=True)
        c = env.O.conv2d_rect_f32(xd, wd, bd, Cout, (ks, ks), stride, (pad, pad), relu=True)
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)) and bool((a > 0).any())


# ------------------------------------------------------------------------------------------------ pools
POOL_SHAPES = [(2, 5, 1, 1), (1, 7, 2, 3), (2, 64, 5, 5)]


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["2x5x1x1", "1x7x2x3", "2x64x5x5"])
def test_average_pool_excludes_padding(env, shape):
    """window sizes 1 (1x1 map), 2, 4, 6 (2x3 map) and 4, 6, 9 (5x5 map)"""
    x = _rand(shape, 600 + shape[1], 1.0, 0.5)
    ref, bound = R.avg_pool(x, 1, 1)
    got = _nchw(env.O.pool3_f32(_nhwc(x, env.dev), 1, 1, True))
    err = (got - ref).abs()
    print(f"avg pool {shape}: max err/bound {float((err / bound).max()):.3f}")
    assert got.shape == ref.shape == x.shape and bool((err <= bound).all())
    if shape[2:] == (1, 1):
        assert torch.equal(got, x.double())                     # one tap, divided by 1


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=["2x5x1x1", "1x7x2x3", "2x64x5x5"])
def test_max_pool_stride_1_pad_1_is_bit_equal(env, shape):
    x = _rand(shape, 610 + shape[1], 1.0, -10.0)                # (all negative: padding must never win)
    assert float(x.max()) < 0.0
    for nan in (False, True):
        if nan:
            x[0, 0, 0, 0] = x[-1, -1, -1, -1] = float("nan")
        want = F.max_pool2d(x, 3, 1, 1)
        got = env.O.pool3_f32(_nhwc(x, env.dev), 1, 1, False).permute(0, 3, 1, 2).contiguous().cpu()
        assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(want).any()) == nan
        assert torch.equal(torch.nan_to_num(got, nan=0.0).view(torch.int32), torch.nan_to_num(want, nan=0.0).contiguous().view(torch.int32))


def test_max_pool_stride_2_pad_0_equals_maxpool3s2_and_refusals(env):
    for shape in ((2, 5, 9, 11), (1, 7, 3, 3), (2, 64, 7, 8)):
        x = _rand(shape, 620 + shape[1])
        x[0, 0, 1, 1] = float("nan")
        xd = _nhwc(x, env.dev)
        a, b = env.O.maxpool3s2_f32(xd), env.O.pool3_f32(xd, 2, 0, False)
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)) and bool(torch.isnan(a).any())
    xd = _nhwc(_rand((1, 4, 2, 2), 629), env.dev)
    out = torch.full((1, 2, 2, 4), SENTINEL, device=env.dev)
    st = env.O._stream()
    call = lambda **k: env.lib.udt_pool3_f32(*[{**dict(x=xd.data_ptr(), out=out.data_ptr(), N=1, H=2, W=2, C=4, ld_x=4, ld_out=4, stride=1,
                                                       pad=1, average=1, stream=st), **k}[a]
                                               for a in ("x", "out", "N", "H", "W", "C", "ld_x", "ld_out", "stride", "pad", "average", "stream")])
    for bad in (dict(stride=3), dict(stride=0), dict(pad=2), dict(pad=0), dict(ld_x=3), dict(ld_out=3), dict(N=0)):
        assert call(**bad) == -1, bad
    assert call(x=None) == -2
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError):
        env.O.pool3_f32(xd, 1, 0, True)
    assert call() == 0


# ------------------------------------------------------------------------------------------------ input stage, global mean
@pytest.mark.parametrize("quantise", [True, False], ids=["quantised", "continuous"])
@pytest.mark.parametrize("hw", [(8, 8), (512, 384), (300, 299)], ids=["8x8", "512x384", "300x299"])
def test_input_stage_against_float64(env, hw, quantise):
    g = torch.Generator().manual_seed(hw[0])
    s = torch.rand((1, 3, *hw), generator=g)
    x = torch.rand((1, 3, *hw), generator=g) * 2.0 - 1.0
    s.view(-1)[:3] = torch.tensor([0.0, 1.0, 1.5])
    x.view(-1)[:3] = torch.tensor([-1.0, 1.0, -1.5])              # (out of range: clamped)
    ref, bound = R.input_stage(s, x, quantise)
    got = _nchw(env.O.fid_input(s.to(env.dev), x.to(env.dev), quantise))
    err = (got - ref).abs()
    print(f"input stage {hw} {'quantised' if quantise else 'continuous'}: max err/bound {float((err / bound).max()):.3f}")
    assert got.shape == ref.shape == (2, 3, 299, 299) and bool((err <= bound).all())
    assert float(got.min()) >= -1.0 and float(got.max()) <= 1.0


def test_input_stage_levels_quantise_to_themselves_and_refusals(env):
    """a frame whose values sit exactly on k/255 is saved as k: at the frame's own size the resize is the identity, and the output is
    2 fp32(q/255) - 1, bit for bit, q the saved value"""
    k = torch.arange(256, dtype=torch.float64)
    s = (k / 255.0).float().reshape(1, 1, 16, 16).repeat(1, 3, 1, 1).contiguous()
    x = (s * 2.0 - 1.0).contiguous()
    saved = R.saved_values(s, x)
    assert torch.equal(saved[:1], k.float().reshape(1, 1, 16, 16).repeat(1, 3, 1, 1))         # the fake frame: k exactly
    assert bool(((saved[1:] - saved[:1]).abs() <= 1.0).all())    # (the real frame went through 2 s - 1 and back: k, or the level next to it)
    got = env.O.fid_input(s.to(env.dev), x.to(env.dev), True, size=16).permute(0, 3, 1, 2).cpu()
    want = (saved / 255.0) * 2.0 - 1.0                           # fp32, every operation rounded on its own
    assert want.dtype == torch.float32 and torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32))
    out = torch.full((2, 4, 4, 3), SENTINEL, device=env.dev)
    sd, xd, st = s.to(env.dev), x.to(env.dev), env.O._stream()
    f = env.lib.udt_fid_input_f32
    assert f(sd.data_ptr(), xd.data_ptr(), out.data_ptr(), 1, 16, 16, 4, 2, 1, st) == -1             # ld_out < 3
    assert f(sd.data_ptr(), xd.data_ptr(), out.data_ptr(), 0, 16, 16, 4, 3, 1, st) == -1
    assert f(sd.data_ptr(), xd.data_ptr(), out.data_ptr(), 1, 16, 16, 0, 3, 1, st) == -1
    assert f(sd.data_ptr(), None, out.data_ptr(), 1, 16, 16, 4, 3, 1, st) == -2
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("hw", [(1, 1), (8, 8)], ids=["P 1", "P 64"])
def test_mean_pixels_against_float64(env, hw):
    x = _rand((3, 70, *hw), 640 + hw[0], 1.0, 0.3)
    ref, bound = R.mean_pixels(x)
    got = env.O.mean_pixels_f32(_nhwc(x, env.dev)).double().cpu()
    err = (got - ref).abs()
    print(f"mean over {hw[0] * hw[1]} pixels: max err/bound {float((err / bound).max()):.3f}")
    assert got.shape == (3, 70) and bool((err <= bound).all())
    if hw == (1, 1):
        assert torch.equal(got, x.double().reshape(3, 70))
        out = torch.full((3, 70), SENTINEL, device=env.dev)
        xd = _nhwc(x, env.dev)
        assert env.lib.udt_mean_pixels_f32(xd.data_ptr(), out.data_ptr(), 3, 1, 70, 69, 70, env.O._stream()) == -1
        assert env.lib.udt_mean_pixels_f32(xd.data_ptr(), out.data_ptr(), 3, 0, 70, 70, 70, env.O._stream()) == -1
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ moments
def _accumulate(env, x, total=None, outer=None):
    D = x.shape[1]
    total = torch.zeros(D, dtype=torch.float64, device=env.dev) if total is None else total
    outer = torch.zeros((D, D), dtype=torch.float64, device=env.dev) if outer is None else outer
    env.O.moments_accum_f64(x, total, outer)
    return total, outer


@pytest.mark.parametrize("n,D", [(1, 1), (5, 17), (4, 64), (33, 48)])
def test_moments_of_exact_integers_equal_the_host_result(env, n, D):
    """asymmetric X (no symmetry between rows and columns, nor between columns i and j), integers up to 2^22 so that the products reach
    2^44 and stay exact in fp64: a wrong lane map of the f64 MFMA's result puts sums into the wrong rows and cannot pass"""
    r, c = torch.arange(n, dtype=torch.int64).reshape(-1, 1), torch.arange(D, dtype=torch.int64).reshape(1, -1)
    x = (((r * 2654435761 + c * 40503 + r * c * 7) % 4194301) - 2097150).float()
    assert torch.equal(x.double(), x.double().round()) and (D == 1 or not torch.equal(x[:, 0], x[:, -1]))
    xd = x.double()
    total, outer = _accumulate(env, x.to(env.dev))
    want = xd.t() @ xd
    assert float(want.abs().max()) < 2.0 ** 53 and (D == 1 or not torch.equal(want, want.flip(0).flip(1)))
    assert torch.equal(outer.cpu(), want) and torch.equal(total.cpu(), xd.sum(0))
    assert torch.equal(outer, outer.t())


def test_moments_of_random_data_accumulation_and_strides(env):
    x = _rand((33, 48), 650, 1.0, 0.5)
    s_ref, o_ref, s_bound, o_bound = R.moments(x)
    total, outer = _accumulate(env, x.to(env.dev))
    es, eo = (total.cpu() - s_ref).abs(), (outer.cpu() - o_ref).abs()
    print(f"moments 33 x 48: sum err/bound {float((es / s_bound).max()):.3f}, outer err/bound {float((eo / o_bound).max()):.3f}")
    assert bool((es <= s_bound).all()) and bool((eo <= o_bound).all())
    # two accumulating calls against one call on the concatenation: the chains of the two parts, and one more rounding of the sum
    t2, o2 = _accumulate(env, x[:13].to(env.dev))
    _accumulate(env, x[13:].to(env.dev), t2, o2)
    assert bool(((t2.cpu() - s_ref).abs() <= s_bound + R.V * s_ref.abs()).all())
    assert bool(((o2.cpu() - o_ref).abs() <= o_bound + R.V * o_ref.abs()).all())
    # rows with a stride: columns 3 .. 50 of a 56-wide matrix whose other columns hold 1e30; accumulators inside sentinels
    wide = torch.full((33, 56), HUGE, device=env.dev)
    wide[:, 3:51] = x.to(env.dev)
    tw = torch.full((48 + 16,), SENTINEL, dtype=torch.float64, device=env.dev)
    ow = torch.full((48 + 2, 48), SENTINEL, dtype=torch.float64, device=env.dev)
    tw[8:56] = 0.0
    ow[1:49] = 0.0
    env.O.moments_accum_f64(wide[:, 3:51], tw[8:56], ow[1:49])
    assert torch.equal(tw[8:56], total) and torch.equal(ow[1:49], outer)          # the same bits for every ld
    assert bool((tw[:8] == SENTINEL).all()) and bool((tw[56:] == SENTINEL).all()) and bool((ow[0] == SENTINEL).all()) and bool((ow[49] == SENTINEL).all())
    # refusals write nothing
    xd, st = x.to(env.dev), env.O._stream()
    tw.fill_(SENTINEL)
    ow.fill_(SENTINEL)
    f = env.lib.udt_moments_accum_f64
    assert f(xd.data_ptr(), tw.data_ptr(), ow.data_ptr(), 0, 48, 48, st) == -1
    assert f(xd.data_ptr(), tw.data_ptr(), ow.data_ptr(), 33, 0, 48, st) == -1
    assert f(xd.data_ptr(), tw.data_ptr(), ow.data_ptr(), 33, 48, 47, st) == -1
    assert f(None, tw.data_ptr(), ow.data_ptr(), 33, 48, 48, st) == -2 and f(xd.data_ptr(), tw.data_ptr(), None, 33, 48, 48, st) == -2
    torch.cuda.synchronize()
    assert bool((tw == SENTINEL).all()) and bool((ow == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ blocks and the module
@pytest.fixture(scope="module")
def module(env):
    from udifftext_amd.fid_inception import FID
    return FID().fill_synthetic_().to(env.dev)


@pytest.fixture(scope="module")
def sd(module):
    return {k: v.cpu() for k, v in module.state_dict().items()}


def _rel(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


BLOCK_CASES = {"Mixed_5b": (1, 192, 5, 5), "Mixed_6a": (1, 288, 5, 5), "Mixed_6b": (1, 768, 3, 3), "Mixed_7a": (1, 768, 5, 5),
               "Mixed_7b": (1, 1280, 2, 2), "Mixed_7c": (1, 2048, 2, 2)}


@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_block_against_float64_at_the_measured_allowance(env, module, sd, name):
    """concatenation order, the pool of each block (7c's is a max-pool), BatchNorm folding, the scratch-map slices.  Allowance = 8 x
    the distance of the fp32 CPU restatement from float64 on this input, relative to the largest float64 output.  Measured on the
    MI355X (fp32 CPU restatement / allowance / GPU): 5b 3.49e-07 / 2.79e-06 / 2.77e-07, 6a 1.92e-06 / 1.54e-05 / 3.22e-07, 6b 5.95e-07 /
    4.76e-06 / 1.70e-07, 7a 4.97e-07 / 3.97e-06 / 1.56e-07, 7b 1.08e-06 / 8.62e-06 / 3.11e-07, 7c 1.09e-06 / 8.69e-06 / 1.93e-07
    (profiles/fid.txt)."""
    x = _rand(BLOCK_CASES[name], 700 + len(name) + int(name[-2]), 1.0).abs()
    ref = R.BLOCKS[name](x.double(), sd)
    measured = _rel(R.BLOCKS[name](x.float(), sd), ref)
    got = _nchw(module.run_block(name, _nhwc(x, env.dev)))
    rel = _rel(got, ref)
    print(f"block {name} {tuple(x.shape)} -> {tuple(ref.shape)}: fp32 CPU restatement {measured:.3e}, allowance {8 * measured:.3e}, GPU {rel:.3e}")
    assert got.shape == ref.shape and ref.shape[1] == R.BLOCK_WIDTHS[name] and measured > 0.0
    # every branch is alive in the reference, so a swapped or missing one cannot hide behind zeros
    assert all(float(ref[:, a:b].max()) > 0.0 for a, b in zip(range(0, ref.shape[1], 64), range(64, ref.shape[1] + 1, 64)))
    assert rel <= 8.0 * measured
    if name == "Mixed_7c":                                       # the average pool there instead would be far off
        other = R.inception_e(x.double(), sd, "Mixed_7c", "avg")
        assert _rel(other, ref) > 1e3 * rel


def _frames(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3, H, W), generator=g), torch.rand((n, 3, H, W), generator=g) * 2.0 - 1.0


def test_module_features_and_statistics(env, module, sd):
    """2 + 2 frames of 64 x 96 through ``features`` against the float64 restatement; allowance = 8 x the distance of the fp32 CPU
    restatement from float64 on these frames, relative to the largest float64 feature.  Measured on the MI355X: restatement 2.518e-07,
    allowance 2.015e-06, GPU 2.081e-07 (profiles/fid.txt)."""
    from udifftext_amd.fid_inception import FIDStats
    s, x = _frames(2, 64, 96, 801)
    ref = R.features(s, x, sd)
    measured = _rel(R.features(s, x, sd, dtype=torch.float32), ref)
    feats = module.features((s.to(env.dev), x.to(env.dev)))
    got = feats.double().cpu()
    rel = _rel(got, ref)
    print(f"features {tuple(got.shape)}: fp32 CPU restatement {measured:.3e}, allowance {8 * measured:.3e}, GPU {rel:.3e}; "
          f"largest feature {float(ref.max()):.3e}")
    assert got.shape == ref.shape == (4, 2048) and feats.dtype == torch.float32 and feats.is_cuda and measured > 0.0
    assert float(ref.max()) > 0.0 and float((ref > 0).double().mean()) > 0.1
    assert rel <= 8.0 * measured
    # a frame's features do not depend on what else shares the batch, nor on the run
    assert torch.equal(module.features((s.to(env.dev), x.to(env.dev))), feats)
    assert torch.equal(module.features((s[1:].to(env.dev), x[1:].to(env.dev))), feats[[1, 3]])
    assert torch.equal(module.features(s.to(env.dev)), feats[:2])
    assert not torch.equal(module.features(s.to(env.dev), quantise=False), feats[:2])
    # the statistics of these features against the restatement's on the same features
    st = FIDStats(module).update(s.to(env.dev), x.to(env.dev))
    assert st.n == 2 and st.dim == 2048
    for k, f in enumerate((feats[:2].cpu(), feats[2:].cpu())):
        s_ref, o_ref, s_bound, o_bound = R.moments(f)
        assert bool(((st.sum[k].cpu() - s_ref).abs() <= s_bound).all()) and bool(((st.outer[k].cpu() - o_ref).abs() <= o_bound).all())
    (mu1, c1), _ = st.moments()
    mu_ref, c_ref = R.statistics(feats[:2].cpu())
    scale = float(np.abs(c_ref).max())
    assert np.allclose(mu1, mu_ref, rtol=1e-13, atol=0) and float(np.abs(c1 - c_ref).max()) <= 1e-9 * scale
    with pytest.raises(ValueError, match="at least 2 images"):
        FIDStats(module).update(s[:1].to(env.dev), x[:1].to(env.dev)).compute()


def test_fid_of_a_set_against_itself_is_zero_within_the_bound(env, module):
    """the same 6 feature rows as the fake and as the real set, on the first 64 features (a row stride of 2048 over 64 columns)"""
    from udifftext_amd.fid_inception import FIDStats
    s, _ = _frames(6, 32, 48, 811)
    full = module.features(s.to(env.dev))
    f = torch.cat((full, full), 0)[:, :64]
    assert f.stride(0) == 2048
    st = FIDStats(dim=64, device=env.dev).update_features(f)
    assert st.n == 6 and torch.equal(st.sum[0], st.sum[1]) and torch.equal(st.outer[0], st.outer[1])
    (_, c), _ = st.moments()
    got, bound = st.compute(), R.frechet_zero_bound(c)
    print(f"FID(set, set): {got:.3e}, bound {bound:.3e}, tr Sigma {float(np.trace(c)):.3e}")
    assert abs(got) <= bound
    other = FIDStats(dim=64, device=env.dev).update_features(torch.cat((full, full.flip(1)), 0)[:, :64])
    assert other.compute() > 1e3 * bound


def test_evaluate_with_fid(env, module):
    from udifftext_amd import config as C, pipeline, synth
    from udifftext_amd.fid_inception import FIDStats
    from udifftext_amd.lpips_alex import LPIPS
    H, W, STEPS, SEEDS = 64, 128, 2, [[31, 32], [33, 34]]
    engine = pipeline.build_engine(env.dev)
    lp = LPIPS().fill_synthetic_().to(env.dev)
    cfgs = C.default_runtime_config(steps=STEPS, batch_size=2, noise_iters=0)
    batches = lambda: [synth.synthetic_batch(2, H, W, 4, seed=70 + k) for k in range(2)]
    run = lambda **kw: pipeline.evaluate(cfgs, engine, pipeline.init_sampling(STEPS, 5.0, env.dev), batches(), S.MeanReader(), env.dev,
                                         in_flight=2, fuse=1, image_seeds=SEEDS, return_samples=True, **kw)
    plain, res = run(), run(fid=module, lpips=lp)
    assert set(res) == set(plain) | {"fid", "fid_stats", "fid_note", "lpips", "lpips_sum", "lpips_per_image"}
    assert res["accuracy"] == plain["accuracy"] and res["pred"] == plain["pred"] and res["correct"] == plain["correct"]
    for (a, za), (b, zb) in zip(res["outputs"], plain["outputs"]):
        assert torch.equal(a, b) and torch.equal(za, zb)
    assert res["total"] == 4 and res["fid_stats"]["n"] == 4 and "rank-deficient" in res["fid_note"]
    want = FIDStats(module)
    for o, b in zip(res["outputs"], batches()):
        want.update(o[0], b["image"].to(env.dev))
    # (evaluate: one chunk of 4; here two of 2 — chains of 4, or of 2 + 2 and one more addition, of non-negative terms: each within
    # 4 v of the exact sum, so within 8 v of each other)
    for key, mine in (("sum", want.sum.cpu()), ("outer", want.outer.cpu())):
        assert float(mine.min()) >= 0.0 and bool(((mine - res["fid_stats"][key]).abs() <= 8 * R.V * mine).all()), key
    print(f"evaluate fid {res['fid']:.6e} ({res['fid_note']})")
    assert isinstance(res["fid"], float) and np.isfinite(res["fid"]) and res["fid"] > 0.0
    want_lp = [lp(o[0], b["image"].to(env.dev)).cpu().tolist() for o, b in zip(res["outputs"], batches())]
    assert res["lpips_per_image"] == want_lp and all(v > 0.0 for vs in want_lp for v in vs)
    # a single image: no covariance, no number, a note; the keys of the run with fid alone
    one = synth.synthetic_batch(1, H, W, 4, seed=70)
    single = pipeline.evaluate(C.default_runtime_config(steps=STEPS, batch_size=1, noise_iters=0), engine,
                               pipeline.init_sampling(STEPS, 5.0, env.dev), [one], S.MeanReader(), env.dev, image_seeds=[[31]], fid=module)
    assert set(single) == {"accuracy", "correct", "total", "pred", "label", "fid", "fid_stats", "fid_note"}
    assert single["fid"] is None and "at least 2 images" in single["fid_note"] and single["fid_stats"]["n"] == 1
