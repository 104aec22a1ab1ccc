"""The LPIPS kernels (csrc/lpips.hip) and udifftext_amd.lpips_alex.LPIPS on the GPU against the float64 restatement of tests/lpips_ref.py.

Convolution and layer distance are held PER ELEMENT to the bounds derived there from the kernels' stated roundings; max-pool and
input stage are bit-equal; every case prints its largest err / bound.

Whole network: no bound can be derived simply, so it is measured — the restatement is run in fp32 on the CPU on this test's own
inputs, its largest relative distance from the float64 run over the test's three pairs is taken, and the GPU is allowed 8 times
that (its summation order differs, and fp32 CPU kernels vary).  Measured on the inputs below (synthetic weights): fp32 CPU restatement
against float64 1.044e-07 relative, so the allowance is 8.354e-07; the MI355X run sits at 1.737e-07 (profiles/lpips.txt).
"""
import pytest
import torch
import torch.nn.functional as F

import evaluate_standin as S
import lpips_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


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


# ------------------------------------------------------------------------------------------------ convolution
# name -> (x shape NCHW, Cout, kernel, stride, padding)
CONV_CASES = {
    "conv1 2x3x67x75": ((2, 3, 67, 75), 64, 11, 4, 2),
    "conv2 2x64x7x9": ((2, 64, 7, 9), 192, 5, 1, 2),
    "conv3 1x192x5x7": ((1, 192, 5, 7), 384, 3, 1, 1),
    "conv4 1x384x5x7": ((1, 384, 5, 7), 256, 3, 1, 1),
    "conv5 3x256x3x3": ((3, 256, 3, 3), 256, 3, 1, 1),
    "Cout 37, Cin 3, 11x11 / 4": ((1, 3, 35, 43), 37, 11, 4, 2),
    "a single output pixel": ((1, 3, 7, 7), 64, 11, 4, 2),
    # this kernel's own tiles (128 pixels x 64 channels, K in chunks of 16): three row tiles with a partial one, two column tiles with a
    # partial one, K = 576 + a case whose K = 27 is no multiple of the chunk
    "3x3 on 2x64x12x12 -> 70": ((2, 64, 12, 12), 70, 3, 1, 1),
    "3x3 on 1x3x9x9 -> 5 (K 27)": ((1, 3, 9, 9), 5, 3, 1, 1),
}


def _conv_run(env, x, w, b, stride, pad, relu):
    Cout, _, ks, _ = w.shape
    out = env.O.conv2d_f32(_nhwc(x, env.dev), env.P.pack_conv_f32(w).to(env.dev), None if b is None else b.to(env.dev), Cout, ks, stride, pad,
                           relu=relu)
    ref, bound = R.conv(x, w, b, stride, pad, relu)
    got = _nchw(out)
    assert got.shape == ref.shape
    return got, ref, bound


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_against_float64_per_element(env, name, relu):
    shape, Cout, ks, stride, pad = CONV_CASES[name]
    seed = 100 + list(CONV_CASES).index(name) * 3
    x = _rand(shape, seed)
    w = _rand((Cout, shape[1], ks, ks), seed + 1, (shape[1] * ks * ks) ** -0.5)
    b = _rand((Cout,), seed + 2, 0.5)
    got, ref, bound = _conv_run(env, x, w, b, stride, pad, relu)
    err = (got - ref).abs()
    print(f"conv {name} {'relu' if relu else 'linear'}: out {tuple(ref.shape)}, max err/bound {float((err / bound).max()):.3f}")
    assert bool((bound > 0).all()) and bool((err <= bound).all())
    if relu:
        assert bool((got >= 0).all()) and bool((got == 0).any()) and bool((got > 0).any())


def test_conv_huge_right_column_leaves_the_left_edge_alone(env):
    """the right-most input column holds +-1e6: an output whose window does not reach it still meets its own (small) bound — a tap
    that wrapped from the left edge of a row into the end of the previous one would read it"""
    x = _rand((1, 3, 35, 43), 170)
    x[..., -1] = torch.where(_rand((1, 3, 35), 171) > 0, 1e6, -1e6)
    w, b = _rand((64, 3, 11, 11), 172, 363 ** -0.5), _rand((64,), 173, 0.5)
    got, ref, bound = _conv_run(env, x, w, b, 4, 2, False)
    err = (got - ref).abs()
    left = bound[..., :-1]                     # (8 x 10 outputs: only the last column's windows, columns 34 .. 44, reach input column 42)
    assert float(left.max()) < 1e-3 and float(bound[..., -1].min()) > 1e-1
    print(f"conv huge column: max err/bound {float((err / bound).max()):.3f}; left outputs' largest bound {float(left.max()):.2e}")
    assert bool((err <= bound).all())


def test_conv_without_bias_and_refusals_write_nothing(env):
    x, w = _rand((1, 3, 9, 9), 180), _rand((5, 3, 3, 3), 181, 27 ** -0.5)
    got, ref, bound = _conv_run(env, x, w, None, 1, 1, False)
    assert bool(((got - ref).abs() <= bound).all())
    xd, wd = _nhwc(x, env.dev), env.P.pack_conv_f32(w).to(env.dev)
    out = torch.full((1, 9, 9, 5), SENTINEL, device=env.dev)
    st = env.O._stream()
    call = lambda **k: env.lib.udt_conv2d_f32(*[{**dict(x=xd.data_ptr(), w=wd.data_ptr(), bias=None, out=out.data_ptr(), N=1, H=9, W=9,
                                                         Cin=3, ld_x=3, Cout=5, ld_out=5, ksize=3, stride=1, pad=1, relu=0, stream=st),
                                                  **k}[a] for a in ("x", "w", "bias", "out", "N", "H", "W", "Cin", "ld_x", "Cout", "ld_out",
                                                                    "ksize", "stride", "pad", "relu", "stream")])
    for bad in (dict(ksize=13), dict(stride=5), dict(stride=0), dict(pad=3), dict(ld_x=2), dict(ld_out=4), dict(H=2, W=2, ksize=7, pad=0),
                dict(N=0)):
        assert call(**bad) == -1, bad                          # UDT_ERR_BAD_SHAPE
    assert call(w=None) == -2 and call(out=None) == -2         # UDT_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError):
        env.O.conv2d_f32(xd, wd, None, 5, 3, 5, 1)
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(((_nchw(out) - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------ max-pool, input stage
@pytest.mark.parametrize("shape,shift", [((2, 64, 15, 23), 0.0), ((1, 192, 7, 8), 0.0), ((2, 5, 9, 11), -10.0), ((1, 7, 3, 3), 0.0)],
                         ids=["2x64x15x23", "1x192x7x8 floor drops a column", "all negative", "3x3 -> 1x1"])
def test_maxpool_is_bit_equal(env, shape, shift):
    x = _rand(shape, 200 + shape[1], 1.0, shift)
    if shift:
        assert float(x.max()) < 0.0
    want = F.max_pool2d(x, 3, 2)
    got = env.O.maxpool3s2_f32(_nhwc(x, env.dev)).permute(0, 3, 1, 2).contiguous().cpu()
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.contiguous().view(torch.int32))
    with pytest.raises(ValueError):
        env.O.maxpool3s2_f32(_nhwc(x[..., :2], env.dev))
    # a NaN makes every window that holds it NaN, as F.max_pool2d does — first, middle or last element of a window
    x[0, 0, 0, 0] = x[0, 1, 1, 1] = x[0, 2, 2, 2] = float("nan")
    want = F.max_pool2d(x, 3, 2)
    got = env.O.maxpool3s2_f32(_nhwc(x, env.dev)).permute(0, 3, 1, 2).contiguous().cpu()
    assert bool(torch.isnan(want[0, :3, 0, 0]).all()) and torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


@pytest.mark.parametrize("quantise", [True, False])
def test_input_stage_is_bit_equal(env, quantise):
    base = (torch.arange(0, 256, dtype=torch.float64) / 255.0).float()
    edge = torch.cat((base, torch.nextafter(base, torch.tensor(2.0)).clamp_max(1.0), torch.nextafter(base, torch.tensor(-1.0)).clamp_min(0.0)))
    s = torch.cat((edge, torch.rand(2 * 3 * 13 * 31 - edge.numel(), generator=torch.Generator().manual_seed(7)))).reshape(2, 3, 13, 31)
    x = (s.flip(0) * 2.0 - 1.0).contiguous()
    x.view(-1)[:3] = torch.tensor([-1.0, 1.0, 0.0])
    want = R.input_stage(s, x, quantise)
    shift, scale = torch.tensor(R.SHIFT, device=env.dev), torch.tensor(R.SCALE, device=env.dev)
    got = env.O.lpips_input(s.to(env.dev), x.to(env.dev), shift, scale, quantise).permute(0, 3, 1, 2).cpu()
    assert got.shape == want.shape == (4, 3, 13, 31)
    assert torch.equal(got.contiguous().view(torch.int32), want.view(torch.int32))
    if quantise:
        # and directly against numpy on the same s and x: test.py:94 / :102, :110-113 (astype(np.uint8)), lpips.im2tensor, the scaling layer
        import numpy as np
        fake = (s.numpy().transpose(0, 2, 3, 1) * 255).astype(np.uint8)
        real = (((x + 1.0) / 2.0).numpy().transpose(0, 2, 3, 1) * 255).astype(np.uint8)
        assert fake.min() == 0 and fake.max() == 255 and real.min() == 0 and real.max() == 255
        sh = torch.Tensor([-.030, -.088, -.188])[None, :, None, None]
        sc = torch.Tensor([.458, .448, .450])[None, :, None, None]
        png = torch.cat([torch.Tensor((img / (255.0 / 2.0) - 1.0)[:, :, :, np.newaxis].transpose((3, 2, 0, 1))) for img in (*fake, *real)])
        assert torch.equal(got.contiguous().view(torch.int32), ((png - sh) / sc).view(torch.int32))


# ------------------------------------------------------------------------------------------------ layer distance
def _layer_feats(N, C, h, w, seed):
    return _rand((2 * N, C, h, w), seed).clamp_min(0.0) * (1.0 + torch.arange(C).reshape(1, C, 1, 1) / C)


LAYER_CASES = {"C 64 on 15x15": (1, 64, 15, 15), "C 384 on 3x5": (1, 384, 3, 5), "one pixel": (1, 64, 1, 1), "N 3, C 192 on 7x11": (3, 192, 7, 11),
               "more than one partial per lane: 2 pairs, 70x70": (2, 8, 70, 70)}


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("name", list(LAYER_CASES) + ["zero pixel in both", "zero pixel in one"])
def test_layer_against_float64(env, name, accumulate):
    N, C, h, w = LAYER_CASES.get(name, (2, 64, 3, 5))
    f = _layer_feats(N, C, h, w, 300 + len(name))
    if name == "zero pixel in both":
        f[:, :, 1, 2] = 0.0
    if name == "zero pixel in one":
        f[:N, :, 1, 2] = 0.0
        f[N + 1, :, 0, 0] = 0.0
    lin = _rand((C,), 301).abs()
    prev = _rand((N,), 302).abs()
    out = prev.clone().to(env.dev) if accumulate else torch.full((N,), SENTINEL, device=env.dev)
    env.O.lpips_layer(_nhwc(f, env.dev), lin.to(env.dev), out, accumulate)
    ref, bound = R.layer(f, lin, prev if accumulate else None)
    err = (out.double().cpu() - ref).abs()
    print(f"layer {name} {'accumulate' if accumulate else 'overwrite'}: d {ref.tolist()}, max err/bound {float((err / bound).max()):.3f}")
    assert bool(torch.isfinite(out).all()) and bool((err <= bound).all())
    if name.startswith("zero pixel in one"):       # that pixel contributes sum_c w_c u_c^2 of the other image: not zero, and finite
        assert float(ref.min()) > 0.0


def test_layer_refusals(env):
    f, lin, out = _nhwc(_layer_feats(1, 8, 2, 2, 1), env.dev), torch.ones(8, device=env.dev), torch.full((1,), SENTINEL, device=env.dev)
    need = env.O.lpips_layer_scratch_bytes(1, 4)
    assert need == 4 and env.O.lpips_layer_scratch_bytes(3, 65) == 3 * 2 * 4
    scratch = torch.zeros(need, dtype=torch.uint8, device=env.dev)
    st = env.O._stream()
    assert env.lib.udt_lpips_layer_f32(f.data_ptr(), lin.data_ptr(), out.data_ptr(), 1, 4, 8, 8, 0, scratch.data_ptr(), need - 1, st) == -3
    assert env.lib.udt_lpips_layer_f32(f.data_ptr(), lin.data_ptr(), out.data_ptr(), 1, 4, 8, 7, 0, scratch.data_ptr(), need, st) == -1
    assert env.lib.udt_lpips_layer_f32(f.data_ptr(), lin.data_ptr(), out.data_ptr(), 1, 4, 8, 8, 0, None, need, st) == -2
    torch.cuda.synchronize()
    assert float(out[0]) == SENTINEL


# ------------------------------------------------------------------------------------------------ the module
@pytest.fixture(scope="module")
def module(env):
    from udifftext_amd.lpips_alex import LPIPS
    return LPIPS().fill_synthetic_().to(env.dev)


def _pairs(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3, H, W), generator=g), torch.rand((n, 3, H, W), generator=g) * 2.0 - 1.0


def test_module_against_float64_at_the_measured_allowance(env, module):
    """two pairs of 3x64x96 (maps 15x23, 7x11, 3x5) and one of 3x96x64 against float64; allowance = 8 x the largest relative distance of
    the fp32 CPU restatement from float64 on these inputs, computed here.  Measured: restatement 1.044e-07, allowance 8.354e-07,
    MI355X 1.737e-07."""
    sd = {k: v.cpu() for k, v in module.state_dict().items()}
    groups = [_pairs(2, 64, 96, 401), _pairs(1, 96, 64, 402)]
    d64 = torch.cat([R.lpips(s, x, sd) for s, x in groups])
    d32 = torch.cat([R.lpips(s, x, sd, dtype=torch.float32) for s, x in groups]).double()
    got = torch.cat([module(s.to(env.dev), x.to(env.dev)) for s, x in groups]).double().cpu()
    measured = float(((d32 - d64).abs() / d64).max())
    rel = float(((got - d64).abs() / d64).max())
    print(f"LPIPS {got.tolist()} (float64 {d64.tolist()}): fp32 CPU restatement {measured:.3e} relative, allowance {8 * measured:.3e}, "
          f"GPU {rel:.3e}")
    assert got.shape == (3,) and float(d64.min()) > 1e-3 and measured > 0.0
    assert rel <= 8.0 * measured
    # run to run, and whatever else is in the batch: the same bits
    again = torch.cat([module(s.to(env.dev), x.to(env.dev)) for s, x in groups]).double().cpu()
    alone = module(groups[0][0][1:].to(env.dev), groups[0][1][1:].to(env.dev)).double().cpu()
    assert torch.equal(again, got) and torch.equal(alone, got[1:2])


def test_module_identity_is_exactly_zero_and_quantise_matters(env, module):
    s, x = _pairs(2, 64, 96, 411)
    same = module(((x + 1.0) * 0.5).to(env.dev), x.to(env.dev))
    assert same.dtype == torch.float32 and same.is_cuda and torch.equal(same.cpu(), torch.zeros(2))
    a, b = module(s.to(env.dev), x.to(env.dev), quantise=True), module(s.to(env.dev), x.to(env.dev), quantise=False)
    assert not torch.equal(a, b) and torch.allclose(a, b, rtol=0.05)
    sd = {k: v.cpu() for k, v in module.state_dict().items()}
    assert torch.allclose(b.double().cpu(), R.lpips(s, x, sd, quantise=False), rtol=1e-4)


# ------------------------------------------------------------------------------------------------ evaluate
def test_evaluate_with_lpips(env, module):
    from udifftext_amd import config as C, pipeline, synth
    H, W, STEPS, SEEDS = 64, 128, 2, [[31, 32], [33, 34]]
    engine = pipeline.build_engine(env.dev)
    cfgs = C.default_runtime_config(steps=STEPS, batch_size=2, noise_iters=0)
    batches = lambda: [synth.synthetic_batch(2, H, W, 4, seed=70 + k) for k in range(2)]
    run = lambda **kw: pipeline.evaluate(cfgs, engine, pipeline.init_sampling(STEPS, 5.0, env.dev), batches(), S.MeanReader(), env.dev,
                                         in_flight=2, fuse=1, image_seeds=SEEDS, return_samples=True, **kw)
    plain, res = run(), run(lpips=module)
    assert set(res) == set(plain) | {"lpips", "lpips_sum", "lpips_per_image"}
    assert res["accuracy"] == plain["accuracy"] and res["pred"] == plain["pred"] and res["correct"] == plain["correct"]
    for (a, za), (b, zb) in zip(res["outputs"], plain["outputs"]):
        assert torch.equal(a, b) and torch.equal(za, zb)
    want = [module(o[0], b["image"].to(env.dev)).cpu().tolist() for o, b in zip(res["outputs"], batches())]
    print(f"evaluate lpips_per_image {res['lpips_per_image']}")
    assert res["lpips_per_image"] == want and all(v > 0.0 for vs in want for v in vs)
    assert res["lpips_sum"] == sum(v for vs in want for v in vs) and res["lpips"] == res["lpips_sum"] / 4 and res["total"] == 4
