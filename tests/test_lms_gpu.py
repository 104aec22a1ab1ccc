"""LinearMultistepSampler on the MI355X: the fused multistep kernel (udt_cfg_multistep_step) against an fp32 torch restatement and
its argument checks, LMS 20 steps end to end against the REAL reference's trajectory (tests/golden/lms_golden.npz), hipGraph replay
against eager launches, the lanes of predict_many / predict_sharded and sample_in_flight.

Tolerances are those of tests/test_samplers_gpu.py: latent rel_rms <= 6e-2 (chaotic steps with random weights, G9), decoded image
<= 4e-2; predict_many vs predict 3e-2; batches in flight vs sequential 2e-2; the kernel alone 1e-5.  Setting UDT_PARITY_REPORT to
a file path appends every measured value to that file.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lms_golden.npz")
REPORT = os.environ.get("UDT_PARITY_REPORT")


def _check(name, got, ref, rel_rms):
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    r = (got - ref).pow(2).mean().sqrt().item() / max(ref.pow(2).mean().sqrt().item(), 1e-30)
    if REPORT:
        os.makedirs(os.path.dirname(os.path.abspath(REPORT)), exist_ok=True)
        with open(REPORT, "a") as f:
            f.write(f"{name:55s} rel_rms {r:.3e} (tol {rel_rms:.1e})\n")
    assert r <= rel_rms, f"{name}: rel_rms {r:.3e} > {rel_rms}"


@pytest.fixture(scope="module")
def engine(cuda):
    from udifftext_amd import lib, pipeline
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)
    return pipeline.build_engine(cuda)


def _cond(engine, cuda, seed):
    from udifftext_amd import pipeline, synth
    batch = synth.synthetic_batch(1, 256, 256, 4, seed=seed)
    torch.manual_seed(1234)
    batch, buc = pipeline.prepare_batch(batch, cuda)
    c, uc = engine.conditioner.get_unconditional_conditioning(batch, batch_uc=buc, force_uc_zero_embeddings=["label"])
    return c, uc


@pytest.fixture(scope="module")
def cond256(engine, cuda):
    return _cond(engine, cuda, 0)


@pytest.fixture(scope="module")
def cond256b(engine, cuda):
    return _cond(engine, cuda, 3)


# -------------------------------------------------------------------------------------------------------- the kernel
def _restated(xin, eps, c_out, scale, sigma, ks, hist):
    e = eps[..., :4].permute(0, 3, 1, 2)
    B = xin.shape[0]
    du, dc = xin + c_out * e[:B], xin + c_out * e[B:]
    den = du + scale * (dc - du)
    d = (xin - den) / sigma
    acc = ks[0] * d
    for k, h in zip(ks[1:], hist):
        acc = acc + k * h
    return xin + acc, d


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("alias", [False, True])
def test_kernel_vs_torch(cuda, B, ld, n, alias):
    from udifftext_amd import ops
    torch.manual_seed(B * 100 + ld * 10 + n)
    h, w = 24, 40                                              # non-square, hw not a multiple of the 256-thread block
    xin = torch.randn((B, 4, h, w), device=cuda)
    hist = [torch.randn((B, 4, h, w), device=cuda) for _ in range(n - 1)]
    eps = torch.randn((2 * B, h, w, ld), device=cuda)
    ks = [(-1.3, 0.41, -0.27, 0.11, -0.05, 0.031, -0.017, 0.009)[j] for j in range(n)]
    c_out, scale, sigma = -3.7, 5.0, 3.65
    want, want_d = _restated(xin.double(), eps.double(), c_out, scale, sigma, ks, [t.double() for t in hist])
    d_out = torch.full_like(xin, float("nan"))
    if alias:
        out = xin.clone()
        ret = ops.cfg_multistep_step(out, eps, c_out, scale, sigma, ks, hist=hist, d_out=d_out)
    else:
        out = torch.full_like(xin, float("nan"))
        ret = ops.cfg_multistep_step(xin, eps, c_out, scale, sigma, ks, hist=hist, d_out=d_out, out=out)
    torch.cuda.synchronize()
    assert ret is out
    for what, got, ref in (("xout", out, want), ("d_out", d_out, want_d)):
        err = (got.double() - ref).abs().max().item() / ref.abs().max().item()
        assert err <= 1e-5, f"n={n} alias={alias} {what}: relative error {err:.2e}"


def test_kernel_rejects_bad_arguments(cuda):
    from udifftext_amd import lib, ops
    x = torch.randn((2, 4, 8, 8), device=cuda)
    h1, h2, d = torch.randn_like(x), torch.randn_like(x), torch.empty_like(x)
    eps = torch.randn((4, 8, 8, 4), device=cuda)
    with pytest.raises(ValueError):                            # d_out aliasing a history term in use
        ops.cfg_multistep_step(x, eps, -1.0, 5.0, 1.0, [1.0, 0.5, 0.25], hist=[h1, h2], d_out=h2)
    with pytest.raises(ValueError):                            # d_out aliasing xin
        ops.cfg_multistep_step(x, eps, -1.0, 5.0, 1.0, [1.0], d_out=x)
    with pytest.raises(ValueError):                            # ld_eps not a multiple of 4
        ops.cfg_multistep_step(x, torch.randn((4, 8, 8, 6), device=cuda), -1.0, 5.0, 1.0, [1.0], d_out=d)
    flat = torch.randn(eps.numel() + 4, device=cuda)
    with pytest.raises(ValueError):                            # eps not 16-byte aligned
        ops.cfg_multistep_step(x, flat[1:1 + eps.numel()].view(eps.shape), -1.0, 5.0, 1.0, [1.0], d_out=d)
    with pytest.raises(ValueError):                            # sigma = 0 (to_d divides by it)
        ops.cfg_multistep_step(x, eps, -1.0, 5.0, 0.0, [1.0], d_out=d)
    # below the wrapper's own checks: the C entry point refuses n outside 1..8, a null d_out and a null history term in use
    so = lib.load()
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(n, hist=(), d_out=d):
        k = lib.MultistepCoefs(-1.0, 5.0, 1.0, n)
        for j in range(lib.MULTISTEP_MAX):
            k.k[j] = 0.5
        for j, t in enumerate(hist):
            k.hist[j + 1] = None if t is None else t.data_ptr()
        return so.udt_cfg_multistep_step(p(x), p(eps), p(x), None if d_out is None else p(d_out), 2, 64, 4, k,
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad_arg = -2
    assert call(0) == bad_arg and call(9) == bad_arg and call(-1) == bad_arg
    assert call(1, d_out=None) == bad_arg
    assert call(3, hist=(h1, None)) == bad_arg
    assert call(3, hist=(h1, h2)) == 0                        # the same call with both terms present runs
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ end to end vs reference
def test_lms_vs_reference_golden(engine, cond256, cuda):
    """the reference LinearMultistepSampler (order 4) on the G9 batch (256x256, 'TEXT', batch 1, CFG 5), 20 steps"""
    from udifftext_amd import pipeline, rng
    lg = np.load(GOLD)
    c, uc = cond256
    sampler = pipeline.init_sampling(20, 5.0, cuda, sampler="linear_multistep")
    with rng.per_image([int(lg["lms_20_seed"][0])]):
        x0 = rng.randn((1, 4, 32, 32))
        np.testing.assert_array_equal(x0.numpy(), lg["lms_20_x0"])
        z = sampler(engine, x0.to(cuda), cond=c, uc=uc)
    _check("lms_20: latent vs reference", z.cpu(), lg["lms_20_latent"], 6e-2)
    dec = engine.decode_first_stage(z)
    _check("lms_20: decoded image vs reference", dec[:, :, ::8, ::8].cpu(), lg["lms_20_decoded_sub"], 4e-2)


def test_graph_replay_matches_eager_launches(engine, cond256, cond256b, cuda):
    """6 steps (the 4-slot derivative ring wraps), captured per step index and replayed — bit-equal to eager launches;
    then a second batch through rebind(), and a run from init_step 2 (empty history) on a runner of its own"""
    from udifftext_amd import pipeline
    (c, uc), (c2, uc2) = cond256, cond256b
    torch.manual_seed(5)
    x0 = torch.randn((1, 4, 32, 32), device=cuda)
    eager = pipeline.init_sampling(6, 5.0, cuda, sampler="linear_multistep")
    eager.use_graphs = False
    graphed = pipeline.init_sampling(6, 5.0, cuda, sampler="linear_multistep")
    ze = eager(engine, x0.clone(), cond=c, uc=uc)
    zg = graphed(engine, x0.clone(), cond=c, uc=uc)
    assert graphed.use_graphs and len(graphed._graphed) == 1, "graph capture fell back to eager launches"
    gs = next(iter(graphed._graphed.values()))
    assert {f"d{m}" for m in range(4)} <= set(gs.bufs)
    assert torch.equal(ze, zg)
    n_graphs = len(gs.graphs)
    ze2 = eager(engine, x0.clone(), cond=c2, uc=uc2)
    zg2 = graphed(engine, x0.clone(), cond=c2, uc=uc2)
    assert next(iter(graphed._graphed.values())) is gs and len(gs.graphs) == n_graphs
    assert torch.equal(ze2, zg2) and not torch.equal(ze, ze2)
    ze3 = eager(engine, x0.clone(), cond=c2, uc=uc2, init_step=2)
    zg3 = graphed(engine, x0.clone(), cond=c2, uc=uc2, init_step=2)
    assert torch.equal(ze3, zg3) and not torch.equal(ze3, ze2)


def test_predict_many_matches_predict(engine, cuda):
    """3 lanes x 1 batch each, per-image seeds, 6 steps, against predict() batch by batch under the same seeds"""
    from udifftext_amd import config as Cf, pipeline, rng, synth
    cfgs = Cf.default_runtime_config(steps=6, batch_size=1, noise_iters=0)
    batches = [synth.synthetic_batch(1, 256, 256, 4, seed=80 + i) for i in range(3)]
    seeds = [[900 + i] for i in range(3)]
    seq = pipeline.init_sampling(6, 5.0, cuda, sampler="linear_multistep")
    ref = []
    for b, s in zip(batches, seeds):
        with rng.per_image(s):
            ref.append(pipeline.predict(cfgs, engine, seq, {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in b.items()}))
    par = pipeline.init_sampling(6, 5.0, cuda, sampler="linear_multistep")
    got = pipeline.predict_many(cfgs, engine, par, batches, in_flight=3, fuse=1, image_seeds=seeds)
    assert len(got) == len(ref) and len(par._in_flight) == 3
    for i, ((s_ref, z_ref), (s_got, z_got)) in enumerate(zip(ref, got)):
        _check(f"lms: predict_many latent of batch {i} vs predict", z_got.cpu(), z_ref.cpu(), 3e-2)
        _check(f"lms: predict_many image of batch {i} vs predict", s_got.cpu(), s_ref.cpu(), 3e-2)


def test_predict_sharded_matches_predict(engine, cuda):
    """one rank, a global batch of 2 images in micro-batches of 1 on 2 lanes, against predict() per image and per-image seed"""
    from udifftext_amd import config as Cf, parallel, pipeline, rng, synth
    gb = synth.synthetic_batch(2, 256, 256, 4, seed=41)
    cfgs = Cf.default_runtime_config(steps=5, batch_size=1, noise_iters=0)
    sampler = pipeline.init_sampling(5, 5.0, cuda, sampler="linear_multistep")
    (frames,) = parallel.predict_sharded(cfgs, engine, sampler, [gb], [77], micro_batch=1, in_flight=2, device=cuda)
    assert frames.shape[0] == 2
    seq = pipeline.init_sampling(5, 5.0, cuda, sampler="linear_multistep")
    for i in range(2):
        b = parallel.slice_batch(gb, i, i + 1)
        with rng.per_image([parallel.image_seed(77, i)]):
            s_ref, _ = pipeline.predict(cfgs, engine, seq, {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in b.items()})
        _check(f"lms: predict_sharded image {i} vs predict", frames[i:i + 1].cpu(), s_ref.cpu(), 3e-2)


def test_sample_in_flight_matches_sequential(engine, cond256, cond256b, cuda):
    from udifftext_amd import pipeline
    (c, uc), (c2, uc2) = cond256, cond256b
    torch.manual_seed(11)
    xa, xb = torch.randn((1, 4, 32, 32), device=cuda), torch.randn((1, 4, 32, 32), device=cuda)
    seq = pipeline.init_sampling(6, 5.0, cuda, sampler="linear_multistep")
    za, zb = seq(engine, xa.clone(), cond=c, uc=uc), seq(engine, xb.clone(), cond=c2, uc=uc2)
    par = pipeline.init_sampling(6, 5.0, cuda, sampler="linear_multistep")
    for _ in range(2):                                          # second round replays through rebind()
        ya, yb = par.sample_in_flight(engine, [xa.clone(), xb.clone()], [c, c2], [uc, uc2])
        _check("lms: 2 batches in flight, batch A vs sequential", ya.cpu(), za.cpu(), 2e-2)
        _check("lms: 2 batches in flight, batch B vs sequential", yb.cpu(), zb.cpu(), 2e-2)
