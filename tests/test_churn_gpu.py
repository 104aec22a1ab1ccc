"""EulerEDMSampler with s_churn > 0 on the MI355X: the fused churn launch (udt_unet_input_churn) against float64 and against
udt_unet_input, the sampler end to end against the REAL reference's churned trajectory and noise search
(tests/golden/churn_golden.npz), hipGraph replay against eager launches (the noise-slot rule included), the launch count of a
churned step, the lanes of predict_many, independence of batching, and the attend-and-excite / detailed / sampler_step paths.

Tolerances are the sibling samplers' (tests/test_samplers_gpu.py, tests/test_engine_gpu.py): latent rel_rms <= 6e-2 (10 chaotic
steps with random weights, as euler_a_20), decoded image <= 4e-2; predict_many vs predict 3e-2; in flight vs sequential 2e-2.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "churn_golden.npz")
REPORT = os.environ.get("UDT_PARITY_REPORT")          # optional: a file that collects the measured values, one line per check


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


def _cond(engine, cuda, seed, size=256, B=1):
    from udifftext_amd import pipeline, synth
    batch, buc = pipeline.prepare_batch(synth.synthetic_batch(B, size, size, 4, seed=seed), cuda)
    c, uc = engine.conditioner.get_unconditional_conditioning(batch, batch_uc=buc, force_uc_zero_embeddings=["label"])
    return batch, c, uc


@pytest.fixture(scope="module")
def cond256(engine, cuda):
    torch.manual_seed(1234)
    return _cond(engine, cuda, 0)


@pytest.fixture(scope="module")
def cond256b(engine, cuda):
    return _cond(engine, cuda, 3)


@pytest.fixture(scope="module")
def cg():
    return np.load(GOLD)


def _copy(b):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in b.items()}


# -------------------------------------------------------------------------------------------------------- the kernel
SENTINEL = 0x7E57                                               # bf16 bit pattern no packed value of these inputs takes


def _sentinel_xin(B, h, w, cpad, dev):
    return torch.full((2 * B, h, w, cpad), SENTINEL, dtype=torch.int16, device=dev).view(torch.bfloat16)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("cpad", [8, 16])
def test_kernel_vs_float64_and_unet_input(cuda, B, cpad):
    from udifftext_amd import ops
    torch.manual_seed(B * 100 + cpad)
    h, w = 24, 40                                              # hw = 960: not a multiple of the 256-thread block, 4 blocks per sample
    x = torch.randn((B, 4, h, w), device=cuda) * 7.0
    noise = torch.randn((B, 4, h, w), device=cuda)
    kn, c_in = 0.41, 0.37
    x0, n0 = x.clone(), noise.clone()
    xin = _sentinel_xin(B, h, w, cpad, cuda)
    ops.unet_input_churn(x, noise, xin, c_in, kn)
    torch.cuda.synchronize()
    assert torch.equal(noise, n0)
    # x <- x + kn*noise: one fp32 rounding of the sum (and one of the product without FMA contraction)
    p = float(np.float32(kn)) * n0.double()
    err = (x.double() - (x0.double() + p)).abs()
    bound = 2.0 ** -23 * (x0.double().abs() + p.abs())
    assert bool((err <= bound).all()), f"x + kn*noise: max err/bound {(err / bound).max().item():.3f}"
    assert not torch.equal(x, x0)
    # the packed pair: bit-equal to udt_unet_input on the STORED x, both halves; the other channels untouched
    xin_ref = _sentinel_xin(B, h, w, cpad, cuda)
    ops.unet_input(x, xin_ref, c_in)
    torch.cuda.synchronize()
    got, ref = xin.view(torch.int16), xin_ref.view(torch.int16)
    assert torch.equal(got[:B, ..., :4], ref[:B, ..., :4]) and torch.equal(got[B:, ..., :4], ref[B:, ..., :4])
    assert torch.equal(got[:B, ..., :4], got[B:, ..., :4])
    assert bool((got[..., 4:] == SENTINEL).all()) and bool((got[..., :4] != SENTINEL).any())
    want = (x.double() * float(np.float32(c_in))).permute(0, 2, 3, 1)
    assert (xin[:B, ..., :4].double() - want).abs().max().item() <= 2.0 ** -8 * want.abs().max().item()       # (bf16: 8 bits)


def test_kernel_rejects_bad_arguments(cuda):
    from udifftext_amd import ops
    x = torch.randn((2, 4, 8, 8), device=cuda)
    xin = torch.zeros((4, 8, 8, 8), dtype=torch.bfloat16, device=cuda)
    with pytest.raises(ValueError):                            # noise aliasing x
        ops.unet_input_churn(x, x, xin, 0.5, 0.1)
    with pytest.raises(ValueError):                            # cpad not a multiple of 8
        ops.unet_input_churn(x, torch.randn_like(x), torch.zeros((4, 8, 8, 12), dtype=torch.bfloat16, device=cuda), 0.5, 0.1)


# ------------------------------------------------------------------------------------------------ end to end vs reference
def test_churned_sampler_vs_reference_golden(engine, cond256, cg, cuda):
    """the reference EulerEDMSampler(s_churn=2), 10 steps on the G9 batch (256x256, 'TEXT', batch 1, CFG 5): latent <= 6e-2,
    decoded image <= 4e-2 — the bounds of the sibling stochastic run euler_a_20"""
    from udifftext_amd import pipeline, rng
    batch, c, uc = cond256
    run = "euler_churn_10"
    sampler = pipeline.init_sampling(10, 5.0, cuda, s_churn=2.0)
    with rng.per_image([int(cg[f"{run}_seed"][0])]):
        x0 = rng.randn((1, 4, 32, 32))
        np.testing.assert_array_equal(x0.numpy(), cg[f"{run}_x0"])
        z = sampler(engine, x0.to(cuda), cond=c, batch=batch, uc=uc)
    _check(f"{run}: latent vs reference", z.cpu(), cg[f"{run}_latent"], 6e-2)
    dec = engine.decode_first_stage(z)
    _check(f"{run}: decoded image vs reference", dec[:, :, ::8, ::8].cpu(), cg[f"{run}_decoded_sub"], 4e-2)


def test_noise_search_under_churn_vs_reference_golden(engine, cond256, cg, cuda):
    """get_init_noise(noise_iters=2) with s_churn=2: the candidate the reference keeps wins, and the generator has taken the
    reference's draws: candidate 0, its 2 churn draws, candidate 1, its 2 churn draws, the unused candidate 2.  In the golden
    the SECOND candidate wins (so its position behind candidate 0's churn draws is pinned); the reference's two scores are
    -0.083405 and -0.083263, 1.7e-3 apart (make_churn_golden.py: the synthetic weights allow no wider margin), against a measured
    score error of 2e-4 on the noise search (profiles/r06_parity_report.txt)"""
    from udifftext_amd import config as C, pipeline
    batch, c, uc = cond256
    sampler = pipeline.init_sampling(10, 5.0, cuda, s_churn=2.0)
    cfgs = C.default_runtime_config(steps=10, batch_size=1, noise_iters=2)
    seed = int(cg["euler_churn_search_seed"][0])
    torch.manual_seed(seed)
    xs = sampler.get_init_noise(cfgs, engine, cond=c, batch=batch, uc=uc)
    nxt = torch.randn(4)
    np.testing.assert_array_equal(xs.cpu().numpy(), cg["euler_churn_search_x0"])    # same candidate wins
    torch.manual_seed(seed)
    draws = [torch.randn((1, 4, 32, 32)) for _ in range(7)]
    assert torch.equal(nxt, torch.randn(4))
    assert any(torch.equal(xs.cpu(), draws[k]) for k in (0, 3))


# ------------------------------------------------------------------------------------------------ graph replay vs eager
def _window_only_steps_1_and_2(cuda, **kw):
    """4 steps of which only steps 1 and 2 churn: s_tmin / s_tmax between the schedule's sigmas"""
    from udifftext_amd import pipeline
    sig = pipeline.init_sampling(4, 5.0, cuda)._host_sigmas()
    s = pipeline.init_sampling(4, 5.0, cuda, s_churn=2.0, s_tmax=0.5 * (sig[0] + sig[1]), s_tmin=0.5 * (sig[2] + sig[3]), **kw)
    assert [i for i, (e,) in s.plans(s._host_sigmas()) if e.churn != 0.0] == [1, 2]
    return s


@pytest.mark.parametrize("window", [False, True])
def test_graph_replay_matches_eager_launches(engine, cond256, cond256b, cuda, window):
    """the same launches, captured per step index and replayed — bit-equal; a second batch through rebind() re-uses the runner;
    the static noise buffer is refreshed per run.  window: only steps 1 and 2 of 4 churn, reading slots 0 and 1"""
    from udifftext_amd import pipeline
    batch, c, uc = cond256
    make = (lambda: _window_only_steps_1_and_2(cuda)) if window else (lambda: pipeline.init_sampling(4, 5.0, cuda, s_churn=2.0))
    torch.manual_seed(5)
    x0 = torch.randn((1, 4, 32, 32), device=cuda)
    eager, graphed = make(), make()
    eager.use_graphs = False
    noise = eager.draw_step_noise(x0.shape, cuda)
    assert noise.shape == ((2 if window else 4), 1, 4, 32, 32)
    ze = eager(engine, x0.clone(), cond=c, batch=batch, uc=uc, noise=noise)
    zg = graphed(engine, x0.clone(), cond=c, batch=batch, uc=uc, noise=noise)
    assert graphed.use_graphs and len(graphed._graphed) == 1, "graph capture fell back to eager launches"
    assert torch.equal(ze, zg)
    b2, c2, uc2 = cond256b
    gs = next(iter(graphed._graphed.values()))
    n_graphs = len(gs.graphs)
    assert tuple(gs.noise.shape) == tuple(noise.shape)
    ze2 = eager(engine, x0.clone(), cond=c2, batch=b2, uc=uc2, noise=noise)
    zg2 = graphed(engine, x0.clone(), cond=c2, batch=b2, uc=uc2, noise=noise)
    assert next(iter(graphed._graphed.values())) is gs and len(gs.graphs) == n_graphs == 4
    assert torch.equal(ze2, zg2) and not torch.equal(ze, ze2)
    other = torch.randn_like(noise)
    zg3 = graphed(engine, x0.clone(), cond=c2, batch=b2, uc=uc2, noise=other)
    assert not torch.equal(zg3, zg2)
    assert torch.equal(zg3, eager(engine, x0.clone(), cond=c2, batch=b2, uc=uc2, noise=other))
    if window:                                                 # slot rule: swapping the two slots changes the result
        assert not torch.equal(graphed(engine, x0.clone(), cond=c2, batch=b2, uc=uc2, noise=noise.flip(0).contiguous()), zg2)
    # a deterministic run and a churned run of one schedule never share a runner
    plain = pipeline.init_sampling(4, 5.0, cuda)
    assert plain._runner_key(engine, x0, plain.plans(plain._host_sigmas())) != graphed._runner_key(
        engine, x0, graphed.plans(graphed._host_sigmas()))
    assert not torch.equal(plain(engine, x0.clone(), cond=c2, batch=b2, uc=uc2), zg2)


def test_launch_count_of_a_churned_step(engine, cond256, cuda, monkeypatch):
    """a churned step has the deterministic step's launches: its noise lands in the launch that packs the UNet input"""
    from sgm.modules.diffusionmodules.sampling import _Stepper
    from udifftext_amd import ops
    batch, c, uc = cond256
    s = _window_only_steps_1_and_2(cuda)
    plans = dict(s.plans(s._host_sigmas()))
    calls = {"unet_input": 0, "unet_input_churn": 0, "axpy_": 0}
    for nm in calls:
        def counted(*a, _f=getattr(ops, nm), _nm=nm, **k):
            calls[_nm] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, nm, counted)
    stepper = _Stepper(engine, c, uc, 1, (32, 32), 5.0)
    torch.manual_seed(2)
    x = torch.randn((1, 4, 32, 32), device=cuda) * s._host_sigmas()[0]
    noise = torch.randn((1, 4, 32, 32), device=cuda)
    stepper.run_plan({"x": x}, plans[1], noise)                # churned
    assert calls == {"unet_input": 0, "unet_input_churn": 1, "axpy_": 0}
    stepper.run_plan({"x": x}, plans[3], None)                 # not churned
    assert calls == {"unet_input": 1, "unet_input_churn": 1, "axpy_": 0}
    stepper.check()
    assert bool(torch.isfinite(x).all())
    with pytest.raises(ValueError, match="draw"):              # a churned step without its draw is an error, not a silent plain step
        stepper.run_plan({"x": x}, plans[2], None)


# ------------------------------------------------------------------------------------------------------------- lanes
def test_predict_many_matches_predict(engine, cuda):
    """2 lanes x 2 fused batches with per-image seeds against predict() batch by batch under the same seeds"""
    from udifftext_amd import config as C, pipeline, rng, synth
    cfgs = C.default_runtime_config(steps=3, batch_size=1, noise_iters=0)
    batches = [synth.synthetic_batch(1, 256, 256, 4, seed=60 + i) for i in range(4)]
    seeds = [[700 + i] for i in range(4)]
    seq = pipeline.init_sampling(3, 5.0, cuda, s_churn=2.0)
    ref = []
    for b, s in zip(batches, seeds):
        with rng.per_image(s):
            ref.append(pipeline.predict(cfgs, engine, seq, _copy(b)))
    par = pipeline.init_sampling(3, 5.0, cuda, s_churn=2.0)
    got = pipeline.predict_many(cfgs, engine, par, batches, in_flight=2, fuse=2, image_seeds=seeds)
    assert len(got) == len(ref) and len(par._in_flight) == 2
    for i, ((s_ref, z_ref), (s_got, z_got)) in enumerate(zip(ref, got)):
        _check(f"euler churn: predict_many latent of batch {i} vs predict", z_got.cpu(), z_ref.cpu(), 3e-2)
        _check(f"euler churn: predict_many image of batch {i} vs predict", s_got.cpu(), s_ref.cpu(), 3e-2)


def test_sample_in_flight_matches_sequential(engine, cond256, cond256b, cuda):
    from udifftext_amd import pipeline
    _, c, uc = cond256
    _, c2, uc2 = cond256b
    torch.manual_seed(11)
    xa, xb = torch.randn((1, 4, 32, 32), device=cuda), torch.randn((1, 4, 32, 32), device=cuda)
    seq = pipeline.init_sampling(4, 5.0, cuda, s_churn=2.0)
    na, nb = seq.draw_step_noise(xa.shape, cuda), seq.draw_step_noise(xb.shape, cuda)
    za, zb = seq(engine, xa.clone(), cond=c, uc=uc, noise=na), seq(engine, xb.clone(), cond=c2, uc=uc2, noise=nb)
    par = pipeline.init_sampling(4, 5.0, cuda, s_churn=2.0)
    for _ in range(2):                                          # second round replays through rebind()
        ya, yb = par.sample_in_flight(engine, [xa.clone(), xb.clone()], [c, c2], [uc, uc2], noises=[na, nb])
        _check("euler churn: 2 batches in flight, batch A vs sequential", ya.cpu(), za.cpu(), 2e-2)
        _check("euler churn: 2 batches in flight, batch B vs sequential", yb.cpu(), zb.cpu(), 2e-2)
    assert len(par._in_flight) == 2 and par.use_graphs


def test_churn_noise_is_independent_of_batching(engine, cuda):
    """image 0 of a batch of 2 vs the same image alone under the same per-image seeds: only the batch-dependence of the arithmetic
    separates them (different noise would be an O(1) difference) — the 6e-2 the deterministic Euler pair is held to"""
    from udifftext_amd import config as C, parallel, pipeline, rng, synth
    gb = synth.synthetic_batch(2, 256, 256, 4, seed=21)
    out = {}
    sampler = pipeline.init_sampling(10, 5.0, cuda, s_churn=2.0)
    for tag, b, seeds in (("pair", gb, [31, 32]), ("alone", parallel.slice_batch(gb, 0, 1), [31])):
        cfgs = C.default_runtime_config(steps=10, batch_size=len(seeds), noise_iters=0)
        with rng.per_image(seeds):
            _, z = pipeline.predict(cfgs, engine, sampler, _copy(b))
        out[tag] = z[:1].cpu()
    _check("euler churn: image 0 in a batch of 2 vs alone", out["pair"], out["alone"], 6e-2)


# ------------------------------------------------------------------------------- attend-and-excite, detailed, sampler_step
def test_attend_and_excite_with_churn(engine, cond256, cuda, tmp_path, monkeypatch):
    from udifftext_amd import pipeline
    monkeypatch.chdir(tmp_path)                                 # (the loop may write ./temp/inters/<name>.gif)
    batch, c, uc = cond256
    torch.manual_seed(6)
    x0 = torch.randn((1, 4, 32, 32), device=cuda)
    zs = {}
    for churn in (2.0, 0.0):
        sampler = pipeline.init_sampling(4, 5.0, cuda, s_churn=churn)
        torch.manual_seed(7)
        zs[churn] = sampler(engine, x0.clone(), cond=c, batch=batch, uc=uc, aae_enabled=True)
        assert bool(torch.isfinite(zs[churn]).all())
        assert len(sampler.last_local_losses) == 4 and all(np.isfinite(sampler.last_local_losses))      # one per step
    assert not torch.equal(zs[2.0], zs[0.0])
    # every churned step adds noise of 0.66 sigma_i to a latent of about sigma_i: the two final latents are O(1) apart, where
    # a lost draw would leave only rounding differences (~1e-2)
    rel = ((zs[2.0] - zs[0.0]).pow(2).mean().sqrt() / zs[0.0].pow(2).mean().sqrt()).item()
    assert rel > 0.1, f"the churn draws did not reach the attend-and-excite loop (rel_rms {rel:.2e})"


def test_detailed_loop_with_churn(engine, cuda, tmp_path, monkeypatch):
    """detailed=True: the middle step runs with map emission, the loop is the same churned Euler loop — the latent equals the
    plain call's from the same draws up to the two text-attention forms' rounding (1.5e-2, tests/test_engine_gpu.py)"""
    from udifftext_amd import pipeline
    monkeypatch.chdir(tmp_path)
    batch, c, uc = _cond(engine, cuda, 9)
    sampler = pipeline.init_sampling(4, 5.0, cuda, s_churn=2.0)
    torch.manual_seed(11)
    x0 = torch.randn((1, 4, 32, 32), device=cuda)
    noise = sampler.draw_step_noise(x0.shape, cuda)
    z0 = sampler(engine, x0.clone(), cond=c, batch=batch, uc=uc, noise=noise)
    z1 = sampler(engine, x0.clone(), cond=c, batch=batch, uc=uc, noise=noise, detailed=True)
    _check("euler churn: detailed=True latent vs the plain sampler", z1.cpu(), z0.cpu(), 1.5e-2)
    assert (tmp_path / "temp" / "seg_map" / f"seg_{batch['name'][0]}.npy").exists()


def test_sampler_step_with_gamma_on_tensors(engine, cond256, cuda):
    """the reference-shaped step (sampling.py:324-353) with gamma > 0 against a torch restatement from the same draw"""
    from udifftext_amd import pipeline, rng
    batch, c, uc = cond256
    sampler = pipeline.init_sampling(10, 5.0, cuda, s_churn=2.0, s_noise=0.8)
    sig = sampler._host_sigmas()
    sigma = torch.full((1,), sig[3], device=cuda)
    nxt = torch.full((1,), sig[4], device=cuda)
    torch.manual_seed(13)
    x = torch.randn((1, 4, 32, 32), device=cuda) * sig[3]
    torch.manual_seed(14)
    got, inter, ll = sampler.sampler_step(sigma, nxt, engine, x.clone(), c, batch, uc, gamma=0.2)
    torch.manual_seed(14)
    eps = rng.randn(x.shape).to(cuda) * 0.8
    sh = sigma * 1.2
    xh = x + eps * ((sh ** 2 - sigma ** 2) ** 0.5).reshape(1, 1, 1, 1)
    den = sampler.denoise(xh, engine, sh, c, uc)
    want = xh + (xh - den) / sh.reshape(1, 1, 1, 1) * (nxt - sh).reshape(1, 1, 1, 1)
    assert inter is None
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert err <= 1e-5, f"sampler_step(gamma=0.2): relative error {err:.2e}"
    plain, _, _ = sampler.sampler_step(sigma, nxt, engine, x.clone(), c, batch, uc, gamma=0.0)
    assert not torch.equal(plain, got)


# ----------------------------------------------------------------------------------------------------- unchanged default
def test_default_is_unchanged_by_the_churn_arguments(engine, cond256, cuda):
    from udifftext_amd import pipeline
    batch, c, uc = cond256
    torch.manual_seed(9)
    x0 = torch.randn((1, 4, 32, 32), device=cuda)
    a = pipeline.init_sampling(10, 5.0, cuda)
    b = pipeline.init_sampling(10, 5.0, cuda, s_churn=0.0)
    torch.manual_seed(1)
    za = a(engine, x0.clone(), cond=c, batch=batch, uc=uc)
    after = torch.randn(4)
    torch.manual_seed(1)
    assert torch.equal(after, torch.randn(4))                  # no draw was taken
    assert torch.equal(za, b(engine, x0.clone(), cond=c, batch=batch, uc=uc))
