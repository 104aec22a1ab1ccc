"""The sampler family beyond Euler on the MI355X: the fused step kernel (udt_cfg_sampler_step) against an fp32 torch restatement,
every new sampler end to end against the REAL reference's trajectory (tests/golden/sampler_golden.npz), hipGraph replay
against eager launches, the lanes of predict_many, and the ancestral noise's independence of batching.

Tolerances are the engine's (tests/test_engine_gpu.py): latent rel_rms <= 6e-2 (10 chaotic steps with random weights, G9),
decoded image <= 4e-2; predict_many vs predict 3e-2; the kernel alone 1e-5.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sampler_golden.npz")
REPORT = os.environ.get("UDT_PARITY_REPORT")          # optional: a file that collects the measured values, one line per check

# golden run -> (pipeline.init_sampling name, steps)
RUNS = {"dpmpp2m_20": ("dpmpp2m", 20), "euler_a_20": ("euler_a", 20), "heun_10": ("heun", 10), "dpmpp2s_a_10": ("dpmpp2s_a", 10)}
NEW = ["dpmpp2m", "heun", "euler_a", "dpmpp2s_a"]


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


@pytest.fixture(scope="module")
def cond256(engine, cuda):
    from udifftext_amd import pipeline, synth
    batch = synth.synthetic_batch(1, 256, 256, 4, seed=0)
    torch.manual_seed(1234)
    batch, buc = pipeline.prepare_batch(batch, cuda)
    c, uc = engine.conditioner.get_unconditional_conditioning(batch, batch_uc=buc, force_uc_zero_embeddings=["label"])
    return batch, c, uc


@pytest.fixture(scope="module")
def sg():
    return np.load(GOLD)


# -------------------------------------------------------------------------------------------------------- the kernel
def _restated(xin, eps, c_out, scale, kx, kd, aux, ka, prev, kp, noise, kn):
    e = eps[..., :4].permute(0, 3, 1, 2)
    B = xin.shape[0]
    du, dc = xin + c_out * e[:B], xin + c_out * e[B:]
    den = du + scale * (dc - du)
    out = kx * xin + kd * den
    for t, k in ((aux, ka), (prev, kp), (noise, kn)):
        if t is not None:
            out = out + k * t
    return out, den


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("ld", [4, 8])
@pytest.mark.parametrize("mode", ["xd", "all", "alias_xin", "alias_aux", "noise_only", "prev_only"])
def test_kernel_vs_torch(cuda, B, ld, mode):
    from udifftext_amd import ops
    torch.manual_seed(B * 100 + ld)
    h, w = 24, 40                                              # non-square, hw not a multiple of the 256-thread block
    r = lambda: torch.randn((B, 4, h, w), device=cuda)
    xin, aux, prev, noise = r(), r(), r(), r()
    eps = torch.randn((2 * B, h, w, ld), device=cuda)
    coef = dict(c_out=-3.7, scale=5.0, kx=0.93, kd=0.07, ka=1.3, kp=-0.21, kn=0.41)
    use = {"xd": (), "all": ("aux", "prev", "noise"), "alias_xin": ("aux", "prev", "noise"), "alias_aux": ("aux", "noise"),
           "noise_only": ("noise",), "prev_only": ("prev",)}[mode]
    args = {k: (v if k in use else None) for k, v in (("aux", aux), ("prev", prev), ("noise", noise))}
    want, want_den = _restated(xin, eps, coef["c_out"], coef["scale"], coef["kx"], coef["kd"], args["aux"], coef["ka"],
                               args["prev"], coef["kp"], args["noise"], coef["kn"])
    den = torch.full_like(xin, float("nan"))
    if mode == "alias_xin":
        out = xin.clone()
        ops.cfg_sampler_step(out, eps, aux=args["aux"], prev=args["prev"], noise=args["noise"], denoised=den, **coef)
    elif mode == "alias_aux":
        out = args["aux"].clone()
        ops.cfg_sampler_step(xin, eps, aux=out, noise=args["noise"], out=out, denoised=den, **coef)
    else:
        out = torch.full_like(xin, float("nan"))
        ops.cfg_sampler_step(xin, eps, aux=args["aux"], prev=args["prev"], noise=args["noise"], out=out, denoised=den, **coef)
    torch.cuda.synchronize()
    for got, ref in ((out, want), (den, want_den)):
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        assert err <= 1e-5, f"{mode}: relative error {err:.2e}"


def test_kernel_rejects_bad_arguments(cuda):
    from udifftext_amd import ops
    x = torch.randn((2, 4, 8, 8), device=cuda)
    eps = torch.randn((4, 8, 8, 4), device=cuda)
    with pytest.raises(ValueError):                            # den_out aliasing an input
        ops.cfg_sampler_step(x, eps, -1.0, 5.0, 1.0, 0.0, denoised=x)
    with pytest.raises(ValueError):                            # ld_eps not a multiple of 4
        ops.cfg_sampler_step(x, torch.randn((4, 8, 8, 6), device=cuda), -1.0, 5.0, 1.0, 0.0)


# ------------------------------------------------------------------------------------------------ end to end vs reference
@pytest.mark.parametrize("run", list(RUNS))
def test_sampler_vs_reference_golden(engine, cond256, sg, cuda, run):
    """the reference sampler on the G9 batch (256x256, 'TEXT', batch 1, CFG 5): latent <= 6e-2, decoded image <= 4e-2"""
    from udifftext_amd import pipeline, rng
    name, steps = RUNS[run]
    batch, c, uc = cond256
    sampler = pipeline.init_sampling(steps, 5.0, cuda, sampler=name)
    with rng.per_image([int(sg[f"{run}_seed"][0])]):
        x0 = rng.randn((1, 4, 32, 32))
        np.testing.assert_array_equal(x0.numpy(), sg[f"{run}_x0"])
        z = sampler(engine, x0.to(cuda), cond=c, uc=uc)
    _check(f"{run}: latent vs reference", z.cpu(), sg[f"{run}_latent"], 6e-2)
    dec = engine.decode_first_stage(z)
    _check(f"{run}: decoded image vs reference", dec[:, :, ::8, ::8].cpu(), sg[f"{run}_decoded_sub"], 4e-2)


@pytest.mark.parametrize("name", NEW)
def test_graph_replay_matches_eager_launches(engine, cond256, cuda, name):
    """the same launches, captured per step index and replayed — bit-equal; then a second batch through rebind()"""
    from udifftext_amd import pipeline, synth
    batch, c, uc = cond256
    torch.manual_seed(5)
    x0 = torch.randn((1, 4, 32, 32), device=cuda)
    eager = pipeline.init_sampling(4, 5.0, cuda, sampler=name)
    eager.use_graphs = False
    graphed = pipeline.init_sampling(4, 5.0, cuda, sampler=name)
    noise = eager.draw_step_noise(x0.shape, cuda)
    ze = eager(engine, x0.clone(), cond=c, uc=uc, noise=noise)
    zg = graphed(engine, x0.clone(), cond=c, uc=uc, noise=noise)
    assert graphed.use_graphs and len(graphed._graphed) == 1, "graph capture fell back to eager launches"
    assert torch.equal(ze, zg)
    b2 = synth.synthetic_batch(1, 256, 256, 4, seed=3)
    b2, buc2 = pipeline.prepare_batch(b2, cuda)
    c2, uc2 = engine.conditioner.get_unconditional_conditioning(b2, batch_uc=buc2, force_uc_zero_embeddings=["label"])
    gs = next(iter(graphed._graphed.values()))
    n_graphs = len(gs.graphs)
    ze2 = eager(engine, x0.clone(), cond=c2, uc=uc2, noise=noise)
    zg2 = graphed(engine, x0.clone(), cond=c2, uc=uc2, noise=noise)
    assert next(iter(graphed._graphed.values())) is gs and len(gs.graphs) == n_graphs
    assert torch.equal(ze2, zg2) and not torch.equal(ze, ze2)
    if name in ("euler_a", "dpmpp2s_a"):                       # the static noise buffer is refreshed per run
        zg3 = graphed(engine, x0.clone(), cond=c2, uc=uc2, noise=torch.randn_like(noise))
        assert not torch.equal(zg3, zg2)


@pytest.mark.parametrize("name", ["dpmpp2m", "euler_a"])
def test_predict_many_matches_predict(engine, cuda, name):
    """2 lanes x 2 fused batches with per-image seeds against predict() batch by batch under the same seeds"""
    from udifftext_amd import config as C, pipeline, rng, synth
    cfgs = C.default_runtime_config(steps=3, batch_size=1, noise_iters=0)
    batches = [synth.synthetic_batch(1, 256, 256, 4, seed=60 + i) for i in range(4)]
    seeds = [[700 + i] for i in range(4)]
    seq = pipeline.init_sampling(3, 5.0, cuda, sampler=name)
    ref = []
    for b, s in zip(batches, seeds):
        with rng.per_image(s):
            ref.append(pipeline.predict(cfgs, engine, seq, {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in b.items()}))
    par = pipeline.init_sampling(3, 5.0, cuda, sampler=name)
    got = pipeline.predict_many(cfgs, engine, par, batches, in_flight=2, fuse=2, image_seeds=seeds)
    assert len(got) == len(ref) and len(par._in_flight) == 2
    for i, ((s_ref, z_ref), (s_got, z_got)) in enumerate(zip(ref, got)):
        _check(f"{name}: predict_many latent of batch {i} vs predict", z_got.cpu(), z_ref.cpu(), 3e-2)
        _check(f"{name}: predict_many image of batch {i} vs predict", s_got.cpu(), s_ref.cpu(), 3e-2)


def test_sample_in_flight_matches_sequential(engine, cond256, cuda):
    from udifftext_amd import pipeline, synth
    _, c, uc = cond256
    b2 = synth.synthetic_batch(1, 256, 256, 4, seed=3)
    b2, buc2 = pipeline.prepare_batch(b2, cuda)
    c2, uc2 = engine.conditioner.get_unconditional_conditioning(b2, batch_uc=buc2, force_uc_zero_embeddings=["label"])
    torch.manual_seed(11)
    xa, xb = torch.randn((1, 4, 32, 32), device=cuda), torch.randn((1, 4, 32, 32), device=cuda)
    seq = pipeline.init_sampling(4, 5.0, cuda, sampler="dpmpp2s_a")
    na, nb = seq.draw_step_noise(xa.shape, cuda), seq.draw_step_noise(xb.shape, cuda)
    za, zb = seq(engine, xa.clone(), cond=c, uc=uc, noise=na), seq(engine, xb.clone(), cond=c2, uc=uc2, noise=nb)
    par = pipeline.init_sampling(4, 5.0, cuda, sampler="dpmpp2s_a")
    for _ in range(2):                                          # second round replays through rebind()
        ya, yb = par.sample_in_flight(engine, [xa.clone(), xb.clone()], [c, c2], [uc, uc2], noises=[na, nb])
        _check("dpmpp2s_a: 2 batches in flight, batch A vs sequential", ya.cpu(), za.cpu(), 2e-2)
        _check("dpmpp2s_a: 2 batches in flight, batch B vs sequential", yb.cpu(), zb.cpu(), 2e-2)


def test_euler_a_noise_is_independent_of_batching(engine, cuda):
    """image 0 of a batch of 2 vs the same image alone under the same per-image seeds: only the batch-dependence of the arithmetic
    separates them (different noise would be an O(1) difference); the Euler sampler on the same pair measures that dependence"""
    from udifftext_amd import config as C, parallel, pipeline, rng, synth
    gb = synth.synthetic_batch(2, 256, 256, 4, seed=21)
    out = {}
    for name in ("euler", "euler_a"):
        sampler = pipeline.init_sampling(10, 5.0, cuda, sampler=name)
        for tag, b, seeds in (("pair", gb, [31, 32]), ("alone", parallel.slice_batch(gb, 0, 1), [31])):
            cfgs = C.default_runtime_config(steps=10, batch_size=len(seeds), noise_iters=0)
            with rng.per_image(seeds):
                _, z = pipeline.predict(cfgs, engine, sampler, {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in b.items()})
            out[name, tag] = z[:1].cpu()
    _check("euler: image 0 in a batch of 2 vs alone", out["euler", "pair"], out["euler", "alone"], 6e-2)
    _check("euler_a: image 0 in a batch of 2 vs alone", out["euler_a", "pair"], out["euler_a", "alone"], 6e-2)


def test_init_sampling_default_is_the_euler_path(engine, cond256, cuda):
    """the default sampler is still EulerEDMSampler, and its 10-step latent is bit-equal to the directly built sampler's"""
    from sgm.modules.diffusionmodules.sampling import EulerEDMSampler
    from udifftext_amd import pipeline
    batch, c, uc = cond256
    s = pipeline.init_sampling(10, 5.0, cuda)
    assert type(s) is EulerEDMSampler
    direct = EulerEDMSampler(
        num_steps=10,
        discretization_config={"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"},
        guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 5.0}},
        s_churn=0.0, s_tmin=0.0, s_tmax=999.0, s_noise=1.0, verbose=False, device=cuda)
    torch.manual_seed(9)
    x0 = torch.randn((1, 4, 32, 32), device=cuda)
    assert torch.equal(s(engine, x0.clone(), cond=c, batch=batch, uc=uc), direct(engine, x0.clone(), cond=c, batch=batch, uc=uc))
