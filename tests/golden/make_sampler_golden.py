"""Generate tests/golden/sampler_golden.npz by running the REAL reference's sampler classes (HeunEDMSampler,
EulerAncestralSampler, DPMPP2SAncestralSampler, DPMPP2MSampler; reference sampling.py:140-215,423-567) on the CPU.

    UDT_REFERENCE=<reference checkout> python tests/golden/make_sampler_golden.py        # ~6 minutes

Two parts:
  * the engine (make_golden.py's import recipe and synthetic weights, the G9 batch: 256x256, "TEXT", batch 1, CFG 5) sampled
    by DPM++ 2M 20 steps, Euler ancestral 20, Heun 10 and DPM++ 2S ancestral 10 -> x0, latent RMS after every step, the final
    latent and a decoded sub-sample (keys ``<name>_*``);
  * every sampler driven by an analytic toy network through the reference's own DiscreteDenoiser (quantised sigma, EpsScaling)
    and VanillaCFG, over 20- and 50-step schedules, with eta = 0 and init_step > 0 variants -> the latent after every step
    (keys ``toy_<case>_*``).  It pins the host coefficient math of the fused step (tests/test_samplers_cpu.py).

Noise: image i of a run owns ``torch.Generator().manual_seed(seed_i)``; x0 is its first draw and the ancestral samplers'
``noise_sampler`` takes every later draw, one per step, the last step included — the draw sequence of ``rng.per_image(seeds)``
in udifftext_amd.

REFERENCE QUIRK: ``get_ancestral_step(..., eta=0)`` returns the python float 0.0 as sigma_up, which ``append_dims`` in
``ancestral_step`` cannot take (AttributeError); the eta = 0 cases run with that 0.0 as a zero tensor, the intended value.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import time
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (install_stubs / import_reference / strip_ckpt / sub; exits without UDT_REFERENCE)

from udifftext_amd import synth  # noqa: E402

DISC = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}

# engine runs: name -> (class, steps, extra params, seed)
ENGINE_RUNS = {
    "dpmpp2m_20": ("DPMPP2MSampler", 20, {}, 501),
    "euler_a_20": ("EulerAncestralSampler", 20, {"eta": 1.0, "s_noise": 1.0}, 502),
    "heun_10": ("HeunEDMSampler", 10, {"s_churn": 0.0, "s_tmin": 0.0, "s_tmax": 999.0, "s_noise": 1.0}, 503),
    "dpmpp2s_a_10": ("DPMPP2SAncestralSampler", 10, {"eta": 1.0, "s_noise": 1.0}, 504),
}

# toy runs: case -> (class, steps, extra params, init_step)
TOY_SEEDS = (11, 12)
TOY_HW = 4
TOY_RUNS = {}
for _n in (20, 50):
    TOY_RUNS[f"dpmpp2m_{_n}"] = ("DPMPP2MSampler", _n, {}, 0)
    TOY_RUNS[f"euler_a_{_n}"] = ("EulerAncestralSampler", _n, {"eta": 1.0, "s_noise": 1.0}, 0)
    TOY_RUNS[f"heun_{_n}"] = ("HeunEDMSampler", _n, {"s_churn": 0.0, "s_tmin": 0.0, "s_tmax": 999.0, "s_noise": 1.0}, 0)
    TOY_RUNS[f"dpmpp2s_a_{_n}"] = ("DPMPP2SAncestralSampler", _n, {"eta": 1.0, "s_noise": 1.0}, 0)
TOY_RUNS["dpmpp2m_20_init3"] = ("DPMPP2MSampler", 20, {}, 3)
TOY_RUNS["euler_a_20_eta0"] = ("EulerAncestralSampler", 20, {"eta": 0.0, "s_noise": 1.0}, 0)
TOY_RUNS["euler_a_20_eta05"] = ("EulerAncestralSampler", 20, {"eta": 0.5, "s_noise": 0.7}, 0)
TOY_RUNS["dpmpp2s_a_20_eta0"] = ("DPMPP2SAncestralSampler", 20, {"eta": 0.0, "s_noise": 1.0}, 0)


def toy_network(x_in, c_noise, cond):
    """eps of the CFG pair [uncond; cond] from the c_in-scaled input and the quantised timestep index"""
    n = x_in.shape[0] // 2
    t = torch.sin(c_noise.to(x_in.dtype) / 100.0).reshape(-1, 1, 1, 1) * 0.05
    return torch.cat((0.8 * torch.tanh(x_in[:n]), torch.tanh(x_in[n:] + 0.25)), 0) + t


def make_sampler(S, cls, steps, params, scale):
    return getattr(S, cls)(num_steps=steps, discretization_config=DISC,
                           guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": scale}},
                           verbose=False, device="cpu", **params)


def run(S, sampler, model, x0, cond, uc, gens, init_step=0):
    """the reference __call__ with per-image noise draws; -> (final latent, latent after every step)"""
    traj = []
    orig = sampler.sampler_step

    def recording_step(*a, **k):
        r = orig(*a, **k)
        traj.append((r[0] if isinstance(r, tuple) else r).clone())
        return r

    sampler.sampler_step = recording_step
    if hasattr(sampler, "noise_sampler"):
        sampler.noise_sampler = lambda x: torch.cat([torch.randn((1,) + tuple(x.shape[1:]), generator=g) for g in gens], 0).to(x.dtype)
    kw = {"init_step": init_step} if init_step else {}
    with contextlib.redirect_stdout(io.StringIO()):
        z = sampler(model, x0.clone(), cond=cond, uc=uc, **kw)
    assert torch.equal(traj[-1], z)
    return z, torch.stack(traj, 0)


def main():
    t0 = time.time()
    torch.set_grad_enabled(False)
    MG.import_reference()
    from sgm.util import instantiate_from_config
    import sgm.modules.diffusionmodules.sampling as S

    get_ancestral_step = S.get_ancestral_step

    def ancestral_step_eta0_as_tensor(sigma_from, sigma_to, eta=1.0):
        down, up = get_ancestral_step(sigma_from, sigma_to, eta=eta)
        return down, (torch.zeros_like(sigma_to) if not torch.is_tensor(up) else up)

    S.get_ancestral_step = ancestral_step_eta0_as_tensor

    cfg = yaml.safe_load(open(os.path.join(MG.REF, "configs/test/textdesign_sd_2.yaml")))
    MG.strip_ckpt(cfg)
    model = instantiate_from_config(cfg["model"]).eval()
    torch.nn.Module.train(model.conditioner.embedders[0], False)      # (make_golden.py: the LabelEncoder dropout quirk)
    for name, p in model.state_dict().items():
        if not synth.is_computed_buffer(name):
            p.copy_(synth.synthetic_tensor(name, tuple(p.shape)))
    print(f"[sampler golden] reference engine ready ({time.time() - t0:.1f}s)")
    out = {}

    # ---------------------------------------------------------------- toy network through the reference denoiser + guider
    toy = types.SimpleNamespace(denoiser=model.denoiser, model=toy_network)
    out["toy_seeds"] = np.array(TOY_SEEDS)
    for case, (cls, steps, params, init_step) in TOY_RUNS.items():
        gens = [torch.Generator().manual_seed(s) for s in TOY_SEEDS]
        x0 = torch.cat([torch.randn((1, 4, TOY_HW, TOY_HW), generator=g) for g in gens], 0).double()
        sampler = make_sampler(S, cls, steps, params, 5.0)
        _, traj = run(S, sampler, toy, x0, {}, {}, gens, init_step)
        out[f"toy_{case}_x0"] = x0.numpy()
        out[f"toy_{case}_traj"] = traj.numpy()
    print(f"[sampler golden] {len(TOY_RUNS)} toy trajectories ({time.time() - t0:.1f}s)")

    # ---------------------------------------------------------------- the engine on the G9 batch
    batch256 = synth.synthetic_batch(1, 256, 256, 4, seed=0)
    torch.manual_seed(1234)
    buc = {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in batch256.items()}
    buc["label"] = ["" for _ in batch256["label"]]
    buc["txt"] = ["" for _ in batch256["txt"]]
    c, uc = model.conditioner.get_unconditional_conditioning(batch256, batch_uc=buc, force_uc_zero_embeddings=["label"])

    class _TorchProxy:                                     # (make_golden.py: the samplers' torch.device on the CPU)
        def __getattr__(self, n):
            return getattr(torch, n)

        @staticmethod
        def device(*a, **k):
            return torch.device("cpu")

    S.torch = _TorchProxy()
    for name, (cls, steps, params, seed) in ENGINE_RUNS.items():
        gen = torch.Generator().manual_seed(seed)
        x0 = torch.randn((1, 4, 32, 32), generator=gen)
        sampler = make_sampler(S, cls, steps, params, 5.0)
        z, traj = run(S, sampler, model, x0, c, uc, [gen])
        out[f"{name}_seed"] = np.array([seed])
        out[f"{name}_x0"] = x0.numpy()
        out[f"{name}_latent_rms"] = traj.pow(2).mean(dim=(1, 2, 3, 4)).sqrt().numpy()
        out[f"{name}_latent"] = z.numpy()
        out[f"{name}_decoded_sub"] = model.decode_first_stage(z)[:, :, ::8, ::8].numpy()
        print(f"[sampler golden] {name} done ({time.time() - t0:.1f}s)")
    np.savez_compressed(os.path.join(HERE, "sampler_golden.npz"), **out)
    print(f"[sampler golden] written ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
