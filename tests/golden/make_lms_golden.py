"""Generate tests/golden/lms_golden.npz by running the REAL reference's LinearMultistepSampler (reference sampling.py:180-215,
sampling_utils.py:12-24) on the CPU.

    UDT_REFERENCE=<reference checkout> python tests/golden/make_lms_golden.py        # under a minute; a re-run is byte-identical

Imports the reference through make_golden.py's recipe and drives it with make_sampler_golden.py's toy network; neither is changed.
Three parts:
  * the reference's own ``linear_multistep_coeff(order, t, i, j)`` for the 20- and 50-step LegacyDDPM schedules, orders 1-4, every
    valid (i, j) (keys ``coef_<steps>_o<order>``, [steps, order], NaN where the reference refuses the order; ``coef_<steps>_sigmas``
    is the schedule).  t is the fp32 schedule (``sigmas.cpu().numpy()``, what the reference's __call__ passes) widened to float64,
    so quad integrates in float64: under NumPy 2 the fp32 array itself would evaluate the integrand in float32 (~1e-7 relative);
  * LinearMultistepSampler driven by the toy network through the reference's own DiscreteDenoiser (quantised sigma, EpsScaling) and
    VanillaCFG: orders 1-4 over 20 steps, order 4 over 50 steps, and order 4 from init_step 3 of 20 -> the latent after every step
    (keys ``toy_<case>_*``).  It pins the host coefficients and the history ring of the fused step (tests/test_lms_cpu.py);
  * the engine (make_golden.py's synthetic weights, the G9 batch: 256x256, "TEXT", batch 1, CFG 5) sampled by LMS (order 4),
    20 steps -> x0, the latent RMS after every step, the final latent and a decoded sub-sample (keys ``lms_20_*``).

REFERENCE QUIRKS:
  * LinearMultistepSampler.__call__ calls its first argument as a bare denoiser, ``denoiser(*guider.prepare_inputs(...), **kwargs)``,
    where the other reference samplers take the engine; it is driven here with ``lambda x, s, c: model.denoiser(net, x, s, c)``.
  * __call__ has no init_step: it would be forwarded into that denoiser call.  The init_step case instead runs the reference over
    the truncated schedule sigmas[init_step:], with x scaled by the FULL schedule's sqrt(1 + sigma_0^2) (what this package does); the
    truncated run's step i' is step init_step + i' of the full schedule, with cur_order = min(i' + 1, order).

The trajectory is recorded from the denoiser's input (x before every step) and the returned latent.
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import time

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (install_stubs / import_reference / strip_ckpt; exits without UDT_REFERENCE)
import make_sampler_golden as SG  # noqa: E402  (toy_network, TOY_SEEDS, TOY_HW, make_sampler)

from udifftext_amd import synth  # noqa: E402

COEF_STEPS = (20, 50)
COEF_ORDERS = (1, 2, 3, 4)
# toy runs: case -> (order, steps, init_step)
TOY_RUNS = {f"lms_o{o}_20": (o, 20, 0) for o in (1, 2, 3, 4)}
TOY_RUNS["lms_o4_50"] = (4, 50, 0)
TOY_RUNS["lms_o4_20_init3"] = (4, 20, 3)
ENGINE_RUN = ("lms_20", 4, 20, 505)                   # name, order, steps, seed


def run(sampler, net, denoiser, x0, cond, uc, init_step=0):
    """the reference __call__ with a wrapped denoiser; -> (final latent, latent after every step)"""
    inputs = []

    def bare_denoiser(x, s, c):
        inputs.append(x[: x.shape[0] // 2].clone())              # the CFG pair's first half is x itself
        return denoiser(net, x, s, c)

    if init_step:
        full = sampler.prepare_sampling_loop

        def truncated(x, cond, uc=None, num_steps=None):
            x, s_in, sigmas, num_sigmas, cond, uc = full(x, cond, uc, num_steps)
            return x, s_in, sigmas[init_step:], num_sigmas - init_step, cond, uc

        sampler.prepare_sampling_loop = truncated
    with contextlib.redirect_stdout(io.StringIO()):
        z = sampler(bare_denoiser, x0.clone(), cond=cond, uc=uc)
    return z, torch.stack(inputs[1:] + [z], 0)


def main():
    t0 = time.time()
    torch.set_grad_enabled(False)
    MG.import_reference()
    from sgm.util import instantiate_from_config
    import sgm.modules.diffusionmodules.sampling as S
    from sgm.modules.diffusionmodules.sampling_utils import linear_multistep_coeff

    out = {}
    # ---------------------------------------------------------------- the reference's quadrature coefficients
    for steps in COEF_STEPS:
        sigmas = SG.make_sampler(S, "LinearMultistepSampler", steps, {}, 5.0).discretization(steps, device="cpu")
        t32 = sigmas.detach().cpu().numpy()
        t = t32.astype(np.float64)
        out[f"coef_{steps}_sigmas"] = t32
        worst = 0.0
        for order in COEF_ORDERS:
            c = np.full((steps, order), np.nan)
            for i in range(order - 1, steps):
                for j in range(order):
                    c[i, j] = linear_multistep_coeff(order, t, i, j)
                    c32 = linear_multistep_coeff(order, t32, i, j)
                    worst = max(worst, abs(c32 - c[i, j]) / max(abs(c[i, j]), 1e-300))
            out[f"coef_{steps}_o{order}"] = c
        print(f"[lms golden] {steps}-step coefficients; the fp32 array's values differ by up to {worst:.2e} relative")

    cfg = yaml.safe_load(open(os.path.join(MG.REF, "configs/test/textdesign_sd_2.yaml")))
    MG.strip_ckpt(cfg)
    model = instantiate_from_config(cfg["model"]).eval()
    torch.nn.Module.train(model.conditioner.embedders[0], False)      # (make_golden.py: the LabelEncoder dropout quirk)
    for name, p in model.state_dict().items():
        if not synth.is_computed_buffer(name):
            p.copy_(synth.synthetic_tensor(name, tuple(p.shape)))
    print(f"[lms golden] reference engine ready ({time.time() - t0:.1f}s)")

    # ---------------------------------------------------------------- toy network through the reference denoiser + guider
    out["toy_seeds"] = np.array(SG.TOY_SEEDS)
    for case, (order, steps, init_step) in TOY_RUNS.items():
        gens = [torch.Generator().manual_seed(s) for s in SG.TOY_SEEDS]
        x0 = torch.cat([torch.randn((1, 4, SG.TOY_HW, SG.TOY_HW), generator=g) for g in gens], 0).double()
        sampler = SG.make_sampler(S, "LinearMultistepSampler", steps, {"order": order}, 5.0)
        _, traj = run(sampler, SG.toy_network, model.denoiser, x0, {}, {}, init_step)
        assert traj.shape[0] == steps - init_step
        out[f"toy_{case}_x0"] = x0.numpy()
        out[f"toy_{case}_traj"] = traj.numpy()
    print(f"[lms golden] {len(TOY_RUNS)} toy trajectories ({time.time() - t0:.1f}s)")

    # ---------------------------------------------------------------- the engine on the G9 batch
    batch256 = synth.synthetic_batch(1, 256, 256, 4, seed=0)
    torch.manual_seed(1234)
    buc = {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in batch256.items()}
    buc["label"] = ["" for _ in batch256["label"]]
    buc["txt"] = ["" for _ in batch256["txt"]]
    c, uc = model.conditioner.get_unconditional_conditioning(batch256, batch_uc=buc, force_uc_zero_embeddings=["label"])
    name, order, steps, seed = ENGINE_RUN
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randn((1, 4, 32, 32), generator=gen)
    sampler = SG.make_sampler(S, "LinearMultistepSampler", steps, {"order": order}, 5.0)
    z, traj = run(sampler, model.model, model.denoiser, x0, c, uc)
    out[f"{name}_seed"] = np.array([seed])
    out[f"{name}_x0"] = x0.numpy()
    out[f"{name}_latent_rms"] = traj.pow(2).mean(dim=(1, 2, 3, 4)).sqrt().numpy()
    out[f"{name}_latent"] = z.numpy()
    out[f"{name}_decoded_sub"] = model.decode_first_stage(z)[:, :, ::8, ::8].numpy()
    print(f"[lms golden] {name} done ({time.time() - t0:.1f}s)")
    np.savez_compressed(os.path.join(HERE, "lms_golden.npz"), **out)
    print(f"[lms golden] written ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
