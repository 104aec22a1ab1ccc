"""Generate tests/golden/precond_golden.npz and precond_golden_disc.npz (the toy runs under DiscreteDenoiser: float64 latents after
every step of 76 runs do not fit one file under the 1 MiB limit of a committed file) by running the REAL reference's samplers and loss through its own denoisers
(denoiser.py:6-63: Denoiser, DiscreteDenoiser), scalings (denoiser_scaling.py: Eps, V, EDM), guiders (guiders.py: VanillaCFG,
IdentityGuider) and discretizations (discretizer.py: LegacyDDPM, EDM) on the CPU.

    UDT_REFERENCE=<reference checkout> python tests/golden/make_precond_golden.py        # a few minutes

Three parts (make_golden.py's import recipe and synthetic weights, make_sampler_golden.py's toy network, make_churn_golden.py's
torch proxy and recording run are reused by import):
  (a) toy trajectories in float64 on a 4x4 latent at seeds (11, 12), 20 steps: {DiscreteDenoiser, Denoiser} x {Eps, V, EDM} x
      {VanillaCFG 5, IdentityGuider} x {legacy DDPM, EDM sigma_min 0.03 sigma_max 14.6} under Euler, DPM++ 2M and Heun, plus Euler
      ancestral, DPM++ 2S ancestral, linear multistep order 4 and churned Euler (s_churn 4) under DiscreteDenoiser + V + Identity on
      the legacy schedule.  The denoisers are ``.double()``: their sigma table holds the fp32 values as float64, so the scaling is
      evaluated in float64 like everything else (and linear_multistep_coeff gets the fp32 schedule as float64 for the same reason:
      it would otherwise take its node differences in fp32).  Unguided, the toy network is the conditional half of ``toy_network``.  Stored: the
      latent after every step (``toy_<case>_traj``) and the c_noise the network saw at every evaluation (``toy_<case>_cnoise``).
  (b) the engine on the G9 batch (256x256, "TEXT", batch 1, synthetic weights) with ``model.denoiser`` swapped and nothing else:
      ``v_cfg_euler_10`` (DiscreteDenoiser + V, CFG 5, Euler 10 steps), ``edm_cont_identity_dpmpp2m_10`` (Denoiser + EDM,
      IdentityGuider, the EDM schedule above, DPM++ 2M 10 steps) -> x0, latent RMS after every step, the final latent, a decoded
      sub-sample; ``v_identity_search`` (DiscreteDenoiser + V, IdentityGuider, get_init_noise with noise_iters 2 on the default
      generator at torch.manual_seed(77)) -> the winner, both scores and their relative gap.  As in make_churn_golden.py the gap is
      compared with the 3e-2 score tolerance of tests/test_engine_gpu.py and the verdict printed: only a larger gap makes "the
      same candidate wins" a test.
  (c) the loss: StandardDiffusionLoss.get_diff_loss on the reference denoiser's output for B = 3 in float64 under autograd, pairs
      Eps/Eps, V/V, EDM/EDM and Eps/Unit under both denoisers -> per-sample loss and d mean_b(loss_b) / dF.
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

import make_golden as MG  # noqa: E402  (install_stubs / import_reference / strip_ckpt; exits without UDT_REFERENCE)
import make_sampler_golden as MSG  # noqa: E402  (toy_network, run)
import make_churn_golden as MCG  # noqa: E402  (TorchProxy, run)

from udifftext_amd import synth  # noqa: E402

MOD = "sgm.modules.diffusionmodules."
EDM = {"s_churn": 0.0, "s_tmin": 0.0, "s_tmax": 999.0, "s_noise": 1.0}
TOY_SEEDS = (11, 12)
TOY_HW = 4
STEPS = 20
SCALINGS = {"eps": ("EpsScaling", "EpsWeighting", {}), "v": ("VScaling", "VWeighting", {}),
            "edm": ("EDMScaling", "EDMWeighting", {"sigma_data": 0.5})}
DISCS = {"legacy": {"target": MOD + "discretizer.LegacyDDPMDiscretization"},
         "edm": {"target": MOD + "discretizer.EDMDiscretization", "params": {"sigma_min": 0.03, "sigma_max": 14.6}}}
GUIDERS = {"cfg": {"target": MOD + "guiders.VanillaCFG", "params": {"scale": 5.0}}, "identity": {"target": MOD + "guiders.IdentityGuider"}}
SAMPLERS = {"euler": ("EulerEDMSampler", dict(EDM)), "dpmpp2m": ("DPMPP2MSampler", {}), "heun": ("HeunEDMSampler", dict(EDM))}
EXTRA = {"euler_a": ("EulerAncestralSampler", {"eta": 1.0, "s_noise": 1.0}), "dpmpp2s_a": ("DPMPP2SAncestralSampler", {"eta": 1.0, "s_noise": 1.0}),
         "lms4": ("LinearMultistepSampler", {"order": 4}), "euler_churn": ("EulerEDMSampler", dict(EDM, s_churn=4.0))}
SEARCH_SEED = 77
SEARCH_SCORE_TOL = 3e-2                 # tests/test_engine_gpu.py: noise-search scores vs the oracle


def denoiser_config(discrete: bool, scaling: str, weighting: str = None) -> dict:
    sc, wt, params = SCALINGS[scaling]
    wcfg = {"target": MOD + "denoiser_weighting." + (weighting or wt)}
    scfg = {"target": MOD + "denoiser_scaling." + sc}
    if params:
        scfg["params"] = dict(params)
        if weighting is None:
            wcfg["params"] = dict(params)
    if discrete:
        return {"target": MOD + "denoiser.DiscreteDenoiser",
                "params": {"num_idx": 1000, "weighting_config": wcfg, "scaling_config": scfg, "discretization_config": DISCS["legacy"]}}
    return {"target": MOD + "denoiser.Denoiser", "params": {"weighting_config": wcfg, "scaling_config": scfg}}


def make_sampler(S, cls, steps, params, guider, disc):
    return getattr(S, cls)(num_steps=steps, discretization_config=DISCS[disc], guider_config=GUIDERS[guider], verbose=False,
                           device="cpu", **params)


def toy_net(pair: bool, seen: list):
    def net(x_in, c_noise, cond):
        seen.append(float(c_noise.reshape(-1)[0]))
        if pair:
            return MSG.toy_network(x_in, c_noise, cond)
        t = torch.sin(c_noise.to(x_in.dtype) / 100.0).reshape(-1, 1, 1, 1) * 0.05
        return torch.tanh(x_in + 0.25) + t                               # the conditional half of toy_network
    return net


def run_toy(S, proxy, cls, params, denoiser, guider, disc):
    """one toy run -> (trajectory, the c_noise of every evaluation)"""
    gens = [torch.Generator().manual_seed(s) for s in TOY_SEEDS]
    x0 = torch.cat([torch.randn((1, 4, TOY_HW, TOY_HW), generator=g) for g in gens], 0).double()
    seen = []
    toy = types.SimpleNamespace(denoiser=denoiser, model=toy_net(guider == "cfg", seen))
    sampler = make_sampler(S, cls, STEPS, params, guider, disc)
    if cls == "EulerEDMSampler":
        _, traj, _ = MCG.run(proxy, sampler, toy, x0, {}, {}, gens, {"name": ["toy"]})
    elif cls == "LinearMultistepSampler":                                 # (its first argument is a bare denoiser: make_lms_golden.py)
        inputs = []

        def bare(x, s, c):
            inputs.append(x[:x0.shape[0]].clone())                        # the first B rows are the latent under both guiders
            return denoiser(toy.model, x, s, c)
        with contextlib.redirect_stdout(io.StringIO()):
            z = sampler(bare, x0.clone(), cond={}, uc={})
        traj = torch.stack(inputs[1:] + [z], 0)
    else:
        _, traj = MSG.run(S, sampler, toy, x0, {}, {}, gens)
    return x0, traj, np.array(seen)


def engine_run(S, proxy, model, c, uc, batch, cls, params, guider, disc, seed):
    gen = torch.Generator().manual_seed(seed)
    x0 = torch.randn((1, 4, 32, 32), generator=gen)
    sampler = make_sampler(S, cls, 10, params, guider, disc)
    if cls == "EulerEDMSampler":
        z, traj, _ = MCG.run(proxy, sampler, model, x0, c, uc, [gen], batch)
    else:
        z, traj = MSG.run(S, sampler, model, x0, c, uc, [gen])
    return {"seed": np.array([seed]), "x0": x0.numpy(), "latent_rms": traj.pow(2).mean(dim=(1, 2, 3, 4)).sqrt().numpy(),
            "latent": z.numpy(), "decoded_sub": model.decode_first_stage(z)[:, :, ::8, ::8].numpy()}


def main():
    t0 = time.time()
    torch.set_grad_enabled(False)
    MG.import_reference()
    from sgm.util import instantiate_from_config
    import sgm.modules.diffusionmodules.sampling as S
    from sgm.modules.diffusionmodules.loss import StandardDiffusionLoss

    proxy = MCG.TorchProxy()
    S.torch = proxy
    # LinearMultistepSampler hands linear_multistep_coeff the schedule as an fp32 numpy array, whose node differences it then takes
    # in fp32; like the ``.double()`` denoisers, the float64 runs here give it the same values as float64
    coeff = S.linear_multistep_coeff
    S.linear_multistep_coeff = lambda order, t, i, j: coeff(order, np.asarray(t, dtype=np.float64), i, j)
    out = {"toy_seeds": np.array(TOY_SEEDS)}

    # ---------------------------------------------------------------- (a) toy network through the reference denoisers + guiders
    n = 0
    for dn, discrete in (("disc", True), ("cont", False)):
        for sc in SCALINGS:
            den = instantiate_from_config(denoiser_config(discrete, sc)).double()
            for gd in GUIDERS:
                for ds in DISCS:
                    for sm, (cls, params) in SAMPLERS.items():
                        case = f"{dn}_{sc}_{gd}_{ds}_{sm}"
                        x0, traj, seen = run_toy(S, proxy, cls, params, den, gd, ds)
                        assert bool(torch.isfinite(traj).all()), case
                        out["toy_x0"] = x0.numpy()
                        out[f"toy_{case}_traj"], out[f"toy_{case}_cnoise"] = traj.numpy(), seen
                        n += 1
    den = instantiate_from_config(denoiser_config(True, "v")).double()
    for sm, (cls, params) in EXTRA.items():
        case = f"disc_v_identity_legacy_{sm}"
        x0, traj, seen = run_toy(S, proxy, cls, params, den, "identity", "legacy")
        assert bool(torch.isfinite(traj).all()) and np.array_equal(x0.numpy(), out["toy_x0"]), case
        out[f"toy_{case}_traj"], out[f"toy_{case}_cnoise"] = traj.numpy(), seen
        n += 1
    print(f"[precond golden] {n} toy trajectories ({time.time() - t0:.1f}s)")

    # ---------------------------------------------------------------- the classes' own values (float64 inputs)
    import sgm.modules.diffusionmodules.denoiser_scaling as RS
    import sgm.modules.diffusionmodules.denoiser_weighting as RW
    from sgm.modules.diffusionmodules.discretizer import EDMDiscretization
    from sgm.modules.diffusionmodules.sigma_sampling import EDMSampling
    grid = torch.tensor([0.02, 0.3, 1.0, 2.5, 14.6, 80.0], dtype=torch.float64)
    out["cls_sigma_grid"] = grid.numpy()
    out["cls_edm_scaling"] = torch.stack(RS.EDMScaling()(grid), 0).numpy()
    out["cls_edm_scaling_sd1"] = torch.stack(RS.EDMScaling(sigma_data=1.0)(grid), 0).numpy()
    out["cls_v_scaling"] = torch.stack(RS.VScaling()(grid), 0).numpy()
    out["cls_edm_weighting"], out["cls_v_weighting"] = RW.EDMWeighting()(grid).numpy(), RW.VWeighting()(grid).numpy()
    out["cls_edm_disc_default_10"] = EDMDiscretization()(10).numpy()
    out["cls_edm_disc_20"] = EDMDiscretization(sigma_min=0.03, sigma_max=14.6)(20).numpy()
    out["cls_edm_disc_20_flip_nozero"] = EDMDiscretization(sigma_min=0.03, sigma_max=14.6)(20, do_append_zero=False, flip=True).numpy()
    rand = torch.randn((5,), generator=torch.Generator().manual_seed(31))
    out["cls_edm_sampling_rand"] = rand.numpy()
    out["cls_edm_sampling"] = EDMSampling()(5, rand=rand).numpy()
    out["cls_edm_sampling_p"] = EDMSampling(p_mean=-0.4, p_std=1.0)(5, rand=rand).numpy()
    torch.manual_seed(32)
    out["cls_edm_sampling_drawn"] = EDMSampling()(4).numpy()             # one torch.randn((4,)) of the default generator

    # ---------------------------------------------------------------- (c) the loss formula under autograd
    g = torch.Generator().manual_seed(21)
    B = 3
    z = torch.randn((B, 4, TOY_HW, TOY_HW), generator=g).double()
    noise = torch.randn((B, 4, TOY_HW, TOY_HW), generator=g).double()
    sigmas = torch.tensor([0.3, 2.5, 11.0], dtype=torch.float64)
    out["loss_z"], out["loss_noise"], out["loss_sigmas"] = z.numpy(), noise.numpy(), sigmas.numpy()
    loss_obj = types.SimpleNamespace(type="l2")
    for dn, discrete in (("disc", True), ("cont", False)):
        for name, sc, wt in (("eps", "eps", None), ("v", "v", None), ("edm", "edm", None), ("eps_unit", "eps", "UnitWeighting")):
            den = instantiate_from_config(denoiser_config(discrete, sc, wt)).double()
            seen, leaf = [], []
            net = toy_net(False, seen)

            def network(x_in, c_noise, cond):
                f = net(x_in, c_noise, cond).detach().requires_grad_(True)
                leaf.append(f)
                return f
            with torch.enable_grad():
                noised = z + noise * sigmas.reshape(-1, 1, 1, 1)
                w = den.w(sigmas).reshape(-1, 1, 1, 1)
                per_sample = StandardDiffusionLoss.get_diff_loss(loss_obj, den(network, noised, sigmas, {}), z, w)
                per_sample.mean().backward()
            out[f"loss_{dn}_{name}_f"] = leaf[0].detach().numpy()
            out[f"loss_{dn}_{name}_w"] = w.reshape(-1).numpy()
            out[f"loss_{dn}_{name}_per_sample"] = per_sample.detach().numpy()
            out[f"loss_{dn}_{name}_dF"] = leaf[0].grad.numpy()
    print(f"[precond golden] loss cases ({time.time() - t0:.1f}s)")

    # ---------------------------------------------------------------- (b) the engine on the G9 batch, denoiser swapped
    cfg = yaml.safe_load(open(os.path.join(MG.REF, "configs/test/textdesign_sd_2.yaml")))
    MG.strip_ckpt(cfg)
    model = instantiate_from_config(cfg["model"]).eval()
    torch.nn.Module.train(model.conditioner.embedders[0], False)      # (make_golden.py: the LabelEncoder dropout quirk)
    for name, p in model.state_dict().items():
        if not synth.is_computed_buffer(name):
            p.copy_(synth.synthetic_tensor(name, tuple(p.shape)))
    print(f"[precond golden] reference engine ready ({time.time() - t0:.1f}s)")
    batch256 = synth.synthetic_batch(1, 256, 256, 4, seed=0)
    torch.manual_seed(1234)
    buc = {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in batch256.items()}
    buc["label"] = ["" for _ in batch256["label"]]
    buc["txt"] = ["" for _ in batch256["txt"]]
    c, uc = model.conditioner.get_unconditional_conditioning(batch256, batch_uc=buc, force_uc_zero_embeddings=["label"])

    model.denoiser = instantiate_from_config(denoiser_config(True, "v"))
    for k, v in engine_run(S, proxy, model, c, uc, batch256, "EulerEDMSampler", dict(EDM), "cfg", "legacy", 506).items():
        out[f"v_cfg_euler_10_{k}"] = v
    print(f"[precond golden] v_cfg_euler_10 done ({time.time() - t0:.1f}s)")

    sampler = make_sampler(S, "EulerEDMSampler", 10, dict(EDM), "identity", "legacy")
    cfgs = types.SimpleNamespace(batch_size=1, channel=4, factor=8, gpu=0, noise_iters=2)
    torch.manual_seed(SEARCH_SEED)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        xs = sampler.get_init_noise(cfgs, model, cond=c, batch=batch256, uc=uc)
    line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("Init local loss")][0]
    best, worst = float(line.split("Best")[1].split("Worst")[0]), float(line.split("Worst")[1])
    gap = abs(worst - best) / max(abs(best), abs(worst))
    print(f"[precond golden] noise search: best {best:.6f} worst {worst:.6f} relative gap {gap:.3e} ({time.time() - t0:.1f}s)")
    if gap <= SEARCH_SCORE_TOL:
        print(f"[precond golden] MARGIN NOT MET: seed {SEARCH_SEED}: the candidates' scores are {gap:.2e} apart, inside the "
              f"{SEARCH_SCORE_TOL} score tolerance: the test pins the draw order and the two scores instead")
    out["v_identity_search_gap"], out["v_identity_search_seed"] = np.array([gap]), np.array([SEARCH_SEED])
    out["v_identity_search_x0"], out["v_identity_search_scores"] = xs.numpy(), np.array([best, worst])

    model.denoiser = instantiate_from_config(denoiser_config(False, "edm"))
    for k, v in engine_run(S, proxy, model, c, uc, batch256, "DPMPP2MSampler", {}, "identity", "edm", 507).items():
        out[f"edm_cont_identity_dpmpp2m_10_{k}"] = v
    print(f"[precond golden] edm_cont_identity_dpmpp2m_10 done ({time.time() - t0:.1f}s)")
    # two files, each under the 1 MiB limit of a committed file: the toy runs under DiscreteDenoiser, and everything else
    disc = {k: out.pop(k) for k in list(out) if k.startswith("toy_disc_")}
    disc["toy_seeds"], disc["toy_x0"] = out["toy_seeds"], out["toy_x0"]
    np.savez_compressed(os.path.join(HERE, "precond_golden_disc.npz"), **disc)
    np.savez_compressed(os.path.join(HERE, "precond_golden.npz"), **out)
    print(f"[precond golden] written ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
