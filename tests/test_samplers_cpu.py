"""The sampler family beyond Euler (HeunEDMSampler, EulerAncestralSampler, DPMPP2SAncestralSampler, DPMPP2MSampler), host side:

* every reference ``target:`` string instantiates with the reference's constructor parameters;
* the host coefficient plans, applied through a plain-torch restatement of the fused step's formula (udt_cfg_sampler_step),
  reproduce the REAL reference samplers' trajectories under an analytic toy network (tests/golden/sampler_golden.npz,
  make_sampler_golden.py) — 20- and 50-step schedules, the last step, eta = 0, init_step > 0;
* the ancestral noise contract: one draw per step (the last one included), step-major, per image under rng.per_image;
* what the fused path does not implement raises NotImplementedError.
"""
import os

import numpy as np
import pytest
import torch

import udifftext_amd  # noqa: F401  (puts the sgm mirror on sys.path)
from udifftext_amd import pipeline, rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "sampler_golden.npz")

S_MOD = "sgm.modules.diffusionmodules.sampling"
DISC = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
CFG5 = {"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 5.0}}
EDM = {"s_churn": 0.0, "s_tmin": 0.0, "s_tmax": 999.0, "s_noise": 1.0}

# (class, params) with the reference's constructor parameters
CLASSES = {
    "HeunEDMSampler": EDM,
    "EulerAncestralSampler": {"eta": 1.0, "s_noise": 1.0},
    "DPMPP2SAncestralSampler": {"eta": 1.0, "s_noise": 1.0},
    "DPMPP2MSampler": {},
}
# tests/golden/make_sampler_golden.py TOY_RUNS
TOY_RUNS = {}
for _n in (20, 50):
    TOY_RUNS[f"dpmpp2m_{_n}"] = ("DPMPP2MSampler", _n, {}, 0)
    TOY_RUNS[f"euler_a_{_n}"] = ("EulerAncestralSampler", _n, {"eta": 1.0, "s_noise": 1.0}, 0)
    TOY_RUNS[f"heun_{_n}"] = ("HeunEDMSampler", _n, EDM, 0)
    TOY_RUNS[f"dpmpp2s_a_{_n}"] = ("DPMPP2SAncestralSampler", _n, {"eta": 1.0, "s_noise": 1.0}, 0)
TOY_RUNS["dpmpp2m_20_init3"] = ("DPMPP2MSampler", 20, {}, 3)
TOY_RUNS["euler_a_20_eta0"] = ("EulerAncestralSampler", 20, {"eta": 0.0, "s_noise": 1.0}, 0)
TOY_RUNS["euler_a_20_eta05"] = ("EulerAncestralSampler", 20, {"eta": 0.5, "s_noise": 0.7}, 0)
TOY_RUNS["dpmpp2s_a_20_eta0"] = ("DPMPP2SAncestralSampler", 20, {"eta": 0.0, "s_noise": 1.0}, 0)


def _make(cls, steps=10, guider=CFG5, **params):
    from sgm.util import instantiate_from_config
    return instantiate_from_config({"target": f"{S_MOD}.{cls}", "params": dict(
        discretization_config=DISC, num_steps=steps, guider_config=guider, verbose=False, device="cpu", **params)})


@pytest.fixture(scope="module")
def sg():
    return np.load(GOLD)


@pytest.mark.parametrize("cls", list(CLASSES) + ["EulerEDMSampler"])
def test_reference_targets_instantiate(cls):
    from sgm.modules.diffusionmodules.guiders import VanillaCFG
    params = CLASSES.get(cls, EDM)
    s = _make(cls, 20, **params)
    assert type(s).__name__ == cls and s.num_steps == 20 and isinstance(s.guider, VanillaCFG)
    for k, v in params.items():
        assert getattr(s, k) == v
    assert callable(s.get_init_noise) and callable(s.sample_lane) and callable(s.sample_in_flight)


@pytest.mark.parametrize("name,cls", list(pipeline.SAMPLERS.items()))
def test_init_sampling_selects_the_sampler(name, cls):
    s = pipeline.init_sampling(20, 5.0, "cpu", sampler=name)
    assert type(s).__name__ == cls and s.guider.scale == 5.0 and s.num_steps == 20
    if cls == "EulerEDMSampler":
        assert (s.s_churn, s.s_tmin, s.s_tmax, s.s_noise) == (0.0, 0.0, 999.0, 1.0)
    with pytest.raises(ValueError):
        pipeline.init_sampling(20, 5.0, "cpu", sampler="lms")


def test_init_sampling_default_is_euler():
    from sgm.modules.diffusionmodules.sampling import EulerEDMSampler
    assert type(pipeline.init_sampling(10, 5.0, "cpu")) is EulerEDMSampler


# ------------------------------------------------------------------------------------------ coefficient plans vs the reference
def _toy_eps(x_in, idx):
    """tests/golden/make_sampler_golden.py toy_network for one CFG pair (uncond, cond) at timestep index idx"""
    t = float(np.sin(idx / 100.0)) * 0.05
    return 0.8 * torch.tanh(x_in) + t, torch.tanh(x_in + 0.25) + t


def _run_plans_torch(sampler, x0, noise, init_step, table):
    """the fused step restated in torch (float64 arithmetic, coefficients rounded to fp32 as the kernel receives them):
    per evaluation den = CFG(src + c_out*eps_u, src + c_out*eps_c); out = kx*src + kd*den + ka*aux + kp*prev + kn*noise"""
    f32 = lambda v: float(np.float32(v))
    sig = sampler._host_sigmas()
    x = x0.clone() * (1.0 + sig[0] ** 2.0) ** 0.5
    bufs = {"x": x, "t": torch.zeros_like(x), "h0": torch.zeros_like(x), "h1": torch.zeros_like(x)}
    traj = []
    for i, plan in sampler.plans(sig, init_step):
        for e in plan:
            src = bufs[e.src]
            idx = int((table - e.sigma).abs().argmin())
            sq = float(table[idx])
            eu, ec = _toy_eps(src * (1.0 / (sq * sq + 1.0) ** 0.5), idx)
            du, dc = src + f32(-sq) * eu, src + f32(-sq) * ec
            den = du + f32(sampler.guider.scale) * (dc - du)
            out = f32(e.kx) * src + f32(e.kd) * den
            if e.aux:
                out = out + f32(e.ka) * bufs[e.aux]
            if e.prev:
                out = out + f32(e.kp) * bufs[e.prev]
            if e.kn != 0.0:
                out = out + f32(e.kn) * noise[i - init_step]
            if e.den_out:
                bufs[e.den_out] = den
            bufs[e.out] = out
        traj.append(bufs["x"].clone())
    return torch.stack(traj, 0)


@pytest.mark.parametrize("case", list(TOY_RUNS))
def test_plans_reproduce_reference_toy_trajectories(sg, case):
    from sgm.modules.diffusionmodules.discretizer import LegacyDDPMDiscretization
    cls, steps, params, init_step = TOY_RUNS[case]
    sampler = _make(cls, steps, **params)
    table = LegacyDDPMDiscretization()(1000, do_append_zero=False, flip=True).float()
    seeds = [int(s) for s in sg["toy_seeds"]]
    x0_ref, traj_ref = torch.from_numpy(sg[f"toy_{case}_x0"]), torch.from_numpy(sg[f"toy_{case}_traj"])
    with rng.per_image(seeds):
        x0 = rng.randn(x0_ref.shape)
        noise = sampler.draw_step_noise(x0.shape, "cpu", None, init_step)
    assert torch.equal(x0.double(), x0_ref)                          # the reference's first draw of every generator
    assert (noise is not None) == (cls in ("EulerAncestralSampler", "DPMPP2SAncestralSampler"))
    traj = _run_plans_torch(sampler, x0.double(), noise.double() if noise is not None else None, init_step, table)
    assert traj.shape == traj_ref.shape
    for k in range(traj.shape[0]):
        err = (traj[k] - traj_ref[k]).abs().max().item() / traj_ref[k].abs().max().item()
        assert err <= 1e-6, f"{case}: step {k + init_step}: relative error {err:.2e}"


def test_unet_evaluations_per_sampler():
    """UNet evaluations per run: Heun 2 per step but 1 on the last, DPM++ 2S-a 2 per step but 1 where sigma_down = 0 (the last
    step with eta > 0), Euler-a and DPM++ 2M one per step"""
    def evals(cls, n, **p):
        s = _make(cls, n, **p)
        return sum(len(plan) for _, plan in s.plans(s._host_sigmas()))
    assert evals("HeunEDMSampler", 10, **EDM) == 19
    assert evals("DPMPP2SAncestralSampler", 10, eta=1.0, s_noise=1.0) == 19
    assert evals("DPMPP2SAncestralSampler", 10, eta=0.0, s_noise=1.0) == 19
    assert evals("EulerAncestralSampler", 20, eta=1.0, s_noise=1.0) == 20
    assert evals("DPMPP2MSampler", 20) == 20


def test_last_step_returns_the_denoised_latent():
    """sigma_next = 0: every sampler's last evaluation is x = den exactly (kx = 0, kd = 1), no noise, no history term"""
    for cls, p in CLASSES.items():
        s = _make(cls, 10, **p)
        sig = s._host_sigmas()
        plan = s.step_plan(sig, len(sig) - 2)
        e = plan[-1]
        assert len(plan) == 1 and e.kx == 0.0 and e.kd == 1.0 and e.kn == 0.0 and e.aux is None and e.prev is None, (cls, plan)
        assert all(np.isfinite(v) for v in (e.kx, e.kd, e.ka, e.kp, e.kn))


# ------------------------------------------------------------------------------------------------------ noise contract
@pytest.mark.parametrize("cls", ["EulerAncestralSampler", "DPMPP2SAncestralSampler"])
def test_ancestral_draw_order(cls):
    s = _make(cls, 7, eta=1.0, s_noise=1.0)
    shape = (3, 4, 5, 6)
    torch.manual_seed(21)
    got = s.draw_step_noise(shape, "cpu")
    torch.manual_seed(21)
    want = torch.stack([rng.randn(shape) for _ in range(7)], 0)       # one [B,4,h,w] draw per step, the last step included
    assert got.shape == (7,) + shape and torch.equal(got, want)
    torch.manual_seed(21)
    assert torch.equal(s.draw_step_noise(shape, "cpu", None, 2), want[:5])      # init_step: the loop's steps only
    # per image: image 1 of a batch of 3 sees the draws of a batch-1 run with its own seed
    with rng.per_image([4, 5, 6]):
        batched = s.draw_step_noise(shape, "cpu")
    with rng.per_image([5]):
        alone = s.draw_step_noise((1,) + shape[1:], "cpu")
    assert torch.equal(batched[:, 1:2], alone)
    # behind the initial-noise draw (predict: get_init_noise, then the sampler), the steps take the generator's next draws
    with rng.per_image([5]):
        rng.randn((1,) + shape[1:])
        after = s.draw_step_noise((1,) + shape[1:], "cpu")
    assert torch.equal(after[:-1], alone[1:])


def test_deterministic_samplers_draw_nothing():
    for cls in ("HeunEDMSampler", "DPMPP2MSampler"):
        s = _make(cls, 5, **CLASSES[cls])
        torch.manual_seed(3)
        assert s.draw_step_noise((1, 4, 8, 8), "cpu") is None
        nxt = torch.randn(4)
        torch.manual_seed(3)
        assert torch.equal(nxt, torch.randn(4))                    # the generator did not advance


# --------------------------------------------------------------------------------------------------- unsupported options
@pytest.mark.parametrize("cls", list(CLASSES))
def test_unsupported_options_raise(cls):
    x = torch.zeros((1, 4, 8, 8))
    s = _make(cls, 5, **CLASSES[cls])
    with pytest.raises(NotImplementedError, match="attend-and-excite"):
        s(None, x, {}, {}, aae_enabled=True)
    with pytest.raises(NotImplementedError, match="detailed"):
        s(None, x, {}, {}, detailed=True)
    s = _make(cls, 5, guider={"target": "sgm.modules.diffusionmodules.guiders.IdentityGuider"}, **CLASSES[cls])
    with pytest.raises(NotImplementedError, match="VanillaCFG"):
        s(None, x, {}, {})
    with pytest.raises(NotImplementedError, match="VanillaCFG"):
        s.sample_lane(None, x, {}, {}, slot=0, n_lanes=2)


def test_heun_churn_raises():
    s = _make("HeunEDMSampler", 5, **dict(EDM, s_churn=0.5))
    with pytest.raises(NotImplementedError, match="s_churn"):
        s(None, torch.zeros((1, 4, 8, 8)), {}, {})
