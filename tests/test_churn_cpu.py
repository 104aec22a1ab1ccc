"""EulerEDMSampler with s_churn > 0 (the stochastic Karras "churn" step, reference sampling.py:89-137, 324-353), host side:

* the plans (``EulerEval(sigma_hat, sigma_next, churn=kn)``), applied through a plain-torch restatement of the two launches of a
  churned step (udt_unet_input_churn, udt_cfg_euler_step), reproduce the REAL reference's trajectories under the analytic toy
  network (tests/golden/churn_golden.npz, make_churn_golden.py): gamma 0.2, the sqrt(2) - 1 clamp, an s_tmin / s_tmax window,
  s_noise != 1, init_step > 0;
* the draw contract: one draw per CHURNED step from init_step on, in step order, per image under rng.per_image; nothing drawn
  and no generator advanced without churn;
* s_churn = 0 leaves the plans as they were; a churned last step still returns the denoised latent;
* the C ABI and pipeline.init_sampling carry the feature.
"""
import os
import re

import numpy as np
import pytest
import torch

import udifftext_amd  # noqa: F401  (puts the sgm mirror on sys.path)
from udifftext_amd import lib, pipeline, rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "churn_golden.npz")

S_MOD = "sgm.modules.diffusionmodules.sampling"
DISC = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
CFG5 = {"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 5.0}}
EDM = {"s_churn": 0.0, "s_tmin": 0.0, "s_tmax": 999.0, "s_noise": 1.0}

# tests/golden/make_churn_golden.py TOY_RUNS: case -> (steps, parameters, init_step)
TOY_RUNS = {
    "euler_churn_20": (20, dict(EDM, s_churn=4.0), 0),
    "euler_churn_50_clamped": (50, dict(EDM, s_churn=40.0), 0),
    "euler_churn_50_window": (50, dict(EDM, s_churn=10.0, s_tmin=0.5, s_tmax=8.0), 0),
    "euler_churn_20_snoise": (20, dict(EDM, s_churn=4.0, s_noise=0.7), 0),
    "euler_churn_20_init3": (20, dict(EDM, s_churn=4.0), 3),
}
# the gamma the issue expects of every churned step of the case
GAMMA = {"euler_churn_20": 0.2, "euler_churn_50_clamped": 2 ** 0.5 - 1, "euler_churn_50_window": 0.2, "euler_churn_20_snoise": 0.2,
         "euler_churn_20_init3": 0.2}


def _make(steps=10, cls="EulerEDMSampler", **params):
    from sgm.util import instantiate_from_config
    return instantiate_from_config({"target": f"{S_MOD}.{cls}", "params": dict(
        discretization_config=DISC, num_steps=steps, guider_config=CFG5, verbose=False, device="cpu", **dict(EDM, **params))})


@pytest.fixture(scope="module")
def cg():
    return np.load(GOLD)


def _churned(sampler, init_step=0):
    return [i for i, (e,) in sampler.plans(sampler._host_sigmas(), init_step) if e.churn != 0.0]


# ------------------------------------------------------------------------------------------ coefficient plans vs the reference
def _toy_eps(x_in, idx):
    """tests/golden/make_sampler_golden.py toy_network for one CFG pair (uncond, cond) at timestep index idx"""
    t = float(np.sin(idx / 100.0)) * 0.05
    return 0.8 * torch.tanh(x_in) + t, torch.tanh(x_in + 0.25) + t


def _run_plans_torch(sampler, x0, noise, init_step, table):
    """a churned Euler step restated in torch (float64 arithmetic, coefficients rounded to fp32 as the kernels receive them):
    udt_unet_input_churn x += churn*noise[slot]; then udt_cfg_euler_step at sigma_hat: den = CFG(x + c_out*eps_u, x + c_out*eps_c),
    c_in / c_out / timestep from the QUANTISED sigma_hat, d = (x - den)/sigma_hat, x += d*(sigma_next - sigma_hat) unquantised"""
    from sgm.modules.diffusionmodules.sampling import EulerEval, plan_noise_slots
    f32 = lambda v: float(np.float32(v))
    sig = sampler._host_sigmas()
    x = x0.clone() * (1.0 + sig[0] ** 2.0) ** 0.5
    plans = sampler.plans(sig, init_step)
    slots = plan_noise_slots(plans)
    traj = []
    for i, plan in plans:
        (e,) = plan
        assert isinstance(e, EulerEval) and e.src == "x"
        if e.churn != 0.0:
            x = x + f32(e.churn) * noise[slots[i]]
        idx = int((table - e.sigma).abs().argmin())
        sq = float(table[idx])
        eu, ec = _toy_eps(x * (1.0 / (sq * sq + 1.0) ** 0.5), idx)
        du, dc = x + f32(-sq) * eu, x + f32(-sq) * ec
        den = du + f32(sampler.guider.scale) * (dc - du)
        x = x + (x - den) / f32(e.sigma) * (f32(e.sigma_next) - f32(e.sigma))
        traj.append(x.clone())
    return torch.stack(traj, 0)


@pytest.mark.parametrize("case", list(TOY_RUNS))
def test_plans_reproduce_reference_toy_trajectories(cg, case):
    from sgm.modules.diffusionmodules.discretizer import LegacyDDPMDiscretization
    steps, params, init_step = TOY_RUNS[case]
    sampler = _make(steps, **params)
    table = LegacyDDPMDiscretization()(1000, do_append_zero=False, flip=True).float()
    seeds = [int(s) for s in cg["toy_seeds"]]
    x0_ref, traj_ref = torch.from_numpy(cg[f"toy_{case}_x0"]), torch.from_numpy(cg[f"toy_{case}_traj"])
    churned_ref = [int(i) for i in cg[f"toy_{case}_churned"]]
    # the steps the REFERENCE churned, and its gamma there, are the ones the plans churn
    assert _churned(sampler, init_step) == churned_ref
    np.testing.assert_allclose(cg[f"toy_{case}_gamma"][[i - init_step for i in churned_ref]], GAMMA[case], rtol=1e-12)
    sig = sampler._host_sigmas()
    for i, (e,) in sampler.plans(sig, init_step):
        g = GAMMA[case] if i in churned_ref else 0.0
        assert e.sigma == pytest.approx(sig[i] * (1.0 + g), rel=1e-15) and e.sigma_next == sig[i + 1]
        assert e.churn == pytest.approx(params["s_noise"] * ((sig[i] * (1.0 + g)) ** 2 - sig[i] ** 2) ** 0.5, rel=1e-12)
    with rng.per_image(seeds):
        x0 = rng.randn(x0_ref.shape)
        noise = sampler.draw_step_noise(x0.shape, "cpu", None, init_step)
    assert torch.equal(x0.double(), x0_ref)                          # the reference's first draw of every generator
    assert noise.shape == (len(churned_ref),) + tuple(x0.shape)
    traj = _run_plans_torch(sampler, x0.double(), noise.double(), init_step, table)
    assert traj.shape == traj_ref.shape
    for k in range(traj.shape[0]):
        err = (traj[k] - traj_ref[k]).abs().max().item() / traj_ref[k].abs().max().item()
        assert err <= 1e-6, f"{case}: step {k + init_step}: relative error {err:.2e}"


def test_window_case_churns_a_middle_stretch_only(cg):
    steps, params, _ = TOY_RUNS["euler_churn_50_window"]
    churned = [int(i) for i in cg["toy_euler_churn_50_window_churned"]]
    assert 0 < churned[0] and churned[-1] < steps - 1 and churned == list(range(churned[0], churned[-1] + 1))
    sig = _make(steps, **params)._host_sigmas()
    assert all((0.5 <= sig[i] <= 8.0) == (i in churned) for i in range(steps))


# ------------------------------------------------------------------------------------------------------- draw contract
def test_churn_draw_count_and_order():
    shape = (3, 4, 5, 6)
    s = _make(7, s_churn=1.4)                                         # gamma 0.2 on all 7 steps
    assert _churned(s) == list(range(7))
    torch.manual_seed(21)
    got = s.draw_step_noise(shape, "cpu")
    torch.manual_seed(21)
    want = torch.stack([rng.randn(shape) for _ in range(7)], 0)       # one [B,4,h,w] draw per churned step, in step order
    assert got.shape == (7,) + shape and torch.equal(got, want)
    torch.manual_seed(21)
    assert torch.equal(s.draw_step_noise(shape, "cpu", None, 2), want[:5])      # init_step drops the earlier steps' draws
    # behind the initial-noise draw (predict: get_init_noise, then the sampler), the steps take the generator's next draws
    with rng.per_image([5]):
        alone = s.draw_step_noise((1,) + shape[1:], "cpu")
    with rng.per_image([5]):
        rng.randn((1,) + shape[1:])
        after = s.draw_step_noise((1,) + shape[1:], "cpu")
    assert torch.equal(after[:-1], alone[1:])


def test_window_draws_one_tensor_per_churned_step():
    shape = (2, 4, 4, 4)
    steps, params, _ = TOY_RUNS["euler_churn_50_window"]
    s = _make(steps, **params)
    churned = _churned(s)
    assert 0 < len(churned) < steps
    torch.manual_seed(8)
    got = s.draw_step_noise(shape, "cpu")
    after = torch.randn(4)
    torch.manual_seed(8)
    want = torch.stack([rng.randn(shape) for _ in churned], 0)
    assert torch.equal(got, want) and torch.equal(after, torch.randn(4))       # exactly len(churned) draws, no more
    # init_step inside the window: only the churned steps from init_step on draw, and the k-th of THEM reads slot k
    from sgm.modules.diffusionmodules.sampling import plan_noise_slots
    init = churned[2]
    torch.manual_seed(8)
    late = s.draw_step_noise(shape, "cpu", None, init)
    assert torch.equal(late, want[:len(churned) - 2])
    assert plan_noise_slots(s.plans(s._host_sigmas(), init)) == {i: k for k, i in enumerate(churned[2:])}
    # init_step behind the window: nothing left to draw
    torch.manual_seed(8)
    assert s.draw_step_noise(shape, "cpu", None, churned[-1] + 1) is None
    assert torch.equal(torch.randn(shape), want[0])


def test_churn_draws_are_per_image():
    shape = (3, 4, 5, 6)
    s = _make(6, s_churn=1.2)
    with rng.per_image([4, 5, 6]):
        batched = s.draw_step_noise(shape, "cpu")
    with rng.per_image([5]):
        alone = s.draw_step_noise((1,) + shape[1:], "cpu")
    assert torch.equal(batched[:, 1:2], alone)                       # image 1 of 3 == a batch-1 run with its own seed


def test_no_churn_draws_nothing():
    for params in ({}, {"s_churn": 0.0, "s_noise": 0.5}, {"s_churn": 3.0, "s_tmin": 500.0}):      # (no sigma reaches s_tmin = 500)
        s = _make(5, **params)
        torch.manual_seed(3)
        assert s.draw_step_noise((1, 4, 8, 8), "cpu") is None
        nxt = torch.randn(4)
        torch.manual_seed(3)
        assert torch.equal(nxt, torch.randn(4))                    # the generator did not advance


# ------------------------------------------------------------------------------------------------------------- plans
def test_plans_without_churn_are_unchanged():
    from sgm.modules.diffusionmodules.sampling import EulerEval, Eval, plan_noise_slots, plans_add_noise
    for init in (0, 3):
        s = _make(10)
        sig = s._host_sigmas()
        today = [(i, (EulerEval(sig[i], sig[i + 1]),)) for i in range(init, 10)]
        assert s.plans(sig, init) == today and tuple(s.plans(sig, init)) == tuple(today)
        assert hash(tuple(s.plans(sig, init))) == hash(tuple(today))                  # the graph runners' cache key
        assert not plans_add_noise(today) and plan_noise_slots(today) == {}
    assert EulerEval(2.0, 1.0) == EulerEval(2.0, 1.0, "x", 0.0) and EulerEval(2.0, 1.0).churn == 0.0
    assert Eval(2.0, "x", "x").churn == 0.0
    assert EulerEval(2.0, 1.0, churn=0.3) != EulerEval(2.0, 1.0)                      # a churned run never shares a runner
    # s_tmin / s_tmax / s_noise alone change nothing
    s = _make(10, s_tmin=1.0, s_tmax=5.0, s_noise=0.3)
    assert s.plans(s._host_sigmas()) == [(i, (EulerEval(sig[i], sig[i + 1]),)) for i in range(10)]


def test_noise_slots_of_ancestral_plans_stay_one_per_step():
    from sgm.modules.diffusionmodules.sampling import plan_noise_slots
    s = pipeline.init_sampling(6, 5.0, "cpu", sampler="euler_a")
    plans = s.plans(s._host_sigmas(), 2)
    assert plan_noise_slots(plans) == {2: 0, 3: 1, 4: 2, 5: 3}                        # the last step (kn = 0) included


def test_churned_last_step_returns_the_denoised_latent():
    """sigma_next = 0: x + (x - den)/sigma_hat * (0 - sigma_hat) = den, from the churned x at sigma_hat"""
    s = _make(10, s_churn=2.0)
    sig = s._host_sigmas()
    (e,) = s.step_plan(sig, 9)
    assert e.sigma_next == 0.0 and e.churn > 0.0 and e.sigma == pytest.approx(sig[9] * 1.2)
    from sgm.modules.diffusionmodules.discretizer import LegacyDDPMDiscretization
    table = LegacyDDPMDiscretization()(1000, do_append_zero=False, flip=True).float()
    g = torch.Generator().manual_seed(1)
    x = torch.randn((1, 4, 4, 4), generator=g).double() * sig[9]
    nz = torch.randn((1, 4, 4, 4), generator=g).double()
    xh = x + float(np.float32(e.churn)) * nz
    idx = int((table - e.sigma).abs().argmin())
    sq = float(table[idx])
    eu, ec = _toy_eps(xh * (1.0 / (sq * sq + 1.0) ** 0.5), idx)
    du, dc = xh - float(np.float32(sq)) * eu, xh - float(np.float32(sq)) * ec
    den = du + 5.0 * (dc - du)
    out = xh + (xh - den) / float(np.float32(e.sigma)) * (0.0 - float(np.float32(e.sigma)))
    assert (out - den).abs().max().item() <= 1e-12 * den.abs().max().item()


def test_gamma_uses_the_schedules_step_count():
    """n = num_sigmas - 1, not reduced by init_step; the 2-step schedule of the noise search has n = 2"""
    s = _make(20, s_churn=4.0)
    sig = s._host_sigmas()
    assert s.churn_gamma(sig, 0) == pytest.approx(0.2) and s.step_plan(sig, 5, init_step=5) == s.step_plan(sig, 5)
    sig2 = s._host_sigmas(2)
    assert s.churn_gamma(sig2, 0) == 2 ** 0.5 - 1                                     # min(4 / 2, sqrt(2) - 1)
    s = _make(20, s_churn=0.5)
    assert s.churn_gamma(s._host_sigmas(2), 1) == 0.25
    assert [len(p) for _, p in s._search_plans(s._host_sigmas(2))] == [1, 1]
    assert all(e.churn > 0 for _, (e,) in s._search_plans(s._host_sigmas(2)))


# ------------------------------------------------------------------------------------------------------------ surface
def test_header_and_symbol_table_hold_the_new_entry_point():
    header = open(os.path.join(ROOT, "include", "udt_kernels.h")).read()
    m = re.search(r"int\s+udt_unet_input_churn\s*\(([^;]*)\)\s*;", header)
    assert m, "include/udt_kernels.h does not declare udt_unet_input_churn"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    restype, argtypes = lib.SYMBOLS["udt_unet_input_churn"]
    assert n_args == len(argtypes) == 9
    assert re.search(r"int\s+udt_unet_input\s*\(const float\* x, void\* xin, int32_t B, int32_t hw, int32_t cpad, float c_in, "
                     r"void\* stream\);", header), "udt_unet_input keeps its signature"
    from udifftext_amd import ops
    assert callable(ops.unet_input_churn)


def test_init_sampling_forwards_the_churn_settings():
    from sgm.modules.diffusionmodules.sampling import EulerEDMSampler, HeunEDMSampler
    s = pipeline.init_sampling(10, 5.0, "cpu", s_churn=2)
    assert type(s) is EulerEDMSampler and (s.s_churn, s.s_tmin, s.s_tmax, s.s_noise) == (2, 0.0, 999.0, 1.0)
    s = pipeline.init_sampling(10, 5.0, "cpu", sampler="euler", s_churn=1.5, s_tmin=0.2, s_tmax=9.0, s_noise=0.9)
    assert (s.s_churn, s.s_tmin, s.s_tmax, s.s_noise) == (1.5, 0.2, 9.0, 0.9)
    s._check_fast_path()                                                              # Euler runs churn ...
    h = pipeline.init_sampling(10, 5.0, "cpu", sampler="heun", s_churn=1.5)
    assert type(h) is HeunEDMSampler and h.s_churn == 1.5
    with pytest.raises(NotImplementedError, match="s_churn"):                         # ... Heun still refuses it
        h._check_fast_path()
    d = pipeline.init_sampling(10, 5.0, "cpu")
    assert (d.s_churn, d.s_tmin, d.s_tmax, d.s_noise) == (0.0, 0.0, 999.0, 1.0)
    pipeline.init_sampling(10, 5.0, "cpu", sampler="euler_a", s_churn=0.0)            # ignored where it does not apply
