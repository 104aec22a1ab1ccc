"""LinearMultistepSampler, host side:

* the reference ``target:`` string instantiates with ``order``, and ``init_sampling(sampler="linear_multistep")`` builds it;
* the closed-form float64 coefficients equal the reference's own ``linear_multistep_coeff`` (tests/golden/lms_golden.npz,
  make_lms_golden.py) to 1e-10 relative;
* the plans, applied through a plain-torch restatement of the fused step (udt_cfg_multistep_step), reproduce the REAL reference
  sampler's trajectories under make_sampler_golden.py's toy network — orders 1-4, 20 and 50 steps, init_step > 0;
* the derivative ring: one evaluation per step, and no slot written while it still holds a live history term;
* what the fused path does not implement raises NotImplementedError.
"""
import os

import numpy as np
import pytest
import torch

import udifftext_amd  # noqa: F401  (puts the sgm mirror on sys.path)
from udifftext_amd import pipeline, rng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "lms_golden.npz")

TARGET = "sgm.modules.diffusionmodules.sampling.LinearMultistepSampler"
DISC = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
CFG5 = {"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 5.0}}
# tests/golden/make_lms_golden.py TOY_RUNS: case -> (order, steps, init_step)
TOY_RUNS = {f"lms_o{o}_20": (o, 20, 0) for o in (1, 2, 3, 4)}
TOY_RUNS["lms_o4_50"] = (4, 50, 0)
TOY_RUNS["lms_o4_20_init3"] = (4, 20, 3)


def _make(steps=20, guider=CFG5, **params):
    from sgm.util import instantiate_from_config
    return instantiate_from_config({"target": TARGET, "params": dict(
        discretization_config=DISC, num_steps=steps, guider_config=guider, verbose=False, device="cpu", **params)})


@pytest.fixture(scope="module")
def lg():
    return np.load(GOLD)


def test_reference_target_instantiates():
    from sgm.modules.diffusionmodules.guiders import VanillaCFG
    s = _make(20, order=3)
    assert type(s).__name__ == "LinearMultistepSampler" and s.order == 3 and s.num_steps == 20
    assert isinstance(s.guider, VanillaCFG) and s.guider.scale == 5.0
    assert _make(20).order == 4                                      # the reference's default
    assert callable(s.get_init_noise) and callable(s.sample_lane) and callable(s.sample_in_flight)


def test_init_sampling_builds_it():
    s = pipeline.init_sampling(20, 5.0, "cpu", sampler="linear_multistep")
    assert type(s).__name__ == "LinearMultistepSampler" and s.order == 4 and s.num_steps == 20 and s.guider.scale == 5.0


def test_draws_no_noise():
    s = _make(5)
    torch.manual_seed(3)
    assert s.draw_step_noise((1, 4, 8, 8), "cpu") is None
    nxt = torch.randn(4)
    torch.manual_seed(3)
    assert torch.equal(nxt, torch.randn(4))                          # the generator did not advance


# -------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("steps", [20, 50])
def test_coefficients_match_the_reference(lg, steps):
    from sgm.modules.diffusionmodules.sampling import linear_multistep_coeff
    t = lg[f"coef_{steps}_sigmas"]
    assert t.dtype == np.float32                                     # the reference's fp32 schedule ...
    mine = np.array(_make(steps)._host_sigmas())
    assert np.abs(mine - t).max() <= 1e-6 * t.max()                  # ... which this package's matches (to the CPU's last ulp)
    sig = [float(v) for v in t]
    for order in (1, 2, 3, 4):
        ref = lg[f"coef_{steps}_o{order}"]
        for i in range(steps):
            for j in range(order):
                if i < order - 1:
                    assert np.isnan(ref[i, j])
                    with pytest.raises(ValueError):
                        linear_multistep_coeff(order, sig, i, j)
                    continue
                got = linear_multistep_coeff(order, sig, i, j)
                assert abs(got - ref[i, j]) <= 1e-10 * abs(ref[i, j]), (steps, order, i, j, got, ref[i, j])


@pytest.mark.parametrize("order", [1, 2, 4, 8])
def test_coefficients_sum_to_the_step(order):
    """the Lagrange basis sums to 1, so a step's coefficients integrate 1 over [t_i, t_i+1]: sum k = sigma_next - sigma"""
    s = _make(30, order=order)
    sig = s._host_sigmas()
    for i, (e,) in s.plans(sig):
        total = e.k0 + sum(k for _, k in e.hist)
        assert abs(total - (sig[i + 1] - sig[i])) <= 1e-9 * sig[i], (order, i, total)


# -------------------------------------------------------------------------------------------------- plans vs the reference
def _toy_eps(x_in, idx):
    """tests/golden/make_sampler_golden.py toy_network for one CFG pair (uncond, cond) at timestep index idx"""
    t = float(np.sin(idx / 100.0)) * 0.05
    return 0.8 * torch.tanh(x_in) + t, torch.tanh(x_in + 0.25) + t


def _run_plans_torch(sampler, x0, init_step, table):
    """the fused step restated in torch (float64 arithmetic, scalars rounded to fp32 as the kernel receives them):
    den = CFG(src + c_out*eps_u, src + c_out*eps_c); d = (src - den)/sigma; out = src + (k0*d + k1*hist1 + ...); d_out = d"""
    f32 = lambda v: float(np.float32(v))
    sig = sampler._host_sigmas()
    x = x0.clone() * (1.0 + sig[0] ** 2.0) ** 0.5
    bufs = {"x": x}
    traj = []
    for i, plan in sampler.plans(sig, init_step):
        for e in plan:
            src = bufs[e.src]
            idx = int((table - e.sigma).abs().argmin())
            sq = float(table[idx])
            eu, ec = _toy_eps(src * (1.0 / (sq * sq + 1.0) ** 0.5), idx)
            du, dc = src + f32(-sq) * eu, src + f32(-sq) * ec
            den = du + f32(sampler.guider.scale) * (dc - du)
            d = (src - den) / f32(e.sigma)
            acc = f32(e.k0) * d
            for b, k in e.hist:
                acc = acc + f32(k) * bufs[b]
            bufs[e.d_out] = d
            bufs[e.out] = src + acc
        traj.append(bufs["x"].clone())
    return torch.stack(traj, 0)


@pytest.mark.parametrize("case", list(TOY_RUNS))
def test_plans_reproduce_reference_toy_trajectories(lg, case):
    from sgm.modules.diffusionmodules.discretizer import LegacyDDPMDiscretization
    order, steps, init_step = TOY_RUNS[case]
    sampler = _make(steps, order=order)
    table = LegacyDDPMDiscretization()(1000, do_append_zero=False, flip=True).float()
    seeds = [int(s) for s in lg["toy_seeds"]]
    x0_ref, traj_ref = torch.from_numpy(lg[f"toy_{case}_x0"]), torch.from_numpy(lg[f"toy_{case}_traj"])
    with rng.per_image(seeds):
        x0 = rng.randn(x0_ref.shape)
    assert torch.equal(x0.double(), x0_ref)
    traj = _run_plans_torch(sampler, x0.double(), init_step, table)
    assert traj.shape == traj_ref.shape
    for k in range(traj.shape[0]):
        err = (traj[k] - traj_ref[k]).abs().max().item() / traj_ref[k].abs().max().item()
        assert err <= 1e-6, f"{case}: step {k + init_step}: relative error {err:.2e}"


# ------------------------------------------------------------------------------------------------------ the ring
@pytest.mark.parametrize("order,steps,init_step", [(1, 10, 0), (2, 10, 0), (4, 20, 0), (4, 20, 3), (4, 50, 0), (8, 20, 0),
                                                   (8, 20, 5)])
def test_plans_keep_the_history_ring_live(order, steps, init_step):
    """one evaluation per step; step i writes d{i % order} and reads the derivatives of steps i-1, i-2, ... (newest first) —
    slots that no later write has overwritten, distinct from the slot it writes"""
    from sgm.modules.diffusionmodules.sampling import MultistepEval, plan_buffers
    s = _make(steps, order=order)
    sig = s._host_sigmas()
    plans = s.plans(sig, init_step)
    assert [i for i, _ in plans] == list(range(init_step, steps))
    assert sorted(plan_buffers(plans)) == sorted(f"d{m}" for m in range(min(order, steps - init_step)))
    holder = {}                                                       # slot -> step whose derivative it holds
    for i, plan in plans:
        assert len(plan) == 1
        (e,) = plan
        assert isinstance(e, MultistepEval) and e.src == "x" and e.out == "x" and e.sigma == sig[i]
        cur = min(i - init_step + 1, order)
        assert len(e.hist) == cur - 1
        slots = [b for b, _ in e.hist]
        assert e.d_out not in slots and len(set(slots)) == len(slots)
        assert [holder[b] for b in slots] == [i - j for j in range(1, cur)]
        holder[e.d_out] = i


def test_last_step_is_the_plain_multistep_sum():
    """sigma_next = 0 needs no special case (unlike DPM++ 2M's x = den): the last step returns exactly x + sum k*d with the
    reference's order-4 weights, summed in the reference's order"""
    from sgm.modules.diffusionmodules.sampling import linear_multistep_coeff
    s = _make(20)
    sig = s._host_sigmas()
    assert sig[-1] == 0.0
    (e,) = s.step_plan(sig, 19)
    ks = [e.k0] + [k for _, k in e.hist]
    assert ks == [linear_multistep_coeff(4, sig, 19, j) for j in range(4)]
    assert [b for b, _ in e.hist] == ["d2", "d1", "d0"]
    g = torch.Generator().manual_seed(0)
    x, d, h1, h2, h3 = (torch.randn((2, 4, 8, 8), generator=g, dtype=torch.float64) for _ in range(5))
    want = x + sum(k * t for k, t in zip(ks, (d, h1, h2, h3)))
    got = x + (((e.k0 * d + e.hist[0][1] * h1) + e.hist[1][1] * h2) + e.hist[2][1] * h3)
    assert torch.equal(got, want)


# --------------------------------------------------------------------------------------------------- unsupported options
def test_unsupported_options_raise():
    x = torch.zeros((1, 4, 8, 8))
    s = _make(5)
    with pytest.raises(NotImplementedError, match="attend-and-excite"):
        s(None, x, {}, {}, aae_enabled=True)
    with pytest.raises(NotImplementedError, match="detailed"):
        s(None, x, {}, {}, detailed=True)
    s = _make(5, guider={"target": "sgm.modules.diffusionmodules.guiders.IdentityGuider"})
    with pytest.raises(NotImplementedError, match="VanillaCFG"):
        s(None, x, {}, {})
    with pytest.raises(NotImplementedError, match="VanillaCFG"):
        s.sample_lane(None, x, {}, {}, slot=0, n_lanes=2)
    s = _make(5, order=9)
    for call in (lambda: s(None, x, {}, {}), lambda: s.sample_lane(None, x, {}, {}, slot=0, n_lanes=2),
                 lambda: s.sample_in_flight(None, [x, x], [{}, {}], [{}, {}])):
        with pytest.raises(NotImplementedError, match="order 9"):
            call()
