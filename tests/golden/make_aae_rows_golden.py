"""Generate tests/golden/aae_rows_golden.npz: the REAL reference's EulerEDMSampler.attend_and_excite (reference sampling.py:233-252) run
on the CPU at B = 1, one toy sample at a time — what every row of the row-wise loop (udt_aae_row_update_f32,
EulerEDMSampler.attend_and_excite_rows) has to reproduce on its own, whatever its batch mates do.

    UDT_REFERENCE=<reference checkout> python tests/golden/make_aae_rows_golden.py        # seconds

The engine is a stub around the reference's own DiscreteDenoiser (configs/test/textdesign_sd_2.yaml): ``model.model(x, c_noise, cond)``
stashes x, ``loss_fn.get_min_local_loss`` returns the smooth toy loss of tests/aae_rows_ref.py of the stashed x, and the loop — clone,
requires_grad, torch.autograd.grad, x - alpha * grad, the exit condition — is the reference's.  Samples on [1, 4, 8, 8], in groups that
share (alpha, thres, max_iter, iter_enabled):
    group 0  iter_enabled, max_iter 20, thres -0.5: update counts 1, two different middle values, and the cap 21
    group 1  iter_enabled, max_iter 2,  thres -0.5: the cap 3 (and one sample that ends at 2)
    group 2  iter_enabled False: one update
Asserted here: at every iteration |loss - thres| >= 1e-3 max(|thres|, 1), so that no fp32 reordering can flip a count.
Stored: x0, x_final, counts, the per-iteration losses (NaN-padded), the groups' settings, the toy's parameters.  Data only.
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (import_reference; exits without UDT_REFERENCE)

import aae_rows_ref as R  # noqa: E402

ALPHA = 18.0
# group -> (thres, max_iter, iter_enabled)
GROUPS = [(-0.5, 20, True), (-0.5, 2, True), (0.0, 20, False)]
# sample -> (group, offset c, amplitude of x0 - t, seed)
SAMPLES = [
    (0, -0.80, 0.10, 1),          # below thres at once: 1 update
    (0, -0.80, 1.00, 2),          # a middle count
    (0, -0.80, 2.50, 3),          # another middle count
    (0, 0.00, 1.00, 4),           # never below thres: the cap, 21
    (1, -0.80, 2.50, 5),          # max_iter 2: the cap, 3
    (1, -0.80, 0.45, 6),          # max_iter 2: below thres at the second evaluation
    (2, -0.80, 2.50, 7),          # iter_enabled False: 1 update
]
PAD = 24


def main():
    MG.import_reference()
    from sgm.util import instantiate_from_config
    import sgm.modules.diffusionmodules.sampling as S

    cfg = yaml.safe_load(open(os.path.join(MG.REF, "configs/test/textdesign_sd_2.yaml")))
    denoiser = instantiate_from_config(cfg["model"]["params"]["denoiser_config"])
    sampler = S.EulerEDMSampler(num_steps=10, discretization_config={"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"},
                                guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 5.0}},
                                verbose=False, device="cpu")
    out = {k: [] for k in ("x0", "x_final", "counts", "losses", "group", "toy_w", "toy_t", "toy_c")}
    for group, c, amp, seed in SAMPLES:
        thres, max_iter, iter_enabled = GROUPS[group]
        g = torch.Generator().manual_seed(9100 + seed)
        w = 1.0 + 4.0 * torch.rand((1, 4, 8, 8), generator=g)
        t = torch.randn((1, 4, 8, 8), generator=g)
        x0 = t + amp * torch.randn((1, 4, 8, 8), generator=g)
        cc = torch.tensor([c], dtype=torch.float32)
        stash, losses = {}, []

        class Net:
            diffusion_model = types.SimpleNamespace(attn_map_cache=[])

            def __call__(self, x, c_noise, cond):
                stash["x"] = x

        def get_min_local_loss(cache, mask, seg_mask):
            ll = R.toy_loss(stash["x"], w, t, cc)
            losses.append(float(ll.detach()))
            return ll

        model = types.SimpleNamespace(denoiser=denoiser, model=Net(), loss_fn=types.SimpleNamespace(get_min_local_loss=get_min_local_loss))
        with torch.enable_grad():
            xf = sampler.attend_and_excite(x0.clone(), model, torch.tensor([5.0]), {}, {"mask": None, "seg_mask": None}, ALPHA, iter_enabled,
                                           thres, max_iter=max_iter)
        if iter_enabled:
            margin = 1e-3 * max(abs(thres), 1.0)
            assert all(abs(v - thres) >= margin for v in losses), (seed, losses, thres)
        assert len(losses) <= PAD
        out["x0"].append(x0[0].numpy())
        out["x_final"].append(xf.detach()[0].numpy())
        out["counts"].append(len(losses))
        out["losses"].append(np.array(losses + [np.nan] * (PAD - len(losses)), dtype=np.float32))
        out["group"].append(group)
        out["toy_w"].append(w[0].numpy())
        out["toy_t"].append(t[0].numpy())
        out["toy_c"].append(c)
        print(f"[aae rows golden] sample {seed} group {group}: {len(losses)} updates, losses {losses[0]:.4f} .. {losses[-1]:.4f}")
    counts = out["counts"]
    g0 = sorted(n for n, s in zip(counts, SAMPLES) if s[0] == 0)
    assert g0[0] == 1 and g0[-1] == 21 and 1 < g0[1] < g0[2] < 21, g0
    assert [n for n, s in zip(counts, SAMPLES) if s[0] == 1] == [3, 2] and counts[-1] == 1, counts
    res = {k: np.stack(v) if isinstance(v[0], np.ndarray) else np.array(v) for k, v in out.items()}
    res["toy_c"] = res["toy_c"].astype(np.float32)
    res["counts"] = res["counts"].astype(np.int32)
    res["group"] = res["group"].astype(np.int32)
    res["alpha"] = np.array([ALPHA], dtype=np.float64)
    res["group_thres"] = np.array([g[0] for g in GROUPS], dtype=np.float64)
    res["group_max_iter"] = np.array([g[1] for g in GROUPS], dtype=np.int32)
    res["group_iter_enabled"] = np.array([int(g[2]) for g in GROUPS], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, "aae_rows_golden.npz"), **res)
    print(f"[aae rows golden] written: counts {counts}")


if __name__ == "__main__":
    main()
