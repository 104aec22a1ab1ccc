"""Generate tests/golden/optim_golden.npz (G16): two accumulation windows of two micro-batches each with the REAL reference's
FullLoss, torch.optim.AdamW and LitEma, on the CPU.

    UDT_REFERENCE=<reference checkout> python tests/golden/make_optim_golden.py        # ~5 minutes, ~12 GB

Lightning is not installed where the goldens are made, so its loop is written out by hand.  What it restates:

  * configs/train.yaml:21 ``accumulate_grad_batches: N``: Lightning's automatic optimisation calls ``(loss / N).backward()`` per
    micro-batch without clearing the gradients inside a window, and ``optimizer.step()`` + ``zero_grad()`` on the window's last
    micro-batch;
  * sgm/models/diffusion.py:75-77 builds ``LitEma(self.model)`` in the constructor, while every UNet parameter still requires a
    gradient, and configure_optimizers (:202-222) then takes ``requires_grad`` from the tensors opt_keys does not select.  In that
    order LitEma.forward cannot run: sgm/modules/ema.py:53-54 asserts that a tensor without requires_grad has no shadow (this
    script tried it: AssertionError at the first update).  The one order in which the reference's EMA runs with opt_keys is
    LitEma AFTER requires_grad is settled — shadows for the trained tensors only, which ema.py:46-52 then moves.  That is the
    order used here, and the stored model_ema.* key list is that LitEma's;
  * diffusion.py:178-180: ``on_train_batch_end`` runs after EVERY micro-batch, after the optimiser step where there is one: the EMA
    moves and counts num_updates per micro-batch (ema.py:36-38: decay = min(decay, (1 + n) / (10 + n)) = 2/11, 3/12, 4/13, 5/14).

Model, conditioning, z, optimiser (lr 1.6e-2, eps 1.0, weight decay 1e-2, lambda_local_loss = 0) and the first three draws are G14 /
G15c's (make_golden.py); the fourth draw is the next one of G15c's generator.  Stored, per trained tensor as the ``sub()`` samples
G15c stores (gradients 256 values, displacements 128): each micro-batch's loss dict, each window's accumulated gradient, p_k - p_0
after each window, shadow - p_0 after each of the four EMA updates, the model_ema.* key list with the trained keys marked.

Conditions asserted here and stored:
  * ``g16_grad_ratio`` [2]: (rms g_a + rms g_b) / 2 / rms((g_a + g_b) / 2) <= 1.5 per window (over all trained tensors): an error of
    TOL per evaluation is at most ratio * TOL of the mean;
  * ``g16_shadow_ratio`` [4]: the same for each shadow displacement, a fixed combination sum_k c_k (p_k - p_0):
    sum_k |c_k| rms(p_k - p_0) / rms(shadow - p_0) <= 1.5 (the first displacement is exactly zero: no optimiser step yet; ratio 1);
  * window 2 evaluated with window 1's update ignored: both micro-batch losses move by >= 3 x TOL_LOSS_FREE (relative) and the
    accumulated gradient by >= 5 x TOL_GRAD_FREE x its ratio (tests/test_iterated_gpu.py's free-running bounds).
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import time

import numpy as np
import torch
import torch.nn as nn
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as MG  # noqa: E402  (import recipe, G15C_* optimiser settings; exits without UDT_REFERENCE)
from aae_fixture import sub as gsub, train_batch  # noqa: E402

from udifftext_amd import synth  # noqa: E402

N_ACC = 2
TOL_LOSS_FREE, TOL_GRAD_FREE = MG.G15C_LOSS_TOL, MG.G15C_GRAD_TOL
RATIO_MAX = 1.5


def _rms(ts) -> float:
    return (sum(float(t.double().pow(2).sum()) for t in ts) / sum(t.numel() for t in ts)) ** 0.5


def _pack(ts, n):
    return np.stack([np.pad(gsub(t, n).numpy(), (0, n - gsub(t, n).numel())) for t in ts])


def build_model():
    MG.import_reference()
    from sgm.util import instantiate_from_config
    cfg = yaml.safe_load(open(os.path.join(MG.REF, "configs/test/textdesign_sd_2.yaml")))
    MG.strip_ckpt(cfg)
    model = instantiate_from_config(cfg["model"]).eval()
    nn.Module.train(model.conditioner.embedders[0], False)                # (the goldens pin the dropout-free network: make_golden.py)
    for name, p in model.state_dict().items():
        if not synth.is_computed_buffer(name):
            p.copy_(synth.synthetic_tensor(name, tuple(p.shape)))
    return model


def main():
    t0 = time.time()
    torch.set_grad_enabled(False)
    model = build_model()
    from sgm.modules.ema import LitEma
    print(f"[optim golden] reference engine built ({time.time() - t0:.1f}s)", flush=True)
    g14 = np.load(os.path.join(HERE, "train_golden.npz"))
    g15 = np.load(os.path.join(HERE, "iterated_golden.npz"))
    tb = train_batch()
    torch.manual_seed(4321)
    z = torch.randn((2, 4, 16, 16)) * 0.8
    noise1 = torch.randn((2, 4, 16, 16))
    assert np.array_equal(z.numpy(), g14["g14_z"]) and np.array_equal(noise1.numpy(), g14["g14_noise"])
    gen = torch.Generator().manual_seed(1515)
    draws = [(torch.tensor([700, 250]), noise1)]
    for _ in range(3):                                                    # G15c's two draws and the generator's next one
        draws.append((torch.randint(0, 1000, (2,), generator=gen), torch.randn((2, 4, 16, 16), generator=gen)))
    assert np.array_equal(torch.stack([d[0] for d in draws[:3]]).numpy(), g15["g15c_sigma_idx"])
    assert np.array_equal(torch.stack([d[1] for d in draws[:3]]).numpy(), g15["g15c_noise"])

    loss_fn = model.loss_fn
    loss_fn.lambda_local_loss = 0.0
    sigmas_tab = model.denoiser.sigmas
    model.learning_rate = MG.G15C_LR
    model.optimizer_config = {"target": "torch.optim.AdamW", "params": {"eps": MG.G15C_EPS}}
    model.opt_keys = ["t_attn", "t_norm"]
    with contextlib.redirect_stdout(io.StringIO()):
        (opt,), _ = model.configure_optimizers()                           # diffusion.py:202-222
    model.use_ema = True
    model.model_ema = LitEma(model.model, decay=0.9999)                    # diffusion.py:75-77 (see the module docstring for the order)
    named = [("model." + n, p_) for n, p_ in model.model.named_parameters() if any(k in n for k in ("t_attn", "t_norm"))]
    names, params = [n for n, _ in named], [p_ for _, p_ in named]
    assert names == [str(n) for n in g14["g14_names"]]
    assert [id(p_) for p_ in opt.param_groups[0]["params"]] == [id(p_) for p_ in params]
    assert opt.defaults["weight_decay"] == MG.G15C_WD and opt.defaults["eps"] == MG.G15C_EPS
    assert [n_ for n_, p_ in model.model.named_parameters() if p_.requires_grad] == [n[len("model."):] for n in names]
    ema = model.model_ema
    ema_keys = ["model_ema." + k for k in ema.state_dict()]
    s_names = [ema.m_name2s_name[n[len("model."):]] for n in names]
    trained_keys = {"model_ema." + s for s in s_names}
    p0 = [p_.detach().clone() for p_ in params]
    shadows = lambda: [getattr(ema, s) for s in s_names]

    recorded = {}
    real_cond = model.conditioner.forward

    def cond_once(b, *a, **k):
        if "cond" not in recorded:
            recorded["cond"] = real_cond(b, *a, **k)
        return recorded["cond"]
    real_randn_like = torch.randn_like
    cur = {}
    loss_fn.sigma_sampler = lambda n, rand=None: sigmas_tab[cur["idx"]]
    out = {}
    dps, disp = [], []                                    # p_k - p_0 per window; shadow - p_0 after each EMA update
    grad_ratio, shadow_ratio, decays = [], [], []

    def ema_update():
        ema(model.model)                                                   # diffusion.py:178-180
        decays.append(1.0 - float((1 + ema.num_updates) / (10 + ema.num_updates)))
        disp.append([s_.detach() - q_ for s_, q_ in zip(shadows(), p0)])

    def micro(draw):
        cur["idx"], cur["noise"] = draw
        loss, ld = loss_fn(model.model, model.denoiser, model.conditioner, z, tb, model.first_stage_model, model.scale_factor)
        (loss / N_ACC).backward()                                          # Lightning: accumulate_grad_batches = N
        return ld

    try:
        model.conditioner.forward = cond_once
        torch.randn_like = lambda t, **k: cur["noise"].clone()
        with torch.enable_grad():
            call = 0
            stale = None
            for w in range(2):
                opt.zero_grad(set_to_none=True)
                parts, lds = [], []
                for j in range(N_ACC):
                    ld = micro(draws[w * N_ACC + j])
                    lds.append(ld)
                    acc = [p_.grad.detach().clone() for p_ in params]
                    parts.append([a_ * N_ACC for a_ in acc] if j == 0 else [(a_ - b_ / N_ACC) * N_ACC for a_, b_ in zip(acc, parts[0])])
                    for kk, v in ld.items():
                        out[f"g16_{call + j + 1}_" + kk.replace("/", "_")] = np.array([float(v.detach())])
                    if j + 1 < N_ACC:                                      # on_train_batch_end of a micro-batch without a step
                        ema_update()
                gacc = [p_.grad.detach().clone() for p_ in params]
                ratio = 0.5 * (_rms(parts[0]) + _rms(parts[1])) / _rms(gacc)
                assert ratio <= RATIO_MAX, ("gradient ratio", w, ratio)
                grad_ratio.append(ratio)
                if w == 0:                                                 # window 2 with this window's update ignored
                    saved = [p_.grad for p_ in params]
                    for p_ in params:
                        p_.grad = None
                    st_l = [float(micro(draws[N_ACC + j])["loss/full_loss"].detach()) for j in range(N_ACC)]
                    stale = (st_l, [p_.grad.detach().clone() for p_ in params])
                    for p_, g_ in zip(params, saved):
                        p_.grad = g_
                else:
                    true_l = [float(ld_["loss/full_loss"].detach()) for ld_ in lds]
                    for a_, b_ in zip(true_l, stale[0]):
                        assert abs(a_ - b_) >= 3 * TOL_LOSS_FREE * abs(a_), ("stale loss", true_l, stale[0])
                    gd = (sum(float((a_ - b_).double().pow(2).sum()) for a_, b_ in zip(gacc, stale[1])) /
                          sum(float(a_.double().pow(2).sum()) for a_ in gacc)) ** 0.5
                    assert gd >= 5 * TOL_GRAD_FREE * ratio, ("stale gradient", gd, ratio)
                    out["g16_loss_update_ignored"] = np.array(stale[0])
                    out["g16_grad_update_ignored_rel"] = np.array([gd])
                    print(f"[optim golden] window 2 losses {true_l}, with window 1's update ignored {stale[0]}; gradient moved by {gd:.3f}")
                opt.step()
                ema_update()                                               # on_train_batch_end of the stepping micro-batch
                call += N_ACC
                dps.append([p_.detach() - q_ for p_, q_ in zip(params, p0)])
                out[f"g16_w{w + 1}_grad_sub"] = _pack(gacc, MG.G15C_GRAD_SUB)
                out[f"g16_w{w + 1}_grad_stats"] = np.stack([MG.stats(g_) for g_ in gacc])
                out[f"g16_w{w + 1}_dp_sub"] = _pack(dps[-1], MG.G15C_DP_SUB)
                out[f"g16_w{w + 1}_dp_stats"] = np.stack([MG.stats(d_) for d_ in dps[-1]])
                print(f"[optim golden] window {w + 1}: losses {[float(ld_['loss/full_loss'].detach()) for ld_ in lds]}, gradient ratio {ratio:.3f} "
                      f"({time.time() - t0:.1f}s)", flush=True)
    finally:
        model.conditioner.forward = real_cond
        torch.randn_like = real_randn_like
    assert int(ema.num_updates) == 2 * N_ACC and len(disp) == 2 * N_ACC
    assert np.allclose(decays, [9 / 11, 9 / 12, 9 / 13, 9 / 14])          # one_minus_decay of updates 1 .. 4
    out["g16_one_minus_decay"] = np.array(decays)
    # shadow_j - p_0 = c[0] (p_1 - p_0) + c[1] (p_2 - p_0): update j saw p_0, p_1, p_1, p_2
    c = [0.0, 0.0]
    for j in range(2 * N_ACC):
        omd = decays[j]
        c = [ci * (1 - omd) for ci in c]
        if j > 0:
            c[0 if j < 3 else 1] += omd
        if j == 0:
            assert all(not bool(d_.any()) for d_ in disp[0])              # no optimiser step yet: the shadow has not moved
            ratio = 1.0
        else:
            ratio = sum(abs(ci) * _rms(dps[i]) for i, ci in enumerate(c)) / _rms(disp[j])
            comb = [c[0] * a_ + c[1] * b_ for a_, b_ in zip(dps[0], dps[1])]
            # (fp32 cancellation in shadow - p_0 and p_k - p_0 leaves ~1e-4 of the displacement; wrong coefficients would leave ~1e-1)
            err = (sum(float((a_ - b_).double().pow(2).sum()) for a_, b_ in zip(comb, disp[j])) /
                   sum(float(b_.double().pow(2).sum()) for b_ in disp[j])) ** 0.5
            assert err <= 1e-3, ("shadow displacement is not the stated combination", j, err)
        assert ratio <= RATIO_MAX, ("shadow ratio", j, ratio)
        shadow_ratio.append(ratio)
        out[f"g16_{j + 1}_shadow_sub"] = _pack(disp[j], MG.G15C_DP_SUB)
        out[f"g16_{j + 1}_shadow_coefs"] = np.array(c)
    cond = recorded["cond"]
    # (G14's conditioning, which the tests feed: the same draws; the label encoder's fp32 sums depend on the host's thread count)
    assert np.array_equal(cond["concat"].detach().numpy(), g14["g14_c_concat"])
    assert np.allclose(cond["t_crossattn"].detach().numpy(), g14["g14_c_txt"], rtol=1e-4, atol=1e-5)
    out.update({"g16_sigma_idx": torch.stack([d[0] for d in draws]).numpy(), "g16_noise": torch.stack([d[1] for d in draws]).numpy(),
                "g16_names": np.array(names), "g16_grad_ratio": np.array(grad_ratio), "g16_shadow_ratio": np.array(shadow_ratio),
                "g16_ema_keys": np.array(ema_keys), "g16_ema_trained": np.array([k in trained_keys for k in ema_keys]),
                "g16_lr": np.array([MG.G15C_LR]), "g16_eps": np.array([MG.G15C_EPS]), "g16_weight_decay": np.array([MG.G15C_WD]),
                "g16_accumulate": np.array([N_ACC])})
    path = os.path.join(HERE, "optim_golden.npz")
    np.savez_compressed(path, **out)
    print(f"[optim golden] done ({time.time() - t0:.1f}s): gradient ratios {grad_ratio}, shadow ratios {shadow_ratio}, "
          f"{len(ema_keys)} model_ema keys ({len(trained_keys)} trained), {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
