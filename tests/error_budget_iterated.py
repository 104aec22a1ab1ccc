"""Error growth of the ITERATED reverse-pass forms (CPU, the oracle): how much does a per-gradient error grow over the attend-and-excite
loop and over three AdamW steps?  Not a test — a script (``python tests/error_budget_iterated.py``, ~5 minutes) whose output calibrates
the free-running tolerances of tests/test_iterated_gpu.py.

The fp32 oracle (oracle/backward.py, oracle/training.py) runs the G15 loops of tests/golden/iterated_golden.npz twice: clean, and with a
relative error of E = 1e-2 injected into every gradient it produces, in two forms:

  rand   g + E rms(g) N(0, 1), an independent draw per gradient            (uncorrelated rounding)
  scale  g (1 + E)                                                          (an error that points the same way at every iteration)

and reports, per quantity, the deviation from the clean run divided by E — the growth factor G.  A GPU gradient within TOL of the
reference then moves a free-running quantity by at most G TOL; the tests state their tolerances from these factors.

  G15a(ii)  three attend-and-excite updates: the displacement x_3 - x_0 (rel rms)
  G15c      three training steps: the losses of steps 2 / 3 (relative to the loss), the gradients of steps 2 / 3 and p_k - p_0 (rel rms
            over all trained tensors)

``--rounding``: the per-evaluation error of the training loss itself — the eps-prediction loss of the three G15c draws with the HIP
path's bf16 roundings injected (tests/error_budget.py) against fp32.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import backward as obw, nets, sampling, spec, training as otr     # noqa: E402
from udifftext_amd import synth                                              # noqa: E402
from aae_fixture import aae_batch, train_batch                               # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
E = 1e-2


def _rel(a, b):
    return float((a - b).double().pow(2).sum().sqrt() / b.double().pow(2).sum().sqrt())


def _rel_all(a: dict, b: dict):
    num = sum(float((a[n] - b[n]).double().pow(2).sum()) for n in b)
    den = sum(float(b[n].double().pow(2).sum()) for n in b)
    return (num / den) ** 0.5


def _inject(kind: str, g: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
    if kind == "clean":
        return g
    if kind == "scale":
        return g * (1.0 + E)
    return g + E * g.pow(2).mean().sqrt() * torch.randn(g.shape, generator=gen)


def _g14_cond():
    """G15c trains at G14's conditioning"""
    g14 = np.load(os.path.join(GOLD, "train_golden.npz"))
    return {"concat": torch.from_numpy(g14["g14_c_concat"]), "t_crossattn": torch.from_numpy(g14["g14_c_txt"])}


def engine_sd():
    cfg = spec.EngineConfig()
    d = synth.synthetic_state_dict(spec.engine_param_shapes(cfg))
    d["denoiser.sigmas"] = sampling.denoiser_sigma_table(1000)
    d["loss_fn.g_kernel"] = sampling.gaussian_kernel(3, 1.0, 12)
    return d, cfg


def aae_loop(sd, cfg, g):
    """G15a(ii): x_{k+1} = x_k - alpha grad(x_k), three updates"""
    batch = aae_batch()
    g13 = np.load(os.path.join(GOLD, "aae_golden.npz"))                 # (G15a runs at G13's conditioning)
    c = {"concat": torch.from_numpy(g13["g13_c_concat"]), "t_crossattn": torch.from_numpy(g13["g13_c_txt"])}
    x0, sigma = torch.from_numpy(g["g15a_ii_x"][0]), torch.from_numpy(g["g15a_sigma"])
    alpha = float(g["g15a_alpha"][0])
    res = {}
    for kind in ("clean", "rand", "scale"):
        gen = torch.Generator().manual_seed(1)
        x = x0.clone()
        for _ in range(3):
            _, gr = obw.attend_and_excite_grad(sd, cfg, x, sigma, c, batch["mask"], batch["seg_mask"])
            x = x - alpha * _inject(kind, gr, gen)
        res[kind] = x - x0
        print(f"[budget] G15a(ii) {kind}: |x_3 - x_0| rms {float(res[kind].pow(2).mean().sqrt()):.4e}", flush=True)
    for kind in ("rand", "scale"):
        print(f"[budget] G15a(ii) {kind:5s}: displacement x_3 - x_0  G = {_rel(res[kind], res['clean']) / E:.3f}")


def train_loop(sd, cfg, g):
    """G15c: three AdamW steps (torch.optim.AdamW, the golden's lr / eps / weight decay, LambdaLR epoch 1 before step 3)"""
    tb = train_batch()
    z = torch.from_numpy(g["g15c_z"])
    cond = _g14_cond()
    idxs, noises = torch.from_numpy(g["g15c_sigma_idx"]), torch.from_numpy(g["g15c_noise"])
    lr, eps, wd = float(g["g15c_lr"][0]), float(g["g15c_eps"][0]), float(g["g15c_weight_decay"][0])
    names = otr.trainable_names(sd)
    out = {}
    for kind in ("clean", "rand", "scale"):
        gen = torch.Generator().manual_seed(2)
        sdk = dict(sd)
        params = [torch.nn.Parameter(sd[n].clone()) for n in names]
        opt = torch.optim.AdamW(params, lr=lr, eps=eps, weight_decay=wd)
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lambda ep: 0.95 ** ep)
        rec = []
        for k in range(3):
            if k == 2:
                sched.step()
            for n, p_ in zip(names, params):
                sdk[n] = p_.detach()
            ld, gr = otr.training_grads(sdk, cfg, z, cond, tb["seg"], tb["seg_mask"], idxs[k], noises[k], 0.0)
            with torch.enable_grad():
                for n, p_ in zip(names, params):
                    p_.grad = _inject(kind, gr[n], gen)
                opt.step()
            rec.append((float(ld["loss/full_loss"]), gr, {n: p_.detach() - sd[n] for n, p_ in zip(names, params)}))
            print(f"[budget] G15c {kind} step {k + 1}: loss {rec[-1][0]:.6f}", flush=True)
        out[kind] = rec
    cl = out["clean"]
    for kind in ("rand", "scale"):
        r = out[kind]
        for k in range(3):
            print(f"[budget] G15c {kind:5s} step {k + 1}: loss G = {abs(r[k][0] - cl[k][0]) / abs(cl[k][0]) / E:.3f}  "
                  f"|dL| / L = {abs(cl[k][0] - cl[k - 1][0]) / abs(cl[k][0]) if k else float('nan'):.3f}  "
                  f"grad G = {_rel_all(r[k][1], cl[k][1]) / E:.3f}  p_k - p_0 G = {_rel_all(r[k][2], cl[k][2]) / E:.3f}")


def train_loss_rounding(sd, cfg, g):
    """the PER-EVALUATION error of the training loss: the eps-prediction loss of G15c's three draws with the HIP path's bf16 roundings
    injected (tests/error_budget.py, the flags of its "all" row) against the fp32 loss"""
    import error_budget as eb
    z = torch.from_numpy(g["g15c_z"])
    cond = _g14_cond()
    table = sd["denoiser.sigmas"]
    base = dict(W=False, A=False, O=False, N=False, N_ln=True, P=False, R32=False, A8=False, L8=False)
    for k in range(3):
        idx, noise = torch.from_numpy(g["g15c_sigma_idx"][k]), torch.from_numpy(g["g15c_noise"][k])
        sigma = table[idx][:, None, None, None]
        noised = z + noise * sigma
        xin = torch.cat((noised / (sigma ** 2 + 1.0) ** 0.5, cond["concat"]), dim=1)
        losses = []
        for fl in ({}, dict(W=True, A=True, O=True, N=True, P=True)):
            eb.FLAGS.update(base)
            eb.FLAGS.update(fl)
            eps = eb.unet(sd, xin, idx, cond["t_crossattn"], cfg.unet)
            losses.append(float((sigma ** -2.0 * (eps * (-sigma) + noised - z) ** 2).reshape(2, -1).mean(1).mean()))
        print(f"[budget] G15c draw {k + 1}: eps-prediction loss fp32 {losses[0]:.6f}, with the bf16 roundings {losses[1]:.6f}: "
              f"rel err {abs(losses[1] - losses[0]) / abs(losses[0]):.3e}", flush=True)
    eb.FLAGS.update(base)


if __name__ == "__main__":
    torch.set_grad_enabled(False)
    g = np.load(os.path.join(GOLD, "iterated_golden.npz"))
    sd, cfg = engine_sd()
    if "--rounding" in sys.argv:
        train_loss_rounding(sd, cfg, g)
        sys.exit(0)
    if "--train" not in sys.argv:
        aae_loop(sd, cfg, g)
    if "--aae" not in sys.argv:
        train_loop(sd, cfg, g)
