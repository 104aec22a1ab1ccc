"""A torch restatement of one accumulation window of the reference's training loop — accumulate, AdamW, LitEma, in that order —
for tests/test_optim_cpu.py and tests/test_optim_gpu.py.  TEST INFRASTRUCTURE: plain torch on whatever device the tensors are on.

What it restates (the loop tests/golden/make_optim_golden.py runs on the real reference):
  * Lightning with ``accumulate_grad_batches = N`` (configs/train.yaml:21): ``(loss / N).backward()`` per micro-batch, .grad summing
    up inside a window; ``optimizer.step()`` on the window's last micro-batch;
  * torch.optim.AdamW's single-tensor step (decoupled weight decay, bias-corrected moments);
  * ``on_train_batch_end`` after EVERY micro-batch, after the step where there is one (sgm/models/diffusion.py:178-180):
    LitEma.forward (sgm/modules/ema.py:33-52) with decay = min(decay, (1 + n) / (10 + n)) counted per micro-batch.
"""
from __future__ import annotations

from typing import Callable, Dict, List

import torch

T = Dict[str, torch.Tensor]


def one_minus_decay(num_updates: int, decay: float = 0.9999) -> float:
    """1 - decay of LitEma's update number ``num_updates`` (1-based), in its fp32 arithmetic (ema.py:36-40)"""
    n = torch.tensor(num_updates, dtype=torch.int)
    d = torch.minimum(torch.tensor(decay, dtype=torch.float32), (1 + n) / (10 + n))
    return float(1.0 - d)


def adamw_step(p: T, g: T, m: T, v: T, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2) -> None:
    """torch.optim.AdamW (_single_tensor_adamw), in place on p / m / v"""
    b1, b2 = betas
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    for n in p:
        p[n].mul_(1.0 - lr * weight_decay)
        m[n].lerp_(g[n], 1.0 - b1)
        v[n].mul_(b2).addcmul_(g[n], g[n], value=1.0 - b2)
        denom = (v[n].sqrt() / bc2 ** 0.5).add_(eps)
        p[n].addcdiv_(m[n], denom, value=-lr / bc1)


def ema_update(shadow: T, p: T, omd: float) -> None:
    """LitEma.forward's tensor update (ema.py:50-52)"""
    for n in p:
        shadow[n].sub_(omd * (shadow[n] - p[n]))


def window_loop(p: T, grad_fn: Callable[[T, int], tuple], n_calls: int, accumulate: int, lr: float, eps: float, weight_decay: float,
                decay: float = 0.9999) -> dict:
    """run ``n_calls`` micro-batches from the parameters ``p`` (updated in place).  ``grad_fn(p, k)`` -> (loss dict, {name: gradient
    of micro-batch k's loss}).  Returns {"losses": [loss dict per call], "grads": [accumulated (mean) gradient per window],
    "dp": [p - p_0 per window], "shadow": [shadow - p_0 per call], "omd": [1 - decay per call], "steps": calls that stepped}"""
    p0 = {n: t.clone() for n, t in p.items()}
    shadow = {n: t.clone() for n, t in p.items()}
    m = {n: torch.zeros_like(t) for n, t in p.items()}
    v = {n: torch.zeros_like(t) for n, t in p.items()}
    acc: T = {}
    out = {"losses": [], "grads": [], "dp": [], "shadow": [], "omd": [], "steps": []}
    step = 0
    for k in range(n_calls):
        ld, g = grad_fn(p, k)
        out["losses"].append(ld)
        for n in p:                                                  # (loss / N).backward(): .grad += g / N
            acc[n] = g[n] / accumulate if n not in acc else acc[n] + g[n] / accumulate
        if (k + 1) % accumulate == 0:
            step += 1
            out["grads"].append({n: t.clone() for n, t in acc.items()})
            adamw_step(p, acc, m, v, step, lr, eps=eps, weight_decay=weight_decay)
            acc = {}
            out["dp"].append({n: p[n] - p0[n] for n in p})
            out["steps"].append(k + 1)
        omd = one_minus_decay(k + 1, decay)                          # on_train_batch_end
        ema_update(shadow, p, omd)
        out["omd"].append(omd)
        out["shadow"].append({n: shadow[n] - p0[n] for n in p})
    return out


def rel_sub(tensors: T, ref_sub, names: List[str]):
    """rel rms over all tensors of their strided sub-samples (aae_fixture.sub) against a golden's [n_tensors, width] array;
    returns (rel rms, worst tensor's rel rms, its name)"""
    from aae_fixture import sub
    ref_sub = torch.as_tensor(ref_sub)
    num = den = 0.0
    worst = (0.0, "")
    for i, n in enumerate(names):
        s_ = sub(tensors[n], ref_sub.shape[1]).cpu().double()
        r_ = ref_sub[i, :s_.numel()].double()
        e, d = float((s_ - r_).pow(2).sum()), float(r_.pow(2).sum())
        num, den = num + e, den + d
        if d > 0 and (e / d) ** 0.5 > worst[0]:
            worst = ((e / d) ** 0.5, n)
    return (num / den) ** 0.5 if den > 0 else (0.0 if num == 0 else float("inf")), worst[0], worst[1]
