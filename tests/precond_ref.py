"""Torch restatement of the preconditioned sampler-step kernels (udt_precond_*) and of the preconditioned loss, for any dtype
(the tests evaluate it in float64).

oracle.sampling.denoise_cfg is eps-prediction only; this file is the general form the kernels state in include/udt_kernels.h:

    den_{u,c} = c_skip*x + c_out*F_{u,c};  pair: den = den_u + scale*(den_c - den_u);  unguided: den = c_skip*x + c_out*F

with the three updates (Euler, the affine sampler form, linear multistep), the UNet-input pack, a plan runner that drives any
sampler's plans through them with a network given as a function, and the loss mean(w (c_skip*noised + c_out*F - target)^2) under
autograd.  ``closed_form`` holds the scalings / weightings as formulas of their own (reference denoiser_scaling.py:4-31,
denoiser_weighting.py:4-24), independent of the package's classes.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import torch


# ------------------------------------------------------------------------------------------------------------ closed forms
def closed_form(kind: str, sigma: float, sigma_data: float = 0.5):
    """(c_skip, c_out, c_in, c_noise) of EpsScaling / VScaling / EDMScaling at sigma, in Python floats (float64)"""
    if kind == "eps":
        return 1.0, -sigma, 1.0 / math.sqrt(sigma * sigma + 1.0), sigma
    if kind == "v":
        d = sigma * sigma + 1.0
        return 1.0 / d, -sigma / math.sqrt(d), 1.0 / math.sqrt(d), sigma
    if kind == "edm":
        d = sigma * sigma + sigma_data * sigma_data
        return sigma_data * sigma_data / d, sigma * sigma_data / math.sqrt(d), 1.0 / math.sqrt(d), 0.25 * math.log(sigma)
    raise ValueError(kind)


def weighting(kind: str, sigma: float, sigma_data: float = 0.5) -> float:
    """UnitWeighting / EpsWeighting / VWeighting / EDMWeighting at sigma"""
    if kind == "unit":
        return 1.0
    if kind == "eps":
        return sigma ** -2.0
    sd = 1.0 if kind == "v" else sigma_data
    return (sigma * sigma + sd * sd) / (sigma * sd) ** 2


# ------------------------------------------------------------------------------------------------------------ the kernels' formulas
def nhwc_rows(f: torch.Tensor) -> torch.Tensor:
    """network output NHWC [rows, h, w, ld] -> NCHW [rows, 4, h, w] (the first four channels)"""
    return f[..., :4].permute(0, 3, 1, 2)


def den(x: torch.Tensor, f: torch.Tensor, c_skip: float, c_out: float, scale: float, pair: bool) -> torch.Tensor:
    """x [B,4,h,w]; f NCHW [2B,4,h,w] (uncond first) when pair, else [B,4,h,w]"""
    B = x.shape[0]
    assert f.shape[0] == (2 * B if pair else B)
    if not pair:
        return c_skip * x + c_out * f
    du, dc = c_skip * x + c_out * f[:B], c_skip * x + c_out * f[B:]
    return du + scale * (dc - du)


def unet_input(x: torch.Tensor, c_in: float, noise: Optional[torch.Tensor] = None, kn: float = 0.0):
    """-> (the stored x, the packed channels x * c_in)"""
    if noise is not None:
        x = x + kn * noise
    return x, x * c_in


def euler_step(x, f, c_skip, c_out, sigma, sigma_next, scale, pair):
    """-> (x_next, den)"""
    d0 = den(x, f, c_skip, c_out, scale, pair)
    return x + (x - d0) / sigma * (sigma_next - sigma), d0


def sampler_step(x, f, c_skip, c_out, scale, pair, kx=0.0, kd=0.0, aux=None, ka=0.0, prev=None, kp=0.0, noise=None, kn=0.0):
    """-> (xout, den)"""
    d0 = den(x, f, c_skip, c_out, scale, pair)
    out = kx * x + kd * d0
    for t, k in ((aux, ka), (prev, kp), (noise, kn)):
        if t is not None:
            out = out + k * t
    return out, d0


def multistep_step(x, f, c_skip, c_out, scale, pair, sigma, coefs, hist=()):
    """-> (xout, d)"""
    d = (x - den(x, f, c_skip, c_out, scale, pair)) / sigma
    acc = coefs[0] * d
    for k, h in zip(coefs[1:], hist):
        acc = acc + k * h
    return x + acc, d


# ------------------------------------------------------------------------------------------------------------ the plan runner
def toy_net(pair: bool) -> Callable:
    """tests/golden/make_sampler_golden.py toy_network; unguided: its conditional half"""
    def net(x_in: torch.Tensor, c_noise: float) -> torch.Tensor:
        t = math.sin(c_noise / 100.0) * 0.05
        if pair:
            return torch.cat((0.8 * torch.tanh(x_in) + t, torch.tanh(x_in + 0.25) + t), 0)
        return torch.tanh(x_in + 0.25) + t
    return net


def run_plans(plans, x0: torch.Tensor, net: Callable, coefs: Callable, scale: float, pair: bool, noise=None, slots=None):
    """drive ``plans`` ((step, plan) pairs of sampling.EulerEval / Eval / MultistepEval) through the formulas above.
    net(x_in, c_noise) -> NCHW network output (2B rows when pair); coefs(sigma) -> (c_skip, c_out, c_in, c_noise) floats.
    -> (latent after every step [steps, B, 4, h, w], the c_noise of every evaluation)"""
    from sgm.modules.diffusionmodules.sampling import EulerEval, MultistepEval
    bufs: Dict[str, torch.Tensor] = {"x": x0.clone()}
    traj, seen = [], []
    slots = slots or {}
    for i, plan in plans:
        nz = noise[slots[i]] if noise is not None and i in slots else None
        for e in plan:
            c_skip, c_out, c_in, c_noise = coefs(e.sigma)
            churn = getattr(e, "churn", 0.0)
            bufs[e.src], xin = unet_input(bufs[e.src], c_in, nz if churn != 0.0 else None, churn)
            seen.append(c_noise)
            f = net(xin, c_noise)
            x = bufs[e.src]
            if isinstance(e, EulerEval):
                bufs[e.src], _ = euler_step(x, f, c_skip, c_out, e.sigma, e.sigma_next, scale, pair)
            elif isinstance(e, MultistepEval):
                bufs[e.out], bufs[e.d_out] = multistep_step(x, f, c_skip, c_out, scale, pair, e.sigma, (e.k0,) + tuple(k for _, k in e.hist),
                                                            [bufs[b] for b, _ in e.hist])
            else:
                out, d0 = sampler_step(x, f, c_skip, c_out, scale, pair, e.kx, e.kd, bufs[e.aux] if e.aux else None, e.ka,
                                       bufs[e.prev] if e.prev else None, e.kp, nz if e.kn != 0.0 else None, e.kn)
                bufs[e.out] = out
                if e.den_out:
                    bufs[e.den_out] = d0
        traj.append(bufs["x"].clone())
    return torch.stack(traj, 0), seen


# ------------------------------------------------------------------------------------------------------------ the loss
def loss_and_grad(f: torch.Tensor, noised: torch.Tensor, target: torch.Tensor, c_skip, c_out, w):
    """f / noised / target NCHW [B,4,h,w]; c_skip / c_out / w [B] -> (loss_b [B], d mean_b(loss_b) / d f) by autograd"""
    col = lambda v: torch.as_tensor(v, dtype=f.dtype).reshape(-1, 1, 1, 1)
    with torch.enable_grad():
        leaf = f.detach().clone().requires_grad_(True)
        out = col(c_skip) * noised + col(c_out) * leaf
        per_sample = (col(w) * (out - target) ** 2).reshape(f.shape[0], -1).mean(dim=1)
        per_sample.mean().backward()
    return per_sample.detach(), leaf.grad


def training_grads(sd, cfg, z, cond, noise, sigma, coefs, w):
    """the diffusion term of the training loss on the fp32 CPU oracle UNet (oracle.nets) under autograd, for any preconditioning:
    noised = z + noise*sigma_b; F = unet(noised*c_in_b, c_noise_b); loss = mean_b mean(w_b (c_skip_b*noised + c_out_b*F - z)^2).
    coefs: one (c_skip, c_out, c_in, c_noise) per sample; w [B].  -> (loss, {trainable name: gradient})"""
    from oracle import nets
    from oracle import training as otr
    names = otr.trainable_names(sd)
    col = lambda v: torch.tensor([float(a) for a in v], dtype=z.dtype).reshape(-1, 1, 1, 1)
    c_skip, c_out, c_in = (col([k[i] for k in coefs]) for i in range(3))
    c_noise = torch.tensor([float(k[3]) for k in coefs], dtype=z.dtype)
    with torch.enable_grad():
        sdg = dict(sd)
        for n in names:
            sdg[n] = sd[n].detach().clone().requires_grad_(True)
        noised = z + noise * col(sigma)
        f = nets.unet_forward(sdg, torch.cat((noised * c_in, cond["concat"]), dim=1), c_noise, cond["t_crossattn"], cfg.unet)
        loss = (col(w) * (c_skip * noised + c_out * f - z) ** 2).reshape(z.shape[0], -1).mean(dim=1).mean()
        gs = torch.autograd.grad(loss, [sdg[n] for n in names])
    return loss.detach(), dict(zip(names, gs))
