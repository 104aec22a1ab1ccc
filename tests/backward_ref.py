"""Plain restatements of csrc/backward.hip's operations for tests/sliced_check.py (a helper, not a test; CPU only).

Every function evaluates the closed form in ``dtype`` (float64: the reference; float32: the CPU evaluation that shows a bound is
attainable in the kernel's arithmetic) on bf16- or fp32-valued operands and returns plain tensors.  With ``emulate=True`` the same
computation is rounded where the kernel's header comment says the kernel rounds — the stored result to its storage type; for the
flash-attention backward also P and dS before the second products (and O, where the stored forward output is not given) — which gives
``emul``; ``floor_err = emul - ref64``.  ``*_abs`` entries are the same formula with every summand replaced by its absolute value (the
condition-number scale A of check_sliced; the sum|summands| of check_fp32_sum).
"""
import math

import torch

F64 = torch.float64


def bf(t):
    """round to bf16, keep the dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------------ flash attention backward
def attn_bwd_head(q, k, v, d_o, scale, dtype=F64, emulate=False, drop_dq=None, pad_score0=0, o=None):
    """one head: q, k, v, d_o [N, 64] -> dict(dq, dk, dv) in ``dtype``; emulate=False adds "abs" (dict of the three abs-valued
    results), emulate="both" returns (exact dict with "abs", emulated dict) from one evaluation of S, P and dP.
    o [N, 64]: the stored forward output the kernel is given (an operand: D = rowsum(dO o O) is taken from it, in the reference
    too); default: P V, exact in the reference and rounded to bf16 in the emulation.
    drop_dq = (q0, k0): the dq launch loses keys k0 .. k0 + 31 for the owner tile of queries q0 .. q0 + 127 (a planted defect).
    pad_score0 = P: P padded keys (K = V = 0) take part in the softmax with score 0 instead of being masked (a planted defect)."""
    q, k, v, d_o = (t.to(dtype) for t in (q, k, v, d_o))
    s = q @ k.t() * scale
    if pad_score0:
        m = torch.maximum(s.max(dim=-1, keepdim=True).values, torch.zeros((), dtype=dtype))
        e = torch.exp(s - m)
        p = e / (e.sum(dim=-1, keepdim=True) + pad_score0 * torch.exp(-m))
    else:
        p = torch.softmax(s, dim=-1)
    del s
    o_given = o is not None
    o = o.to(dtype) if o_given else p @ v
    dp = d_o @ v.t()

    def finish(emul):
        dsum = (d_o * (bf(o) if emul and not o_given else o)).sum(dim=-1, keepdim=True)
        ds = p * (dp - dsum)
        pm, dsm = (bf(p), bf(ds)) if emul else (p, ds)
        dq = dsm @ k
        if drop_dq is not None:
            q0, k0 = drop_dq
            dq[q0:q0 + 128] -= dsm[q0:q0 + 128, k0:k0 + 32] @ k[k0:k0 + 32]
        out = {"dq": dq * scale, "dk": dsm.t() @ q * scale, "dv": pm.t() @ d_o}
        if emul:
            return {n: bf(t) for n, t in out.items()}
        ads = p * (dp.abs() + dsum.abs())
        out["abs"] = {"dq": ads @ k.abs() * scale, "dk": ads.t() @ q.abs() * scale, "dv": p.t() @ d_o.abs()}
        return out
    if emulate == "both":
        return finish(False), finish(True)
    return finish(bool(emulate))


def attn_bwd(qkv, d_o, heads, scale, dtype=F64, emulate=False, o=None, **defect):
    """qkv [B, N, 3 C], d_o [B, N, C] (C = heads * 64) -> d(qkv) [B, N, 3 C] in ``dtype``; emulate=False: (d(qkv), abs scales
    {dq, dk, dv: rms over the tensor}); emulate="both": (exact, emulated, abs scales)"""
    B, N, C3 = qkv.shape
    C = C3 // 3
    outs = [torch.empty((B, N, C3), dtype=dtype) for _ in range(2 if emulate == "both" else 1)]
    sq = {"dq": 0.0, "dk": 0.0, "dv": 0.0}
    for b in range(B):
        for h in range(heads):
            c = slice(h * 64, (h + 1) * 64)
            r = attn_bwd_head(qkv[b, :, :C][:, c], qkv[b, :, C:2 * C][:, c], qkv[b, :, 2 * C:][:, c], d_o[b][:, c], scale, dtype, emulate,
                              o=None if o is None else o[b][:, c], **defect)
            for out, rr in zip(outs, r if emulate == "both" else (r,)):
                for i, nm in enumerate(("dq", "dk", "dv")):
                    out[b, :, i * C + h * 64:i * C + (h + 1) * 64] = rr[nm]
                    if "abs" in rr:
                        sq[nm] += float(rr["abs"][nm].double().pow(2).sum())
    scales = {nm: math.sqrt(val / (B * N * C)) for nm, val in sq.items()}
    if emulate == "both":
        return outs[0], outs[1], scales
    return outs[0] if emulate else (outs[0], scales)


def attn_ref_emul(qkv, d_o, heads, scale, o=None):
    """(ref64, floor_err, abs scales) of the flash-attention backward (o [B, N, C]: the stored forward output, if the kernel is given one)"""
    ref, emul, scales = attn_bwd(qkv, d_o, heads, scale, emulate="both", o=o)
    return ref, emul - ref, scales


# ------------------------------------------------------------------------------------------------ text cross-attention backward
def xattn_bwd(q, kv, d_p, d_o, heads, scale, dtype=F64, emulate=False, probs=None):
    """q [B, N, C], kv [B, L, 2 C], d_p [B * heads, N, L] or None, d_o [B, N, C] or None -> dict(dq [B, N, C], dk, dv [B, L, C]
    [, abs]).  ``probs`` [B * heads, N, L]: the stored fp32 probabilities the kernels read (default: recomputed in ``dtype``)."""
    B, N, C = q.shape
    L = kv.shape[1]
    q, kv = q.to(dtype), kv.to(dtype)
    qh = q.reshape(B, N, heads, 64).permute(0, 2, 1, 3)
    kh = kv[..., :C].reshape(B, L, heads, 64).permute(0, 2, 1, 3)
    vh = kv[..., C:].reshape(B, L, heads, 64).permute(0, 2, 1, 3)
    if probs is None:
        sim = qh @ kh.transpose(-1, -2) * scale
        p = sim.softmax(dim=-1) if L > 1 else sim.sigmoid()
    else:
        p = probs.to(dtype).reshape(B, heads, N, L)
    g = torch.zeros((B, heads, N, L), dtype=dtype)
    ga = torch.zeros((B, heads, N, L), dtype=dtype)
    if d_p is not None:
        g = g + d_p.to(dtype).reshape(B, heads, N, L)
        ga = ga + d_p.to(dtype).abs().reshape(B, heads, N, L)
    doh = None
    if d_o is not None:
        doh = d_o.to(dtype).reshape(B, N, heads, 64).permute(0, 2, 1, 3)
        g = g + doh @ vh.transpose(-1, -2)
        ga = ga + doh.abs() @ vh.abs().transpose(-1, -2)
    if L > 1:
        ds = p * (g - (p * g).sum(dim=-1, keepdim=True)) * scale
        dsa = p * (ga + (p * ga).sum(dim=-1, keepdim=True)) * scale
    else:
        ds = p * (1 - p) * g * scale
        dsa = p * (1 - p) * ga * scale
    back = lambda t, n: t.permute(0, 2, 1, 3).reshape(B, n, C)
    out = {"dq": back(ds @ kh, N), "dk": back(ds.transpose(-1, -2) @ qh, L),
           "dv": back(p.transpose(-1, -2) @ doh, L) if doh is not None else torch.zeros((B, L, C), dtype=dtype)}
    if emulate:
        return {n: bf(t) for n, t in out.items()}
    out["abs"] = {"dq": rms(back(dsa @ kh.abs(), N)), "dk": rms(back(dsa.transpose(-1, -2) @ qh.abs(), L)),
                  "dv": rms(back(p.transpose(-1, -2) @ doh.abs(), L)) if doh is not None else 0.0}
    return out


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_bwd(x, dy, gamma, eps, add=None, dtype=F64, emulate=False):
    """dx [rows, C] (+ add); not emulate: (dx, abs scale)"""
    x, dy, gamma = x.to(dtype), dy.to(dtype), gamma.to(dtype)
    mean = x.mean(dim=-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(dim=-1, keepdim=True) + eps).rsqrt()
    xh = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(dim=-1, keepdim=True) - xh * (g * xh).mean(dim=-1, keepdim=True))
    if add is not None:
        dx = dx + add.to(dtype)
    if emulate:
        return bf(dx)
    a = rstd * (g.abs() + g.abs().mean(dim=-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(dim=-1, keepdim=True))
    if add is not None:
        a = a + add.to(dtype).abs()
    return dx, rms(a)


def ln_param_grad(x, dy, eps, dtype=F64, last_row=True):
    """(d gamma, d beta) [C] and their sum|summands| (x - mean counts as two summands: it cancels)"""
    x, dy = x.to(dtype), dy.to(dtype)
    mean = x.mean(dim=-1, keepdim=True)
    rstd = ((x - mean).pow(2).mean(dim=-1, keepdim=True) + eps).rsqrt()
    n = x.shape[0] if last_row else x.shape[0] - 1
    dg = (dy * (x - mean) * rstd)[:n].sum(dim=0)
    db = dy[:n].sum(dim=0)
    return dg, db, (dy.abs() * (x.abs() + mean.abs()) * rstd).sum(dim=0), dy.abs().sum(dim=0)


# ------------------------------------------------------------------------------------------------ GroupNorm (+ SiLU)
def gn_bwd(x, dy, gamma, beta, groups, eps, silu, add=None, dtype=F64, emulate=False):
    """x, dy [B, HW, C] channel-last -> dx [B, HW, C] (+ add); not emulate: (dx, abs scale)"""
    B, HW, C = x.shape
    cpg = C // groups
    x, dy, gamma, beta = x.to(dtype), dy.to(dtype), gamma.to(dtype), beta.to(dtype)
    xg = x.reshape(B, HW, groups, cpg)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    rstd = ((xg - mean).pow(2).mean(dim=(1, 3), keepdim=True) + eps).rsqrt()
    xh = (xg - mean) * rstd
    ga, be = gamma.reshape(1, 1, groups, cpg), beta.reshape(1, 1, groups, cpg)
    dz = dy.reshape(B, HW, groups, cpg)
    if silu:
        y0 = xh * ga + be
        sg = torch.sigmoid(y0)
        dz = dz * sg * (1 + y0 * (1 - sg))
    t = dz * ga
    dx = (rstd * (t - t.mean(dim=(1, 3), keepdim=True) - xh * (t * xh).mean(dim=(1, 3), keepdim=True))).reshape(B, HW, C)
    if add is not None:
        dx = dx + add.to(dtype)
    if emulate:
        return bf(dx)
    a = (rstd * (t.abs() + t.abs().mean(dim=(1, 3), keepdim=True) + xh.abs() * (t * xh).abs().mean(dim=(1, 3), keepdim=True)))
    a = a.reshape(B, HW, C)
    if add is not None:
        a = a + add.to(dtype).abs()
    return dx, rms(a)


# ------------------------------------------------------------------------------------------------ GEGLU, 2x2 sums
def geglu(ag, dy, dtype=F64, emulate=False):
    """ag [rows, 2 inner] = [x | gate], dy [rows, inner] -> (forward [rows, inner], backward [rows, 2 inner])"""
    ag, dy = ag.to(dtype), dy.to(dtype)
    a, gt = ag.chunk(2, dim=-1)
    cdf = 0.5 * (1 + torch.erf(gt / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * gt * gt) / math.sqrt(2.0 * math.pi)
    fwd = a * gt * cdf
    bwd = torch.cat((dy * gt * cdf, dy * a * (cdf + gt * pdf)), dim=-1)
    return (bf(fwd), bf(bwd)) if emulate else (fwd, bwd)


def sum2x2(dy, dtype=F64, emulate=False):
    """dy [B, 2H, 2W, C] -> [B, H, W, C]; not emulate: (sum, abs scale)"""
    B, H2, W2, C = dy.shape
    d = dy.to(dtype).reshape(B, H2 // 2, 2, W2 // 2, 2, C)
    s = d.sum(dim=(2, 4))
    return bf(s) if emulate else (s, rms(d.abs().sum(dim=(2, 4))))


# ------------------------------------------------------------------------------------------------ fp32 sums
def wgrad(dy, x, dtype=F64, last_row=True):
    """dW [N, K] = dy^T x and sum|summands|"""
    n = dy.shape[0] if last_row else dy.shape[0] - 1
    return dy[:n].to(dtype).t() @ x[:n].to(dtype), dy.to(dtype).abs().t() @ x.to(dtype).abs()


def colsum(x, dtype=F64, last_row=True):
    n = x.shape[0] if last_row else x.shape[0] - 1
    return x[:n].to(dtype).sum(dim=0), x.to(dtype).abs().sum(dim=0)


# ------------------------------------------------------------------------------------------------ AdamW, loss seeds
def adamw(p, g, m, v, step, lr, betas, eps, wd, grad_scale, dtype=F64):
    """torch.optim.AdamW's update restated: -> (p, m, v)"""
    p, g, m, v = (t.to(dtype) for t in (p, g, m, v))
    b1, b2 = betas
    g = g * grad_scale
    p = p * (1 - lr * wd)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** step)) * m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    return p, m, v


def precond_loss_grad(f, noised, target, c_skip, c_out, w, dtype=F64, emulate=False):
    """f [B, h, w, 4] NHWC, noised / target [B, 4, h, w], per-sample c_skip, c_out, w [B] -> (loss [B], d (mean_b loss_b) / d f
    [B, h, w, 4]); not emulate: also the seed's abs scale.  The eps-prediction loss is c_skip = 1, c_out = -sigma, w = sigma^-2."""
    f, noised, target, cs, co, w = (t.to(dtype) for t in (f, noised, target, c_skip, c_out, w))
    B = f.shape[0]
    e = lambda t: t.reshape(B, 1, 1, 1)
    fn, tg = noised.permute(0, 2, 3, 1), target.permute(0, 2, 3, 1)
    out = e(cs) * fn + e(co) * f
    r = out - tg
    loss = (e(w) * r * r).reshape(B, -1).mean(dim=1)
    gs = e(co) * 2 * e(w) / (B * r[0].numel())
    seed = gs * r
    if emulate:
        return loss, bf(seed)
    return loss, seed, rms(gs.abs() * ((e(cs) * fn).abs() + (e(co) * f).abs() + tg.abs()))
