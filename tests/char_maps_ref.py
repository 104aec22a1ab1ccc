"""float64 restatements of the two character-map kernels (a helper, not a test): tests/test_char_maps_cpu.py shows them equal to the
reference's own reductions, tests/test_char_maps_gpu.py holds the kernels to them.

* ``tattn_maps`` — udt_tattn_fused_maps' map output, from the operands of the launch (the tables udt_tattn_prepare produced, row-major:
  attention_ref.tattn_unpack).  The probabilities are attention_ref.tattn_fused's P (the same four lines); the header's ROUNDING
  paragraph: "each probability is the bf16 value the output GEMM of the kernel reads (the fp32 softmax rounded to bf16 once ...); the
  heads are added in ascending order in fp32; the sum is multiplied by fp32(weight / heads)" — ``emulate`` rounds P to bf16 and nothing
  else (the fp32 additions are what the checker's 2^-18 A allowance is for).
* ``bilinear`` — udt_resize_bilinear_f32 with exact rational taps and weights, and the sum of the absolute summands.
"""
import torch

import attention_ref as R

F64 = torch.float64


def tattn_probs(x, A, sc, eps, dtype=F64):
    """attention_ref.tattn_fused's P: x [B, N, C], A [B, hp, C] row-major, sc [B, hp, 2] -> (P [B, N, hp / 16, 16], Sabs [B, N, hp])
    with Sabs_j = rstd sum_k |x_k A'_kj| + rstd |mean s_j| + |c_j|, the absolute summands of the score"""
    B, N, C = x.shape
    hp = A.shape[1]
    x, A, sc = (t.to(dtype) for t in (x, A, sc))
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x * x).mean(dim=-1, keepdim=True) - mean * mean).clamp_min(0)
    rstd = (var + eps).rsqrt()
    S = rstd * (x @ A.transpose(1, 2) - mean * sc[:, None, :, 0]) + sc[:, None, :, 1]
    P = S.reshape(B, N, hp // 16, 16).softmax(dim=-1)
    Sabs = rstd * (x.abs() @ A.abs().transpose(1, 2)) + rstd * (mean * sc[:, None, :, 0]).abs() + sc[:, None, :, 1].abs()
    return P, Sabs


def tattn_maps(x, A, sc, heads, L, map_from, eps, weight=1.0, emulate=False):
    """-> maps [B - map_from, L, N] float64 = weight / heads * sum_h P[b, t, h, l]; emulate=False also returns, element by element,
    mean_h P_hl (1 + 2 max_j Sabs_hj) over the real columns j < L of head h — the softmax's sensitivity to its scores' fp32 rounding;
    its RMS (``rms``) is the checker's abs scale"""
    P, Sabs = tattn_probs(x, A, sc, eps)
    B, N = x.shape[:2]
    P = P[map_from:, :, :heads, :L]                                         # [b, N, heads, L]
    m = (R.bf(P) if emulate else P).sum(dim=2) * (weight / heads)
    m = m.permute(0, 2, 1).contiguous()                                     # [b, L, N]
    if emulate:
        return m
    smax = Sabs.reshape(B, N, -1, 16)[map_from:, :, :heads, :L].amax(dim=-1, keepdim=True)      # [b, N, heads, 1]
    a = (P * (1 + 2 * smax)).sum(dim=2) * (abs(weight) / heads)
    return m, a.permute(0, 2, 1).contiguous()


def rms(t):
    return float(t.pow(2).mean().sqrt()) if t.numel() else 0.0


def reference_reduction(layer_probs, heads):
    """the reference's own reduction (openaimodel.py:559-591) of full probabilities, one [b * heads, n, l] tensor per layer:
    stack -> mean -> reshape (-1, heads, n, l) -> mean over heads -> permute -> [b, l, n]"""
    m = torch.stack(list(layer_probs), dim=0).mean(dim=0)
    _, n, l = m.shape
    return m.reshape(-1, heads, n, l).mean(dim=1).permute(0, 2, 1)


def _taps(n_in, n_out):
    """-> (i0, i1 int64 [n_out], w1 float64 [n_out]) of the half-pixel rule, from integers: source coordinate
    max(0, (2 i + 1) n_in - n_out) / (2 n_out)"""
    i = torch.arange(n_out, dtype=torch.int64)
    den = 2 * n_out
    num = ((2 * i + 1) * n_in - n_out).clamp_min(0)
    q, r = num // den, num % den
    i0 = q.clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    return i0, i1, r.to(F64) / den


def bilinear(x, H, W):
    """x [..., h, w] -> (out, abs_sum) float64 [..., H, W]: bilinear, half-pixel centres, edge clamp, no antialiasing"""
    x = x.to(F64)
    h, w = x.shape[-2:]
    y0, y1, wy = _taps(h, H)
    x0, x1, wx = _taps(w, W)
    wy, wx = wy.to(x.device).reshape(H, 1), wx.to(x.device).reshape(1, W)

    def mix(t):
        r0, r1 = t[..., y0, :], t[..., y1, :]
        top = (1 - wx) * r0[..., x0] + wx * r0[..., x1]
        bot = (1 - wx) * r1[..., x0] + wx * r1[..., x1]
        return (1 - wy) * top + wy * bot
    return mix(x), mix(x.abs())
