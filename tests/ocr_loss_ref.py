"""float64 references for the OCR loss and its reverse pass (a helper, not a test; CPU and device tensors).

  mattn_bwd_ref        udt_mattn_bwd written out (dS = P (dP - delta)), pinned against torch.autograd by tests/test_ocr_loss_cpu.py;
  mattn_bwd_emul       the same rounded where the header says the kernel rounds: the stored dq / dk / dv, to bf16, once
  ce_ref               udt_ocr_ce_f32: clamped character cross entropy, its seed, and the softmax the bound is stated in
  crop_resize_bwd_ref  the adjoint of udt_crop_resize_aa_f32 from crop_resize_ref.tables (the transposed matrices: the tap rule is
                       not restated) with the forward's bound, transposed
  vjp_ref              encoder -> one teacher-forced refinement pass -> head under a FIXED cotangent of the logits
  chain_ref            encoder -> one teacher-forced refinement pass -> head -> clamped cross entropy, composed from oracle.parseq
                       under torch.autograd, in any dtype (float64: the reference; bfloat16: the "bf16 twin" whose error bounds the
                       kernels' — a measurement taken from the reference alone)
  fixture              the shared inputs of the CPU and GPU tests; no GPU value enters it
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

import crop_resize_ref as R

N_CLS = 95
SHARPEN = 16.0          # head.weight, head.bias multiplier: with the synthetic weights as they are every row clamps (CE ~ 3 > 1)
CROP_SIZES = [(40, 150), (64, 200), (17, 33), (128, 384), (32, 128), (9, 301)]
WRONG_ROW, WRONG_LABEL = 1, "ZZ~"


# ------------------------------------------------------------------------------------------------ masked attention
def _heads(t, heads):
    B, n, C = t.shape
    return t.double().reshape(B, n, heads, C // heads).transpose(1, 2)           # [B, H, n, D]


def _probs(q, k, mask, kpm, scale):
    s = q @ k.transpose(-2, -1) * scale
    if mask is not None:
        s = s + mask.double().to(s.device)
    if kpm is not None:
        s = s.masked_fill(kpm.bool().to(s.device)[:, None, None, :], float("-inf"))
    mx = s.max(-1, keepdim=True).values
    e = torch.where(torch.isinf(s) & (s < 0), torch.zeros_like(s), torch.exp(s - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)))
    den = e.sum(-1, keepdim=True)
    return torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))    # a fully masked query: zeros, as the kernels


def mattn_fwd_ref(q, k, v, mask, kpm, scale, heads):
    P = _probs(_heads(q, heads), _heads(k, heads), mask, kpm, scale)
    o = P @ _heads(v, heads)
    return o.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)


def mattn_bwd_ref(q, k, v, d_o, mask, kpm, scale, heads):
    """q, d_o [B, nq, heads*D], k, v [B, lk, heads*D] -> (dq, dk, dv) float64, same layouts"""
    qh, kh, vh, gh = (_heads(t, heads) for t in (q, k, v, d_o))
    P = _probs(qh, kh, mask, kpm, scale)
    dP = gh @ vh.transpose(-2, -1)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    back = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)
    return back(dS @ kh * scale), back(dS.transpose(-2, -1) @ qh * scale), back(P.transpose(-2, -1) @ gh)


def mattn_bwd_abs(q, k, v, d_o, mask, kpm, scale, heads):
    """the same formulas with every summand replaced by its absolute value: the condition-number scale of check_sliced"""
    qh, kh, vh, gh = (_heads(t, heads) for t in (q, k, v, d_o))
    P = _probs(qh, kh, mask, kpm, scale)
    dPa = gh.abs() @ vh.abs().transpose(-2, -1)
    dSa = P * (dPa + (P * dPa).sum(-1, keepdim=True))
    back = lambda t: t.transpose(1, 2).reshape(t.shape[0], t.shape[2], -1)
    return back(dSa @ kh.abs() * scale), back(dSa.transpose(-2, -1) @ qh.abs() * scale), back(P.transpose(-2, -1) @ gh.abs())


def bf16_round(t):
    return t.float().bfloat16().double()


def mattn_bwd_emul(q, k, v, d_o, mask, kpm, scale, heads):
    """include/udt_kernels.h, udt_mattn_bwd, ROUNDING: only the stored dq, dk, dv are rounded (bf16, once)"""
    return tuple(bf16_round(t) for t in mattn_bwd_ref(q, k, v, d_o, mask, kpm, scale, heads))


# ------------------------------------------------------------------------------------------------ cross entropy
def ce_ref(logits, targets, n_chars, weight=None):
    """logits [N, L, C], targets int [N, T], n_chars int [N], weight [N] or None ->
    dict(loss [N] clamped, raw [N] unclamped, d_logits [N, L, C], softmax [N, L, C], onehot [N, L, C], lse_abs [N]) in float64"""
    x = logits.double().cpu()
    N, L, C = x.shape
    tg, nc = targets.cpu().long(), n_chars.cpu().long()
    w = torch.ones(N, dtype=torch.float64) if weight is None else weight.double().cpu()
    sm = torch.softmax(x, -1)
    lse = torch.logsumexp(x, -1)
    onehot = torch.zeros_like(x)
    raw = torch.zeros(N, dtype=torch.float64)
    lse_abs = torch.zeros(N, dtype=torch.float64)
    d = torch.zeros_like(x)
    for b in range(N):
        n = int(nc[b])
        t = torch.arange(n)
        onehot[b, t, tg[b, :n]] = 1.0
        picked = x[b, t, tg[b, :n]]
        raw[b] = (lse[b, :n] - picked).mean()
        lse_abs[b] = (lse[b, :n].abs() + picked.abs()).mean()
        if bool(raw[b] <= 1.0):
            d[b, :n] = w[b] * (sm[b, :n] - onehot[b, :n]) / n
    return {"loss": raw.clamp(max=1.0), "raw": raw, "d_logits": d, "softmax": sm, "onehot": onehot, "lse_abs": lse_abs}


# ------------------------------------------------------------------------------------------------ crop + resize, adjoint
def crop_resize_bwd_ref(d_out, boxes, img_shape, mul=1.0):
    """d_out [N, C, oh, ow], boxes [N, 5] (one per image at most) -> (d_img float64 [B, C, H, W], bound float64 [B, 1, H, W]):
    d_img[box] = mul * Wy^T d_out Wx with crop_resize_ref's tables; the bound is crop_resize_ref.crop_resize's, transposed — K and S
    are now the largest tap count and absolute sum of a COLUMN of the same tables (the outputs one input sample feeds):
        |got - ref| <= (Ky + Kx + 16) 2^-23 Sy Sx max|d_out[n]| |mul|        inside box n, and exactly 0 outside every box"""
    B, C, H, W = img_shape
    d = d_out.double().cpu()
    oh, ow = d.shape[-2:]
    d_img = torch.zeros((B, C, H, W), dtype=torch.float64)
    bound = torch.zeros((B, 1, H, W), dtype=torch.float64)
    for n, (i, t, b, l, r) in enumerate(torch.as_tensor(boxes).reshape(-1, 5).tolist()):
        Wy, _, _ = R.tables(b - t, oh)
        Wx, _, _ = R.tables(r - l, ow)
        d_img[i, :, t:b, l:r] = mul * (Wy.T @ d[n] @ Wx)
        Ky, Kx = int((Wy != 0).sum(0).max()), int((Wx != 0).sum(0).max())
        Sy, Sx = float(Wy.abs().sum(0).max()), float(Wx.abs().sum(0).max())
        bound[i, :, t:b, l:r] = (Ky + Kx + 16) * 2.0 ** -23 * Sy * Sx * float(d[n].abs().max()) * abs(mul)
    return d_img, bound


# ------------------------------------------------------------------------------------------------ the chain
def refine_masks(L, dtype=torch.float32):
    tgt_mask = torch.triu(torch.full((L, L), float("-inf"), dtype=dtype), 1)
    query_mask = tgt_mask.clone()
    query_mask[torch.triu(torch.ones(L, L, dtype=torch.bool), 2)] = 0
    return tgt_mask, query_mask


def refine_logits(sd, x, tgt_in):
    """encoder + one teacher-forced refinement pass + head, oracle.parseq's functions in the dtype of sd / x"""
    from oracle import parseq as OP
    L = tgt_in.shape[1]
    tgt_mask, query_mask = refine_masks(L, x.dtype)
    kpm = (tgt_in == OP.Tokenizer().eos_id).int().cumsum(-1) > 0
    memory = OP.vit_encode(sd, x)
    pos_q = sd["pos_queries"][:, :L].expand(x.shape[0], -1, -1)
    out = OP.decode(sd, tgt_in, memory, tgt_mask, kpm, tgt_query=pos_q, tgt_query_mask=query_mask)
    return F.linear(out, sd["head.weight"], sd["head.bias"])


def chain_ref(sd, x, tgt_in, labels, dtype=torch.float64, weight=None):
    """-> (unclamped CE [N], d sum_b w_b min(1, CE_b) / d x [N, 3, h, w]) under torch.autograd, every tensor in ``dtype``;
    returned as float64"""
    from oracle import parseq as OP
    sd = {k: v.to(dtype) for k, v in sd.items()}
    gt = OP.Tokenizer().encode(labels)
    with torch.enable_grad():
        xg = x.detach().cpu().to(dtype).requires_grad_(True)
        logits = refine_logits(sd, xg, tgt_in.cpu())
        raw = torch.stack([F.cross_entropy(logits[b, :len(y)], gt[b, 1:len(y) + 1]) for b, y in enumerate(labels)])
        w = torch.ones_like(raw) if weight is None else torch.as_tensor(weight).to(dtype).expand_as(raw)
        (d_x,) = torch.autograd.grad((w * raw.clamp(max=1.0)).sum(), [xg])
    return raw.detach().double(), d_x.double()


def vjp_ref(sd, x, tgt_in, cotangent, dtype=torch.float64):
    """d <refine_logits(x), cotangent> / d x under torch.autograd, every tensor in ``dtype`` -> (logits, d_x) as float64: the tape's
    reverse pass without the cross entropy in front of it (whose softmax turns a logit error into a relative gradient error)"""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    with torch.enable_grad():
        xg = x.detach().cpu().to(dtype).requires_grad_(True)
        logits = refine_logits(sd, xg, tgt_in.cpu())
        (d_x,) = torch.autograd.grad((logits * cotangent.cpu().to(dtype)).sum(), [xg])
    return logits.detach().double(), d_x.double()


def rel_rms(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ the fixture
def synthetic_weights():
    from udifftext_amd import synth
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "parseq_golden.npz"))
    keys, shapes = list(G["state_dict_keys"]), [eval(s) for s in G["state_dict_shapes"]]
    return {k: synth.synthetic_tensor("parseq." + k, sh) for k, sh in zip(keys, shapes)}


def sharpened_weights():
    """the synthetic PARSeq weights with the head multiplied by SHARPEN (fp32)"""
    sd = synthetic_weights()
    sd["head.weight"] = sd["head.weight"] * SHARPEN
    sd["head.bias"] = sd["head.bias"] * SHARPEN
    return sd


E2E_SEED = 2            # the first seed >= 2 whose crops keep every unclamped float64 CE in [0.02, 0.22] under the oracle's tokens


def e2e_crops():
    """the crops of the end-to-end test (sizes CROP_SIZES): more confident rows than the chain fixture's, so that the forward's bf16
    error, which the sharpened head multiplies by 16, stays inside the 3e-2 the losses are held to"""
    g = torch.Generator().manual_seed(E2E_SEED)
    return [torch.rand((3, h, w), generator=g) for h, w in CROP_SIZES]


def oracle_reading(sd, crops):
    """-> (x, tgt_in, labels, raw64): the oracle's own AR tokens, the first 6 characters it reads (row WRONG_ROW gets WRONG_LABEL)"""
    from oracle import parseq as OP
    tok = OP.Tokenizer()
    with torch.no_grad():
        x = OP.predictor_transform(crops)
        ar = OP.parseq_forward(sd, x, refine_iters=0)
        tgt_in = torch.cat([torch.full((len(crops), 1), tok.bos_id, dtype=torch.long), ar[:, :-1].argmax(-1)], dim=1)
        labels = [(y[:6] or "a") for y in tok.decode(refine_logits(sd, x, tgt_in).softmax(-1))[0]]
    labels[WRONG_ROW] = WRONG_LABEL
    raw64, _ = chain_ref(sd, x, tgt_in, labels, torch.float64)
    return x, tgt_in, labels, raw64


def jitter(x, k):
    """draw k of an input for the bf16 twin: x itself for k = 0, else x (1 + 1e-6 n), n ~ N(0, 1) seeded by k — far below bf16's
    resolution, yet every rounding of the twin falls differently"""
    if k == 0:
        return x
    return x * (1 + 1e-6 * torch.randn(x.shape, generator=torch.Generator().manual_seed(k), dtype=torch.float64).to(x.dtype))


_FIXTURE = {}


def fixture():
    """dict(sd, crops, x [6, 3, 32, 128], tgt_in [6, L], labels, raw64 [6], d_x64, raw_twin, d_x_twin) — computed once per process"""
    if _FIXTURE:
        return _FIXTURE
    from oracle import parseq as OP
    sd = sharpened_weights()
    torch.manual_seed(1)
    crops = [torch.rand(3, h, w) for h, w in CROP_SIZES]
    with torch.no_grad():
        x = OP.predictor_transform(crops)
        tok = OP.Tokenizer()
        ar = OP.parseq_forward(sd, x, refine_iters=0)                        # the oracle's own AR pass
        tgt_in = torch.cat([torch.full((len(crops), 1), tok.bos_id, dtype=torch.long), ar[:, :-1].argmax(-1)], dim=1)
        refined = refine_logits(sd, x, tgt_in)
        labels = [y[:6] for y in tok.decode(refined.softmax(-1))[0]]
    labels[WRONG_ROW] = WRONG_LABEL
    raw64, d_x64 = chain_ref(sd, x, tgt_in, labels, torch.float64)
    raw_twin, d_x_twin = chain_ref(sd, x, tgt_in, labels, torch.bfloat16)
    _FIXTURE.update(sd=sd, crops=crops, x=x, tgt_in=tgt_in, labels=labels, raw64=raw64, d_x64=d_x64, raw_twin=raw_twin,
                    d_x_twin=d_x_twin)
    return _FIXTURE


def load_predictor(sd, device):
    import udifftext_amd  # noqa: F401
    from sgm.modules.predictors.model import ParseqPredictor
    from sgm.util import skip_param_init
    with skip_param_init():
        m = ParseqPredictor(ckpt_path=None)
    missing, unexpected = m.parseq.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return m.to(device).eval()
