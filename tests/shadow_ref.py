"""Op-level float64 shadow of ``udifftext_amd.ops`` (test helper, like mx8_ref.py — not a conftest).

Inside ``with Shadow(...) as sh:`` every function of ``udifftext_amd.ops`` that the model code calls is replaced by a wrapper.
The model modules call them as ``ops.<fn>(...)``, so patching the module attributes reaches every call site.  For each call the
wrapper clones the tensor arguments (``out=`` may alias ``x`` / ``residual``; some ops work in place), runs the HIP op,
synchronises, and computes a float64 reference FROM THE CLONES — the op's own inputs, exactly as the HIP path produced them
(teacher forcing: error cannot build up from one op to the next, so every launch is held to its own per-op bound).  Side outputs
are checked too: GroupNorm column statistics, MX8 twins, row statistics, the probabilities of ``xattention``.

Only the outermost ``ops`` call is checked (ops functions call each other through module globals).  Host-only helpers pass
through (PASSTHROUGH); any other ops function without a reference is recorded as a failure that names it.

The reference functions (``ref_*``) are plain torch and device-agnostic: tests/test_shadow_ref_cpu.py pins them on the CPU
against independent torch compositions.

Bounds, per op class (CLASSES), all taken from the op's existing unit test (the fp32 class's k: from a float32 restatement):
  * per element, scaled to the tensor: |got - ref| <= rtol * |ref| + atol * RMS(ref);
  * localisation: every 32-row x 32-column block of the output has RMS(err) <= k * max(RMS(ref_block), 0.1 * RMS(ref)), so
    one wrong tile fails although the global error is small; k per class, from measurement (see CLASSES).
"""
from __future__ import annotations

import inspect
import math
import os
from collections import defaultdict
from typing import Optional

import torch
import torch.nn.functional as F

import mx8_ref

F64 = torch.float64

# ------------------------------------------------------------------------------------------------ bounds per op class
# rtol / atol: tests/test_ops_gpu.py _close (RTOL 1.5e-2, ATOL_BF16 2e-2 on unit-RMS operands; 3e-2 for the fused GroupNorm
# convolution and the fused text attention), test_lean_gpu.py, test_mx8_gpu.py (same quantised operands).  k: the localisation
# factor, about 3x the worst block ratio measured on the MI355X over the five production calls (the parity report lists both):
# bf16-output ops 2.6e-3 (bf16 rounding of the output: 2^-9 rms relative), the e4m3 attention 1.8e-2, the fp32 xattn probabilities
# 1.6e-7.  conv+gn, gn-table and softmax are not on the shipped path (UDT_FUSE_GN is off; the VAE runs attention_d512): their k
# is the bf16 one.
# f32 (posterior_sample, mask_downsample: fp32 in, fp32 out): rtol / atol from tests/test_ops_gpu.py test_layout_and_misc (rtol 1e-5;
# atol 1e-5 for the posterior sample, 1e-6 for the mask: the class takes the tighter one, scaled by RMS(ref) like every class).  Its k is
# NOT taken from the kernel: tests/test_shadow_ref_cpu.py test_f32_class_localisation_factor measures the worst 32 x 32 block ratio of a
# float32 torch restatement of both ops against the float64 references at the shapes the shadow runs produce (moments [4, 64, 64, 8],
# [1, 32, 48, 8], [2, 32, 48, 8]; masks [4, 1, 512, 512], [2, 1, 256, 384]): 1.16e-7 for the posterior sample (0 for the mask: four binary
# pixels times 0.25 is exact), times 8 for another operation order and a fast exp -> k = 9.3e-7.  A wrong tile is off by ~1.
CLASSES = {
    # name             rtol    atol    k
    "gemm":           (1.5e-2, 2e-2, 8e-3),
    "conv":           (1.5e-2, 2e-2, 8e-3),
    "conv+gn":        (1.5e-2, 3e-2, 8e-3),
    "gemm-mx8":       (1.5e-2, 2e-2, 8e-3),
    "attn":           (1.5e-2, 2e-2, 8e-3),
    "attn-mx8":       (1.5e-2, 1e-1, 5.5e-2),
    "xattn":          (1.5e-2, 2e-2, 8e-3),
    "xattn-probs":    (1e-3, 1e-4, 1e-6),
    "tattn":          (1.5e-2, 3e-2, 8e-3),
    "norm":           (1.5e-2, 2e-2, 8e-3),
    "gn-table":       (2e-3, 2e-3, 8e-3),
    "softmax":        (1.5e-2, 1e-3, 8e-3),
    "elementwise":    (1.5e-2, 1e-2, 8e-3),
    "f32":            (1e-5, 1e-6, 9.3e-7),
    "layout":         (0.0, 0.0, 0.0),
}
# rel-RMS bounds of the unit tests that state one (test_mx8_gpu REL_GEMM / REL_ATTN8 / REL_Q8)
REL_RMS = {"gemm-mx8": 5e-3, "attn-mx8": 3.5e-2, "q8": 4e-2}
STATS_RTOL = 2e-2                       # test_mx8_gpu._check_q8 / test_ops_gpu colstats: partial sums vs the output's own sums

PASSTHROUGH = {"mx8_of", "gn_stats_of", "gn_strip_ok", "launch_context", "count_work", "check_async_errors",
               "prof_enable", "prof_reset", "prof_get"}


def _d(t):
    return t.to(F64)


def _silu(x):
    return x * torch.sigmoid(x)


def _gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# --------------------------------------------------------------------------------------------------- reference functions
def ref_gemm_epilogue(acc, bias=None, rowvec=None, rows_per_batch=0, residual=None, flags=0, alpha=1.0):
    """acc fp64 [M, N] -> the udt_gemm epilogue: alpha * acc + bias + rowvec[row // rows_per_batch] + residual, then ReLU / SiLU;
    GEGLU: columns come in blocks of 64 = [32 value | the 32 matching gate columns] -> value * gelu_erf(gate)"""
    from udifftext_amd import lib as L
    M, N = acc.shape
    v = acc * alpha
    if bias is not None:
        v = v + _d(bias[:N])
    if rowvec is not None:
        rv = _d(rowvec[:, :N])
        v = v + rv.repeat_interleave(rows_per_batch, dim=0)[:M]
    if flags & L.GEMM_GEGLU:
        blk = v.reshape(M, N // 64, 2, 32)
        return (blk[:, :, 0] * _gelu_erf(blk[:, :, 1])).reshape(M, N // 2)
    if residual is not None:
        v = v + _d(residual)
    if flags & L.GEMM_RELU:
        v = v.clamp_min(0.0)
    if flags & L.GEMM_SILU_OUT:
        v = _silu(v)
    return v


def ref_linear(x2, w, N, **epi):
    """x2 [M, K] (the rows the op reads), w [>=N, K] -> epilogue(x2 @ w[:N]^T)"""
    K = x2.shape[1]
    return ref_gemm_epilogue(_d(x2) @ _d(w[:N, :K]).t(), **epi)


def ref_ln_linear(x2, w_folded, c, N, eps, **epi):
    """LayerNorm-folded GEMM from the original math: rstd * ((x - mean) @ Wf^T) + c, statistics of the raw rows in fp64"""
    x = _d(x2)
    mean = x.mean(dim=1, keepdim=True)
    xc = x - mean
    rstd = 1.0 / torch.sqrt((xc * xc).mean(dim=1, keepdim=True) + eps)
    acc = rstd * (xc @ _d(w_folded[:N, :x.shape[1]]).t())
    return ref_gemm_epilogue(acc, bias=c, **epi)


def mx8_weights(wq, colscale, N):
    return wq[:N].view(torch.float8_e4m3fn).to(F64) * _d(colscale[:N])[:, None]


def ref_linear_mx8(xdec, wq, colscale, N, bias=None, ln=None, **epi):
    """the MX8 GEMM on the SAME quantised operands: dequantised x (mx8_ref.decode) @ (e4m3 w * per-channel scale)^T; ln = (c, s,
    mean, rstd): LayerNorm-folded, rstd * (xq @ W'^T - mean * s) + c (mean / rstd of the rows the producer quantised)"""
    acc = _d(xdec) @ mx8_weights(wq, colscale, N).t()
    if ln is not None:
        c, s, mean, rstd = ln
        acc = rstd[:, None] * (acc - mean[:, None] * _d(s[:N])[None, :])
        return ref_gemm_epilogue(acc, bias=c, **epi)
    return ref_gemm_epilogue(acc, bias=bias, **epi)


def ref_conv2d(x, w, bias=None, *, ksize=3, stride=1, pad=None, upsample=False, x2=None, out_hw=None, residual=None, rowvec=None,
               flags=0, n_out=None, in_scsh=None, in_act=0):
    """NHWC implicit-GEMM convolution: sources concatenated on channels, optional GroupNorm scale / shift table + SiLU on the input
    (applied BEFORE zero padding: padded taps stay zero), nearest x2 upsampling, top / left padding ``pad`` and as much zero
    padding at the bottom / right as the output size ``out_hw`` needs; w [N, ksize*ksize*(C1+C2)] tap-major.  -> fp64 [B,Ho,Wo,N]"""
    from udifftext_amd import lib as L
    xin = _d(x) if x2 is None else torch.cat([_d(x), _d(x2)], dim=-1)
    B, H, W_, Ct = xin.shape
    if in_scsh is not None:
        t = _d(in_scsh).reshape(B, Ct // 64, 2, 64)
        sc = t[:, :, 0].reshape(B, 1, 1, Ct)
        sh = t[:, :, 1].reshape(B, 1, 1, Ct)
        xin = xin * sc + sh
        if in_act == 1:
            xin = _silu(xin)
    xin = xin.permute(0, 3, 1, 2)
    if upsample:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    Hv, Wv = xin.shape[2], xin.shape[3]
    if pad is None:
        pad = (ksize // 2, ksize // 2)
    if out_hw is None:
        out_hw = ((Hv + 2 * pad[0] - ksize) // stride + 1, (Wv + 2 * pad[1] - ksize) // stride + 1)
    Ho, Wo = out_hw
    pb = max(0, (Ho - 1) * stride + ksize - pad[0] - Hv)
    pr = max(0, (Wo - 1) * stride + ksize - pad[1] - Wv)
    xin = F.pad(xin, (pad[1], pr, pad[0], pb))
    N = w.shape[0] if n_out is None else n_out
    wk = _d(w[:N]).reshape(N, ksize, ksize, Ct).permute(0, 3, 1, 2)
    y = F.conv2d(xin, wk, None, stride=stride)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)
    acc = y.reshape(B * Ho * Wo, N)
    res = _d(residual).reshape(B * Ho * Wo, N) if residual is not None else None
    out = ref_gemm_epilogue(acc, bias=bias, rowvec=rowvec, rows_per_batch=Ho * Wo, residual=res,
                            flags=flags & ~(L.GEMM_CONV | L.GEMM_OUT_F32))
    return out.reshape(B, Ho, Wo, N)


def ref_group_norm(x, gamma, beta, groups, eps, silu, x2=None):
    """GroupNorm (+ SiLU) over NHWC [B, ..., C1 (+C2)], statistics of the data in fp64"""
    xin = _d(x) if x2 is None else torch.cat([_d(x), _d(x2)], dim=-1)
    B, Ct = xin.shape[0], xin.shape[-1]
    xr = xin.reshape(B, -1, groups, Ct // groups)
    mean = xr.mean(dim=(1, 3), keepdim=True)
    var = ((xr - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((xr - mean) / torch.sqrt(var + eps)).reshape(xin.shape) * _d(gamma) + _d(beta)
    return _silu(y) if silu else y


def ref_gn_table(x, gamma, beta, groups, eps, x2=None):
    """gn_finalize's table from the DATA: fp64 [B, Ct/64, 2, 64] = (gamma * rstd, beta - mean * gamma * rstd) per (sample, channel)"""
    xin = _d(x) if x2 is None else torch.cat([_d(x), _d(x2)], dim=-1)
    B, Ct = xin.shape[0], xin.shape[-1]
    xr = xin.reshape(B, -1, groups, Ct // groups)
    mean = xr.mean(dim=(1, 3))
    var = ((xr - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    cpg = Ct // groups
    sc = _d(gamma)[None, :] * rstd.repeat_interleave(cpg, dim=1)
    sh = _d(beta)[None, :] - mean.repeat_interleave(cpg, dim=1) * sc
    return torch.stack([sc.reshape(B, Ct // 64, 64), sh.reshape(B, Ct // 64, 64)], dim=2)


def ref_layer_norm(x, gamma, beta, eps):
    return F.layer_norm(_d(x), (x.shape[-1],), _d(gamma), _d(beta), eps)


def ref_attention(q, k, v, heads, head_dim, scale):
    """softmax(q k^T * scale) v per (sample, head): q [B, Nq, >=heads*D], k / v [B, Nk, >=heads*D] -> ([B, Nq, heads*D], probs
    [B*heads, Nq, Nk]) in fp64, one (sample, head) at a time"""
    B, Nq = q.shape[0], q.shape[1]
    Nk = k.shape[1]
    o = torch.empty((B, Nq, heads * head_dim), dtype=F64, device=q.device)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * head_dim, (h + 1) * head_dim)
            p = torch.softmax((_d(q[b, :, sl]) @ _d(k[b, :, sl]).t()) * scale, dim=-1)
            o[b, :, sl] = p @ _d(v[b, :, sl])
    return o


def ref_probs(q, k, heads, head_dim, scale):
    B, Nq = q.shape[0], q.shape[1]
    out = []
    for b in range(B):
        for h in range(heads):
            sl = slice(h * head_dim, (h + 1) * head_dim)
            out.append(torch.softmax((_d(q[b, :, sl]) @ _d(k[b, :, sl]).t()) * scale, dim=-1))
    return torch.stack(out)


def ref_tattn(x, kv, wq, wo, gamma, beta, bias, heads, scale, zero_samples, eps):
    """x + to_out(softmax(LN(x) Wq^T K^T * scale) V) + bias per sample; the first zero_samples samples see a zero context
    (k = v = 0: uniform softmax over zeros -> output 0, only the bias remains)"""
    B, N, C = x.shape
    xd = _d(x)
    out = xd + _d(bias[:C])
    for b in range(zero_samples, B):
        y = ref_layer_norm(x[b], gamma, beta, eps)
        q = y @ _d(wq[:C, :C]).t()
        o = ref_attention(q[None], kv[b:b + 1, :, :C], kv[b:b + 1, :, C:2 * C], heads, 64, scale)[0]
        out[b] = out[b] + o @ _d(wo[:C, :C]).t()
    return out


def ref_timestep_embedding(t, dim):
    half = dim // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=F64, device=t.device) / half)
    a = _d(t).reshape(-1, 1) * f[None, :]
    return torch.cat([torch.cos(a), torch.sin(a)], dim=-1)


def ref_masked_attention(q, k, v, heads, scale, mask=None, key_padding_mask=None):
    """nn.MultiheadAttention's core: per (sample, head) softmax(q k^T * scale + mask, key-padded columns -inf) v.  q [B, Nq, heads*D],
    k / v [B, Lk, >=heads*D] row views whose first heads*D columns are live; mask [Nq, Lk] additive (may hold -inf),
    key_padding_mask [B, Lk] (true = ignore) -> fp64 [B, Nq, heads*D]"""
    B, Nq, Cq = q.shape
    D = Cq // heads
    o = torch.empty((B, Nq, heads * D), dtype=F64, device=q.device)
    for b in range(B):
        for h in range(heads):
            sl = slice(h * D, (h + 1) * D)
            s = (_d(q[b, :, sl]) @ _d(k[b, :, sl]).t()) * scale
            if mask is not None:
                s = s + _d(mask)
            if key_padding_mask is not None:
                s = s.masked_fill(key_padding_mask[b].bool()[None, :], float("-inf"))
            o[b, :, sl] = torch.softmax(s, dim=-1) @ _d(v[b, :, sl])
    return o


def ref_posterior_sample(moments, noise, scale):
    """moments NHWC [B, h, w, ld >= 8] (mean in channels 0..3, logvar in 4..7, whatever ld is), noise NCHW [B, 4, h, w] ->
    scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise), fp64 NCHW [B, 4, h, w] (the reference's distributions.py clamps)"""
    m = _d(moments)
    mean = m[..., 0:4].permute(0, 3, 1, 2)
    logvar = m[..., 4:8].permute(0, 3, 1, 2).clamp(-30.0, 20.0)
    return scale * (mean + torch.exp(0.5 * logvar) * _d(noise))


def ref_mask_downsample(mask):
    """the rule udt_mask_downsample implements (csrc/elementwise.hip mask_downsample_kernel): mask [B, 1, H, W] -> [B, 1, H // 8, W // 8],
    out[oy, ox] = the mean of the four pixels (8 oy + 3 + dy, 8 ox + 3 + dx), dy, dx in {0, 1} — bilinear x 1/8 with
    align_corners False samples at 8 o + 3.5, halfway between pixels 3 and 4 of each 8 x 8 block, on both axes"""
    B, _, H, W_ = mask.shape
    h, w = H // 8, W_ // 8
    m = _d(mask)[:, :, :8 * h, :8 * w].reshape(B, 1, h, 8, w, 8)
    return 0.25 * (m[:, :, :, 3, :, 3] + m[:, :, :, 3, :, 4] + m[:, :, :, 4, :, 3] + m[:, :, :, 4, :, 4])


def ref_embed_tokens(idx, table, pe):
    """idx [n_tok] (rows of Lc = pe.shape[0] tokens each) -> table[idx] + pe[token % Lc], fp64 [n_tok, D]"""
    Lc = pe.shape[0]
    pos = torch.arange(idx.numel(), device=idx.device) % Lc
    return _d(table)[idx.long().reshape(-1)] + _d(pe)[pos]


def decode_q8(q8, n_cols, fixed=None):
    """an Mx8Act -> fp32 [M, n_cols]; fixed = (first column, multiplier): columns from there on are e4m3(v * multiplier)"""
    dec = mx8_ref.decode(q8.data[:, :n_cols].contiguous(), q8.scale)
    if fixed is not None and fixed[0] < n_cols:
        c0, mul = fixed
        dec[:, c0:] = q8.data[:, c0:n_cols].contiguous().view(torch.float8_e4m3fn).float() / mul
    return dec


# --------------------------------------------------------------------------------------------------------- the checks
def _rms(t):
    return float(t.pow(2).mean().sqrt()) if t.numel() else 0.0


def _as2d(t):
    t = t.reshape(-1, t.shape[-1]) if t.dim() >= 2 else t.reshape(1, -1)
    return t


def block_ratio(err, ref):
    """max over 32 x 32 blocks of RMS(err_block) / max(RMS(ref_block), 0.1 RMS(ref)) (partial edge blocks count as whole ones)"""
    e, r = _as2d(err), _as2d(ref)
    R, Cc = e.shape
    pr, pc = (-R) % 32, (-Cc) % 32
    cnt = torch.ones_like(e)
    if pr or pc:
        e, r, cnt = F.pad(e, (0, pc, 0, pr)), F.pad(r, (0, pc, 0, pr)), F.pad(cnt, (0, pc, 0, pr))
    def bsum(t):
        return t.reshape(e.shape[0] // 32, 32, e.shape[1] // 32, 32).sum(dim=(1, 3))
    n = bsum(cnt).clamp_min(1)
    eb = (bsum(e * e) / n).sqrt()
    rb = (bsum(r * r) / n).sqrt()
    floor = 0.1 * _rms(_as2d(ref))
    return float((eb / rb.clamp_min(max(floor, 1e-300))).max())


class Shadow:
    """see the module docstring.  ``trace_dir``: also turn on the library's profiler for classes 0-3 (+ trace) and attribute every
    traced launch to the shadow-checked call that issued it (``families``, ``unchecked_launches``)."""

    def __init__(self, name: str, report: Optional[str] = None, trace_dir: Optional[str] = None):
        self.name, self.report, self.trace_dir = name, report, trace_dir
        self.failures: list = []
        self.worst = defaultdict(lambda: {"elem": 0.0, "blk": 0.0, "rms": 0.0, "n": 0})
        self.calls = 0
        self.depth = 0
        self._saved = {}
        self._stats_owner = {}           # GnStats.data ptr -> (producer's output, its per-sample rows)
        self._q8_owner = {}              # Mx8Act.data ptr -> the bf16 values it twins (fp64 row statistics of an LN fold)
        self._tables = {}                # TattnTables.A storage ptr -> (base ptr, row bytes, prepare operands)
        self._launch_calls: list = []    # (op, shape, launches in classes 0..3)
        self.families = defaultdict(int)
        self.family_worst = defaultdict(lambda: {"elem": 0.0, "blk": 0.0})
        self.op_families = defaultdict(int)      # (op, family) -> traced launches: which plan served which ops function
        self.unchecked_launches = 0
        self.traced = 0
        self.seen = defaultdict(int)     # (op, shape note) -> comparisons; (op, "call") -> checked calls of that op

    # ---------------------------------------------------------------------------------------------------- patching
    def __enter__(self):
        from udifftext_amd import ops
        self.ops = ops
        for nm, fn in list(vars(ops).items()):
            if nm.startswith("_") or not inspect.isfunction(fn) or fn.__module__ != ops.__name__:
                continue
            self._saved[nm] = fn
            if nm in PASSTHROUGH:
                continue
            setattr(ops, nm, self._wrap(nm, fn))
        if self.trace_dir is not None:
            from udifftext_amd import lib as L
            torch.cuda.synchronize()
            self._lib = L.load()
            self._lib.udt_prof_trace(0)
            self._saved["prof_reset"]()
            self._lib.udt_prof_trace(1)
            self._saved["prof_enable"](0xF)
        return self

    def __exit__(self, *exc):
        from udifftext_amd import ops
        for nm, fn in self._saved.items():
            setattr(ops, nm, fn)
        if self.trace_dir is not None:
            torch.cuda.synchronize()
            ops.prof_enable(0)
            path = os.path.join(self.trace_dir, f"shadow_trace_{self.name.replace(' ', '_')}.csv")
            self._lib.udt_prof_dump(path.encode())
            self._lib.udt_prof_trace(0)
            rows = [ln.split(",", 2) for ln in open(path).read().splitlines()[1:]]
            self.traced = len(rows)
            i = 0
            for op, n, res, fail in self._launch_calls:
                for r in rows[i:i + n]:
                    fam = r[2].split(" ")[0] if r[2] else op            # (untagged launches: the op's name)
                    self.families[fam] += 1
                    self.op_families[(op, fam)] += 1
                    fw = self.family_worst[fam]
                    fw["elem"], fw["blk"] = max(fw["elem"], res[0]), max(fw["blk"], res[1])
                if fail is not None:
                    self.failures[fail] += " [plan: " + "; ".join(r[2] or f"class {r[0]}" for r in rows[i:i + n]) + "]"
                i += n
            self.unchecked_launches = self.traced - i
        self._write_report()
        return False

    def _wrap(self, nm, fn):
        ref = getattr(self, "_ref_" + nm, None)

        def wrapper(*args, **kw):
            if self.depth > 0:
                return fn(*args, **kw)
            if ref is None:
                self.failures.append(f"ops.{nm} was called inside the shadow and has no float64 reference")
                raise AssertionError(f"shadow: ops.{nm} has no reference (add one to tests/shadow_ref.py)")
            if kw.get("probe_in_scsh"):
                return fn(*args, **kw)
            bound = inspect.signature(fn).bind(*args, **kw)
            bound.apply_defaults()
            live = dict(bound.arguments)
            a = {k: _clone(v) for k, v in live.items()}
            before = self._launch_counts()
            self.depth += 1
            try:
                got = fn(*args, **kw)
            finally:
                self.depth -= 1
            torch.cuda.synchronize()
            n = self._launch_counts() - before
            self.calls += 1
            self.seen[(nm, "call")] += 1
            self._cur = [0.0, 0.0, None]
            with torch.no_grad():
                ref(a, got, live)
            fail = None
            if self._cur[2]:
                fail = len(self.failures)
                self.failures.append(f"ops.{nm}: {self._cur[2]}")
            self._launch_calls.append((nm, n, tuple(self._cur), fail))
            return got
        wrapper.__wrapped__ = fn
        return wrapper

    def _launch_counts(self):
        if self.trace_dir is None:
            return 0
        return sum(self._saved["prof_get"](c)[1] for c in range(4))

    # -------------------------------------------------------------------------------------------------- comparison
    def compare(self, what, cls, got, ref, shape_note="", rel_rms=None):
        rtol, atol, k = CLASSES[cls]
        self.seen[(what.split(" ")[0], shape_note)] += 1
        g = got.to(F64)
        r = ref.to(F64).reshape(g.shape)
        err = (g - r)
        rms = _rms(r)
        w = self.worst[cls]
        w["n"] += 1
        if cls == "layout":
            if not torch.equal(g, r):
                self._fail(f"{what} {shape_note}: layout op not exact ({int((g != r).sum())} elements differ)")
            return
        finite = bool(torch.isfinite(g).all())
        scale = rtol * r.abs() + atol * rms + 1e-30
        elem = float((err.abs() / scale).max()) if err.numel() else 0.0
        blk = block_ratio(err, r) if finite else float("inf")
        rr = _rms(err) / max(rms, 1e-300)
        w["elem"], w["blk"], w["rms"] = max(w["elem"], elem), max(w["blk"], blk), max(w["rms"], rr)
        self._cur[0], self._cur[1] = max(self._cur[0], elem), max(self._cur[1], blk / max(k, 1e-30))
        msg = []
        if not finite:
            msg.append("non-finite output")
        if elem > 1.0:
            msg.append(f"element bound exceeded x{elem:.2f} (rtol {rtol:g}, atol {atol:g} RMS)")
        if blk > k:
            msg.append(f"32x32 block error {blk:.3e} > k {k:g}")
        if rel_rms is not None and rr > rel_rms:
            msg.append(f"rel RMS {rr:.3e} > {rel_rms:g}")
        if msg:
            self._fail(f"{what} {shape_note} [{cls}]: " + "; ".join(msg))

    def saw(self, op, pred=None):
        """how many comparisons of ``op`` were made (``pred``: on a shape note it accepts); without ``pred``: checked calls of it"""
        if pred is None:
            return self.seen.get((op, "call"), 0)
        return sum(n for (o, note), n in self.seen.items() if o == op and note != "call" and pred(note))

    def _fail(self, m):
        if self._cur[2] is None:
            self._cur[2] = m
        else:
            self._cur[2] += " | " + m

    def check_q8(self, what, q8, ref, n_cols, fixed=None, ref_is_twin=False):
        """an emitted MX8 twin: decoded values within half an e4m3 step at the block scale (+ the bf16 rounding of the twin and the
        op's own tolerance when ``ref`` is the fp64 reference rather than the bf16 twin), block scales tight, row statistics"""
        M = ref.shape[0]
        r = ref.to(F64).reshape(M, -1)[:, :n_cols]
        dec = decode_q8(q8, n_cols, fixed).to(F64)
        c_blk = n_cols if fixed is None else min(fixed[0], n_cols)
        rb = r[:, :c_blk]
        amax = rb.reshape(M, c_blk // 32, 32).abs().amax(dim=2)
        bound = (amax / 14.0).repeat_interleave(32, dim=1) + rb.abs() * 2.0 ** -7 + 1e-30
        if not ref_is_twin:
            bound = bound + 1.5e-2 * rb.abs() + 2e-2 * _rms(rb)
        e = ((dec[:, :c_blk] - rb).abs() / bound).max().item() if c_blk else 0.0
        w = self.worst["q8"]
        w["n"] += 1
        w["elem"] = max(w["elem"], e)
        self._cur[0] = max(self._cur[0], e)
        if e > 1.0:
            self._fail(f"{what}: MX8 twin off its element bound x{e:.2f}")
        if c_blk:
            qmax = q8.data[:, :c_blk].contiguous().view(torch.float8_e4m3fn).float().reshape(M, c_blk // 32, 32).abs().amax(dim=2)
            live = amax > 1e-20
            if live.any():
                top = float((qmax[live] > 200.0).float().mean())
                if float(qmax[live].max()) > 448.0 or top <= 0.99:
                    self._fail(f"{what}: MX8 block scales not tight (blocks in the top binades {top:.4f})")
            rr = _rms(dec[:, :c_blk] - rb) / max(_rms(rb), 1e-300)
            w["rms"] = max(w["rms"], rr)
            if rr > REL_RMS["q8"]:
                self._fail(f"{what}: MX8 twin rel RMS {rr:.3e} > {REL_RMS['q8']}")
        if fixed is not None and fixed[0] < n_cols:
            v = r[:, fixed[0]:]
            mul = fixed[1]
            got = dec[:, fixed[0]:] * mul
            want = (v * mul).clamp(-448.0, 448.0)
            ok = ((got - want).abs() <= want.abs() * 2.0 ** -4 + 2.0 ** -10 + v.abs() * mul * (2.0 ** -7 + (0 if ref_is_twin else 3e-2))
                  + (0 if ref_is_twin else 2e-2 * _rms(v) * mul)).all()
            if not bool(ok):
                self._fail(f"{what}: fixed-scale columns from {fixed[0]} (x{mul:g}) off e4m3(v * mul)")
        if q8.stats is not None:
            self.check_rowstats(what, q8.stats, r)

    def check_rowstats(self, what, stats, values):
        s = stats.to(F64).sum(dim=0)
        v = values.to(F64)
        e1 = ((s[:, 0] - v.sum(dim=1)).abs() / (STATS_RTOL * v.abs().sum(dim=1) + 1e-30)).max().item()
        e2 = ((s[:, 1] - v.pow(2).sum(dim=1)).abs() / (STATS_RTOL * v.pow(2).sum(dim=1) + 1e-30)).max().item()
        w = self.worst["rowstats"]
        w["n"] += 1
        w["elem"] = max(w["elem"], e1, e2)
        if max(e1, e2) > 1.0:
            self._fail(f"{what}: row statistics off x{max(e1, e2):.2f}")

    def check_colstats(self, what, out, st, B):
        """GnStats [slots, C, 2]: per sample (slots_per_sample consecutive slots; the buffer may hold more slots than the B samples
        use), the column sums / sums of squares of the output"""
        if st is None:
            return
        C = st.data.shape[1]
        o = out.to(F64).reshape(B, -1, out.shape[-1])[..., :C]
        s = st.data[:B * st.slots_per_sample].to(F64).reshape(B, st.slots_per_sample, C, 2).sum(dim=1)
        r1, r2 = o.sum(dim=1), o.pow(2).sum(dim=1)
        n = o.shape[1]
        # the sums of a sample's rows: |d sum| <= 2e-3 * sqrt(n) * RMS + rtol * |sum| ; |d sumsq| <= rtol * sumsq
        e1 = ((s[..., 0] - r1).abs() / (2e-3 * math.sqrt(n) * r2.div(n).sqrt() + 2e-3 * r1.abs() + 1e-30)).max().item()
        e2 = ((s[..., 1] - r2).abs() / (2e-3 * r2 + 1e-30)).max().item()
        w = self.worst["colstats"]
        w["n"] += 1
        w["elem"] = max(w["elem"], e1, e2)
        if max(e1, e2) > 1.0:
            self._fail(f"{what}: GroupNorm column statistics off x{max(e1, e2):.2f}")
        self._stats_owner[st.data.data_ptr()] = out.detach().clone()

    def _note_q8(self, q8, values):
        if q8 is not None:
            self._q8_owner[q8.data.data_ptr()] = values.detach().clone()

    # ------------------------------------------------------------------------------------------------ per-op references
    def _ref_linear(self, a, got, live):
        from udifftext_amd import lib as L
        x, w, flags = a["x"], a["w"], a["flags"]
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        M = x2.shape[0]
        N = w.shape[0] if a["n_out"] is None else a["n_out"]
        res = a["residual"]
        ref = ref_linear(x2, w, N, bias=a["bias"], rowvec=a["rowvec"], rows_per_batch=a["rows_per_batch"],
                         residual=(res.reshape(M, -1) if res is not None else None), flags=flags, alpha=a["alpha"])
        if flags & L.GEMM_TRANSPOSED:
            rpb = a["rows_per_batch"]
            ref = ref.reshape(M // rpb, rpb, N).transpose(1, 2)
        note = f"M={M} N={N} K={K} fl={flags:#x}"
        self.compare("linear", "gemm", got, ref, note)
        self.check_colstats(f"linear {note}", got, self.ops.gn_stats_of(got), M // max(a["rows_per_batch"], 1))
        q8 = self.ops.mx8_of(got)
        if q8 is not None:
            self.check_q8(f"linear {note}", q8, got.reshape(M, -1), got.shape[-1], ref_is_twin=True)
            self._note_q8(q8, got.reshape(M, -1))

    def _ref_ln_linear(self, a, got, live):
        from udifftext_amd import lib as L
        x, w, flags = a["x"], a["w_folded"], a["flags"]
        K = x.shape[-1]
        x2 = x.reshape(-1, K)
        M = x2.shape[0]
        N = w.shape[0] if a["n_out"] is None else a["n_out"]
        n_cols = N // 2 if flags & L.GEMM_GEGLU else N
        res = a["residual"]
        ref = ref_ln_linear(x2, w, a["c"], N, a["eps"], residual=(res.reshape(M, -1) if res is not None else None), flags=flags)
        note = f"M={M} N={N} K={K} fl={flags:#x}"
        if got is None:
            return
        if isinstance(got, self.ops.Mx8Act):
            self.check_q8(f"ln_linear {note} (MX8 only)", got, ref, n_cols, fixed=a["q8_fixed"])
            return
        self.compare("ln_linear", "gemm", got, ref, note)
        q8 = self.ops.mx8_of(got)
        if q8 is not None:
            self.check_q8(f"ln_linear {note}", q8, got.reshape(M, -1), n_cols, fixed=a["q8_fixed"], ref_is_twin=True)

    def _ref_linear_mx8(self, a, got, live):
        from udifftext_amd import lib as L
        x8, wq, flags = a["x"], a["wq"], a["flags"]
        M, K = x8.data.shape
        N = wq.shape[0] if a["n_out"] is None else a["n_out"]
        n_cols = N // 2 if flags & L.GEMM_GEGLU else N
        xdec = mx8_ref.decode(x8.data, x8.scale)
        ln = None
        if a["ln_s"] is not None:
            src = self._q8_owner.get(live["x"].data.data_ptr())
            if src is not None and src.shape[0] == M:
                v = src.to(F64)[:, :K]
                mean = v.mean(dim=1)
                var = (v - mean[:, None]).pow(2).mean(dim=1)
            else:                                      # (a producer the shadow did not see: its emitted row statistics)
                st = x8.stats.to(F64).sum(dim=0)
                mean = st[:, 0] / K
                var = st[:, 1] / K - mean * mean
            ln = (a["ln_c"], a["ln_s"], mean, 1.0 / torch.sqrt(var + a["eps"]))
        res = a["residual"]
        ref = ref_linear_mx8(xdec, wq, a["colscale"], N, bias=a["bias"], ln=ln, flags=flags,
                             residual=(res.reshape(M, -1) if res is not None else None))
        note = f"M={M} N={N} K={K} fl={flags:#x} ln={int(ln is not None)}"
        if isinstance(got, self.ops.Mx8Act):
            self.check_q8(f"linear_mx8 {note} (MX8 only)", got, ref, n_cols, fixed=a["q8_fixed"])
            return
        self.compare("linear_mx8", "gemm-mx8", got, ref, note, rel_rms=REL_RMS["gemm-mx8"])
        self.check_colstats(f"linear_mx8 {note}", got, self.ops.gn_stats_of(got), M // max(a["rows_per_batch"], 1))
        q8 = self.ops.mx8_of(got)
        if q8 is not None:
            self.check_q8(f"linear_mx8 {note}", q8, got.reshape(M, -1), n_cols, fixed=a["q8_fixed"], ref_is_twin=True)
            self._note_q8(q8, got.reshape(M, -1))

    def _ref_bmm_nt(self, a, got, live):
        ref = torch.matmul(_d(a["a"]), _d(a["w"]).transpose(1, 2)) * a["alpha"]
        B, M, K = a["a"].shape
        self.compare("bmm_nt", "gemm", got, ref, f"B={B} M={M} N={a['w'].shape[1]} K={K}")

    def _ref_conv2d(self, a, got, live):
        from udifftext_amd import lib as L
        x = a["x"]
        kw = {k: a[k] for k in ("ksize", "stride", "pad", "upsample", "x2", "out_hw", "rowvec", "flags", "n_out", "in_scsh", "in_act")}
        B = x.shape[0]
        outs = []
        for b in range(B):                       # one image at a time
            kb = dict(kw)
            kb["x2"] = kw["x2"][b:b + 1] if kw["x2"] is not None else None
            kb["rowvec"] = kw["rowvec"][b:b + 1] if kw["rowvec"] is not None else None
            kb["in_scsh"] = kw["in_scsh"].reshape(B, -1)[b:b + 1] if kw["in_scsh"] is not None else None
            outs.append(ref_conv2d(x[b:b + 1], a["w"], a["bias"], residual=(a["residual"][b:b + 1] if a["residual"] is not None else None),
                                   **kb))
        ref = torch.cat(outs)
        C2 = a["x2"].shape[-1] if a["x2"] is not None else 0
        note = (f"{x.shape[1]}x{x.shape[2]} C={x.shape[-1]}+{C2} N={ref.shape[-1]} k{a['ksize']} s{a['stride']}"
                f"{' up' if a['upsample'] else ''}{' gn' if a['in_scsh'] is not None else ''}{' f32' if a['flags'] & L.GEMM_OUT_F32 else ''}")
        self.compare("conv2d", "conv+gn" if a["in_scsh"] is not None else "conv", got, ref, note)
        self.check_colstats(f"conv2d {note}", got, self.ops.gn_stats_of(got), B)

    def _ref_group_norm(self, a, got, live):
        ref = ref_group_norm(a["x"], a["gamma"], a["beta"], a["groups"], a["eps"], a["silu"], x2=a["x2"])
        self.compare("group_norm", "norm", got, ref, f"{tuple(a['x'].shape)} G={a['groups']}")

    def _ref_group_norm_from_stats(self, a, got, live):
        ref = ref_group_norm(a["x"], a["gamma"], a["beta"], a["groups"], a["eps"], a["silu"], x2=a["x2"])
        self.compare("group_norm_from_stats", "norm", got, ref, f"{tuple(a['x'].shape)} G={a['groups']}")

    def _ref_gn_finalize(self, a, got, live):
        x1 = self._stats_owner.get(live["st1"].data.data_ptr())
        x2 = self._stats_owner.get(live["st2"].data.data_ptr()) if live["st2"] is not None else None
        note = f"B={a['B']} HW={a['HW']} C={a['C1']}+{a['C2']}"
        if x1 is None or (a["st2"] is not None and x2 is None):
            self._fail(f"gn_finalize {note}: statistics of a producer the shadow did not see")
            return
        B = a["B"]
        x1 = x1.reshape(B, a["HW"], -1)[..., :a["C1"]]
        x2 = x2.reshape(B, a["HW"], -1)[..., :a["C2"]] if x2 is not None else None
        ref = ref_gn_table(x1, a["gamma"], a["beta"], a["groups"], a["eps"], x2=x2)
        # (scale and shift compared as two tensors: their magnitudes differ)
        g = got.reshape(ref.shape)
        self.compare("gn_finalize scale", "gn-table", g[:, :, 0], ref[:, :, 0], note)
        self.compare("gn_finalize shift", "gn-table", g[:, :, 1], ref[:, :, 1], note)

    def _ref_layer_norm(self, a, got, live):
        self.compare("layer_norm", "norm", got, ref_layer_norm(a["x"], a["gamma"], a["beta"], a["eps"]), f"{tuple(a['x'].shape)}")

    def _ref_xattention(self, a, got, live):
        q, k, v = a["q"], a["k"], a["v"]
        ref = ref_attention(q, k, v, a["heads"], a["head_dim"], a["scale"])
        note = f"B={q.shape[0]} Nq={q.shape[1]} L={k.shape[1]} H={a['heads']}"
        self.compare("xattention", "xattn", got, ref, note)
        if a["probs"] is not None:
            p = ref_probs(q, k, a["heads"], a["head_dim"], a["scale"])
            self.compare("xattention probs", "xattn-probs", live["probs"], p, note)

    def _ref_attention_rowv(self, a, got, live):
        q, k, v = a["q"], a["k"], a["v"]
        ref = ref_attention(q, k, v, a["heads"], 64, a["scale"])
        note = f"B={q.shape[0]} N={q.shape[1]} H={a['heads']}"
        self.compare("attention_rowv", "attn", got, ref, note)
        q8 = self.ops.mx8_of(got)
        if q8 is not None:
            B, N, C = got.shape
            self.check_q8(f"attention_rowv {note}", q8, got.reshape(B * N, C), C, ref_is_twin=True)
            self._note_q8(q8, got.reshape(B * N, C))

    def _ref_attention_d512(self, a, got, live):
        q, k, v = a["q"], a["k"], a["v"]
        self.compare("attention_d512", "attn", got, ref_attention(q, k, v, 1, 512, a["scale"]), f"B={q.shape[0]} N={q.shape[1]}")

    def _ref_attention_mx8(self, a, got, live):
        qkv, B, heads = a["qkv"], a["batch"], a["heads"]
        C = heads * 64
        M = qkv.data.shape[0]
        N = M // B
        dec = decode_q8(qkv, 3 * C, fixed=(2 * C, a["v_mul"])).reshape(B, N, 3 * C)
        ref = ref_attention(dec[..., :C], dec[..., C:2 * C], dec[..., 2 * C:], heads, 64, a["scale"])
        note = f"B={B} N={N} H={heads}"
        self.compare("attention_mx8", "attn-mx8", got, ref, note, rel_rms=REL_RMS["attn-mx8"])
        q8 = self.ops.mx8_of(got)
        if q8 is not None:
            self.check_q8(f"attention_mx8 {note}", q8, got.reshape(M, C), C, ref_is_twin=True)
            self._note_q8(q8, got.reshape(M, C))

    def _ref_masked_attention(self, a, got, live):
        q, k, v, mask, kpm = a["q"], a["k"], a["v"], a["mask"], a["key_padding_mask"]
        ref = ref_masked_attention(q, k, v, a["heads"], a["scale"], mask=mask, key_padding_mask=kpm)
        note = (f"B={q.shape[0]} Nq={q.shape[1]} Lk={k.shape[1]} H={a['heads']} D={q.shape[2] // a['heads']} "
                f"mask={int(mask is not None)} kpm={int(kpm is not None)}")
        self.compare("masked_attention", "attn", got, ref, note)

    def _ref_tattn_prepare(self, a, got, live):
        # the tables are opaque (MFMA fragment order): they are pinned through tattn_fused, whose reference takes these operands
        self._tables[got.A.untyped_storage().data_ptr()] = (got.A.data_ptr(), got.A.stride(0) * got.A.element_size(), a)

    def _ref_tattn_fused(self, a, got, live):
        x, tabs = a["x"], live["tables"]
        B, N, C = x.shape
        kv = torch.zeros((B, 1, 2 * C), dtype=x.dtype, device=x.device)
        prep = None
        if tabs is not None:
            ent = self._tables.get(tabs.A.untyped_storage().data_ptr())
            if ent is None:
                self._fail(f"tattn_fused B={B} N={N} C={C}: tables from a tattn_prepare the shadow did not see")
                return
            base, row, prep = ent
            r0 = (tabs.A.data_ptr() - base) // row
            kv = prep["kv"][r0:r0 + B]
        if prep is None:
            ref = _d(x) + _d(a["bias"][:C])
            if a["zero_samples"] < B:
                self._fail("tattn_fused without tables for context samples")
                return
        else:
            ref = ref_tattn(x, kv, prep["wq"], prep["wo"], prep["gamma"], prep["beta"], a["bias"], a["heads"], prep["scale"],
                            a["zero_samples"], a["eps"])
        note = f"B={B} N={N} C={C} zero={a['zero_samples']}"
        self.compare("tattn_fused", "tattn", got, ref, note)
        q8 = self.ops.mx8_of(got)
        if q8 is not None:
            self.check_q8(f"tattn_fused {note}", q8, got.reshape(B * N, C), C, ref_is_twin=True)
            self._note_q8(q8, got.reshape(B * N, C))

    def _ref_bias_add(self, a, got, live):
        C = a["x"].shape[-1]
        self.compare("bias_add", "elementwise", got, _d(a["x"]) + _d(a["bias"][:C]), f"{tuple(a['x'].shape)}")

    def _ref_softmax_rows_(self, a, got, live):
        self.compare("softmax_rows_", "softmax", got, torch.softmax(_d(a["x"]), dim=-1), f"{tuple(a['x'].shape)}")

    def _ref_timestep_embedding(self, a, got, live):
        self.compare("timestep_embedding", "elementwise", got, ref_timestep_embedding(a["t"], a["dim"]), f"n={a['t'].numel()}")

    def _ref_posterior_sample(self, a, got, live):
        mom = a["moments"]
        self.compare("posterior_sample", "f32", got, ref_posterior_sample(mom, a["noise"], a["scale"]), f"{tuple(mom.shape)}")

    def _ref_mask_downsample(self, a, got, live):
        self.compare("mask_downsample", "f32", got, ref_mask_downsample(a["mask"]), f"{tuple(a['mask'].shape)}")

    def _ref_embed_tokens(self, a, got, live):
        self.compare("embed_tokens", "elementwise", got, ref_embed_tokens(a["idx"], a["table"], a["pe"]),
                     f"n={a['idx'].numel()} Lc={a['pe'].shape[0]} D={a['pe'].shape[1]}")

    def _ref_unet_input(self, a, got, live):
        x, xin0 = a["x"], a["xin"]
        B, _, h, w = x.shape
        want = xin0.clone()
        v = (x.float() * a["c_in"]).permute(0, 2, 3, 1).reshape(B, h * w, 4).bfloat16()
        xv = want.reshape(2 * B, h * w, -1)
        xv[:B, :, :4] = v
        xv[B:, :, :4] = v
        self.compare("unet_input", "elementwise", live["xin"], want, f"B={B} {h}x{w}")

    def _ref_nchw_to_nhwc(self, a, got, live):
        x = a["x"]
        B, Cc, H, W_ = x.shape
        want = torch.zeros((B, H, W_, a["cpad"]), dtype=torch.bfloat16, device=x.device)
        want[..., :Cc] = (x.float() * a["scale"]).permute(0, 2, 3, 1).bfloat16()
        self.compare("nchw_to_nhwc", "layout", got, want, f"{tuple(x.shape)} -> {a['cpad']}")

    def _ref_nhwc_to_nchw(self, a, got, live):
        x = a["x"]
        want = x[..., :a["channels"]].float().permute(0, 3, 1, 2)
        self.compare("nhwc_to_nchw", "layout", got, want, f"{tuple(x.shape)} -> {a['channels']}")

    def _ref_nhwc_set_channels(self, a, got, live):
        src, dst0, c0 = a["src"], a["dst"], a["c0"]
        B, Cc, H, W_ = src.shape
        want = dst0.clone().reshape(B, H, W_, -1)
        want[..., c0:c0 + Cc] = src.float().permute(0, 2, 3, 1).bfloat16()
        self.compare("nhwc_set_channels", "layout", live["dst"], want, f"{tuple(src.shape)} @ {c0}")

    # -------------------------------------------------------------------------------------------------------- report
    def _write_report(self):
        if not self.report:
            return
        os.makedirs(os.path.dirname(self.report), exist_ok=True)
        with open(self.report, "a") as f:
            f.write(f"# shadow: {self.name} — {self.calls} ops calls checked, {self.traced} traced class 0-3 launches\n")
            for cls, w in sorted(self.worst.items()):
                if cls in CLASSES:
                    rtol, atol, k = CLASSES[cls]
                    f.write(f"  shadow {cls:14s} n={w['n']:5d} elem {w['elem']:.3e} (tol 1.0, rtol {rtol:g} atol {atol:g}) "
                            f"block {w['blk']:.3e} (k {k:g}) rel_rms {w['rms']:.3e}\n")
                else:
                    f.write(f"  shadow {cls:14s} n={w['n']:5d} elem {w['elem']:.3e} (tol 1.0) rel_rms {w['rms']:.3e}\n")
            for fam in sorted(self.families):
                fw = self.family_worst[fam]
                f.write(f"  family {fam:22s} launches {self.families[fam]:5d} worst elem {fw['elem']:.3e} (tol 1.0) "
                        f"worst block/k {fw['blk']:.3e} (tol 1.0)\n")
            if self.op_families:
                f.write("  plans " + ", ".join(f"{op}:{fam} {n}" for (op, fam), n in sorted(self.op_families.items())) + "\n")


def _clone(v):
    if isinstance(v, torch.Tensor):
        return v.detach().clone()
    if isinstance(v, tuple) and hasattr(v, "_fields"):
        return type(v)(*[_clone(t) for t in v])
    if isinstance(v, (list, tuple)):
        return type(v)(_clone(t) for t in v)
    return v
