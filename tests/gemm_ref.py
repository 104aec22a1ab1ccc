"""float64 references of the forward GEMM / convolution family (udt_gemm: csrc/gemm.hip and the headers it includes) and the emulation
of the roundings those kernels state (a helper, not a test; plain torch, float64, device-agnostic — no vendor library call).

Every entry returns ``(ref64, emul, abs_terms)``: ``emul`` is the same float64 computation rounded only where the kernel says it
rounds (ONE rounding of the stored result to bf16, none for UDT_GEMM_OUT_F32; the +gn form also rounds the transformed input patch,
conv3p.h:211-216); ``abs_terms`` is the same formula with every summand replaced by its absolute value (the condition-number scale of
tests/sliced_check.py; element-wise it is check_fp32_sum's sum|summands|).  The GEGLU forms return a fourth element: the measured error
of the erf approximations times 0.5 |value gate|, which the caller adds to floor_err (see erf_error).

Epilogue order (gemm.hip epilogue(), lean.h:590-655): acc * alpha + bias + rowvec[row // rows_per_batch] + residual, then ReLU or
SiLU, then the rounding.  GEGLU: value * gelu_erf(gate) on packed [32 value | 32 gate] column blocks.  LayerNorm-folded:
rstd (x w^T - mean s) alpha + c with mean / rstd of the bf16 rows.

Convolutions are nine (four, one) shifted float64 matmuls over NHWC with explicit zero padding.
"""
import contextlib
import math

import torch

F64 = torch.float64
DT = F64                # the working precision: float64, except inside restated_in() (the float32 restatement of the CPU tests)


@contextlib.contextmanager
def restated_in(dtype):
    """the same formulas evaluated in ``dtype`` (float32: accumulation and epilogue in float32, the same single roundings)"""
    global DT
    prev, DT = DT, dtype
    try:
        yield
    finally:
        DT = prev


def bf16_round(t):
    return t.to(torch.float32).to(torch.bfloat16).to(DT)


def _d(t):
    return None if t is None else t.to(DT)


# ------------------------------------------------------------------------------------------------ approximate functions
# coefficients as data, copied from csrc/common.h (gelu_erf_f: Abramowitz-Stegun 7.1.26; geglu_scaled: log2 erfc polynomial)
AS_P, AS_A = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
ERFC_LOG2_POLY = (-1.3553386, -0.636406, -0.086436, 0.014895574, -0.001489955, 5.1346913e-05)     # t, t^2, .. t^6
ERFC_T_MAX = 7.2067347
GEGLU_GS = 0.70710678118654752 * 1.2011224087864498


def erf_as(x):
    z = abs(x)
    t = 1.0 / (1.0 + AS_P * z)
    poly = sum(a * t ** (i + 1) for i, a in enumerate(AS_A))
    return math.copysign(1.0 - poly * math.exp(-z * z), x)


def erfc_poly(z):
    """erfc(z), z >= 0, as lean.h / rowres.h evaluate it: 2^P(t), t = z * sqrt(log2 e) clamped"""
    t = min(z * 1.2011224087864498, ERFC_T_MAX)
    return 2.0 ** sum(c * t ** (i + 1) for i, c in enumerate(ERFC_LOG2_POLY))


def measured_erf_error(n=24001, zmax=6.0):
    """worst |approximation - math.erf| over z in [0, zmax] for both forms, evaluated in float64 on the CPU: (A-S, erfc polynomial)"""
    e_as = e_pl = 0.0
    for i in range(n):
        z = zmax * i / (n - 1)
        e_as = max(e_as, abs(erf_as(z) - math.erf(z)))
        e_pl = max(e_pl, abs((1.0 - erfc_poly(z)) - math.erf(z)))
    return e_as, e_pl


_ERF_ERR = None


def erf_error():
    """the larger of the two measured worst errors (whichever kernel serves a GEGLU case is covered)"""
    global _ERF_ERR
    if _ERF_ERR is None:
        _ERF_ERR = max(measured_erf_error())
    return _ERF_ERR


def gelu_erf(g):
    return 0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752))


# ------------------------------------------------------------------------------------------------ products
def matmul_nt(a, w):
    """a [.., M, K] w [.., N, K] -> (a w^T, |a| |w|^T) in float64"""
    a, w = _d(a), _d(w)
    return a @ w.transpose(-1, -2), a.abs() @ w.abs().transpose(-1, -2)


def upsample2(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def conv_acc(x, w, *, ksize=3, stride=1, pad_t=1, pad_l=1, upsample=False, out_hw=None, x2=None):
    """NHWC x [B, H, W, C1] (+ x2 [B, H, W, C2], channel concat) against w [N, ksize^2 (C1 + C2)] packed tap-major: ksize^2 shifted
    matmuls with explicit zero padding (top / left pad_t / pad_l; bottom / right as far as the output reaches).
    -> (acc, |acc|) as [B, Ho, Wo, N]"""
    x = _d(x)
    if x2 is not None:
        x = torch.cat([x, _d(x2)], dim=-1)
    if upsample:
        x = upsample2(x)
    w = _d(w)
    B, H, W, C = x.shape
    N = w.shape[0]
    if out_hw is None:
        out_hw = ((H + 2 * pad_t - ksize) // stride + 1, (W + 2 * pad_l - ksize) // stride + 1)
    Ho, Wo = out_hw
    need_h, need_w = (Ho - 1) * stride + ksize, (Wo - 1) * stride + ksize
    xp = torch.zeros((B, max(need_h, H + pad_t), max(need_w, W + pad_l), C), dtype=DT, device=x.device)
    xp[:, pad_t:pad_t + H, pad_l:pad_l + W] = x
    acc = torch.zeros((B, Ho, Wo, N), dtype=DT, device=x.device)
    aabs = torch.zeros_like(acc)
    for ky in range(ksize):
        for kx in range(ksize):
            tap = ky * ksize + kx
            wt = w[:, tap * C:(tap + 1) * C]
            xs = xp[:, ky:ky + (Ho - 1) * stride + 1:stride, kx:kx + (Wo - 1) * stride + 1:stride]
            acc += xs @ wt.t()
            aabs += xs.abs() @ wt.abs().t()
    return acc, aabs


def conv_up4_acc(x, w_up4, n_out=None):
    """the phase form on the up4 weights AS PACKED ([4, N rows, 4 C], phase 2a + b, k = (2r + s) C + c): output pixel (2i + a, 2j + b)
    = sum_{r, s} x[i - 1 + a + r, j - 1 + b + s] . w[2a + b][:, (2r + s) C : ...]   (lean.h:718-723) -> [B, 2H, 2W, N]"""
    x, w = _d(x), _d(w_up4)
    B, H, W, C = x.shape
    N = w.shape[1] if n_out is None else n_out
    xp = torch.zeros((B, H + 2, W + 2, C), dtype=DT, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    acc = torch.zeros((B, 2 * H, 2 * W, N), dtype=DT, device=x.device)
    aabs = torch.zeros_like(acc)
    for a in range(2):
        for b in range(2):
            for r in range(2):
                for s in range(2):
                    wt = w[2 * a + b, :N, (2 * r + s) * C:(2 * r + s + 1) * C]
                    xs = xp[:, a + r:a + r + H, b + s:b + s + W]
                    acc[:, a::2, b::2] += xs @ wt.t()
                    aabs[:, a::2, b::2] += xs.abs() @ wt.abs().t()
    return acc, aabs


def gn_on_patch(x, scsh, in_act, emulate):
    """act(x * scale + shift) from the table as given ([B, chunks, 64 scale | 64 shift] fp32), rounded to bf16 when emulating
    (in-image pixels; the zero padding is added by conv_acc afterwards, so it stays zero — conv3p.h:214)"""
    x = _d(x)
    B, H, W, C = x.shape
    t = _d(scsh).reshape(B, C // 64, 2, 64)
    scale = t[:, :, 0].reshape(B, 1, 1, C)
    shift = t[:, :, 1].reshape(B, 1, 1, C)
    y = x * scale + shift
    if in_act == 1:
        y = y * torch.sigmoid(y)
    return bf16_round(y) if emulate else y


# ------------------------------------------------------------------------------------------------ epilogues
def epilogue(acc, aabs, *, alpha=1.0, bias=None, rowvec=None, rows_per_batch=0, residual=None, act=None, out_f32=False):
    """acc / aabs [M, N] -> (ref64, emul, abs_terms)"""
    M = acc.shape[-2]
    v = acc * alpha
    a = aabs * abs(alpha)
    if bias is not None:
        v = v + _d(bias)
        a = a + _d(bias).abs()
    if rowvec is not None:
        rows = torch.arange(M, device=acc.device) // rows_per_batch
        rv = _d(rowvec)[rows][:, :acc.shape[1]]
        v = v + rv
        a = a + rv.abs()
    if residual is not None:
        v = v + _d(residual)
        a = a + _d(residual).abs()
    if act == "relu":
        v = v.clamp_min(0.0)
    elif act == "silu":
        v = v * torch.sigmoid(v)
    return v, (v.clone() if out_f32 else bf16_round(v)), a


def _geglu_scale(val, gate, a_val, a_gate):
    """first-order scale of value * gelu(gate) under perturbations of the two sums in units of their summands' magnitudes:
    a_val |gelu(gate)| + |value| a_gate max|gelu'|   (max |gelu'| = 1.129)"""
    return a_val * gelu_erf(gate).abs() + val.abs() * a_gate * 1.129


def geglu_epilogue(acc, aabs, *, alpha=1.0, bias=None):
    """packed [32 value | 32 gate] blocks of 64 columns -> N / 2 columns; the erf approximation's measured error enters emul's distance
    to ref64 through ``extra`` = erf_error() * 0.5 |value gate| (returned as a fourth element)"""
    M, N = acc.shape
    v = acc * alpha
    a = aabs * abs(alpha)
    if bias is not None:
        v = v + _d(bias)
        a = a + _d(bias).abs()
    v = v.reshape(M, N // 64, 2, 32)
    a = a.reshape(M, N // 64, 2, 32)
    val, gate = v[:, :, 0].reshape(M, N // 2), v[:, :, 1].reshape(M, N // 2)
    out = val * gelu_erf(gate)
    scale = _geglu_scale(val, gate, a[:, :, 0].reshape(M, N // 2), a[:, :, 1].reshape(M, N // 2))
    extra = erf_error() * 0.5 * (val * gate).abs()
    return out, bf16_round(out), scale, extra


def gemm_ref(a, w, *, alpha=1.0, bias=None, rowvec=None, rows_per_batch=0, residual=None, act=None, out_f32=False, geglu=False,
             transposed=False, acc_hook=None):
    """a [M, K] (or [batch, M, K] without a row vector) against w [N, K]; acc_hook(acc) -> acc rewrites the products before the epilogue
    (the planted defects of tests/test_gemm_ref_cpu.py)"""
    acc, aabs = matmul_nt(a, w)
    if acc_hook is not None:
        acc = acc_hook(acc)
    if geglu:
        return geglu_epilogue(acc, aabs, alpha=alpha, bias=bias)
    ref, emul, ab = epilogue(acc, aabs, alpha=alpha, bias=bias, rowvec=rowvec, rows_per_batch=rows_per_batch, residual=residual,
                             act=act, out_f32=out_f32)
    if transposed:                                    # the same values as [batch][N][rows_per_batch]
        t = lambda z: z.reshape(-1, rows_per_batch, z.shape[1]).transpose(1, 2).contiguous()
        return t(ref), t(emul), t(ab)
    return ref, emul, ab


def ln_gemm_ref(x, w_folded, c, s, *, eps=1e-5, alpha=1.0, geglu=False):
    """rstd (x w^T - mean s) alpha + c, mean / rstd of the bf16 rows; abs_terms: every summand by its absolute value (it cancels)"""
    xd = _d(x)
    mean = xd.mean(dim=1, keepdim=True)
    var = (xd * xd).mean(dim=1, keepdim=True) - mean * mean
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)
    acc, aabs = matmul_nt(x, w_folded)
    sd, cd = _d(s), _d(c)
    v = rstd * (acc - mean * sd) * alpha + cd
    a = rstd * (aabs + mean.abs() * sd.abs()) * abs(alpha) + cd.abs()
    if geglu:
        M, N = v.shape
        v4, a4 = v.reshape(M, N // 64, 2, 32), a.reshape(M, N // 64, 2, 32)
        val, gate = v4[:, :, 0].reshape(M, N // 2), v4[:, :, 1].reshape(M, N // 2)
        out = val * gelu_erf(gate)
        scale = _geglu_scale(val, gate, a4[:, :, 0].reshape(M, N // 2), a4[:, :, 1].reshape(M, N // 2))
        return out, bf16_round(out), scale, erf_error() * 0.5 * (val * gate).abs()
    return v, bf16_round(v), a


def conv_ref(x, w, *, ksize=3, stride=1, pad_t=1, pad_l=1, upsample=0, out_hw=None, x2=None, n_out=None, in_scsh=None, in_act=0,
             alpha=1.0, bias=None, rowvec=None, residual=None, act=None, out_f32=False, acc_hook=None):
    """-> (ref64, emul, abs_terms) as [B, Ho, Wo, N].  upsample: 0, 1 (nearest x2, nine taps on the upsampled map) or 2 (the phase
    form: ``w`` is the up4 layout).  in_scsh: the +gn form (x and x2 transformed first; emul rounds the transformed patch).
    acc_hook(acc [B, Ho, Wo, N]) -> acc: as gemm_ref's."""
    hook = acc_hook or (lambda z: z)
    def run(emulate):
        xa, xb = x, x2
        if in_scsh is not None:
            C1 = x.shape[-1]
            cat = x if x2 is None else torch.cat([_d(x), _d(x2)], dim=-1)
            y = gn_on_patch(cat, in_scsh, in_act, emulate)
            xa, xb = y[..., :C1], (None if x2 is None else y[..., C1:])
        if upsample == 2:
            return conv_up4_acc(xa, w, n_out)
        ww = w if n_out is None else w[:n_out]
        return conv_acc(xa, ww, ksize=ksize, stride=stride, pad_t=pad_t, pad_l=pad_l, upsample=bool(upsample), out_hw=out_hw, x2=xb)
    acc, aabs = run(False)
    acc = hook(acc)
    B, Ho, Wo, N = acc.shape
    flat = lambda t: None if t is None else _d(t).reshape(B * Ho * Wo, -1)[:, :N]
    kw = dict(alpha=alpha, bias=bias, rowvec=rowvec, rows_per_batch=Ho * Wo, residual=flat(residual), act=act, out_f32=out_f32)
    ref, emul, ab = epilogue(acc.reshape(-1, N), aabs.reshape(-1, N), **kw)
    if in_scsh is not None:
        acc_e, aabs_e = run(True)
        _, emul, _ = epilogue(hook(acc_e).reshape(-1, N), aabs_e.reshape(-1, N), **kw)
    sh = (B, Ho, Wo, N)
    return ref.reshape(sh), emul.reshape(sh), ab.reshape(sh)


# ------------------------------------------------------------------------------------------------ column statistics
def colstats_ref(stored, slot_of_row, slots):
    """sum and sum of squares of the STORED output ([M, N], what the kernel wrote) per slot -> (ref [slots, N, 2], sum|summands|);
    slot_of_row [M]: the slot each output row belongs to in the kernel's slot order (see gemm_cases.stats_slot_of_row)"""
    v = _d(stored)
    M, N = v.shape
    idx = slot_of_row.to(v.device).long()
    ref = torch.zeros((slots, N, 2), dtype=DT, device=v.device)
    ab = torch.zeros_like(ref)
    ref[:, :, 0].index_add_(0, idx, v)
    ref[:, :, 1].index_add_(0, idx, v * v)
    ab[:, :, 0].index_add_(0, idx, v.abs())
    ab[:, :, 1].index_add_(0, idx, v * v)
    return ref, ab
