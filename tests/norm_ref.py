"""float64 references, their bf16 emulations and float32 restatements of the forward normalisation kernels (csrc/norm.hip) — a helper,
not a test; plain torch, works on CPU and device tensors.

References (float64; shadow_ref's where they fit): GroupNorm (+ SiLU) over one or two concatenated NHWC sources from the data
(``gn_expect``) and from given fp32 statistics records (``gn_expect_records`` — the records are the kernel's input, so the reference is
their float64 combine), udt_gn_finalize's table (``table_from_records``), udt_gn_stats' partials with sum|summands| beside them
(``stats_partials``), LayerNorm (``ln_expect``).  Every ``*_expect`` returns {"ref", "emul", "A"}: the float64 result, the same rounded
once to bf16 where the kernel stores (the floor of sliced_check.check_sliced is emul - ref, never anything from a kernel), and the
condition scale of the form the kernels evaluate: rms(|x| |sc| + |sh|) for GroupNorm's y = x sc + sh, rms(|x - mean| rstd |gamma| + |beta|)
for LayerNorm.

Restatements (float32 where the kernels' comments say fp32, float64 where they say fp64), one per decomposition norm.hip states:
  gn_two_kernel32    gn_stats_kernel + gn_apply_kernel: fp32 sums per (chunk, channel) over udt_gn_nchunks chunks of ceil(HW / nchunks)
                     pixels, fp32 over the group's channels (the partials), fp64 combine, y = x * sc + sh in fp32
  gn_strip32         gn_strip_kernel: fp32 sums per (pixel lane, channel), fp64 per channel, fp64 per group, the same apply
  gn_records32       gn_strip_kernel with records / gn_finalize_kernel + gn_apply_kernel: fp64 sum over the slots' records
  layer_norm32       layernorm_kernel: fp32 row sum, mean, centred sum of squares
Each takes ``defect=`` (None: sound), the planted defects of tests/test_norm_ref_cpu.py.
"""
import torch

import shadow_ref as SR

G = 32
STRIP_THREADS = 512


def _d(t):
    return t.detach().double()


def _bf16(t):
    """one rounding to bf16, back in float64"""
    return t.float().bfloat16().double()


def _silu(y):
    return y * torch.sigmoid(y)


def _rms(t):
    return float(t.pow(2).mean().sqrt())


def cat_sources(x, x2=None):
    return _d(x) if x2 is None else torch.cat([_d(x), _d(x2)], dim=-1)


# ------------------------------------------------------------------------------------------------ float64 references
def _scale_shift(mean, rstd, gamma, beta, cpg):
    """[B, G] moments -> fp64 [B, C] scale = rstd gamma, shift = beta - mean scale"""
    sc = _d(gamma)[None, :] * rstd.repeat_interleave(cpg, dim=1)
    return sc, _d(beta)[None, :] - mean.repeat_interleave(cpg, dim=1) * sc


def gn_moments(x, groups=G, x2=None):
    """(mean, variance) fp64 [B, G] of the data, centred"""
    xin = cat_sources(x, x2)
    B, C = xin.shape[0], xin.shape[-1]
    xr = xin.reshape(B, -1, groups, C // groups)
    mean = xr.mean(dim=(1, 3))
    return mean, ((xr - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))


def _gn_pack(xin, ref, sc, sh):
    B, C = xin.shape[0], xin.shape[-1]
    A = _rms(xin.reshape(B, -1, C).abs() * sc.abs()[:, None, :] + sh.abs()[:, None, :])
    return {"ref": ref, "emul": _bf16(ref), "A": A}


def gn_expect(x, gamma, beta, eps, silu, x2=None, groups=G):
    """GroupNorm (+ SiLU) of the data: shadow_ref.ref_group_norm, its bf16 emulation and the scale/shift form's condition scale"""
    xin = cat_sources(x, x2)
    mean, var = gn_moments(x, groups, x2)
    sc, sh = _scale_shift(mean, 1.0 / torch.sqrt(var + eps), gamma, beta, xin.shape[-1] // groups)
    return _gn_pack(xin, SR.ref_group_norm(x, gamma, beta, groups, eps, silu, x2=x2), sc, sh)


def records(x, slots):
    """what a producer's epilogue would have emitted for x [B, HW, C]: fp32 [B * slots, C, 2] = (sum, sum of squares) per (row slot,
    channel), a sample's pixels cut into ``slots`` consecutive slots of ceil(HW / slots) rows (the last one short, trailing ones may be
    empty: zero records); summed in float64 and rounded once"""
    xd = _d(x)
    B, HW, C = xd.shape
    rows = -(-HW // slots)
    pad = torch.zeros((B, slots * rows - HW, C), dtype=torch.float64, device=xd.device)
    xs = torch.cat([xd, pad], dim=1).reshape(B, slots, rows, C)
    return torch.stack([xs.sum(2), (xs * xs).sum(2)], dim=-1).reshape(B * slots, C, 2).float().contiguous()


def _channel_sums(rec1, slots1, rec2=None, slots2=0, limit=None):
    """fp64 [B, C1 + C2, 2]: each channel's records summed over its source's slots (``limit``: only the first ``limit`` slots)"""
    out = []
    for rec, slots in ((rec1, slots1), (rec2, slots2)):
        if rec is not None:
            r = _d(rec).reshape(-1, slots, rec.shape[-2], 2)
            out.append(r[:, :slots if limit is None else min(slots, limit)].sum(1))
    return torch.cat(out, dim=1)


def _moments_of_sums(cs, HW, groups):
    """channel (sum, sum of squares) fp64 [B, C, 2] -> (mean, variance) [B, G] in the kernels' form q / n - mean^2, clamped at 0"""
    B, C, _ = cs.shape
    cpg = C // groups
    gs = cs.reshape(B, groups, cpg, 2).sum(2)
    n = float(HW) * cpg
    mean = gs[..., 0] / n
    return mean, (gs[..., 1] / n - mean * mean).clamp_min(0.0)


def table_from_records(rec1, slots1, gamma, beta, HW, eps, rec2=None, slots2=0, groups=G):
    """udt_gn_finalize from the GIVEN records: {"table": fp64 [B, C/64, 2, 64], "abs": sum|summands| of the same shape (scale: |sc|;
    shift: |beta| + |mean sc|), "sc" / "sh": fp64 [B, C]}"""
    cs = _channel_sums(rec1, slots1, rec2, slots2)
    B, C, _ = cs.shape
    cpg = C // groups
    mean, var = _moments_of_sums(cs, HW, groups)
    sc, sh = _scale_shift(mean, 1.0 / torch.sqrt(var + eps), gamma, beta, cpg)
    out = {"sc": sc, "sh": sh}
    if C % 64 == 0:
        blk = lambda t: t.reshape(B, C // 64, 64)
        out["table"] = torch.stack([blk(sc), blk(sh)], dim=2)
        out["abs"] = torch.stack([blk(sc.abs()), blk(_d(beta).abs()[None, :] + (mean.repeat_interleave(cpg, dim=1) * sc).abs())], dim=2)
    return out


def gn_expect_records(x, rec1, slots1, gamma, beta, eps, silu, x2=None, rec2=None, slots2=0, groups=G):
    """GroupNorm (+ SiLU) with the statistics of the given records: y = x sc + sh in float64"""
    xin = cat_sources(x, x2)
    t = table_from_records(rec1, slots1, gamma, beta, xin.shape[1], eps, rec2, slots2, groups)
    y = xin * t["sc"][:, None, :] + t["sh"][:, None, :]
    return _gn_pack(xin, _silu(y) if silu else y, t["sc"], t["sh"])


def chunk_rows(HW, nchunks):
    return -(-HW // nchunks)


def stats_partials(x, nchunks, x2=None, groups=G):
    """udt_gn_stats: (partials fp64 [B, nchunks, G, 2], sum|summands| of the same shape = (sum |x|, sum x^2)); chunk k owns pixels
    [k rows, (k + 1) rows) with rows = ceil(HW / nchunks), clipped at HW — trailing chunks can be empty"""
    xin = cat_sources(x, x2)
    B, HW, C = xin.shape
    rows = chunk_rows(HW, nchunks)
    pad = torch.zeros((B, nchunks * rows - HW, C), dtype=torch.float64, device=xin.device)
    xs = torch.cat([xin, pad], dim=1).reshape(B, nchunks, rows, groups, C // groups)
    sq = (xs * xs).sum(dim=(2, 4))
    return torch.stack([xs.sum(dim=(2, 4)), sq], dim=-1), torch.stack([xs.abs().sum(dim=(2, 4)), sq], dim=-1)


def ln_expect(x, gamma, beta, eps):
    xd = _d(x)
    ref = SR.ref_layer_norm(x, gamma, beta, eps)
    mean = xd.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(-1, keepdim=True) + eps)
    return {"ref": ref, "emul": _bf16(ref), "A": _rms((xd - mean).abs() * rstd * _d(gamma).abs() + _d(beta).abs())}


# ------------------------------------------------------------------------------------------------ float32 restatements
def _apply32(xin32, mean, var, gamma, beta, eps, silu, cpg):
    """gn_apply_kernel / gn_strip_kernel after the fp64 combine: rstd and mean rounded to fp32, sc = rstd * gamma, sh = beta - mean * sc,
    y = x * sc + sh (+ SiLU) in fp32, one rounding to bf16.  eps None: the planted 'eps omitted'"""
    rstd = (1.0 / torch.sqrt(var + (0.0 if eps is None else float(torch.tensor(eps, dtype=torch.float32))))).float()
    sc = rstd.repeat_interleave(cpg, dim=1) * gamma.float()[None, :]
    sh = beta.float()[None, :] - mean.float().repeat_interleave(cpg, dim=1) * sc
    y = xin32 * sc[:, None, :] + sh[:, None, :]
    return (_silu(y) if silu else y).bfloat16(), sc, sh


def _straddle_first_only(cs, C1, groups):
    """planted: the group that straddles C1 sums only the first source's channels"""
    cpg = cs.shape[1] // groups
    assert C1 % cpg != 0, "no group straddles C1"
    cs = cs.clone()
    cs[:, C1:(C1 // cpg + 1) * cpg] = 0
    return cs


def gn_two_kernel32(x, gamma, beta, eps, silu, nchunks, x2=None, groups=G, defect=None):
    """-> (y bf16 [B, HW, C], partials fp32 [B, nchunks, G, 2]).  defect: ("drop_last_pixel", b, chunk, cc) the statistics miss the last
    pixel of ``chunk`` for the 16-byte channel chunk cc; ("straddle_first_only",); ("no_eps",)"""
    xin = cat_sources(x, x2).float()
    B, HW, C = xin.shape
    cpg = C // groups
    rows = chunk_rows(HW, nchunks)
    pad = torch.zeros((B, nchunks * rows - HW, C), dtype=torch.float32, device=xin.device)
    xs = torch.cat([xin, pad], dim=1).reshape(B, nchunks, rows, C)
    s, q = xs.sum(2), (xs * xs).sum(2)                          # fp32 per (chunk, channel)
    kind = defect[0] if defect else None
    if kind == "drop_last_pixel":
        _, b, k, cc = defect
        last = min(HW, (k + 1) * rows) - 1
        v = xin[b, last, cc * 8:cc * 8 + 8]
        s[b, k, cc * 8:cc * 8 + 8] -= v
        q[b, k, cc * 8:cc * 8 + 8] -= v * v
    if kind == "straddle_first_only":
        keep = _straddle_first_only(torch.ones((1, C, 1), device=xin.device), x.shape[-1], groups)[0, :, 0]
        s, q = s * keep, q * keep
    part = torch.stack([s.reshape(B, nchunks, groups, cpg).sum(3), q.reshape(B, nchunks, groups, cpg).sum(3)], dim=-1)   # fp32 per group
    tot = part.double().sum(1)                                  # the fp64 combine over the chunks
    n = float(HW) * cpg
    mean = tot[..., 0] / n
    var = (tot[..., 1] / n - mean * mean).clamp_min(0.0)
    y, _, _ = _apply32(xin, mean, var, gamma, beta, None if kind == "no_eps" else eps, silu, cpg)
    return y, part


def strip_seam(HW, pstep):
    """lane 0's first pixel of gn_strip_kernel's tail loop (= 4 pstep x the number of its unrolled rounds)"""
    p = 0
    while p + 3 * pstep < HW:
        p += 4 * pstep
    return p


def gn_strip32(x, gamma, beta, eps, silu, gw, x2=None, groups=G, defect=None):
    """defect: ("double_seam", b, strip) the strip counts lane 0's first tail-loop pixel twice; ("straddle_first_only",)"""
    xin = cat_sources(x, x2).float()
    B, HW, C = xin.shape
    cpg = C // groups
    cw = gw * cpg
    pstep = STRIP_THREADS // (cw // 8)
    k = -(-HW // pstep)
    pad = torch.zeros((B, k * pstep - HW, C), dtype=torch.float32, device=xin.device)
    xs = torch.cat([xin, pad], dim=1).reshape(B, k, pstep, C)
    s, q = xs.sum(1), (xs * xs).sum(1)                          # fp32 per (pixel lane, channel)
    kind = defect[0] if defect else None
    if kind == "double_seam":
        _, b, strip = defect
        p = strip_seam(HW, pstep)
        assert p < HW, "no tail loop at this shape"
        v = xin[b, p, strip * cw:(strip + 1) * cw]
        s[b, p % pstep, strip * cw:(strip + 1) * cw] += v
        q[b, p % pstep, strip * cw:(strip + 1) * cw] += v * v
    cs = torch.stack([s.double().sum(1), q.double().sum(1)], dim=-1)      # fp64 per channel
    if kind == "straddle_first_only":
        cs = _straddle_first_only(cs, x.shape[-1], groups)
    mean, var = _moments_of_sums(cs, HW, groups)
    return _apply32(xin, mean, var, gamma, beta, eps, silu, cpg)[0]


def gn_records32(x, rec1, slots1, gamma, beta, eps, silu, x2=None, rec2=None, slots2=0, groups=G, defect=None):
    """-> (y bf16, table fp32 [B, C/64, 2, 64] or None when C % 64 != 0).  defect: ("lanes_only",) only the first 256 / cpg records of a
    channel are summed; ("table_neighbour", b, c) channel c's table entry lands at c % 64 of the next 64-channel block"""
    xin = cat_sources(x, x2).float()
    B, HW, C = xin.shape
    cpg = C // groups
    kind = defect[0] if defect else None
    cs = _channel_sums(rec1, slots1, rec2, slots2, limit=256 // cpg if kind == "lanes_only" else None)
    mean, var = _moments_of_sums(cs, HW, groups)
    y, sc, sh = _apply32(xin, mean, var, gamma, beta, eps, silu, cpg)
    table = None
    if C % 64 == 0:
        table = torch.stack([sc.reshape(B, C // 64, 64), sh.reshape(B, C // 64, 64)], dim=2)
        if kind == "table_neighbour":
            _, b, c = defect
            table[b, c // 64 + 1, :, c % 64] = table[b, c // 64, :, c % 64]
            table[b, c // 64, :, c % 64] = 0
            sc, sh = table[:, :, 0].reshape(B, C), table[:, :, 1].reshape(B, C)
            y = xin * sc[:, None, :] + sh[:, None, :]
            y = (_silu(y) if silu else y).bfloat16()
    return y, table


def layer_norm32(x, gamma, beta, eps, defect=None):
    """defect: ("skip_second_chunk", row) the row's mean leaves out the channels of lane chunks >= 64 (channels 512 ..); ("no_eps",)"""
    v = x.float()
    C = v.shape[-1]
    s = v.sum(-1, keepdim=True)
    kind = defect[0] if defect else None
    if kind == "skip_second_chunk":
        s[defect[1]] = v[defect[1], :512].sum()
    mean = s / C
    d = v - mean
    q = (d * d).sum(-1, keepdim=True)
    rstd = torch.rsqrt(q / C + (0.0 if kind == "no_eps" else eps))
    return (d * rstd * gamma.float() + beta.float()).bfloat16()
