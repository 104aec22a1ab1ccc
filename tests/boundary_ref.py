"""Exact-bit and float64 restatements of the plugin-boundary kernels (csrc/elementwise.hip, the forward score of csrc/backward.hip) and
of the device packers (csrc/pack.hip) — a helper, not a test; plain torch on the CPU, plain index loops where a layout is an index
formula.  Nothing here comes from udifftext_amd.packing or udifftext_amd.ops: these are the definitions those two are held to.

Bit-exact results are integers: ``bf16_rne_bits`` rounds an fp32 value to bf16 on its bit pattern (round to nearest, ties to even; a NaN
stays a NaN of any payload), ``e4m3_bytes`` gives the OCP e4m3 byte.  fp32 subnormals are outside every definition here (the device
may flush them) and no input holds one.

Bounded results come with the float64 value and the magnitude their bound multiplies:
  posterior64       scale (mean + exp(0.5 clamp(logvar, -30, 20)) noise)  with  |scale| (|mean| + s |noise|)
  timestep64        [cos(t f_k) | sin(t f_k)], f_k = exp(-fp32(ln 10000) k / half)  with  |t f_k| + 1
  mask_downsample64 mean of the centre 2x2 of every 8x8 block  with  0.25 sum|taps|
  local_loss64      loss0 - min_l(max_n(mask_n blur3x3(mean_h p)) + 1 - seg_l)  with the largest per-pixel sum of absolute summands
"""
import math

import torch

LN_10000_F32 = float(torch.tensor(9.210340371976184, dtype=torch.float32))      # the constant as the kernel holds it
FP8_MAX = 448.0


# ------------------------------------------------------------------------------------------------ bits
def f32_bits(x):
    return x.contiguous().view(torch.int32).long() & 0xffffffff


def f32_from_bits(bits):
    b = torch.as_tensor(bits, dtype=torch.int64)
    return torch.where(b >= 2 ** 31, b - 2 ** 32, b).int().view(torch.float32)


def bf16_bits(t):
    """the 16-bit codes of a torch.bfloat16 tensor"""
    return t.contiguous().view(torch.int16).long() & 0xffff


def bf16_value(bits):
    """bf16 codes -> the fp32 values they widen to"""
    return f32_from_bits(torch.as_tensor(bits, dtype=torch.int64) << 16)


def bf16_is_nan(bits):
    return (bits & 0x7fff) > 0x7f80


def bf16_rne_bits(x):
    """fp32 -> bf16 code, round to nearest even, on the bit pattern: the upper half after adding 0x7fff + the kept half's lowest bit.
    The largest finite fp32 carries into the exponent and becomes Inf; a NaN becomes the code 0x7fc0 (compare with ``same_bf16``)"""
    assert x.dtype == torch.float32
    u = f32_bits(x)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    return torch.where(torch.isnan(x), torch.full_like(r, 0x7fc0), r)


def same_bf16(got_bits, want_bits):
    """element-wise: equal codes, or a NaN where a NaN is wanted"""
    return torch.where(bf16_is_nan(want_bits), bf16_is_nan(got_bits), got_bits == want_bits)


def bf16_rne_f64(x):
    """float64 -> the nearest bf16 value (ties to even) in one rounding, as float64; normal range only"""
    m, e = torch.frexp(x)                                                      # x = m 2^e, 0.5 <= |m| < 1: 8 significant bits -> quantum 2^(e-8)
    q = torch.ldexp(torch.ones_like(x), e - 8)
    return torch.round(x / q) * q                                              # torch.round: half to even; x / q is exact


# the values every bit-exact kernel is given: both zeros, both infinities, a NaN, ties between two bf16 neighbours with an even (0x3f80)
# and an odd (0x3f81) lower neighbour in both signs, one fp32 ulp on either side of each tie, the largest finite fp32 in both signs
SPECIAL_BITS = (0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000,
                0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000,
                0x3f807fff, 0x3f808001, 0x3f817fff, 0x3f818001, 0xbf807fff, 0xbf808001, 0xbf817fff, 0xbf818001,
                0x7f7fffff, 0xff7fffff)


def specials():
    return f32_from_bits(list(SPECIAL_BITS))


# ------------------------------------------------------------------------------------------------ layout kernels
def nchw_to_nhwc(x, cpad, scale):
    """x fp32 [B, C, HW] -> bf16 codes [B, HW, cpad]: bf16_rne(fp32(x) * fp32(scale)), channels >= C are +0"""
    B, C, HW = x.shape
    out = torch.zeros((B, HW, cpad), dtype=torch.int64)
    s = torch.tensor(scale, dtype=torch.float32)
    for c in range(C):
        out[:, :, c] = bf16_rne_bits(x[:, c, :] * s)
    return out


def nhwc_to_nchw(src_bits, C):
    """the first C of ld columns of [B, HW, ld], as the 32-bit patterns of the fp32 result [B, C, HW] (src_bits: fp32 patterns, or bf16
    codes << 16 for a bf16 source): a copy"""
    B, HW, ld = src_bits.shape
    out = torch.empty((B, C, HW), dtype=torch.int64)
    for c in range(C):
        out[:, c, :] = src_bits[:, :, c]
    return out


def set_channels(src, dst_bits, c0):
    """src fp32 [B, C, HW] into channels [c0, c0 + C) of bf16 codes [B, HW, cpad]; every other channel keeps its bits"""
    out = dst_bits.clone()
    for c in range(src.shape[1]):
        out[:, :, c0 + c] = bf16_rne_bits(src[:, c, :])
    return out


def embed_tokens(idx, table, pe):
    """bf16_rne(fp32(table[idx[i]] + pe[i % L])), one token at a time"""
    n_tok, L, D = idx.shape[0], pe.shape[0], pe.shape[1]
    out = torch.empty((n_tok, D), dtype=torch.int64)
    for i in range(n_tok):
        out[i] = bf16_rne_bits(table[int(idx[i])] + pe[i % L])
    return out


def add_bf16(a_bits, b_bits):
    return bf16_rne_bits(bf16_value(a_bits) + bf16_value(b_bits))


def bias_add_bf16(x_bits, bias):
    """x bf16 codes [rows, C] + bias fp32 [C]"""
    return bf16_rne_bits(bf16_value(x_bits) + bias[None, :])


def mask_downsample64(m):
    """m [B, H, W] -> (mean of the centre 2x2 of every 8x8 block [B, H/8, W/8] in float64, 0.25 sum|taps|)"""
    B, H, W = m.shape
    ref = torch.zeros((B, H // 8, W // 8), dtype=torch.float64)
    ab = torch.zeros_like(ref)
    md = m.double()
    for oy in range(H // 8):
        for ox in range(W // 8):
            taps = md[:, 8 * oy + 3:8 * oy + 5, 8 * ox + 3:8 * ox + 5]
            ref[:, oy, ox] = taps.sum(dim=(1, 2)) / 4
            ab[:, oy, ox] = taps.abs().sum(dim=(1, 2)) / 4
    return ref, ab


# ------------------------------------------------------------------------------------------------ kernels with a bound
def posterior64(mom, noise, scale):
    """mom fp32 [B, hw, ldm] (mean 0..3, logvar 4..7), noise fp32 [B, 4, hw] -> (z float64 [B, 4, hw], |scale| (|mean| + s |noise|))"""
    sc = float(torch.tensor(scale, dtype=torch.float32))
    mean = mom[:, :, 0:4].double().permute(0, 2, 1)
    s = torch.exp(0.5 * mom[:, :, 4:8].double().permute(0, 2, 1).clamp(-30.0, 20.0))
    return sc * (mean + s * noise.double()), abs(sc) * (mean.abs() + s * noise.double().abs())


def timestep64(t, dim):
    """t fp32 [n] -> (float64 [n, dim] = [cos | sin](t f_k), |t f_k| + 1 in the same layout)"""
    half = dim // 2
    f = torch.exp(-LN_10000_F32 * torch.arange(half, dtype=torch.float64) / half)
    arg = t.double()[:, None] * f[None, :]
    mag = arg.abs() + 1.0
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=1), torch.cat([mag, mag], dim=1)


def timestep_interval(t, dim, U):
    """the bf16 values a result may take: [bf16_rne(ref - delta), bf16_rne(ref + delta)], delta = U 2^-24 (|t f_k| + 1)"""
    ref, mag = timestep64(t, dim)
    delta = U * 2.0 ** -24 * mag
    return bf16_rne_f64(ref - delta), bf16_rne_f64(ref + delta)


def nearest_index(n_out, n_in):
    """F.interpolate(mode="nearest") per axis: src = floor(dst * in / out)"""
    return [(d * n_in) // n_out for d in range(n_out)]


def blur3x3_zero_padded(a, gk):
    """a [..., size, size] float64, gk [9]: out[y, x] = sum_{dy, dx} gk[3 (dy + 1) + dx + 1] a[y + dy, x + dx], zero outside the map"""
    size = a.shape[-1]
    p = torch.zeros(a.shape[:-2] + (size + 2, size + 2), dtype=a.dtype)
    p[..., 1:-1, 1:-1] = a
    out = torch.zeros_like(a)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out += gk[3 * (dy + 1) + dx + 1] * p[..., 1 + dy:1 + dy + size, 1 + dx:1 + dx + size]
    return out


def local_loss64(probs, mask, seg, gk, loss0, mask_batch, heads, size):
    """probs [n_samples * heads, size^2, L], mask [mask_batch, Hm, Wm], seg [mask_batch, seg_l], gk [9], loss0 [n_samples]
    -> (loss0 + the term in float64 [n_samples], the largest per-pixel sum of absolute summands [n_samples])"""
    n_samples, L = probs.shape[0] // heads, probs.shape[2]
    seg_l, Hm, Wm = seg.shape[1], mask.shape[1], mask.shape[2]
    p = probs.double().reshape(n_samples, heads, size, size, L)
    my, mx = nearest_index(size, Hm), nearest_index(size, Wm)
    ref = torch.empty(n_samples, dtype=torch.float64)
    mag = torch.empty(n_samples, dtype=torch.float64)
    for b in range(n_samples):
        bm = b % mask_batch
        mm = mask[bm].double()[my][:, mx]                                      # [size, size]
        best, worst = math.inf, 0.0
        for l in range(seg_l):
            amap = p[b, :, :, :, l].sum(0) / heads
            amag = p[b, :, :, :, l].abs().sum(0) / heads
            val = mm * blur3x3_zero_padded(amap, gk.double())
            vmag = mm.abs() * blur3x3_zero_padded(amag, gk.double().abs())
            best = min(best, float(val.max()) + 1.0 - float(seg[bm, l]))
            worst = max(worst, float(vmag.max()) + 1.0 + abs(float(seg[bm, l])))
        ref[b] = float(loss0[b]) - best
        mag[b] = worst
    return ref, mag


# ------------------------------------------------------------------------------------------------ packed weights
def _round_up(v, m):
    return (v + m - 1) // m * m


def geglu_source_row(n, N):
    """source row of packed row n of a GEGLU projection [2 inner, K]: packed rows come in blocks of 64 = [32 value rows | the 32 gate
    rows that belong to them]; value rows are source rows [0, inner), gate rows [inner, 2 inner)"""
    inner, blk, r = N // 2, n // 64, n % 64
    return blk * 32 + r if r < 32 else inner + blk * 32 + (r - 32)


_E4M3_TABLE = None


def e4m3_table():
    """the 128 non-negative codes' values: code = e << 3 | m; e = 0: m 2^-9, else (1 + m / 8) 2^(e - 7); 0x7f is the NaN"""
    global _E4M3_TABLE
    if _E4M3_TABLE is None:
        v = [(m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7) for e in range(16) for m in range(8)]
        _E4M3_TABLE = torch.tensor(v[:127], dtype=torch.float64)              # 0x00 .. 0x7e = 448
    return _E4M3_TABLE


def e4m3_bytes_by_table(x):
    """|x| <= 448 fp32 -> OCP e4m3 byte, nearest value, a tie to the even code; NaN -> 0x7f"""
    tab = e4m3_table()
    a = x.double().abs().reshape(-1)
    hi = torch.searchsorted(tab, a).clamp(1, 126)                             # tab[hi - 1] <= a <= tab[hi] (a = 0 -> hi = 1)
    lo = hi - 1
    dl, dh = a - tab[lo], tab[hi] - a
    code = torch.where(dl < dh, lo, torch.where(dh < dl, hi, torch.where(lo % 2 == 0, lo, hi)))
    code = torch.where(torch.isnan(a), torch.full_like(code, 0x7f), code)
    sign = (f32_bits(x.float()).reshape(-1) >> 31) & 1
    return (code | (sign << 7)).reshape(x.shape)


def e4m3_bytes(x):
    """torch's float8_e4m3fn cast where this torch has it, else the table"""
    if hasattr(torch, "float8_e4m3fn"):
        return x.float().to(torch.float8_e4m3fn).view(torch.uint8).long()
    return e4m3_bytes_by_table(x)


def fp8_scale(w):
    """per row: max(amax, 1e-12) * fp32(1 / 448), in fp32"""
    amax = w.abs().amax(dim=1)
    return torch.maximum(amax, torch.tensor(1e-12, dtype=torch.float32)) * torch.tensor(1.0 / FP8_MAX, dtype=torch.float32)


def pack_bias(bias, N, Npad, geglu=False):
    out = torch.zeros(Npad, dtype=torch.float32)
    if bias is not None:
        for n in range(N):
            out[n] = bias[geglu_source_row(n, N) if geglu else n]
    return out


def pack_linear(w, bias, fp8=False, geglu=False):
    """w fp32 [N, K] -> {"dims": (N, Npad, K, Kpad), "weight": bf16 codes or e4m3 bytes [Npad, Kpad], "bias": fp32 [Npad],
    "colscale": fp32 [Npad] or None}: N padded to 4, K to 64 (bf16) or 128 (e4m3) with zeros; padding rows have colscale 1"""
    N, K = w.shape
    Npad, Kpad = _round_up(N, 4), _round_up(K, 128 if fp8 else 64)
    src = torch.stack([w[geglu_source_row(n, N) if geglu else n] for n in range(N)])
    weight = torch.zeros((Npad, Kpad), dtype=torch.int64)
    colscale = None
    if fp8:
        scale = fp8_scale(src)
        colscale = torch.ones(Npad, dtype=torch.float32)
        colscale[:N] = scale
        weight[:N, :K] = e4m3_bytes((src / scale[:, None]).clamp(-FP8_MAX, FP8_MAX))
    else:
        weight[:N, :K] = bf16_rne_bits(src)
    return {"dims": (N, Npad, K, Kpad), "weight": weight, "bias": pack_bias(bias, N, Npad, geglu), "colscale": colscale}


def pack_conv(w, bias, segments, n_pad_to):
    """w fp32 [N, Cin, kh, kw] -> bf16 codes [Npad, kh kw Cpad], column (ky kw + kx) Cpad + c'; the concatenated sources of ``segments``
    (None: one source of Cin channels) are padded to 64 channels each, c' counts through the padded sources; N padded to n_pad_to"""
    N, Cin, kh, kw = w.shape
    segs = [Cin] if not segments else list(segments)
    assert sum(segs) == Cin
    Cpad, Npad = sum(_round_up(s, 64) for s in segs), _round_up(N, n_pad_to)
    weight = torch.zeros((Npad, kh * kw * Cpad), dtype=torch.int64)
    for ky in range(kh):
        for kx in range(kw):
            col, c0 = (ky * kw + kx) * Cpad, 0
            for s in segs:
                weight[:N, col:col + s] = bf16_rne_bits(w[:, c0:c0 + s, ky, kx].contiguous())
                col, c0 = col + _round_up(s, 64), c0 + s
    return {"dims": (N, Npad, kh * kw * Cpad, kh * kw * Cpad), "weight": weight, "bias": pack_bias(bias, N, Npad), "colscale": None}
