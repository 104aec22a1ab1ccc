"""Case lists, inputs and the ``case_*`` checks of the plugin-boundary kernels (csrc/elementwise.hip, udt_local_loss_tiled_hw of
csrc/backward.hip) and the device packers (csrc/pack.hip) — a helper, not a test; shared by tests/test_boundary_ref_cpu.py (float32
restatements, mutants) and tests/test_boundary_edges_gpu.py (the kernels).

A ``case_*`` function builds its inputs on the CPU, calls ``impl`` (the code under test: CPU tensors in, CPU tensors out) and holds the
result to tests/boundary_ref.py: integers for the results that are defined to the last bit, tests/sliced_check.py's check_fp32_sum for
the bounded ones.  One line per check goes to ``report``.

Inputs of the bit-exact kernels carry boundary_ref.SPECIAL_BITS at their first and last elements (as many as fit).  No input holds an
fp32 subnormal: the device may flush them, they are outside what is defined here.

The units of the two bounds that are not known in advance, measured on the CPU (tests/test_boundary_ref_cpu.py
test_measured_units_are_the_recorded_ones: the worst |float32 torch evaluation - float64| over 2^-24 x magnitude on these very inputs),
times 4 and not below 4 — the margin for a device expf / sinf / cosf and a contraction that differ from the host's; never from a
GPU result:
  udt_posterior_sample     measured 2.92  ->  U = 11.68
  udt_timestep_embedding   measured 4.41  ->  U = 17.64   (the exponent's own rounding, up to 9.2 x 2^-24, is multiplied by t f_k)
(both figures rounded up to two decimals)
"""
import math

import torch

import boundary_ref as R
import sliced_check as S

POSTERIOR_MEASURED, TIMESTEP_MEASURED = 2.92, 4.41
U_POSTERIOR = max(4.0, 4.0 * POSTERIOR_MEASURED)
U_TIMESTEP = max(4.0, 4.0 * TIMESTEP_MEASURED)

SCALES = (1.0, 0.18215)
NCHW_TO_NHWC = ((1, 1, 1, 8), (2, 9, 5, 16), (3, 4, 257, 8), (1, 8, 1, 8), (2, 17, 3, 24))         # (B, C, HW, cpad)
NHWC_TO_NCHW = ((1, 1, 1, 1), (2, 4, 5, 8), (3, 3, 257, 5))                                        # (B, C, HW, ld)
SET_CHANNELS = ((5, 3, 16), (13, 3, 16), (0, 1, 3))                                                # (c0, C, cpad)
SET_HW, SET_B = (1, 257), 3
EMBED = ((1, 1, 2), (7, 3, 6), (5, 5, 258), (24, 12, 256))                                         # (n_tok, L, D)
EMBED_V = 95
ADD_N = (8, 8 * 257)
BIAS_ADD = ((1, 8), (3, 40), (65, 24))                                                             # (rows, C)
MASK = ((1, 8, 8), (3, 8, 24), (2, 24, 8), (2, 16, 40))                                            # (B, H, W)
LINEAR = ((1, 1), (3, 63), (4, 64), (5, 65), (66, 129))                                            # (N, K)
GEGLU_N = (64, 192)
FP8_K = (1, 127, 129)
CONV_SEGMENTS = (None, (1,), (64,), (65, 63), (3, 200, 1))
CONV_TAPS = ((1, 1), (3, 3), (1, 7))
CONV_NPAD = (4, 64)
CONV_N = (1, 5, 130)
POSTERIOR = ((1, 1), (3, 5), (2, 257))                                                             # (B, hw)
POSTERIOR_LDM = (8, 12)
POSTERIOR_SCALES = (0.18215, -2.5)
LOGVARS = (-40.0, -30.0, 0.0, 20.0, 25.0)
TIMESTEP_DIM = (2, 6, 320)
TIMESTEP_N = (1, 4, 130)
TIMESTEPS = (0.0, 0.5, 19.0, 999.0, 0.25 * math.log(0.002), 0.25 * math.log(80.0), -0.3125)
# (size, Hm, Wm, heads, L, seg_l, n_samples, mask_batch, mask kind)
LOCAL_LOSS = ((1, 8, 8, 1, 1, 1, 1, 1, "random"), (2, 3, 5, 5, 12, 5, 2, 2, "random"), (3, 64, 64, 5, 12, 12, 6, 2, "random"),
              (17, 50, 20, 2, 4, 3, 3, 1, "random"), (17, 8, 8, 5, 12, 1, 2, 2, "random"), (120, 120, 120, 1, 2, 2, 1, 1, "random"),
              (17, 50, 20, 2, 4, 3, 2, 2, "zero"), (17, 8, 8, 2, 4, 3, 2, 2, "corner"))
LOCAL_LOSS_REFUSED_SIZE = 121


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return torch.randn(shape, generator=g) * scale


def plant(t, values=None):
    """``values`` (default: the special values) over the first elements of ``t`` and, reversed, over the last ones; as many as fit"""
    v = R.specials() if values is None else values
    flat = t.reshape(-1)
    k = min(flat.numel(), v.numel())
    if flat.numel() >= 2 * v.numel():
        flat[-v.numel():] = v.flip(0)
    flat[:k] = v[:k]
    return t


# ------------------------------------------------------------------------------------------------ the checks
def hold_bits(name, got_bits, want_bits, report=None, nan_class=True):
    """integer comparison, no tolerance; nan_class: a NaN of any payload where a NaN is wanted (a rounding), else every bit (a copy)"""
    got_bits, want_bits = torch.as_tensor(got_bits).long(), torch.as_tensor(want_bits).long()
    assert got_bits.shape == want_bits.shape, f"{name}: shapes {tuple(got_bits.shape)} {tuple(want_bits.shape)}"
    ok = R.same_bf16(got_bits, want_bits) if nan_class else got_bits == want_bits
    bad = int((~ok).sum())
    at = tuple(int(i) for i in torch.unravel_index((~ok).int().argmax(), ok.shape)) if bad else ()
    S._report(f"{name:55s} bits: " + (f"equal ({ok.numel()} values)" if not bad else f"{bad} of {ok.numel()} differ, first at {at}  FAIL"), report)
    assert not bad, f"{name}: {bad} of {ok.numel()} values differ; first at {at}: got {int(got_bits[at]):#x}, want {int(want_bits[at]):#x}"
    return 0.0


def hold_interval(name, got, t, dim, U, report=None):
    """a bf16 timestep embedding: every element inside [bf16_rne(ref - delta), bf16_rne(ref + delta)].  Reports the units the result
    needs: 0 where it is the rounded reference, else the distance from the reference to the result's rounding interval"""
    g = got.double()
    lo, hi = R.timestep_interval(t, dim, U)
    ref, mag = R.timestep64(t, dim)
    assert g.shape == ref.shape and bool(torch.isfinite(g).all()), f"{name}: shape or non-finite values"
    _, e = torch.frexp(g)
    half_ulp = torch.ldexp(torch.ones_like(g), e - 9)
    need = torch.where(g == R.bf16_rne_f64(ref), torch.zeros_like(g), ((g - ref).abs() - half_ulp).clamp_min(0) / (2.0 ** -24 * mag))
    bad = (g < lo) | (g > hi)
    worst = float(need.max())
    at = tuple(int(i) for i in torch.unravel_index(need.argmax(), need.shape))
    S._report(f"{name:55s} interval: " + ("equal" if worst == 0 else f"worst {worst:.2f} x 2^-24 at {at}, {worst / U:.3f} of U = {U:g}")
              + ("  FAIL" if bool(bad.any()) else ""), report)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the interval; worst needs {worst:.2f} units "
                                 f"at {at}: got {float(g[at]):.9g}, ref {float(ref[at]):.9g}")
    return worst


# ------------------------------------------------------------------------------------------------ layout kernels
def case_nchw_to_nhwc(shape, scale, impl, report=None):
    """impl(x fp32 [B, C, HW], cpad, scale) -> bf16 [B, HW, cpad]"""
    B, C, HW, cpad = shape
    x = plant(_randn((B, C, HW), _gen(1, *shape), 3.0))
    return hold_bits(f"edge nchw_to_nhwc B{B} C{C} HW{HW} cpad{cpad} scale{scale:g}", R.bf16_bits(impl(x, cpad, scale)),
                     R.nchw_to_nhwc(x, cpad, scale), report)


def case_nhwc_to_nchw(shape, src_f32, impl, report=None):
    """impl(src [B, HW, ld] fp32 or bf16, C) -> fp32 [B, C, HW]; the columns past C hold 1e30 / NaN"""
    B, C, HW, ld = shape
    x = plant(_randn((B, HW, C), _gen(2, *shape), 3.0))
    src = torch.full((B, HW, ld), 1e30)
    src[:, 0::2, C:] = float("nan")
    src[:, :, :C] = x
    if src_f32:
        bits = R.f32_bits(src)
    else:
        src = src.bfloat16()
        bits = R.bf16_bits(src) << 16
    got = impl(src, C)
    return hold_bits(f"edge nhwc_to_nchw B{B} C{C} HW{HW} ld{ld} {'fp32' if src_f32 else 'bf16'}", R.f32_bits(got), R.nhwc_to_nchw(bits, C),
                     report, nan_class=False)


def case_set_channels(spec, HW, impl, report=None):
    """impl(src fp32 [B, C, HW], dst bf16 [B, HW, cpad], c0) -> dst afterwards"""
    c0, C, cpad = spec
    g = _gen(3, *spec, HW)
    src = plant(_randn((SET_B, C, HW), g, 3.0))
    dst = _randn((SET_B, HW, cpad), g, 3.0).bfloat16()
    return hold_bits(f"edge nhwc_set_channels c0{c0} C{C} cpad{cpad} HW{HW}", R.bf16_bits(impl(src, dst.clone(), c0)),
                     R.set_channels(src, R.bf16_bits(dst), c0), report)


def embed_inputs(n_tok, L, D):
    """ids with 0 and V - 1, a table whose rows differ in every element, and — special value s at (token s % n_tok, column s) while
    columns last — table and pe entries whose fp32 sum IS the special value (1 + (s - 1), or s + 0)"""
    g = _gen(4, n_tok, L, D)
    idx = torch.randint(0, EMBED_V, (n_tok,), generator=g, dtype=torch.int32)
    idx[-1] = 0
    idx[0] = EMBED_V - 1                                                       # (a single token takes the last row)
    table = _randn((EMBED_V, D), g) + 0.03125 * torch.arange(EMBED_V, dtype=torch.float32)[:, None]
    pe = _randn((L, D), g)
    sp = R.specials()
    for s in range(min(D, sp.numel())):
        tok = s % n_tok
        v = sp[s]
        near_one = bool(torch.isfinite(v)) and 0.5 < abs(float(v)) < 2.0
        base = math.copysign(1.0, float(v)) if near_one else float(v)
        table[int(idx[tok]), s] = base
        pe[tok % L, s] = (v - base) if near_one else math.copysign(0.0, float(v)) if bool(torch.isfinite(v)) else 0.0
    return idx, table, pe


def case_embed(shape, impl, report=None):
    """impl(idx int32 [n_tok], table fp32 [V, D], pe fp32 [L, D]) -> bf16 [n_tok, D]"""
    idx, table, pe = embed_inputs(*shape)
    return hold_bits("edge embed_tokens n_tok%d L%d D%d" % shape, R.bf16_bits(impl(idx, table, pe)), R.embed_tokens(idx, table, pe), report)


def special_parts():
    """the special values split as hi + lo: hi the bf16 truncation (exact in bf16), lo the fp32 rest (0 beside Inf and NaN).  hi + lo is
    the special value in fp32; lo rounded to bf16 still gives the ties (2^-8 beside 1), not the values one ulp off them"""
    sp = R.specials()
    hi = R.f32_from_bits(R.f32_bits(sp) & 0xffff0000)
    return hi, torch.where(torch.isfinite(sp), sp - hi, torch.zeros_like(sp))


def add_inputs(n):
    """bf16 pairs: random ones, and at both ends the parts of the special values as far as bf16 holds them"""
    g = _gen(5, n)
    a, b = _randn((n,), g, 3.0).bfloat16(), _randn((n,), g, 3.0).bfloat16()
    hi, lo = special_parts()
    k = min(n, hi.numel())
    a[:k], b[:k] = hi[:k].bfloat16(), lo[:k].bfloat16()
    if n >= 2 * hi.numel():
        a[-hi.numel():], b[-hi.numel():] = lo.bfloat16(), hi.bfloat16()
    return a, b


def case_add(n, impl, report=None):
    """impl(a bf16 [n], b bf16 [n]) -> a + b bf16 (the kernel's in-place result)"""
    a, b = add_inputs(n)
    return hold_bits(f"edge add_bf16 n{n}", R.bf16_bits(impl(a.clone(), b)), R.add_bf16(R.bf16_bits(a), R.bf16_bits(b)), report)


def case_bias_add(shape, inplace, impl, report=None):
    """impl(x bf16 [rows, C], bias fp32 [C], inplace) -> bf16 [rows, C]; row 0 plus the bias gives the special values exactly (the bias
    is fp32 and holds their low parts unrounded)"""
    rows, C = shape
    g = _gen(6, rows, C)
    x, bias = _randn((rows, C), g, 3.0).bfloat16(), _randn((C,), g)
    hi, lo = special_parts()
    k = min(C, hi.numel())
    x[0, :k], bias[:k] = hi[:k].bfloat16(), lo[:k]
    return hold_bits(f"edge bias_add_bf16 rows{rows} C{C} {'in place' if inplace else 'out of place'}", R.bf16_bits(impl(x.clone(), bias, inplace)),
                     R.bias_add_bf16(R.bf16_bits(x), bias), report)


def centre_taps(H, W):
    m = torch.zeros((H, W), dtype=torch.bool)
    for dy in (3, 4):
        for dx in (3, 4):
            m[dy::8, dx::8] = True
    return m


def case_mask_downsample(shape, impl, report=None):
    """impl(mask fp32 [B, H, W]) -> fp32 [B, H/8, W/8]: a binary mask (exact), the same with 1e30 in every pixel that is no centre tap
    (the same bits), a real-valued one (check_fp32_sum)"""
    B, H, W = shape
    g = _gen(7, *shape)
    binary = (torch.rand((B, H, W), generator=g) > 0.5).float()
    name = f"edge mask_downsample B{B} H{H} W{W}"
    ref, _ = R.mask_downsample64(binary)
    got = impl(binary)
    hold_bits(name + " binary", R.f32_bits(got), R.f32_bits(ref.float()), report, nan_class=False)
    assert bool((got.double() == ref).all())
    poisoned = torch.where(centre_taps(H, W)[None], binary, torch.full_like(binary, 1e30))
    hold_bits(name + " poisoned", R.f32_bits(impl(poisoned)), R.f32_bits(ref.float()), report, nan_class=False)
    real = _randn((B, H, W), g)
    return S.check_fp32_sum(name + " real", impl(real), *R.mask_downsample64(real), report=report)


# ------------------------------------------------------------------------------------------------ packed weights
def hold_packed(name, got, want, report=None):
    assert tuple(got["dims"]) == tuple(want["dims"]), f"{name}: dims {got['dims']}, want {want['dims']}"
    hold_bits(name + " weight", got["weight"], want["weight"], report, nan_class=want["colscale"] is None)
    hold_bits(name + " bias", R.f32_bits(got["bias"]), R.f32_bits(want["bias"]), report, nan_class=False)
    assert (got["colscale"] is None) == (want["colscale"] is None), f"{name}: colscale"
    if want["colscale"] is not None:
        hold_bits(name + " colscale", R.f32_bits(got["colscale"]), R.f32_bits(want["colscale"]), report, nan_class=False)
    return 0.0


def linear_inputs(N, K, fp8):
    g = _gen(8, N, K, fp8)
    w = _randn((N, K), g)
    if fp8:
        w *= torch.exp(_randn((N, 1), g, 2.0))                                 # rows of very different magnitude
        if N > 1:
            w[1] = 0.0                                                         # an all-zero row
        if N > 2:
            w[2] = 0.0
            w[2, K // 2] = -3.7                                                # amax in a single element
    else:
        plant(w)
    return w, _randn((N,), g)


def linear_cases():
    """(N, K, fp8, geglu, with_bias) of every udt_pack_linear case"""
    for N, K_ in LINEAR:
        for with_bias in (True, False):
            yield N, K_, False, False, with_bias
    for N in GEGLU_N:
        yield N, 65, False, True, True
        yield N, 129, True, True, True
    for K_ in FP8_K:
        yield 5, K_, True, False, True
        yield 66, K_, True, False, False


def conv_cases(segments):
    """(N, segments, taps, n_pad_to, with_bias) of every udt_pack_conv case over ``segments``"""
    for taps in CONV_TAPS:
        for n_pad_to in CONV_NPAD:
            for N in CONV_N:
                for with_bias in (False, True):
                    yield N, segments, taps, n_pad_to, with_bias


def case_pack_linear(N, K, fp8, geglu, with_bias, impl, report=None):
    """impl(w fp32 [N, K], bias fp32 [N] or None, fp8, geglu) -> {"dims", "weight" codes / bytes, "bias", "colscale"}"""
    w, bias = linear_inputs(N, K, fp8)
    bias = bias if with_bias else None
    name = f"edge pack_linear {'e4m3' if fp8 else 'bf16'}{' geglu' if geglu else ''} N{N} K{K}{'' if with_bias else ' no bias'}"
    return hold_packed(name, impl(w, bias, fp8, geglu), R.pack_linear(w, bias, fp8, geglu), report)


def conv_inputs(N, segments, taps, Cin_default=5):
    Cin = sum(segments) if segments else Cin_default
    g = _gen(9, N, Cin, *taps)
    return plant(_randn((N, Cin, taps[0], taps[1]), g)), _randn((N,), g)


def case_pack_conv(N, segments, taps, n_pad_to, with_bias, impl, report=None):
    """impl(w fp32 [N, Cin, kh, kw], bias or None, segments or None, n_pad_to) -> as case_pack_linear"""
    w, bias = conv_inputs(N, segments, taps)
    bias = bias if with_bias else None
    name = f"edge pack_conv N{N} segs{'-'.join(map(str, segments)) if segments else 'none'} {taps[0]}x{taps[1]} pad{n_pad_to}" \
           f"{'' if with_bias else ' no bias'}"
    return hold_packed(name, impl(w, bias, segments, n_pad_to), R.pack_conv(w, bias, segments, n_pad_to), report)


# ------------------------------------------------------------------------------------------------ kernels with a bound
def posterior_inputs(B, hw, ldm):
    """moments [B, hw, ldm] with LOGVARS cycled through the logvar channels (the mean beside a -40 is 0, so that the lower clamp shows),
    columns past 8 poisoned; noise [B, 4, hw]"""
    g = _gen(10, B, hw, ldm)
    mom = torch.full((B, hw, ldm), 1e30)
    mom[:, 1::2, 8:] = float("nan")
    mom[:, :, 0:4] = _randn((B, hw, 4), g, 3.0)
    lv = _randn((B, hw, 4), g, 8.0)
    flat = lv.reshape(-1)
    k = torch.arange(0, flat.numel(), 3)
    flat[k] = torch.tensor(LOGVARS)[torch.arange(k.numel()) % len(LOGVARS)]
    mom[:, :, 4:8] = lv
    mean = mom[:, :, 0:4]
    mean[lv == -40.0] = 0.0
    return mom, _randn((B, 4, hw), g)


def case_posterior(shape, ldm, scale, impl, U=U_POSTERIOR, report=None):
    """impl(mom fp32 [B, hw, ldm], noise fp32 [B, 4, hw], scale) -> z fp32 [B, 4, hw]"""
    B, hw = shape
    mom, noise = posterior_inputs(B, hw, ldm)
    ref, mag = R.posterior64(mom, noise, scale)
    return S.check_fp32_sum(f"edge posterior_sample B{B} hw{hw} ldm{ldm} scale{scale:g} U{U:g}", impl(mom, noise, scale), ref, mag, units=U,
                            report=report)


def timestep_inputs(n, dim):
    g = _gen(11, n, dim)
    t = torch.rand((n,), generator=g) * 1010.0 - 10.0
    k = min(n, len(TIMESTEPS))
    t[:k] = torch.tensor([TIMESTEPS[(i + dim) % len(TIMESTEPS)] for i in range(k)])
    return t


def case_timestep(n, dim, impl, U=U_TIMESTEP, report=None):
    """impl(t fp32 [n], dim) -> bf16 [n, dim]"""
    t = timestep_inputs(n, dim)
    return hold_interval(f"edge timestep_embedding n{n} dim{dim} U{U:g}", impl(t, dim).float(), t, dim, U, report)


def gauss9():
    g1 = torch.exp(-(torch.arange(3).float() - 1) ** 2 / 2)
    gk = g1[:, None] * g1[None, :]
    return (gk / gk.sum()).reshape(9).contiguous()


def peak_pixel(b, l, size):
    """the last pixel of row (3 b + 5 l + 1) % size"""
    return ((3 * b + 5 * l + 1) % size) * size + size - 1


def local_loss_inputs(case):
    """probs [n_samples * heads, size^2, L] positive; the map of every (sample, token) has its own peak at a row's LAST pixel and 0.75 of
    it at the next row's first one (the next index in memory, no neighbour on the map), so a wrong row pitch moves the maximum and a blur
    that reads across a row end raises it.  A different mask per image: random binary with the last sampled column set | all zero | one
    corner pixel (top-left in image 0, bottom-right in the last image); seg in {0, 0.5, 1}; a pre-filled loss"""
    size, Hm, Wm, heads, L, seg_l, n_samples, mask_batch, kind = case
    g = _gen(12, *case[:8], len(kind))
    n = size * size
    probs = torch.rand((n_samples, heads, n, L), generator=g) / L
    for b in range(n_samples):
        for l in range(L):
            peak = 0.5 + 0.03125 * ((b + l) % 7)
            probs[b, :, peak_pixel(b, l, size), l] += peak
            probs[b, :, (peak_pixel(b, l, size) + 1) % n, l] += 0.75 * peak
    if kind == "random":
        mask = (torch.rand((mask_batch, Hm, Wm), generator=g) > 0.5).float()
        mask[:, :, R.nearest_index(size, Wm)[-1]] = 1.0
    else:
        mask = torch.zeros((mask_batch, Hm, Wm))
        if kind == "corner":
            mask[0, 0, 0] = 1.0
            mask[-1, -1, -1] = 1.0
    seg = torch.randint(0, 3, (mask_batch, seg_l), generator=g).float() / 2
    return probs.reshape(n_samples * heads, n, L).contiguous(), mask, seg, gauss9(), 0.25 + 0.5 * torch.arange(n_samples).float()


def case_local_loss(case, impl, report=None, what=""):
    """impl(probs, mask [mask_batch, Hm, Wm], seg, gk, loss0, mask_batch, heads, size) -> loss fp32 [n_samples] afterwards.
    Bound: FP32_SUM_UNITS 2^-24 x the largest per-pixel sum of absolute summands (max and min are 1-Lipschitz) + 2^-24 |result|, the
    rounding of the accumulation into the pre-filled loss"""
    size, Hm, Wm, heads, L, seg_l, n_samples, mask_batch, kind = case
    probs, mask, seg, gk, loss0 = local_loss_inputs(case)
    ref, mag = R.local_loss64(probs, mask, seg, gk, loss0, mask_batch, heads, size)
    got = impl(probs, mask, seg, gk, loss0.clone(), mask_batch, heads, size)
    name = f"edge local_loss{what} size{size} mask{Hm}x{Wm} h{heads} L{L} seg{seg_l} {n_samples}/{mask_batch} {kind}"
    return S.check_fp32_sum(name, got, ref, mag + ref.abs() / S.FP32_SUM_UNITS, report=report)
