"""tests/boundary_ref.py and tests/boundary_cases.py without a GPU: a float32 CPU restatement of every plugin-boundary kernel and packer
(torch's own casts and compositions, not boundary_ref's bit arithmetic and index loops) passes every case of
tests/test_boundary_edges_gpu.py through the SAME ``case_*`` functions, udifftext_amd/packing.py is held to the same layout definition,
the units of the two measured bounds are re-measured, and twelve mutants each fail their check.  One line per check goes to
boundary_ref_cpu_report.txt in the temporary directory.
"""
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

import boundary_cases as K
import boundary_ref as R
import sliced_check as S

REPORT = os.path.join(tempfile.gettempdir(), "boundary_ref_cpu_report.txt")


# ------------------------------------------------------------------------------------------------ float32 restatements (mutant=...)
def _bf16(t, mutant=None):
    if mutant == "truncate":
        return R.f32_from_bits(R.f32_bits(t.float()) & 0xffff0000).bfloat16()
    return t.float().bfloat16()


def nchw_to_nhwc32(x, cpad, scale, mutant=None):
    B, C, HW = x.shape
    y = torch.zeros((B, HW, cpad), dtype=torch.bfloat16)
    y[:, :, :C] = _bf16((x * torch.tensor(scale, dtype=torch.float32)).permute(0, 2, 1), mutant)
    return y


def nhwc_to_nchw32(src, C):
    return src[:, :, :C].float().permute(0, 2, 1).contiguous()


def set_channels32(src, dst, c0, mutant=None):
    dst[:, :, c0:c0 + src.shape[1]] = _bf16(src.permute(0, 2, 1), mutant)
    return dst


def embed32(idx, table, pe, mutant=None):
    tok = torch.arange(idx.shape[0])
    pos = tok // pe.shape[0] if mutant == "pe_div" else tok % pe.shape[0]
    return _bf16(table[idx.long()] + pe[pos], mutant)


def add32(a, b, mutant=None):
    return _bf16(a.float() + b.float(), mutant)


def bias_add32(x, bias, inplace, mutant=None):
    return _bf16(x.float() + bias[None, :], mutant)


def mask_downsample32(m, mutant=None):
    o = 4 if mutant == "taps_4_5" else 3
    return 0.25 * (m[:, o::8, o::8] + m[:, o::8, o + 1::8] + m[:, o + 1::8, o::8] + m[:, o + 1::8, o + 1::8])


def posterior32(mom, noise, scale, mutant=None):
    mean, lv = mom[:, :, 0:4].permute(0, 2, 1), mom[:, :, 4:8].permute(0, 2, 1)
    lv = lv if mutant == "no_clamp" else lv.clamp(-30.0, 20.0)
    return torch.tensor(scale, dtype=torch.float32) * (mean + torch.exp(0.5 * lv) * noise)


def timestep32(t, dim, mutant=None, bf16=True):
    half = dim // 2
    k = torch.arange(half, dtype=torch.float32)
    denom = float(half - 1) if mutant == "half_minus_1" else float(half)
    arg = t[:, None] * torch.exp(torch.tensor(-9.210340371976184, dtype=torch.float32) * k / denom)[None, :]
    parts = [torch.sin(arg), torch.cos(arg)] if mutant == "sin_cos" else [torch.cos(arg), torch.sin(arg)]
    out = torch.cat(parts, dim=1)
    return out.bfloat16() if bf16 else out


def local_loss32(probs, mask, seg, gk, loss, mask_batch, heads, size, mutant=None):
    n_samples, L = probs.shape[0] // heads, probs.shape[2]
    seg_l, Hm, Wm = seg.shape[1], mask.shape[1], mask.shape[2]
    amap = probs.reshape(n_samples, heads, size, size, L)[..., :seg_l].sum(1) / float(heads + 1 if mutant == "heads_plus_1" else heads)
    amap = amap.permute(0, 3, 1, 2).contiguous()                                # [n_samples, seg_l, size, size]
    if mutant == "no_border":                                                   # the flat map, zero only before its start and after its end
        flat = F.pad(amap.reshape(n_samples, seg_l, -1), (size + 1, size + 1))
        n = size * size
        blur = sum(gk[3 * (dy + 1) + dx + 1] * flat[..., size + 1 + dy * size + dx:size + 1 + dy * size + dx + n]
                   for dy in (-1, 0, 1) for dx in (-1, 0, 1)).reshape(amap.shape)
    else:
        blur = F.conv2d(amap.reshape(-1, 1, size, size), gk.reshape(1, 1, 3, 3), padding=1).reshape(amap.shape)
    if mutant == "round_index":
        my = [min(Hm - 1, int(d * Hm / size + 0.5)) for d in range(size)]
        mx = [min(Wm - 1, int(d * Wm / size + 0.5)) for d in range(size)]
        mm = mask[:, my][:, :, mx]
    else:
        mm = F.interpolate(mask[:, None], (size, size))[:, 0]                   # nearest
    bm = torch.arange(n_samples) % mask_batch
    pl = (mm[bm][:, None] * blur).reshape(n_samples, seg_l, -1).max(-1)[0] + (1.0 - seg[bm])
    return loss + -pl.min(-1)[0]


def _blocks(inner, h):
    rows = []
    for s in range(0, inner, h):
        rows += list(range(s, min(inner, s + h))) + list(range(inner + s, inner + min(inner, s + h)))
    return torch.tensor(rows)


def pack_linear32(w, bias, fp8, geglu, mutant=None):
    N, K = w.shape
    Npad, Kpad = -(-N // 4) * 4, -(-K // 128) * 128 if fp8 else -(-K // 64) * 64
    b = torch.zeros(N) if bias is None else bias
    if geglu:
        perm = _blocks(N // 2, 64 if mutant == "geglu_64" else 32)
        w, b = w[perm], b[perm]
    out = {"dims": (N, Npad, K, Kpad), "bias": F.pad(b, (0, Npad - N)), "colscale": None}
    if fp8:
        amax = w.abs().amax(dim=1)
        scale = amax / 448.0 if mutant == "no_floor" else amax.clamp_min(1e-12) * torch.tensor(1.0 / 448.0, dtype=torch.float32)
        q = R.e4m3_bytes_by_table((w / scale[:, None]).clamp(-448.0, 448.0))
        out["weight"] = F.pad(q, (0, Kpad - K, 0, Npad - N))
        out["colscale"] = F.pad(scale, (0, Npad - N), value=1.0)
    else:
        out["weight"] = R.bf16_bits(F.pad(w.bfloat16(), (0, Kpad - K, 0, Npad - N)))
    return out


def pack_conv32(w, bias, segments, n_pad_to, mutant=None):
    N, Cin, kh, kw = w.shape
    Npad = -(-N // n_pad_to) * n_pad_to
    wt = w.permute(0, 2, 3, 1).bfloat16()                                       # [N, kh, kw, Cin]
    if mutant == "pad_concatenated":
        parts = [F.pad(wt, (0, -(-Cin // 64) * 64 - Cin))]
    else:
        parts = [F.pad(p, (0, -(-p.shape[3] // 64) * 64 - p.shape[3])) for p in torch.split(wt, list(segments or [Cin]), dim=3)]
    weight = F.pad(torch.cat(parts, dim=3).reshape(N, -1), (0, 0, 0, Npad - N))
    b = torch.zeros(N) if bias is None else bias
    return {"dims": (N, Npad, weight.shape[1], weight.shape[1]), "weight": R.bf16_bits(weight), "bias": F.pad(b, (0, Npad - N)), "colscale": None}


def _wrap(fn, mutant):
    return lambda *a: fn(*a, mutant=mutant)


# ------------------------------------------------------------------------------------------------ the helpers, pinned
def test_bf16_rne_bits_is_torch_rounding_and_covers_the_special_values():
    x = torch.cat([R.specials(), torch.randn(4096, generator=torch.Generator().manual_seed(1)) * 3])
    want = R.bf16_bits(x.bfloat16())
    assert bool(R.same_bf16(R.bf16_rne_bits(x), want).all()) and bool(R.same_bf16(want, R.bf16_rne_bits(x)).all())
    got = R.bf16_rne_bits(R.specials()).tolist()
    assert got == [0x0000, 0x8000, 0x7f80, 0xff80, 0x7fc0, 0x3f80, 0x3f82, 0xbf80, 0xbf82, 0x3f80, 0x3f81, 0x3f81, 0x3f82, 0xbf80, 0xbf81,
                   0xbf81, 0xbf82, 0x7f80, 0xff80]
    trunc = R.bf16_bits(_bf16(R.specials(), "truncate")).tolist()
    assert trunc[6] == 0x3f81 and trunc[10] == 0x3f80 and trunc[17] == 0x7f7f                   # where truncation differs
    y = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    y[:3] = torch.tensor([0.0, 1.00390625, 1.01171875])                                         # 0, and the two ties
    assert R.bf16_rne_f64(y[:3]).tolist() == [0.0, 1.0, 1.015625]
    f = y.float()
    assert torch.equal(R.bf16_rne_f64(f.double()), f.bfloat16().double())                       # (from an fp32 value there is one rounding)
    assert all((b & 0x7fffffff) == 0 or (b & 0x7f800000) != 0 for b in R.SPECIAL_BITS)           # no subnormal among them


def test_e4m3_table_is_the_ocp_format_and_torchs_cast():
    tab = R.e4m3_table()
    assert tab.numel() == 127 and float(tab[0]) == 0 and float(tab[1]) == 2.0 ** -9 and float(tab[8]) == 2.0 ** -6 and float(tab[126]) == 448.0
    assert bool((tab[1:] > tab[:-1]).all())
    x = torch.cat([tab.float(), -tab.float(), (tab[1:] + tab[:-1]).float() / 2, torch.randn(8192, generator=torch.Generator().manual_seed(3)) * 100])
    x = x.clamp(-448.0, 448.0)
    by_table = R.e4m3_bytes_by_table(x)
    assert by_table[:127].tolist() == list(range(127)) and by_table[127 + 1:254].tolist() == [c | 0x80 for c in range(1, 127)]
    assert by_table[254:254 + 126].tolist() == [c + (c & 1) for c in range(126)]                # a tie goes to the even code
    if hasattr(torch, "float8_e4m3fn"):
        assert torch.equal(by_table, x.to(torch.float8_e4m3fn).view(torch.uint8).long())
    assert torch.equal(R.e4m3_bytes(x), by_table)


def test_inputs_hold_what_the_cases_are_about():
    assert {0.0, 0.5, 19.0, 999.0} <= {round(float(v), 4) for n in K.TIMESTEP_N for d in K.TIMESTEP_DIM for v in K.timestep_inputs(n, d)}
    assert any(float(v) < 0 and float(v) != int(v) for v in K.timestep_inputs(4, 2))
    lv = torch.cat([K.posterior_inputs(B, hw, 12)[0][:, :, 4:8].reshape(-1) for B, hw in K.POSTERIOR])
    assert set(K.LOGVARS) <= set(lv.tolist())
    mom, _ = K.posterior_inputs(2, 257, 12)
    assert not bool(torch.isfinite(mom[:, 1::2, 8:]).any()) and bool((mom[:, 0::2, 8:] == 1e30).all()) and bool(torch.isfinite(mom[:, :, :8]).all())
    for shape in K.EMBED:
        idx, table, pe = K.embed_inputs(*shape)
        assert int(idx.max()) == K.EMBED_V - 1 and (int(idx.min()) == 0 or shape[0] == 1)
        plain = table[:, R.specials().numel():]
        assert all(bool((plain[i] != plain[j]).all()) for i in range(0, K.EMBED_V, 7) for j in range(i + 1, K.EMBED_V, 5))
    idx, table, pe = K.embed_inputs(24, 12, 256)
    sums = torch.stack([table[int(idx[s % 24]), s] + pe[(s % 24) % 12, s] for s in range(R.specials().numel())])
    assert torch.equal(R.f32_bits(sums)[:4], R.f32_bits(R.specials())[:4]) and torch.equal(R.f32_bits(sums)[5:], R.f32_bits(R.specials())[5:])
    hi, lo = K.special_parts()
    assert torch.equal(R.f32_bits(hi + lo)[5:], R.f32_bits(R.specials())[5:]) and torch.equal(hi.bfloat16().float()[:4], hi[:4])
    for case in K.LOCAL_LOSS:
        probs, mask, seg, gk, loss0 = K.local_loss_inputs(case)
        size, heads, L, n_samples, mask_batch = case[0], case[3], case[4], case[6], case[7]
        peaks = probs.reshape(n_samples, heads, size * size, L).mean(1).argmax(1)                # [n_samples, L]
        assert size == 1 or peaks.tolist() == [[K.peak_pixel(b, l, size) for l in range(L)] for b in range(n_samples)]
        assert all(p % size == size - 1 for p in peaks.reshape(-1).tolist())
        assert mask_batch == 1 or case[8] == "zero" or not torch.equal(mask[0], mask[1])
    assert float(K.local_loss_inputs(K.LOCAL_LOSS[6])[1].abs().sum()) == 0 and float(K.local_loss_inputs(K.LOCAL_LOSS[7])[1].sum()) == 2


def test_references_are_the_torch_compositions_in_float64():
    mask = (torch.rand((2, 1, 16, 40), generator=torch.Generator().manual_seed(4)) > 0.5).float()
    assert torch.equal(R.mask_downsample64(mask[:, 0])[0], F.interpolate(mask.double(), scale_factor=0.125, mode="bilinear")[:, 0])
    case = K.LOCAL_LOSS[3]
    probs, mask, seg, gk, loss0 = K.local_loss_inputs(case)
    ref, mag = R.local_loss64(probs, mask, seg, gk, loss0, case[7], case[3], case[0])
    want = local_loss32(probs.double(), mask.double(), seg.double(), gk.double(), loss0.double(), case[7], case[3], case[0])
    assert float((ref - want).abs().max()) < 1e-14 and bool((mag >= 1.0).all())
    assert R.nearest_index(17, 50)[:4] == [0, 2, 5, 8] and R.nearest_index(17, 8)[-1] == 7 and R.nearest_index(9, 16)[-1] == 14
    assert [R.geglu_source_row(n, 192) for n in (0, 31, 32, 63, 64, 96, 191)] == [0, 31, 96, 127, 32, 128, 191]


# ------------------------------------------------------------------------------------------------ the two measured bounds
def test_measured_units_are_the_recorded_ones():
    """the worst |float32 torch evaluation - float64| over 2^-24 x magnitude on the cases' inputs: 2.919 and 4.400 where the figures of
    boundary_cases.py were recorded (there rounded up).  Another host's libm may move them a little, which is what the factor 4 is for: here
    the host's figure has to stay within a quarter of the recorded one and under half of U"""
    worst_p = worst_t = 0.0
    for shape in K.POSTERIOR:
        for ldm in K.POSTERIOR_LDM:
            for scale in K.POSTERIOR_SCALES:
                mom, noise = K.posterior_inputs(*shape, ldm)
                ref, mag = R.posterior64(mom, noise, scale)
                worst_p = max(worst_p, float(((posterior32(mom, noise, scale).double() - ref).abs() / (2.0 ** -24 * mag)).max()))
    for n in K.TIMESTEP_N:
        for dim in K.TIMESTEP_DIM:
            t = K.timestep_inputs(n, dim)
            ref, mag = R.timestep64(t, dim)
            worst_t = max(worst_t, float(((timestep32(t, dim, bf16=False).double() - ref).abs() / (2.0 ** -24 * mag)).max()))
    S._report(f"measured units: posterior_sample {worst_p:.3f} (recorded {K.POSTERIOR_MEASURED}), timestep_embedding {worst_t:.3f} "
              f"(recorded {K.TIMESTEP_MEASURED})", REPORT)
    print(f"measured units: posterior {worst_p:.4f}, timestep {worst_t:.4f}")
    assert K.U_POSTERIOR == max(4.0, 4.0 * K.POSTERIOR_MEASURED) and K.U_TIMESTEP == max(4.0, 4.0 * K.TIMESTEP_MEASURED)
    assert worst_p <= K.U_POSTERIOR / 2 and worst_t <= K.U_TIMESTEP / 2
    assert abs(worst_p / K.POSTERIOR_MEASURED - 1) < 0.25 and abs(worst_t / K.TIMESTEP_MEASURED - 1) < 0.25


# ------------------------------------------------------------------------------------------------ every case, float32 restatement
@pytest.mark.parametrize("shape", K.NCHW_TO_NHWC)
def test_restated_nchw_to_nhwc_passes_every_case(shape):
    for scale in K.SCALES:
        K.case_nchw_to_nhwc(shape, scale, nchw_to_nhwc32, report=REPORT)


@pytest.mark.parametrize("shape", K.NHWC_TO_NCHW)
def test_restated_nhwc_to_nchw_passes_every_case(shape):
    for f32 in (True, False):
        K.case_nhwc_to_nchw(shape, f32, nhwc_to_nchw32, report=REPORT)


@pytest.mark.parametrize("spec", K.SET_CHANNELS)
def test_restated_set_channels_passes_every_case(spec):
    for hw in K.SET_HW:
        K.case_set_channels(spec, hw, set_channels32, report=REPORT)


def test_restated_embed_add_bias_add_and_mask_downsample_pass_every_case():
    for shape in K.EMBED:
        K.case_embed(shape, embed32, report=REPORT)
    for n in K.ADD_N:
        K.case_add(n, add32, report=REPORT)
    for shape in K.BIAS_ADD:
        for inplace in (False, True):
            K.case_bias_add(shape, inplace, bias_add32, report=REPORT)
    for shape in K.MASK:
        assert K.case_mask_downsample(shape, mask_downsample32, report=REPORT) <= S.FP32_SUM_UNITS


def test_restated_posterior_and_timestep_pass_every_case():
    for shape in K.POSTERIOR:
        for ldm in K.POSTERIOR_LDM:
            for scale in K.POSTERIOR_SCALES:
                assert K.case_posterior(shape, ldm, scale, posterior32, report=REPORT) <= K.U_POSTERIOR / 2
    for n in K.TIMESTEP_N:
        for dim in K.TIMESTEP_DIM:
            K.case_timestep(n, dim, timestep32, report=REPORT)


@pytest.mark.parametrize("case", K.LOCAL_LOSS)
def test_restated_local_loss_passes_every_case(case):
    assert K.case_local_loss(case, local_loss32, report=REPORT) <= S.FP32_SUM_UNITS


def test_restated_pack_linear_passes_every_case():
    for case in K.linear_cases():
        K.case_pack_linear(*case, pack_linear32, report=REPORT)


@pytest.mark.parametrize("segments", K.CONV_SEGMENTS)
def test_restated_pack_conv_passes_every_case(segments):
    for case in K.conv_cases(segments):
        K.case_pack_conv(*case, pack_conv32, report=REPORT)


# ------------------------------------------------------------------------------------------------ udifftext_amd/packing.py, same definition
def _packing_linear(w, bias, fp8, geglu):
    from udifftext_amd import packing
    N, K_ = w.shape
    b = torch.zeros(N) if bias is None else bias
    if geglu:
        perm = packing.geglu_permutation(N // 2)
        w, b = w[perm], b[perm]
    if fp8:
        q, cs = packing.pack_linear_fp8(w)
        return {"dims": (N, q.shape[0], K_, q.shape[1]), "weight": q.long(), "bias": packing.pad_bias(b), "colscale": cs}
    p = packing.pack_linear(w)
    return {"dims": (N, p.shape[0], K_, p.shape[1]), "weight": R.bf16_bits(p), "bias": packing.pad_bias(b), "colscale": None}


def _packing_conv(w, bias, segments, n_pad_to):
    from udifftext_amd import packing
    p = packing.pack_conv(w, list(segments) if segments else None, n_pad_to)
    b = torch.zeros(w.shape[0]) if bias is None else bias
    return {"dims": (w.shape[0], p.shape[0], p.shape[1], p.shape[1]), "weight": R.bf16_bits(p), "bias": packing.pad_bias(b, n_pad_to),
            "colscale": None}


def test_packing_py_follows_the_layout_definition():
    for case in K.linear_cases():
        K.case_pack_linear(*case, _packing_linear, report=REPORT)
    for segments in K.CONV_SEGMENTS:
        for case in K.conv_cases(segments):
            if case[2] != (1, 7) or case[0] != 130:                             # (one tap shape at the largest N is enough here)
                K.case_pack_conv(*case, _packing_conv, report=REPORT)


# ------------------------------------------------------------------------------------------------ the mutants
def _fails(fn, match):
    with pytest.raises(AssertionError, match=match):
        fn()


def test_mutant_truncating_bf16_conversion():
    _fails(lambda: K.case_nchw_to_nhwc((3, 4, 257, 8), 1.0, _wrap(nchw_to_nhwc32, "truncate"), report=REPORT), "values differ")
    _fails(lambda: K.case_set_channels((5, 3, 16), 257, _wrap(set_channels32, "truncate"), report=REPORT), "values differ")
    _fails(lambda: K.case_embed((24, 12, 256), _wrap(embed32, "truncate"), report=REPORT), "values differ")
    _fails(lambda: K.case_add(8, _wrap(add32, "truncate"), report=REPORT), "values differ")
    _fails(lambda: K.case_bias_add((1, 8), True, _wrap(bias_add32, "truncate"), report=REPORT), "values differ")


def test_mutant_pe_row_by_division():
    for shape in K.EMBED[1:]:
        _fails(lambda: K.case_embed(shape, _wrap(embed32, "pe_div"), report=REPORT), "values differ")
    K.case_embed(K.EMBED[0], _wrap(embed32, "pe_div"), report=REPORT)             # one token: the two agree


def test_mutant_sin_cos_order_and_off_by_one_k():
    for n in K.TIMESTEP_N:
        for dim in K.TIMESTEP_DIM:
            _fails(lambda: K.case_timestep(n, dim, _wrap(timestep32, "sin_cos"), report=REPORT), "outside the interval|non-finite")
            _fails(lambda: K.case_timestep(n, dim, _wrap(timestep32, "half_minus_1"), report=REPORT), "outside the interval|non-finite")


def test_mutant_missing_logvar_clamp():
    for shape in K.POSTERIOR:
        _fails(lambda: K.case_posterior(shape, 12, 0.18215, _wrap(posterior32, "no_clamp"), report=REPORT), "elements beyond")
    # the lower clamp alone: the elements whose logvar is -40 (their mean is 0)
    mom, noise = K.posterior_inputs(2, 257, 8)
    ref, mag = R.posterior64(mom, noise, 1.0)
    low = (mom[:, :, 4:8] == -40.0).permute(0, 2, 1)
    err = (posterior32(mom, noise, 1.0, mutant="no_clamp").double() - ref).abs()
    assert int(low.sum()) > 50 and bool((err[low] > K.U_POSTERIOR * 2.0 ** -24 * mag[low]).all())


def test_mutant_mask_taps_one_pixel_off():
    for shape in K.MASK:
        _fails(lambda: K.case_mask_downsample(shape, _wrap(mask_downsample32, "taps_4_5"), report=REPORT), "values differ")


def test_mutants_of_the_local_loss():
    fails = lambda case, m: _fails(lambda: K.case_local_loss(case, _wrap(local_loss32, m), report=REPORT), "elements beyond")
    fails(K.LOCAL_LOSS[3], "round_index")                                          # 50x20 onto 17x17: Hm is no multiple of size
    for case in K.LOCAL_LOSS[:6]:
        fails(case, "heads_plus_1")
    for case in K.LOCAL_LOSS[:6]:
        fails(case, "no_border")                                                    # (a 1x1 map too: its taps wrap onto the one pixel)


def test_mutant_geglu_blocks_of_64():
    _fails(lambda: K.case_pack_linear(192, 65, False, True, True, _wrap(pack_linear32, "geglu_64"), report=REPORT), "values differ")
    _fails(lambda: K.case_pack_linear(192, 129, True, True, True, _wrap(pack_linear32, "geglu_64"), report=REPORT), "values differ")
    K.case_pack_linear(64, 65, False, True, True, _wrap(pack_linear32, "geglu_64"), report=REPORT)      # inner = 32: one block either way


def test_mutant_padding_over_the_concatenated_channels():
    for segments in ((65, 63), (3, 200, 1)):
        _fails(lambda: K.case_pack_conv(5, segments, (3, 3), 4, True, _wrap(pack_conv32, "pad_concatenated"), report=REPORT), "dims|values differ")
    K.case_pack_conv(5, (64,), (3, 3), 4, True, _wrap(pack_conv32, "pad_concatenated"), report=REPORT)


def test_mutant_scale_without_the_floor():
    for K_ in K.FP8_K:
        _fails(lambda: K.case_pack_linear(5, K_, True, False, True, _wrap(pack_linear32, "no_floor"), report=REPORT), "values differ")
