"""The float64 references of tests/shadow_ref.py against independent torch compositions, on the CPU at small shapes — above all the
conventions that are easy to get wrong: stride-2 bottom / right padding, the GEGLU block permutation, in_scsh applied before the
SiLU with the padding staying zero, the zero-context rows of the fused text attention, the q8_fixed column rule."""
import math

import pytest
import torch
import torch.nn.functional as F

import mx8_ref
import shadow_ref as S

D = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _pack_conv(w):
    """[N, C, k, k] -> [N, k*k*C] tap-major (the layout of packing.pack_conv, restated)"""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


@pytest.mark.parametrize("H,W,stride,pad,out_hw", [(8, 8, 1, (1, 1), None), (8, 8, 2, (1, 1), None), (8, 8, 2, (0, 0), (4, 4)),
                                                   (7, 9, 2, (0, 0), (4, 5))])
def test_conv_reference_padding_and_stride(H, W, stride, pad, out_hw):
    g = _g(1)
    x = torch.randn((2, H, W, 64), generator=g, dtype=D)
    w = torch.randn((8, 64, 3, 3), generator=g, dtype=D)
    b = torch.randn((8,), generator=g, dtype=D)
    got = S.ref_conv2d(x, _pack_conv(w), b, ksize=3, stride=stride, pad=pad, out_hw=out_hw)
    # the reference's Downsample: explicit (0, 1, 0, 1) zero padding (bottom / right) and an unpadded stride-2 convolution
    if out_hw is not None:
        Ho, Wo = out_hw
        xp = F.pad(_nchw(x), (0, (Wo - 1) * 2 + 3 - W, 0, (Ho - 1) * 2 + 3 - H))
        want = F.conv2d(xp, w, b, stride=2)
    else:
        want = F.conv2d(_nchw(x), w, b, stride=stride, padding=pad)
    torch.testing.assert_close(got, want.permute(0, 2, 3, 1), rtol=1e-12, atol=1e-12)


def test_conv_reference_upsample_concat_residual_rowvec():
    g = _g(2)
    x = torch.randn((2, 5, 6, 64), generator=g, dtype=D)
    x2 = torch.randn((2, 5, 6, 128), generator=g, dtype=D)
    w = torch.randn((16, 192, 3, 3), generator=g, dtype=D)
    b = torch.randn((16,), generator=g, dtype=D)
    res = torch.randn((2, 10, 12, 16), generator=g, dtype=D)
    rv = torch.randn((2, 16), generator=g, dtype=D)
    got = S.ref_conv2d(x, _pack_conv(w), b, x2=x2, upsample=True, residual=res, rowvec=rv)
    up = F.interpolate(torch.cat([_nchw(x), _nchw(x2)], 1), size=(10, 12), mode="nearest")
    want = F.conv2d(up, w, b, padding=1).permute(0, 2, 3, 1) + res + rv[:, None, None, :]
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_conv_reference_in_scsh_before_silu_and_padding_stays_zero():
    """GroupNorm + SiLU in front of the convolution: the table is applied to the pixels, the zero padding of the convolution is NOT
    transformed (a shift of 3 would make it silu(3) otherwise)"""
    from udifftext_amd import lib as L
    g = _g(3)
    B, H, W, C1, C2 = 2, 6, 6, 64, 64
    x = torch.randn((B, H, W, C1), generator=g, dtype=D) * 2 + 1
    x2 = torch.randn((B, H, W, C2), generator=g, dtype=D) - 0.5
    gamma = torch.rand((C1 + C2,), generator=g, dtype=D) + 0.5
    beta = torch.randn((C1 + C2,), generator=g, dtype=D) + 3.0
    w = torch.randn((8, C1 + C2, 3, 3), generator=g, dtype=D)
    table = S.ref_gn_table(x, gamma, beta, 32, 1e-5, x2=x2)
    got = S.ref_conv2d(x, _pack_conv(w), None, x2=x2, in_scsh=table, in_act=1, flags=L.GEMM_CONV)
    gn = F.silu(F.group_norm(torch.cat([_nchw(x), _nchw(x2)], 1), 32, gamma, beta, 1e-5))
    want = F.conv2d(gn, w, None, padding=1).permute(0, 2, 3, 1)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    # and the table itself: scale, shift per (sample, channel) in [B, C/64, 2, 64]
    t = table.reshape(B, -1, 2, 64)
    xin = torch.cat([x, x2], -1)
    torch.testing.assert_close((xin * t[:, :, 0].reshape(B, 1, 1, -1) + t[:, :, 1].reshape(B, 1, 1, -1)),
                               F.group_norm(_nchw(xin), 32, gamma, beta, 1e-5).permute(0, 2, 3, 1), rtol=1e-10, atol=1e-10)


def test_group_norm_and_layer_norm_references():
    g = _g(4)
    x = torch.randn((2, 7, 5, 64), generator=g, dtype=D) * 3 + 2
    x2 = torch.randn((2, 7, 5, 128), generator=g, dtype=D)
    gamma, beta = torch.randn((192,), generator=g, dtype=D), torch.randn((192,), generator=g, dtype=D)
    got = S.ref_group_norm(x, gamma, beta, 32, 1e-6, True, x2=x2)
    want = F.silu(F.group_norm(torch.cat([_nchw(x), _nchw(x2)], 1), 32, gamma, beta, 1e-6)).permute(0, 2, 3, 1)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    y = torch.randn((3, 10, 96), generator=g, dtype=D) + 5
    torch.testing.assert_close(S.ref_layer_norm(y, gamma[:96], beta[:96], 1e-5),
                               F.layer_norm(y, (96,), gamma[:96], beta[:96], 1e-5), rtol=1e-12, atol=1e-12)


def test_linear_reference_geglu_block_permutation_and_epilogue():
    from udifftext_amd import lib as L, packing
    g = _g(5)
    M, K, inner = 12, 64, 96
    x = torch.randn((M, K), generator=g, dtype=D)
    w = torch.randn((2 * inner, K), generator=g, dtype=D)
    b = torch.randn((2 * inner,), generator=g, dtype=D)
    perm = packing.geglu_permutation(inner)
    got = S.ref_linear(x, w[perm], 2 * inner, bias=b[perm], flags=L.GEMM_GEGLU)
    h = x @ w.t() + b
    want = h[:, :inner] * F.gelu(h[:, inner:])                    # GEGLU on the unpacked weights (attention.py: x * gelu(gate))
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    # residual, row vector per sample, SiLU after everything, alpha
    r = torch.randn((M, 2 * inner), generator=g, dtype=D)
    rv = torch.randn((3, 2 * inner), generator=g, dtype=D)
    got = S.ref_linear(x, w, 2 * inner, bias=b, residual=r, rowvec=rv, rows_per_batch=4, flags=L.GEMM_SILU_OUT, alpha=0.5)
    want = F.silu(0.5 * (x @ w.t()) + b + rv.repeat_interleave(4, 0) + r)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)


def test_ln_linear_reference_is_layernorm_then_linear():
    from udifftext_amd import packing
    g = _g(6)
    M, K, N = 9, 128, 64
    x = torch.randn((M, K), generator=g) * 2 + 0.7
    w = torch.randn((N, K), generator=g) / math.sqrt(K)
    b = torch.randn((N,), generator=g)
    gamma, beta = torch.rand((K,), generator=g) + 0.5, torch.randn((K,), generator=g)
    wf, c, s = packing.pack_ln_linear(w, b, gamma, beta)
    got = S.ref_ln_linear(x, wf, c, N, 1e-5)
    # (the folded weight is gamma o W rounded to bf16: compare with LayerNorm -> linear on exactly that weight)
    wg = wf[:, :K].double() / gamma.double()[None, :]
    want = F.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5) @ wg.t() - wg @ beta.double() + c.double()
    torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-9)


def test_linear_mx8_reference_on_the_quantised_operands_and_its_layernorm_fold():
    from udifftext_amd import packing
    g = _g(7)
    M, K, N = 16, 256, 64
    x = torch.randn((M, K), generator=g) * 3 + 1
    xq, xs = mx8_ref.encode(x)
    xd = mx8_ref.decode(xq, xs).double()
    w = torch.randn((N, K), generator=g) / 16
    gamma, beta = torch.rand((K,), generator=g) + 0.5, torch.randn((K,), generator=g)
    wq, cs, c, s = packing.pack_ln_linear_mx8(w, None, gamma, beta)
    wd = wq.view(torch.float8_e4m3fn).double() * cs.double()[:, None]
    plain = S.ref_linear_mx8(xd, wq, cs, N)
    torch.testing.assert_close(plain, xd @ wd.t(), rtol=1e-12, atol=1e-12)
    mean = x.double().mean(1)
    rstd = 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-5)
    got = S.ref_linear_mx8(xd, wq, cs, N, ln=(c, s, mean, rstd))
    want = ((xd - mean[:, None]) * rstd[:, None]) @ wd.t() + c.double()[None, :N]
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-6)          # (the packer sums s in fp32)


def test_attention_references_against_sdpa():
    g = _g(8)
    B, Nq, Nk, heads = 2, 10, 7, 3
    q = torch.randn((B, Nq, heads * 64), generator=g, dtype=D)
    k = torch.randn((B, Nk, heads * 64 + 64), generator=g, dtype=D)          # (row views wider than heads * 64)
    v = torch.randn((B, Nk, heads * 64 + 64), generator=g, dtype=D)
    got = S.ref_attention(q, k, v, heads, 64, 0.125)
    split = lambda t: t[..., :heads * 64].reshape(B, -1, heads, 64).transpose(1, 2)   # noqa: E731
    want = F.scaled_dot_product_attention(split(q), split(k), split(v), scale=0.125).transpose(1, 2).reshape(B, Nq, heads * 64)
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    p = S.ref_probs(q, k, heads, 64, 0.125)
    torch.testing.assert_close(p, torch.softmax(split(q) @ split(k).transpose(-1, -2) * 0.125, -1).reshape(B * heads, Nq, Nk))


def test_tattn_reference_and_its_zero_context_rows():
    """x + to_out(attention(LN(x) Wq, K, V)) + bias; the first zero_samples samples: a zero context (k = v = 0) gives a uniform
    softmax over zero values -> x + bias exactly"""
    g = _g(9)
    B, N, heads, Lc = 3, 8, 2, 5
    C = heads * 64
    x = torch.randn((B, N, C), generator=g, dtype=D)
    kv = torch.randn((B, Lc, 2 * C), generator=g, dtype=D)
    wq, wo = torch.randn((C, C), generator=g, dtype=D) / 8, torch.randn((C, C), generator=g, dtype=D) / 8
    gamma, beta, bias = torch.rand((C,), generator=g, dtype=D), torch.randn((C,), generator=g, dtype=D), torch.randn((C,), generator=g, dtype=D)
    got = S.ref_tattn(x, kv, wq, wo, gamma, beta, bias, heads, 0.125, 1, 1e-5)
    kv0 = kv.clone()
    kv0[0] = 0
    split = lambda t: t.reshape(B, -1, heads, 64).transpose(1, 2)   # noqa: E731
    q = F.layer_norm(x, (C,), gamma, beta, 1e-5) @ wq.t()
    o = F.scaled_dot_product_attention(split(q), split(kv0[..., :C]), split(kv0[..., C:]), scale=0.125).transpose(1, 2).reshape(B, N, C)
    want = x + o @ wo.t() + bias
    torch.testing.assert_close(got, want, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(got[0], x[0] + bias, rtol=0, atol=0)


def test_q8_fixed_column_rule_and_block_decode():
    """columns before q8_fixed_col: E8M0 block scales (mx8_ref); from there on e4m3(v * mul), read back as byte / mul"""
    g = _g(10)
    M, C = 8, 128
    v = torch.randn((M, 3 * C), generator=g)
    qk8, qks = mx8_ref.encode(v[:, :2 * C])
    mul = 32.0
    v8 = (v[:, 2 * C:] * mul).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    data = torch.cat([qk8, v8], 1).contiguous()
    scale = torch.zeros((3, M), dtype=torch.int32)
    scale[:2] = qks
    from udifftext_amd.ops import Mx8Act
    dec = S.decode_q8(Mx8Act(data, scale), 3 * C, fixed=(2 * C, mul))
    torch.testing.assert_close(dec[:, :2 * C], mx8_ref.decode(qk8, qks))
    torch.testing.assert_close(dec[:, 2 * C:], v8.view(torch.float8_e4m3fn).float() / mul)
    assert float((dec[:, 2 * C:] - v[:, 2 * C:]).abs().max()) <= float(v[:, 2 * C:].abs().max()) * 2 ** -4


def test_timestep_embedding_reference():
    t = torch.tensor([0.0, 1.0, 441.0, 999.0])
    got = S.ref_timestep_embedding(t, 320)
    half = 160
    f = torch.exp(-math.log(10000) * torch.arange(half, dtype=D) / half)
    a = t.double()[:, None] * f
    torch.testing.assert_close(got, torch.cat([torch.cos(a), torch.sin(a)], -1))


def test_block_localisation_catches_one_wrong_tile():
    """a 1 % error on one 32 x 32 tile of a 256 x 256 output: 1.6e-4 of the global RMS, but 1e-2 of its block"""
    g = _g(11)
    ref = torch.randn((256, 256), generator=g, dtype=D)
    err = torch.zeros_like(ref)
    err[224:, 96:128] = 0.01 * ref[224:, 96:128]
    assert S.block_ratio(err, ref) == pytest.approx(0.01, rel=1e-6)
    assert (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item() < 2e-3
    # ragged edges count, and a small-magnitude block is held to 0.1 of the global RMS
    ref2 = ref[:250, :200].clone()
    ref2[:32, :32] *= 1e-6
    e2 = torch.zeros_like(ref2)
    e2[:32, :32] = 1e-3
    assert S.block_ratio(e2, ref2) == pytest.approx(1e-2, rel=2e-2)


# ------------------------------------------------------------ masked_attention, posterior_sample, mask_downsample, embed_tokens
def _shadow_verdict(cls, got, ref, rel_rms=None):
    """what Shadow.compare says about one output (None: within its bounds)"""
    sh = S.Shadow("cpu")
    sh._cur = [0.0, 0.0, None]
    sh.compare("op", cls, got, ref, "", rel_rms=rel_rms)
    return sh._cur[2]


def _mattn_inputs(seed, B=3, Nq=9, Lk=11, heads=4, D=32, dtype=D):
    g = _g(seed)
    C = heads * D
    q = torch.randn((B, Nq, C), generator=g, dtype=dtype)
    kv = torch.randn((B, Lk, 2 * C + 16), generator=g, dtype=dtype)         # (row views wider than heads * D)
    mask = torch.zeros((Nq, Lk), dtype=torch.float32)
    mask[torch.rand((Nq, Lk), generator=g) < 0.3] = float("-inf")
    mask[:, 0] = 0.0                                                         # every query keeps one key
    kpm = torch.rand((B, Lk), generator=g) < 0.3
    kpm[:, 0] = False
    kpm[1, 1:4] = True
    return q, kv[..., :C], kv[..., C:2 * C + 16], mask, kpm, heads, D


def _sdpa_masked(q, k, v, heads, D, scale, mask, kpm):
    B, Nq = q.shape[:2]
    split = lambda t: t[..., :heads * D].reshape(B, -1, heads, D).transpose(1, 2)   # noqa: E731
    merged = None
    if mask is not None or kpm is not None:
        merged = torch.zeros((B, 1, Nq, k.shape[1]), dtype=q.dtype)
        if mask is not None:
            merged = merged + mask.to(q.dtype)
        if kpm is not None:
            merged = merged.masked_fill(kpm[:, None, None, :], float("-inf"))
    o = F.scaled_dot_product_attention(split(q), split(k), split(v), attn_mask=merged, scale=scale)
    return o.transpose(1, 2).reshape(B, Nq, heads * D)


@pytest.mark.parametrize("use_mask,use_kpm", [(False, False), (True, False), (False, True), (True, True)])
def test_masked_attention_reference_against_sdpa_with_a_merged_mask(use_mask, use_kpm):
    q, k, v, mask, kpm, heads, Dh = _mattn_inputs(12)
    mask, kpm = (mask if use_mask else None), (kpm if use_kpm else None)
    got = S.ref_masked_attention(q, k, v, heads, Dh ** -0.5, mask=mask, key_padding_mask=kpm)
    torch.testing.assert_close(got, _sdpa_masked(q, k, v, heads, Dh, Dh ** -0.5, mask, kpm), rtol=1e-10, atol=1e-10)
    # uint8 key-padding masks (what the kernel is handed) mean the same
    if use_kpm:
        torch.testing.assert_close(S.ref_masked_attention(q, k, v, heads, Dh ** -0.5, mask=mask, key_padding_mask=kpm.to(torch.uint8)), got)


def test_shadow_rejects_a_key_padding_mask_ignored_for_one_sample():
    q, k, v, mask, kpm, heads, Dh = _mattn_inputs(13, dtype=torch.float32)
    q, k, v = q.bfloat16(), k.bfloat16(), v.bfloat16()
    ref = S.ref_masked_attention(q, k, v, heads, Dh ** -0.5, mask=mask, key_padding_mask=kpm)
    right = _sdpa_masked(q.float(), k.float(), v.float(), heads, Dh, Dh ** -0.5, mask, kpm).bfloat16()
    kpm_wrong = kpm.clone()
    kpm_wrong[1] = False                                                     # sample 1 attends to its padded keys
    wrong = _sdpa_masked(q.float(), k.float(), v.float(), heads, Dh, Dh ** -0.5, mask, kpm_wrong).bfloat16()
    assert _shadow_verdict("attn", right, ref) is None
    assert _shadow_verdict("attn", wrong, ref) is not None
    assert torch.equal(wrong[0], right[0]) and torch.equal(wrong[2], right[2])          # (only that sample differs)


def _moments(B, h, w, ld, seed):
    """moments as the VAE encoder's quant_conv leaves them: mean of a few units, log-variance mostly small, some at the clamps"""
    g = _g(seed)
    mom = torch.randn((B, h, w, ld), generator=g) * 3.0
    mom[..., 4:8] = torch.randn((B, h, w, 4), generator=g) * 6.0 - 4.0
    mom[0, 0, :4, 4:8] = torch.tensor([-40.0, 25.0, -30.0, 20.0])
    noise = torch.randn((B, 4, h, w), generator=g)
    return mom, noise


def _posterior_f32(mom, noise, scale, c_logvar=4):
    mean = mom[..., :4].permute(0, 3, 1, 2)
    logvar = mom[..., c_logvar:c_logvar + 4].permute(0, 3, 1, 2).clamp(-30, 20)
    return scale * (mean + torch.exp(0.5 * logvar) * noise)


@pytest.mark.parametrize("ld", [8, 64])
def test_posterior_sample_reference(ld):
    mom, noise = _moments(2, 6, 10, ld, 14)
    got = S.ref_posterior_sample(mom, noise, 0.18215)
    assert got.shape == (2, 4, 6, 10) and got.dtype == D
    m = mom.double()
    want = torch.empty_like(got)
    for c in range(4):                                                       # indexing, one channel at a time
        want[:, c] = 0.18215 * (m[..., c] + torch.exp(0.5 * m[..., 4 + c].clamp(-30, 20)) * noise.double()[:, c])
    torch.testing.assert_close(got, want, rtol=1e-14, atol=1e-14)


def test_shadow_rejects_a_posterior_sample_reading_logvar_from_the_wrong_channel():
    """a kernel that takes the log-variance from the second half of the row (ld / 2 + c) is right at ld = 8 and wrong at ld = 64"""
    for ld in (8, 64):
        mom, noise = _moments(2, 16, 24, ld, 15)
        ref = S.ref_posterior_sample(mom, noise, 0.18215)
        assert _shadow_verdict("f32", _posterior_f32(mom, noise, 0.18215), ref) is None
        wrong = _posterior_f32(mom, noise, 0.18215, c_logvar=ld // 2)
        assert (_shadow_verdict("f32", wrong, ref) is None) == (ld == 8)


@pytest.mark.parametrize("H,W", [(64, 64), (64, 96), (256, 384)])
def test_mask_downsample_reference_is_bilinear_one_eighth(H, W):
    g = _g(16)
    mask = torch.rand((2, 1, H, W), generator=g, dtype=D)                      # (not only binary masks)
    got = S.ref_mask_downsample(mask)
    assert got.shape == (2, 1, H // 8, W // 8)
    torch.testing.assert_close(got, F.interpolate(mask, scale_factor=0.125, mode="bilinear"), rtol=1e-12, atol=1e-12)


def test_shadow_rejects_a_mask_downsample_with_h_and_w_swapped():
    g = _g(17)
    H, W = 256, 384
    mask = (torch.rand((2, 1, H, W), generator=g) > 0.5).float()
    ref = S.ref_mask_downsample(mask)
    right = F.interpolate(mask, scale_factor=0.125, mode="bilinear")
    # the wrong kernel walks the same memory as W rows of H pixels and writes W/8 rows of H/8
    wrong = F.interpolate(mask.reshape(2, 1, W, H), scale_factor=0.125, mode="bilinear").reshape(2, 1, H // 8, W // 8)
    assert _shadow_verdict("f32", right, ref) is None
    assert _shadow_verdict("f32", wrong, ref) is not None
    # ... and is invisible on a square mask
    sq = (torch.rand((2, 1, 256, 256), generator=g) > 0.5).float()
    assert _shadow_verdict("f32", F.interpolate(sq.reshape(2, 1, 256, 256), scale_factor=0.125, mode="bilinear"),
                           S.ref_mask_downsample(sq)) is None


def test_embed_tokens_reference_and_the_wrong_sequence_length():
    g = _g(18)
    B, Lc, Dm = 4, 12, 256
    idx = torch.randint(0, 95, (B * Lc,), generator=g, dtype=torch.int32)
    table = torch.randn((95, Dm), generator=g)
    pe = torch.randn((Lc, Dm), generator=g)
    ref = S.ref_embed_tokens(idx, table, pe)
    want = (table.double()[idx.long()].reshape(B, Lc, Dm) + pe.double()[None]).reshape(B * Lc, Dm)
    torch.testing.assert_close(ref, want, rtol=0, atol=0)
    right = (table[idx.long()] + pe.repeat(B, 1)).bfloat16()
    pos_wrong = torch.arange(B * Lc) % 16 % Lc                                # (position modulo 16, not 12: wrong from the second row on)
    wrong = (table[idx.long()] + pe[pos_wrong]).bfloat16()
    assert _shadow_verdict("elementwise", right, ref) is None
    assert _shadow_verdict("elementwise", wrong, ref) is not None
    assert torch.equal(wrong[:Lc], right[:Lc])


def test_f32_class_localisation_factor():
    """k of the "f32" class comes from the reference side: the worst 32 x 32 block ratio of a float32 torch restatement of
    posterior_sample and mask_downsample against the float64 references, at the shapes the shadow runs produce, times 8 (another
    operation order, a fast exp).  The value in CLASSES must be that, up to what another host's float32 exp changes (a factor 1.5)."""
    worst = 0.0
    for i, (B, h, w) in enumerate([(4, 64, 64), (1, 32, 48), (2, 32, 48)]):
        mom, noise = _moments(B, h, w, 8, 20 + i)
        ref = S.ref_posterior_sample(mom, noise, 0.18215)
        r = S.block_ratio(_posterior_f32(mom, noise, 0.18215).double() - ref, ref)
        print(f"posterior_sample {B}x{h}x{w}: float32 restatement block ratio {r:.3e}")
        worst = max(worst, r)
    for i, (B, H, W) in enumerate([(4, 512, 512), (2, 256, 384)]):
        from udifftext_amd import synth
        mask = synth.synthetic_batch(B, H, W, 9, seed=i)["mask"]
        ref = S.ref_mask_downsample(mask)
        r = S.block_ratio(F.interpolate(mask, scale_factor=0.125, mode="bilinear").double() - ref, ref)
        print(f"mask_downsample {B}x{H}x{W}: float32 restatement block ratio {r:.3e}")
        worst = max(worst, r)
    k = S.CLASSES["f32"][2]
    print(f"worst {worst:.3e} x 8 = {8 * worst:.3e}; CLASSES k {k:g}")
    assert 8 * worst / 1.5 <= k <= 8 * worst * 1.5
