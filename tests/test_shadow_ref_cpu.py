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
