"""Memory footprint of the VAE reverse pass's entry points (udt_attn512_bwd, udt_denoised_f32, udt_seed_add_bf16) as further cases of
the table of tests/test_footprint_gpu.py, registered through that module's own ``case`` decorator as
tests/test_ocr_loss_footprint_gpu.py does it (so tests/test_footprint_cpu.py's "every entry point of the header has a case" sees them
once this module is imported) and run through its ``_run_case``: once on guarded / poisoned buffers with row gaps, once on compact
ones,

  * payloads bit-equal between the two layouts: a poisoned ld gap, a row past n or a guard that reached a result would have made
    it NaN;
  * no guard and no ld gap byte touched, the operands as they were;
  * lse_ws / dsum_ws at exactly their stated size (fp32 [batch * n] each), every byte of them written;
  * no output element left unwritten.
"""
import pytest
import torch

import test_footprint_gpu as T
from test_footprint_gpu import BF16, F32, _chk, _mods, _p, _rand, env  # noqa: F401  (env: the table's fixture)

pytestmark = pytest.mark.gpu

CASES = []                                                  # (name, fn, covered entry points): this module's own


def case(name, covers):
    def deco(fn):
        if name not in [c[0] for c in T.CASES]:             # (a re-import must not register twice)
            T.case(name, covers)(fn)
        CASES.append((name, fn, tuple(covers)))
        return fn
    return deco


def _attn512_bwd_case(b, B, n):
    O, L, lib, P = _mods()
    scale = 512 ** -0.5
    qkv_t = _rand((B, n, 1536), 401).bfloat16()
    qkv = b.inp(qkv_t, ld=1536 + 8, name="q|k|v")
    q, k, v = qkv[..., :512], qkv[..., 512:1024], qkv[..., 1024:]
    qf, kf, vf = (qkv_t[..., i * 512:(i + 1) * 512].float() for i in range(3))
    o_t = (torch.softmax(qf @ kf.transpose(-1, -2) * scale, dim=-1) @ vf).bfloat16()
    o = b.inp(o_t, ld=512 + 8, name="o")
    d_o = b.inp(_rand((B, n, 512), 402, 0.1).bfloat16(), ld=512 + 24, name="d_o")
    dqkv = b.out((B, n, 1536), BF16, ld=1536 + 8, name="dq|dk|dv")
    lse, dsum = b.scratch(B * n * 4, name="lse_ws"), b.scratch(B * n * 4, name="dsum_ws")
    _chk(lib.udt_attn512_bwd(_p(q), _p(k), _p(v), _p(o), _p(d_o), _p(dqkv[..., :512]), _p(dqkv[..., 512:1024]), _p(dqkv[..., 1024:]),
                             _p(lse), _p(dsum), B, n, qkv.stride(1), qkv.stride(1), qkv.stride(1), o.stride(1), d_o.stride(1),
                             dqkv.stride(1), qkv.stride(0), qkv.stride(0), qkv.stride(0), o.stride(0), d_o.stride(0), dqkv.stride(0),
                             scale, O._stream()), "udt_attn512_bwd")
    return {"dqkv": dqkv, "lse": lse, "dsum": dsum}


@case("attn512_bwd B 2 n 40: lse / dsum exact, q|k|v and dq|dk|dv column ranges of guarded buffers", ["udt_attn512_bwd"])
def _attn512_bwd_ragged(b):
    return _attn512_bwd_case(b, 2, 40)


@case("attn512_bwd B 1 n 1: one row", ["udt_attn512_bwd"])
def _attn512_bwd_one_row(b):
    return _attn512_bwd_case(b, 1, 1)


@case("denoised B 3 hw 35, F with 4 of 8 floats a pixel", ["udt_denoised_f32"])
def _denoised(b):
    O, L, lib, P = _mods()
    B, hw = 3, 35
    f = b.inp(_rand((B * hw, 4), 411), ld=8, name="f")
    noised = b.inp(_rand((B, 4, hw), 412), name="noised")
    c_skip, c_out = b.inp(_rand((B,), 413), name="c_skip"), b.inp(_rand((B,), 414), name="c_out")
    out = b.out((B, 4, hw), F32, name="out")
    _chk(lib.udt_denoised_f32(_p(f), _p(noised), _p(c_skip), _p(c_out), _p(out), B, hw, f.stride(0), O._stream()), "udt_denoised_f32")
    return {"out": out}


@case("seed_add B 3 hw 35, channels past 4 left alone", ["udt_seed_add_bf16"])
def _seed_add(b):
    O, L, lib, P = _mods()
    B, hw = 3, 35
    seed = b.inout(_rand((B * hw, 4), 421).bfloat16(), ld=8, name="seed")       # (the gap: channels 4 .. cpad - 1 of each pixel)
    g = b.inp(_rand((B, 4, hw), 422), name="g")
    c_out = b.inp(_rand((B,), 423), name="c_out")
    _chk(lib.udt_seed_add_bf16(_p(seed), _p(g), _p(c_out), B, hw, seed.stride(0), O._stream()), "udt_seed_add_bf16")
    return {"seed": seed}


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_vae_backward_footprint(env, idx):
    name, fn, _ = CASES[idx]
    T._run_case(name, fn, env.dev)


def test_elementwise_entries_vs_float64(env):
    """udt_denoised_f32: one fma per element (2^-23 relative of the two summands' magnitudes); udt_seed_add_bf16: one rounding to bf16
    of the fp32 fma (2^-8 relative, doubled, of the result)"""
    B, h, w, ld, cpad = 3, 5, 7, 8, 64
    f, noised = _rand((B, h, w, ld), 431), _rand((B, 4, h, w), 432)
    c_skip, c_out = _rand((B,), 433), _rand((B,), 434)
    got = env.O.denoised(f.to(env.dev), noised.to(env.dev), c_skip.to(env.dev), c_out.to(env.dev)).cpu().double()
    cs, co = c_skip.double().view(B, 1, 1, 1), c_out.double().view(B, 1, 1, 1)
    f4 = f.double()[..., :4].permute(0, 3, 1, 2)
    ref = cs * noised.double() + co * f4
    mag = (cs * noised.double()).abs() + (co * f4).abs()
    assert bool(((got - ref).abs() <= 2.0 ** -22 * mag).all())
    seed = _rand((B, h, w, cpad), 435).bfloat16()
    g = _rand((B, 4, h, w), 436)
    got = env.O.seed_add_(seed.clone().to(env.dev), g.to(env.dev), c_out.to(env.dev)).cpu()
    assert torch.equal(got[..., 4:], seed[..., 4:])
    ref = seed.double()[..., :4] + (co * g.double()).permute(0, 2, 3, 1)
    mag = seed.double()[..., :4].abs() + (co * g.double()).permute(0, 2, 3, 1).abs()
    assert bool(((got[..., :4].double() - ref).abs() <= 2.0 ** -8 * ref.abs() + 2.0 ** -22 * mag).all())
