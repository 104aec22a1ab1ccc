"""udt_attn512_bwd (csrc/attn512_bwd.hip: flash-attention backward for one head of 512 dims) through the C ABI (``pytest -m gpu``).

dq, dk, dv are held slice by slice with tests/sliced_check.py at the project's margins (2 rms, 4 max, 2^-18 A): the reference is
``backward_ref.attn_bwd_head(..., F64)`` at head_dim 512, the floor its ``emulate=True`` form (P, dS and the results rounded to bf16,
as the kernel's header comment states) minus the reference, the abs scale its "abs" output; the stored GPU forward ``o`` is passed
as the operand.  A slice is what one wave owns: a 32-row block x a 128-column quarter (4096 elements).  Sizes: one row, one tile, a
ragged second tile, more tiles than the one-deep load ring holds; batch strides that differ per operand; q|k|v and dq|dk|dv as column
ranges of [B n, 1536 + 8] matrices; hostile values; determinism; and the host's refusals (nothing launched).
Report lines: profiles/attn512_bwd_report.txt.
"""
import math
import os

import pytest
import torch

import backward_ref as R
import sliced_check as S

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "attn512_bwd_report.txt")
SCALE = 512 ** -0.5
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib, ops
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)

    class Env:
        pass
    Env.ops, Env.L, Env.lib, Env.dev = ops, lib, lib.load(), cuda
    return Env


def _rand(shape, seed, scale=1.0):
    return (torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale).bfloat16().float()


def _inputs(B, n, variant="randn"):
    """(q, k, v, d_o fp32 holding bf16 values [B, n, 512], scale)"""
    q, k, v, d_o = (_rand((B, n, 512), 900 + i) for i in range(4))
    scale = SCALE
    if variant == "one_hot":                                 # score std ~ 90: one key takes all the mass, P one-hot, dS ~ 0
        scale = 4.0
    elif variant == "zero_do":                               # one batch without an incoming gradient
        d_o[-1] = 0
    elif variant == "large_q":                               # |q| ~ 64 against a scale 64 times smaller
        q = (q * 64).bfloat16().float()
        scale = SCALE / 64
    return q, k, v, d_o, scale


def wave_slices(B, n):
    """[B, n, 512]: (batch, 32-row block, 128-column quarter) — the outputs one wave of udt_attn512_bwd owns"""
    for b in range(B):
        for r0 in range(0, n, 32):
            for c0 in range(0, 512, 128):
                yield (b, slice(r0, min(n, r0 + 32)), slice(c0, c0 + 128))


def _reference(q, k, v, d_o, o, scale):
    """(ref64 dict of [B, n, 512], floor dict, abs-scale dict) from tests/backward_ref.py alone"""
    B = q.shape[0]
    ref = {nm: [] for nm in ("dq", "dk", "dv")}
    floor = {nm: [] for nm in ref}
    sq = {nm: 0.0 for nm in ref}
    for b in range(B):
        exact, emul = R.attn_bwd_head(q[b], k[b], v[b], d_o[b], scale, R.F64, emulate="both", o=o[b])
        for nm in ref:
            ref[nm].append(exact[nm])
            floor[nm].append(emul[nm] - exact[nm])
            sq[nm] += float(exact["abs"][nm].double().pow(2).sum())
    numel = q.numel()
    return ({nm: torch.stack(t) for nm, t in ref.items()}, {nm: torch.stack(t) for nm, t in floor.items()},
            {nm: math.sqrt(val / numel) for nm, val in sq.items()})


def _check(env, name, q, k, v, d_o, scale, run):
    """run(qb, kb, vb, ob, gb) -> d(q|k|v) [B, n, 1536] on the device, for bf16 device operands laid out by the caller"""
    B, n = q.shape[:2]
    dev = lambda t: t.bfloat16().to(env.dev)
    qb, kb, vb, gb = dev(q), dev(k), dev(v), dev(d_o)
    ob = env.ops.attention_d512(qb, kb, vb, scale)
    got = run(qb, kb, vb, ob, gb)
    again = run(qb, kb, vb, ob, gb)
    assert got.shape == (B, n, 1536)
    assert torch.equal(got, again), f"{name}: two runs on the same operands differ"
    got = got.float().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: NaN or inf in the result"
    ref, floor, scales = _reference(q, k, v, d_o, ob.float().cpu(), scale)
    for i, nm in enumerate(("dq", "dk", "dv")):
        S.check_sliced(f"attn512 backward {nm} {name}", got[..., i * 512:(i + 1) * 512], ref[nm], floor[nm], wave_slices(B, n),
                       abs_scale=scales[nm], report=REPORT)
    return got


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 97, 160])
def test_sizes(env, n):
    q, k, v, d_o, scale = _inputs(1, n)
    _check(env, f"B1 n{n}", q, k, v, d_o, scale, lambda qb, kb, vb, ob, gb: env.ops.attention_d512_bwd(qb, kb, vb, ob, gb, scale))


def _padded(env, t, rows_pad, ld):
    """a [B, n, C] row view with row stride ld and batch stride (n + rows_pad) * ld; the padding holds NaN"""
    B, n, C = t.shape
    buf = torch.full((B, n + rows_pad, ld), float("nan"), dtype=BF16, device=env.dev)
    buf[:, :n, :C] = t
    return buf[:, :n, :C]


def test_batch_strides_and_column_ranges(env):
    """n = 97 at B = 2: q|k|v are column ranges of one [B n, 1536 + 8] matrix, dq|dk|dv of another, o and d_o have row and batch
    strides of their own; everything between the operands is NaN and must stay out of the result"""
    B, n = 2, 97
    q, k, v, d_o, scale = _inputs(B, n)

    def run(qb, kb, vb, ob, gb):
        qkv = _padded(env, torch.cat((qb, kb, vb), dim=-1), 3, 1536 + 8)
        o_v, g_v = _padded(env, ob, 1, 512 + 8), _padded(env, gb, 5, 512 + 24)
        out = torch.full((B, n + 2, 1536 + 8), float("nan"), dtype=BF16, device=env.dev)
        view = out[:, :n]
        assert len({qkv.stride(0), o_v.stride(0), g_v.stride(0), view.stride(0)}) == 4
        got = env.ops.attention_d512_bwd(qkv[..., :512], qkv[..., 512:1024], qkv[..., 1024:], o_v, g_v, scale, out=view)
        assert bool(torch.isnan(out[:, n:]).all()) and bool(torch.isnan(out[:, :n, 1536:]).all()), "padding of dq|dk|dv written"
        return got.contiguous()
    strided = _check(env, f"B{B} n{n} strided", q, k, v, d_o, scale, run)
    dev = lambda t: t.bfloat16().to(env.dev)
    qb, kb, vb, gb = dev(q), dev(k), dev(v), dev(d_o)
    ob = env.ops.attention_d512(qb, kb, vb, scale)
    dense = env.ops.attention_d512_bwd(qb, kb, vb, ob, gb, scale).float().cpu()
    assert torch.equal(strided, dense), "the result depends on the strides"


@pytest.mark.parametrize("variant", ["one_hot", "zero_do", "large_q"])
def test_hostile_inputs(env, variant):
    B, n = 2, 97
    q, k, v, d_o, scale = _inputs(B, n, variant)
    got = _check(env, f"B{B} n{n} {variant}", q, k, v, d_o, scale,
                 lambda qb, kb, vb, ob, gb: env.ops.attention_d512_bwd(qb, kb, vb, ob, gb, scale))
    if variant == "zero_do":
        # dq and dv rows belong to the batch; dk too (keys of batch 1 see only queries of batch 1)
        assert bool((got[-1] == 0).all()), "d_o == 0 for the batch, dq / dk / dv are not exactly zero"
        assert bool((got[0] != 0).any())


def test_domain_is_refused_on_the_host(env):
    """misaligned pointers, ld % 8 != 0, n = 0, a null pointer: the library's error codes, nothing launched (the outputs keep
    their fill)"""
    B, n = 1, 40
    dev = env.dev
    t = lambda cols=512: torch.zeros((B, n + 1, cols), dtype=BF16, device=dev)
    q, k, v, o, g = t(), t(), t(), t(), t()
    out = torch.full((B, n + 1, 1536 + 16), 7.0, dtype=BF16, device=dev)
    ws = torch.full((2, B * n), 7.0, dtype=torch.float32, device=dev)
    lib = env.lib

    def call(**kw):
        a = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), d_o=g.data_ptr(), dq=out.data_ptr(),
                 dk=out.data_ptr() + 1024, dv=out.data_ptr() + 2048, lse=ws[0].data_ptr(), dsum=ws[1].data_ptr(), batch=B, n=n,
                 ldq=512, ldk=512, ldv=512, ldo=512, lddo=512, ldd=out.stride(1), sq=0, sk=0, sv=0, so=0, sdo=0, sd=0)
        a.update(kw)
        return lib.udt_attn512_bwd(a["q"], a["k"], a["v"], a["o"], a["d_o"], a["dq"], a["dk"], a["dv"], a["lse"], a["dsum"], a["batch"],
                                   a["n"], a["ldq"], a["ldk"], a["ldv"], a["ldo"], a["lddo"], a["ldd"], a["sq"], a["sk"], a["sv"], a["so"],
                                   a["sdo"], a["sd"], SCALE, env.ops._stream())
    BAD_SHAPE, BAD_ARG = -1, -2
    for nm in ("q", "k", "v", "o", "d_o"):
        assert call(**{nm: q.data_ptr() + 2}) == BAD_ARG, f"{nm} off by one element"
        assert call(**{nm: q.data_ptr() + 8}) == BAD_ARG, f"{nm} 8-byte aligned only"
        assert call(**{nm: None}) == BAD_ARG, f"{nm} null"
    for nm in ("dq", "dk", "dv"):
        assert call(**{nm: out.data_ptr() + 2}) == BAD_ARG, f"{nm} off by one element"
        assert call(**{nm: None}) == BAD_ARG, f"{nm} null"
    assert call(lse=None) == BAD_ARG and call(dsum=None) == BAD_ARG
    for nm in ("ldq", "ldk", "ldv", "ldo", "lddo", "ldd"):
        assert call(**{nm: 516}) == BAD_SHAPE, f"{nm} % 8 != 0"
        assert call(**{nm: 504}) == BAD_SHAPE, f"{nm} < 512"
    for nm in ("sq", "sk", "sv", "so", "sdo", "sd"):
        assert call(**{nm: 4}) == BAD_SHAPE, f"{nm} % 8 != 0"
    assert call(n=0) == BAD_SHAPE and call(n=-3) == BAD_SHAPE and call(batch=0) == BAD_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 7.0).all()), "a refused call wrote something"
    assert call() == 0                                        # and the same arguments, unbroken, run
    torch.cuda.synchronize()
    assert bool((out[:, :n, :1536] == 0).all()) and bool((out[:, n:] == 7.0).all()) and bool((out[:, :, 1536:] == 7.0).all())
