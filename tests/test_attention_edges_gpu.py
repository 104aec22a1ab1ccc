"""The forward attention kernels (csrc/attention.hip, csrc/tattn.hip) at the edges no other kernel-level test launches (``pytest -m
gpu``): every instantiation and dispatch branch of the launchers — attn_d64_kernel / attn_d64_v2_kernel at 1 .. 6 key tiles with
ragged query and key tails and 1 .. 18 work units, all four (q32 | q64) x (whole | key split) forms of the 512-dim kernel with ragged
tails, xattn_kernel at L = 1 .. 16 and head_dim 64 / 128, mattn_kernel with fully masked rows, softmax_rows_kernel, tattn_fused_kernel at
1 .. 8 channel splits with and without tables — each result held slice by slice (one wave's or one workgroup's outputs) to a float64
reference by tests/sliced_check.py with its recorded margins, the bounds from tests/attention_ref.py's emulation of the kernel's stated
roundings (never from the kernel's output), every launch repeated bit for bit, and the rows past a ragged result untouched.
Inputs and checks: tests/attention_cases.py, the same ones tests/test_attention_ref_cpu.py shows a float32 CPU evaluation to pass.
One line per check goes to attention_edges_report.txt next to the run's parity report (tests/test_backward_gpu.py REPORT);
profiles/attention_edges_report.txt is a passing run's.
"""
import os
import tempfile

import pytest
import torch

import attention_cases as K
import attention_ref as R
import sliced_check as S
import test_backward_gpu

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(test_backward_gpu.REPORT), "attention_edges_report.txt")     # a file of its own, same directory
PAD_ROWS = 3


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib, ops
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)

    class Env:
        @staticmethod
        def traced(fn):
            """(fn(), the tags of the launches it made in the library's profiler)"""
            ops.prof_reset(); Env.lib.udt_prof_trace(1); ops.prof_enable(0x3f)
            try:
                out = fn()
                torch.cuda.synchronize()
            finally:
                ops.prof_enable(0)
            path = os.path.join(tempfile.gettempdir(), "udt_attention_edges_trace.csv")
            Env.lib.udt_prof_dump(path.encode())
            Env.lib.udt_prof_trace(0)
            return out, [ln.split(",", 2)[2] for ln in open(path).read().splitlines()[1:]]
    Env.ops, Env.L, Env.lib, Env.dev = ops, lib, lib.load(), cuda
    return Env


def _bf(env, t):
    return t.bfloat16().to(env.dev).contiguous()


def _on(env, *ts):
    return tuple(None if t is None else t.to(env.dev) for t in ts)


def _marked(env, B, n, C):
    """a bf16 result buffer with PAD_ROWS more rows per sample than the launch may write, pre-filled with the marker"""
    full = torch.full((B, n + PAD_ROWS, C), K.MARKER, dtype=torch.bfloat16, device=env.dev)
    return full, full[:, :n]


def _untouched(full, n, what):
    assert bool((full[:, n:] == K.MARKER).all()), f"{what}: rows past the result were written"


# ------------------------------------------------------------------------------------------------ flash attention, head_dim 64
def _d64_case(env, entry, B, H, nq, nk, variant):
    q, k, v = K.flash_inputs(B, H, nq, nk, variant)
    exp = R.flash_ref_emul(*_on(env, q, k, v), H, 0.125, kernel=K.D64_RULE[entry])
    qb, kb, vb = _bf(env, q), _bf(env, k), _bf(env, v)
    if entry == "vt":
        vt = vb.transpose(1, 2).contiguous()
        run = lambda out: env.ops.attention(qb, kb, vt, H, 0.125, out=out)
    else:
        run = lambda out: env.ops.attention_rowv(qb, kb, vb, H, 0.125, out=out)
    full, out = _marked(env, B, nq, H * 64)
    run(out)
    p = K.d64_launch(B, H, nq, nk)
    name = f"edge attn d64 {entry} B{B} H{H} nq{nq} nk{nk} {variant} (units {p['units']} of G {p['G']}, {p['ntiles']} key tiles)"
    K.hold_flash(name, out, exp, B, H, nq, report=REPORT)
    _untouched(full, nq, name)
    full2, out2 = _marked(env, B, nq, H * 64)
    run(out2)
    assert torch.equal(full, full2), f"{name}: not deterministic"


@pytest.mark.parametrize("entry,nk", [(e, nk) for e, nks in (("vt", K.D64_NK), ("rowv", K.D64_NK_ROWV)) for nk in nks])
def test_flash_attention_d64_edges(env, entry, nk):
    for B, H, nq, nk_ in K.D64_SHAPES[entry]:
        if nk_ == nk:
            _d64_case(env, entry, B, H, nq, nk, "randn")


@pytest.mark.parametrize("variant", K.FLASH_VARIANTS)
@pytest.mark.parametrize("entry", ["vt", "rowv"])
def test_flash_attention_d64_hostile_values(env, entry, variant):
    for B, H, nq, nk in K.D64_VARIANT_SHAPES:
        _d64_case(env, entry, B, H, nq, nk, variant)


# ------------------------------------------------------------------------------------------------ flash attention, one head of 512
def _d512_case(env, B, nq, nk, key_split, variant):
    plan = K.attn512_plan(B, nq, nk, key_split)
    q, k, v = K.flash_inputs(B, 1, nq, nk, variant, head_dim=512)
    exp = R.flash_ref_emul(*_on(env, q, k, v), 1, 512 ** -0.5, 512, kernel="d512", ksplit=plan["ksplit"], kt_per=plan["kt_per"])
    qb, kb, vb = _bf(env, q), _bf(env, k), _bf(env, v)
    full, out = _marked(env, B, nq, 512)
    _, tags = env.traced(lambda: env.ops.attention_d512(qb, kb, vb, 512 ** -0.5, out=out, key_split=key_split))
    # the launch's own tag names the plan: a later change of the plan cannot silently move this case to another kernel
    assert tags == [f"attn512 B={B} nq={nq} nk={nk} ksplit={plan['ksplit']}"], (tags, plan)
    if key_split:
        ks = K.a5_key_split(B, nq, nk)
        assert env.lib.udt_attn512_workspace_bytes(B, nq, nk) == (B * ks * nq * 514 * 4 if ks > 1 else 0)
    name = (f"edge attn d512 B{B} nq{nq} nk{nk} {variant} (q{plan['q']}, ksplit {plan['ksplit']} x {plan['kt_per']} tiles, last "
            f"{plan['last']})")
    K.hold_flash(name, out, exp, B, 1, nq, head_dim=512, report=REPORT)
    _untouched(full, nq, name)
    full2, out2 = _marked(env, B, nq, 512)
    env.ops.attention_d512(qb, kb, vb, 512 ** -0.5, out=out2, key_split=key_split)
    assert torch.equal(full, full2), f"{name}: not deterministic"


@pytest.mark.parametrize("B,nq,nk,key_split", K.D512_SHAPES)
def test_flash_attention_d512_edges(env, B, nq, nk, key_split):
    _d512_case(env, B, nq, nk, key_split, "randn")


@pytest.mark.parametrize("variant", K.FLASH_VARIANTS)
def test_flash_attention_d512_hostile_values(env, variant):
    shapes = K.D512_VARIANT_SHAPES + ((K.D512_SPLIT_VARIANT_SHAPE,) if variant in ("neg", "late_spike") else ())
    for B, nq, nk, key_split in shapes:
        _d512_case(env, B, nq, nk, key_split, variant)


# ------------------------------------------------------------------------------------------------ short-context attention
@pytest.mark.parametrize("hd", K.XATTN_HEAD_DIM)
@pytest.mark.parametrize("L", K.XATTN_L)
def test_short_context_attention_edges(env, L, hd):
    B, H = K.XATTN_BH
    C = H * hd
    for nq in K.XATTN_NQ:
        q, kv = K.xattn_inputs(B, H, hd, nq, L)
        ref = R.xattn_fwd(*_on(env, q, kv), H, hd, hd ** -0.5)
        base = R.xattn_probs_base(q, kv, H, hd, hd ** -0.5)
        qb, kvb = _bf(env, q), _bf(env, kv)

        def run(with_probs):
            full = torch.full((B * nq + PAD_ROWS, C), K.MARKER, dtype=torch.bfloat16, device=env.dev)
            pfull = torch.full((B * H * nq * L + 8,), K.MARKER, dtype=torch.float32, device=env.dev)
            probs = pfull[:B * H * nq * L].reshape(B * H, nq, L)
            out = full[:B * nq].reshape(B, nq, C)
            env.ops.xattention(qb, kvb[..., :C], kvb[..., C:], H, hd, hd ** -0.5, probs=probs if with_probs else None, out=out)
            assert bool((full[B * nq:] == K.MARKER).all()), "rows past the result were written"
            assert bool((pfull[B * H * nq * L:] == K.MARKER).all()) and (with_probs or bool((pfull == K.MARKER).all()))
            return full, pfull, out, probs
        full, pfull, out, probs = run(True)
        name = f"edge xattn L{L} D{hd} nq{nq}"
        K.hold_xattn_out(name + " out", out, ref, B, H, hd, nq, report=REPORT)
        K.hold_xattn_probs(name, probs, ref, base, report=REPORT)
        full2, pfull2, _, _ = run(True)
        assert torch.equal(full, full2) and torch.equal(pfull, pfull2), f"{name}: not deterministic"
        full3, _, out3, _ = run(False)                          # probs = NULL: the same output
        K.hold_xattn_out(name + " out, probs NULL", out3, ref, B, H, hd, nq, report=REPORT)
        assert torch.equal(full, full3), f"{name}: the output depends on whether the probabilities are written"


# ------------------------------------------------------------------------------------------------ masked small attention
def _mattn_case(env, D, lk, nq, um, uk, special=None):
    B, H = K.MATTN_BH
    q, k, v, mask, kpm = K.mattn_inputs(B, H, D, nq, lk, um, uk, special)
    ref, a = R.mattn_fwd(*_on(env, q, k, v), H, D ** -0.5, *_on(env, mask, kpm))
    qb, kb, vb = _bf(env, q), _bf(env, k), _bf(env, v)
    mk, kp = _on(env, mask, kpm)
    full, out = _marked(env, B, nq, H * D)
    env.ops.masked_attention(qb, kb, vb, H, D ** -0.5, mask=mk, key_padding_mask=kp, out=out)
    name = f"edge mattn D{D} lk{lk} nq{nq} mask{int(um)} kpm{int(uk)}{' ' + special if special else ''}"
    K.hold_mattn(name, out, ref, a, B, H, D, nq, report=REPORT)
    _untouched(full, nq, name)
    full2, out2 = _marked(env, B, nq, H * D)
    env.ops.masked_attention(qb, kb, vb, H, D ** -0.5, mask=mk, key_padding_mask=kp, out=out2)
    assert torch.equal(full, full2), f"{name}: not deterministic"
    return out, ref


@pytest.mark.parametrize("D,lk", K.MATTN_D_LK)
def test_masked_attention_edges(env, D, lk):
    for nq in K.MATTN_NQ:
        for um in (False, True):
            for uk in (False, True):
                _mattn_case(env, D, lk, nq, um, uk)


@pytest.mark.parametrize("D,lk", K.MATTN_D_LK)
def test_masked_attention_fully_masked_rows_and_huge_ignored_keys(env, D, lk):
    """a fully masked query row is zeros (torch gives NaN) — by the mask alone (row 0) and by mask + key padding (row 2 of sample 1);
    1e30 in K and V at the ignored keys does not reach the output"""
    out, ref = _mattn_case(env, D, lk, 5, True, True, "dead")
    dead = (ref == 0).all(dim=-1)
    assert dead.tolist() == [[True, False, False, False, False], [True, False, True, False, False]]
    assert bool((out[dead] == 0).all()), "a fully masked row is not exactly zero"
    out, ref = _mattn_case(env, D, lk, 5, True, True, "huge")
    assert float(out.float().abs().max()) < 10


# ------------------------------------------------------------------------------------------------ row softmax
@pytest.mark.parametrize("cols", K.SOFTMAX_COLS)
def test_softmax_rows_edges(env, cols):
    x = K.softmax_inputs(cols)
    ref = R.softmax_rows(x.to(env.dev))
    rows, ld = K.SOFTMAX_ROWS, cols + K.SOFTMAX_LD_EXTRA

    def run():
        buf = torch.full((rows + 1, ld), K.MARKER, dtype=torch.bfloat16, device=env.dev)
        buf[:rows, :cols] = x.bfloat16().to(env.dev)
        env.L.check(env.lib.udt_softmax_rows(buf.data_ptr(), rows, cols, ld, torch.cuda.current_stream().cuda_stream), "udt_softmax_rows")
        assert bool((buf[:rows, cols:] == K.MARKER).all()) and bool((buf[rows] == K.MARKER).all()), "elements past cols / rows were written"
        return buf
    buf = run()
    K.hold_softmax(f"edge softmax_rows {rows}x{cols} ld{ld}", buf[:rows, :cols], ref, report=REPORT)
    assert torch.equal(buf, run()), "not deterministic"


# ------------------------------------------------------------------------------------------------ fused text cross-attention
@pytest.mark.parametrize("heads,B,n_tok,L,zero", K.TATTN_SHAPES)
def test_fused_text_attention_edges(env, heads, B, n_tok, L, zero):
    C = heads * 64
    TT, tiles, nsplit = K.tattn_launch(heads, B, n_tok)
    x, kv, wq, wo, gamma, beta, bias = K.tattn_inputs(heads, B, n_tok, L)
    xb, kvb, wqb, wob = (_bf(env, t) for t in (x, kv, wq, wo))
    ga, be, bi = _on(env, gamma, beta, bias)
    name = f"heads{heads} B{B} n{n_tok} L{L} zero{zero} ({tiles} tiles of {TT} x {nsplit} channel splits)"
    # the tables, against the float64 fold
    tabs = env.ops.tattn_prepare(kvb, wqb, wob, ga, be, heads, K.TATTN_SCALE)
    A, BmT = R.tattn_unpack(tabs.A.float(), tabs.BmT.float())
    sc = tabs.sc.clone()
    K.hold_tattn_tables(f"edge tattn tables {name}", {"A": A, "sc": sc, "BmT": BmT},
                        R.tattn_prepare(*_on(env, kv, wq, wo, gamma, beta), heads, K.TATTN_SCALE), report=REPORT)
    again = env.ops.tattn_prepare(kvb, wqb, wob, ga, be, heads, K.TATTN_SCALE)
    assert all(torch.equal(a, b) for a, b in zip(tabs, again)), "tattn_prepare: not deterministic"
    # the fused launch, from the tables it was given (zero_samples == B: NULL tables)
    xd = x.to(env.dev)
    ref, a = R.tattn_fused(xd, A, sc, BmT, bi, heads, zero, K.TATTN_EPS)
    emul = R.tattn_fused(xd, A, sc, BmT, bi, heads, zero, K.TATTN_EPS, emulate=True)
    given = None if zero == B else tabs
    out = env.ops.tattn_fused(xb, given, bi, heads, zero, K.TATTN_EPS)
    K.hold_tattn_out(f"edge tattn fused {name}", out, (ref, emul, a), heads, B, n_tok, report=REPORT)
    assert torch.equal(out[:zero], (xb[:zero].float() + bi).bfloat16()), "zero-context samples are not bit-exact bf16(x + bias)"
    assert torch.equal(out, env.ops.tattn_fused(xb, given, bi, heads, zero, K.TATTN_EPS)), "tattn_fused: not deterministic"
