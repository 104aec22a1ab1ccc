"""tests/attention_ref.py and the bounds of tests/test_attention_edges_gpu.py prove themselves on the CPU (``-m "not gpu"``).

1. Each reference, in float64, equals an independent torch composition (scaled_dot_product_attention, the masked core of
   nn.MultiheadAttention, the unfused LayerNorm -> to_q -> softmax -> to_out chain).
2. For EVERY case of tests/attention_cases.py a float32 evaluation of the reference formula with the kernel's roundings passes the very
   check_sliced call the GPU test makes: the bounds are attainable in fp32 arithmetic on exactly these inputs, hostile ones included.
3. Every planted defect fails that call, and the failure names the slice the defect sits in.
4. The shape lists launch what they claim (pure-Python mirrors of the launchers' rules).
"""
import math
import re

import pytest
import torch
import torch.nn.functional as F

import attention_cases as K
import attention_ref as R
import sliced_check as S

F32, F64 = torch.float32, torch.float64


@pytest.fixture()
def rep(tmp_path):
    return str(tmp_path / "attention_edges_report.txt")


def _fails(match, fn, *args, **kw):
    with pytest.raises(AssertionError) as e:
        fn(*args, **kw)
    for m in ([match] if isinstance(match, str) else match):
        assert m in str(e.value), f"the failure does not name {m}: {e.value}"


def _fails_only_at(where, fn, *args, **kw):
    """fn fails, and every slice its message names is ``where`` (check_sliced lists a slice once per bound it misses)"""
    with pytest.raises(AssertionError) as e:
        fn(*args, **kw)
    named = re.findall(r"slice (\[[^\]]*\])", str(e.value))
    assert named and set(named) == {where} and re.search(r": [12] of \d+ slices", str(e.value)), str(e.value)


def _sdpa(q, k, v, heads, hd, scale, mask=None):
    qh, kh, vh = (R._heads(t.double(), heads, hd) for t in (q, k, v))
    return R._unheads(F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, scale=scale))


# ------------------------------------------------------------------------------------------------ 1. the references
@pytest.mark.parametrize("B,H,nq,nk,hd", [(2, 3, 70, 200, 64), (2, 1, 45, 333, 512)])
def test_flash_reference_is_scaled_dot_product_attention(B, H, nq, nk, hd):
    q, k, v = K.flash_inputs(B, H, nq, nk, head_dim=hd)
    ref, a = R.flash_fwd(q, k, v, H, hd ** -0.5, hd)
    want = _sdpa(q, k, v, H, hd, hd ** -0.5)
    assert float((ref - want).abs().max()) < 1e-13
    assert a >= R.rms(ref)
    # the online forms are the same function up to the P and output roundings (2^-9 each), whatever the tile, maximum rule and key split
    for kernel, ksplit, kt_per in (("d64", 1, 0), ("v2", 1, 0), ("d512", 1, 0), ("d512", 3, 4)):
        emul = R.flash_fwd(q, k, v, H, hd ** -0.5, hd, emulate=True, kernel=kernel, ksplit=ksplit, kt_per=kt_per)
        assert float((emul - want).abs().max()) < 2.0 ** -7 * float(want.abs().max()), kernel


@pytest.mark.parametrize("L", [1, 2, 16])
def test_xattn_reference(L):
    q, kv = K.xattn_inputs(2, 2, 128, 40, L)
    r = R.xattn_fwd(q, kv, 2, 128, 128 ** -0.5)
    if L > 1:
        want = _sdpa(q, kv[..., :256], kv[..., 256:], 2, 128, 128 ** -0.5)
    else:
        sim = torch.einsum("bnhd,bhd->bnh", q.double().reshape(2, 40, 2, 128), kv.double()[:, 0, :256].reshape(2, 2, 128)) * 128 ** -0.5
        want = (torch.sigmoid(sim)[..., None] * kv.double()[:, 0, 256:].reshape(2, 1, 2, 128)).reshape(2, 40, 256)
    assert float((r["out"] - want).abs().max()) < 1e-13
    assert r["probs"].shape == (4, 40, L) and K.R.xattn_probs_base(q, kv, 2, 128, 128 ** -0.5) < 1e-6


def test_mattn_reference_and_fully_masked_rows():
    B, H, D, nq, lk = 2, 2, 32, 5, 65
    q, k, v, mask, kpm = K.mattn_inputs(B, H, D, nq, lk, True, True, special="dead")
    ref, _ = R.mattn_fwd(q, k, v, H, D ** -0.5, mask, kpm)
    full = mask.double()[None, None] + torch.zeros((B, 1, 1, lk), dtype=F64).masked_fill(kpm[:, None, None, :], -math.inf)
    qh, kh, vh = (R._heads(t.double(), H, D) for t in (q, k, v))
    want = R._unheads(torch.softmax(qh @ kh.transpose(-1, -2) * D ** -0.5 + full, dim=-1) @ vh)       # (NaN where a row is fully masked)
    dead = torch.isnan(want).all(dim=-1)
    assert torch.equal(dead, torch.isinf(full).all(dim=-1)[:, 0])
    live_sdpa = _sdpa(q, k, v, H, D, D ** -0.5, mask=full)[~dead]
    assert float((ref[~dead] - live_sdpa).abs().max()) < 1e-13
    assert bool(dead[0, 0]) and bool(dead[1, 0]) and bool(dead[1, 2]) and not bool(dead[0, 2]) and int(dead.sum()) == 3
    assert bool((ref[dead] == 0).all()) and not bool((ref[~dead] == 0).all(dim=-1).any())
    assert float((ref[~dead] - want[~dead]).abs().max()) < 1e-13
    q, k, v, mask, kpm = K.mattn_inputs(B, H, D, nq, lk, True, True, special="huge")
    ref, a = R.mattn_fwd(q, k, v, H, D ** -0.5, mask, kpm)
    assert float(k.abs().max()) > 9e29 and float(ref.abs().max()) < 10 and a < 10, "the ignored keys' 1e30 reached the output"


def test_softmax_reference():
    x = K.softmax_inputs(2056)
    ref = R.softmax_rows(x)
    want = torch.exp(x.double() - torch.logsumexp(x.double(), dim=-1, keepdim=True))
    assert float((ref - want).abs().max()) < 1e-14
    assert float((ref[1] - 1 / 2056).abs().max()) < 1e-15 and float(ref[2, 1028]) > 1 - 1e-12 and float(ref[2, 0]) < 1e-40


@pytest.mark.parametrize("heads,L", [(5, 12), (10, 5), (5, 1)])
def test_tattn_references_are_the_unfused_chain(heads, L):
    B, N, C = 2, 64, heads * 64
    x, kv, wq, wo, gamma, beta, bias = K.tattn_inputs(heads, B, N, L)
    t = R.tattn_prepare(kv, wq, wo, gamma, beta, heads, K.TATTN_SCALE)
    got, _ = R.tattn_fused(x, t["A"], torch.stack((t["A"].sum(dim=-1), t["c"]), dim=-1), t["BmT"], bias, heads, 1, K.TATTN_EPS)
    y = F.layer_norm(x.double(), (C,), gamma.double(), beta.double(), K.TATTN_EPS)
    o = _sdpa(y @ wq.double().t(), kv[..., :C], kv[..., C:], heads, 64, K.TATTN_SCALE)
    want = o @ wo.double().t() + bias.double() + x.double()
    want[:1] = x[:1].double() + bias.double()
    assert float((got - want).abs().max()) < 1e-11
    A, BmT = t["A"].float(), t["BmT"].float()
    pa, pb = R.tattn_pack(A, BmT)
    ua, ub = R.tattn_unpack(pa, pb)
    assert torch.equal(ua, A) and torch.equal(ub, BmT) and not torch.equal(pa, A)
    hp = R.tattn_hp(heads)
    assert bool((t["c"][t["pad"]] == -1e30).all()) and int(t["pad"].sum()) == B * (hp - heads * L)


# ------------------------------------------------------------------------------------------------ 2. float32 attains every bound
def _flash_case(B, H, nq, nk, variant, hd, **plan):
    q, k, v = K.flash_inputs(B, H, nq, nk, variant, head_dim=hd)
    exp = R.flash_ref_emul(q, k, v, H, hd ** -0.5, hd, **plan)
    got = R.flash_fwd(q, k, v, H, hd ** -0.5, hd, dtype=F32, emulate=True, **plan)
    return (q, k, v), exp, got


@pytest.mark.parametrize("entry", ["vt", "rowv"])
def test_float32_d64_passes_every_shape(entry, rep):
    for B, H, nq, nk in K.D64_SHAPES[entry]:
        _, exp, got = _flash_case(B, H, nq, nk, "randn", 64, kernel=K.D64_RULE[entry])
        K.hold_flash(f"fp32 d64 {entry} B{B} H{H} nq{nq} nk{nk}", got, exp, B, H, nq, report=rep)


@pytest.mark.parametrize("variant", K.FLASH_VARIANTS)
@pytest.mark.parametrize("entry", ["vt", "rowv"])
def test_float32_d64_passes_every_variant(entry, variant, rep):
    for B, H, nq, nk in K.D64_VARIANT_SHAPES:
        (q, k, v), exp, got = _flash_case(B, H, nq, nk, variant, 64, kernel=K.D64_RULE[entry])
        K.hold_flash(f"fp32 d64 {entry} B{B} H{H} nq{nq} nk{nk} {variant}", got, exp, B, H, nq, report=rep)
        if variant == "grow":                                   # the maxima grow, by less than A2_DEFER after the first tile
            s2 = R._heads(q.double(), H, 64) @ R._heads(k.double(), H, 64).transpose(-1, -2) * (0.125 * R.LOG2E)
            grow = s2.max(dim=-1).values - s2[..., :64].max(dim=-1).values
            assert 3.0 < float(grow.min()) and float(grow.max()) < R.A2_DEFER


def _d512_plan(B, nq, nk, key_split):
    plan = K.attn512_plan(B, nq, nk, key_split)
    return plan, {"kernel": "d512", "ksplit": plan["ksplit"], "kt_per": plan["kt_per"]}


@pytest.mark.parametrize("B,nq,nk,key_split", K.D512_SHAPES)
def test_float32_d512_passes_every_shape(B, nq, nk, key_split, rep):
    plan, kw = _d512_plan(B, nq, nk, key_split)
    _, exp, got = _flash_case(B, 1, nq, nk, "randn", 512, **kw)
    K.hold_flash(f"fp32 d512 B{B} nq{nq} nk{nk} q{plan['q']} ksplit{plan['ksplit']}", got, exp, B, 1, nq, head_dim=512, report=rep)


@pytest.mark.parametrize("variant", K.FLASH_VARIANTS)
def test_float32_d512_passes_every_variant(variant, rep):
    shapes = K.D512_VARIANT_SHAPES + ((K.D512_SPLIT_VARIANT_SHAPE,) if variant in ("neg", "late_spike") else ())
    for B, nq, nk, key_split in shapes:
        plan, kw = _d512_plan(B, nq, nk, key_split)
        _, exp, got = _flash_case(B, 1, nq, nk, variant, 512, **kw)
        K.hold_flash(f"fp32 d512 B{B} nq{nq} nk{nk} {variant}", got, exp, B, 1, nq, head_dim=512, report=rep)


@pytest.mark.parametrize("hd", K.XATTN_HEAD_DIM)
@pytest.mark.parametrize("L", K.XATTN_L)
def test_float32_xattn_passes(L, hd, rep):
    B, H = K.XATTN_BH
    for nq in K.XATTN_NQ:
        q, kv = K.xattn_inputs(B, H, hd, nq, L)
        ref = R.xattn_fwd(q, kv, H, hd, hd ** -0.5)
        got = R.xattn_fwd(q, kv, H, hd, hd ** -0.5, dtype=F32, emulate=True)
        K.hold_xattn_out(f"fp32 xattn out L{L} D{hd} nq{nq}", got["out"], ref, B, H, hd, nq, report=rep)
        base = R.xattn_probs_base(q, kv, H, hd, hd ** -0.5)     # (printed to the report: the measured base of the probabilities' bound)
        assert 0 < base < 1e-6
        K.hold_xattn_probs(f"fp32 xattn probs L{L} D{hd} nq{nq}", got["probs"], ref, base, report=rep)
        _fails("probs off", K.hold_xattn_probs, "one probability moved", ref["probs"] + 16 * base * (torch.arange(L) == L - 1), ref, base, report=rep)


def _mattn_run(B, H, D, nq, lk, um, uk, special, rep, what="fp32"):
    q, k, v, mask, kpm = K.mattn_inputs(B, H, D, nq, lk, um, uk, special)
    ref, a = R.mattn_fwd(q, k, v, H, D ** -0.5, mask, kpm)
    got = R.mattn_fwd(q, k, v, H, D ** -0.5, mask, kpm, dtype=F32, emulate=True)
    K.hold_mattn(f"{what} mattn D{D} lk{lk} nq{nq} mask{int(um)} kpm{int(uk)} {special or ''}", got, ref, a, B, H, D, nq, report=rep)


@pytest.mark.parametrize("D,lk", K.MATTN_D_LK)
def test_float32_mattn_passes(D, lk, rep):
    B, H = K.MATTN_BH
    assert K.mattn_guard_ok(D, lk)
    for nq in K.MATTN_NQ:
        for um in (False, True):
            for uk in (False, True):
                _mattn_run(B, H, D, nq, lk, um, uk, None, rep)
    for special in ("dead", "huge"):
        _mattn_run(B, H, D, 5, lk, True, True, special, rep)


@pytest.mark.parametrize("cols", K.SOFTMAX_COLS)
def test_float32_softmax_rows_passes(cols, rep):
    x = K.softmax_inputs(cols)
    K.hold_softmax(f"fp32 softmax_rows cols{cols}", R.softmax_rows(x, dtype=F32, emulate=True), R.softmax_rows(x), report=rep)


def _tattn_case(heads, B, n_tok, L, zero, dtype=F32, **defect):
    """(expected of the fused launch, a ``dtype`` evaluation of it, the float64 tables, float32-evaluated tables): tables as the prepare
    kernel stores them — bf16 A' and Bm^T, fp32 (s, c)"""
    x, kv, wq, wo, gamma, beta, bias = K.tattn_inputs(heads, B, n_tok, L)
    t64 = R.tattn_prepare(kv, wq, wo, gamma, beta, heads, K.TATTN_SCALE)
    t32 = R.tattn_prepare(kv, wq, wo, gamma, beta, heads, K.TATTN_SCALE, dtype=F32, emulate=True)
    tabs = {"A": t32["A"], "sc": torch.stack((t32["s"], t32["c"]), dim=-1), "BmT": t32["BmT"]}
    args = (x, tabs["A"], tabs["sc"], tabs["BmT"], bias, heads, zero, K.TATTN_EPS)
    ref, a = R.tattn_fused(*args)
    emul = R.tattn_fused(*args, emulate=True)
    got = R.tattn_fused(*args, dtype=dtype, emulate=True, **defect)
    return (ref, emul, a), got, t64, tabs


@pytest.mark.parametrize("heads,B,n_tok,L,zero", K.TATTN_SHAPES)
def test_float32_tattn_passes(heads, B, n_tok, L, zero, rep):
    exp, got, t64, tabs = _tattn_case(heads, B, n_tok, L, zero)
    K.hold_tattn_out(f"fp32 tattn heads{heads} B{B} n{n_tok} L{L} zero{zero}", got, exp, heads, B, n_tok, report=rep)
    x, _, _, _, _, _, bias = K.tattn_inputs(heads, B, n_tok, L)
    assert torch.equal(got[:zero], R.bf(x[:zero] + bias))
    K.hold_tattn_tables(f"fp32 tattn tables heads{heads} B{B} L{L}", tabs, t64, report=rep)


# ------------------------------------------------------------------------------------------------ 3. planted defects
DEFECT_SHAPE = (2, 2, 129, 200)                                 # a d64 variant shape: 4 key tiles, the last one partial


@pytest.mark.parametrize("kernel", ["d64", "v2"])
def test_defects_in_a_d64_launch(kernel, rep):
    B, H, nq, nk = DEFECT_SHAPE
    bad = lambda variant, **d: R.flash_fwd(*K.flash_inputs(B, H, nq, nk, variant), H, 0.125, emulate=True, kernel=kernel, **d)
    exp = {v: R.flash_ref_emul(*K.flash_inputs(B, H, nq, nk, v), H, 0.125, kernel=kernel) for v in ("randn", "neg", "late_spike", "grow")}
    hold = lambda variant, got: K.hold_flash(f"defect {variant}", got, exp[variant], B, H, nq, report=rep)
    hold("randn", bad("randn"))
    _fails("slice [0, 0:32, 0:64]", hold, "randn", bad("randn", drop_last_key=True))               # (every slice fails: the first is named first)
    hold("neg", bad("neg"))
    _fails("slice [0, 0:32, 0:64]", hold, "neg", bad("neg", pad_score0=1))
    # (on randn one padded key among 200 takes 1 / sum_j exp(s_j) = 0.3 % of every row's mass: a uniform relative error AT the bf16
    #  floor, which no bound derived from the roundings can see — as test_sliced_check_cpu.py's defect f; ``neg`` is the input that shows it)
    _fails("slice [0, 0:32, 0:64]", hold, "late_spike", bad("late_spike", skip_rescale=3))
    if kernel == "d64":                                         # (v2 defers every rescale of ``grow`` by design: nothing to skip)
        _fails("out of bound", hold, "grow", bad("grow", skip_rescale=2))
    _fails_only_at("[1, 96:128, 64:128]", hold, "randn", bad("randn", stale_block=((1, 1, 96), (0, 1))))
    # the one live query of the second workgroup (64 elements: check_sliced merges it with the units that follow, named by the first)
    _fails_only_at("[1, 128:129, 0:64]", hold, "randn", bad("randn", stale_block=((1, 0, 128), (1, 1))))


def test_defects_in_a_d512_launch(rep):
    B, nq, nk, key_split = 2, 33, 1056, True
    plan, kw = _d512_plan(B, nq, nk, key_split)
    assert plan["ksplit"] == 4
    qkv = K.flash_inputs(B, 1, nq, nk, head_dim=512)
    exp = R.flash_ref_emul(*qkv, 1, 512 ** -0.5, 512, **kw)
    bad = lambda **d: R.flash_fwd(*qkv, 1, 512 ** -0.5, 512, emulate=True, **kw, **d)
    hold = lambda got: K.hold_flash("defect d512", got, exp, B, 1, nq, head_dim=512, report=rep)
    hold(bad())
    for z in range(4):
        _fails("slice [0, 0:32, 0:128]", hold, bad(drop_slice=z))
    _fails("slice [0, 0:32, 0:128]", hold, bad(drop_last_key=True))
    # the second 32-query tile of sample 1 is ONE live query: its four quarters (512 elements, fewer than MIN_SLICE) join the slice in
    # front of them, which is the only one that fails and is named by its first unit
    with pytest.raises(AssertionError) as e:
        hold(bad(stale_block=((1, 0, 32), (0, 0))))
    assert set(re.findall(r"slice (\[[^\]]*\] \(\d+ elements\))", str(e.value))) == {"[1, 0:32, 384:512] (4608 elements)"}, str(e.value)
    nqkv = K.flash_inputs(B, 1, nq, nk, "neg", head_dim=512)
    _fails("slice [0, 0:32, 0:128]", K.hold_flash, "defect d512 neg", R.flash_fwd(*nqkv, 1, 512 ** -0.5, 512, emulate=True, **kw, pad_score0=1),
           R.flash_ref_emul(*nqkv, 1, 512 ** -0.5, 512, **kw), B, 1, nq, head_dim=512, report=rep)
    lqkv = K.flash_inputs(B, 1, nq, nk, "late_spike", head_dim=512)
    lexp = R.flash_ref_emul(*lqkv, 1, 512 ** -0.5, 512, **kw)
    _fails("out of bound", K.hold_flash, "defect d512 late_spike", R.flash_fwd(*lqkv, 1, 512 ** -0.5, 512, emulate=True, **kw, skip_rescale=32),
           lexp, B, 1, nq, head_dim=512, report=rep)


def test_defect_two_heads_swapped_in_tattn(rep):
    heads, B, n_tok, L, zero = 5, 3, 64, 5, 1
    exp, got, _, _ = _tattn_case(heads, B, n_tok, L, zero, dtype=F64, swap_heads=(1, 3))
    with pytest.raises(AssertionError) as e:
        K.hold_tattn_out("defect tattn", got, exp, heads, B, n_tok, report=rep)
    # sample 0 is the zero-context sample (x + bias: no heads), every workgroup of samples 1 and 2 is wrong
    assert "of 24 slices" in str(e.value) and str(e.value).index("slice [") == str(e.value).index("slice [64:128, 0:32]"), str(e.value)


# ------------------------------------------------------------------------------------------------ 4. what the lists launch
def test_d64_lists_cover_the_launcher():
    for entry, nks in (("vt", K.D64_NK), ("rowv", K.D64_NK_ROWV)):
        shapes = K.D64_SHAPES[entry]
        assert {(nq, nk) for _, _, nq, nk in shapes} == {(nq, nk) for nq in K.D64_NQ for nk in nks}
        plans = [K.d64_launch(*s) for s in shapes]
        assert {(p["ntiles"], p["partial"]) for p in plans} >= {(1, True), (1, False), (2, True), (2, False), (3, True), (3, False),
                                                                (4, True), (5, True), (6, True)}
        if entry == "vt":
            assert all(nk % 8 == 0 for _, _, _, nk in shapes)
        else:
            assert {nk % 8 for _, _, _, nk in shapes} >= {0, 1, 4}
        for nq in K.D64_NQ:                                     # every query count with every unit count it can have, G = 8 and 16
            units = {p["units"] for s, p in zip(shapes, plans) if s[2] == nq}
            assert units == ({8, 2, 14, 18} if nq > 128 else {1, 7, 8, 9}), (nq, units)
        assert {p["G"] for p in plans} == {8, 16, 24} and {p["units"] for p in plans} >= {1, 7, 8, 9}
        assert any(p["units"] < p["G"] for p in plans) and any(p["units"] == p["G"] for p in plans)
        assert {(p["qtiles"], p["ragged_wave"], p["dead_waves"]) for p in plans} == {(1, True, True), (1, True, False), (2, True, True)}
        for s in K.D64_VARIANT_SHAPES:
            p = K.d64_launch(*s)
            assert p["partial"] and p["ragged_wave"] and p["ntiles"] >= 4 and (entry == "rowv" or s[3] % 8 == 0)


def test_d512_list_covers_the_four_instantiations():
    plans = {s: K.attn512_plan(*s) for s in K.D512_SHAPES}
    inst = lambda p: (p["q"], "split" if p["ksplit"] > 1 else "whole")
    assert {inst(p) for p in plans.values()} == {(32, "whole"), (64, "whole"), (32, "split"), (64, "split")}
    for i in ((32, "whole"), (64, "whole"), (32, "split"), (64, "split")):
        mine = [s for s, p in plans.items() if inst(p) == i]
        tails = {s[1] % i[0] for s in mine}
        assert tails == ({1, 31, 33, 63} if i[0] == 64 else {1, 31}), (i, tails)
        assert {s[2] % 32 for s in mine} == {0, 1, 31}, i
    # the arithmetic the shapes were chosen by
    assert plans[(112, 97, 32, False)] == {"q": 64, "ksplit": 1, "kt_per": 0, "last": 1, "ntiles": 1}
    assert plans[(30, 97, 1057, True)] == {"q": 64, "ksplit": 4, "kt_per": 9, "last": 7, "ntiles": 34}
    assert plans[(56, 65, 575, True)]["ksplit"] == 2 and plans[(1, 33, 545, True)]["ksplit"] == 2
    assert plans[(1, 63, 1823, True)] == {"q": 32, "ksplit": 7, "kt_per": 9, "last": 3, "ntiles": 57}
    assert plans[(1, 95, 33, True)]["ksplit"] == 1              # planned through the split entry, too few tiles to split
    for q in (32, 64):                                          # a last slice with fewer tiles than kt_per, on both instantiations
        assert any(p["q"] == q and p["ksplit"] > 1 and p["last"] < p["kt_per"] for p in plans.values())
    # a5_key_split never returns 8: a slice count of 8 costs 1 / 8 + 0.16 in one round, 7 costs 1 / 7 + 0.14 — 7 is the most it plans
    assert max(K.a5_key_split(b, 64, 1 << 15) for b in range(1, 192)) == 7
    for s in K.D512_VARIANT_SHAPES + (K.D512_SPLIT_VARIANT_SHAPE,):
        p = K.attn512_plan(*s)
        assert s[1] % 32 and s[2] % 32
    assert inst(K.attn512_plan(*K.D512_VARIANT_SHAPES[0])) == (64, "whole") and inst(K.attn512_plan(*K.D512_VARIANT_SHAPES[1])) == (32, "split")
    assert inst(K.attn512_plan(*K.D512_SPLIT_VARIANT_SHAPE)) == (64, "split")
    # the plan the existing contract test pins through udt_attn512_workspace_bytes
    assert [K.a5_key_split(*a) for a in ((4, 4096, 4096), (1, 4096, 4096), (1, 64, 4096), (1, 9216, 9216), (1, 64, 300))] == [1, 4, 7, 5, 1]


def test_small_attention_lists():
    assert all(K.mattn_guard_ok(D, lk) for D, lk in K.MATTN_D_LK) and not K.mattn_guard_ok(64, 129) and not K.mattn_guard_ok(32, 257)
    assert {lk for _, lk in K.MATTN_D_LK} >= {63, 64, 65, 129, 256} and {D for D, _ in K.MATTN_D_LK} == {8, 32, 64}
    assert {nq % 4 for nq in K.MATTN_NQ} == {1, 2, 3}
    assert max(K.XATTN_L) == 16 and {1, 2, 13} <= set(K.XATTN_L) and {nq % 256 for nq in K.XATTN_NQ} == {1, 255}
    assert {c // 8 for c in K.SOFTMAX_COLS} == {1, 255, 256, 257}


def test_tattn_list_covers_splits_context_lengths_and_zero_samples():
    seen = {}
    for heads, B, n_tok, L, zero in K.TATTN_SHAPES:
        TT, tiles, nsplit = K.tattn_launch(heads, B, n_tok)
        assert n_tok % TT == 0 and TT == (64 if heads == 5 else 32)
        seen.setdefault(heads, []).append((nsplit, L, "B" if zero == B else zero))
    assert set(seen) == {5, 10, 20}
    for heads, got in seen.items():
        assert {g[0] for g in got} == {1, 2, 4, 8} and {g[1] for g in got} == {1, 5, 12} and {g[2] for g in got} == {0, 1, "B"}, (heads, got)
    assert K.tattn_launch(5, 4, 4096) == (64, 256, 1) and K.tattn_launch(5, 4, 4032)[2] == 2
