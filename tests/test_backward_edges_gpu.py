"""csrc/backward.hip's entry points at the edges no other kernel-level test launches, through the C ABI (``pytest -m gpu``): every
template instantiation and dispatch branch the launchers can take, ragged and tiny sizes, and hostile values — each result held slice
by slice to a float64 reference by tests/sliced_check.py (bounds from tests/backward_ref.py's emulation of the kernel's stated
roundings, never from the kernel's output), fp32 sums element by element to 16 x 2^-24 x sum|summands|, and every launch repeated
bit for bit.  Inputs: tests/backward_cases.py (the same ones tests/test_sliced_check_cpu.py shows a float32 CPU evaluation to pass).
"""
import math
import os

import pytest
import torch

import backward_cases as K
import backward_ref as R
import sliced_check as S

pytestmark = pytest.mark.gpu
SCALE = 64 ** -0.5


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


def _dev(env, t, bf16=True):
    return None if t is None else (t.bfloat16() if bf16 else t).to(env.dev).contiguous()


# ------------------------------------------------------------------------------------------------ flash attention backward
ATTN_SIZES = [(1, 1, 31), (1, 1, 33), (1, 2, 127), (1, 2, 128), (1, 2, 129), (1, 5, 160), (2, 5, 384), (9, 20, 384), (9, 20, 300)]
ATTN_CASES = [(*s, "randn") for s in ATTN_SIZES] + [(B, H, N, v) for (B, H, N) in ((1, 2, 129), (9, 20, 300)) for v in K.ATTN_VARIANTS]


def _attn_instantiation(B, H, N):
    """(load ring depth, FULL) udt_attn_bwd's launcher picks: units = B H ceil(N / 128) <= 512 -> ring 4, else 1; FULL = N % 128 == 0"""
    units = B * H * ((N + 127) // 128)
    return (4 if units <= 512 else 1), N % 128 == 0


def test_the_attention_cases_launch_all_four_instantiations():
    assert "UDT_ATTN_BWD_PF" not in os.environ, "the ring depth must be the launcher's own choice"
    assert {_attn_instantiation(B, H, N) for B, H, N, _ in ATTN_CASES} == {(4, True), (4, False), (1, True), (1, False)}
    assert _attn_instantiation(9, 20, 384) == (1, True) and _attn_instantiation(9, 20, 300) == (1, False)
    for v in K.ATTN_VARIANTS:
        assert (1, 2, 129, v) in ATTN_CASES and (9, 20, 300, v) in ATTN_CASES


@pytest.mark.parametrize("B,H,N,variant", ATTN_CASES)
def test_flash_attention_backward_edges(env, B, H, N, variant):
    qkv, d_o = K.attn_inputs(B, H, N, variant)
    C = H * 64
    qb, gb = _dev(env, qkv), _dev(env, d_o)
    o = env.ops.attention_rowv(qb[..., :C], qb[..., C:2 * C], qb[..., 2 * C:], H, SCALE)
    got = env.ops.attention_bwd(qb, o, gb, H, SCALE)
    again = env.ops.attention_bwd(qb, o, gb, H, SCALE)
    ref, floor, scales = R.attn_ref_emul(qkv, d_o, H, SCALE, o=o.float().cpu())     # (o is an operand: D = rowsum(dO o O))
    got = got.float().cpu()
    ring, full = _attn_instantiation(B, H, N)
    for i, nm in enumerate(("dq", "dk", "dv")):
        c = slice(i * C, (i + 1) * C)
        S.check_sliced(f"edge attention backward {nm} B{B} H{H} N{N} {variant} (ring {ring}, FULL {int(full)})", got[..., c], ref[..., c],
                       floor[..., c], S.attn_slices(B, H, N), abs_scale=scales[nm])
    assert torch.equal(again.float().cpu(), got), "not deterministic"


# ------------------------------------------------------------------------------------------------ text cross-attention backward
def _xattn_case(env, B, H, N, L, use_dp, use_do):
    q, kv, d_o, d_p = K.xattn_inputs(B, H, N, L)
    C = H * 64
    qh = q.double().reshape(B, N, H, 64).permute(0, 2, 1, 3)
    kh = kv.double()[..., :C].reshape(B, L, H, 64).permute(0, 2, 1, 3)
    sim = qh @ kh.transpose(-1, -2) * SCALE
    probs = (sim.softmax(dim=-1) if L > 1 else sim.sigmoid()).reshape(B * H, N, L).float()    # the stored fp32 operand
    dp, do = (d_p if use_dp else None), (d_o if use_do else None)
    ref = R.xattn_bwd(q, kv, dp, do, H, SCALE, probs=probs)
    emul = R.xattn_bwd(q, kv, dp, do, H, SCALE, probs=probs, emulate=True)
    return q, kv, dp, do, probs, ref, emul


@pytest.mark.parametrize("use_dp,use_do", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("L", [1, 13, 16])
def test_text_cross_attention_backward_query_side_edges(env, L, use_dp, use_do):
    B, H = 2, 2
    C = H * 64
    for N in (1, 255, 257):                                 # the kernel's workgroup takes 256 queries
        q, kv, dp, do, probs, ref, emul = _xattn_case(env, B, H, N, L, use_dp, use_do)
        kvb = _dev(env, kv)
        args = (kvb[..., :C], kvb[..., C:], _dev(env, probs, False), _dev(env, dp, False), _dev(env, do), H, SCALE)
        got = env.ops.xattention_bwd(*args)
        S.check_sliced(f"edge text cross-attention dq N{N} L{L} dP{int(use_dp)} dO{int(use_do)}", got, ref["dq"], emul["dq"] - ref["dq"],
                       S.attn_slices(B, H, N), abs_scale=ref["abs"]["dq"])
        assert torch.equal(got, env.ops.xattention_bwd(*args)), "not deterministic"


@pytest.mark.parametrize("use_dp,use_do", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("L", [1, 13, 16])
def test_text_cross_attention_backward_context_side_edges(env, L, use_dp, use_do):
    B, H = 2, 2
    C = H * 64
    for N in (65, 127, 129):                                # query ranges of 128, tiles of 64
        q, kv, dp, do, probs, ref, emul = _xattn_case(env, B, H, N, L, use_dp, use_do)
        kvb = _dev(env, kv)
        args = (_dev(env, q), kvb[..., C:], _dev(env, probs, False), _dev(env, dp, False), _dev(env, do), H, SCALE)
        dk, dv = env.ops.xattention_bwd_kv(*args)
        for nm, got in (("dk", dk), ("dv", dv)):
            S.check_sliced(f"edge text cross-attention {nm} N{N} L{L} dP{int(use_dp)} dO{int(use_do)}", got, ref[nm], emul[nm] - ref[nm],
                           S.attn_slices(B, H, L), abs_scale=ref["abs"][nm])
        dk2, dv2 = env.ops.xattention_bwd_kv(*args)
        assert torch.equal(dk, dk2) and torch.equal(dv, dv2), "not deterministic"


# ------------------------------------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("C", [8, 328, 512, 520, 1024, 1032, 1536, 1544, 2048])
def test_layernorm_backward_edges(env, C):
    """NCH = ceil(C / 512) = 1 .. 4, channel counts that leave a wave partly idle, rows that do not fill the 4-row workgroup"""
    for rows in (1, 5, 303):
        for variant in ("randn",) + K.LN_VARIANTS:
            x, dy, add, gamma = K.ln_inputs(rows, C, variant)
            for a in (None, add):
                ref, scale = R.ln_bwd(x, dy, gamma, 1e-5, a)
                floor = R.ln_bwd(x, dy, gamma, 1e-5, a, emulate=True) - ref
                args = (_dev(env, x), _dev(env, dy), gamma.to(env.dev), 1e-5)
                got = env.ops.layer_norm_bwd(*args, add=_dev(env, a))
                S.check_sliced(f"edge LayerNorm backward {rows}x{C} {variant}{' + add' if a is not None else ''}", got, ref, floor,
                               S.row_col_slices(rows, C, 4, 512), abs_scale=scale)
                assert torch.equal(got, env.ops.layer_norm_bwd(*args, add=_dev(env, a))), "not deterministic"


@pytest.mark.parametrize("variant", ("randn",) + K.LN_VARIANTS)
@pytest.mark.parametrize("rows,C", [(r, c) for c in (320, 2048) for r in (1, 63, 65, 16400)])
def test_layernorm_parameter_gradient_edges(env, rows, C, variant):
    """udt_colparts' cap of 256 workgroups (16400 rows: 65 rows per workgroup, the last ones empty), NCH = 1 and 4"""
    x, dy, _, _ = K.ln_inputs(rows, C, variant)
    dg, db, ag, ab = R.ln_param_grad(x, dy, 1e-5)
    got_g, got_b = env.ops.layer_norm_param_grad(_dev(env, x), _dev(env, dy), 1e-5)
    S.check_fp32_sum(f"edge LayerNorm d gamma {rows}x{C} {variant}", got_g, dg, ag)
    S.check_fp32_sum(f"edge LayerNorm d beta {rows}x{C} {variant}", got_b, db, ab)
    g2, b2 = env.ops.layer_norm_param_grad(_dev(env, x), _dev(env, dy), 1e-5)
    assert torch.equal(got_g, g2) and torch.equal(got_b, b2), "not deterministic"


# ------------------------------------------------------------------------------------------------ GroupNorm
def test_gn_nchunks_changes_at_32_pixels(env):
    assert env.lib.udt_gn_nchunks(31, 320) == 1 and env.lib.udt_gn_nchunks(32, 320) == 2 and env.lib.udt_gn_nchunks(33, 320) == 2


@pytest.mark.parametrize("variant", ("randn",) + K.GN_VARIANTS)
@pytest.mark.parametrize("B,HW,C", [(1, 1, 64), (2, 128, 64), (2, 129, 64), (1, 4, 4160), (1, 32, 320), (1, 33, 320)])
def test_groupnorm_backward_edges(env, B, HW, C, variant):
    """one pixel; two channels per group; the apply kernel's 1024-piece workgroup boundary (128 / 129 pixels of 64 channels); the
    one-workgroup-per-group dispatch for C > 4096 although partials are given; the first pixel count with two chunks and the next"""
    x, dy, add, gamma, beta, silu = K.gn_inputs(B, HW, C, variant)
    dx_, dd, ga, be = _dev(env, x), _dev(env, dy), gamma.to(env.dev), beta.to(env.dev)
    results = {}
    for a in ((add, None) if variant == "randn" else (add,)):
        ref, scale = R.gn_bwd(x, dy, gamma, beta, 32, 1e-5, silu, a)
        floor = R.gn_bwd(x, dy, gamma, beta, 32, 1e-5, silu, a, emulate=True) - ref
        for chunked in (True, False):
            try:
                env.ops.GN_BWD_CHUNKED = chunked
                got = env.ops.group_norm_bwd(dx_, dd, ga, be, 32, 1e-5, silu, add=_dev(env, a))
                again = env.ops.group_norm_bwd(dx_, dd, ga, be, 32, 1e-5, silu, add=_dev(env, a))
            finally:
                env.ops.GN_BWD_CHUNKED = True
            name = (f"edge GroupNorm backward B{B} HW{HW} C{C} {variant}{' + add' if a is not None else ''} "
                    f"({'chunked' if chunked else 'one workgroup per group'})")
            S.check_sliced(name + " by (sample, group)", got, ref, floor, S.gn_group_slices(B, C, 32), abs_scale=scale)
            S.check_sliced(name + " by apply workgroup", got.reshape(B, -1), ref.reshape(B, -1), floor.reshape(B, -1),
                           S.flat_slices(B, HW * C, 8192), abs_scale=scale)
            assert torch.equal(got, again), "not deterministic"
            results[(a is not None, chunked)] = got
    if C > 4096:                                            # both settings take the one-workgroup-per-group kernel
        assert torch.equal(results[(True, True)], results[(True, False)])


# ------------------------------------------------------------------------------------------------ GEGLU, 2x2 sums
@pytest.mark.parametrize("rows", [1, 33])
def test_geglu_edges(env, rows):
    inner = 8
    ag, dy = K.geglu_inputs(rows, inner)
    (rf, rb), (ef, eb) = R.geglu(ag, dy), R.geglu(ag, dy, emulate=True)
    gf, gb = env.ops.geglu(_dev(env, ag)), env.ops.geglu_bwd(_dev(env, ag), _dev(env, dy))
    S.check_sliced(f"edge GEGLU forward {rows}x{inner}", gf, rf, ef - rf, S.row_col_slices(rows, inner, 1, 2048))
    S.check_sliced(f"edge GEGLU backward {rows}x{inner}", gb, rb, eb - rb, S.row_col_slices(rows, 2 * inner, 1, 2048))
    assert torch.equal(gf, env.ops.geglu(_dev(env, ag))) and torch.equal(gb, env.ops.geglu_bwd(_dev(env, ag), _dev(env, dy)))


@pytest.mark.parametrize("B,H,W,C", [(2, 3, 5, 8), (1, 2, 2, 8), (1, 5, 3, 40)])
def test_sum2x2_edges(env, B, H, W, C):
    d = K.pair_inputs(B * 4 * H * W, C, 8)[0].reshape(B, 2 * H, 2 * W, C)
    ref, scale = R.sum2x2(d)
    got = env.ops.sum2x2(_dev(env, d))
    rs = lambda t: t.reshape(B * H * W, C)
    S.check_sliced(f"edge 2x2 sums B{B} {H}x{W}x{C}", rs(got), rs(ref), rs(R.sum2x2(d, emulate=True) - ref),
                   S.row_col_slices(B * H * W, C, 32, 2048), abs_scale=scale)
    assert torch.equal(got, env.ops.sum2x2(_dev(env, d)))


# ------------------------------------------------------------------------------------------------ fp32 sums
def _wgrad_case(env, Rr, N, Kk):
    dy, x = K.pair_inputs(Rr, N, Kk)
    ref, asum = R.wgrad(dy, x)
    got = env.ops.weight_grad(_dev(env, dy), _dev(env, x))
    S.check_fp32_sum(f"edge dW {Rr}x{N}x{Kk}", got, ref, asum)
    assert torch.equal(got, env.ops.weight_grad(_dev(env, dy), _dev(env, x))), "not deterministic"
    return dy, x, ref, asum, got


@pytest.mark.parametrize("Rr", [1, 31, 32, 33, 64, 65])
def test_weight_gradient_small_edges(env, Rr):
    """row counts around the 32-row step and the 64-row split threshold; outputs narrower than, equal to and wider than a 128 tile"""
    for N in (8, 120, 128, 136):
        for Kk in (8, 120, 128, 136):
            _wgrad_case(env, Rr, N, Kk)
    assert env.lib.udt_wgrad_splits(65, 128, 128) == 2 and env.lib.udt_wgrad_splits(64, 128, 128) == 1


def test_weight_gradient_uses_fewer_ranges_than_it_sizes_partials_for(env):
    """R = 900, N = 640, K = 1280: udt_wgrad_splits says 11, ranges rounded up to 96 rows need 10: the 11th partial tile stays untouched"""
    Rr, N, Kk = 900, 640, 1280
    dy, x, ref, asum, got = _wgrad_case(env, Rr, N, Kk)
    Ssplit = env.lib.udt_wgrad_splits(Rr, N, Kk)
    assert Ssplit == 11
    rps = (math.ceil(Rr / Ssplit) + 31) // 32 * 32
    s_used = math.ceil(Rr / rps)
    assert (rps, s_used) == (96, 10)
    sentinel = 12345.5
    part = torch.full((Ssplit, N, Kk), sentinel, dtype=torch.float32, device=env.dev)
    dw = torch.empty((N, Kk), dtype=torch.float32, device=env.dev)
    dyb, xb = _dev(env, dy), _dev(env, x)
    env.L.check(env.lib.udt_wgrad_bf16(dyb.data_ptr(), xb.data_ptr(), dw.data_ptr(), part.data_ptr(), Rr, N, Kk, N, Kk,
                                       torch.cuda.current_stream().cuda_stream), "udt_wgrad_bf16")
    assert torch.equal(dw, got)
    assert bool((part[s_used:] == sentinel).all()), "partials beyond the ranges in use were written"
    assert not bool((part[:s_used] == sentinel).any())
    for r in range(s_used):                                 # each range's partial tile is that range's product
        pr, pa = R.wgrad(dy[r * rps:(r + 1) * rps], x[r * rps:(r + 1) * rps])
        S.check_fp32_sum(f"edge dW 900x640x1280 partial of range {r}", part[r], pr, pa)


def test_weight_gradient_last_range_of_one_row(env):
    assert env.lib.udt_wgrad_splits(2049, 128, 128) == 33       # ranges of 64 rows: the 33rd holds row 2048 alone
    _wgrad_case(env, 2049, 128, 128)


@pytest.mark.parametrize("rows", [1, 3, 63, 65, 16400])
def test_column_sum_edges(env, rows):
    for C in (2, 130, 648):
        x = K.pair_inputs(rows, C, 8)[0]
        ref, asum = R.colsum(x)
        got = env.ops.colsum(_dev(env, x))
        S.check_fp32_sum(f"edge column sums {rows}x{C}", got, ref, asum)
        assert torch.equal(got, env.ops.colsum(_dev(env, x))), "not deterministic"
    assert env.lib.udt_colparts(16400) == 1024 and env.lib.udt_colparts(16384) == 1024 and env.lib.udt_colparts(65) == 8


@pytest.mark.parametrize("P", [1, 17, 64, 67])
def test_reduce_rows_f32_edges(env, P):
    for n in (1, 33):
        for accumulate in (0, 1):
            g = K._gen(P, n, accumulate)
            src = torch.randn((P, n), generator=g)
            prev = torch.randn((n,), generator=g)
            out, src_d = prev.clone().to(env.dev), src.to(env.dev)
            env.L.check(env.lib.udt_reduce_rows_f32(src_d.data_ptr(), out.data_ptr(), P, n, accumulate,
                                                    torch.cuda.current_stream().cuda_stream), "udt_reduce_rows_f32")
            ref = src.double().sum(dim=0) + (prev.double() if accumulate else 0)
            asum = src.double().abs().sum(dim=0) + (prev.double().abs() if accumulate else 0)
            S.check_fp32_sum(f"edge fp32 row reduction P{P} n{n} accumulate{accumulate}", out, ref, asum)


# ------------------------------------------------------------------------------------------------ AdamW, loss seeds
@pytest.mark.parametrize("step", [1, 100000])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_adamw_edges(env, n, step):
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))          # the C ABI takes floats
    for case, (wd, gs, zero) in {"default": (1e-2, 1.0, False), "g = 0, v = 0": (1e-2, 1.0, True), "grad_scale": (1e-2, 0.125 / 3, False),
                                 "no decay": (0.0, 1.0, False)}.items():
        g = K._gen(n, step)
        p0, gr = torch.randn((n,), generator=g), torch.randn((n,), generator=g)
        m0, v0 = 0.1 * torch.randn((n,), generator=g), 0.01 * torch.rand((n,), generator=g)
        if zero:
            gr, m0, v0 = torch.zeros(n), 0.1 * torch.randn((n,), generator=g), torch.zeros(n)
        lr, betas, eps = 8e-4, (0.9, 0.999), 1e-8
        p, m, v = p0.clone().to(env.dev), m0.clone().to(env.dev), v0.clone().to(env.dev)
        env.ops.adamw_(p, gr.to(env.dev), m, v, step, lr, betas, eps, wd, gs)
        rp, rm, rv = R.adamw(p0, gr, m0, v0, step, f32(lr), (f32(betas[0]), f32(betas[1])), f32(eps), f32(wd), f32(gs))
        # (p - update cancels: the existing test's atol; m and v are sums of like-signed or dominant terms)
        for nm, got, ref, atol in (("p", p, rp, 1e-7), ("m", m, rm, 1e-12), ("v", v, rv, 1e-12)):
            assert torch.allclose(got.double().cpu(), ref, rtol=1e-5, atol=atol), f"AdamW {nm}, n {n}, step {step}, {case}"


@pytest.mark.parametrize("sigma", [0.002, 80.0])
def test_loss_seed_edges(env, sigma):
    B, h, w = 1, 3, 3
    f, noised, target = K.seed_inputs(B, h, w)
    sg = torch.tensor([sigma])
    wide = torch.zeros((B, h, w, 8))
    wide[..., :4] = f
    wide[..., 4:] = 7.0                                     # (channels past the fourth are not read)
    dev = lambda t: t.to(env.dev).contiguous()
    coefs = {"eps-prediction": (torch.ones(1), -sg, sg ** -2.0),
             "preconditioned": (1 / (sg ** 2 + 1), sg / (sg ** 2 + 1).sqrt(), 1 + sg ** -2.0)}
    for nm, coef in coefs.items():
        if nm == "eps-prediction":
            run = lambda: env.ops.diff_loss_grad(dev(wide), dev(noised), dev(target), dev(sg), cpad=8)
        else:
            run = lambda: env.ops.precond_loss_grad(dev(wide), dev(noised), dev(target), *(dev(c) for c in coef), cpad=8)
        loss, seed = run()
        rl, rs_, scale = R.precond_loss_grad(f, noised, target, *coef)
        _, emul = R.precond_loss_grad(f, noised, target, *coef, emulate=True)
        assert torch.allclose(loss.double().cpu(), rl, rtol=1e-5), f"{nm} loss at sigma {sigma}"
        S.check_sliced(f"edge {nm} loss seed B1 hw9 sigma {sigma}", seed[..., :4], rs_, emul - rs_, iter([(slice(None),)]),
                       abs_scale=scale)
        assert not bool(seed[..., 4:].any())
        loss2, seed2 = run()
        assert torch.equal(loss, loss2) and torch.equal(seed, seed2)
