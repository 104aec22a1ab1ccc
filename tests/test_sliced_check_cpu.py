"""tests/sliced_check.py proves itself on the CPU (``-m "not gpu"``).

1. For every family of csrc/backward.hip — one benign case and every hostile case of tests/test_backward_edges_gpu.py — a float32 CPU
   evaluation of the closed form, rounded where the kernel rounds, passes the check: the bounds are attainable in fp32 arithmetic.
2. Planted defects a .. g (one zeroed query row, one dropped key tile, two swapped heads, a 1 % gain on one GroupNorm group, a lost
   last row, padded keys scored 0, a shifted ragged tail) pass the old global ``rel_rms <= tol`` assertion — the hole — and fail
   check_sliced / check_fp32_sum.
"""
import pytest
import torch

import backward_cases as K
import backward_ref as R
import sliced_check as S

F32 = torch.float32
TOL_OP, TOL_ATTN = 1.5e-2, 2e-2                 # the global bounds of tests/test_backward_gpu.py, tests/test_training_gpu.py
SCALE = 64 ** -0.5


def _rel(got, ref):                             # (as _rel of the GPU test files)
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300)).item()


@pytest.fixture(autouse=True)
def _report_to_tmp(tmp_path, monkeypatch):
    monkeypatch.setattr(S, "REPORT", str(tmp_path / "parity_report.txt"))


def _fails(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ------------------------------------------------------------------------------------------------ 1. fp32 passes
@pytest.mark.parametrize("B,H,N,variant", [(1, 2, 129, "randn")] + [(1, 2, 129, v) for v in K.ATTN_VARIANTS]
                         + [(9, 20, 300, v) for v in K.ATTN_VARIANTS])
def test_float32_attention_backward_passes(B, H, N, variant):
    qkv, d_o = K.attn_inputs(B, H, N, variant)
    ref, floor, scales = R.attn_ref_emul(qkv, d_o, H, SCALE)
    got = R.attn_bwd(qkv, d_o, H, SCALE, dtype=F32, emulate=True)
    C = H * 64
    for i, nm in enumerate(("dq", "dk", "dv")):
        c = slice(i * C, (i + 1) * C)
        S.check_sliced(f"fp32 attention backward {nm} B{B} H{H} N{N} {variant}", got[..., c], ref[..., c], floor[..., c],
                       S.attn_slices(B, H, N), abs_scale=scales[nm])


@pytest.mark.parametrize("L", [1, 13, 16])
@pytest.mark.parametrize("use_dp,use_do", [(True, False), (False, True), (True, True)])
def test_float32_text_cross_attention_backward_passes(L, use_dp, use_do):
    B, H, N = 1, 2, 257
    q, kv, d_o, d_p = K.xattn_inputs(B, H, N, L)
    args = (q, kv, d_p if use_dp else None, d_o if use_do else None, H, SCALE)
    ref = R.xattn_bwd(*args)
    emul = R.xattn_bwd(*args, emulate=True)
    got = R.xattn_bwd(*args, dtype=F32, emulate=True)
    for nm, n in (("dq", N), ("dk", L), ("dv", L)):
        S.check_sliced(f"fp32 text cross-attention {nm} L{L}", got[nm], ref[nm], emul[nm] - ref[nm], S.attn_slices(B, H, n),
                       abs_scale=ref["abs"][nm])


@pytest.mark.parametrize("variant", ("randn",) + K.LN_VARIANTS)
@pytest.mark.parametrize("with_add", [False, True])
def test_float32_layernorm_backward_and_parameter_gradients_pass(variant, with_add):
    rows, C = 303, 1544
    x, dy, add, gamma = K.ln_inputs(rows, C, variant)
    a = add if with_add else None
    ref, scale = R.ln_bwd(x, dy, gamma, 1e-5, a)
    S.check_sliced(f"fp32 LayerNorm backward {variant}", R.ln_bwd(x, dy, gamma, 1e-5, a, dtype=F32, emulate=True), ref,
                   R.ln_bwd(x, dy, gamma, 1e-5, a, emulate=True) - ref, S.row_col_slices(rows, C, 4, 512), abs_scale=scale)
    dg, db, ag, ab = R.ln_param_grad(x, dy, 1e-5)
    dg32, db32, _, _ = R.ln_param_grad(x, dy, 1e-5, dtype=F32)
    S.check_fp32_sum(f"fp32 LayerNorm d gamma {variant}", dg32, dg, ag)
    S.check_fp32_sum(f"fp32 LayerNorm d beta {variant}", db32, db, ab)


@pytest.mark.parametrize("variant", ("randn",) + K.GN_VARIANTS)
@pytest.mark.parametrize("B,HW,C", [(2, 129, 64), (1, 33, 320)])
def test_float32_groupnorm_backward_passes(variant, B, HW, C):
    x, dy, add, gamma, beta, silu = K.gn_inputs(B, HW, C, variant)
    ref, scale = R.gn_bwd(x, dy, gamma, beta, 32, 1e-5, silu, add)
    floor = R.gn_bwd(x, dy, gamma, beta, 32, 1e-5, silu, add, emulate=True) - ref
    got = R.gn_bwd(x, dy, gamma, beta, 32, 1e-5, silu, add, dtype=F32, emulate=True)
    S.check_sliced(f"fp32 GroupNorm backward {variant} (sample, group)", got, ref, floor, S.gn_group_slices(B, C, 32), abs_scale=scale)
    S.check_sliced(f"fp32 GroupNorm backward {variant} (sample, apply workgroup)", got.reshape(B, -1), ref.reshape(B, -1),
                   floor.reshape(B, -1), S.flat_slices(B, HW * C, 8192), abs_scale=scale)


@pytest.mark.parametrize("rows,inner", [(33, 8), (64, 128)])
def test_float32_geglu_and_2x2_sums_pass(rows, inner):
    ag, dy = K.geglu_inputs(rows, inner)
    (rf, rb), (ef, eb), (gf, gb) = R.geglu(ag, dy), R.geglu(ag, dy, emulate=True), R.geglu(ag, dy, dtype=F32, emulate=True)
    S.check_sliced("fp32 GEGLU forward", gf, rf, ef - rf, S.row_col_slices(rows, inner, 1, 2048))
    S.check_sliced("fp32 GEGLU backward", gb, rb, eb - rb, S.row_col_slices(rows, 2 * inner, 1, 2048))
    d = K.pair_inputs(6 * 10, 8 * inner, 8)[0].reshape(1, 6, 10, 8 * inner)      # H = 3, W = 5
    ref, scale = R.sum2x2(d)
    S.check_sliced("fp32 2x2 sums", R.sum2x2(d, dtype=F32, emulate=True).reshape(15, -1), ref.reshape(15, -1),
                   (R.sum2x2(d, emulate=True) - ref).reshape(15, -1), S.row_col_slices(15, 8 * inner, 1, 2048), abs_scale=scale)


@pytest.mark.parametrize("R_,N,K_", [(65, 136, 120), (900, 640, 1280), (16400, 8, 130)])
def test_float32_weight_gradient_and_column_sums_pass(R_, N, K_):
    dy, x = K.pair_inputs(R_, N, K_)
    ref, asum = R.wgrad(dy, x)
    S.check_fp32_sum(f"fp32 dW {R_}x{N}x{K_}", R.wgrad(dy, x, dtype=F32)[0], ref, asum)
    ref, asum = R.colsum(x)
    S.check_fp32_sum(f"fp32 column sums {R_}x{K_}", R.colsum(x, dtype=F32)[0], ref, asum)


@pytest.mark.parametrize("sigma", [0.002, 80.0])
def test_float32_loss_seeds_pass(sigma):
    f, noised, target = K.seed_inputs(1, 3, 3)
    sg = torch.tensor([sigma])
    for nm, coef in (("eps-prediction", (torch.ones(1), -sg, sg ** -2.0)), ("preconditioned", (1 / (sg ** 2 + 1), sg / (sg ** 2 + 1).sqrt(),
                                                                                              1 + sg ** -2.0))):
        _, ref, scale = R.precond_loss_grad(f, noised, target, *coef)
        _, emul = R.precond_loss_grad(f, noised, target, *coef, emulate=True)
        _, got = R.precond_loss_grad(f, noised, target, *coef, dtype=F32, emulate=True)
        S.check_sliced(f"fp32 {nm} loss seed sigma {sigma}", got, ref, emul - ref, iter([(slice(None),)]), abs_scale=scale)


# ------------------------------------------------------------------------------------------------ 2. planted defects
def test_helper_counts_coverage_and_demands_exact_zeros():
    ref = torch.randn((64, 64), dtype=torch.float64)
    emul = R.bf(ref)
    S.check_sliced("cover", emul, ref, emul - ref, S.row_col_slices(64, 64, 32, 64))
    _fails(S.check_sliced, "a slice is missing", emul, ref, emul - ref, list(S.row_col_slices(64, 64, 32, 64))[:1])
    _fails(S.check_sliced, "a slice counted twice", emul, ref, emul - ref, list(S.row_col_slices(64, 64, 32, 64)) * 2)
    ref[:32] = 0
    emul = R.bf(ref)
    S.check_sliced("zero slice", emul, ref, emul - ref, S.row_col_slices(64, 64, 32, 64))
    emul[3, 5] = 1e-30
    _fails(S.check_sliced, "zero slice polluted", emul, ref, emul - ref, S.row_col_slices(64, 64, 32, 64))


@pytest.fixture(scope="module")
def big_dq():
    """dq of the suite's B5 H5 N4096 case: (ref64, the emulation before its output rounding, what owner tile 1 of head (0, 0) gets
    from key tile 2).  Head 1 of sample 0 is head 0 plus 1 %: two swapped heads are wrong by as much as the heads differ, and on
    independent heads (100 % error on 2 / 25 of the tensor) the old global assertion fails too — the hole is heads that are close."""
    B = H = 5
    N = 4096
    qkv, d_o = K.attn_inputs(B, H, N)
    C = H * 64
    for i in range(3):
        qkv[0, :, i * C + 64:i * C + 128] = K._bf(qkv[0, :, i * C:i * C + 64] * (1 + 0.01 * torch.randn((N, 64), generator=K._gen(i))))
    d_o[0, :, 64:128] = K._bf(d_o[0, :, :64] * (1 + 0.01 * torch.randn((N, 64), generator=K._gen(7))))
    ref = torch.empty((B, N, C), dtype=torch.float64)
    emul = torch.empty((B, N, C), dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            c = slice(h * 64, (h + 1) * 64)
            q, k, v, g = (t.double() for t in (qkv[b, :, :C][:, c], qkv[b, :, C:2 * C][:, c], qkv[b, :, 2 * C:][:, c], d_o[b][:, c]))
            p = torch.softmax(q @ k.t() * SCALE, dim=-1)
            o = p @ v
            dp = g @ v.t()
            ref[b, :, c] = (p * (dp - (g * o).sum(dim=-1, keepdim=True))) @ k * SCALE
            ds = R.bf(p * (dp - (g * R.bf(o)).sum(dim=-1, keepdim=True)))
            emul[b, :, c] = ds @ k * SCALE
            if b == 0 and h == 0:
                dropped = ds[128:256, 64:96] @ k[64:96] * SCALE       # what owner tile 1 gets from key tile 2
    return ref, emul, dropped


def _both(name, bad, ref, floor, slices, tol, **kw):
    old = _rel(bad, ref)
    assert old <= tol, f"{name}: the old global assertion was expected to pass (rel_rms {old:.3e} > {tol})"
    _fails(S.check_sliced, name, bad, ref, floor, slices, **kw)


def test_defects_a_b_c_in_a_5x5x4096_dq(big_dq):
    ref, emul_pre, dropped = big_dq
    emul = R.bf(emul_pre)
    floor = emul - ref
    sl = lambda: S.attn_slices(5, 5, 4096)
    S.check_sliced("5x5x4096 dq, no defect", emul, ref, floor, sl())
    bad = emul.clone()
    bad[3, 1234, 128:192] = 0                                                     # a. one query row zeroed (1 row in 102400)
    _both("a. one query row zeroed", bad, ref, floor, sl(), TOL_ATTN)
    bad = emul_pre.clone()
    bad[0, 128:256, :64] -= dropped                                               # b. one 32-key tile lost for one 128-query owner tile
    _both("b. one streamed key tile dropped", R.bf(bad), ref, floor, sl(), TOL_ATTN)
    bad = emul.clone()
    bad[0, :, :64], bad[0, :, 64:128] = emul[0, :, 64:128], emul[0, :, :64]       # c. two (nearly equal) heads swapped in sample 0
    _both("c. two heads swapped", bad, ref, floor, sl(), TOL_ATTN)


def test_defect_d_one_percent_gain_on_one_groupnorm_group():
    B, HW, C = 2, 256, 320
    x, dy, add, gamma, beta, silu = K.gn_inputs(B, HW, C)
    ref, scale = R.gn_bwd(x, dy, gamma, beta, 32, 1e-5, silu)
    emul = ref.clone()
    emul[1, :, 70:80] *= 1.01                                                     # (sample 1, group 7)
    emul = R.bf(emul)
    floor = R.bf(ref) - ref
    _both("d. 1 % gain on one (sample, group)", emul, ref, floor, S.gn_group_slices(B, C, 32), TOL_OP, abs_scale=scale)


def test_defect_e_last_row_left_out_of_a_column_sum_and_a_dw():
    dy, x = K.pair_inputs(16400, 64, 128)
    for nm, fn, args in (("dW", R.wgrad, (dy, x)), ("column sums", R.colsum, (x,))):
        ref, asum = fn(*args)
        good = fn(*args, dtype=F32)[0]
        S.check_fp32_sum(f"{nm}, no defect", good, ref, asum)
        bad = fn(*args, dtype=F32, last_row=False)[0]
        old = _rel(bad, ref)
        assert old <= TOL_OP, f"e. {nm}: the old global assertion was expected to pass ({old:.3e})"
        _fails(S.check_fp32_sum, f"e. last row left out of {nm}", bad, ref, asum)


def test_defect_f_padded_keys_scored_zero():
    """Padded keys that take part in the softmax with score 0 cost each query 1 / sum_j exp(s_j) of its probability mass.  On randn
    inputs at N = 1023 (one padded key) that is 6e-4: the old assertion passes, and so does the sliced one — randn cannot see the defect
    at all.  With every real score at -30 the padded key dominates: the sliced check fails (and there the global one does too: the
    whole gradient is gone — on those inputs the hole is that no test ran them)."""
    B, H, N = 1, 1, 1023
    qkv, d_o = K.attn_inputs(B, H, N)
    ref, floor, scales = R.attn_ref_emul(qkv, d_o, H, SCALE)
    bad = R.attn_bwd(qkv, d_o, H, SCALE, emulate=True, pad_score0=1)
    for i, nm in enumerate(("dq", "dk", "dv")):
        c = slice(i * 64, (i + 1) * 64)
        assert _rel(bad[..., c], ref[..., c]) <= TOL_ATTN
    B, H, N = 1, 2, 129
    qkv, d_o = K.attn_inputs(B, H, N, "neg")
    ref, floor, scales = R.attn_ref_emul(qkv, d_o, H, SCALE)
    bad = R.attn_bwd(qkv, d_o, H, SCALE, emulate=True, pad_score0=31)
    C = H * 64
    for i, nm in enumerate(("dq", "dk", "dv")):
        c = slice(i * C, (i + 1) * C)
        _fails(S.check_sliced, f"f. padded keys scored 0: {nm}", bad[..., c], ref[..., c], floor[..., c], S.attn_slices(B, H, N),
               abs_scale=scales[nm])


def test_defect_g_tail_rows_of_a_ragged_tile_shifted_by_one():
    B, H, N, L = 2, 10, 4100, 12                                                  # the query-side kernel's last workgroup holds 4 rows
    q, kv, d_o, d_p = K.xattn_inputs(B, H, N, L)
    ref = R.xattn_bwd(q, kv, d_p, d_o, H, SCALE)
    emul = R.xattn_bwd(q, kv, d_p, d_o, H, SCALE, emulate=True)["dq"]
    floor = emul - ref["dq"]
    bad = emul.clone()
    bad[1, 4096:4100, 192:256] = emul[1, 4095:4099, 192:256]
    _both("g. ragged tail shifted by one row", bad, ref["dq"], floor, S.attn_slices(B, H, N), TOL_OP, abs_scale=ref["abs"]["dq"])
