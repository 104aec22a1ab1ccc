"""The references, case lists and checks of the forward GEMM / convolution edge cases, without a GPU: tests/gemm_ref.py pinned against
independent torch compositions (F.conv2d, F.layer_norm, F.gelu in float64), every case of tests/gemm_cases.py evaluated in float32 on the
CPU and passed through the SAME checks tests/test_gemm_edges_gpu.py applies to the kernels (the bounds admit a correct fp32
implementation; no case needs the kernel to pass), planted defects that must fail in the slice that holds them, and the coverage of the
launchers by the lists through the planner mirrors at 256 CUs.
"""
import math
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

import udifftext_amd  # noqa: F401
from udifftext_amd import packing

import gemm_cases as K
import gemm_ref as R
import sliced_check as S

REPORT = os.path.join(tempfile.gettempdir(), "gemm_ref_cpu_report.txt")
CUS = 256
D = torch.float64


def _rn(*s, seed=0):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(*s, generator=g, dtype=D)


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _w_oihw(w, C, k):
    return w.reshape(w.shape[0], k, k, C).permute(0, 3, 1, 2)          # packed tap-major [N, (ky, kx, c)] -> [N, C, ky, kx]


# ------------------------------------------------------------------------------------------------ the references, pinned
@pytest.mark.parametrize("H,W,stride,pad,out_hw", [(9, 9, 1, (1, 1), None), (9, 9, 2, (1, 1), None), (10, 6, 2, (0, 0), (5, 3)),
                                                  (12, 20, 1, (1, 1), None), (8, 8, 2, (1, 0), (4, 4))])
def test_conv_acc_is_conv2d(H, W, stride, pad, out_hw):
    x, w = _rn(2, H, W, 8, seed=1), _rn(5, 72, seed=2)
    acc, aabs = R.conv_acc(x, w, stride=stride, pad_t=pad[0], pad_l=pad[1], out_hw=out_hw)
    Ho, Wo = acc.shape[1:3]
    need_h, need_w = (Ho - 1) * stride + 3, (Wo - 1) * stride + 3
    xp = F.pad(_nchw(x), (pad[1], max(need_w - W - pad[1], 0), pad[0], max(need_h - H - pad[0], 0)))
    ref = F.conv2d(xp, _w_oihw(w, 8, 3), stride=stride)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)
    assert torch.allclose(acc, ref, rtol=0, atol=1e-12)
    ref_abs = F.conv2d(xp.abs(), _w_oihw(w, 8, 3).abs(), stride=stride)[:, :, :Ho, :Wo].permute(0, 2, 3, 1)
    assert torch.allclose(aabs, ref_abs, rtol=0, atol=1e-12)


def test_conv_acc_upsample_two_sources_and_1x1():
    x, x2, w = _rn(2, 4, 6, 8, seed=3), _rn(2, 4, 6, 4, seed=4), _rn(5, 9 * 12, seed=5)
    cat = torch.cat([x, x2], dim=-1)
    acc, _ = R.conv_acc(x, w, x2=x2)
    assert torch.allclose(acc, F.conv2d(_nchw(cat), _w_oihw(w, 12, 3), padding=1).permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    acc, _ = R.conv_acc(x, w[:, :72], upsample=True)
    up = F.interpolate(_nchw(x), scale_factor=2, mode="nearest")
    assert torch.allclose(acc, F.conv2d(up, _w_oihw(w[:, :72], 8, 3), padding=1).permute(0, 2, 3, 1), rtol=0, atol=1e-12)
    acc, _ = R.conv_acc(x, w[:, :12], ksize=1, pad_t=0, pad_l=0, x2=x2)
    assert torch.allclose(acc, cat @ w[:, :12].t(), rtol=0, atol=1e-12)


def test_conv_up4_acc_is_the_upsampled_convolution():
    """on weights whose phase sums are exact in bf16 (small integers) the packed phase form IS the nine-tap upsampled convolution"""
    g = torch.Generator()
    g.manual_seed(6)
    w = torch.randint(-2, 3, (8, 64, 3, 3), generator=g).float()
    x = _rn(2, 5, 7, 64, seed=7)
    up4 = packing.pack_conv_up4(w, n_pad_to=4)
    assert up4.shape == (4, 8, 256)
    acc, _ = R.conv_up4_acc(x, up4.float())
    ref = F.conv2d(F.interpolate(_nchw(x), scale_factor=2, mode="nearest"), w.double(), padding=1).permute(0, 2, 3, 1)
    assert torch.allclose(acc, ref, rtol=0, atol=1e-11)


def test_gn_on_patch_is_group_norm_through_its_table():
    B, H, W, C, groups, eps = 2, 4, 5, 128, 32, 1e-5
    x, gamma, beta = _rn(B, H, W, C, seed=8), _rn(C, seed=9), _rn(C, seed=10)
    xg = _nchw(x).reshape(B, groups, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    rstd = (var + eps).rsqrt()
    scale = gamma.reshape(1, C) * rstd.repeat_interleave(C // groups, dim=1)
    shift = beta.reshape(1, C) - mean.repeat_interleave(C // groups, dim=1) * scale
    scsh = torch.stack([scale.reshape(B, C // 64, 64), shift.reshape(B, C // 64, 64)], dim=2)
    for act in (0, 1):
        y = R.gn_on_patch(x, scsh, act, emulate=False)
        ref = F.group_norm(_nchw(x), groups, gamma, beta, eps)
        ref = F.silu(ref) if act else ref
        assert torch.allclose(y, ref.permute(0, 2, 3, 1), rtol=0, atol=1e-11)


def test_epilogue_order_geglu_transposed_and_layernorm_fold():
    a, w, bias, res, rv = _rn(10, 64, seed=11), _rn(128, 64, seed=12), _rn(128, seed=13), _rn(10, 128, seed=14), _rn(3, 128, seed=15)
    ref, emul, ab = R.gemm_ref(a, w, alpha=0.5, bias=bias, rowvec=rv, rows_per_batch=4, residual=res, act="silu")
    pre = (a @ w.t()) * 0.5 + bias + rv[torch.arange(10) // 4] + res
    assert torch.allclose(ref, F.silu(pre), rtol=0, atol=1e-12)
    assert torch.equal(emul, F.silu(pre).float().bfloat16().double())
    assert torch.allclose(ab, (a.abs() @ w.abs().t()) * 0.5 + bias.abs() + rv[torch.arange(10) // 4].abs() + res.abs(), rtol=0, atol=1e-12)
    assert torch.equal(R.gemm_ref(a, w, act="relu")[0], (a @ w.t()).clamp_min(0))
    assert torch.equal(R.gemm_ref(a, w, out_f32=True)[1], a @ w.t())
    # GEGLU on packed [32 value | 32 gate] blocks
    out = R.gemm_ref(a, w, bias=bias, geglu=True)[0]
    full = (a @ w.t() + bias).reshape(10, 2, 2, 32)
    assert torch.allclose(out, (full[:, :, 0] * F.gelu(full[:, :, 1])).reshape(10, 64), rtol=0, atol=1e-12)
    # transposed: the same values as [batch][N][rows]
    t = R.gemm_ref(a[:8], w, bias=bias, transposed=True, rows_per_batch=4)[0]
    assert torch.equal(t, (a[:8] @ w.t() + bias).reshape(2, 4, 128).transpose(1, 2))
    # LayerNorm folded: W' = W gamma, c = W beta + b, s = row sums of W'
    gamma, beta = _rn(64, seed=16), _rn(64, seed=17)
    wf = w * gamma
    c, s = w @ beta + bias, wf.sum(dim=1)
    ref = R.ln_gemm_ref(a, wf, c, s, eps=1e-5)[0]
    assert torch.allclose(ref, F.layer_norm(a, (64,), gamma, beta, 1e-5) @ w.t() + bias, rtol=0, atol=1e-10)
    ref = R.ln_gemm_ref(a, wf, c, s, eps=1e-5, geglu=True)[0]
    full = (F.layer_norm(a, (64,), gamma, beta, 1e-5) @ w.t() + bias).reshape(10, 2, 2, 32)
    assert torch.allclose(ref, (full[:, :, 0] * F.gelu(full[:, :, 1])).reshape(10, 64), rtol=0, atol=1e-10)


def test_erf_approximations_measured_against_math_erf():
    """the coefficients are data in csrc/common.h; their worst error is measured here in float64, not guessed (the report's header quotes
    it).  Abramowitz-Stegun 7.1.26 states 1.5e-7, the erfc polynomial's comment 2.9e-7."""
    e_as, e_poly = R.measured_erf_error()
    assert 5e-8 < e_as < 1.6e-7 and 5e-8 < e_poly < 3.2e-7, (e_as, e_poly)
    assert R.erf_error() == max(e_as, e_poly)
    assert abs(R.erf_as(0.3) - math.erf(0.3)) < 2e-7 and abs(R.erf_as(-1.7) - math.erf(-1.7)) < 2e-7


def test_colstats_ref_and_slot_orders():
    v = _rn(12, 8, seed=18)
    ref, ab = R.colstats_ref(v, torch.arange(12) // 4, 4)
    assert torch.allclose(ref[1, :, 0], v[4:8].sum(0)) and torch.allclose(ref[2, :, 1], (v[8:] ** 2).sum(0)) and bool((ref[3] == 0).all())
    assert torch.allclose(ab[0, :, 0], v[:4].abs().sum(0))
    # the phase form's order: [image][phase][tile of the image][wave pixel block]
    c = K.C(2, 8, 16, 64, 128, ups=2, stats=True)
    p = K.predict(c, CUS)
    slot, slots = K.stats_slot_of_row(c, p)
    assert p.stats[:2] == (64, 2 * 4 * 1 * 2) and slots == 16 and int(slot.max()) == 15
    m = slot.reshape(2, 16, 32)
    assert int(m[0, 0, 0]) == 0 and int(m[0, 0, 1]) == 2 and int(m[0, 1, 0]) == 4 and int(m[0, 8, 0]) == 1 and int(m[1, 0, 0]) == 8
    assert all(int((slot == s).sum()) == 64 for s in range(16))
    # conv3p, four images of 8 x 8 per tile with a ragged last group
    c = K.C(5, 8, 8, 64, 128, gn=0, stats=True)
    p = K.predict(c, CUS)
    slot, slots = K.stats_slot_of_row(c, p)
    assert slots == 8 and slot.reshape(5, 64)[:, 0].tolist() == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------------------------------------ the float32 evaluation of every case
ALL = K.all_cases()


@pytest.mark.parametrize("i", range(0, len(ALL), 8))
def test_float32_evaluation_passes_the_gpu_checks(i):
    for name, c, variant in ALL[i:i + 8]:
        p = K.predict(c, CUS)
        t = K.inputs(c, variant)
        exp = K.reference(c, t)
        got = K.eval32(c, t)
        K.hold("cpu32 " + name, c, p, got, exp, t, report=REPORT)
        if p.stats:
            # the statistics' contract: sums of the stored output, in fp32
            rows, slots, _ = p.stats
            slot, _ = K.stats_slot_of_row(c, p)
            ref, ab = R.colstats_ref(got.reshape(p.d.M, -1), slot, slots)
            with R.restated_in(torch.float32):
                got_st = R.colstats_ref(got.reshape(p.d.M, -1), slot, slots)[0]
            S.check_fp32_sum("cpu32 stats " + name, got_st, ref, ab, report=REPORT)


# ------------------------------------------------------------------------------------------------ planted defects
def _fails_in(name, c, variant, hook, region, max_slices):
    """the defective float32 evaluation fails, the first failing slice lies inside ``region`` (index ranges per dimension), and at most
    ``max_slices`` slices fail (a slice can be reported twice: rms and max; a short unit is merged with its successor and named by itself)"""
    p = K.predict(c, CUS)
    t = K.inputs(c, variant)
    exp = K.reference(c, t)
    K.hold("sound " + name, c, p, K.eval32(c, t), exp, t, report=REPORT)
    got = K.eval32(c, t, acc_hook=lambda acc: hook(acc, t, p))
    with pytest.raises(AssertionError) as e:
        K.hold("defect " + name, c, p, got, exp, t, report=REPORT)
    n_fail, n_all, idxs = K.failed_slices(str(e.value))
    assert 1 <= n_fail <= 2 * max_slices and max_slices < n_all, str(e.value)
    for (a, b), (lo, hi) in zip(idxs[0], region):
        a, b = (0 if a is None else a), (10 ** 9 if b is None else b)
        assert lo <= a and b <= hi, (idxs[0], region, str(e.value))


def test_defect_last_ktile_of_a_splitk_slice_dropped_in_one_tile():
    c = K.G(257, 192, 576, knobs={"lean_splitk": 2}, res=True)           # slices of 5 and 4 K-tiles; tile (1, 0): rows 128:256, columns 0:128

    def hook(acc, t, p):
        assert (p.plan.splitk, p.plan.kt_per) == (2, 5)
        acc = acc.clone()
        ks = slice(4 * 64, 5 * 64)
        acc[128:256, 0:128] -= t["a"][128:256, ks] @ t["w"][0:128, ks].t()
        return acc
    _fails_in("split-K K-tile", c, "randn", hook, [(128, 256), (0, 128)], 4)


def test_defect_rowvec_once_per_tile():
    c = K.G(257, 200, 192, rowvec=24, res=True)

    def hook(acc, t, p):
        acc = acc.clone()
        rows = torch.arange(128, 256)
        acc[128:256, 128:200] += t["rowvec"][128 // 24, 128:200] - t["rowvec"][rows // 24][:, 128:200]
        return acc
    _fails_in("rowvec per tile", c, "randn", hook, [(128, 256), (128, 200)], 4)


def test_defect_bias_of_the_n_tail_tile_from_the_previous_tile():
    c = K.G(257, 200, 64)

    def hook(acc, t, p):
        acc = acc.clone()
        acc[:, 128:200] += t["bias"][0:72] - t["bias"][128:200]
        return acc
    _fails_in("N-tail bias", c, "randn", hook, [(0, 257), (128, 200)], 10)


def test_defect_two_sources_split_one_ktile_off_the_boundary():
    c = K.C(2, 9, 8, 384, 136, ksize=1, C2=192, knobs={"lean_splitk": 2}, rowvec=True)

    def hook(acc, t, p):
        # in tile (0, 0) the last K-tile of source 1 is read from source 2's first 64 channels
        acc = acc.clone().reshape(p.d.M, -1)
        x1, x2 = t["x"].reshape(-1, 384), t["x2"].reshape(-1, 192)
        wk = t["w"][0:128, 320:384]
        acc[0:128, 0:128] += (x2[0:128, 0:64] - x1[0:128, 320:384]) @ wk.t()
        return acc.reshape(2, 9, 8, -1)
    p = K.predict(c, CUS)
    assert p.family == "lean1" and p.tile[0] == "rows"
    with pytest.raises(AssertionError) as e:
        t = K.inputs(c)
        K.hold("defect two sources", c, p, K.eval32(c, t, acc_hook=lambda acc: hook(acc, t, p)), K.reference(c, t), t, report=REPORT)
    n_fail, n_all, idxs = K.failed_slices(str(e.value).split(" ring")[0])
    assert n_fail <= 8 and 4 < n_all and idxs[0][0][1] <= 128 and idxs[0][1][1] <= 128, str(e.value)


def test_defect_tap_wrapped_across_the_right_edge_on_border_only():
    c = K.C(3, 8, 16, 64, 136)                                            # 16 x 8 tiles: one tile per image; N tiles 0:128, 128:136

    def hook(acc, t, p):
        # image 1, channels 0:128: tap (1, 2) of the pixels in the last column reads (y + 1, 0) instead of the zero padding
        acc = acc.clone()
        wt = t["w"][0:128, 5 * 64:6 * 64]
        acc[1, 0:7, 15, 0:128] += t["x"][1, 1:8, 0] @ wt.t()
        return acc
    _fails_in("wrapped tap", c, "border_only", hook, [(1, 2), (0, 8), (0, 16), (0, 128)], 1)


def test_defect_halo_row_from_the_next_image_on_image_steps():
    c = K.C(3, 8, 8, 64, 128)

    def hook(acc, t, p):
        # image 0: the taps of the row below the image read image 1's first row
        acc = acc.clone()
        xp = F.pad(t["x"][1, 0], (0, 0, 1, 1))                            # [W + 2, C]
        for kx in range(3):
            acc[0, 7] += xp[kx:kx + 8] @ t["w"][:, (6 + kx) * 64:(7 + kx) * 64].t()
        return acc
    _fails_in("halo from next image", c, "image_steps", hook, [(0, 1), (0, 8), (0, 8), (0, 128)], 1)


def test_defect_one_phase_with_another_phases_weights():
    c = K.C(3, 8, 16, 64, 128, ups=2)

    def hook(acc, t, p):
        # image 2: phase (1, 0) computed with phase (0, 1)'s weights
        w = t["w"].clone()
        w[2] = t["w"][1]
        bad, _ = R.conv_up4_acc(t["x"][2:3], w)
        acc = acc.clone()
        acc[2, 1::2, 0::2] = bad[0, 1::2, 0::2]
        return acc
    _fails_in("phase weights", c, "randn", hook, [(2, 3), (0, 16), (0, 32), (0, 128)], 1)


def test_defect_padding_pixel_given_the_groupnorm_shift():
    c = K.C(3, 8, 8, 64, 128, gn=1)

    def hook(acc, t, p):
        # image 1 (of the four in the tile): the padding above-left of pixel (0, 0) holds act(shift) instead of zero
        sh = t["scsh"][1, :, 1].reshape(-1)
        acc = acc.clone()
        acc[1, 0, 0] += (F.silu(sh) @ t["w"][:, 0:64].t()).to(acc.dtype)
        return acc
    # (the tile holds images 0..3: the slice is the tile's; the ring check names the image)
    _fails_in("padding shift", c, "randn", hook, [(1, 2), (0, 8), (0, 8), (0, 128)], 1)


# ------------------------------------------------------------------------------------------------ coverage of the launchers
def test_the_lists_cover_the_launchers():
    P = [(n, c, K.predict(c, CUS)) for n, c, _ in ALL]
    fams = {p.family for _, _, p in P}
    assert fams >= {"conv_n4", "lean1", "lean5", "lean6", "lean7", "conv3p", "gemm8", "gemm"} | {f"lconv3:{g}" for g in (0, 1, 2, 4, 5)} | \
        {"wconv3:3", "wconv3:6"}, fams
    # every case lands in the family its list is named for, and its tag names it
    for fam, lst in K.FAMILIES.items():
        for c in lst:
            p = K.predict(c, CUS)
            want = {"lean": "lean", "lean_conv1": "lean", "gemm8": "gemm8 ", "gen1": "gemm ", "conv_n4": "conv_n4", "lconv": ("lconv3", "wconv3"),
                    "conv3p": "conv3p+gn"}[fam]
            assert p.tag.startswith(want), (fam, c, p.tag)
            d = p.d
            assert max(d.M * d.K, d.N * d.K, d.M * d.N) * d.batch <= 4.2e6 and d.M * d.N * d.K * d.batch <= 2e9, (c, d.M, d.N, d.K)

    def of(f):
        return [(c, p) for _, c, p in P if p.family.startswith(f)]
    # lean GEMM: instantiations (plain | GEGLU | LN | LN + GEGLU | statistics), split counts with a short last slice, ragged tails
    for cfg, forms in (("lean1", {"plain", "geglu", "ln", "ln+geglu", "stats"}), ("lean5", {"plain", "ln", "stats"}),
                       ("lean6", {"plain", "geglu", "ln"}), ("lean7", {"ln", "ln+geglu"})):
        got = {("ln" if p.d.ln else "") + ("+" if p.d.ln and c.get("geglu") else "") + ("geglu" if c.get("geglu") else "") or
               ("stats" if p.d.colstats else "plain") for c, p in of(cfg)}
        assert got >= forms, (cfg, got)
    for cfg in ("lean1", "lean5", "lean6"):
        sk = {(p.plan.splitk, p.plan.nkt - (p.plan.splitk - 1) * p.plan.kt_per < p.plan.kt_per) for c, p in of(cfg)}
        assert (1, False) in sk and ((2, True) in sk or (3, True) in sk), (cfg, sk)
        # (configuration 5 serves N % 160 == 0 only: it has no N tail)
        assert any(p.d.M % p.plan.bm for c, p in of(cfg)) and (cfg == "lean5" or any(p.d.N % p.plan.bn for c, p in of(cfg)))
    assert {(2, True), (3, True)} <= {(p.plan.splitk, p.plan.nkt % p.plan.kt_per != 0) for c, p in of("lean")}
    assert {p.plan.tiles_n for c, p in of("lean7")} >= {1, 2, 4}
    conv1 = [(c, p) for c, p in of("lean") if c["kind"] == "conv"]
    assert any(p.plan.splitk == 2 and (c["C1"] // 64) % p.plan.kt_per != 0 for c, p in conv1)
    # gemm8: both widths, whole tiles and stream-K ranges that straddle a tile, every instantiation
    g8 = of("gemm8")
    assert {p.plan.bn for c, p in g8} == {128, 160} and {p.plan.fixup for c, p in g8} == {True, False}
    assert any(p.plan.fixup and p.plan.nkt % p.plan.ipw != 0 and p.plan.tiles > 1 for c, p in g8)
    for bn in (128, 160):
        sub = [(c, p) for c, p in g8 if p.plan.bn == bn]
        assert {c["kind"] for c, p in sub} == {"gemm", "conv"} and any(p.d.colstats for c, p in sub), bn
        assert any(p.d.M < 256 for c, p in sub) and any(p.d.M > 256 for c, p in sub)
    assert any(c.get("trans") for c, p in g8) and any(p.d.batch == 3 for c, p in g8) and any(c.get("geglu") for c, p in g8)
    assert {c.get("act") for c, p in g8} >= {"relu", "silu"} and any(c.get("f32") for c, p in g8)
    assert {p.d.knobs["rows_epi"] for c, p in g8} == {0, 1} and any(0 < p.d.knobs["n_block"] < p.plan.tiles_n and p.plan.tiles_n % p.d.knobs["n_block"]
                                                                     for c, p in g8)
    assert {(p.d.stride, p.d.pad_t, p.d.upsample, p.d.C2 > 0) for c, p in g8 if c["kind"] == "conv" and p.d.ksize == 3} >= \
        {(2, 1, 0, False), (2, 0, 0, False), (1, 1, 1, False), (1, 1, 0, False), (1, 1, 0, True)}
    # first generation: fix-up on and off, GEMM and convolution
    g1 = of("gemm")
    g1 = [(c, p) for c, p in g1 if p.family == "gemm"]
    assert {(c["kind"], p.plan.fixup) for c, p in g1} == {("gemm", True), ("gemm", False), ("conv", True), ("conv", False)}
    assert {p.d.N for c, p in g1} >= {4, 12, 64}
    # lean / wide convolutions: geometries, slices with a short last slice, statistics, residual, row vector
    lc = of("lconv3") + of("wconv3")
    assert {(p.plan.splitk, p.plan.chunks % p.plan.ch_per != 0) for c, p in lc} >= {(1, False), (2, True), (3, True)}
    for geo in (0, 1, 2, 3, 4, 5, 6):
        sub = [(c, p) for c, p in lc if p.plan.geo == geo]
        assert sub and any(p.d.colstats for c, p in sub) and {c["B"] for c, p in sub} >= {1, 3}, geo
    assert any(p.d.N % p.plan.bn for c, p in lc) and any(c.get("res") for c, p in lc) and any(c.get("rowvec") for c, p in lc)
    # conv3p+gn: tilings, widths, sources, activation, whole tiles and cuts between chunks, statistics, ragged image groups
    c3 = of("conv3p")
    assert {(p.geo.TW, p.geo.TH, p.geo.NI) for c, p in c3} == {(32, 8, 1), (16, 16, 1), (8, 8, 4)}
    assert {p.plan.bn for c, p in c3} == {128, 160} and {p.plan.fixup for c, p in c3} == {True, False}
    assert {p.d.in_act for c, p in c3} == {0, 1} and {p.d.C2 > 0 for c, p in c3} == {True, False} and any(p.d.colstats for c, p in c3)
    assert {c["B"] % 4 for c, p in c3 if p.geo.NI == 4} >= {1, 3}
    # conv_n4
    assert {(c["H"], c["W"]) for c, p in of("conv_n4")} == {(13, 9), (8, 8), (24, 40)} and {c["C1"] for c, p in of("conv_n4")} == {64, 512}
    # every convolution route has the two hostile-value variants, every GEMM route its two
    vf = {K.predict(c, CUS).family for c in K.CONV_VARIANT_CASES}
    assert vf >= {f"lconv3:{g}" for g in (0, 1, 2, 4, 5)} | {"wconv3:3", "wconv3:6", "conv3p", "gemm8", "gemm", "conv_n4", "lean1"}, vf
    assert {K.predict(c, CUS).family for c in K.GEMM_VARIANT_CASES} >= {"lean1", "lean5", "lean6", "gemm8", "gemm"}


def test_mirrors_follow_the_cu_count():
    """the mirrors are parametrised by the device's CU count: a smaller chip plans fewer stream-K workgroups"""
    c = dict(K.G(257, 136, 6400), knobs={"lean": 0})
    assert K.predict(c, 256).plan.G > K.predict(c, 64).plan.G
