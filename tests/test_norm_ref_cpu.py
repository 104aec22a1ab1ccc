"""tests/norm_ref.py and tests/norm_cases.py without a GPU: the references pinned against independent torch compositions, the launcher
mirrors' own properties, every case and variant of tests/test_norm_edges_gpu.py passed by a float32 restatement of norm.hip's stated
decompositions through the SAME hold_* functions (no case needs the kernel in order to pass), and seven planted defects, each failing
in the slice that holds it.  One line per check goes to norm_ref_cpu_report.txt in the temporary directory.
"""
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

import norm_cases as K
import norm_ref as R
import shadow_ref as SR
import sliced_check as S

REPORT = os.path.join(tempfile.gettempdir(), "norm_ref_cpu_report.txt")
G = K.G


# ------------------------------------------------------------------------------------------------ the references, pinned
@pytest.mark.parametrize("shape", [(2, 33, 64, 32), (1, 100, 320, 0)])
@pytest.mark.parametrize("silu", [0, 1])
def test_norm_ref_group_norm_is_torch_group_norm_in_float64(shape, silu):
    x, x2, gamma, beta = K.gn_inputs(*shape, "randn")
    exp = R.gn_expect(x, gamma, beta, 1e-5, silu, x2)
    cat = R.cat_sources(x, x2)
    want = F.group_norm(cat.permute(0, 2, 1), G, gamma.double(), beta.double(), 1e-5).permute(0, 2, 1)
    want = F.silu(want) if silu else want
    assert float((exp["ref"] - want).abs().max()) < 1e-12
    assert torch.equal(exp["emul"], exp["ref"].float().bfloat16().double()) and exp["emul"].dtype == torch.float64
    # the condition scale, written out per element
    B, HW, C = cat.shape
    cpg = C // G
    a = torch.zeros_like(cat)
    for b in range(B):
        for g in range(G):
            blk = cat[b, :, g * cpg:(g + 1) * cpg]
            rstd = 1.0 / (blk.var(unbiased=False) + 1e-5).sqrt()
            sc = rstd * gamma.double()[g * cpg:(g + 1) * cpg]
            a[b, :, g * cpg:(g + 1) * cpg] = blk.abs() * sc.abs() + (beta.double()[g * cpg:(g + 1) * cpg] - blk.mean() * sc).abs()
    assert abs(exp["A"] / float(a.pow(2).mean().sqrt()) - 1) < 1e-12


@pytest.mark.parametrize("rows,C", [(5, 520), (1, 8)])
def test_norm_ref_layer_norm_is_the_formula_in_float64(rows, C):
    x, gamma, beta = K.ln_inputs(rows, C, "tails")
    exp = R.ln_expect(x, gamma, beta, 1e-6)
    xd = x.double()
    mean = xd.sum(-1, keepdim=True) / C
    var = ((xd - mean) ** 2).sum(-1, keepdim=True) / C
    want = (xd - mean) / (var + 1e-6).sqrt() * gamma.double() + beta.double()
    assert float((exp["ref"] - want).abs().max()) < 1e-12
    a = (xd - mean).abs() / (var + 1e-6).sqrt() * gamma.double().abs() + beta.double().abs()
    assert abs(exp["A"] / float(a.pow(2).mean().sqrt()) - 1) < 1e-12


def test_norm_ref_partials_and_records_are_direct_sums():
    B, HW, C1, C2 = 2, 289, 64, 32
    x, x2, _, _ = K.gn_inputs(B, HW, C1, C2, "tails")
    cat = R.cat_sources(x, x2)
    n = K.gn_nchunks(HW)
    ref, ab = R.stats_partials(x, n, x2)
    assert n == 18 and ref.shape == (B, 18, G, 2)
    cpg = (C1 + C2) // G
    for k in (0, 7, 16, 17):
        blk = cat[:, k * 17:min(HW, (k + 1) * 17)].reshape(B, -1, G, cpg)
        assert torch.allclose(ref[:, k, :, 0], blk.sum(dim=(1, 3)), rtol=1e-13, atol=1e-12)
        assert torch.allclose(ref[:, k, :, 1], (blk * blk).sum(dim=(1, 3)), rtol=1e-13, atol=1e-12)
        assert torch.allclose(ab[:, k, :, 0], blk.abs().sum(dim=(1, 3)), rtol=1e-13, atol=1e-12)
    assert bool((ref[:, 17] == 0).all()) and bool((ab[:, 17] == 0).all())          # the empty chunk
    rec = R.records(x2, 7)                                                          # 7 slots of 42 rows: the last one holds 37
    assert rec.shape == (B * 7, C2, 2) and rec.dtype == torch.float32
    for b in range(B):
        for s in (0, 6):
            blk = x2[b, s * 42:min(HW, (s + 1) * 42)].double()
            assert torch.equal(rec[b * 7 + s, :, 0], blk.sum(0).float()) and torch.equal(rec[b * 7 + s, :, 1], (blk * blk).sum(0).float())
    empty = R.records(x[:, :9], 7)                                                  # 9 pixels in 7 slots of 2 rows: slots 5, 6 empty
    assert bool((empty.reshape(B, 7, C1, 2)[:, 5:] == 0).all()) and bool((empty.reshape(B, 7, C1, 2)[:, 4, :, 1] > 0).all())


def test_norm_ref_table_from_records_is_the_table_of_the_data_up_to_record_rounding():
    B, HW, C1, C2 = 1, 289, 320, 64
    x, x2, gamma, beta = K.gn_inputs(B, HW, C1, C2, "randn")
    rec1, rec2 = K.gn_records(x, x2, 23, 2)
    t = R.table_from_records(rec1, 23, gamma, beta, HW, 1e-5, rec2, 2)
    want = SR.ref_gn_table(x, gamma, beta, G, 1e-5, x2=x2)
    assert t["table"].shape == want.shape == (B, 6, 2, 64)
    assert float(((t["table"] - want).abs() / t["abs"]).max()) < 1e-5              # fp32 records: 2^-24 per record, amplified by mean^2 / var
    by_data = R.gn_expect(x, gamma, beta, 1e-5, 1, x2)
    by_rec = R.gn_expect_records(x, rec1, 23, gamma, beta, 1e-5, 1, x2, rec2, 2)
    assert float((by_data["ref"] - by_rec["ref"]).abs().max()) < 1e-4 and abs(by_data["A"] / by_rec["A"] - 1) < 1e-5
    # exact records (a constant sample) give the data's table exactly: q / n - mean^2 is 0 in float64
    xc = torch.full((1, 100, 128), -3.0)
    tc = R.table_from_records(R.records(xc, 3), 3, gamma[:128], beta[:128], 100, 1e-6)
    assert torch.equal(tc["table"][:, :, 0].reshape(-1), gamma[:128].double() / (1e-6 ** 0.5))


# ------------------------------------------------------------------------------------------------ the mirrors' own properties
def test_norm_mirror_properties():
    assert [K.gn_nchunks(hw) for hw in (1, 9, 15, 16, 33, 289, 2047, 2048, 2100)] == [1, 1, 1, 1, 2, 18, 127, 128, 128]
    assert R.chunk_rows(289, 18) == 17 and 17 * 17 == 289                              # chunk 17 of (.,289,.) is empty
    assert R.chunk_rows(2100, 128) == 17 and 2100 - 123 * 17 == 9                      # ragged chunk 123, chunks 124 .. 127 empty
    for shape, gw in K.STRIP_GW.items():
        assert K.gn_strip_groups(*shape[1:]) == gw, shape
    assert set(K.STRIP_GW.values()) == {1, 2, 4, 8} and set(K.STRIP_GW) == set(K.STRIP)
    assert K.gn_strip_groups(819, 320, 0) == 4 and K.gn_strip_groups(820, 320, 0) == 0 and 819 * 40 * 2 <= 65536 < 820 * 40 * 2
    assert K.gn_strip_groups(256, 4096, 0) == 1 and K.gn_strip_groups(257, 4096, 0) == 0 and 256 * 128 * 2 == 65536
    for shape in K.STRIP_REFUSED:
        assert K.gn_strip_groups(*shape[1:]) == 0 and K.gn_strip_groups(*shape[1:], limit=False) > 0
    assert K.gn_strip_groups(16, 8192 + 64, 0) == 0                                    # cw > 256
    assert K.gn_strip_groups(16, 32, 0) == 8 and K.gn_strip_groups(16, 96, 4) == 0     # cpg 1: eight groups per 16 bytes; C2 % 8
    geo = lambda s: K.strip_geometry(s[2], s[3], K.STRIP_GW[s])
    assert geo((2, 33, 64, 32)) == {"cw": 24, "nch": 3, "pstep": 170, "idle": 2}
    assert geo((2, 9, 320, 0)) == {"cw": 40, "nch": 5, "pstep": 102, "idle": 2}
    assert geo((1, 64, 1280, 640)) == {"cw": 120, "nch": 15, "pstep": 34, "idle": 2}
    assert geo((1, 64, 2560, 0))["pstep"] == 51 and geo((1, 16, 3200, 0)) == {"cw": 200, "nch": 25, "pstep": 20, "idle": 12}
    assert geo((1, 256, 4096, 0)) == {"cw": 128, "nch": 16, "pstep": 32, "idle": 0}
    assert R.strip_seam(819, 102) == 816 and R.strip_seam(256, 32) == 256 and R.strip_seam(64, 34) == 0      # loop + tail, no tail, tail only
    assert [K.stats_layout(c) for c in (64, 320, 1024, 2048, 2560, 4096)] == \
        [(32, 0, False), (6, 16, False), (2, 0, False), (1, 0, False), (1, 0, True), (1, 0, True)]
    assert [K.finalize_lanes(s[2] + s[3]) for s, _, _ in K.REC_TABLE] == [64, 12, 21, 3, 2]
    assert [(s1 > K.finalize_lanes(s[2] + s[3])) for s, s1, _ in K.REC_TABLE] == [False, False, True, True, True]
    assert [K.ln_nch(c) for c in K.LN_C] == [1, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8]
    # the apply pass: 1024 pieces per workgroup
    pieces = lambda s: s[1] * (s[2] + s[3]) // 8
    assert pieces((1, 9, 320, 0)) == 360 and pieces((1, 2100, 64, 0)) == 16 * 1024 + 416 and 768 < pieces((1, 125, 64, 0)) < 1024
    assert K.tail_pixels(289, 320, 0)[:4] == [0, 16, 17, 33] and 288 in K.tail_pixels(289, 320, 0)
    assert {407, 408, 815, 816, 818} <= set(K.tail_pixels(819, 320, 0))


# ------------------------------------------------------------------------------------------------ every case, float32 restatement
def _two32(x, x2, gamma, beta, eps, act, n):
    return R.gn_two_kernel32(x, gamma, beta, eps, act, n, x2=x2)


def _strip32(x, x2, gamma, beta, eps, act, gw):
    return R.gn_strip32(x, gamma, beta, eps, act, gw, x2=x2)


def _rec32(x, x2, rec1, slots1, rec2, slots2, gamma, beta, eps, act):
    return R.gn_records32(x, rec1, slots1, gamma, beta, eps, act, x2=x2, rec2=rec2, slots2=slots2)


@pytest.mark.parametrize("shape", K.TWO_KERNEL + K.STRIP_REFUSED)
def test_restated_two_kernel_group_norm_passes_every_case(shape):
    for variant, eps, act in K.VARIANTS:
        w, units = K.case_two_kernel(shape, variant, eps, act, _two32, report=REPORT)
        assert w < 1.0 and units <= S.FP32_SUM_UNITS


@pytest.mark.parametrize("shape", K.STRIP)
def test_restated_strip_group_norm_passes_every_case(shape):
    for variant, eps, act in K.VARIANTS:
        assert K.case_strip(shape, variant, eps, act, _strip32, report=REPORT) < 1.0


@pytest.mark.parametrize("form,shape,slots1,slots2", [("strip",) + c for c in K.REC_STRIP] + [("table",) + c for c in K.REC_TABLE])
def test_restated_group_norm_from_records_passes_every_case(form, shape, slots1, slots2):
    for variant, eps, act in K.VARIANTS:
        w, units = K.case_records(form, shape, slots1, slots2, variant, eps, act, _rec32, report=REPORT)
        assert w < 1.0 and units <= S.FP32_SUM_UNITS


def test_records_cases_hold_an_all_zero_slot_in_each_form():
    for cases, shape, slots in ((K.REC_STRIP, (2, 9, 320, 0), 7), (K.REC_TABLE, (1, 16, 4096, 0), 5)):
        assert (shape, slots, 0) in cases
        x, _, _, _ = K.gn_inputs(*shape, "randn")
        rec = R.records(x, slots).reshape(shape[0], slots, shape[2], 2)
        assert bool((rec[:, -1] == 0).all()) and bool((rec[:, 0, :, 1] > 0).all())


@pytest.mark.parametrize("C", K.LN_C)
def test_restated_layer_norm_passes_every_case(C):
    for rows in K.LN_ROWS:
        for variant, eps in K.LN_VARIANTS:
            assert K.case_ln(rows, C, variant, eps, R.layer_norm32, report=REPORT) < 1.0


# ------------------------------------------------------------------------------------------------ planted defects
def _inside(idx, region):
    """every range of a reported slice index lies inside ``region`` (one (lo, hi) per dimension)"""
    return all(lo <= (0 if a is None else a) and (10 ** 9 if b is None else b) <= hi for (a, b), (lo, hi) in zip(idx, region))


def _fails_in(fn, regions, n_units):
    """fn() must fail check_sliced, in at most ``n_units`` slices, every reported one inside one of ``regions``"""
    with pytest.raises(AssertionError, match="slices out of bound") as e:
        fn()
    n_fail, n_all, idxs = K.failed_slices(str(e.value))
    assert 1 <= n_fail <= 2 * n_units < n_all, str(e.value)                           # a slice can be reported twice: rms and max
    assert idxs and all(any(_inside(i, r) for r in regions) for i in idxs), (idxs, regions, str(e.value))


FULL = (0, 10 ** 9)


def test_defect_last_pixel_of_one_chunk_dropped_for_one_channel_chunk():
    """sample 1, chunk 5 (pixels 85:102), channel chunk 5 (channels 40:48, inside group 4 = 40:50): caught on ``tails``, whose spikes sit
    on the chunks' first and last pixels — and recorded here to PASS on ``randn`` (the group's rstd moves by about 0.1 %, under the bf16
    floor), which is why the variant exists"""
    shape, defect = (2, 289, 320, 0), ("drop_last_pixel", 1, 5, 5)
    impl = lambda x, x2, gamma, beta, eps, act, n: R.gn_two_kernel32(x, gamma, beta, eps, act, n, x2=x2, defect=defect)
    assert 101 in K.tail_pixels(289, 320, 0)

    def run(variant):
        x, x2, gamma, beta = K.gn_inputs(*shape, variant)
        y, part = impl(x, x2, gamma, beta, 1e-5, 0, 18)
        K.hold_gn(f"defect dropped pixel {variant}", y, R.gn_expect(x, gamma, beta, 1e-5, 0), ("span",), report=REPORT)
    _fails_in(lambda: run("tails"), [((1, 2), FULL, (40, 50))], 1)
    run("randn")                                                                       # the recorded miss
    # the partials name the chunk and the group on either variant
    x, x2, gamma, beta = K.gn_inputs(*shape, "randn")
    _, part = impl(x, x2, gamma, beta, 1e-5, 0, 18)
    with pytest.raises(AssertionError, match=r"1 of 1152 elements .* at \(1, 5, 4\)"):
        K.hold_partials("defect dropped pixel randn", part, *R.stats_partials(x, 18), report=REPORT)


def test_defect_seam_pixel_counted_twice_in_one_strip():
    """strip 3 of (1,819,320,0) (channels 120:160, groups 12 .. 15) counts pixel 816 — lane 0's first tail-loop pixel — twice"""
    shape = (1, 819, 320, 0)
    x, x2, gamma, beta = K.gn_inputs(*shape, "tails")
    y = R.gn_strip32(x, gamma, beta, 1e-6, 0, 4, defect=("double_seam", 0, 3))
    exp = R.gn_expect(x, gamma, beta, 1e-6, 0)
    _fails_in(lambda: K.hold_gn("defect seam", y, exp, ("strip", 40), report=REPORT), [((0, 1), FULL, (120, 160))], 4)
    S.check_sliced("sound seam", R.gn_strip32(x, gamma, beta, 1e-6, 0, 4), exp["ref"], exp["emul"] - exp["ref"], S.gn_strip_slices(1, 320, 40),
                   abs_scale=exp["A"], report=REPORT)
    _fails_in(lambda: S.check_sliced("defect seam by strip", y, exp["ref"], exp["emul"] - exp["ref"], S.gn_strip_slices(1, 320, 40),
                                     abs_scale=exp["A"], report=REPORT), [((0, 1), FULL, (120, 160))], 1)


def test_defect_straddling_group_reads_only_the_first_source():
    """(2,100,320,64): group 26 = channels 312:324 straddles C1 = 320 (and the 64-channel block boundary)"""
    shape = (2, 100, 320, 64)
    x, x2, gamma, beta = K.gn_inputs(*shape, "randn")
    y, _ = R.gn_two_kernel32(x, gamma, beta, 1e-5, 1, 6, x2=x2, defect=("straddle_first_only",))
    _fails_in(lambda: K.hold_gn("defect straddle", y, R.gn_expect(x, gamma, beta, 1e-5, 1, x2), ("span",), report=REPORT),
              [((0, 1), FULL, (312, 324)), ((1, 2), FULL, (312, 324))], 2)


def test_defect_records_beyond_the_slot_lanes_ignored():
    """(1,289,320,64) at 23 + 2 slots, cpg 12: 21 slot lanes, records 21 and 22 of the first source's channels are lost — every group that
    holds a first-source channel (0 .. 26, channels below 324) fails, the five groups of the second source alone pass"""
    shape = (1, 289, 320, 64)
    x, x2, gamma, beta = K.gn_inputs(*shape, "randn")
    rec1, rec2 = K.gn_records(x, x2, 23, 2)
    y, table = R.gn_records32(x, rec1, 23, gamma, beta, 1e-5, 0, x2=x2, rec2=rec2, slots2=2, defect=("lanes_only",))
    exp = R.gn_expect_records(x, rec1, 23, gamma, beta, 1e-5, 0, x2, rec2, 2)
    with pytest.raises(AssertionError, match="slices out of bound") as e:
        K.hold_gn("defect slot lanes", y, exp, ("span",), report=REPORT)
    n_fail, n_all, idxs = K.failed_slices(str(e.value))
    assert n_all == 32 and 27 <= n_fail <= 54 and all(_inside(i, ((0, 1), FULL, (0, 324))) for i in idxs), str(e.value)
    t = R.table_from_records(rec1, 23, gamma, beta, 289, 1e-5, rec2, 2)
    with pytest.raises(AssertionError, match=r"^defect slot lanes table scale: 324 of 384 elements"):
        K.hold_table("defect slot lanes", table, t, report=REPORT)
    K.hold_table("sound slot lanes", table[:, 5:, :, 4:], {k: t[k][:, 5:, :, 4:] for k in ("table", "abs")}, report=REPORT)    # channels 324:384


def test_defect_table_entry_written_into_the_neighbouring_block():
    """(2,289,640,0): sample 1's entry of channel 70 lands at column 6 of block 2 (channel 134's place); its own place stays 0"""
    shape = (2, 289, 640, 0)
    x, x2, gamma, beta = K.gn_inputs(*shape, "randn")
    rec1, _ = K.gn_records(x, None, 12, 0)
    y, table = R.gn_records32(x, rec1, 12, gamma, beta, 1e-5, 1, defect=("table_neighbour", 1, 70))
    t = R.table_from_records(rec1, 12, gamma, beta, 289, 1e-5)
    with pytest.raises(AssertionError, match=r"2 of 1280 elements .* at \(1, [12], 6\)"):
        K.hold_table("defect table block", table, t, report=REPORT)
    exp = R.gn_expect_records(x, rec1, 12, gamma, beta, 1e-5, 1)
    _fails_in(lambda: K.hold_gn("defect table block", y, exp, ("span",), report=REPORT),
              [((1, 2), FULL, (60, 80)), ((1, 2), FULL, (120, 140))], 2)


def test_defect_layer_norm_mean_without_the_second_lane_chunk():
    """C = 520: row 5's mean leaves out channels 512:520 (lane 0's chunk ``lane + 64``).  Units of fewer than 1024 elements merge with
    their successors and keep the first one's name: the slices are [0:4, 0:512] and [0:4, 512:520] + rows 4:7 — row 5 is in the second"""
    x, gamma, beta = K.ln_inputs(7, 520, "offset")
    exp = R.ln_expect(x, gamma, beta, 1e-5)
    y = R.layer_norm32(x, gamma, beta, 1e-5, defect=("skip_second_chunk", 5))
    with pytest.raises(AssertionError, match="slices out of bound") as e:
        K.hold_ln("defect ln chunk", y, exp, x, beta, report=REPORT)
    n_fail, n_all, idxs = K.failed_slices(str(e.value))
    assert n_all == 2 and n_fail <= 2 and all(i == [(0, 4), (512, 520)] for i in idxs), str(e.value)
    good = R.layer_norm32(x, gamma, beta, 1e-5)
    assert torch.equal(y[:5], good[:5]) and torch.equal(y[6:], good[6:]) and not torch.equal(y[5], good[5])


def test_defect_eps_omitted_is_exposed_by_the_constant_variant():
    shape = (2, 289, 320, 0)
    x, x2, gamma, beta = K.gn_inputs(*shape, "constant")
    y, _ = R.gn_two_kernel32(x, gamma, beta, 1e-5, 0, 18, defect=("no_eps",))
    with pytest.raises(AssertionError, match="non-finite"):
        K.hold_gn("defect no eps", y, R.gn_expect(x, gamma, beta, 1e-5, 0), ("span",), report=REPORT)
    xr, _, _, _ = K.gn_inputs(*shape, "randn")                                         # ... and by no other variant: eps is 1e-5 of a variance of 4
    yr, _ = R.gn_two_kernel32(xr, gamma, beta, 1e-5, 0, 18, defect=("no_eps",))
    K.hold_gn("defect no eps randn", yr, R.gn_expect(xr, gamma, beta, 1e-5, 0), ("span",), report=REPORT)
    xl, gl, bl = K.ln_inputs(5, 520, "constant")
    with pytest.raises(AssertionError, match="non-finite"):
        K.hold_ln("defect ln no eps", R.layer_norm32(xl, gl, bl, 1e-5, defect=("no_eps",)), R.ln_expect(xl, gl, bl, 1e-5), xl, bl, report=REPORT)


def test_restated_constant_rows_and_groups_are_exact():
    """a constant LayerNorm row is bf16(beta) bit for bit (hold_ln asserts it; here: that the rows exist), a constant group's mean and
    variance are exact in the two-kernel form"""
    x, gamma, beta = K.ln_inputs(7, 4096, "constant")
    assert (x == x[:, :1]).all(dim=1).tolist() == [True, False, False, True, False, False, True]
    y = R.layer_norm32(x, gamma, beta, 1e-6)
    assert torch.equal(y[0], beta.bfloat16()) and torch.equal(y[3], beta.bfloat16())
    xg, _, gg, bg = K.gn_inputs(1, 2100, 64, 0, "constant")
    assert bool((xg[:, :, 6:8] == 0.5).all()) and bool((xg[:, :, 62:] == -3.0).all())
    _, part = R.gn_two_kernel32(xg, gg, bg, 1e-6, 0, 128)
    tot = part.double().sum(1)[0]
    assert tot[3].tolist() == [0.5 * 4200, 0.25 * 4200] and tot[31].tolist() == [-3.0 * 4200, 9.0 * 4200]
