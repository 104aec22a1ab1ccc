"""tests/footprint.py can fail: planted violations by CPU stand-in "kernels" (torch functions) are each rejected, with a
message that names the region; a correct stand-in passes; the sentinel comparison is bitwise."""
import pytest
import torch

import footprint as fp

CPU = torch.device("cpu")
ROWS, COLS, LD = 7, 24, 40


def _rowsum_kernel(x_view, out_view):
    """a correct stand-in: out[r] = sum of the row's payload"""
    out_view.copy_(x_view.float().sum(-1, keepdim=True))


def _operands(dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(0)
    return torch.randn((ROWS, COLS), generator=g).to(dtype)


def test_layout_and_guard_sizes():
    view, rec = fp.guarded((3, ROWS, COLS), torch.bfloat16, CPU, ld=LD)
    assert view.shape == (3, ROWS, COLS) and view.stride() == (ROWS * LD, LD, 1)
    assert rec.lead >= fp.GUARD_MIN_BYTES and rec.trail >= fp.GUARD_MIN_BYTES
    wide, wrec = fp.guarded((2, 1024), torch.float32, CPU, ld=1040)
    assert wrec.lead >= 256 * 1040 * 4 and wrec.trail >= 256 * 1040 * 4          # at least 256 rows of the view on each side
    assert view.data_ptr() % 16 == 0 and wide.data_ptr() % 16 == 0
    assert fp.holds_sentinel(view)                                                # the payload starts out as sentinel
    view.zero_()
    assert not fp.holds_sentinel(view)
    fp.assert_untouched(rec)
    s, srec = fp.exact_scratch(1000, CPU)
    assert s.numel() == 1000 and s.dtype == torch.uint8 and s.data_ptr() % 16 == 0 and srec.body == 1000
    fp.assert_untouched(srec)


def test_correct_kernel_passes():
    x = _operands()
    want = torch.empty((ROWS, 1))
    _rowsum_kernel(x, want)
    xv, xrec = fp.poisoned(x, ld=LD)
    ov, orec = fp.guarded((ROWS, 1), torch.float32, CPU, ld=3)
    _rowsum_kernel(xv, ov)
    assert fp.bit_equal(ov, want) and not fp.holds_sentinel(ov)
    fp.assert_untouched(xrec)
    fp.assert_untouched(orec)


def test_write_into_lead_guard_is_caught():
    ov, rec = fp.guarded((ROWS, COLS), torch.bfloat16, CPU, ld=LD)
    ov.zero_()
    ov.as_strided((1,), (1,), ov.storage_offset() - 1).fill_(1.0)      # one element before the view
    with pytest.raises(AssertionError, match="lead guard") as e:
        fp.assert_untouched(rec)
    assert f"byte {rec.lead - 2} " in str(e.value)


def test_write_into_trail_guard_is_caught():
    ov, rec = fp.guarded((ROWS, COLS), torch.bfloat16, CPU, ld=LD)
    ov.zero_()
    end = ov.storage_offset() + (ROWS - 1) * LD + COLS
    ov.as_strided((1,), (1,), end).fill_(1.0)                          # one element past the last row's payload
    with pytest.raises(AssertionError, match=r"trail guard \(0 bytes past") as e:
        fp.assert_untouched(rec)
    assert f"byte {rec.lead + rec.body} " in str(e.value)


def test_write_into_ld_gap_of_a_middle_row_is_caught():
    ov, rec = fp.guarded((ROWS, COLS), torch.bfloat16, CPU, ld=LD)
    ov.zero_()
    ov.as_strided((1,), (1,), ov.storage_offset() + 3 * LD + COLS).fill_(1.0)   # row 3, first gap element
    with pytest.raises(AssertionError, match="ld gap of row 3") as e:
        fp.assert_untouched(rec)
    assert f"column {COLS})" in str(e.value)


def test_write_past_exact_scratch_is_caught():
    s, rec = fp.exact_scratch(1000, CPU)
    s.zero_()
    fp.assert_untouched(rec)
    s.as_strided((1,), (1,), s.storage_offset() + 1000).fill_(0)
    with pytest.raises(AssertionError, match=r"trail guard \(0 bytes past"):
        fp.assert_untouched(rec)


def test_reading_the_full_ld_wide_row_is_caught_by_poison():
    x = _operands()
    want = torch.empty((ROWS, 1))
    _rowsum_kernel(x, want)
    xv, xrec = fp.poisoned(x, ld=LD)

    def wrong_kernel(x_view, out_view):                                # sums ld columns instead of the payload
        rows = x_view.as_strided((ROWS, LD), (LD, 1))
        out_view.copy_(rows.float().sum(-1, keepdim=True))
    got = torch.empty((ROWS, 1))
    wrong_kernel(xv, got)
    assert not fp.bit_equal(got, want)
    assert bool(torch.isnan(got).all())
    fp.assert_untouched(xrec)                                          # reading leaves no trace: only the poison shows it


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_comparison_is_bitwise_nan_over_nan(dtype):
    ov, rec = fp.guarded((ROWS, COLS), dtype, CPU, ld=LD)
    gap = ov.as_strided((1,), (1,), ov.storage_offset() + 2 * LD + COLS)
    assert bool(torch.isnan(gap).all())                                # the sentinel is a NaN ...
    gap.fill_(float("nan"))                                            # ... overwritten by the canonical NaN: still NaN, other bits
    assert bool(torch.isnan(gap).all())
    with pytest.raises(AssertionError, match="ld gap of row 2"):
        fp.assert_untouched(rec)
    # and bit_equal tells two NaNs with different payloads apart, and +0 from -0
    a = torch.zeros((4,), dtype=dtype)
    b = a.clone()
    b[1] = -0.0
    assert torch.equal(a, b) and not fp.bit_equal(a, b)
    n1, _ = fp.guarded((4,), dtype, CPU)
    n2 = torch.full((4,), float("nan"), dtype=dtype)
    assert not fp.bit_equal(n1, n2)
    assert fp.bit_equal(n1, n1.clone())


def test_poison_patterns():
    for dtype, pat in ((torch.bfloat16, 0x7FC1), (torch.float32, 0x7FC00001), (torch.uint8, 0xFF), (torch.int32, 0xFFFFFFFF)):
        t = torch.zeros((2, 4), dtype=dtype)
        v, rec = fp.poisoned(t, ld=8)
        assert rec.pattern == pat == fp.in_poison(dtype)
        gap = v.as_strided((1,), (1,), v.storage_offset() + 4)
        assert int(fp.bits(gap)[0]) & ((1 << (8 * t.element_size())) - 1) == pat
        assert bool((v == 0).all())
        fp.assert_untouched(rec)


def test_every_entry_point_of_the_header_is_in_the_table_or_exempt():
    """every function include/udt_kernels.h declares has a case in tests/test_footprint_gpu.py, or an entry in its EXEMPT table
    that says why it has no footprint to check"""
    import os
    import re

    import test_footprint_gpu as table
    from udifftext_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "udt_kernels.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(udt_[a-z0-9_]+)\s*\(", code))
    assert declared == set(lib.SYMBOLS), declared ^ set(lib.SYMBOLS)
    covered = {name for _, _, covers in table.CASES for name in covers}
    assert not (covered - declared), covered - declared
    assert not (set(table.EXEMPT) - declared), set(table.EXEMPT) - declared
    assert not (covered & set(table.EXEMPT)), covered & set(table.EXEMPT)
    missing = declared - covered - set(table.EXEMPT)
    assert not missing, f"no footprint case and no stated exemption: {sorted(missing)}"
    assert all(reason for reason in table.EXEMPT.values())
    assert set(table.COMPARED) <= {c[0] for c in table.CASES}
