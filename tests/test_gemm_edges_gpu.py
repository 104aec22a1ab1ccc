"""The forward GEMM and convolution kernels behind udt_gemm (csrc/gemm.hip: conv_n4, the lean GEMMs 1 / 5 / 6 and the row-resident 7, lconv3 /
wconv3 with geometries 0 .. 6, conv3p+gn, gemm8 on both tile widths, the first-generation 256 x 64 kernel) at the edges no other
kernel-level test launches (``pytest -m gpu``): the smallest shapes that reach each branch of the planners, routes forced through
udt_debug_set only, every launch's profiler tag asserted against the tag tests/gemm_cases.py's mirror of the planners predicts for this
device's CU count, each result held tile by tile (one wave's outputs of one tile; image x tile x N-tile for the convolutions, then border
ring against interior) to a float64 reference by tests/sliced_check.py with its recorded margins, the bounds from tests/gemm_ref.py's
emulation of the kernels' stated roundings (never from the kernel's output), fp32 outputs and column statistics element-wise by
check_fp32_sum, the marker rows and columns around the result untouched, and every launch repeated bit for bit.
Inputs and checks: tests/gemm_cases.py, the same ones tests/test_gemm_ref_cpu.py shows a float32 CPU evaluation to pass.
One line per check goes to gemm_edges_report.txt next to the run's parity report (tests/test_backward_gpu.py REPORT);
profiles/gemm_edges_report.txt is a passing run's.
"""
import ctypes as C
import os
import tempfile

import pytest
import torch

import gemm_cases as K
import gemm_ref as R
import sliced_check as S
import test_backward_gpu

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(test_backward_gpu.REPORT), "gemm_edges_report.txt")      # a file of its own, same directory


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib, ops
    assert lib.load().udt_device_arch_ok() == 1
    assert (lib.GEMM_OUT_F32, lib.GEMM_GEGLU, lib.GEMM_RELU, lib.GEMM_TRANSPOSED, lib.GEMM_CONV, lib.GEMM_SILU_OUT) == \
        (K.F_F32, K.F_GEGLU, K.F_RELU, K.F_TRANS, K.F_CONV, K.F_SILU)
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
            path = os.path.join(tempfile.gettempdir(), "udt_gemm_edges_trace.csv")
            Env.lib.udt_prof_dump(path.encode())
            Env.lib.udt_prof_trace(0)
            return out, [ln.split(",", 2)[2] for ln in open(path).read().splitlines()[1:]]

        @staticmethod
        def reset_knobs():
            for key, v in K.KNOB_DEFAULTS.items():
                assert Env.lib.udt_debug_set(key.encode(), v) == 0
    Env.ops, Env.L, Env.lib, Env.dev = ops, lib, lib.load(), cuda
    Env.cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    Env.reset_knobs()
    yield Env
    Env.reset_knobs()


def _buf(env, shape, dtype, pad_rows=0, pad_cols=0, src=None):
    """a marker-filled device buffer ``pad_rows`` rows (second-to-last dimension) and ``pad_cols`` columns wider than ``shape``, and the
    view of ``shape`` inside it (filled from ``src`` when given)"""
    full_shape = tuple(shape[:-2]) + (shape[-2] + pad_rows, shape[-1] + pad_cols)
    full = torch.full(full_shape, K.MARKER, dtype=dtype, device=env.dev)
    view = full[..., :shape[-2], :shape[-1]]
    if src is not None:
        view.copy_(src.to(env.dev).to(dtype))
    return full, view


def _guards_ok(full, view_shape, what):
    rows, cols = view_shape[-2], view_shape[-1]
    assert bool((full[..., rows:, :] == K.MARKER).all()), f"{what}: rows past the result were written"
    assert bool((full[..., :, cols:] == K.MARKER).all()), f"{what}: columns past the result were written"


def _launch(env, c, p, t):
    """build the descriptor of a case over marker-padded buffers and launch it once -> (out view, out full, stats or None, tags)"""
    d, ops = p.d, env.ops
    bf, f32 = torch.bfloat16, torch.float32
    n_cols = d.N // 2 if c.get("geglu") else d.N
    odt = f32 if c.get("f32") else bf
    keep = []
    dev = lambda k, dt=bf: t[k].to(env.dev).to(dt).contiguous() if k in t else None
    kw = dict(M=d.M, N=d.N, K=d.K, flags=d.flags, alpha=d.alpha, rows_per_batch=d.rows_per_batch, batch=d.batch)
    if c["kind"] == "gemm":
        la, lo, lr = c.get("ld_extra", (0, 0, 0))
        bsh = (d.batch,) if d.batch > 1 else ()
        a_full, a = _buf(env, bsh + (d.M, d.K), bf, 0, la, t["a"])
        w = dev("w")
        if c.get("trans"):
            rpb = d.rows_per_batch
            o_full = torch.full((d.M // rpb + 1, d.N, rpb), K.MARKER, dtype=odt, device=env.dev)     # one more batch element as the guard
            out = o_full[:d.M // rpb]
            ldo = 0
        else:
            o_full, out = _buf(env, bsh + (d.M, n_cols), odt, K.PAD_ROWS, lo + K.PAD_COLS)
            ldo = o_full.stride(-2)
        kw.update(a=a.data_ptr(), w=w.data_ptr(), out=out.data_ptr(), lda=a_full.stride(-2), ldo=ldo)
        if d.batch > 1:
            kw.update(ldw=d.K, stride_a=a_full.stride(0), stride_w=w.stride(0), stride_out=o_full.stride(0))
        if d.residual:
            r_full, r = _buf(env, bsh + (d.M, n_cols), bf, 0, lr, t["res"])
            kw.update(residual=r.data_ptr(), ldr=r_full.stride(-2))
            keep.append(r_full)
        keep += [a_full, w]
    else:
        x, x2, w = dev("x"), dev("x2"), dev("w")
        lo = c.get("ld_extra", (0, 0, 0))[1]
        o_full, out = _buf(env, (d.M, d.N), odt, K.PAD_ROWS, lo + K.PAD_COLS)
        kw.update(a=x.data_ptr(), a2=None if x2 is None else x2.data_ptr(), w=w.data_ptr(), out=out.data_ptr(), lda=0, ldo=o_full.stride(0),
                  Hin=d.Hin, Win=d.Win, C1=d.C1, C2=d.C2, Hout=d.Hout, Wout=d.Wout, ksize=d.ksize, stride=d.stride, pad_t=d.pad_t,
                  pad_l=d.pad_l, upsample=d.upsample)
        if d.upsample == 2:
            kw.update(ldw=w.shape[2], stride_w=w.stride(0))
        if d.residual:
            r_full, r = _buf(env, (d.M, d.N), bf, 0, 8, t["res"].reshape(d.M, d.N))
            kw.update(residual=r.data_ptr(), ldr=r_full.stride(0))
            keep.append(r_full)
        if d.in_scsh:
            sc = dev("scsh", f32)
            kw.update(in_scsh=sc.data_ptr(), in_act=d.in_act)
            keep.append(sc)
        keep += [x, x2, w]
    if "bias" in t:
        b = dev("bias", f32)
        kw.update(bias=b.data_ptr())
        keep.append(b)
    if d.ln:
        s = dev("s", f32)
        kw.update(ln_colsum=s.data_ptr(), ln_eps=1e-5)
        keep.append(s)
    if d.rowvec:
        rv = dev("rowvec", f32)
        kw.update(rowvec=rv.data_ptr(), ld_rowvec=rv.stride(0))
        keep.append(rv)
    desc = ops.gemm_desc(**kw)
    stats = None
    if d.colstats:
        rows, slots = env.lib.udt_gemm_colstats_rows(C.byref(desc)), env.lib.udt_gemm_colstats_slots(C.byref(desc))
        assert p.stats is not None and (rows, slots) == p.stats[:2], (rows, slots, p.stats)
        stats = torch.full((slots + 1, d.N, 2), K.MARKER, dtype=f32, device=env.dev)
        desc.colstats = stats.data_ptr()
    _, tags = env.traced(lambda: ops.run_gemm(desc, env.dev, fused_gn=d.in_scsh))
    ops.check_async_errors()
    return out, o_full, stats, tags


def _case(env, name, c, variant):
    p = K.predict(c, env.cus)
    t = K.inputs(c, variant)
    dev_t = {k: v.to(env.dev) for k, v in t.items()}
    exp = K.reference(c, dev_t, env.dev)
    try:
        for key, v in p.d.knobs.items():
            assert env.lib.udt_debug_set(key.encode(), v) == 0
        out, o_full, stats, tags = _launch(env, c, p, t)
        # the launch's own tag names the plan: a later change of a plan cannot silently move this case to another kernel
        assert tags == [p.tag], (tags, p.tag)
        out2, o_full2, stats2, _ = _launch(env, c, p, t)
    finally:
        env.reset_knobs()
    name = f"edge {name} [{p.tag.split(' ')[0]}]"
    got = out.reshape(exp[0].shape) if c["kind"] == "conv" else out
    K.hold(name, c, p, got, exp, t, report=REPORT)
    if c.get("trans"):
        assert bool((o_full[-1] == K.MARKER).all()), f"{name}: elements past the result were written"
    else:
        _guards_ok(o_full, out.shape, name)
    assert torch.equal(o_full, o_full2), f"{name}: not deterministic"
    if stats is not None:
        rows, slots, _ = p.stats
        slot, _ = K.stats_slot_of_row(c, p)
        stored = out.reshape(p.d.M, p.d.N).float()
        ref, ab = R.colstats_ref(stored, slot.to(env.dev), slots)
        S.check_fp32_sum(name + " stats", stats[:slots], ref, ab, report=REPORT)           # (slots past M: sum|summands| = 0 -> exactly zero)
        assert bool((stats[slots:] == K.MARKER).all()), f"{name}: statistics past the last slot were written"
        assert torch.equal(stats, stats2), f"{name}: statistics not deterministic"


def _ids(lst):
    return [K._name(c) for c in lst]


@pytest.mark.parametrize("c", K.LEAN_GEMM, ids=_ids(K.LEAN_GEMM))
def test_lean_gemm_edges(env, c):
    _case(env, K._name(c), c, "randn")


@pytest.mark.parametrize("c", K.LEAN_CONV1, ids=_ids(K.LEAN_CONV1))
def test_lean_conv1x1_edges(env, c):
    _case(env, K._name(c), c, "randn")


@pytest.mark.parametrize("c", K.GEMM8, ids=_ids(K.GEMM8))
def test_gemm8_edges(env, c):
    _case(env, K._name(c), c, "randn")


@pytest.mark.parametrize("c", K.GEN1, ids=_ids(K.GEN1))
def test_first_generation_edges(env, c):
    _case(env, K._name(c), c, "randn")


@pytest.mark.parametrize("c", K.CONV_N4, ids=_ids(K.CONV_N4))
def test_conv_n4_edges(env, c):
    _case(env, K._name(c), c, "randn")


@pytest.mark.parametrize("c", K.LCONV, ids=_ids(K.LCONV))
def test_lean_and_wide_conv3_edges(env, c):
    _case(env, K._name(c), c, "randn")


@pytest.mark.parametrize("c", K.CONV3P, ids=_ids(K.CONV3P))
def test_conv3p_gn_edges(env, c):
    _case(env, K._name(c), c, "randn")


@pytest.mark.parametrize("variant", K.GEMM_VARIANTS)
@pytest.mark.parametrize("c", K.GEMM_VARIANT_CASES, ids=_ids(K.GEMM_VARIANT_CASES))
def test_gemm_hostile_values(env, c, variant):
    _case(env, f"{variant} {K._name(c)}", c, variant)


@pytest.mark.parametrize("variant", K.CONV_VARIANTS)
@pytest.mark.parametrize("c", K.CONV_VARIANT_CASES, ids=_ids(K.CONV_VARIANT_CASES))
def test_conv_hostile_values(env, c, variant):
    _case(env, f"{variant} {K._name(c)}", c, variant)
