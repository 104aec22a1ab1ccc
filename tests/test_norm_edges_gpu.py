"""The forward normalisation kernels (csrc/norm.hip) at the edges no other value test launches (``pytest -m gpu``): both thread layouts of
gn_stats_kernel with idle row groups, an empty trailing chunk and the chunk-count clamps, gn_apply_kernel from partials and from the
udt_gn_finalize table over prefetching, tail-only and mixed spans, gn_strip_kernel at gw 8 / 4 / 2 / 1 on either side of its 64 KiB
admission limit with and without statistics records, gn_finalize_kernel with fewer and more records than slot lanes, and
layernorm_kernel<1..8> — each bf16 result held group by group and work unit by work unit to a float64 reference by tests/sliced_check.py
with its recorded margins, the bounds from tests/norm_ref.py's one bf16 rounding of the float64 result (never from the kernel's output),
the fp32 partials and tables element-wise by check_fp32_sum, every launch's profiler tag asserted against tests/norm_cases.py's mirror of
the launchers, and every launch repeated bit for bit.
Inputs and checks: tests/norm_cases.py, the same ones tests/test_norm_ref_cpu.py shows a float32 CPU restatement to pass.
One line per check goes to norm_edges_report.txt next to the run's parity report (tests/test_backward_gpu.py REPORT);
profiles/norm_edges_report.txt is a passing run's.
"""
import os
import tempfile

import pytest
import torch

import norm_cases as K
import sliced_check as S
import test_backward_gpu

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(test_backward_gpu.REPORT), "norm_edges_report.txt")         # a file of its own, same directory
G = K.G
MARKER = 7.0                                                                                     # pre-fills the fp32 partials


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
            path = os.path.join(tempfile.gettempdir(), "udt_norm_edges_trace.csv")
            Env.lib.udt_prof_dump(path.encode())
            Env.lib.udt_prof_trace(0)
            return out, [ln.split(",", 2)[2] for ln in open(path).read().splitlines()[1:]]

        @staticmethod
        def launch(strip, fn, tags, what):
            """fn() under ops.GN_STRIP = strip, traced, then once more: the tags are ``tags`` and the two results are bit-identical"""
            prev = ops.GN_STRIP
            try:
                ops.GN_STRIP = strip
                out, got = Env.traced(fn)
                again = fn()
            finally:
                ops.GN_STRIP = prev
            assert got == tags, f"{what}: launched {got}, the mirror predicts {tags}"
            assert torch.equal(out, again), f"{what}: not deterministic"
            return out
    Env.ops, Env.L, Env.lib, Env.dev = ops, lib, lib.load(), cuda
    return Env


def _bf(t):
    return None if t is None else t.bfloat16().contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _two_kernel_impl(env, shape, strip):
    B, HW, C1, C2 = shape

    def impl(x, x2, gamma, beta, eps, act, n):
        xb, x2b = _bf(x), _bf(x2)
        assert env.lib.udt_gn_nchunks(HW, C1 + C2) == n
        y = env.launch(strip, lambda: env.ops.group_norm(xb, gamma, beta, G, eps, bool(act), x2=x2b), K.tags_two_kernel(*shape), str(shape))

        def stats():
            part = torch.full((B, n, G, 2), MARKER, dtype=torch.float32, device=env.dev)
            env.L.check(env.lib.udt_gn_stats(_ptr(xb), _ptr(x2b), _ptr(part), B, HW, C1, C2, G, torch.cuda.current_stream().cuda_stream),
                        "udt_gn_stats")
            return part
        part = stats()
        assert torch.equal(part, stats()), f"{shape}: udt_gn_stats is not deterministic"
        return y, part
    return impl


@pytest.mark.parametrize("shape", K.TWO_KERNEL)
def test_group_norm_two_kernel_edges(env, shape):
    for variant, eps, act in K.VARIANTS:
        K.case_two_kernel(shape, variant, eps, act, _two_kernel_impl(env, shape, False), dev=env.dev, report=REPORT)


@pytest.mark.parametrize("shape", K.STRIP_REFUSED)
def test_group_norm_one_pixel_past_the_strip_limit_runs_as_two_kernels(env, shape):
    assert env.lib.udt_gn_strip_ok(*shape, G) == 0 and env.lib.udt_gn_strip_ok(shape[0], shape[1] - 1, shape[2], shape[3], G) == 1
    for variant, eps, act in K.VARIANTS:
        K.case_two_kernel(shape, variant, eps, act, _two_kernel_impl(env, shape, True), dev=env.dev, report=REPORT)


@pytest.mark.parametrize("shape", K.STRIP)
def test_group_norm_strip_edges(env, shape):
    assert env.lib.udt_gn_strip_ok(*shape, G) == 1

    def impl(x, x2, gamma, beta, eps, act, gw):
        xb, x2b = _bf(x), _bf(x2)
        return env.launch(True, lambda: env.ops.group_norm(xb, gamma, beta, G, eps, bool(act), x2=x2b), K.tags_strip(*shape, gw), str(shape))
    for variant, eps, act in K.VARIANTS:
        K.case_strip(shape, variant, eps, act, impl, dev=env.dev, report=REPORT)


@pytest.mark.parametrize("form,shape,slots1,slots2", [("strip",) + c for c in K.REC_STRIP] + [("table",) + c for c in K.REC_TABLE])
def test_group_norm_from_records_edges(env, form, shape, slots1, slots2):
    B, HW, C1, C2 = shape
    ops = env.ops

    def impl(x, x2, rec1, s1, rec2, s2, gamma, beta, eps, act):
        xb, x2b = _bf(x), _bf(x2)
        st1, st2 = ops.GnStats(rec1, s1), (ops.GnStats(rec2, s2) if rec2 is not None else None)
        run = lambda: ops.group_norm_from_stats(xb, st1, gamma, beta, G, eps, bool(act), x2=x2b, st2=st2)
        if form == "strip":
            return env.launch(True, run, K.tags_strip(*shape, K.STRIP_GW[shape], records=True), str(shape)), None
        y = env.launch(False, run, K.tags_table(*shape, s1), str(shape))
        table = env.launch(False, lambda: ops.gn_finalize(st1, C1, st2, C2, gamma, beta, B, HW, G, eps), K.tags_table(*shape, s1)[:1],
                           str(shape))
        return y, table
    for variant, eps, act in K.VARIANTS:
        K.case_records(form, shape, slots1, slots2, variant, eps, act, impl, dev=env.dev, report=REPORT)


@pytest.mark.parametrize("C", K.LN_C)
def test_layer_norm_edges(env, C):
    def impl(x, gamma, beta, eps):
        xb = _bf(x)
        # udt_layernorm tags nothing: one untagged launch
        return env.launch(env.ops.GN_STRIP, lambda: env.ops.layer_norm(xb, gamma, beta, eps), [""], f"layernorm C{C}")
    for rows in K.LN_ROWS:
        for variant, eps in K.LN_VARIANTS:
            K.case_ln(rows, C, variant, eps, impl, dev=env.dev, report=REPORT)


def test_norm_mirrors_match_the_library(env):
    for hw in list(range(1, 70)) + [255, 256, 257, 289, 819, 820, 2047, 2048, 2049, 2100, 4096, 16384]:
        assert env.lib.udt_gn_nchunks(hw, 320) == K.gn_nchunks(hw), hw
    shapes = [s[1:] for s in K.TWO_KERNEL + K.STRIP + K.STRIP_REFUSED] + [s[1:] for s, _, _ in K.REC_STRIP + K.REC_TABLE]
    shapes += [(hw, c1, c2) for hw in (1, 64, 102, 103, 256, 1024, 4096) for c1, c2 in ((32, 0), (128, 0), (320, 320), (960, 320), (1280, 1280),
                                                                                       (96, 4), (8256, 0), (48, 0))]
    for hw, c1, c2 in shapes:
        assert env.lib.udt_gn_strip_ok(1, hw, c1, c2, G) == (1 if K.gn_strip_groups(hw, c1, c2) else 0), (hw, c1, c2)
    assert S.FP32_SUM_UNITS == 16.0 and (S.MIN_SLICE, S.ULP_ALLOWANCE) == (1024, 2.0 ** -18)
