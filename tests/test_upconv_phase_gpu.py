"""The phase form of the upsampling convolutions (csrc/lean.h lconv3_kernel / csrc/wide.h wconv3_kernel PHASE: nearest x2 upsample
+ conv3x3 as four 2x2 phase convolutions of the low-resolution map on packing.pack_conv_up4 weights) against the float64 reference
built from the SAME bf16 3x3 weights, and against the nine-tap instance (udt_gemm_desc.upsample = 1) it replaces, run on the same
inputs.  ``pytest -m gpu``.

Bounds.  Every element within test_ops_gpu._close (rtol 1.5e-2, atol 2e-2).  The relative RMS error against float64 at most 1.5x
that of the nine-tap instance: the phase weights are fp32 sums of bf16 taps rounded once more to bf16 (relative RMS 2^-9 / sqrt(3)
per weight, ~1.6e-3 on the output) beside the one bf16 rounding of the output both instances share (~1.7e-3): sqrt(2) expected.
The measured ratios are printed (profiles/upconv_phase_parity.txt).

Reference op: Upsample.forward of sgm/modules/diffusionmodules/openaimodel.py:99-101 / model.py:64-68."""
import math
import os
import tempfile

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1.5e-2, 2e-2            # test_ops_gpu._close
RATIO = 1.5
F64 = torch.float64


def _close(got, ref, what=""):
    err = (got.to(F64) - ref).abs()
    bad = (err > ATOL + RTOL * ref.abs()).sum().item()
    assert bad == 0, f"{what}: {bad}/{err.numel()} off, max err {err.max().item():.4g} (ref max {ref.abs().max().item():.4g})"


def _rel(got, ref):
    return ((got.to(F64) - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib as L, ops as O, packing as P
    lib = L.load()
    assert lib.udt_device_arch_ok() == 1, "tests expect a gfx950 device"

    class Env:
        ops, packing = O, P

        @staticmethod
        def dbg(key, val):
            L.check(lib.udt_debug_set(key.encode(), int(val)), "udt_debug_set " + key)

        @staticmethod
        def reset():
            for k in ("lean_splitk", "wide_conv"):
                L.check(lib.udt_debug_set(k.encode(), -1), "udt_debug_set " + k)

        @staticmethod
        def traced(fn):
            """(fn(), the tags of the launches it made in the library's profiler: 'lconv3+up ... up4' (lean phase form) / 'lconv3+up ...' (nine taps) /
            'wconv3 ... up4' (wide phase form))"""
            O.prof_reset(); lib.udt_prof_trace(1); O.prof_enable(0x3f)
            try:
                out = fn()
                torch.cuda.synchronize()
            finally:
                O.prof_enable(0)
            path = os.path.join(tempfile.gettempdir(), "udt_upconv_phase_trace.csv")
            lib.udt_prof_dump(path.encode())
            lib.udt_prof_trace(0)
            return out, [ln.split(",", 2)[2] for ln in open(path).read().splitlines()[1:]]
    yield Env
    Env.reset()


_DATA = {}


def _data(env, dev, B, H, W, C, N, bias, border=False, seed=41):
    """inputs, both weight layouts and the float64 reference of one case: built once, shared, never modified"""
    key = (B, H, W, C, N, bias, border)
    if key not in _DATA:
        g = torch.Generator(device="cpu").manual_seed(seed + 7 * len(_DATA))
        x = torch.randn((B, H, W, C), generator=g)
        if border:
            m = torch.zeros((1, H, W, 1))
            m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = 1, 1, 1, 1
            x = x * m
        x = x.to(dev).bfloat16()
        w4 = (torch.randn((N, C, 3, 3), generator=g) / math.sqrt(9 * C)).to(dev)
        w4 = w4 * (1.0 + torch.arange(N, device=dev)[:, None, None, None] / N)            # asymmetric in the output channel
        b = torch.randn((N,), generator=g).to(dev) if bias else None
        up = F.interpolate(x.to(F64).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
        ref = F.conv2d(up, w4.bfloat16().to(F64), b.to(F64) if bias else None, padding=1).permute(0, 2, 3, 1).contiguous()
        _DATA[key] = (x, env.packing.pack_conv(w4), env.packing.pack_conv_up4(w4), b, ref)
    return _DATA[key]


def _both(env, x, w, w4, b, **kw):
    """(phase result, its tag, nine-tap result, its tag)"""
    out, tags = env.traced(lambda: env.ops.conv2d(x, w, b, ksize=3, upsample=True, w_up4=w4, **kw))
    par, ptags = env.traced(lambda: env.ops.conv2d(x, w, b, ksize=3, upsample=True, **kw))
    assert len(tags) == 1 and len(ptags) == 1, (tags, ptags)
    return out, tags[0], par, ptags[0]


def _check(what, out, par, ref):
    e, ep = _rel(out, ref), _rel(par, ref)
    print(f"upconv_phase parity: {what}: rel rms phase {e:.4e} nine-tap {ep:.4e} ratio {e / ep:.3f}")
    _close(out, ref, what)
    _close(par, ref, what + " (nine-tap instance)")
    assert e <= RATIO * ep, f"{what}: rel rms {e:.3e} > {RATIO} x {ep:.3e} of the nine-tap instance"


def _lean_phase(tag):
    return tag.startswith("lconv3+up ") and tag.endswith(" up4")


def _nine_tap(tag):
    return tag.startswith("lconv3+up ") and "up4" not in tag


def _wide_phase(tag):
    return tag.startswith("wconv3 ") and tag.endswith(" up4")


def _splitk(tag):
    return int(tag.split("splitk=")[1].split()[0])


def _check_stats(what, env, st_out, B):
    """the emitted column sums against the sums of the stored bf16 output, within the shadow's statistics bound (shadow_ref.check_colstats)"""
    st = env.ops.gn_stats_of(st_out)
    assert st is not None, f"{what}: no statistics emitted"
    N = st_out.shape[-1]
    o = st_out.to(F64).reshape(B, -1, N)
    n = o.shape[1]
    assert st.data.shape[0] == B * st.slots_per_sample
    s = st.data.to(F64).reshape(B, st.slots_per_sample, N, 2).sum(dim=1)
    r1, r2 = o.sum(dim=1), o.pow(2).sum(dim=1)
    e1 = ((s[..., 0] - r1).abs() / (2e-3 * math.sqrt(n) * r2.div(n).sqrt() + 2e-3 * r1.abs() + 1e-30)).max().item()
    e2 = ((s[..., 1] - r2).abs() / (2e-3 * r2 + 1e-30)).max().item()
    assert max(e1, e2) <= 1.0, f"{what}: column statistics off x{max(e1, e2):.2f}"


def test_8x8_geometry_one_chunk(env, cuda):
    B, H, W, C, N = 2, 8, 8, 64, 128
    x, w, w4, b, ref = _data(env, cuda, B, H, W, C, N, False)
    out, tag, par, ptag = _both(env, x, w, w4, b)
    assert _lean_phase(tag) and "tile=8x8" in tag and _splitk(tag) == 1, tag
    assert _nine_tap(ptag), ptag
    _check("8x8 B=2 C=64 N=128", out, par, ref)
    st_out, _ = env.traced(lambda: env.ops.conv2d(x, w, b, ksize=3, upsample=True, w_up4=w4, colstats=True))
    assert torch.equal(st_out, out)
    _check_stats("8x8 statistics", env, st_out, B)


def test_16x8_geometry_two_chunks_n_tail_bias(env, cuda):
    B, H, W, C, N = 1, 8, 16, 128, 192
    x, w, w4, b, ref = _data(env, cuda, B, H, W, C, N, True)
    out, tag, par, ptag = _both(env, x, w, w4, b)
    assert _lean_phase(tag) and "tile=16x8" in tag, tag
    assert _nine_tap(ptag), ptag
    _check("16x8 B=1 8x16 C=128 N=192 bias", out, par, ref)
    st_out, _ = env.traced(lambda: env.ops.conv2d(x, w, b, ksize=3, upsample=True, w_up4=w4, colstats=True))
    assert torch.equal(st_out, out)
    _check_stats("16x8 statistics", env, st_out, B)


def test_16x8_border_only_input(env, cuda):
    B, H, W, C, N = 1, 8, 16, 128, 192
    x, w, w4, b, ref = _data(env, cuda, B, H, W, C, N, True, border=True)
    assert x[:, 1:-1, 1:-1].abs().max().item() == 0 and x.abs().max().item() > 0
    out, tag, par, _ = _both(env, x, w, w4, b)
    assert _lean_phase(tag), tag
    _check("16x8 border-only input", out, par, ref)


def test_slices_and_ticket_bit_identical(env, cuda):
    B, H, W, C, N = 1, 8, 8, 1280, 128
    x, w, w4, b, ref = _data(env, cuda, B, H, W, C, N, False)
    out, tag, par, _ = _both(env, x, w, w4, b)
    assert _lean_phase(tag) and _splitk(tag) > 1, tag
    again = env.ops.conv2d(x, w, b, ksize=3, upsample=True, w_up4=w4)
    torch.cuda.synchronize()
    assert torch.equal(out, again), "the sliced phase convolution changed bits between two launches"
    _check("slices B=1 8x8 C=1280 N=128", out, par, ref)


@pytest.mark.parametrize("C", [128, 1280])
def test_wide_instance_forced(env, cuda, C):
    B, H, W, N = 1, 16, 16, 160
    x, w, w4, b, ref = _data(env, cuda, B, H, W, C, N, False)
    try:
        env.dbg("wide_conv", 1)
        out, tag = env.traced(lambda: env.ops.conv2d(x, w, b, ksize=3, upsample=True, w_up4=w4))
        again = env.ops.conv2d(x, w, b, ksize=3, upsample=True, w_up4=w4)
        st_out = env.ops.conv2d(x, w, b, ksize=3, upsample=True, w_up4=w4, colstats=True)
        torch.cuda.synchronize()
    finally:
        env.reset()
    par, ptag = env.traced(lambda: env.ops.conv2d(x, w, b, ksize=3, upsample=True))
    assert len(tag) == 1 and _wide_phase(tag[0]) and "tile=16x16" in tag[0], tag
    assert _nine_tap(ptag[0]), ptag
    if C == 1280:
        assert _splitk(tag[0]) > 1, tag
    assert torch.equal(out, again) and torch.equal(out, st_out)
    _check(f"wide B=1 16x16 C={C} N=160", out, par, ref)
    _check_stats(f"wide statistics C={C}", env, st_out, B)


def test_unserved_shape_takes_the_nine_tap_path_unchanged(env, cuda):
    """a map the patch-staged kernels do not tile (12 x 12 -> 24 x 24), N = 320: the gathered convolution, with or without the layout"""
    B, H, W, C, N = 1, 12, 12, 64, 320
    x, w, w4, b, ref = _data(env, cuda, B, H, W, C, N, True)
    out, tag, par, ptag = _both(env, x, w, w4, b)
    assert "up4" not in tag and tag == ptag, (tag, ptag)
    assert torch.equal(out, par)
    _close(out, ref, "unserved 12x12 N=320")


def test_module_forward_takes_the_phase_form_and_keeps_the_flop_count(env, cuda):
    """hipnn.Conv2d.forward(upsample=True) passes its cached up4 layout; the work counter keeps the reference formulation's nine taps"""
    from sgm.modules import hipnn as H
    B, Hh, Ww, C, N = 2, 8, 8, 64, 128
    conv = H.Conv2d(C, N, 3, padding=1).to(cuda)
    g = torch.Generator(device="cpu").manual_seed(77)
    x = torch.randn((B, Hh, Ww, C), generator=g).to(cuda).bfloat16()
    env.ops.WORK_COUNTER = {}
    try:
        with torch.no_grad():
            out, tags = env.traced(lambda: conv(x, upsample=True))
        flops = env.ops.WORK_COUNTER.get("conv3x3")
    finally:
        env.ops.WORK_COUNTER = None
    assert len(tags) == 1 and _lean_phase(tags[0]), tags
    assert H.has_layout(conv, "up4")
    assert flops == 2.0 * B * 4 * Hh * Ww * N * C * 9
    up = F.interpolate(x.to(F64).permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    ref = F.conv2d(up, conv.weight.detach().bfloat16().to(F64), conv.bias.detach().to(F64), padding=1).permute(0, 2, 3, 1)
    _close(out, ref, "Conv2d.forward(upsample=True)")
