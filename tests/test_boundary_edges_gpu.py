"""The plugin-boundary kernels (csrc/elementwise.hip: layout, embedding, latent sampling, mask, local loss; udt_local_loss_tiled_hw of
csrc/backward.hip) and the device packers (csrc/pack.hip) at the edges no other value test launches (``pytest -m gpu``), through the C
ABI: odd sizes, sizes that are no multiple of a workgroup, one element, rectangular masks, padded leading dimensions with poisoned
padding, every special fp32 value.  Results that are one correctly rounded fp32 operation and one round-to-nearest-even conversion are
compared as integers with tests/boundary_ref.py; udt_posterior_sample, udt_timestep_embedding and the local loss are held to float64
with the bounds tests/boundary_cases.py records (from the CPU, never from a result here).  Every launch writes into a buffer with
markers before and after it, which must survive, and is made twice with bit-identical results; every documented refusal returns its
code and writes nothing.
Inputs and checks: tests/boundary_cases.py, the same ones tests/test_boundary_ref_cpu.py shows a float32 CPU restatement to pass.
One line per check goes to boundary_edges_report.txt next to the run's parity report (tests/test_backward_gpu.py REPORT);
profiles/boundary_edges_report.txt is a passing run's.
"""
import ctypes as C
import os

import pytest
import torch

import boundary_cases as K
import boundary_ref as R
import sliced_check as S
import test_backward_gpu
from test_ops_gpu import _packed_tensor

pytestmark = pytest.mark.gpu
REPORT = os.path.join(os.path.dirname(test_backward_gpu.REPORT), "boundary_edges_report.txt")
GUARD = 64                                             # marker elements before and after every output (keeps 16-byte alignment)
MARKER = -7.0
BAD_SHAPE, BAD_ARG = -1, -2


class Guarded:
    """a tensor of ``shape`` with GUARD marker elements on either side of it in the same allocation"""

    def __init__(self, shape, dtype, dev, init=None):
        n = 1
        for s in shape:
            n *= s
        self.full = torch.full((n + 2 * GUARD,), MARKER, dtype=dtype, device=dev)
        self.t = self.full[GUARD:GUARD + n].view(shape)
        if init is not None:
            self.t.copy_(init)

    def ptr(self):
        return self.t.data_ptr()

    def result(self, what):
        """the tensor on the CPU, after checking the markers"""
        torch.cuda.synchronize()
        m = torch.full((GUARD,), MARKER, dtype=self.full.dtype)
        assert torch.equal(self.full[:GUARD].cpu(), m) and torch.equal(self.full[-GUARD:].cpu(), m), f"{what}: wrote outside its output"
        return self.t.cpu().clone()

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.full == MARKER).all())


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def twice(once, what):
    """once() launches into fresh buffers and returns CPU tensors: two calls must agree bit for bit"""
    a, b = once(), once()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: not deterministic"
    return a


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)
    S._report(f"units: posterior_sample U = {K.U_POSTERIOR:g} (4 x {K.POSTERIOR_MEASURED} measured on the CPU), timestep_embedding U = "
              f"{K.U_TIMESTEP:g} (4 x {K.TIMESTEP_MEASURED}); local loss and real-valued mask: {S.FP32_SUM_UNITS:g}", REPORT)

    class Env:
        @staticmethod
        def st():
            return torch.cuda.current_stream().cuda_stream

        @staticmethod
        def ok(rc, what):
            assert rc == 0, f"{what}: status {rc}"
    Env.L, Env.lib, Env.dev = lib, lib.load(), cuda
    return Env


# ------------------------------------------------------------------------------------------------ layout kernels
@pytest.mark.parametrize("shape", K.NCHW_TO_NHWC)
def test_nchw_to_nhwc_edges(env, shape):
    def impl(x, cpad, scale):
        B, C, HW = x.shape
        xd = x.to(env.dev)

        def once():
            y = Guarded((B, HW, cpad), torch.bfloat16, env.dev)
            env.ok(env.lib.udt_nchw_to_nhwc(xd.data_ptr(), y.ptr(), B, C, HW, cpad, scale, env.st()), "udt_nchw_to_nhwc")
            return y.result(f"nchw_to_nhwc {shape}")
        return twice(once, f"nchw_to_nhwc {shape}")
    for scale in K.SCALES:
        K.case_nchw_to_nhwc(shape, scale, impl, report=REPORT)


@pytest.mark.parametrize("shape", K.NHWC_TO_NCHW)
def test_nhwc_to_nchw_edges(env, shape):
    def impl(src, Cc):
        B, HW, ld = src.shape
        sd = src.to(env.dev)

        def once():
            y = Guarded((B, Cc, HW), torch.float32, env.dev)
            env.ok(env.lib.udt_nhwc_to_nchw(sd.data_ptr(), y.ptr(), B, Cc, HW, ld, int(src.dtype == torch.float32), env.st()), "udt_nhwc_to_nchw")
            return y.result(f"nhwc_to_nchw {shape}")
        return twice(once, f"nhwc_to_nchw {shape}")
    for f32 in (True, False):
        K.case_nhwc_to_nchw(shape, f32, impl, report=REPORT)


@pytest.mark.parametrize("spec", K.SET_CHANNELS)
def test_nhwc_set_channels_edges(env, spec):
    def impl(src, dst, c0):
        B, Cc, HW = src.shape
        sd = src.to(env.dev)

        def once():
            y = Guarded(tuple(dst.shape), torch.bfloat16, env.dev, init=dst)
            env.ok(env.lib.udt_nhwc_set_channels(sd.data_ptr(), y.ptr(), B, Cc, HW, dst.shape[2], c0, env.st()), "udt_nhwc_set_channels")
            return y.result(f"set_channels {spec}")
        return twice(once, f"set_channels {spec}")
    for hw in K.SET_HW:
        K.case_set_channels(spec, hw, impl, report=REPORT)


@pytest.mark.parametrize("shape", K.EMBED)
def test_embed_tokens_edges(env, shape):
    def impl(idx, table, pe):
        i, t, p = idx.to(env.dev), table.to(env.dev), pe.to(env.dev)

        def once():
            y = Guarded((idx.shape[0], pe.shape[1]), torch.bfloat16, env.dev)
            env.ok(env.lib.udt_embed_tokens(i.data_ptr(), t.data_ptr(), p.data_ptr(), y.ptr(), idx.shape[0], pe.shape[0], pe.shape[1], env.st()),
                   "udt_embed_tokens")
            return y.result(f"embed_tokens {shape}")
        return twice(once, f"embed_tokens {shape}")
    K.case_embed(shape, impl, report=REPORT)


def test_add_and_bias_add_edges(env):
    def add(a, b):
        bd = b.to(env.dev)

        def once():
            x = Guarded(tuple(a.shape), torch.bfloat16, env.dev, init=a)
            env.ok(env.lib.udt_add_bf16(x.ptr(), bd.data_ptr(), a.numel(), env.st()), "udt_add_bf16")
            return x.result("add_bf16")
        return twice(once, "add_bf16")

    def bias_add(x, bias, inplace):
        rows, Cc = x.shape
        bd, xd = bias.to(env.dev), x.to(env.dev)

        def once():
            y = Guarded((rows, Cc), torch.bfloat16, env.dev, init=x if inplace else None)
            env.ok(env.lib.udt_bias_add_bf16(y.ptr() if inplace else xd.data_ptr(), bd.data_ptr(), y.ptr(), rows, Cc, env.st()), "udt_bias_add_bf16")
            return y.result("bias_add_bf16")
        got = twice(once, "bias_add_bf16")
        assert torch.equal(_bits(xd.cpu()), _bits(x))                             # the out-of-place source is read only
        return got
    for n in K.ADD_N:
        K.case_add(n, add, report=REPORT)
    for shape in K.BIAS_ADD:
        for inplace in (False, True):
            K.case_bias_add(shape, inplace, bias_add, report=REPORT)


@pytest.mark.parametrize("shape", K.MASK)
def test_mask_downsample_edges(env, shape):
    B, H, W = shape

    def impl(m):
        md = m.to(env.dev)

        def once():
            y = Guarded((B, H // 8, W // 8), torch.float32, env.dev)
            env.ok(env.lib.udt_mask_downsample(md.data_ptr(), y.ptr(), B, H, W, env.st()), "udt_mask_downsample")
            return y.result(f"mask_downsample {shape}")
        return twice(once, f"mask_downsample {shape}")
    assert K.case_mask_downsample(shape, impl, report=REPORT) <= S.FP32_SUM_UNITS


# ------------------------------------------------------------------------------------------------ kernels with a bound
@pytest.mark.parametrize("shape", K.POSTERIOR)
def test_posterior_sample_edges(env, shape):
    B, hw = shape

    def impl(mom, noise, scale):
        md, nd = mom.to(env.dev), noise.to(env.dev)

        def once():
            z = Guarded((B, 4, hw), torch.float32, env.dev)
            env.ok(env.lib.udt_posterior_sample(md.data_ptr(), nd.data_ptr(), z.ptr(), B, hw, mom.shape[2], scale, env.st()), "udt_posterior_sample")
            return z.result(f"posterior_sample {shape}")
        return twice(once, f"posterior_sample {shape}")
    for ldm in K.POSTERIOR_LDM:
        for scale in K.POSTERIOR_SCALES:
            w = K.case_posterior(shape, ldm, scale, impl, report=REPORT)
            print(f"posterior_sample {shape} ldm {ldm} scale {scale}: worst {w:.2f} x 2^-24 of U = {K.U_POSTERIOR:g}")


@pytest.mark.parametrize("dim", K.TIMESTEP_DIM)
def test_timestep_embedding_edges(env, dim):
    def impl(t, d):
        td = t.to(env.dev)

        def once():
            y = Guarded((t.shape[0], d), torch.bfloat16, env.dev)
            env.ok(env.lib.udt_timestep_embedding(td.data_ptr(), y.ptr(), t.shape[0], d, env.st()), "udt_timestep_embedding")
            return y.result(f"timestep_embedding dim {d}")
        return twice(once, f"timestep_embedding dim {d}")
    for n in K.TIMESTEP_N:
        w = K.case_timestep(n, dim, impl, report=REPORT)
        print(f"timestep_embedding n {n} dim {dim}: needs {w:.2f} x 2^-24 of U = {K.U_TIMESTEP:g}")


def _local_loss_call(env, entry, ptrs, loss, scratch, n_samples, mask_batch, heads, size, L, seg_l, Hm, Wm):
    lib = env.lib
    if entry == "udt_local_loss":
        return lib.udt_local_loss(*ptrs, loss, n_samples, heads, size, L, seg_l, Hm, Wm, env.st())
    if entry == "udt_local_loss_tiled":
        return lib.udt_local_loss_tiled(*ptrs, loss, n_samples, mask_batch, heads, size, L, seg_l, Hm, Wm, env.st())
    return lib.udt_local_loss_tiled_hw(*ptrs, loss, scratch, n_samples, mask_batch, heads, size, size, L, seg_l, Hm, Wm, env.st())


def _local_loss_impl(env, entry, case):
    def impl(probs, mask, seg, gk, loss0, mask_batch, heads, size):
        n_samples, L, seg_l, Hm, Wm = probs.shape[0] // heads, probs.shape[2], seg.shape[1], mask.shape[1], mask.shape[2]
        dev = [t.to(env.dev) for t in (probs, mask, seg, gk)]

        def once():
            loss = Guarded((n_samples,), torch.float32, env.dev, init=loss0)
            scratch = Guarded((n_samples * seg_l * 2,), torch.float32, env.dev)
            env.ok(_local_loss_call(env, entry, [t.data_ptr() for t in dev], loss.ptr(), scratch.ptr(), n_samples, mask_batch, heads, size, L,
                                    seg_l, Hm, Wm), entry)
            scratch.result(f"{entry} scratch {case}")
            return loss.result(f"{entry} {case}")
        return twice(once, f"{entry} {case}")
    return impl


@pytest.mark.parametrize("case", K.LOCAL_LOSS)
def test_local_loss_edges(env, case):
    n_samples, mask_batch = case[6], case[7]
    got = {}
    for entry in ("udt_local_loss_tiled", "udt_local_loss_tiled_hw") + (("udt_local_loss",) if n_samples == mask_batch else ()):
        def impl(*a, entry=entry):
            got[entry] = _local_loss_impl(env, entry, case)(*a)
            return got[entry]
        assert K.case_local_loss(case, impl, report=REPORT, what=entry[len("udt_local_loss"):]) <= S.FP32_SUM_UNITS
    assert torch.equal(_bits(got["udt_local_loss_tiled_hw"]), _bits(got["udt_local_loss_tiled"])), "_tiled_hw is not bit-equal to _tiled at h == w"
    if "udt_local_loss" in got:
        assert torch.equal(_bits(got["udt_local_loss"]), _bits(got["udt_local_loss_tiled"]))


def test_local_loss_refuses_size_121(env):
    size, heads, L = K.LOCAL_LOSS_REFUSED_SIZE, 1, 2
    probs = torch.full((heads, size * size, L), 0.5, device=env.dev)
    mask, seg, gk = torch.ones((1, 8, 8), device=env.dev), torch.ones((1, L), device=env.dev), K.gauss9().to(env.dev)
    ptrs = [t.data_ptr() for t in (probs, mask, seg, gk)]
    for entry in ("udt_local_loss", "udt_local_loss_tiled", "udt_local_loss_tiled_hw"):
        loss, scratch = Guarded((1,), torch.float32, env.dev), Guarded((2 * L,), torch.float32, env.dev)
        assert _local_loss_call(env, entry, ptrs, loss.ptr(), scratch.ptr(), 1, 1, heads, size, L, L, 8, 8) == BAD_SHAPE, entry
        assert loss.untouched() and scratch.untouched(), entry
    S._report(f"{'edge local_loss size121':55s} refused by the three entry points, loss untouched", REPORT)


# ------------------------------------------------------------------------------------------------ packed weights
def _handle_out(env, h, fp8):
    lib = env.lib
    N, Npad, K_, Kpad, dtype = (lib.udt_packed_dim(h, i) for i in range(5))
    assert dtype == (env.L.DTYPE_FP8_E4M3 if fp8 else env.L.DTYPE_BF16)
    w = _packed_tensor(lib, h, "w", (Npad, Kpad), torch.uint8 if fp8 else torch.bfloat16).cpu()
    out = {"dims": (N, Npad, K_, Kpad), "weight": w.long() if fp8 else R.bf16_bits(w),
           "bias": _packed_tensor(lib, h, "b", (Npad,), torch.float32).cpu(),
           "colscale": _packed_tensor(lib, h, "s", (Npad,), torch.float32).cpu() if fp8 else None}
    assert fp8 or not lib.udt_packed_colscale(h)
    env.ok(lib.udt_free_packed(h), "udt_free_packed")
    return out


def _same_packed(a, b, what):
    assert a["dims"] == b["dims"] and torch.equal(a["weight"], b["weight"]) and torch.equal(_bits(a["bias"]), _bits(b["bias"])), what
    assert a["colscale"] is None or torch.equal(_bits(a["colscale"]), _bits(b["colscale"])), what


def _pack_linear_impl(env):
    def impl(w, bias, fp8, geglu):
        wd, bd = w.to(env.dev), None if bias is None else bias.to(env.dev)

        def once():
            h = C.c_void_p()
            env.ok(env.lib.udt_pack_linear(wd.data_ptr(), None if bd is None else bd.data_ptr(), w.shape[0], w.shape[1],
                                           env.L.DTYPE_FP8_E4M3 if fp8 else env.L.DTYPE_BF16, int(geglu), C.byref(h), env.st()), "udt_pack_linear")
            return _handle_out(env, h, fp8)
        a, b = once(), once()
        _same_packed(a, b, "udt_pack_linear: not deterministic")
        return a
    return impl


def _pack_conv_impl(env):
    def impl(w, bias, segments, n_pad_to):
        wd, bd = w.to(env.dev), None if bias is None else bias.to(env.dev)
        N, Cin, kh, kw = w.shape
        segs = (C.c_int32 * len(segments))(*segments) if segments else None

        def once():
            h = C.c_void_p()
            env.ok(env.lib.udt_pack_conv(wd.data_ptr(), None if bd is None else bd.data_ptr(), N, Cin, kh, kw, segs, len(segments or ()), n_pad_to,
                                         C.byref(h), env.st()), "udt_pack_conv")
            return _handle_out(env, h, False)
        a, b = once(), once()
        _same_packed(a, b, "udt_pack_conv: not deterministic")
        return a
    return impl


def test_pack_linear_edges(env):
    for case in K.linear_cases():
        K.case_pack_linear(*case, _pack_linear_impl(env), report=REPORT)


@pytest.mark.parametrize("segments", K.CONV_SEGMENTS)
def test_pack_conv_edges(env, segments):
    for case in K.conv_cases(segments):
        K.case_pack_conv(*case, _pack_conv_impl(env), report=REPORT)


# ------------------------------------------------------------------------------------------------ refusals
# entry -> (argument names, a valid call, [(changes, status)]); pointer arguments are named p_*: every one is a marker-filled buffer that
# must be unchanged afterwards (None = a null pointer).  The conditions are the launchers' checks in elementwise.hip / backward.hip.
def _nulls(names, code=BAD_ARG):
    return [({n: None}, code) for n in names]


def _nonpos(names, code=BAD_SHAPE):
    return [({n: v}, code) for n in names for v in (0, -1)]


REFUSALS = {
    "udt_posterior_sample": (("p_mom", "p_noise", "p_z", "B", "hw", "ldm", "scale"), dict(B=2, hw=5, ldm=8, scale=1.0),
                             _nulls(("p_mom", "p_noise", "p_z")) + _nonpos(("B", "hw")) + [({"ldm": 7}, BAD_SHAPE), ({"ldm": 4}, BAD_SHAPE)]),
    "udt_nchw_to_nhwc": (("p_x", "p_y", "B", "C", "HW", "cpad", "scale"), dict(B=2, C=4, HW=5, cpad=8, scale=1.0),
                         _nulls(("p_x", "p_y")) + _nonpos(("B", "C", "HW")) + [({"cpad": 12}, BAD_SHAPE), ({"C": 9}, BAD_SHAPE),
                                                                                ({"cpad": 4}, BAD_SHAPE), ({"cpad": 0}, BAD_SHAPE)]),
    "udt_nhwc_to_nchw": (("p_x", "p_y", "B", "C", "HW", "ld", "f32"), dict(B=2, C=4, HW=5, ld=8, f32=1),
                         _nulls(("p_x", "p_y")) + _nonpos(("B", "C", "HW")) + [({"ld": 3}, BAD_SHAPE)]),
    "udt_nhwc_set_channels": (("p_src", "p_dst", "B", "C", "HW", "cpad", "c0"), dict(B=2, C=3, HW=5, cpad=16, c0=5),
                              _nulls(("p_src", "p_dst")) + _nonpos(("B", "C", "HW")) + [({"c0": -1}, BAD_SHAPE), ({"c0": 14}, BAD_SHAPE),
                                                                                         ({"cpad": 7}, BAD_SHAPE)]),
    "udt_embed_tokens": (("p_idx", "p_table", "p_pe", "p_out", "n_tok", "L", "D"), dict(n_tok=4, L=2, D=6),
                         _nulls(("p_idx", "p_table", "p_pe", "p_out")) + _nonpos(("n_tok", "L", "D")) + [({"D": 7}, BAD_SHAPE), ({"D": 1}, BAD_SHAPE)]),
    "udt_timestep_embedding": (("p_t", "p_out", "n", "dim"), dict(n=4, dim=6),
                               _nulls(("p_t", "p_out")) + _nonpos(("n", "dim")) + [({"dim": 7}, BAD_SHAPE), ({"dim": 1}, BAD_SHAPE)]),
    "udt_mask_downsample": (("p_mask", "p_out", "B", "H", "W"), dict(B=2, H=16, W=8),
                            _nulls(("p_mask", "p_out")) + _nonpos(("B", "H", "W")) + [({"H": 12}, BAD_SHAPE), ({"W": 9}, BAD_SHAPE), ({"H": 7}, BAD_SHAPE)]),
    "udt_local_loss": (("p_probs", "p_mask", "p_seg", "p_gk", "p_loss", "B", "heads", "size", "L", "seg_l", "Hm", "Wm"),
                       dict(B=2, heads=2, size=3, L=4, seg_l=3, Hm=8, Wm=8),
                       _nulls(("p_probs", "p_mask", "p_seg", "p_gk", "p_loss")) + _nonpos(("B", "heads", "size", "L", "seg_l"))
                       + [({"size": 121}, BAD_SHAPE), ({"seg_l": 5}, BAD_SHAPE)]),
    "udt_local_loss_tiled": (("p_probs", "p_mask", "p_seg", "p_gk", "p_loss", "n_samples", "mask_batch", "heads", "size", "L", "seg_l", "Hm", "Wm"),
                             dict(n_samples=4, mask_batch=2, heads=2, size=3, L=4, seg_l=3, Hm=8, Wm=8),
                             _nulls(("p_probs", "p_mask", "p_seg", "p_gk", "p_loss")) + _nonpos(("n_samples", "mask_batch", "heads", "size", "L", "seg_l"))
                             + [({"size": 121}, BAD_SHAPE), ({"seg_l": 5}, BAD_SHAPE), ({"mask_batch": 3}, BAD_SHAPE)]),
    "udt_local_loss_tiled_hw": (("p_probs", "p_mask", "p_seg", "p_gk", "p_loss", "p_scratch", "n_samples", "mask_batch", "heads", "h", "w", "L",
                                 "seg_l", "Hm", "Wm"), dict(n_samples=4, mask_batch=2, heads=2, h=3, w=3, L=4, seg_l=3, Hm=8, Wm=8),
                                _nulls(("p_probs", "p_mask", "p_seg", "p_gk", "p_loss", "p_scratch"))
                                + _nonpos(("n_samples", "mask_batch", "heads", "h", "w", "L", "seg_l", "Hm", "Wm"))
                                + [({"h": 121, "w": 121}, BAD_SHAPE), ({"h": 120, "w": 121}, BAD_SHAPE), ({"seg_l": 5}, BAD_SHAPE),
                                   ({"mask_batch": 3}, BAD_SHAPE)]),
    "udt_bias_add_bf16": (("p_x", "p_bias", "p_out", "rows", "C"), dict(rows=3, C=8),
                          _nulls(("p_x", "p_bias", "p_out")) + _nonpos(("rows", "C")) + [({"C": 12}, BAD_SHAPE), ({"C": 4}, BAD_SHAPE)]),
    "udt_add_bf16": (("p_x", "p_y", "n"), dict(n=16), _nulls(("p_x", "p_y")) + _nonpos(("n",)) + [({"n": 12}, BAD_SHAPE), ({"n": 7}, BAD_SHAPE)]),
}


@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_refusals_return_their_code_and_write_nothing(env, entry):
    names, valid, refusals = REFUSALS[entry]
    bufs = {n: torch.full((4096,), MARKER, dtype=torch.float32, device=env.dev) for n in names if n.startswith("p_")}
    fn = getattr(env.lib, entry)
    for changes, status in refusals:
        args = {n: bufs[n].data_ptr() for n in bufs}
        args.update(valid)
        args.update(changes)
        assert fn(*[args[n] for n in names], env.st()) == status, (entry, changes)
    torch.cuda.synchronize()
    assert all(bool((b == MARKER).all()) for b in bufs.values()), f"{entry}: a refused call wrote"
    S._report(f"{'edge refusals ' + entry:55s} {len(refusals)} refused with their codes, buffers untouched", REPORT)


def test_packer_refusals_return_their_code_and_no_handle(env):
    lib, Ld = env.lib, env.L
    w = torch.full((4096,), MARKER, dtype=torch.float32, device=env.dev)
    segs = (C.c_int32 * 2)(3, 2)
    n = 0

    def refused(call, status):
        nonlocal n
        h = C.c_void_p()
        assert call(C.byref(h)) == status and not h.value
        n += 1
    lin = lambda N, K_, dtype, geglu, wp=w.data_ptr(): lambda out: lib.udt_pack_linear(wp, None, N, K_, dtype, geglu, out, env.st())
    refused(lin(4, 8, Ld.DTYPE_BF16, 0, wp=None), BAD_ARG)
    assert lib.udt_pack_linear(w.data_ptr(), None, 4, 8, Ld.DTYPE_BF16, 0, None, env.st()) == BAD_ARG
    for N, K_, dtype, geglu in ((0, 8, Ld.DTYPE_BF16, 0), (-1, 8, Ld.DTYPE_BF16, 0), (4, 0, Ld.DTYPE_BF16, 0), (4, 8, Ld.DTYPE_F32, 0), (4, 8, 3, 0),
                                (4, 8, -1, 0), (32, 8, Ld.DTYPE_BF16, 1), (96, 8, Ld.DTYPE_FP8_E4M3, 1), (65, 8, Ld.DTYPE_BF16, 1)):
        refused(lin(N, K_, dtype, geglu), BAD_SHAPE)
    conv = lambda N, Cin, kh, kw, sg, ns, npad, wp=w.data_ptr(): lambda out: lib.udt_pack_conv(wp, None, N, Cin, kh, kw, sg, ns, npad, out, env.st())
    refused(conv(4, 5, 3, 3, segs, 2, 4, wp=None), BAD_ARG)
    assert lib.udt_pack_conv(w.data_ptr(), None, 4, 5, 3, 3, segs, 2, 4, None, env.st()) == BAD_ARG
    for a in ((0, 5, 3, 3, segs, 2, 4), (4, 0, 3, 3, None, 0, 4), (4, 5, 0, 3, segs, 2, 4), (4, 5, 3, -1, segs, 2, 4), (4, 5, 3, 3, segs, 2, 0),
              (4, 5, 3, 3, segs, -1, 4), (4, 5, 3, 3, None, 2, 4), (4, 6, 3, 3, segs, 2, 4), (4, 4, 3, 3, segs, 2, 4),
              (4, 5, 3, 3, (C.c_int32 * 2)(5, 0), 2, 4), (4, 5, 3, 3, (C.c_int32 * 2)(6, -1), 2, 4)):
        refused(conv(*a), BAD_SHAPE)
    torch.cuda.synchronize()
    assert bool((w == MARKER).all())
    S._report(f"{'edge refusals udt_pack_linear / udt_pack_conv':55s} {n + 2} refused with their codes, no handle", REPORT)
