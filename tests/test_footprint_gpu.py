"""Memory footprint of every kernel entry point: guards, poisoned padding, exact scratch, aliasing (tests/footprint.py).

Each case of the table runs its op twice:
  1. on GUARDED buffers — every operand a strided view inside an arena whose lead guard, trail guard and ld gaps hold NaN poison,
     every output inside an arena of output sentinel, every scratch buffer of exactly the stated size between two guards;
  2. on COMPACT buffers — dense tensors of exactly the operand's shape;
and asserts that the payloads are BIT-EQUAL, that no guard or gap byte changed, that no output element was left unwritten, and —
for GEMM launches that plan a workspace — that its first 4 KiB read zero afterwards.  (The guarded run comes first: a mistake
in a case's own sizes then lands in a guard and is reported.)  No tolerance is involved: the kernels are deterministic.

Leading dimensions are multiples of 8 elements (16 bytes for bf16) and views start 256-byte aligned, as every slice the product
hands to a kernel does: the launch plans (lean_plan / lean_conv_plan / conv_n4_applies in csrc/gemm.hip) key on 16-byte aligned
pointers and ld % 8, so a guarded layout of that kind takes the SAME plan as the compact one and the comparison can be bitwise.
COMPARED lists the cases that are compared with a float64 reference at their existing test's bound instead; it is empty: none
of the shapes below changes its plan with the stride.  ``test_census`` holds the count.

Shapes the library refuses were replaced by the nearest accepted one with the same ragged property (noted at the case):
  split-K GEMM               96 x 640 x 2560 next to the 96 x 640 x 2048 launch: lean_plan cuts K from 40 K-tiles of 64 up, so K = 2048
                             plans no slabs; both run twice back to back
  transposed GEMM epilogue   M = 132 (rows_per_batch 44: the epilogue needs rows_per_batch % 4 == 0; 130 has no such divisor)
  softmax_rows               cols 72, ld 88 (udt_softmax_rows needs cols % 8 == 0; 77 is refused)
  linear_mx8 emitting        the first of (130, 256, 256), (130, 640, 640), (130, 1280, 1280) that udt_gemm_q8_ok accepts

The ops that had no direct numeric test get one here against float64 (bounds from the arithmetic, see each test).
"""
import contextlib
import ctypes as C
import math
import os

import pytest
import torch
import torch.nn.functional as F

import footprint as fp
import mx8_ref

pytestmark = pytest.mark.gpu

BF16, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32
TOL_OP = 1.5e-2                       # tests/test_backward_gpu.py: relative RMS of a reverse-pass op against float64 / autograd
WS_HEADER = 4096                      # include/udt_kernels.h: "the first 4 KiB of a workspace ... are zero again after every successful launch"

# case name -> reason: compared with float64 at its existing bound instead of bit-equal because the plan differs with the stride
COMPARED: dict = {}

# entry points of include/udt_kernels.h without a case of their own, and why
EXEMPT = {
    # pure size / capability queries: no launch
    "udt_gemm_workspace_bytes": "size query (exercised: every workspace below has exactly this size)",
    "udt_workspace_bytes": "alias of udt_gemm_workspace_bytes",
    "udt_gemm_colstats_rows": "query", "udt_gemm_colstats_slots": "size query (exercised by the colstats case)",
    "udt_gemm_rowstat_parts": "size query (exercised by the linear_mx8 case)", "udt_gemm_q8_ok": "query",
    "udt_gemm_in_scsh_ok": "query", "udt_gemm_up4_ok": "query", "udt_attn512_workspace_bytes": "size query (exercised)",
    "udt_tattn_hp": "size query (exercised)", "udt_tattn_rowstat_parts": "size query (exercised)",
    "udt_gn_nchunks": "size query (exercised)", "udt_gn_strip_ok": "query", "udt_colparts": "size query (exercised)",
    "udt_wgrad_splits": "size query (exercised)", "udt_xattn_kv_splits": "size query (exercised)",
    # packed-weight handles: the library allocates their memory itself
    "udt_pack_linear": "packed-weight handle", "udt_pack_conv": "packed-weight handle", "udt_packed_weight": "packed-weight handle",
    "udt_packed_bias": "packed-weight handle", "udt_packed_colscale": "packed-weight handle", "udt_packed_dim": "packed-weight handle",
    "udt_free_packed": "packed-weight handle",
    # services
    "udt_version": "service", "udt_status_string": "service", "udt_last_hip_error": "service", "udt_device_arch_ok": "service",
    "udt_debug_set": "service", "udt_prof_enable": "profiling service", "udt_prof_reset": "profiling service",
    "udt_prof_trace": "profiling service", "udt_prof_dump": "profiling service", "udt_prof_get": "profiling service",
    # same function under a second name (csrc/pack.hip): the launch is the covered one
    "udt_gemm_fwd": "udt_gemm under its SURVEY name", "udt_conv1x1_fwd": "udt_gemm restricted to 1x1 convolutions",
    "udt_sampler_step": "udt_cfg_euler_step under its SURVEY name",
    # square-map forms that only forward to the covered h x w entry points (csrc/backward.hip)
    "udt_local_loss_bwd": "forwards to udt_local_loss_bwd_hw with h = w = size",
    "udt_local_loss_seg_bwd": "forwards to udt_local_loss_seg_bwd_hw with h = w = size",
}

CASES = []                            # (name, fn, covered entry points)
SEEN = {"bit_equal": [], "compared": []}
REPORT_LINES = []


def case(name, covers):
    def deco(fn):
        CASES.append((name, fn, tuple(covers)))
        return fn
    return deco


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(tuple(shape), generator=g) * scale + shift


def _p(t):
    return None if t is None else t.data_ptr()


class Bufs:
    """the buffers of one run of a case: guarded / poisoned / exact (guarded=True) or compact"""

    def __init__(self, dev, guarded):
        self.dev, self.guarded = dev, guarded
        self.records = []
        self.workspaces = []
        self.scratches = []           # (name, stated bytes, view)
        self.keep = []                # every tensor handed out stays alive until the run is over (cases pass raw pointers)

    def _hold(self, t):
        self.keep.append(t)
        return t

    def inp(self, t, ld=None, name="in"):
        t = t.to(self.dev)
        if not self.guarded:
            return self._hold(t.contiguous().clone())
        v, rec = fp.poisoned(t, ld=ld, name=name)
        self.records.append(rec)
        return v

    def inout(self, t, ld=None, name="inout"):
        """an operand the kernel updates in place: guards and gaps hold the output sentinel (a NaN as well)"""
        t = t.to(self.dev)
        if not self.guarded:
            return self._hold(t.contiguous().clone())
        v, rec = fp.poisoned(t, ld=ld, name=name, pattern=fp.out_sentinel(t.dtype))
        self.records.append(rec)
        return v

    def out(self, shape, dtype, ld=None, name="out"):
        if not self.guarded:
            v, rec = fp.guarded(shape, dtype, self.dev, name=name)        # dense, sentinel-filled as well
            self.keep.append(rec)
            return v
        v, rec = fp.guarded(shape, dtype, self.dev, ld=ld, name=name)
        self.records.append(rec)
        return v

    def scratch(self, nbytes, name="scratch", dtype=F32):
        nbytes = int(nbytes)
        if self.guarded:
            v, rec = fp.exact_scratch(nbytes, self.dev, name=name)
            self.records.append(rec)
        else:
            v = torch.full((nbytes,), 0xFF, dtype=U8, device=self.dev)
        self.scratches.append((name, nbytes, v))
        return v.view(dtype) if dtype != U8 else v

    def workspace(self, nbytes):
        """a GEMM workspace of exactly ``nbytes``: header zeroed once (the stated contract), slabs left as 0xFF"""
        assert nbytes >= WS_HEADER
        v = self.scratch(nbytes, name="gemm workspace", dtype=U8)
        v[:WS_HEADER] = 0
        self.workspaces.append(v)
        return v

    @contextlib.contextmanager
    def ops_alloc(self):
        """route what the ops.* wrappers allocate themselves — the stream-K workspace and the column statistics — through this
        object, at exactly the sizes the library states; on exit every workspace header must read zero"""
        from udifftext_amd import lib as L, ops as O
        lib = L.load()
        n_before = len(self.workspaces)

        def ws(nbytes, device):
            return self.workspace(nbytes)

        def attach_colstats(d, out, n_cols, rows_per_batch):
            rows = lib.udt_gemm_colstats_rows(C.byref(d))
            if rows <= 0:
                return False
            slots = lib.udt_gemm_colstats_slots(C.byref(d))
            st = self.out((slots, n_cols, 2), F32, name="colstats")
            d.colstats = st.data_ptr()
            out.gn_stats = O.GnStats(st, rows_per_batch // rows)
            return True
        prev = (O._ws, O._attach_colstats)
        O._ws, O._attach_colstats = ws, attach_colstats
        try:
            yield
        finally:
            O._ws, O._attach_colstats = prev
        self.check_headers(n_before)

    def check_headers(self, first=0):
        for w in self.workspaces[first:]:
            nz = torch.nonzero(w[:WS_HEADER])
            assert nz.numel() == 0, f"GEMM workspace header not zero after the launch: first non-zero byte {int(nz[0, 0])}"

    def check(self):
        for rec in self.records:
            fp.assert_untouched(rec)
        self.check_headers()

    def scratch_report(self):
        out = []
        for name, stated, v in self.scratches:
            w = torch.nonzero(v != 0xFF)
            out.append(f"{name} stated {stated} B, highest byte written {int(w[-1, 0]) + 1 if w.numel() else 0}")
        return "; ".join(out)


def _run_case(name, fn, dev):
    g = Bufs(dev, True)
    got = fn(g)
    torch.cuda.synchronize()
    g.check()
    c = Bufs(dev, False)
    want = fn(c)
    torch.cuda.synchronize()
    c.check_headers()
    assert set(got) == set(want) and got, name
    for k in sorted(got):
        if not k.startswith("~"):         # "~name": the kernel leaves part of this output alone by contract (checked by the case)
            assert not fp.holds_sentinel(got[k]), f"{name}: output '{k}' still holds the sentinel: an element was not written"
        assert fp.bit_equal(got[k], want[k]), (
            f"{name}: output '{k}' differs between the guarded / poisoned layout and the compact one "
            f"({int((fp.bits(got[k]) != fp.bits(want[k])).sum())} of {got[k].numel()} elements)")
    SEEN["compared" if name in COMPARED else "bit_equal"].append(name)
    line = f"{name}: bit-equal ({', '.join(sorted(got))}); guards clean ({len(g.records)} arenas)"
    sr = g.scratch_report()
    if sr:
        line += f"; {sr}"
    REPORT_LINES.append(line)


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib, ops, packing
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)

    class Env:
        pass
    Env.O, Env.L, Env.lib, Env.P, Env.dev = ops, lib, lib.load(), packing, cuda
    yield Env
    path = os.environ.get("UDT_FOOTPRINT_REPORT")
    if path and REPORT_LINES:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("# one line per case of tests/test_footprint_gpu.py (written with UDT_FOOTPRINT_REPORT set)\n")
            f.write("\n".join(REPORT_LINES) + "\n")
            f.write(f"# {len(SEEN['bit_equal'])} cases bit-equal, {len(SEEN['compared'])} compared by bound ({len(COMPARED)} named)\n")


def _mods():
    from udifftext_amd import lib as L, ops as O, packing as P
    return O, L, L.load(), P


def _chk(rc, what):
    from udifftext_amd import lib as L
    L.check(rc, what)


# =================================================================================================== GEMM family
def _lin(M, N, K, seed=1):
    O, L, lib, P = _mods()
    x = _rand((M, K), seed).bfloat16()
    w = P.pack_linear(_rand((N, K), seed + 1, 1.0 / math.sqrt(K)) * (1.0 + torch.arange(N)[:, None] / N))
    bias = _rand((N,), seed + 2)
    return x, w, bias


def _linear_case(M, N, K):
    def fn(b):
        O, L, lib, P = _mods()
        x, w, bias = _lin(M, N, K)
        out = b.out((M, N), BF16, ld=N + 64)
        with b.ops_alloc():
            O.linear(b.inp(x, ld=K + 8, name="x"), b.inp(w, name="w"), b.inp(bias, name="bias"), out=out)
        return {"out": out}
    return fn


case("linear 130x320x320 ldo=N+64", ["udt_gemm"])(_linear_case(130, 320, 320))
case("linear 70x640x64 ldo=N+64", ["udt_gemm"])(_linear_case(70, 640, 64))


def _twice_case(K, must_split):
    def fn(b):
        O, L, lib, P = _mods()
        M, N = 96, 640
        x, w, bias = _lin(M, N, K)
        xv, wv, bv = b.inp(x, ld=K + 8, name="x"), b.inp(w, name="w"), b.inp(bias, name="bias")
        out1, out2 = b.out((M, N), BF16, ld=N + 64, name="out1"), b.out((M, N), BF16, ld=N + 64, name="out2")
        d = O.gemm_desc(a=_p(xv), w=_p(wv), bias=_p(bv), out=_p(out1), M=M, N=N, K=K, lda=xv.stride(0), ldo=out1.stride(0))
        need = lib.udt_gemm_workspace_bytes(C.byref(d))
        if not must_split and need == 0:                      # (no slabs planned: two plain launches)
            for o in (out1, out2):
                d.out = _p(o)
                _chk(lib.udt_gemm(C.byref(d), None, 0, O._stream()), "udt_gemm")
            assert fp.bit_equal(out1, out2)
            return {"out1": out1, "out2": out2}
        assert need > WS_HEADER, "this shape is expected to plan split-K slabs"
        ws = b.workspace(need)
        _chk(lib.udt_gemm(C.byref(d), _p(ws), need, O._stream()), "udt_gemm")
        b.check_headers()                                     # after the first launch ...
        d.out = _p(out2)
        _chk(lib.udt_gemm(C.byref(d), _p(ws), need, O._stream()), "udt_gemm")
        b.check_headers()                                     # ... and after the second on the same workspace
        _chk(lib.udt_check_async_error(_p(ws), need, O._stream()), "udt_check_async_error")
        assert fp.bit_equal(out1, out2)
        assert lib.udt_gemm(C.byref(d), _p(ws), need - 1, O._stream()) == -3        # UDT_ERR_WORKSPACE: one byte less is refused
        return {"out1": out1, "out2": out2}
    return fn


# (lean_plan cuts K from 40 K-tiles up: 96 x 640 x 2048 — 32 K-tiles — plans no slabs on the lean kernels; 2560 is the nearest K that does)
case("linear 96x640x2048 twice back to back (workspace exact where one is planned)", ["udt_gemm"])(_twice_case(2048, False))
case("linear split-K 96x640x2560 twice, workspace exact, header zero after each, udt_check_async_error",
     ["udt_gemm", "udt_check_async_error"])(_twice_case(2560, True))


def _epilogue_case(kind):
    def fn(b):
        O, L, lib, P = _mods()
        M, N, K = (132 if kind == "transposed" else 130), 320, 320
        x, w, bias = _lin(M, N, K, seed=11)
        xv = b.inp(x, ld=K + 8, name="x")
        kw, shape, dt, ld = {}, (M, N), BF16, N + 64
        if kind == "bias+residual":
            kw = dict(residual=b.inp(_rand((M, N), 14).bfloat16(), ld=N + 72, name="residual"))
        elif kind == "rowvec":
            kw = dict(rowvec=b.inp(_rand((2, N), 15), ld=N + 64, name="rowvec"), rows_per_batch=65)
        elif kind == "geglu":
            w, bias = P.pack_geglu(_rand((N, K), 12, 1 / math.sqrt(K)), _rand((N,), 13, 0.5))
            kw, shape, ld = dict(flags=L.GEMM_GEGLU), (M, N // 2), N // 2 + 64
        elif kind == "out_f32":
            kw, dt = dict(flags=L.GEMM_OUT_F32), F32
        elif kind == "transposed":
            kw, shape, ld = dict(flags=L.GEMM_TRANSPOSED, rows_per_batch=44), (3, N, 44), None
        elif kind == "silu_out":
            kw = dict(flags=L.GEMM_SILU_OUT)
        out = b.out(shape, dt, ld=ld)
        with b.ops_alloc():
            O.linear(xv, b.inp(w, name="w"), b.inp(bias, name="bias"), out=out, **kw)
        return {"out": out}
    return fn


for _k in ("bias+residual", "rowvec", "geglu", "out_f32", "transposed", "silu_out"):
    case(f"linear epilogue {_k} 130x320x320", ["udt_gemm"])(_epilogue_case(_k))


@case("linear out aliases residual, bit-equal to out of place", ["udt_gemm"])
def _alias_res(b):
    O, L, lib, P = _mods()
    M, N, K = 130, 320, 320
    x, w, bias = _lin(M, N, K, seed=21)
    r = _rand((M, N), 24).bfloat16()
    xv, wv, bv = b.inp(x, ld=K + 8, name="x"), b.inp(w, name="w"), b.inp(bias, name="bias")
    sep = b.out((M, N), BF16, ld=N + 64, name="out of place")
    rio = b.inout(r, ld=N + 64, name="out = residual")
    with b.ops_alloc():
        O.linear(xv, wv, bv, residual=b.inp(r, ld=N + 64, name="residual"), out=sep)
        O.linear(xv, wv, bv, residual=rio, out=rio)
    assert fp.bit_equal(sep, rio), "out= aliasing residual differs from the out-of-place launch"
    return {"sep": sep, "inplace": rio}


def _ln_linear_case(M, N, K, geglu):
    def fn(b):
        O, L, lib, P = _mods()
        x = _rand((M, K), 31, 1.5, 0.3).bfloat16()
        gamma, beta = _rand((K,), 32, 0.2, 1.0), _rand((K,), 33, 0.2)
        w = _rand((N, K), 34, 1 / math.sqrt(K))
        wp, c, s = P.pack_ln_linear(w, _rand((N,), 35, 0.5), gamma, beta, geglu=geglu)
        n_cols = N // 2 if geglu else N
        out = b.out((M, n_cols), BF16, ld=n_cols + 64)
        with b.ops_alloc():
            O.ln_linear(b.inp(x, ld=K + 8, name="x"), b.inp(wp, name="w"), b.inp(c, name="c"), b.inp(s, name="s"), out=out,
                        flags=L.GEMM_GEGLU if geglu else 0)
        return {"out": out}
    return fn


case("ln_linear 777x2560x320 GEGLU", ["udt_ln_gemm_fwd"])(_ln_linear_case(777, 2560, 320, True))
case("ln_linear 130x960x320", ["udt_ln_gemm_fwd"])(_ln_linear_case(130, 960, 320, False))


@case("linear_mx8 emitting M=130: q8_out ld_q8>N, q8_scale / rowstat_out exact", ["udt_gemm"])
def _mx8_emit(b):
    O, L, lib, P = _mods()
    M = 130
    for N, K in ((256, 256), (640, 640), (1280, 1280)):
        x = _rand((M, K), 41) * torch.logspace(-1, 1, M)[:, None]
        xq, xs = mx8_ref.encode(x)
        wq, cs = P.pack_linear_fp8(_rand((N, K), 42, 1 / math.sqrt(K)))
        xv, sv, wv, cv = b.inp(xq, name="x e4m3"), b.inp(xs, name="x scales"), b.inp(wq, name="w e4m3"), b.inp(cs, name="colscale")
        bv = b.inp(_rand((N,), 43), name="bias")
        out = b.out((M, N), BF16, ld=N + 64)
        q8 = b.out((M, N), U8, ld=N + 64, name="q8_out")
        q8s = b.out(((N + 127) // 128, M), I32, name="q8_scale")
        d = O.gemm_desc(a=_p(xv), w=_p(wv), bias=_p(bv), out=_p(out), M=M, N=N, K=K, lda=K, ldo=out.stride(0), flags=L.GEMM_MX8,
                        colscale=_p(cv), a_scale=_p(sv), q8_out=_p(q8), q8_scale=_p(q8s), ld_q8=q8.stride(0))
        parts = lib.udt_gemm_rowstat_parts(C.byref(d))
        if lib.udt_gemm_q8_ok(C.byref(d)) and parts > 0:
            break
    else:
        raise AssertionError("no MX8-emitting plan at M = 130 for any of the candidate shapes")
    rs = b.out((parts, M, 2), F32, name="rowstat_out")
    d.rowstat_out = _p(rs)
    need = lib.udt_gemm_workspace_bytes(C.byref(d))
    ws = b.workspace(need) if need else None
    _chk(lib.udt_gemm(C.byref(d), _p(ws), need, O._stream()), "udt_gemm mx8")
    return {"out": out, "q8": q8, "q8_scale": q8s, "rowstat": rs}


@case("bmm_nt 2x70x72x64, stride_out larger than the problem", ["udt_gemm"])
def _bmm(b):
    O, L, lib, P = _mods()
    Bn, M, N, K = 2, 70, 72, 64
    a = _rand((Bn, M, K), 51).bfloat16()
    w = _rand((Bn, N, K), 52, 1 / math.sqrt(K)).bfloat16()
    big = b.out((Bn, M + 10, N), BF16, ld=N + 8)           # 10 spare rows per problem: stride_out = (M + 10) * ld
    out = big[:, :M]
    with b.ops_alloc():
        O.bmm_nt(b.inp(a, ld=K + 8, name="a"), b.inp(w, ld=K + 8, name="w"), out=out, alpha=0.5)
    spare = big[:, M:]
    assert fp.all_sentinel(spare), "rows between the batched outputs were written"
    return {"out": out, "~spare": spare}


# =================================================================================================== convolutions
def _conv_case(B, H, W, C1, N, *, C2=0, ksize=3, stride=1, upsample=False, up4=False, f32=False, residual=True, colstats=False,
               scsh=False, cu_share=None):
    def fn(b):
        O, L, lib, P = _mods()
        Cin = C1 + C2
        x1 = b.inp(_rand((B, H, W, C1), 61, 1.0, 0.2).bfloat16(), name="x")
        x2 = b.inp(_rand((B, H, W, C2), 62).bfloat16(), name="x2") if C2 else None
        w = _rand((N, Cin, ksize, ksize), 63, 1 / math.sqrt(Cin * ksize * ksize))
        w = w * (1.0 + torch.arange(ksize * ksize).reshape(1, 1, ksize, ksize) / 4.0)
        wp = b.inp(P.pack_conv(w, [C1, C2] if C2 else None), name="w")
        bias = b.inp(P.pad_bias(_rand((N,), 64)), name="bias")
        Hv, Wv = (2 * H, 2 * W) if upsample else (H, W)
        pad = ksize // 2
        Ho, Wo = (Hv + 2 * pad - ksize) // stride + 1, (Wv + 2 * pad - ksize) // stride + 1
        dt = F32 if f32 else BF16
        ldo = N + (8 if N < 64 else 64)
        out = b.out((B, Ho, Wo, N), dt, ld=ldo)                       # a channel slice of a wider NHWC buffer
        kw = {}
        if residual and not f32:
            kw["residual"] = b.inp(_rand((B, Ho, Wo, N), 65).bfloat16(), ld=N + 72, name="residual")
        if up4:
            kw["w_up4"] = b.inp(P.pack_conv_up4(w), name="w_up4")
        if scsh:
            xf = x1.float().reshape(B, H * W, 32, C1 // 32)
            mean = xf.mean(dim=(1, 3), keepdim=True)
            rstd = (xf.var(dim=(1, 3), unbiased=False, keepdim=True) + 1e-5).rsqrt()
            gamma, beta = _rand((C1,), 66, 0.2, 1.0).to(b.dev), _rand((C1,), 67, 0.2).to(b.dev)
            scale = (rstd.expand(B, 1, 32, C1 // 32).reshape(B, C1)) * gamma
            shift = beta - mean.expand(B, 1, 32, C1 // 32).reshape(B, C1) * scale
            tab = torch.stack([scale.reshape(B, C1 // 64, 64), shift.reshape(B, C1 // 64, 64)], dim=2).contiguous()
            kw.update(in_scsh=b.inp(tab, name="in_scsh"), in_act=1)
        ctx = O.launch_context(cu_share=cu_share) if cu_share else contextlib.nullcontext()
        with b.ops_alloc(), ctx:
            O.conv2d(x1, wp, bias, ksize=ksize, stride=stride, upsample=upsample, x2=x2, out=out, n_out=N,
                     flags=L.GEMM_OUT_F32 if f32 else 0, colstats=colstats, **kw)
        res = {"out": out}
        if colstats:
            st = O.gn_stats_of(out)
            assert st is not None, "this shape is expected to emit column statistics"
            res["~colstats"] = st.data                               # (slots past the last image are not written)
            live = st.data[:B * st.slots_per_sample]
            assert not fp.holds_sentinel(live), "a live statistics slot was not written"
        return res
    return fn


case("conv3x3 B2 13x9x64->128 (ragged map)", ["udt_gemm"])(_conv_case(2, 13, 9, 64, 128))
case("conv3x3 B1 16x16x320->320 (lean)", ["udt_gemm"])(_conv_case(1, 16, 16, 320, 320))
# the wide 16 x 16 x 160 instance by lean_conv_plan's own rule: units * share >= CUs, i.e. a launch planned for 1/128 of the device
case("conv3x3 B1 16x16x320->320 cu_share=128 (wide by its own rule)", ["udt_gemm"])(_conv_case(1, 16, 16, 320, 320, cu_share=128))
case("conv3x3 stride 2 16x16x320->320", ["udt_gemm"])(_conv_case(1, 16, 16, 320, 320, stride=2))
case("conv3x3 nearest x2 upsample 8x8x320->320 (nine taps)", ["udt_gemm"])(_conv_case(1, 8, 8, 320, 320, upsample=True))
case("conv3x3 nearest x2 upsample 8x8x320->320 (w_up4 phase form)", ["udt_gemm"])(_conv_case(1, 8, 8, 320, 320, upsample=True, up4=True))
case("conv1x1 two sources 8x8 320+320->320", ["udt_gemm"])(_conv_case(1, 8, 8, 320, 320, C2=320, ksize=1))
case("conv3x3 four output channels fp32 13x9x64", ["udt_gemm"])(_conv_case(1, 13, 9, 64, 4, f32=True))
case("conv3x3 colstats B2 16x16x320->320, statistics exact", ["udt_gemm"])(_conv_case(2, 16, 16, 320, 320, colstats=True))
case("conv3x3 fused GroupNorm input (in_scsh) 2x16x16x320->320", ["udt_gn_silu_conv3x3_fwd"])(_conv_case(2, 16, 16, 320, 320, scsh=True))


# =================================================================================================== attention
def _qkv(b, B, n, Cc, seed, ld_extra=64):
    t = _rand((B, n, 3 * Cc), seed).bfloat16()
    return b.inp(t, ld=3 * Cc + ld_extra, name="q|k|v")


def _rowv_case(B, H, Nq, Nk, q8=False):
    def fn(b):
        O, L, lib, P = _mods()
        Cc = H * 64
        buf = _qkv(b, B, max(Nq, Nk), Cc, 71)
        q, k, v = buf[:, :Nq, :Cc], buf[:, :Nk, Cc:2 * Cc], buf[:, :Nk, 2 * Cc:]
        out = b.out((B, Nq, Cc), BF16, ld=Cc + 64)
        if not q8:
            O.attention_rowv(q, k, v, H, 0.125, out=out)
            return {"out": out}
        q8o = b.out((B * Nq, Cc), U8, ld=Cc + 64, name="q8_out")
        q8s = b.out((Cc // 128, B * Nq), I32, name="q8_scale")
        _chk(lib.udt_attn_rowv_q8_fwd(_p(q), _p(k), _p(v), _p(out), B, H, Nq, Nk, q.stride(1), k.stride(1), v.stride(1), out.stride(1),
                                      q.stride(0), k.stride(0), v.stride(0), out.stride(0), 0.125, _p(q8o), _p(q8s), q8o.stride(0),
                                      O._stream()), "udt_attn_rowv_q8_fwd")
        return {"out": out, "q8": q8o, "q8_scale": q8s}
    return fn


case("attention_rowv (1,5,200,136) slices of q|k|v", ["udt_attn_rowv_fwd"])(_rowv_case(1, 5, 200, 136))
case("attention_rowv (3,2,130,40) slices of q|k|v", ["udt_attn_rowv_fwd"])(_rowv_case(3, 2, 130, 40))
case("attention_rowv emit_q8 (3,2,130,40)", ["udt_attn_rowv_q8_fwd"])(_rowv_case(3, 2, 130, 40, q8=True))


@case("attention transposed V (1,5,72,136)", ["udt_attn_fwd"])
def _attn_vt(b):
    O, L, lib, P = _mods()
    B, H, Nq, Nk = 1, 5, 72, 136
    Cc = H * 64
    qk = b.inp(_rand((B, max(Nq, Nk), 2 * Cc), 72).bfloat16(), ld=2 * Cc + 64, name="q|k")
    vt = b.inp(_rand((B, Cc, Nk), 73).bfloat16(), ld=Nk + 8, name="v^T")
    out = b.out((B, Nq, Cc), BF16, ld=Cc + 64)
    O.attention(qk[:, :Nq, :Cc], qk[:, :Nk, Cc:], vt, H, 0.125, out=out)
    return {"out": out}


def _attn_mx8_case(B, H, n):
    def fn(b):
        O, L, lib, P = _mods()
        Cc = H * 64
        qkv = _rand((B * n, 3 * Cc), 74)
        qkv[:, 2 * Cc:] *= 0.3
        qk8, qks = mx8_ref.encode(qkv[:, :2 * Cc])                    # (2 C is a multiple of 128 for even C / 64)
        v8 = (qkv[:, 2 * Cc:] * 64.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(U8)
        data = b.inp(torch.cat([qk8, v8], dim=1), ld=3 * Cc + 16, name="qkv8")
        ld8 = data.stride(0)
        scale = torch.zeros(((ld8 + 127) // 128, B * n), dtype=I32)
        scale[:qks.shape[0]] = qks
        scale[qks.shape[0]:] = 0x7F7F7F7F                             # unit scale bytes over the fixed-scale v third
        sc = b.inp(scale, name="qkv scales")
        out = b.out((B * n, Cc), BF16, ld=Cc + 64)
        q8o = b.out((B * n, Cc), U8, ld=Cc + 64, name="q8_out")
        q8s = b.out((Cc // 128, B * n), I32, name="q8_scale")
        _chk(lib.udt_attn_mx8_fwd(_p(data), _p(sc), _p(out), B, H, n, ld8, out.stride(0), 0.125, 1.0 / 64.0, _p(q8o), _p(q8s),
                                  q8o.stride(0), O._stream()), "udt_attn_mx8_fwd")
        return {"out": out, "q8": q8o, "q8_scale": q8s}
    return fn


case("attention_mx8 n=4 (smallest n % 4 == 0 below the 128-query tile), ld8 > 3C", ["udt_attn_mx8_fwd"])(_attn_mx8_case(2, 2, 4))
case("attention_mx8 n=132 (one full + one ragged query tile), ld8 > 3C", ["udt_attn_mx8_fwd"])(_attn_mx8_case(2, 2, 132))


def _attn512_case(B, Nq, Nk, split):
    def fn(b):
        O, L, lib, P = _mods()
        nk = Nk
        if split:                                                     # the smallest key count the library splits for this (B, Nq)
            nk = next(k for k in range(8, 4096) if lib.udt_attn512_workspace_bytes(B, Nq, k) > 0)
            assert lib.udt_attn512_workspace_bytes(B, Nq, nk - 1) == 0
        buf = b.inp(_rand((B, max(Nq, nk), 3 * 512), 75).bfloat16(), ld=3 * 512 + 64, name="q|k|v")
        q, k, v = buf[:, :Nq, :512], buf[:, :nk, 512:1024], buf[:, :nk, 1024:]
        out = b.out((B, Nq, 512), BF16, ld=512 + 64)
        args = (_p(q), _p(k), _p(v), _p(out), B, Nq, nk, q.stride(1), k.stride(1), v.stride(1), out.stride(1),
                q.stride(0), k.stride(0), v.stride(0), out.stride(0), 512 ** -0.5)
        if split:
            need = lib.udt_attn512_workspace_bytes(B, Nq, nk)
            ws = b.scratch(need, name=f"attn512 key-split workspace (nk {nk})", dtype=U8)
            _chk(lib.udt_attn512_split_fwd(*args, _p(ws), need, O._stream()), "udt_attn512_split_fwd")
            assert lib.udt_attn512_split_fwd(*args, _p(ws), need - 1, O._stream()) == -3
        else:
            _chk(lib.udt_attn512_fwd(*args, O._stream()), "udt_attn512_fwd")
        return {"out": out}
    return fn


case("attention_d512 (1,33,290) direct", ["udt_attn512_fwd"])(_attn512_case(1, 33, 290, False))
case("attention_d512 key split at the smallest split nk, nq 33, workspace exact", ["udt_attn512_split_fwd"])(_attn512_case(1, 33, 0, True))


def _xattn_case(B, H, Nq, Lc):
    def fn(b):
        O, L, lib, P = _mods()
        Cc = H * 64
        q = b.inp(_rand((B, Nq, Cc), 76).bfloat16(), ld=Cc + 64, name="q")
        kv = b.inp(_rand((B, Lc, 2 * Cc), 77).bfloat16(), ld=2 * Cc + 64, name="k|v")
        out = b.out((B, Nq, Cc), BF16, ld=Cc + 64)
        probs = b.out((B * H, Nq, Lc), F32, name="probs")
        O.xattention(q, kv[..., :Cc], kv[..., Cc:], H, 64, 0.125, probs=probs, out=out)
        return {"out": out, "probs": probs}
    return fn


case("xattention (1,10,64,300,12) probs guarded ldo>C", ["udt_xattn_fwd"])(_xattn_case(1, 10, 300, 12))
case("xattention (1,5,64,70,1) probs guarded ldo>C", ["udt_xattn_fwd"])(_xattn_case(1, 5, 70, 1))


@case("masked_attention Nq7 Lk26 D32 mask + key padding, strided", ["udt_mattn_fwd"])
def _mattn(b):
    O, L, lib, P = _mods()
    B, H, D, Nq, Lk = 2, 4, 32, 7, 26
    Cc = H * D
    q = b.inp(_rand((B, Nq, Cc), 78).bfloat16(), ld=Cc + 8, name="q")
    kv = b.inp(_rand((B, Lk, 2 * Cc), 79).bfloat16(), ld=2 * Cc + 8, name="k|v")
    mask = torch.zeros((Nq, Lk))
    mask[torch.triu(torch.ones((Nq, Lk), dtype=torch.bool), diagonal=20)] = float("-inf")
    kpm = torch.zeros((B, Lk), dtype=U8)
    kpm[1, 22:] = 1
    mv, kv_pm = b.inp(mask, ld=Lk + 6, name="mask"), b.inp(kpm, name="key padding mask")
    out = b.out((B, Nq, Cc), BF16, ld=Cc + 8)
    k, v = kv[..., :Cc], kv[..., Cc:]
    _chk(lib.udt_mattn_fwd(_p(q), _p(k), _p(v), _p(out), _p(mv), _p(kv_pm), B, H, D, Nq, Lk, q.stride(1), k.stride(1), v.stride(1),
                           out.stride(1), mv.stride(0), q.stride(0), k.stride(0), v.stride(0), out.stride(0), D ** -0.5, O._stream()),
         "udt_mattn_fwd")
    return {"out": out}


def _tattn_case(heads, q8):
    def fn(b):
        O, L, lib, P = _mods()
        B, n_tok, Lc, zero = 3, 64, 12, 1
        Cc = heads * 64
        hp = lib.udt_tattn_hp(heads)
        x = b.inp(_rand((B, n_tok, Cc), 81, 1.5, 0.3).bfloat16(), name="x")
        kv = b.inp(_rand((B, Lc, 2 * Cc), 82).bfloat16(), name="k|v")
        wq = b.inp(P.pack_linear(_rand((Cc, Cc), 83, 1 / math.sqrt(Cc))), name="wq")
        wo = b.inp(P.pack_linear(_rand((Cc, Cc), 84, 1 / math.sqrt(Cc))), name="wo")
        gamma, beta = b.inp(_rand((Cc,), 85, 0.2, 1.0), name="gamma"), b.inp(_rand((Cc,), 86, 0.2), name="beta")
        bias = b.inp(_rand((Cc,), 87, 0.3), name="bias")
        tabs = O.TattnTables(b.out((B, hp, Cc), BF16, name="A'"), b.out((B, hp, 2), F32, name="sc"), b.out((B, Cc, hp), BF16, name="BmT"))
        O.tattn_prepare(kv, wq, wo, gamma, beta, heads, 0.125, out=tabs)
        out = b.out((B, n_tok, Cc), BF16)
        # (the tables of the zero-context samples are never read: only samples >= zero_samples must be written)
        res = {"out": out, "~A'": tabs.A, "~sc": tabs.sc, "~BmT": tabs.BmT}
        if not q8:
            O.tattn_fused(x, tabs, bias, heads, zero, 1e-5, out=out)
            return res
        parts = lib.udt_tattn_rowstat_parts(B, n_tok, Cc)
        assert parts > 0
        M = B * n_tok
        q8o, q8s = b.out((M, Cc), U8, name="q8_out"), b.out((Cc // 128, M), I32, name="q8_scale")
        rs = b.out((parts, M, 2), F32, name="rowstat_out")
        _chk(lib.udt_tattn_fused_q8(_p(x), _p(out), _p(tabs.A), _p(tabs.sc), _p(tabs.BmT), _p(bias), B, n_tok, Cc, heads, zero, 1e-5,
                                    _p(q8o), _p(q8s), _p(rs), O._stream()), "udt_tattn_fused_q8")
        res.update({"q8": q8o, "q8_scale": q8s, "rowstat": rs})
        return res
    return fn


case("tattn_prepare + tattn_fused heads 5 n_tok 64 B3 zero 1, tables guarded", ["udt_tattn_prepare", "udt_tattn_fused"])(_tattn_case(5, False))
case("tattn_prepare + tattn_fused_q8 C=640, three extra outputs guarded", ["udt_tattn_prepare", "udt_tattn_fused_q8"])(_tattn_case(10, True))


@case("softmax_rows rows 5 cols 72 ld 88", ["udt_softmax_rows"])
def _softmax(b):
    O, L, lib, P = _mods()
    x = b.inout(_rand((5, 72), 88, 3.0).bfloat16(), ld=88, name="x")
    _chk(lib.udt_softmax_rows(_p(x), 5, 72, x.stride(0), O._stream()), "udt_softmax_rows")
    return {"x": x}


# =================================================================================================== norms
def _gn_operands(b, B, HW, C1, C2, seed=91):
    x = b.inp(_rand((B, HW, C1), seed, 2.0, 0.7).bfloat16(), name="x")
    x2 = b.inp(_rand((B, HW, C2), seed + 1, 0.5, -0.3).bfloat16(), name="x2") if C2 else None
    gamma, beta = b.inp(_rand((C1 + C2,), seed + 2, 0.2, 1.0), name="gamma"), b.inp(_rand((C1 + C2,), seed + 3, 0.2), name="beta")
    return x, x2, gamma, beta


def _gn_two_kernel_case(B, HW, C1, C2=0, inplace=False):
    def fn(b):
        O, L, lib, P = _mods()
        G, Ct = 32, C1 + C2
        x, x2, gamma, beta = _gn_operands(b, B, HW, C1, C2)
        nch = lib.udt_gn_nchunks(HW, Ct)
        part = b.scratch(B * nch * G * 2 * 4, name="GroupNorm partials")
        y = b.out((B, HW, Ct), BF16, name="y")
        _chk(lib.udt_gn_stats(_p(x), _p(x2), _p(part), B, HW, C1, C2, G, O._stream()), "udt_gn_stats")
        _chk(lib.udt_gn_apply(_p(x), _p(x2), _p(y), _p(part), _p(gamma), _p(beta), B, HW, C1, C2, G, 1e-5, 1, O._stream()), "udt_gn_apply")
        res = {"y": y, "partials": part}
        if inplace:
            xio = b.inout(x.clone(), name="x = y")
            _chk(lib.udt_gn_apply(_p(xio), None, _p(xio), _p(part), _p(gamma), _p(beta), B, HW, C1, 0, G, 1e-5, 1, O._stream()),
                 "udt_gn_apply in place")
            assert fp.bit_equal(xio, y), "udt_gn_apply with y = x differs from the out-of-place launch"
            res["inplace"] = xio
        return res
    return fn


case("group_norm two-kernel (2,9,320), partials exact, in place", ["udt_gn_stats", "udt_gn_apply"])(_gn_two_kernel_case(2, 9, 320, inplace=True))
case("group_norm two-kernel (1,576,640), partials exact", ["udt_gn_stats", "udt_gn_apply"])(_gn_two_kernel_case(1, 576, 640))
case("group_norm two-kernel two sources HW 9 640+320", ["udt_gn_stats", "udt_gn_apply"])(_gn_two_kernel_case(2, 9, 640, 320))


def _slot_stats(x, slots):
    """column statistics as a producer's epilogue leaves them: fp32 [B * slots, C, 2] over `slots` row ranges per sample"""
    B, HW, Cc = x.shape
    xs = x.float().reshape(B, slots, HW // slots, Cc)
    return torch.stack([xs.sum(dim=2), xs.pow(2).sum(dim=2)], dim=-1).reshape(B * slots, Cc, 2).contiguous()


def _gn_strip_case(B, HW, C1, C2, stats):
    def fn(b):
        O, L, lib, P = _mods()
        G = 32
        assert lib.udt_gn_strip_ok(B, HW, C1, C2, G) == 1
        x, x2, gamma, beta = _gn_operands(b, B, HW, C1, C2, seed=95)
        y = b.out((B, HW, C1 + C2), BF16, name="y")
        if not stats:
            _chk(lib.udt_gn_strip(_p(x), _p(x2), _p(y), _p(gamma), _p(beta), B, HW, C1, C2, G, 1e-5, 1, O._stream()), "udt_gn_strip")
        else:
            s1 = b.inp(_slot_stats(x, 1), name="stats1")
            s2 = b.inp(_slot_stats(x2, 1), name="stats2") if C2 else None
            _chk(lib.udt_gn_strip_stats(_p(x), _p(x2), _p(y), _p(s1), 1, _p(s2), 1 if C2 else 0, _p(gamma), _p(beta), B, HW, C1, C2, G,
                                        1e-5, 1, O._stream()), "udt_gn_strip_stats")
        return {"y": y}
    return fn


# (udt_gn_strip_ok admits any strip of <= 64 KiB whose group width pads to 8 channels: one pixel is its smallest map)
case("gn_strip (2,1,320) smallest admitted shape", ["udt_gn_strip"])(_gn_strip_case(2, 1, 320, 0, False))
case("gn_strip (2,9,320+320) two sources", ["udt_gn_strip"])(_gn_strip_case(2, 9, 320, 320, False))
case("gn_strip_stats (2,1,320) smallest admitted shape", ["udt_gn_strip_stats"])(_gn_strip_case(2, 1, 320, 0, True))
case("gn_strip_stats (2,9,320+320) two sources", ["udt_gn_strip_stats"])(_gn_strip_case(2, 9, 320, 320, True))


@case("gn_finalize + gn_apply_scsh (2,64,320)", ["udt_gn_finalize", "udt_gn_apply_scsh"])
def _gn_scsh(b):
    O, L, lib, P = _mods()
    B, HW, Cc, G, slots = 2, 64, 320, 32, 2
    x, _, gamma, beta = _gn_operands(b, B, HW, Cc, 0, seed=99)
    st = b.inp(_slot_stats(x, slots), name="stats1")
    scsh = b.out((B, Cc // 64, 2, 64), F32, name="scsh")
    _chk(lib.udt_gn_finalize(_p(st), slots, Cc, None, 0, 0, _p(gamma), _p(beta), _p(scsh), B, HW, G, 1e-5, O._stream()), "udt_gn_finalize")
    y = b.out((B, HW, Cc), BF16, name="y")
    _chk(lib.udt_gn_apply_scsh(_p(x), None, _p(y), _p(scsh), B, HW, Cc, 0, 1, O._stream()), "udt_gn_apply_scsh")
    return {"scsh": scsh, "y": y}


def _ln_case(rows, Cc):
    def fn(b):
        O, L, lib, P = _mods()
        x = b.inp(_rand((rows, Cc), 101, 2.0, 0.3).bfloat16(), name="x")
        y = b.out((rows, Cc), BF16, name="y")
        O.layer_norm(x, b.inp(_rand((Cc,), 102, 0.2, 1.0), name="gamma"), b.inp(_rand((Cc,), 103, 0.2), name="beta"), 1e-5, out=y)
        return {"y": y}
    return fn


for _r, _c in ((5, 320), (513, 640), (3, 4096)):
    case(f"layer_norm ({_r},{_c})", ["udt_layernorm"])(_ln_case(_r, _c))


# =================================================================================================== sampler / boundary elementwise
HW35, B3 = 35, 3


def _eps8(b, B, hw, seed):
    return b.inp(_rand((2 * B * hw, 4), seed), ld=8, name="eps (channels 4..7 poisoned)")


@case("cfg_euler_step ld_eps 8, den_out guarded", ["udt_cfg_euler_step"])
def _euler(b):
    O, L, lib, P = _mods()
    x = b.inout(_rand((B3, 4, HW35), 111, 10.0), name="x")
    den = b.out((B3, 4, HW35), F32, name="den_out")
    eps = _eps8(b, B3, HW35, 112)
    _chk(lib.udt_cfg_euler_step(_p(x), _p(eps), _p(den), B3, HW35, eps.stride(0), -3.2, 3.2, 2.9, 5.0, O._stream()), "udt_cfg_euler_step")
    return {"x": x, "den": den}


@case("cfg_sampler_step ld_eps 8, all terms, xout / den_out guarded", ["udt_cfg_sampler_step"])
def _sampler(b):
    O, L, lib, P = _mods()
    xin, aux, prev, noise = (b.inp(_rand((B3, 4, HW35), 113 + i, 3.0), name=n) for i, n in enumerate(("xin", "aux", "prev", "noise")))
    xout, den = b.out((B3, 4, HW35), F32, name="xout"), b.out((B3, 4, HW35), F32, name="den_out")
    k = L.SamplerCoefs(0.9, 0.2, -0.1, 0.05, 0.3, -3.2, 5.0)
    eps = _eps8(b, B3, HW35, 117)
    _chk(lib.udt_cfg_sampler_step(_p(xin), _p(eps), _p(aux), _p(prev), _p(noise), _p(xout), _p(den), B3, HW35, eps.stride(0), k,
                                  O._stream()), "udt_cfg_sampler_step")
    x2 = b.inout(xin.clone(), name="xout = xin")                      # the alias the header allows
    _chk(lib.udt_cfg_sampler_step(_p(x2), _p(eps), _p(aux), _p(prev), _p(noise), _p(x2), None, B3, HW35, eps.stride(0), k,
                                  O._stream()), "udt_cfg_sampler_step in place")
    assert fp.bit_equal(x2, xout)
    return {"xout": xout, "den": den, "inplace": x2}


@case("cfg_multistep_step ld_eps 8, n 3, xout / d_out guarded", ["udt_cfg_multistep_step"])
def _multistep(b):
    O, L, lib, P = _mods()
    xin, h1, h2 = (b.inp(_rand((B3, 4, HW35), 118 + i, 3.0), name=n) for i, n in enumerate(("xin", "hist1", "hist2")))
    xout, dout = b.out((B3, 4, HW35), F32, name="xout"), b.out((B3, 4, HW35), F32, name="d_out")
    k = L.MultistepCoefs(-3.2, 5.0, 3.2, 3)
    for j, cf in enumerate((-0.5, 0.2, -0.05)):
        k.k[j] = cf
    k.hist[1], k.hist[2] = _p(h1), _p(h2)
    eps = _eps8(b, B3, HW35, 121)
    _chk(lib.udt_cfg_multistep_step(_p(xin), _p(eps), _p(xout), _p(dout), B3, HW35, eps.stride(0), k, O._stream()),
         "udt_cfg_multistep_step")
    return {"xout": xout, "d_out": dout}


def _unet_input_case(churn):
    def fn(b):
        O, L, lib, P = _mods()
        cpad = 64
        x = b.inout(_rand((B3, 4, HW35), 122, 10.0), name="x")
        xin = b.out((2 * B3 * HW35, cpad), BF16, name="xin")
        if churn:
            noise = b.inp(_rand((B3, 4, HW35), 123), name="noise")
            _chk(lib.udt_unet_input_churn(_p(x), _p(noise), _p(xin), B3, HW35, cpad, 0.37, 0.8, O._stream()), "udt_unet_input_churn")
        else:
            _chk(lib.udt_unet_input(_p(x), _p(xin), B3, HW35, cpad, 0.37, O._stream()), "udt_unet_input")
        assert not fp.holds_sentinel(xin[:, :4])
        assert fp.all_sentinel(xin[:, 4:]), "channels >= 4 of xin were touched"
        return {"x": x, "~xin": xin}
    return fn


case("unet_input cpad 64: channels >= 4 keep their sentinel", ["udt_unet_input"])(_unet_input_case(False))
case("unet_input_churn cpad 64: channels >= 4 keep their sentinel", ["udt_unet_input_churn"])(_unet_input_case(True))


@case("posterior_sample ldm 16", ["udt_posterior_sample"])
def _posterior(b):
    O, L, lib, P = _mods()
    mom = _rand((B3 * HW35, 8), 124)
    mom[:, 4:] *= 5
    z = b.out((B3, 4, HW35), F32, name="z")
    mv = b.inp(mom, ld=16, name="moments")
    _chk(lib.udt_posterior_sample(_p(mv), _p(b.inp(_rand((B3, 4, HW35), 125), name="noise")), _p(z), B3, HW35, mv.stride(0), 0.18215,
                                  O._stream()), "udt_posterior_sample")
    return {"z": z}


@case("nchw_to_nhwc C 4 cpad 64: channels >= C exact zeros", ["udt_nchw_to_nhwc"])
def _to_nhwc(b):
    O, L, lib, P = _mods()
    y = b.out((B3 * HW35, 64), BF16, name="y")
    _chk(lib.udt_nchw_to_nhwc(_p(b.inp(_rand((B3, 4, HW35), 126), name="x")), _p(y), B3, 4, HW35, 64, 0.5, O._stream()), "udt_nchw_to_nhwc")
    assert bool((fp.bits(y[:, 4:]) == 0).all()), "channels >= C are not exact (+0) zeros"
    return {"y": y}


def _to_nchw_case(f32):
    def fn(b):
        O, L, lib, P = _mods()
        src = _rand((B3 * HW35, 4), 127)
        x = b.inp(src if f32 else src.bfloat16(), ld=64, name="x (ld 64 poisoned)")
        y = b.out((B3, 4, HW35), F32, name="y")
        _chk(lib.udt_nhwc_to_nchw(_p(x), _p(y), B3, 4, HW35, x.stride(0), 1 if f32 else 0, O._stream()), "udt_nhwc_to_nchw")
        return {"y": y}
    return fn


case("nhwc_to_nchw from bf16, ld 64 poisoned", ["udt_nhwc_to_nchw"])(_to_nchw_case(False))
case("nhwc_to_nchw from fp32, ld 64 poisoned", ["udt_nhwc_to_nchw"])(_to_nchw_case(True))


@case("nhwc_set_channels C 5 at c0 4 of cpad 64: every other channel keeps its sentinel", ["udt_nhwc_set_channels"])
def _set_channels(b):
    O, L, lib, P = _mods()
    dst = b.out((B3 * HW35, 64), BF16, name="dst")
    _chk(lib.udt_nhwc_set_channels(_p(b.inp(_rand((B3, 5, HW35), 128), name="src")), _p(dst), B3, 5, HW35, 64, 4, O._stream()),
         "udt_nhwc_set_channels")
    assert not fp.holds_sentinel(dst[:, 4:9])
    assert fp.all_sentinel(dst[:, :4]) and fp.all_sentinel(dst[:, 9:]), "a channel outside [c0, c0 + C) was touched"
    return {"~dst": dst}


@case("embed_tokens n_tok 26 L 13 D 72", ["udt_embed_tokens"])
def _embed(b):
    O, L, lib, P = _mods()
    g = torch.Generator().manual_seed(129)
    idx = torch.randint(0, 95, (26,), generator=g, dtype=I32)
    out = b.out((26, 72), BF16, name="out")
    _chk(lib.udt_embed_tokens(_p(b.inp(idx, name="idx")), _p(b.inp(_rand((95, 72), 130), name="table")), _p(b.inp(_rand((13, 72), 131), name="pe")),
                              _p(out), 26, 13, 72, O._stream()), "udt_embed_tokens")
    return {"out": out}


@case("timestep_embedding n 3 dim 320", ["udt_timestep_embedding"])
def _temb(b):
    O, L, lib, P = _mods()
    out = b.out((3, 320), BF16, name="out")
    _chk(lib.udt_timestep_embedding(_p(b.inp(torch.tensor([999.0, 979.0, 0.0]), name="t")), _p(out), 3, 320, O._stream()), "udt_timestep_embedding")
    return {"out": out}


@case("mask_downsample B 2 64x96", ["udt_mask_downsample"])
def _maskds(b):
    O, L, lib, P = _mods()
    out = b.out((2, 1, 8, 12), F32, name="out")
    _chk(lib.udt_mask_downsample(_p(b.inp((_rand((2, 1, 64, 96), 132) > 0).float(), name="mask")), _p(out), 2, 64, 96, O._stream()),
         "udt_mask_downsample")
    return {"out": out}


@case("bias_add rows 5 C 320 out of place and in place", ["udt_bias_add_bf16"])
def _bias_add(b):
    O, L, lib, P = _mods()
    x = _rand((5, 320), 133).bfloat16()
    bias = b.inp(_rand((320,), 134), name="bias")
    out = b.out((5, 320), BF16, name="out")
    O.bias_add(b.inp(x, name="x"), bias, out=out)
    xio = b.inout(x, name="x = out")
    O.bias_add(xio, bias, out=xio)
    assert fp.bit_equal(out, xio), "udt_bias_add_bf16 with out = x differs from the out-of-place launch"
    return {"out": out, "inplace": xio}


@case("add_ n = 8 x 33", ["udt_add_bf16"])
def _add(b):
    O, L, lib, P = _mods()
    x = b.inout(_rand((264,), 135).bfloat16(), name="x")
    O.add_(x, b.inp(_rand((264,), 136).bfloat16(), name="y"))
    return {"x": x}


def _gk9():
    xs = torch.arange(3).float()
    g1 = torch.exp(-(xs - 1) ** 2 / 2)
    gk = g1[:, None] * g1[None, :]
    return (gk / gk.sum()).reshape(9).contiguous()


def _ll_operands(b, n_samples, mask_batch, heads, n, Lc, seg_l, Hm, Wm, seed=141):
    probs = b.inp(torch.softmax(_rand((n_samples * heads, n, Lc), seed, 2.0), dim=-1), name="probs")
    mask = torch.zeros((mask_batch, 1, Hm, Wm))
    mask[:, :, Hm // 4:(3 * Hm) // 4, Wm // 8:(7 * Wm) // 8] = 1
    seg = torch.zeros((mask_batch, seg_l))
    seg[:, :3] = 1
    return probs, b.inp(mask, name="mask"), b.inp(seg, name="seg_mask"), b.inp(_gk9(), name="gkernel9")


@case("local_loss + local_loss_tiled size 6 heads 5 L 12 seg_l 5", ["udt_local_loss", "udt_local_loss_tiled"])
def _ll_fwd(b):
    O, L, lib, P = _mods()
    heads, size, Lc, seg_l, Hm = 5, 6, 12, 5, 48
    probs, mask, seg, gk = _ll_operands(b, 4, 2, heads, size * size, Lc, seg_l, Hm, Hm)
    loss_t = b.inout(torch.zeros((4,)), name="loss (tiled)")
    _chk(lib.udt_local_loss_tiled(_p(probs), _p(mask), _p(seg), _p(gk), _p(loss_t), 4, 2, heads, size, Lc, seg_l, Hm, Hm, O._stream()),
         "udt_local_loss_tiled")
    loss = b.inout(torch.zeros((2,)), name="loss")
    _chk(lib.udt_local_loss(_p(probs), _p(mask), _p(seg), _p(gk), _p(loss), 2, heads, size, Lc, seg_l, Hm, Hm, O._stream()), "udt_local_loss")
    return {"loss_tiled": loss_t, "loss": loss}


# =================================================================================================== reverse pass and training
def _ln_bwd_case(rows, Cc, add):
    def fn(b):
        O, L, lib, P = _mods()
        x = b.inp(_rand((rows, Cc), 151, 2.0, 0.5).bfloat16(), name="x")
        dy = b.inp(_rand((rows, Cc), 152).bfloat16(), name="dy")
        ad = b.inp(_rand((rows, Cc), 153).bfloat16(), name="add") if add else None
        dx = b.out((rows, Cc), BF16, name="dx")
        _chk(lib.udt_layernorm_bwd(_p(x), _p(dy), _p(b.inp(_rand((Cc,), 154, 0.2, 1.0), name="gamma")), _p(ad), _p(dx), rows, Cc, 1e-5,
                                   O._stream()), "udt_layernorm_bwd")
        return {"dx": dx}
    return fn


for _r, _c in ((5, 320), (301, 320), (3, 2048)):
    for _a in (False, True):
        case(f"layernorm_bwd rows {_r} C {_c}{' + add' if _a else ''}", ["udt_layernorm_bwd"])(_ln_bwd_case(_r, _c, _a))


def _gn_bwd_case(B, HW, Cc, chunked):
    def fn(b):
        O, L, lib, P = _mods()
        G = 32
        x = b.inp(_rand((B, HW, Cc), 155, 1.5, 0.3).bfloat16(), name="x")
        dy = b.inp(_rand((B, HW, Cc), 156).bfloat16(), name="dy")
        ad = b.inp(_rand((B, HW, Cc), 157).bfloat16(), name="add")
        gamma, beta = b.inp(_rand((Cc,), 158, 0.2, 1.0), name="gamma"), b.inp(_rand((Cc,), 159, 0.1), name="beta")
        dx = b.out((B, HW, Cc), BF16, name="dx")
        part = b.scratch(2 * B * lib.udt_gn_nchunks(HW, Cc) * G * 2 * 4, name="gn_bwd partials") if chunked else None
        _chk(lib.udt_gn_bwd(_p(x), _p(dy), _p(gamma), _p(beta), _p(ad), _p(dx), _p(part), B, HW, Cc, G, 1e-5, 1, O._stream()), "udt_gn_bwd")
        return {"dx": dx}
    return fn


for _s in ((2, 9, 320), (1, 9, 960)):
    case(f"gn_bwd {_s} chunked, partials exact", ["udt_gn_bwd"])(_gn_bwd_case(*_s, True))
    case(f"gn_bwd {_s} one workgroup per group", ["udt_gn_bwd"])(_gn_bwd_case(*_s, False))


@case("geglu_fwd / geglu_bwd rows 3 inner 40", ["udt_geglu_fwd", "udt_geglu_bwd"])
def _geglu(b):
    O, L, lib, P = _mods()
    ag = b.inp(_rand((3, 80), 161, 1.5).bfloat16(), name="ag")
    dy = b.inp(_rand((3, 40), 162).bfloat16(), name="dy")
    out, dag = b.out((3, 40), BF16, name="out"), b.out((3, 80), BF16, name="dag")
    _chk(lib.udt_geglu_fwd(_p(ag), _p(out), 3, 40, O._stream()), "udt_geglu_fwd")
    _chk(lib.udt_geglu_bwd(_p(ag), _p(dy), _p(dag), 3, 40, O._stream()), "udt_geglu_bwd")
    return {"out": out, "dag": dag}


@case("sum2x2 B 1 H 3 W 5 C 8", ["udt_sum2x2_bf16"])
def _sum2x2(b):
    O, L, lib, P = _mods()
    dx = b.out((1, 3, 5, 8), BF16, name="dx")
    _chk(lib.udt_sum2x2_bf16(_p(b.inp(_rand((1, 6, 10, 8), 163).bfloat16(), name="dy")), _p(dx), 1, 3, 5, 8, O._stream()), "udt_sum2x2_bf16")
    return {"dx": dx}


@case("center_tokens B 3 L 12 and L 1, D 300", ["udt_center_tokens"])
def _center(b):
    O, L, lib, P = _mods()
    res = {}
    for Lc in (12, 1):
        out = b.out((3, Lc, 300), BF16, name=f"out L{Lc}")
        _chk(lib.udt_center_tokens(_p(b.inp(_rand((3, Lc, 300), 164, 1.0, 2.0), name="x")), _p(out), 3, Lc, 300, O._stream()), "udt_center_tokens")
        res[f"out L{Lc}"] = out
    return res


@case("transpose R 70 C 72 ld 80 Rp 128: columns >= R exact zeros", ["udt_transpose_bf16"])
def _transpose(b):
    O, L, lib, P = _mods()
    out = b.out((72, 128), BF16, name="out")
    src = b.inp(_rand((70, 72), 165).bfloat16(), ld=80, name="in")
    _chk(lib.udt_transpose_bf16(_p(src), _p(out), 70, 72, src.stride(0), 128, O._stream()),
         "udt_transpose_bf16")
    assert bool((fp.bits(out[:, 70:]) == 0).all()), "columns >= R are not exact (+0) zeros"
    return {"out": out}


@case("reduce_rows_f32 P 3 n 257, overwrite and accumulate", ["udt_reduce_rows_f32"])
def _reduce_rows(b):
    O, L, lib, P = _mods()
    src = b.inp(_rand((3, 257), 166), name="in")
    out = b.out((257,), F32, name="out")
    _chk(lib.udt_reduce_rows_f32(_p(src), _p(out), 3, 257, 0, O._stream()), "udt_reduce_rows_f32")
    acc = b.inout(_rand((257,), 167), name="out (accumulate)")
    _chk(lib.udt_reduce_rows_f32(_p(src), _p(acc), 3, 257, 1, O._stream()), "udt_reduce_rows_f32 accumulate")
    return {"out": out, "acc": acc}


@case("colsum rows 70 C 72, partials exact", ["udt_colsum_bf16"])
def _colsum(b):
    O, L, lib, P = _mods()
    part = b.scratch(lib.udt_colparts(70) * 72 * 4, name="colsum partials")
    out = b.out((72,), F32, name="out")
    _chk(lib.udt_colsum_bf16(_p(b.inp(_rand((70, 72), 168).bfloat16(), name="x")), _p(part), _p(out), 70, 72, O._stream()), "udt_colsum_bf16")
    return {"out": out}


@case("ln_param_grad rows 70 C 320, partials exact", ["udt_ln_param_grad"])
def _ln_pg(b):
    O, L, lib, P = _mods()
    part = b.scratch(lib.udt_colparts(70) * 2 * 320 * 4, name="ln_param_grad partials")
    out = b.out((2, 320), F32, name="dgamma_dbeta")
    _chk(lib.udt_ln_param_grad(_p(b.inp(_rand((70, 320), 169, 2.0, 0.5).bfloat16(), name="x")), _p(b.inp(_rand((70, 320), 170).bfloat16(), name="dy")),
                               _p(part), _p(out), 70, 320, 1e-5, O._stream()), "udt_ln_param_grad")
    return {"out": out}


@case("wgrad (1000,648,72) ldy/ldx wider, partials exact", ["udt_wgrad_bf16"])
def _wgrad(b):
    O, L, lib, P = _mods()
    R, N, K = 1000, 648, 72
    S = lib.udt_wgrad_splits(R, N, K)
    assert S > 1
    part = b.scratch(S * N * K * 4, name=f"wgrad partials ({S} splits)")
    dw = b.out((N, K), F32, name="dw")
    dy, x = b.inp(_rand((R, N), 171).bfloat16(), ld=N + 8, name="dy"), b.inp(_rand((R, K), 172).bfloat16(), ld=K + 8, name="x")
    _chk(lib.udt_wgrad_bf16(_p(dy), _p(x), _p(dw), _p(part), R, N, K, dy.stride(0), x.stride(0), O._stream()), "udt_wgrad_bf16")
    return {"dw": dw}


@case("attn_bwd B 1 H 5 n 40: lse / dsum exact, dq|dk|dv slices of one guarded buffer", ["udt_attn_bwd"])
def _attn_bwd(b):
    O, L, lib, P = _mods()
    B, H, n = 1, 5, 40
    Cc = H * 64
    qkv_t = _rand((B, n, 3 * Cc), 173).bfloat16()
    qkv = b.inp(qkv_t, ld=3 * Cc + 64, name="q|k|v")
    q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
    qf, kf, vf = (t.float().reshape(B, n, H, 64).permute(0, 2, 1, 3) for t in (q, k, v))
    o_t = (torch.softmax(qf @ kf.transpose(-1, -2) * 0.125, dim=-1) @ vf).permute(0, 2, 1, 3).reshape(B, n, Cc).bfloat16()
    o = b.inp(o_t, ld=Cc + 64, name="o")
    d_o = b.inp(_rand((B, n, Cc), 174, 0.1).bfloat16(), ld=Cc + 64, name="d_o")          # (o and d_o share ldo)
    dqkv = b.out((B, n, 3 * Cc), BF16, ld=3 * Cc + 64, name="dq|dk|dv")
    lse, dsum = b.scratch(B * H * n * 4, name="lse_ws"), b.scratch(B * H * n * 4, name="dsum_ws")
    _chk(lib.udt_attn_bwd(_p(q), _p(k), _p(v), _p(o), _p(d_o), _p(dqkv[..., :Cc]), _p(dqkv[..., Cc:2 * Cc]), _p(dqkv[..., 2 * Cc:]), _p(lse),
                          _p(dsum), B, H, n, qkv.stride(1), o.stride(1), dqkv.stride(1), 0.125, O._stream()), "udt_attn_bwd")
    return {"dqkv": dqkv, "lse": lse, "dsum": dsum}


def _xattn_bwd_operands(b, B, H, nq, Lc, seed=175):
    Cc = H * 64
    kv = b.inp(_rand((B, Lc, 2 * Cc), seed).bfloat16(), ld=2 * Cc + 64, name="k|v")
    q = b.inp(_rand((B, nq, Cc), seed + 1).bfloat16(), name="q")
    sim = _rand((B * H, nq, Lc), seed + 2, 2.0)
    probs = b.inp(torch.softmax(sim, dim=-1) if Lc > 1 else torch.sigmoid(sim), name="probs")
    d_p = b.inp(_rand((B * H, nq, Lc), seed + 3), name="d_probs")
    d_o = b.inp(_rand((B, nq, Cc), seed + 4).bfloat16(), ld=Cc + 64, name="d_o")
    return Cc, kv, q, probs, d_p, d_o


def _xattn_bwd_case(Lc):
    def fn(b):
        O, L, lib, P = _mods()
        B, H, nq = 1, 5, 70
        Cc, kv, q, probs, d_p, d_o = _xattn_bwd_operands(b, B, H, nq, Lc)
        dq = b.out((B, nq, Cc), BF16, ld=Cc + 64, name="dq")
        _chk(lib.udt_xattn_bwd(_p(kv[..., :Cc]), _p(kv[..., Cc:]), _p(probs), _p(d_p), _p(d_o), _p(dq), B, H, 64, nq, Lc, kv.stride(1),
                               d_o.stride(1), dq.stride(1), 0.125, O._stream()), "udt_xattn_bwd")
        return {"dq": dq}
    return fn


case("xattn_bwd nq 70 L 12 lddq>C", ["udt_xattn_bwd"])(_xattn_bwd_case(12))
case("xattn_bwd nq 70 L 1 lddq>C", ["udt_xattn_bwd"])(_xattn_bwd_case(1))


@case("xattn_bwd_kv nq 70 L 12, partials exact, lddkv>C", ["udt_xattn_bwd_kv"])
def _xattn_kv(b):
    O, L, lib, P = _mods()
    B, H, nq, Lc = 2, 5, 70, 12
    Cc, kv, q, probs, d_p, d_o = _xattn_bwd_operands(b, B, H, nq, Lc, seed=181)
    S = lib.udt_xattn_kv_splits(nq)
    part = b.scratch(S * B * Lc * H * 64 * 2 * 4, name=f"xattn_bwd_kv partials ({S} splits)")
    dk, dv = b.out((B, Lc, Cc), BF16, ld=Cc + 64, name="dk"), b.out((B, Lc, Cc), BF16, ld=Cc + 64, name="dv")
    _chk(lib.udt_xattn_bwd_kv(_p(q), _p(kv[..., Cc:]), _p(probs), _p(d_p), _p(d_o), _p(dk), _p(dv), _p(part), B, H, 64, nq, Lc, q.stride(1),
                              kv.stride(1), d_o.stride(1), dk.stride(1), 0.125, O._stream()), "udt_xattn_bwd_kv")
    return {"dk": dk, "dv": dv}


LL = dict(heads=5, h=6, w=10, Lc=12, seg_l=5, Hm=48, Wm=80)


@case("local_loss_tiled_hw 6x10, scratch exact", ["udt_local_loss_tiled_hw"])
def _ll_tiled_hw(b):
    O, L, lib, P = _mods()
    n_s, mb = 4, 2
    probs, mask, seg, gk = _ll_operands(b, n_s, mb, LL["heads"], LL["h"] * LL["w"], LL["Lc"], LL["seg_l"], LL["Hm"], LL["Wm"])
    scratch = b.scratch(n_s * LL["seg_l"] * 2 * 4, name="local-loss scratch")
    loss = b.inout(torch.zeros((n_s,)), name="loss")
    _chk(lib.udt_local_loss_tiled_hw(_p(probs), _p(mask), _p(seg), _p(gk), _p(loss), _p(scratch), n_s, mb, LL["heads"], LL["h"], LL["w"],
                                     LL["Lc"], LL["seg_l"], LL["Hm"], LL["Wm"], O._stream()), "udt_local_loss_tiled_hw")
    return {"loss": loss}


@case("local_loss_bwd_hw 6x10, scratch exact, d_probs guarded", ["udt_local_loss_bwd_hw"])
def _ll_bwd_hw(b):
    O, L, lib, P = _mods()
    n_s, mb = 4, 2
    probs, mask, seg, gk = _ll_operands(b, n_s, mb, LL["heads"], LL["h"] * LL["w"], LL["Lc"], LL["seg_l"], LL["Hm"], LL["Wm"])
    scratch = b.scratch(n_s * LL["seg_l"] * 2 * 4, name="local-loss scratch")
    dp = b.inout(torch.zeros((n_s * LL["heads"], LL["h"] * LL["w"], LL["Lc"])), name="d_probs")
    loss = b.inout(torch.zeros((n_s,)), name="loss")
    _chk(lib.udt_local_loss_bwd_hw(_p(probs), _p(mask), _p(seg), _p(gk), _p(dp), _p(loss), _p(scratch), n_s, mb, LL["heads"], LL["h"], LL["w"],
                                   LL["Lc"], LL["seg_l"], LL["Hm"], LL["Wm"], 0.5, O._stream()), "udt_local_loss_bwd_hw")
    assert int((dp != 0).sum()) > 0
    return {"d_probs": dp, "loss": loss}


@case("local_loss_seg_bwd_hw 6x10, scratch exact, d_probs guarded", ["udt_local_loss_seg_bwd_hw"])
def _ll_seg_hw(b):
    O, L, lib, P = _mods()
    B = 2
    probs, _, seg_mask, gk = _ll_operands(b, B, B, LL["heads"], LL["h"] * LL["w"], LL["Lc"], LL["seg_l"], LL["Hm"], LL["Wm"])
    seg = b.inp((_rand((B, LL["seg_l"], LL["Hm"], LL["Wm"]), 191) > 0.3).float(), name="seg")
    scratch = b.scratch(B * LL["seg_l"] * 4, name="local-loss (segments) scratch")
    dp = b.inout(torch.zeros((B * LL["heads"], LL["h"] * LL["w"], LL["Lc"])), name="d_probs")
    loss = b.inout(torch.zeros((B,)), name="loss")
    _chk(lib.udt_local_loss_seg_bwd_hw(_p(probs), _p(seg), _p(seg_mask), _p(gk), _p(dp), _p(loss), _p(scratch), B, LL["heads"], LL["h"], LL["w"],
                                       LL["Lc"], LL["seg_l"], LL["Hm"], LL["Wm"], 0.5, O._stream()), "udt_local_loss_seg_bwd_hw")
    return {"d_probs": dp, "loss": loss}


@case("diff_loss_grad B 2 hw 35 ld_eps 8 poisoned cpad 64: channels >= 4 exact zeros", ["udt_diff_loss_grad"])
def _diff_loss(b):
    O, L, lib, P = _mods()
    B, hw = 2, 35
    eps = b.inp(_rand((B * hw, 4), 192), ld=8, name="eps")
    noised, target = b.inp(_rand((B, 4, hw), 193, 3.0), name="noised"), b.inp(_rand((B, 4, hw), 194), name="target")
    sigma = b.inp(torch.tensor([3.2, 0.7]), name="sigma")
    d_eps, loss = b.out((B * hw, 64), BF16, name="d_eps"), b.out((B,), F32, name="loss")
    _chk(lib.udt_diff_loss_grad(_p(eps), _p(noised), _p(target), _p(sigma), _p(d_eps), _p(loss), B, hw, eps.stride(0), 64, O._stream()), "udt_diff_loss_grad")
    assert bool((fp.bits(d_eps[:, 4:]) == 0).all()), "channels >= 4 of d_eps are not exact (+0) zeros"
    return {"d_eps": d_eps, "loss": loss}


@case("adamw_f32 n 257", ["udt_adamw_f32"])
def _adamw(b):
    O, L, lib, P = _mods()
    p, m, v = b.inout(_rand((257,), 195), name="p"), b.inout(_rand((257,), 196, 0.1), name="m"), b.inout(_rand((257,), 197).abs() * 0.01, name="v")
    g = b.inp(_rand((257,), 198), name="g")
    _chk(lib.udt_adamw_f32(_p(p), _p(g), _p(m), _p(v), 257, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 3, 0.5, O._stream()), "udt_adamw_f32")
    return {"p": p, "m": m, "v": v}


@case("axpy_f32 n 257", ["udt_axpy_f32"])
def _axpy(b):
    O, L, lib, P = _mods()
    x = b.inout(_rand((257,), 199), name="x")
    _chk(lib.udt_axpy_f32(_p(x), _p(b.inp(_rand((257,), 200), name="y")), -0.37, 257, O._stream()), "udt_axpy_f32")
    return {"x": x}


# =================================================================================================== the table runs
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_footprint(env, idx):
    name, fn, _ = CASES[idx]
    try:
        _run_case(name, fn, env.dev)
    except Exception as e:                                # noqa: BLE001
        msg = str(e)
        if "HIP error" in msg or "hipError" in msg or "illegal memory access" in msg:
            # a device fault is a finding of its own: nothing more is launched on the faulted device in this session
            pytest.exit(f"GPU fault in footprint case '{name}': {msg}", returncode=3)
        raise


def test_census(env):
    """no silent downgrading: every case that ran is bit-equal unless COMPARED names it, with its reason"""
    assert set(SEEN["compared"]) <= set(COMPARED)
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)
    if len(SEEN["bit_equal"]) + len(SEEN["compared"]) == len(CASES):           # (the whole table ran)
        assert len(SEEN["compared"]) == len(COMPARED)
    print(f"footprint: {len(SEEN['bit_equal'])} cases bit-equal, {len(SEEN['compared'])} compared by bound, {len(COMPARED)} named")


# =================================================================================================== float64 references of the ops without one
def _rel(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300)).item()


def test_axpy_vs_float64(env):
    """x + a y is one fused multiply-add: |got - ref| <= 2^-23 |ref| (half an ulp of the result, doubled for the fp32 rounding of ref)"""
    x, y, a = _rand((257,), 199), _rand((257,), 200), -0.37
    got = env.O.axpy_(x.to(env.dev), y.to(env.dev), a).cpu().double()
    ref = x.double() + float(torch.tensor(a, dtype=F32)) * y.double()
    err = (got - ref).abs()
    print(f"axpy: max |err| / |ref| {float((err / ref.abs().clamp_min(1e-300)).max()):.3e} (bound {2.0 ** -23:.3e})")
    assert bool((err <= 2.0 ** -23 * ref.abs()).all())


@pytest.mark.parametrize("Lc", [1, 12])
def test_center_tokens_vs_float64(env, Lc):
    """bf16 rounding of the result (2^-8 relative: half an ulp of 8 significant bits, doubled) plus the fp32 mean of at most 16 terms
    and the fp32 subtraction (2^-20 of max |x|)"""
    x = _rand((3, Lc, 300), 164, 1.0, 2.0)
    got = env.O.center_tokens(x.to(env.dev)).cpu().double()
    ref = x.double() - x.double().mean(dim=1, keepdim=True)
    err = (got - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * float(x.abs().max())
    print(f"center_tokens L {Lc}: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("rows", [5, 301])
def test_layernorm_bwd_ragged_rows_vs_float64(env, rows):
    """four rows per workgroup: 5 and 301 leave a tail of one row; TOL_OP over the tensor AND per row, so that one wrong tail row
    cannot hide in the tensor-wide RMS"""
    Cc = 320
    x, dy, add = _rand((rows, Cc), 151, 2.0, 0.5).bfloat16(), _rand((rows, Cc), 152).bfloat16(), _rand((rows, Cc), 153).bfloat16()
    gamma = _rand((Cc,), 154, 0.2, 1.0)
    with torch.enable_grad():
        t = x.double().requires_grad_(True)
        (ref,) = torch.autograd.grad((F.layer_norm(t, (Cc,), gamma.double(), None, 1e-5) * dy.double()).sum(), [t])
    for ad in (None, add):
        got = env.O.layer_norm_bwd(x.to(env.dev), dy.to(env.dev), gamma.to(env.dev), 1e-5, add=None if ad is None else ad.to(env.dev))
        want = ref if ad is None else ref + ad.double()
        row_rel = (got.double().cpu() - want).pow(2).mean(dim=1).sqrt() / want.pow(2).mean(dim=1).sqrt()
        print(f"layernorm_bwd rows {rows} add {ad is not None}: rel_rms {_rel(got, want):.3e}, worst row {float(row_rel.max()):.3e} (tol {TOL_OP})")
        assert _rel(got, want) <= TOL_OP
        assert float(row_rel.max()) <= TOL_OP, f"row {int(row_rel.argmax())} is off: {float(row_rel.max()):.3e}"


def test_geglu_ragged_vs_float64(env):
    """rows 3, inner 40: 15 vectors of 8 in one partly filled workgroup"""
    ag, dy = _rand((3, 80), 161, 1.5).bfloat16(), _rand((3, 40), 162).bfloat16()
    with torch.enable_grad():
        t = ag.double().requires_grad_(True)
        a, gt = t.chunk(2, dim=-1)
        y = a * F.gelu(gt)
        (ref,) = torch.autograd.grad((y * dy.double()).sum(), [t])
    r_f, r_b = _rel(env.O.geglu(ag.to(env.dev)), y.detach()), _rel(env.O.geglu_bwd(ag.to(env.dev), dy.to(env.dev)), ref)
    print(f"geglu 3x40: forward rel_rms {r_f:.3e}, backward {r_b:.3e} (tol {TOL_OP})")
    assert r_f <= TOL_OP and r_b <= TOL_OP


def test_sum2x2_ragged_vs_float64(env):
    """B 1, H 3, W 5, C 8: odd map sides, one vector per pixel"""
    dy = _rand((1, 6, 10, 8), 163).bfloat16()
    ref = dy.double().reshape(1, 3, 2, 5, 2, 8).sum(dim=(2, 4))
    r = _rel(env.O.sum2x2(dy.to(env.dev)), ref)
    print(f"sum2x2 3x5: rel_rms {r:.3e} (tol {TOL_OP})")
    assert r <= TOL_OP
