"""Thin torch-tensor front end over the C ABI (device pointers + the current HIP stream).

torch is used for device memory and stream plumbing only; every computation below is a launch into
libudt_kernels.so.  All functions raise if a tensor is not on a GPU — there is no CPU path.

Every wrapper reads "check, allocate, one ``L.check(lib.udt_…)``".  What several of them share has one home each:
  _drop_sidecars               the sidecar rule (``out.gn_stats`` / ``out.mx8``): whoever overwrites a tensor drops both
  run_gemm                     the stream-K workspace of every descriptor launch (udt_gemm, udt_gn_silu_conv3x3_fwd, udt_ln_gemm_fwd)
  _strides                     row strides, then batch strides of [B, N, *] row views (the flash / masked attention argument tails)
  _masks                       additive mask + key-padding mask of masked_attention / masked_attention_bwd
  _count_gemm / _count_attn    the WORK_COUNTER amounts bench.py reads
  _ll_dims / _ll_scratch       checks and scratch of the local_loss_* wrappers
  _nchw4 / _multistep_coefs    fp32 NCHW operand check and udt_multistep_coefs of the sampler steps
  conv_out_hw                  a convolution's output size (defined in packing.py: it launches nothing)
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from typing import NamedTuple, Optional, Sequence

import torch

from . import lib as L
from .packing import conv_out_hw  # noqa: F401  (host arithmetic, no launch: kept with the layout helpers, reached as ops.conv_out_hw)

# ---------------------------------------------------------------------------------------- launch context
# The stream-K kernels need (a) a workspace whose first 4 KiB (slab flags + error word) are zero between launches
# and that no concurrent stream shares, and (b) the number of launch streams sharing the device (``cu_share``: all
# their workgroups must be resident).  Both are properties of the CALLER's launch stream, so they travel in a
# thread-local context that ``gemm_desc`` / ``run_gemm`` read — the C ABI itself keeps no such state
# (udt_gemm_desc.cu_share, caller-owned workspace).
WORKSPACE_BYTES = 96 << 20      # >= 256 workgroups x (256 x 160) fp32 slab + header: covers every plan of the library


class Workspace:
    """A stream-K workspace owned by whoever launches on one stream (a sampling runner, a captured graph): allocated
    with it, passed explicitly, freed with it, never regrown while launches or captured graphs may reference it."""

    def __init__(self, device, nbytes: int = WORKSPACE_BYTES):
        if torch.device(device).type != "cuda":
            raise L.UdtError("udifftext_amd workspaces live on the GPU (no CPU fallback)")
        # zero-initialised: the kernels keep 'slab ready' flags in the first 4 KiB and restore them to 0
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)

    def check(self, stream: Optional[int] = None) -> None:
        """synchronise ``stream`` (default: current) and raise UdtError if a launch on this workspace timed out"""
        L.check(L.load().udt_check_async_error(self.buf.data_ptr(), self.buf.numel(), _stream() if stream is None else stream),
                "udt_check_async_error")


class _Ctx(threading.local):
    cu_share = 1
    workspace: Optional[Workspace] = None


_ctx = _Ctx()
_default_ws: dict = {}


@contextlib.contextmanager
def launch_context(cu_share: Optional[int] = None, workspace: Optional[Workspace] = None):
    """launches issued inside run with this CU share / on this workspace (thread-local, re-entrant)"""
    prev = (_ctx.cu_share, _ctx.workspace)
    if cu_share is not None:
        _ctx.cu_share = max(1, int(cu_share))
    if workspace is not None:
        _ctx.workspace = workspace
    try:
        yield
    finally:
        _ctx.cu_share, _ctx.workspace = prev


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise L.UdtError("udifftext_amd ops need device tensors (no CPU fallback)")
    return t.data_ptr()


def _ws(nbytes: int, device) -> torch.Tensor:
    ws = _ctx.workspace
    if ws is None:
        # eager callers without a context: one default workspace per (device, stream) — concurrent streams must not
        # share the flags and slabs.  Fixed size, so a buffer a captured graph references is never replaced.
        key = (device.type, device.index, _stream())
        ws = _default_ws.get(key)
        if ws is None:
            ws = _default_ws[key] = Workspace(device)
    if ws.buf.numel() < nbytes:
        raise L.UdtError(f"stream-K workspace of {ws.buf.numel()} bytes is too small for this launch ({nbytes})")
    return ws.buf


def check_async_errors() -> None:
    """check every default (per-stream) workspace — tests and eager callers; runners check their own"""
    for (_, _, stream), ws in list(_default_ws.items()):
        ws.check(stream)


# optional algorithmic work accounting for bench.py's roofline objects: {"gemm": flops, "gemm_bytes": bytes, "attn": ...}
# (2*M*N*K per GEMM launch, 4*B*H*Nq*Nk*D per flash-attention launch; operands + result once for the bytes)
WORK_COUNTER: Optional[dict] = None


def count_work(kind: str, amount: float) -> None:
    if WORK_COUNTER is not None:
        WORK_COUNTER[kind] = WORK_COUNTER.get(kind, 0.0) + amount


def _bf16(t: torch.Tensor) -> None:
    if t.dtype != torch.bfloat16:
        raise ValueError(f"expected bf16 tensor, got {t.dtype}")


# -------------------------------------------------------------------------------------------- sidecars
# A producer hangs what its epilogue emitted next to its result on the result tensor: the column statistics (``out.gn_stats``) and
# the MX8 twin (``out.mx8``).  A consumer trusts what it finds there, so: an op ATTACHES only what its own launch emits, and
# every op DROPS both sidecars of a caller-visible bf16 tensor it is about to overwrite (an ``out=`` argument, the operand of an
# in-place op; a fresh allocation carries none).  A view is a new tensor object: hipnn.carry_stats / carry_mx8 hand them over.
class GnStats(NamedTuple):
    """column statistics a producer's epilogue emitted for its output (udt_gemm_desc.colstats): fp32
    [slots, C, 2] = per-(row slot, channel) (sum, sum of squares); a sample owns ``slots_per_sample`` consecutive slots"""
    data: torch.Tensor
    slots_per_sample: int


def gn_stats_of(t: Optional[torch.Tensor]) -> Optional[GnStats]:
    return getattr(t, "gn_stats", None) if t is not None else None


class Mx8Act(NamedTuple):
    """an activation in the MX8 form the UDT_GEMM_MX8 consumers read (BASELINE config #5): OCP e4m3 elements + one E8M0 scale
    per 32 consecutive columns of a row, written by the PRODUCING kernel's epilogue (udt_gemm_desc.q8_out, udt_tattn_fused_q8,
    udt_attn_rowv_q8_fwd, udt_gn_apply_scsh_q8) — never by a pass of its own.
      data  uint8 [M, K]            e4m3 bytes
      scale int32 [K / 128, M]      byte j of dword (t, m) = scale of columns [128 t + 32 j, + 32) of row m
      stats fp32 [P, M, 2] or None  partial (sum, sum of squares) of every row — for a LayerNorm-folded consumer"""
    data: torch.Tensor
    scale: torch.Tensor
    stats: Optional[torch.Tensor] = None


def mx8_of(t: Optional[torch.Tensor]) -> Optional[Mx8Act]:
    """the MX8 twin a producer attached to its bf16 result (``out.mx8``), if any"""
    return getattr(t, "mx8", None) if t is not None else None


def _drop_sidecars(t: torch.Tensor) -> torch.Tensor:
    """``t`` is about to be overwritten: what an earlier launch into it left on it describes data that is gone (-> t)"""
    attrs = vars(t)
    attrs.pop("gn_stats", None)
    attrs.pop("mx8", None)
    return t


# ------------------------------------------------------------------------------------------------ GEMM
def gemm_desc(**kw) -> L.GemmDesc:
    d = L.GemmDesc()
    d.batch = 1
    d.alpha = 1.0
    d.cu_share = _ctx.cu_share
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def run_gemm(d: L.GemmDesc, device, fused_gn: bool = False, entry: str = "udt_gemm", check: bool = True) -> int:
    """launch ``entry`` (fused_gn: udt_gn_silu_conv3x3_fwd) on ``d`` with the stream-K workspace its plan asks for.
    check=False hands the status back for the caller to explain"""
    if fused_gn:
        entry = "udt_gn_silu_conv3x3_fwd"
    lib = L.load()
    need = lib.udt_gemm_workspace_bytes(C.byref(d))
    ws_ptr, ws_bytes = None, 0
    if need:
        ws = _ws(need, device)
        ws_ptr, ws_bytes = ws.data_ptr(), ws.numel()
    rc = getattr(lib, entry)(C.byref(d), ws_ptr, ws_bytes, _stream())
    if check:
        L.check(rc, entry)
    return rc


def _count_gemm(kind: str, flops: float, nbytes: Optional[float] = None) -> None:
    """one GEMM launch for bench.py's roofline (call under ``if WORK_COUNTER is not None``); kind = "gemm" | "gemm_fp8";
    nbytes = None: the launch counts no bytes"""
    count_work(kind, flops)
    if nbytes is not None:
        count_work(kind + "_bytes", nbytes)
    count_work(kind + "_launches", 1.0)


GN_STRIP = True       # one-launch strip GroupNorm where the shape allows (tests switch it off to compare with the two-kernel path)


def _attach_colstats(d: L.GemmDesc, out: torch.Tensor, n_cols: int, rows_per_batch: int) -> bool:
    """ask the library whether this problem can emit column statistics; if so allocate them and point the
    descriptor at them (the tensor rides on ``out.gn_stats``)"""
    lib = L.load()
    rows = lib.udt_gemm_colstats_rows(C.byref(d))
    if rows <= 0:
        return False
    slots = lib.udt_gemm_colstats_slots(C.byref(d))
    st = torch.empty((slots, n_cols, 2), dtype=torch.float32, device=out.device)
    d.colstats = st.data_ptr()
    out.gn_stats = GnStats(st, rows_per_batch // rows)
    return True


def _mx8_alloc(M: int, cols: int, device) -> Mx8Act:
    return Mx8Act(torch.empty((M, cols), dtype=torch.uint8, device=device),
                  torch.empty(((cols + 127) // 128, M), dtype=torch.int32, device=device))


def _attach_q8(d: L.GemmDesc, M: int, cols: int, device, rowstats: bool, fixed: Optional[tuple] = None) -> Optional[Mx8Act]:
    """ask the library whether this launch can also emit its result as an MX8 activation (+ partial row statistics); if so
    allocate the buffers and point the descriptor at them.  fixed = (first column, multiplier): columns from there on are written
    with that fixed scale instead of block scales (udt_gemm_desc.q8_fixed_col)"""
    q = _mx8_alloc(M, cols, device)
    d.q8_out, d.q8_scale, d.ld_q8 = q.data.data_ptr(), q.scale.data_ptr(), cols
    if fixed is not None:
        d.q8_fixed_col, d.q8_fixed_mul = int(fixed[0]), float(fixed[1])
    lib = L.load()
    parts = lib.udt_gemm_rowstat_parts(C.byref(d)) if rowstats else 0
    if not lib.udt_gemm_q8_ok(C.byref(d)) or (rowstats and parts <= 0):
        d.q8_out, d.q8_scale, d.ld_q8, d.q8_fixed_col = None, None, 0, 0
        return None
    if rowstats:
        st = torch.empty((parts, M, 2), dtype=torch.float32, device=device)
        d.rowstat_out = st.data_ptr()
        q = Mx8Act(q.data, q.scale, st)
    return q


def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, rowvec: Optional[torch.Tensor] = None, rows_per_batch: int = 0,
           flags: int = 0, alpha: float = 1.0, n_out: Optional[int] = None, colstats: bool = False,
           emit_q8: bool = False, emit_rowstats: bool = False) -> torch.Tensor:
    """out[M, N] = epilogue(x[M, K] @ w[N, K]^T).  x may be a strided row view (last dim contiguous).
    colstats: also emit the per-column partial sums of the output (``out.gn_stats``, None when the plan cannot) —
    the GroupNorm statistics of the next layer; needs rows_per_batch (rows of one sample)."""
    _bf16(x); _bf16(w)
    K = x.shape[-1]
    x2 = x.reshape(-1, K) if x.is_contiguous() else x
    assert x2.dim() == 2 and x2.stride(1) == 1
    M = x2.shape[0]
    N = w.shape[0] if n_out is None else n_out
    assert w.shape[1] == K and w.is_contiguous()
    n_cols = N // 2 if (flags & L.GEMM_GEGLU) else N
    if out is None:
        dt = torch.float32 if (flags & L.GEMM_OUT_F32) else torch.bfloat16
        if flags & L.GEMM_TRANSPOSED:
            assert rows_per_batch > 0
            out = torch.empty((M // rows_per_batch, N, rows_per_batch), dtype=dt, device=x.device)
        else:
            out = torch.empty((M, n_cols), dtype=dt, device=x.device)
    else:
        _drop_sidecars(out)
    ldo = out.stride(0) if not (flags & L.GEMM_TRANSPOSED) else 0
    d = gemm_desc(a=_ptr(x2), w=_ptr(w), bias=_ptr(bias), residual=_ptr(residual), rowvec=_ptr(rowvec), out=_ptr(out),
                  M=M, N=N, K=K, lda=x2.stride(0), ldo=ldo, ldr=(residual.stride(0) if residual is not None else 0),
                  rows_per_batch=rows_per_batch, ld_rowvec=(rowvec.stride(0) if rowvec is not None else 0), flags=flags,
                  alpha=alpha)
    if colstats and rows_per_batch > 0 and out.is_contiguous():
        _attach_colstats(d, out, n_cols, rows_per_batch)
    q8 = None
    if emit_q8 and not (flags & (L.GEMM_OUT_F32 | L.GEMM_TRANSPOSED | L.GEMM_GEGLU)) and d.colstats is None and rowvec is None:
        q8 = _attach_q8(d, M, n_cols, x.device, emit_rowstats)      # (None: the plan has no emitting epilogue)
    run_gemm(d, x.device)
    if q8 is not None:
        out.mx8 = q8
    if WORK_COUNTER is not None:
        _count_gemm("gemm", 2.0 * M * N * K, 2.0 * (M * K + N * K) + out.numel() * out.element_size()
                    + (2.0 * M * n_cols if residual is not None else 0.0))
    return out


def linear_mx8(x: Mx8Act, wq: torch.Tensor, colscale: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
               out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, rows_per_batch: int = 0,
               flags: int = 0, n_out: Optional[int] = None, colstats: bool = False, emit_q8: bool = False,
               emit_rowstats: bool = False, ln_c: Optional[torch.Tensor] = None, ln_s: Optional[torch.Tensor] = None,
               eps: float = 1e-5, want_bf16: bool = True, q8_fixed: Optional[tuple] = None):
    """out[M, N] (bf16) = epilogue(dequant(x) @ dequant(wq)^T) on the MX8 path (UDT_GEMM_MX8): x an Mx8Act, wq e4m3 [N, K]
    with per-output-channel fp32 scales.  ln_c / ln_s: the GEMM is LayerNorm-folded (packing.pack_ln_linear_mx8; x.stats holds
    the row statistics its producer emitted).  emit_q8: the result again as an Mx8Act (``out.mx8``; with GEGLU and
    want_bf16=False ONLY that — the function then returns the Mx8Act)."""
    xq = x.data
    assert xq.dtype == torch.uint8 and wq.dtype == torch.uint8 and xq.is_contiguous() and wq.is_contiguous()
    M, K = xq.shape
    N = wq.shape[0] if n_out is None else n_out
    assert wq.shape[1] == K and K % 128 == 0 and colscale.dtype == torch.float32 and colscale.numel() >= N
    assert x.scale.dtype == torch.int32 and x.scale.shape == (K // 128, M) and x.scale.is_contiguous()
    geglu = bool(flags & L.GEMM_GEGLU)
    n_cols = N // 2 if geglu else N
    only_q8 = emit_q8 and not want_bf16
    if out is not None:
        _drop_sidecars(out)
    elif not only_q8:
        out = torch.empty((M, n_cols), dtype=torch.bfloat16, device=xq.device)
    d = gemm_desc(a=_ptr(xq), w=_ptr(wq), bias=_ptr(ln_c if ln_c is not None else bias), residual=_ptr(residual),
                  out=_ptr(out), M=M, N=N, K=K, lda=K, ldo=(out.stride(0) if out is not None else 0),
                  ldr=(residual.stride(0) if residual is not None else 0), rows_per_batch=rows_per_batch,
                  flags=flags | L.GEMM_MX8, colscale=_ptr(colscale), a_scale=_ptr(x.scale))
    if ln_s is not None:
        if x.stats is None:
            raise L.UdtError("linear_mx8: a LayerNorm-folded MX8 GEMM needs the row statistics of its input (Mx8Act.stats)")
        assert x.stats.dtype == torch.float32 and x.stats.is_contiguous() and x.stats.shape[1:] == (M, 2)
        d.ln_colsum, d.ln_eps = _ptr(ln_s), eps
        d.rowstat_in, d.rowstat_in_parts = _ptr(x.stats), x.stats.shape[0]
    if out is not None and colstats and rows_per_batch > 0 and out.is_contiguous():
        _attach_colstats(d, out, n_cols, rows_per_batch)
    q8 = None
    if emit_q8:
        q8 = _attach_q8(d, M, n_cols, xq.device, emit_rowstats and not geglu, fixed=q8_fixed)
        if q8 is None:
            raise L.UdtError(f"udt_gemm has no MX8-emitting plan for M={M} N={N} K={K} flags={flags:#x}")
    run_gemm(d, xq.device)
    if WORK_COUNTER is not None:
        _count_gemm("gemm_fp8", 2.0 * M * N * K)
    if only_q8:
        return q8
    if q8 is not None:
        out.mx8 = q8
    return out


def ln_linear(x: torch.Tensor, w_folded: torch.Tensor, c: torch.Tensor, s: torch.Tensor, *, eps: float = 1e-5,
              out: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, flags: int = 0,
              n_out: Optional[int] = None, emit_q8: bool = False, want_bf16: bool = True, q8_fixed: Optional[tuple] = None,
              q8_or_none: bool = False):
    """out = epilogue(LayerNorm(x) @ W^T + b) in ONE launch (udt_ln_gemm_fwd): x holds the raw rows, (w_folded, c, s) come
    from packing.pack_ln_linear; the row statistics are taken inside the GEMM (reference attention.py:310-339).
    q8_or_none: with emit_q8, return None (nothing launched) instead of raising when the library has no emitting plan for the shape
    (row-resident kernel switched off through udt_debug_set / UDT_LEAN, unaligned rows) — the caller then takes its bf16 path."""
    _bf16(x); _bf16(w_folded)
    K = x.shape[-1]
    x2 = x.reshape(-1, K) if x.is_contiguous() else x
    assert x2.dim() == 2 and x2.stride(1) == 1 and w_folded.shape[1] == K and w_folded.is_contiguous()
    M = x2.shape[0]
    N = w_folded.shape[0] if n_out is None else n_out
    n_cols = N // 2 if (flags & L.GEMM_GEGLU) else N
    only_q8 = emit_q8 and not want_bf16
    if out is not None:
        _drop_sidecars(out)
    elif not only_q8:
        out = torch.empty((M, n_cols), dtype=torch.bfloat16, device=x.device)
    d = gemm_desc(a=_ptr(x2), w=_ptr(w_folded), bias=_ptr(c), residual=_ptr(residual), out=_ptr(out), M=M, N=N, K=K,
                  lda=x2.stride(0), ldo=(out.stride(0) if out is not None else 0),
                  ldr=(residual.stride(0) if residual is not None else 0), flags=flags, ln_colsum=_ptr(s), ln_eps=eps)
    q8 = None
    if emit_q8:
        # (the row-resident K = 320 kernel's emitting epilogue: q|k|v for the e4m3 self-attention of config #5 at the 64x64 level)
        q8 = _attach_q8(d, M, n_cols, x.device, False, fixed=q8_fixed)
        if q8 is None:
            if q8_or_none:
                return None
            raise L.UdtError(f"udt_ln_gemm_fwd has no MX8-emitting plan for M={M} N={N} K={K}")
    rc = run_gemm(d, x.device, entry="udt_ln_gemm_fwd", check=False)
    if rc in (-1, -2) and x.is_cuda:            # UDT_ERR_BAD_SHAPE / UDT_ERR_BAD_ARG
        # the LayerNorm-folded form exists on the lean kernels only: a problem their plan declines (lean kernels switched off at
        # run time through udt_debug_set, unaligned out / residual pointers, > 2 GiB operands) says so loudly instead of
        # surfacing as a bare status code from inside a transformer block
        raise L.UdtError(f"udt_ln_gemm_fwd declined M={M} N={N} K={K} flags={flags:#x} (status {rc}): the LayerNorm-folded GEMM "
                         "needs the lean kernel family (UDT_LEAN / udt_debug_set('lean') != 0) and 16-byte aligned operands; "
                         "set UDT_LN_GEMM=0 to run layernorm + GEMM instead")
    L.check(rc, "udt_ln_gemm_fwd")
    if WORK_COUNTER is not None:
        _count_gemm("gemm", 2.0 * M * N * K, 2.0 * (M * K + N * K) + (2.0 if out is not None else 0.0) * M * n_cols
                    + (1.0 * M * n_cols if q8 is not None else 0.0) + (2.0 * M * n_cols if residual is not None else 0.0))
    if only_q8:
        return q8
    if q8 is not None:
        out.mx8 = q8
    return out


def bmm_nt(a: torch.Tensor, w: torch.Tensor, *, out: Optional[torch.Tensor] = None, alpha: float = 1.0) -> torch.Tensor:
    """Batched out[b] = a[b] @ w[b]^T with a [B, M, K], w [B, N, K] bf16 (row-strided views allowed)."""
    _bf16(a); _bf16(w)
    B, M, K = a.shape
    N = w.shape[1]
    assert a.stride(2) == 1 and w.stride(2) == 1 and w.shape[0] == B and w.shape[2] == K
    out = _drop_sidecars(out) if out is not None else torch.empty((B, M, N), dtype=torch.bfloat16, device=a.device)
    d = gemm_desc(a=_ptr(a), w=_ptr(w), out=_ptr(out), M=M, N=N, K=K, lda=a.stride(1), ldw=w.stride(1),
                  ldo=out.stride(1), batch=B, stride_a=a.stride(0), stride_w=w.stride(0), stride_out=out.stride(0),
                  alpha=alpha)
    run_gemm(d, a.device)
    if WORK_COUNTER is not None:
        _count_gemm("gemm", 2.0 * B * M * N * K, 2.0 * B * (M * K + N * K + M * N))
    return out


def conv2d(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *, ksize: int = 3, stride: int = 1,
           pad: Optional[tuple] = None, upsample: bool = False, x2: Optional[torch.Tensor] = None,
           out_hw: Optional[tuple] = None, residual: Optional[torch.Tensor] = None,
           rowvec: Optional[torch.Tensor] = None, flags: int = 0, n_out: Optional[int] = None,
           out: Optional[torch.Tensor] = None, colstats: bool = False, in_scsh: Optional[torch.Tensor] = None,
           in_act: int = 0, probe_in_scsh: bool = False, w_up4: Optional[torch.Tensor] = None):
    """NHWC convolution as implicit GEMM.  x [B,H,W,C1] (+ optional x2 [B,H,W,C2], channel concat) bf16;
    w [N, ksize*ksize*(C1+C2)] packed tap-major.  Returns [B,Hout,Wout,N].
    w_up4 (with upsample): the same weights in the phase layout [4, N, 4*C1] (packing.pack_conv_up4) — the launch runs as four 2x2
    phase convolutions of the low-resolution map where the library serves the shape (udt_gemm_up4_ok), else on ``w`` as without it;
    in_scsh / in_act: GroupNorm scale/shift table (gn_finalize) + activation applied to the input on the staged patch
    (udt_gn_silu_conv3x3_fwd); colstats: emit the output's column statistics (``out.gn_stats``);
    probe_in_scsh: no launch — returns whether the library would accept in_scsh for this problem."""
    _bf16(x); _bf16(w)
    assert x.is_contiguous() and w.is_contiguous()
    B, H, W_, C1 = x.shape
    C2 = 0
    if x2 is not None:
        _bf16(x2)
        assert x2.is_contiguous() and x2.shape[:3] == x.shape[:3]
        C2 = x2.shape[3]
    if pad is None:
        pad = (ksize // 2, ksize // 2)
    Ho, Wo = conv_out_hw(H, W_, ksize, stride, pad, upsample) if out_hw is None else out_hw
    N = w.shape[0] if n_out is None else n_out
    K = ksize * ksize * (C1 + C2)
    assert w.shape[1] == K, (w.shape, K)
    M = B * Ho * Wo
    if probe_in_scsh:
        pass                                      # (nothing is written)
    elif out is None:
        dt = torch.float32 if (flags & L.GEMM_OUT_F32) else torch.bfloat16
        out = torch.empty((B, Ho, Wo, N), dtype=dt, device=x.device)
    else:
        _drop_sidecars(out)
    d = gemm_desc(a=_ptr(x), a2=_ptr(x2), w=_ptr(w), bias=_ptr(bias), residual=_ptr(residual), rowvec=_ptr(rowvec),
                  out=_ptr(out), M=M, N=N, K=K, lda=0, ldo=(out.stride(2) if out is not None else N),
                  ldr=(residual.stride(2) if residual is not None else 0),
                  Hin=H, Win=W_, C1=C1, C2=C2, Hout=Ho, Wout=Wo, ksize=ksize, stride=stride, pad_t=pad[0], pad_l=pad[1],
                  upsample=1 if upsample else 0, rows_per_batch=Ho * Wo,
                  ld_rowvec=(rowvec.stride(0) if rowvec is not None else 0), flags=flags | L.GEMM_CONV)
    if probe_in_scsh:
        return bool(L.load().udt_gemm_in_scsh_ok(C.byref(d)))
    if w_up4 is not None and upsample and ksize == 3 and x2 is None and in_scsh is None:
        _bf16(w_up4)
        assert w_up4.is_contiguous() and w_up4.dim() == 3 and w_up4.shape[0] == 4 and w_up4.shape[1] >= N and w_up4.shape[2] == 4 * C1, \
            (w_up4.shape, N, C1)
        d.upsample, d.w, d.ldw, d.stride_w = 2, _ptr(w_up4), w_up4.shape[2], w_up4.stride(0)
        if not L.load().udt_gemm_up4_ok(C.byref(d)):
            d.upsample, d.w, d.ldw, d.stride_w = 1, _ptr(w), 0, 0
    if in_scsh is not None:                       # (before the statistics probe: the plan depends on it)
        assert in_scsh.dtype == torch.float32 and in_scsh.is_contiguous() and in_scsh.numel() == B * (C1 + C2) * 2
        d.in_scsh = in_scsh.data_ptr()
        d.in_act = int(in_act)
    if colstats:
        _attach_colstats(d, out, N, Ho * Wo)
    run_gemm(d, x.device, fused_gn=in_scsh is not None)
    return out


# ------------------------------------------------------------------------------------------- attention
def _strides(*views: Optional[torch.Tensor], between: tuple = ()) -> tuple:
    """the stride tail of the attention entry points: the row strides of [B, N, *] row views, ``between``, then their batch
    strides (a view that is None: 0)"""
    return (*[0 if t is None else t.stride(1) for t in views], *between, *[0 if t is None else t.stride(0) for t in views])


def _count_attn(kind: str, flops: float, nbytes: float) -> None:
    """one attention launch for bench.py's roofline (call under ``if WORK_COUNTER is not None``); kind = "attn" | "attn_fp8" """
    count_work(kind, flops)
    count_work(kind + "_bytes", nbytes)
    count_work(kind + "_launches", 1.0)


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, scale: float,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q,k: [B, N, *] row views whose first heads*64 columns are the head-major projections (last dim
    contiguous); vt: [B, heads*64, Nk].  Returns o [B, Nq, heads*64]."""
    _bf16(q); _bf16(k); _bf16(vt)
    B, Nq = q.shape[0], q.shape[1]
    Nk = k.shape[1]
    assert q.stride(2) == 1 and k.stride(2) == 1 and vt.stride(2) == 1
    out = _drop_sidecars(out) if out is not None else torch.empty((B, Nq, heads * 64), dtype=torch.bfloat16, device=q.device)
    L.check(L.load().udt_attn_fwd(_ptr(q), _ptr(k), _ptr(vt), _ptr(out), B, heads, Nq, Nk, *_strides(q, k, vt, out), scale, _stream()),
            "udt_attn_fwd")
    if WORK_COUNTER is not None:
        _count_attn("attn", 4.0 * B * heads * Nq * Nk * 64, 2.0 * B * heads * 64 * (2 * Nq + 2 * Nk))
    return out


def attention_rowv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float,
                   out: Optional[torch.Tensor] = None, emit_q8: bool = False) -> torch.Tensor:
    """flash attention with V row-major like K: q, k, v [B, N, *] row views (e.g. the column ranges of one q|k|v
    projection) whose first heads*64 columns are the head-major projections.  Returns o [B, Nq, heads*64].
    emit_q8: o ALSO as an MX8 activation (``out.mx8``) for an e4m3 ``to_out`` (heads even)."""
    _bf16(q); _bf16(k); _bf16(v)
    B, Nq = q.shape[0], q.shape[1]
    Nk = k.shape[1]
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1 and v.shape[1] == Nk
    out = _drop_sidecars(out) if out is not None else torch.empty((B, Nq, heads * 64), dtype=torch.bfloat16, device=q.device)
    args = (_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, heads, Nq, Nk, *_strides(q, k, v, out), scale)
    if emit_q8 and heads % 2 == 0 and out.is_contiguous():
        q8 = _mx8_alloc(B * Nq, heads * 64, q.device)
        L.check(L.load().udt_attn_rowv_q8_fwd(*args, _ptr(q8.data), _ptr(q8.scale), heads * 64, _stream()), "udt_attn_rowv_q8_fwd")
        out.mx8 = q8
    else:
        L.check(L.load().udt_attn_rowv_fwd(*args, _stream()), "udt_attn_rowv_fwd")
    if WORK_COUNTER is not None:
        _count_attn("attn", 4.0 * B * heads * Nq * Nk * 64, 2.0 * B * heads * 64 * (2 * Nq + 2 * Nk))
    return out


def attention_mx8(qkv: Mx8Act, batch: int, heads: int, scale: float, v_mul: float, out: Optional[torch.Tensor] = None,
                  emit_q8: bool = False) -> torch.Tensor:
    """the same self-attention on e4m3 operands (BASELINE config #5's "fp8 attention", udt_attn_mx8_fwd): qkv is the MX8 form of
    one q|k|v projection [B * N, 3 C] whose emitting epilogue wrote the v third with the fixed multiplier v_mul
    (q8_fixed = (2 C, v_mul)).  Returns o [B, N, C] bf16 (``out.mx8``: o again as an MX8 activation, emit_q8)."""
    C_ = heads * 64
    M, ld8 = qkv.data.shape
    assert qkv.data.dtype == torch.uint8 and qkv.data.is_contiguous() and ld8 >= 3 * C_ and M % batch == 0
    assert qkv.scale.dtype == torch.int32 and qkv.scale.is_contiguous() and qkv.scale.shape == ((ld8 + 127) // 128, M)
    N = M // batch
    out = _drop_sidecars(out) if out is not None else torch.empty((batch, N, C_), dtype=torch.bfloat16, device=qkv.data.device)
    assert out.is_contiguous()
    q8 =_mx8_alloc(M, C_, qkv.data.device) if emit_q8 else None
    L.check(L.load().udt_attn_mx8_fwd(_ptr(qkv.data), _ptr(qkv.scale), _ptr(out), batch, heads, N, ld8, out.stride(1), scale,
                                      1.0 / v_mul, _ptr(q8.data) if q8 else None, _ptr(q8.scale) if q8 else None, C_, _stream()),
            "udt_attn_mx8_fwd")
    if q8 is not None:
        out.mx8 = q8
    if WORK_COUNTER is not None:
        _count_attn("attn_fp8", 4.0 * batch * heads * N * N * 64, 1.0 * batch * heads * 64 * 3 * N + 2.0 * batch * heads * 64 * N)
    return out


def attention_d512(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float,
                   out: Optional[torch.Tensor] = None, key_split: bool = True) -> torch.Tensor:
    """single-head flash attention with head_dim 512 (the VAE mid-block attention): q, k, v [B, N, 512] row views, e.g. the
    column ranges of one q|k|v projection.  Returns o [B, Nq, 512]; no [Nq, Nk] score tensor is materialised.
    ``key_split``: grids too small to fill the CUs (a single image) split the keys over workgroups and merge
    (udt_attn512_split_fwd; the library plans the split, the scratch for the partial results is allocated here)."""
    _bf16(q); _bf16(k); _bf16(v)
    B, Nq = q.shape[0], q.shape[1]
    Nk = k.shape[1]
    assert q.shape[2] == 512 and k.shape[2] == 512 and v.shape[2] == 512 and v.shape[1] == Nk
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    out = _drop_sidecars(out) if out is not None else torch.empty((B, Nq, 512), dtype=torch.bfloat16, device=q.device)
    lib = L.load()
    need = int(lib.udt_attn512_workspace_bytes(B, Nq, Nk)) if key_split else 0
    args = (_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Nq, Nk, *_strides(q, k, v, out), scale)
    if need:
        scratch = torch.empty((need,), dtype=torch.uint8, device=q.device)
        L.check(lib.udt_attn512_split_fwd(*args, _ptr(scratch), need, _stream()), "udt_attn512_split_fwd")
    else:
        L.check(lib.udt_attn512_fwd(*args, _stream()), "udt_attn512_fwd")
    if WORK_COUNTER is not None:
        _count_attn("attn", 4.0 * B * Nq * Nk * 512, 2.0 * B * 512 * (2 * Nq + 2 * Nk))
    return out


def xattention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, head_dim: int, scale: float,
               probs: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [B, Nq, heads*head_dim]; k, v row views [B, L, *] sharing one row stride; probs fp32 [B*heads, Nq, L]."""
    _bf16(q); _bf16(k); _bf16(v)
    B, Nq = q.shape[0], q.shape[1]
    Lc = k.shape[1]
    assert q.is_contiguous() or (q.stride(2) == 1 and q.stride(0) == Nq * q.stride(1))
    assert k.stride(2) == 1 and v.stride(2) == 1 and k.stride(1) == v.stride(1)
    assert k.stride(0) == Lc * k.stride(1) and v.stride(0) == Lc * v.stride(1)
    out = _drop_sidecars(out) if out is not None else torch.empty((B, Nq, heads * head_dim), dtype=torch.bfloat16, device=q.device)
    if probs is not None:
        assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.numel() == B * heads * Nq * Lc
    L.check(L.load().udt_xattn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(probs), B, heads, head_dim, Nq, Lc,
                                   q.stride(1), k.stride(1), out.stride(1), scale, _stream()), "udt_xattn_fwd")
    return out


def _masks(mask: Optional[torch.Tensor], key_padding_mask: Optional[torch.Tensor], B: int, Nq: int, Lk: int) -> tuple:
    """the masks in the form udt_mattn_fwd / udt_mattn_bwd read: additive fp32 [Nq, Lk], key padding uint8 [B, Lk], contiguous"""
    if mask is not None:
        mask = mask.float().contiguous()
        assert mask.shape == (Nq, Lk)
    if key_padding_mask is not None:
        key_padding_mask = key_padding_mask.to(torch.uint8).contiguous()
        assert key_padding_mask.shape == (B, Lk)
    return mask, key_padding_mask


def masked_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float,
                     mask: Optional[torch.Tensor] = None, key_padding_mask: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.MultiheadAttention's core for short sequences (udt_mattn_fwd): q [B, Nq, heads*D], k / v [B, Lk, *] row views
    whose first heads*D columns are the head-major projections; mask fp32 [Nq, Lk] additive; key_padding_mask
    uint8 / bool [B, Lk] (true = ignore).  D = q.shape[-1] // heads, a multiple of 8 up to 64."""
    _bf16(q); _bf16(k); _bf16(v)
    B, Nq, Cq = q.shape
    Lk = k.shape[1]
    D = Cq // heads
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    out = _drop_sidecars(out) if out is not None else torch.empty((B, Nq, heads * D), dtype=torch.bfloat16, device=q.device)
    mask, key_padding_mask = _masks(mask, key_padding_mask, B, Nq, Lk)
    L.check(L.load().udt_mattn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(mask), _ptr(key_padding_mask), B, heads, D,
                                   Nq, Lk, *_strides(q, k, v, out, between=(Lk,)), scale, _stream()), "udt_mattn_fwd")
    return out


class TattnTables(NamedTuple):
    """per-sample tables of the fused text cross-attention (udt_tattn_prepare)"""
    A: torch.Tensor          # bf16 [B, hp, C]
    sc: torch.Tensor         # fp32 [B, hp, 2]
    BmT: torch.Tensor        # bf16 [B, C, hp]

    def rows(self, begin: int, end: Optional[int] = None) -> "TattnTables":
        return TattnTables(self.A[begin:end], self.sc[begin:end], self.BmT[begin:end])


def tattn_prepare(kv: torch.Tensor, wq: torch.Tensor, wo: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, heads: int,
                  scale: float, out: Optional[TattnTables] = None) -> TattnTables:
    """kv bf16 [B, L, 2*C] (hoisted k|v of the context), wq / wo packed bf16 [C, >=C] -> tables (in place into ``out``)"""
    _bf16(kv); _bf16(wq); _bf16(wo)
    B, Lc, two_c = kv.shape
    Cc = heads * 64
    assert two_c == 2 * Cc and kv.is_contiguous() and wq.is_contiguous() and wo.is_contiguous()
    hp = L.load().udt_tattn_hp(heads)
    if out is None:
        out = TattnTables(torch.empty((B, hp, Cc), dtype=torch.bfloat16, device=kv.device),
                          torch.empty((B, hp, 2), dtype=torch.float32, device=kv.device),
                          torch.empty((B, Cc, hp), dtype=torch.bfloat16, device=kv.device))
    L.check(L.load().udt_tattn_prepare(_ptr(kv), two_c, _ptr(wq), wq.stride(0), _ptr(wo), wo.stride(0), _ptr(gamma), _ptr(beta),
                                       _ptr(out.A), _ptr(out.sc), _ptr(out.BmT), B, Lc, Cc, heads, scale, _stream()),
            "udt_tattn_prepare")
    return out


def tattn_fused(x: torch.Tensor, tables: Optional[TattnTables], bias: torch.Tensor, heads: int, zero_samples: int, eps: float,
                out: Optional[torch.Tensor] = None, emit_q8: bool = False) -> torch.Tensor:
    """x bf16 [B, N, C] -> x + t_attn(LayerNorm(x)) (+ bias); the first zero_samples samples see a zero context.
    emit_q8: the result ALSO as an MX8 activation with partial row statistics (``out.mx8``) where the library has the instance."""
    _bf16(x)
    assert x.is_contiguous()
    B, N, Cc = x.shape
    out = _drop_sidecars(out) if out is not None else torch.empty_like(x)
    assert out.is_contiguous()
    if tables is not None:
        assert tables.A.is_contiguous() and tables.sc.is_contiguous() and tables.BmT.is_contiguous() and tables.A.shape[0] == B
    parts = L.load().udt_tattn_rowstat_parts(B, N, Cc) if emit_q8 else 0
    if parts > 0:
        q = _mx8_alloc(B * N, Cc, x.device)
        q = Mx8Act(q.data, q.scale, torch.empty((parts, B * N, 2), dtype=torch.float32, device=x.device))
        L.check(L.load().udt_tattn_fused_q8(_ptr(x), _ptr(out), _ptr(tables.A) if tables else None, _ptr(tables.sc) if tables else None,
                                            _ptr(tables.BmT) if tables else None, _ptr(bias), B, N, Cc, heads, zero_samples, eps,
                                            _ptr(q.data), _ptr(q.scale), _ptr(q.stats), _stream()), "udt_tattn_fused_q8")
        out.mx8 = q
        return out
    L.check(L.load().udt_tattn_fused(_ptr(x), _ptr(out), _ptr(tables.A) if tables else None, _ptr(tables.sc) if tables else None,
                                     _ptr(tables.BmT) if tables else None, _ptr(bias), B, N, Cc, heads, zero_samples, eps, _stream()),
            "udt_tattn_fused")
    return out


def tattn_fused_maps(x: torch.Tensor, tables: TattnTables, bias: torch.Tensor, heads: int, zero_samples: int, eps: float,
                     maps: torch.Tensor, map_from: int, weight: float = 1.0, accumulate: bool = False,
                     out: Optional[torch.Tensor] = None, emit_q8: bool = False) -> torch.Tensor:
    """``tattn_fused`` (same operands, bit-identical result and sidecars) that also writes the head-mean attention maps of the samples
    >= map_from into the caller's ``maps`` fp32 [B - map_from, L, N] (udt_tattn_fused_maps): ``weight / heads * sum_h P``, stored, or
    added to what ``maps`` holds with ``accumulate``.  L = maps.shape[1] is the context length the tables were prepared for."""
    _bf16(x)
    assert x.is_contiguous()
    B, N, Cc = x.shape
    out = _drop_sidecars(out) if out is not None else torch.empty_like(x)
    assert out.is_contiguous()
    assert tables is not None and tables.A.is_contiguous() and tables.sc.is_contiguous() and tables.BmT.is_contiguous()
    assert tables.A.shape[0] == B
    assert maps.dtype == torch.float32 and maps.dim() == 3 and maps.is_contiguous() and maps.device == x.device
    assert maps.shape[0] == B - map_from and maps.shape[2] == N, f"maps {tuple(maps.shape)} for B={B} map_from={map_from} N={N}"
    Lc = maps.shape[1]
    q = None
    parts = L.load().udt_tattn_rowstat_parts(B, N, Cc) if emit_q8 else 0
    if parts > 0:
        q = _mx8_alloc(B * N, Cc, x.device)
        q = Mx8Act(q.data, q.scale, torch.empty((parts, B * N, 2), dtype=torch.float32, device=x.device))
    L.check(L.load().udt_tattn_fused_maps(_ptr(x), _ptr(out), _ptr(tables.A), _ptr(tables.sc), _ptr(tables.BmT), _ptr(bias), B, N, Cc, heads,
                                          zero_samples, eps, _ptr(maps), Lc, map_from, float(weight), int(bool(accumulate)),
                                          _ptr(q.data) if q else None, _ptr(q.scale) if q else None, _ptr(q.stats) if q else None,
                                          _stream()), "udt_tattn_fused_maps")
    if q is not None:
        out.mx8 = q
    return out


def softmax_rows_(x: torch.Tensor) -> torch.Tensor:
    _bf16(x)
    assert x.is_contiguous()
    cols = x.shape[-1]
    _drop_sidecars(x)
    L.check(L.load().udt_softmax_rows(_ptr(x), x.numel() // cols, cols, cols, _stream()), "udt_softmax_rows")
    return x


# --------------------------------------------------------------------------------------- normalisation
def group_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool,
               out: Optional[torch.Tensor] = None, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x bf16 NHWC [B, ..., C1] (+ optional x2 [B, ..., C2] concatenated on channels) -> [B, ..., C1+C2];
    statistics in fp32 over (pixels, channels/groups)."""
    _bf16(x)
    assert x.is_contiguous()
    B, C1 = x.shape[0], x.shape[-1]
    C2 = 0
    if x2 is not None:
        _bf16(x2)
        assert x2.is_contiguous() and x2.shape[:-1] == x.shape[:-1]
        C2 = x2.shape[-1]
    HW = x.numel() // (B * C1)
    lib = L.load()
    out = _drop_sidecars(out) if out is not None else torch.empty(x.shape[:-1] + (C1 + C2,), dtype=torch.bfloat16, device=x.device)
    if GN_STRIP and lib.udt_gn_strip_ok(B, HW, C1, C2, groups):      # one launch, second read out of L2
        L.check(lib.udt_gn_strip(_ptr(x), _ptr(x2), _ptr(out), _ptr(gamma), _ptr(beta), B, HW, C1, C2, groups, eps,
                                 1 if silu else 0, _stream()), "udt_gn_strip")
        return out
    nch = lib.udt_gn_nchunks(HW, C1 + C2)
    part = torch.empty((B, nch, groups, 2), dtype=torch.float32, device=x.device)
    L.check(lib.udt_gn_stats(_ptr(x), _ptr(x2), _ptr(part), B, HW, C1, C2, groups, _stream()), "udt_gn_stats")
    L.check(lib.udt_gn_apply(_ptr(x), _ptr(x2), _ptr(out), _ptr(part), _ptr(gamma), _ptr(beta), B, HW, C1, C2, groups,
                             eps, 1 if silu else 0, _stream()), "udt_gn_apply")
    return out


def gn_finalize(st1: GnStats, C1: int, st2: Optional[GnStats], C2: int, gamma: torch.Tensor, beta: torch.Tensor, B: int,
                HW: int, groups: int, eps: float) -> torch.Tensor:
    """producer-epilogue statistics (one or two concatenated sources) -> per-(sample, channel) GroupNorm scale/shift,
    fp32 [B, (C1+C2)/64, 2, 64] (the table udt_gn_silu_conv3x3_fwd reads)"""
    Ct = C1 + C2
    scsh = torch.empty((B, Ct // 64, 2, 64), dtype=torch.float32, device=st1.data.device)
    L.check(L.load().udt_gn_finalize(_ptr(st1.data), st1.slots_per_sample, C1, _ptr(st2.data) if st2 is not None else None,
                                     st2.slots_per_sample if st2 is not None else 0, C2, _ptr(gamma), _ptr(beta), _ptr(scsh),
                                     B, HW, groups, eps, _stream()), "udt_gn_finalize")
    return scsh


def gn_strip_ok(B: int, HW: int, C1: int, C2: int, groups: int) -> bool:
    """would group_norm run this shape as ONE strip launch (statistics + apply)?"""
    return bool(GN_STRIP and L.load().udt_gn_strip_ok(B, HW, C1, C2, groups))


def group_norm_from_stats(x: torch.Tensor, st1: GnStats, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float,
                          silu: bool, x2: Optional[torch.Tensor] = None, st2: Optional[GnStats] = None,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """GroupNorm (+ SiLU) whose statistics came out of the producers' epilogues (``x.gn_stats``): udt_gn_finalize turns them
    into a per-(sample, channel) scale / shift table, udt_gn_apply_scsh is the one read + write left of the norm"""
    _bf16(x)
    assert x.is_contiguous()
    B, C1 = x.shape[0], x.shape[-1]
    C2 = 0
    if x2 is not None:
        _bf16(x2)
        assert x2.is_contiguous() and x2.shape[:-1] == x.shape[:-1] and st2 is not None
        C2 = x2.shape[-1]
    HW = x.numel() // (B * C1)
    out = _drop_sidecars(out) if out is not None else torch.empty(x.shape[:-1] + (C1 + C2,), dtype=torch.bfloat16, device=x.device)
    if gn_strip_ok(B, HW, C1, C2, groups):          # small levels: one launch, the strip kernel without its statistics pass
        L.check(L.load().udt_gn_strip_stats(_ptr(x), _ptr(x2), _ptr(out), _ptr(st1.data), st1.slots_per_sample,
                                            _ptr(st2.data) if st2 is not None else None,
                                            st2.slots_per_sample if st2 is not None else 0, _ptr(gamma), _ptr(beta), B, HW, C1, C2,
                                            groups, eps, 1 if silu else 0, _stream()), "udt_gn_strip_stats")
        return out
    scsh = gn_finalize(st1, C1, st2, C2, gamma, beta, B, HW, groups, eps)
    L.check(L.load().udt_gn_apply_scsh(_ptr(x), _ptr(x2), _ptr(out), _ptr(scsh), B, HW, C1, C2, 1 if silu else 0, _stream()),
            "udt_gn_apply_scsh")
    return out


def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _bf16(x)
    assert x.is_contiguous()
    Cc = x.shape[-1]
    out = _drop_sidecars(out) if out is not None else torch.empty_like(x)
    L.check(L.load().udt_layernorm(_ptr(x), _ptr(out), _ptr(gamma), _ptr(beta), x.numel() // Cc, Cc, eps, _stream()),
            "udt_layernorm")
    return out


# ---------------------------------------------------------------------------------------- elementwise
def _nchw4(shape, *tensors: Optional[torch.Tensor]) -> None:
    """the latents of a sampler step (a None is an absent term): fp32 NCHW [B,4,h,w], contiguous"""
    B, _, h, w = shape
    for t in tensors:
        if t is not None:
            assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (B, 4, h, w), "fp32 NCHW [B,4,h,w]"


def _multistep_coefs(c_out: float, scale: float, sigma: float, coefs: Sequence[float], hist: Sequence[torch.Tensor]) -> L.MultistepCoefs:
    """udt_multistep_coefs: k[j] = coefs[j]; hist[j + 1] = the j-th older derivative (slot 0 is d itself)"""
    k = L.MultistepCoefs(c_out, scale, sigma, len(coefs))
    for j, c in enumerate(coefs):
        k.k[j] = c
    for j, t in enumerate(hist):
        k.hist[j + 1] = _ptr(t)
    return k


def unet_input(x: torch.Tensor, xin: torch.Tensor, c_in: float) -> None:
    B, _, h, w = x.shape
    _drop_sidecars(xin)
    L.check(L.load().udt_unet_input(_ptr(x), _ptr(xin), B, h * w, xin.shape[-1], c_in, _stream()), "udt_unet_input")


def unet_input_churn(x: torch.Tensor, noise: torch.Tensor, xin: torch.Tensor, c_in: float, kn: float) -> None:
    """one launch of udt_unet_input_churn: x <- x + kn*noise in place (x, noise: fp32 NCHW [B,4,h,w] contiguous, distinct), then
    unet_input on the stored x"""
    B, _, h, w = x.shape
    assert noise is not None
    _nchw4(x.shape, x, noise)
    _drop_sidecars(xin)
    L.check(L.load().udt_unet_input_churn(_ptr(x), _ptr(noise), _ptr(xin), B, h * w, xin.shape[-1], c_in, kn, _stream()),
            "udt_unet_input_churn")


def cfg_euler_step(x: torch.Tensor, eps: torch.Tensor, sigma: float, sigma_next: float, scale: float,
                   denoised: Optional[torch.Tensor] = None, c_out: Optional[float] = None) -> None:
    """c_out defaults to -sigma (EpsScaling); pass the quantised value when it differs from sigma."""
    B, _, h, w = x.shape
    assert x.dtype == torch.float32 and eps.dtype == torch.float32 and x.is_contiguous() and eps.is_contiguous()
    L.check(L.load().udt_cfg_euler_step(_ptr(x), _ptr(eps), _ptr(denoised), B, h * w, eps.shape[-1],
                                        -sigma if c_out is None else c_out, sigma, sigma_next, scale, _stream()),
            "udt_cfg_euler_step")


def cfg_sampler_step(xin: torch.Tensor, eps: torch.Tensor, c_out: float, scale: float, kx: float = 0.0, kd: float = 0.0,
                     aux: Optional[torch.Tensor] = None, ka: float = 0.0, prev: Optional[torch.Tensor] = None, kp: float = 0.0,
                     noise: Optional[torch.Tensor] = None, kn: float = 0.0, out: Optional[torch.Tensor] = None,
                     denoised: Optional[torch.Tensor] = None) -> torch.Tensor:
    """one launch of udt_cfg_sampler_step: den = CFG(xin + c_out*eps_u, xin + c_out*eps_c);
    out = kx*xin + kd*den + ka*aux + kp*prev + kn*noise (a term whose tensor is None is absent); denoised <- den.
    xin / aux / prev / noise / out / denoised: fp32 NCHW [B,4,h,w] contiguous; out defaults to xin (in place)."""
    B, _, h, w = xin.shape
    out = xin if out is None else out
    _nchw4(xin.shape, xin, aux, prev, noise, out, denoised)
    assert eps.dtype == torch.float32 and eps.is_contiguous() and tuple(eps.shape[:-1]) == (2 * B, h, w) and eps.shape[-1] >= 4
    k = L.SamplerCoefs(kx, kd, ka, kp, kn, c_out, scale)
    L.check(L.load().udt_cfg_sampler_step(_ptr(xin), _ptr(eps), _ptr(aux), _ptr(prev), _ptr(noise), _ptr(out), _ptr(denoised),
                                          B, h * w, eps.shape[-1], k, _stream()), "udt_cfg_sampler_step")
    return out


def cfg_multistep_step(xin: torch.Tensor, eps: torch.Tensor, c_out: float, scale: float, sigma: float, coefs: Sequence[float],
                       hist: Sequence[torch.Tensor] = (), d_out: Optional[torch.Tensor] = None,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """one launch of udt_cfg_multistep_step: den = CFG(xin + c_out*eps_u, xin + c_out*eps_c); d = (xin - den)/sigma;
    out = xin + (coefs[0]*d + coefs[1]*hist[0] + ... + coefs[n-1]*hist[n-2]) (hist: the older derivatives, newest first);
    d_out <- d.  xin / hist / out / d_out: fp32 NCHW [B,4,h,w] contiguous; out defaults to xin (in place); d_out is required and
    aliases none of the others."""
    B, _, h, w = xin.shape
    out = xin if out is None else out
    n = len(coefs)
    assert 1 <= n <= L.MULTISTEP_MAX and len(hist) == n - 1, "n = len(coefs) in 1..8 and len(hist) = n - 1"
    assert d_out is not None and all(t is not None for t in hist), "d_out and every hist tensor are required"
    _nchw4(xin.shape, xin, out, d_out, *hist)
    assert eps.dtype == torch.float32 and eps.is_contiguous() and tuple(eps.shape[:-1]) == (2 * B, h, w) and eps.shape[-1] >= 4
    k = _multistep_coefs(c_out, scale, sigma, coefs, hist)
    L.check(L.load().udt_cfg_multistep_step(_ptr(xin), _ptr(eps), _ptr(out), _ptr(d_out), B, h * w, eps.shape[-1], k,
                                            _stream()), "udt_cfg_multistep_step")
    return out


# ---- the same launches under any preconditioning, with or without the CFG pair (udt_precond_*)
def _check_step_args(xin: torch.Tensor, f: torch.Tensor, pair: bool, what: str, *others) -> tuple:
    """shapes of one udt_precond_* step: xin and ``others`` fp32 NCHW [B,4,h,w] contiguous, f fp32 NHWC [(2B if pair else B), h, w, ld]"""
    B, _, h, w = xin.shape
    for t in (xin, *others):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (B, 4, h, w)):
            raise ValueError(f"{what}: fp32 NCHW [B,4,h,w] contiguous tensors")
    rows = 2 * B if pair else B
    if f.dtype != torch.float32 or not f.is_contiguous() or f.dim() != 4 or tuple(f.shape[:-1]) != (rows, h, w):
        raise ValueError(f"{what}: the network output must be fp32 [{rows}, {h}, {w}, ld] ({'CFG pair' if pair else 'unguided'}), "
                         f"got {tuple(f.shape)}")
    return B, h * w, f.shape[-1]


def precond_unet_input(x: torch.Tensor, xin: torch.Tensor, c_in: float, pair: bool = True, noise: Optional[torch.Tensor] = None,
                       kn: float = 0.0) -> None:
    """one launch of udt_precond_unet_input: channels 0..3 of xin's rows [0, B) (and [B, 2B) if ``pair``) = x * c_in; ``noise``:
    the churned form, x <- x + kn*noise in place first"""
    B, _, h, w = x.shape
    rows = 2 * B if pair else B
    for t in (x, noise):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (B, 4, h, w)):
            raise ValueError("precond_unet_input: fp32 NCHW [B,4,h,w] contiguous tensors")
    if xin.dtype != torch.bfloat16 or not xin.is_contiguous() or tuple(xin.shape[:-1]) != (rows, h, w):
        raise ValueError(f"precond_unet_input: xin must be bf16 [{rows}, {h}, {w}, cpad] ({'CFG pair' if pair else 'unguided'}), "
                         f"got {tuple(xin.shape)}")
    _drop_sidecars(xin)
    L.check(L.load().udt_precond_unet_input(_ptr(x), _ptr(noise), _ptr(xin), B, h * w, xin.shape[-1], c_in, kn, int(pair),
                                            _stream()), "udt_precond_unet_input")


def precond_euler_step(x: torch.Tensor, f: torch.Tensor, c_skip: float, c_out: float, sigma: float, sigma_next: float,
                       scale: float = 0.0, pair: bool = True, denoised: Optional[torch.Tensor] = None) -> None:
    """one launch of udt_precond_euler_step: den = guided(c_skip*x + c_out*F); x += (x - den)/sigma * (sigma_next - sigma)"""
    B, hw, ld = _check_step_args(x, f, pair, "precond_euler_step", denoised)
    L.check(L.load().udt_precond_euler_step(_ptr(x), _ptr(f), _ptr(denoised), B, hw, ld, c_skip, c_out, sigma, sigma_next, scale,
                                            int(pair), _stream()), "udt_precond_euler_step")


def precond_sampler_step(xin: torch.Tensor, f: torch.Tensor, c_skip: float, c_out: float, scale: float = 0.0, pair: bool = True,
                         kx: float = 0.0, kd: float = 0.0, aux: Optional[torch.Tensor] = None, ka: float = 0.0,
                         prev: Optional[torch.Tensor] = None, kp: float = 0.0, noise: Optional[torch.Tensor] = None, kn: float = 0.0,
                         out: Optional[torch.Tensor] = None, denoised: Optional[torch.Tensor] = None) -> torch.Tensor:
    """one launch of udt_precond_sampler_step: cfg_sampler_step's update on den = guided(c_skip*xin + c_out*F)"""
    out = xin if out is None else out
    B, hw, ld = _check_step_args(xin, f, pair, "precond_sampler_step", aux, prev, noise, out, denoised)
    k = L.SamplerCoefs(kx, kd, ka, kp, kn, c_out, scale)
    L.check(L.load().udt_precond_sampler_step(_ptr(xin), _ptr(f), _ptr(aux), _ptr(prev), _ptr(noise), _ptr(out), _ptr(denoised),
                                              B, hw, ld, k, c_skip, int(pair), _stream()), "udt_precond_sampler_step")
    return out


def precond_multistep_step(xin: torch.Tensor, f: torch.Tensor, c_skip: float, c_out: float, scale: float, pair: bool, sigma: float,
                           coefs: Sequence[float], hist: Sequence[torch.Tensor] = (), d_out: Optional[torch.Tensor] = None,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """one launch of udt_precond_multistep_step: cfg_multistep_step's update on den = guided(c_skip*xin + c_out*F)"""
    out = xin if out is None else out
    n = len(coefs)
    if not (1 <= n <= L.MULTISTEP_MAX and len(hist) == n - 1) or d_out is None:
        raise ValueError("precond_multistep_step: n = len(coefs) in 1..8, len(hist) = n - 1 and d_out is required")
    B, hw, ld = _check_step_args(xin, f, pair, "precond_multistep_step", out, d_out, *hist)
    k = _multistep_coefs(c_out, scale, sigma, coefs, hist)
    L.check(L.load().udt_precond_multistep_step(_ptr(xin), _ptr(f), _ptr(out), _ptr(d_out), B, hw, ld, k, c_skip, int(pair),
                                                _stream()), "udt_precond_multistep_step")
    return out


def posterior_sample(moments: torch.Tensor, noise: torch.Tensor, scale: float) -> torch.Tensor:
    """moments fp32 NHWC [B, h, w, ld>=8]; noise fp32 NCHW [B,4,h,w] -> z fp32 NCHW."""
    B, h, w, ld = moments.shape
    assert moments.dtype == torch.float32 and noise.dtype == torch.float32 and moments.is_contiguous()
    z = torch.empty((B, 4, h, w), dtype=torch.float32, device=moments.device)
    L.check(L.load().udt_posterior_sample(_ptr(moments), _ptr(noise.contiguous()), _ptr(z), B, h * w, ld, scale,
                                          _stream()), "udt_posterior_sample")
    return z


def nchw_to_nhwc(x: torch.Tensor, cpad: int, scale: float = 1.0) -> torch.Tensor:
    assert x.dtype == torch.float32 and x.is_contiguous()
    B, Cc, H, W_ = x.shape
    y = torch.empty((B, H, W_, cpad), dtype=torch.bfloat16, device=x.device)
    L.check(L.load().udt_nchw_to_nhwc(_ptr(x), _ptr(y), B, Cc, H * W_, cpad, scale, _stream()), "udt_nchw_to_nhwc")
    return y


def nhwc_to_nchw(x: torch.Tensor, channels: int) -> torch.Tensor:
    assert x.is_contiguous() and x.dtype in (torch.float32, torch.bfloat16)
    B, H, W_, ld = x.shape
    y = torch.empty((B, channels, H, W_), dtype=torch.float32, device=x.device)
    L.check(L.load().udt_nhwc_to_nchw(_ptr(x), _ptr(y), B, channels, H * W_, ld, 1 if x.dtype == torch.float32 else 0,
                                      _stream()), "udt_nhwc_to_nchw")
    return y


def nhwc_set_channels(src: torch.Tensor, dst: torch.Tensor, c0: int) -> None:
    assert src.dtype == torch.float32 and src.is_contiguous() and dst.dtype == torch.bfloat16 and dst.is_contiguous()
    B, Cc, H, W_ = src.shape
    _drop_sidecars(dst)
    L.check(L.load().udt_nhwc_set_channels(_ptr(src), _ptr(dst), B, Cc, H * W_, dst.shape[-1], c0, _stream()),
            "udt_nhwc_set_channels")


def embed_tokens(idx: torch.Tensor, table: torch.Tensor, pe: torch.Tensor) -> torch.Tensor:
    assert idx.dtype == torch.int32 and idx.is_contiguous()
    n_tok = idx.numel()
    Lc, D = pe.shape
    out = torch.empty((n_tok, D), dtype=torch.bfloat16, device=idx.device)
    L.check(L.load().udt_embed_tokens(_ptr(idx), _ptr(table), _ptr(pe), _ptr(out), n_tok, Lc, D, _stream()),
            "udt_embed_tokens")
    return out


def timestep_embedding(t: torch.Tensor, dim: int) -> torch.Tensor:
    assert t.dtype == torch.float32 and t.is_contiguous()
    out = torch.empty((t.numel(), dim), dtype=torch.bfloat16, device=t.device)
    L.check(L.load().udt_timestep_embedding(_ptr(t), _ptr(out), t.numel(), dim, _stream()), "udt_timestep_embedding")
    return out


def mask_downsample(mask: torch.Tensor) -> torch.Tensor:
    assert mask.dtype == torch.float32 and mask.is_contiguous()
    B, _, H, W_ = mask.shape
    out = torch.empty((B, 1, H // 8, W_ // 8), dtype=torch.float32, device=mask.device)
    L.check(L.load().udt_mask_downsample(_ptr(mask), _ptr(out), B, H, W_, _stream()), "udt_mask_downsample")
    return out


def crop_resize_aa(img: torch.Tensor, boxes: torch.Tensor, out_hw, mul: float = 1.0, add: float = 0.0) -> torch.Tensor:
    """crop + antialiased bicubic resize + ``mul * v + add`` of every box in one launch (udt_crop_resize_aa_f32): img fp32
    [B, C, H, W]; boxes DEVICE int32 [N, 5] = (image index, top, bottom, left, right), half-open as the slice
    img[index, :, top:bottom, left:right]; -> fp32 [N, C, oh, ow].  The kernel clamps a box to the image; validating boxes is
    the caller's, on the host (ParseqPredictor.transform_boxes)."""
    assert img.dtype == torch.float32 and img.dim() == 4 and img.is_contiguous()
    assert boxes.dtype == torch.int32 and boxes.dim() == 2 and boxes.shape[1] == 5 and boxes.is_contiguous()
    assert boxes.device == img.device
    B, Cc, H, W_ = img.shape
    N, (oh, ow) = boxes.shape[0], (int(v) for v in out_hw)
    out = torch.empty((N, Cc, oh, ow), dtype=torch.float32, device=img.device)
    L.check(L.load().udt_crop_resize_aa_f32(_ptr(img), _ptr(boxes), _ptr(out), B, Cc, H, W_, N, oh, ow, float(mul), float(add), _stream()),
            "udt_crop_resize_aa_f32")
    return out


def resize_bilinear(x: torch.Tensor, out_hw, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bilinear resize (half-pixel centres, edge clamp, no antialiasing) of every [h, w] plane of x fp32 [..., h, w] to ``out_hw`` in one
    launch (udt_resize_bilinear_f32) -> fp32 [..., H, W]"""
    assert x.dtype == torch.float32 and x.dim() >= 2 and x.is_contiguous()
    h, w = x.shape[-2:]
    H, W_ = (int(v) for v in out_hw)
    shape = tuple(x.shape[:-2]) + (H, W_)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == shape and out.is_contiguous() and out.device == x.device
    planes = x.numel() // (h * w) if h * w else 0
    L.check(L.load().udt_resize_bilinear_f32(_ptr(x), _ptr(out), planes, h, w, H, W_, _stream()), "udt_resize_bilinear_f32")
    return out


# ---- LPIPS (csrc/lpips.hip): fp32 channels-last maps [N, H, W, C] whose pixels are dense and whose pixel stride (ld) is >= C
def _nhwc_f32(t: torch.Tensor) -> int:
    """the ld of a channels-last fp32 map (pixels dense in (n, y, x) order), checked"""
    assert t.dtype == torch.float32 and t.dim() == 4 and t.stride(3) == 1
    N, H, W_, Cc = t.shape
    # (the stride of a dimension of size 1 says nothing: the ld is read off the dimensions that do step)
    lds = {t.stride(d) // step if t.stride(d) % step == 0 else -1 for d, size, step in ((0, N, H * W_), (1, H, W_), (2, W_, 1)) if size > 1}
    ld = lds.pop() if lds else Cc
    assert not lds and ld >= Cc, (tuple(t.shape), t.stride())
    return ld


def conv2d_f32(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], cout: int, ksize: int, stride: int, pad: int,
               relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 convolution + bias (+ ReLU) on f32-input MFMA (udt_conv2d_f32): x fp32 [N, H, W, Cin] channels-last, w the packed
    [cout, Kp] weights of ``packing.pack_conv_f32`` -> fp32 [N, Ho, Wo, cout].  A geometry the kernel refuses raises ValueError."""
    N, H, W_, Cin = x.shape
    ldx = _nhwc_f32(x)
    kp = (ksize * ksize * Cin + 15) // 16 * 16
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (cout, kp), (tuple(w.shape), (cout, kp))
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == cout)
    Ho, Wo = conv_out_hw(H, W_, ksize, max(1, stride), (pad, pad))
    if out is None:
        if Ho < 1 or Wo < 1:
            raise ValueError(f"conv2d_f32: a {H} x {W_} map has no output pixel under kernel {ksize}, stride {stride}, padding {pad}")
        out = torch.empty((N, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == (N, Ho, Wo, cout) and out.device == x.device
    L.check(L.load().udt_conv2d_f32(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), N, H, W_, Cin, ldx, cout, _nhwc_f32(out), ksize, stride, pad,
                                    int(relu), _stream()), "udt_conv2d_f32")
    return out


def maxpool3s2_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nn.MaxPool2d(3, 2) (no padding, floor) of a channels-last fp32 map (udt_maxpool3s2_f32)"""
    N, H, W_, Cc = x.shape
    ldx = _nhwc_f32(x)
    if H < 3 or W_ < 3:
        raise ValueError(f"maxpool3s2_f32: a {H} x {W_} map has no 3 x 3 window")
    shape = (N, (H - 3) // 2 + 1, (W_ - 3) // 2 + 1, Cc)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == shape and out.device == x.device
    L.check(L.load().udt_maxpool3s2_f32(_ptr(x), _ptr(out), N, H, W_, Cc, ldx, _nhwc_f32(out), _stream()), "udt_maxpool3s2_f32")
    return out


def lpips_input(samples: torch.Tensor, images: torch.Tensor, shift: torch.Tensor, scale: torch.Tensor, quantise: bool = True,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the LPIPS network input of N pairs in one launch (udt_lpips_input_f32): samples fp32 [N, 3, H, W] in [0, 1], images fp32
    [N, 3, H, W] in [-1, 1] -> fp32 [2 N, H, W, 3] channels-last, the samples' frames first"""
    for t in (samples, images):
        assert t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 3 and t.is_contiguous()
    assert samples.shape == images.shape and samples.device == images.device
    for t in (shift, scale):
        assert t.dtype == torch.float32 and t.numel() == 3 and t.is_contiguous() and t.device == samples.device
    N, _, H, W_ = samples.shape
    if out is None:
        out = torch.empty((2 * N, H, W_, 3), dtype=torch.float32, device=samples.device)
    assert tuple(out.shape) == (2 * N, H, W_, 3) and out.device == samples.device
    L.check(L.load().udt_lpips_input_f32(_ptr(samples), _ptr(images), _ptr(shift), _ptr(scale), _ptr(out), N, H, W_, _nhwc_f32(out),
                                         int(bool(quantise)), _stream()), "udt_lpips_input_f32")
    return out


def lpips_layer_scratch_bytes(n_pairs: int, pixels: int) -> int:
    return int(L.load().udt_lpips_layer_scratch_bytes(int(n_pairs), int(pixels)))


def lpips_layer(feats: torch.Tensor, w: torch.Tensor, out: torch.Tensor, accumulate: bool, scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """one tap of the LPIPS distance (udt_lpips_layer_f32): feats fp32 [2 N, h, w, C] channels-last (pair n = frames n and N + n),
    w fp32 [C] -> out fp32 [N], overwritten or (``accumulate``) added to.  ``scratch``: uint8, at least ``lpips_layer_scratch_bytes``."""
    N2, h, w_, Cc = feats.shape
    ld = _nhwc_f32(feats)
    assert N2 % 2 == 0 and N2 > 0
    N, P = N2 // 2, h * w_
    assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() == Cc and w.device == feats.device
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == N and out.device == feats.device
    need = lpips_layer_scratch_bytes(N, P)
    if scratch is None:
        scratch = torch.empty((need,), dtype=torch.uint8, device=feats.device)
    assert scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.device == feats.device
    L.check(L.load().udt_lpips_layer_f32(_ptr(feats), _ptr(w), _ptr(out), N, P, Cc, ld, int(bool(accumulate)), _ptr(scratch),
                                         scratch.numel(), _stream()), "udt_lpips_layer_f32")
    return out


# ---- FID (csrc/fid.hip): the same fp32 channels-last family; a channel slice t[..., a:b] of a wider map is a valid operand and output
def conv2d_rect_f32(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], cout: int, kernel, stride: int, pad,
                    relu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``conv2d_f32`` with kernel = (kh, kw) and pad = (pad_h, pad_w) (udt_conv2d_rect_f32); x and ``out`` may be channel slices"""
    N, H, W_, Cin = x.shape
    ldx = _nhwc_f32(x)
    (kh, kw), (ph, pw) = (int(v) for v in kernel), (int(v) for v in pad)
    kp = (kh * kw * Cin + 15) // 16 * 16
    assert w.dtype == torch.float32 and w.is_contiguous() and tuple(w.shape) == (cout, kp), (tuple(w.shape), (cout, kp))
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == cout)
    s = max(1, stride)
    Ho, Wo = (H + 2 * ph - kh) // s + 1, (W_ + 2 * pw - kw) // s + 1
    if out is None:
        if Ho < 1 or Wo < 1:
            raise ValueError(f"conv2d_rect_f32: a {H} x {W_} map has no output pixel under kernel {kh} x {kw}, stride {stride}, "
                             f"padding ({ph}, {pw})")
        out = torch.empty((N, Ho, Wo, cout), dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == (N, Ho, Wo, cout) and out.device == x.device
    L.check(L.load().udt_conv2d_rect_f32(_ptr(x), _ptr(w), _ptr(bias), _ptr(out), N, H, W_, Cin, ldx, cout, _nhwc_f32(out), kh, kw, stride,
                                         ph, pw, int(relu), _stream()), "udt_conv2d_rect_f32")
    return out


def pool3_f32(x: torch.Tensor, stride: int, pad: int, average: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """3 x 3 max-pool, or the average that does not count padding (F.avg_pool2d(count_include_pad=False)), stride 1 or 2, padding 0
    or 1, floor mode, of a channels-last fp32 map (udt_pool3_f32)"""
    N, H, W_, Cc = x.shape
    ldx = _nhwc_f32(x)
    stride, pad = int(stride), int(pad)
    if stride not in (1, 2) or pad not in (0, 1) or H + 2 * pad < 3 or W_ + 2 * pad < 3:
        raise ValueError(f"pool3_f32: a {H} x {W_} map, stride {stride}, padding {pad}: stride 1 or 2, padding 0 or 1, one window at least")
    shape = (N, (H + 2 * pad - 3) // stride + 1, (W_ + 2 * pad - 3) // stride + 1, Cc)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    assert tuple(out.shape) == shape and out.device == x.device
    L.check(L.load().udt_pool3_f32(_ptr(x), _ptr(out), N, H, W_, Cc, ldx, _nhwc_f32(out), stride, pad, int(bool(average)), _stream()),
            "udt_pool3_f32")
    return out


def fid_input(samples: torch.Tensor, images: torch.Tensor, quantise: bool = True, size: int = 299,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the Inception input of N pairs in one launch (udt_fid_input_f32): samples fp32 [N, 3, H, W] in [0, 1], images fp32 [N, 3, H, W]
    in [-1, 1] -> fp32 [2 N, size, size, 3] channels-last in [-1, 1], the samples' frames first"""
    for t in (samples, images):
        assert t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 3 and t.is_contiguous()
    assert samples.shape == images.shape and samples.device == images.device
    N, _, H, W_ = samples.shape
    size = int(size)
    if out is None:
        out = torch.empty((2 * N, size, size, 3), dtype=torch.float32, device=samples.device)
    assert tuple(out.shape) == (2 * N, size, size, 3) and out.device == samples.device
    L.check(L.load().udt_fid_input_f32(_ptr(samples), _ptr(images), _ptr(out), N, H, W_, size, _nhwc_f32(out), int(bool(quantise)),
                                       _stream()), "udt_fid_input_f32")
    return out


def mean_pixels_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """global average pool of a channels-last fp32 map [N, h, w, C] -> fp32 [N, C] (udt_mean_pixels_f32); ``out`` may have a row
    stride > C"""
    N, h, w_, Cc = x.shape
    ldx = _nhwc_f32(x)
    if out is None:
        out = torch.empty((N, Cc), dtype=torch.float32, device=x.device)
    assert out.dtype == torch.float32 and tuple(out.shape) == (N, Cc) and out.stride(1) == 1 and out.device == x.device
    ldo = out.stride(0) if N > 1 else Cc
    assert ldo >= Cc
    L.check(L.load().udt_mean_pixels_f32(_ptr(x), _ptr(out), N, h * w_, Cc, ldx, ldo, _stream()), "udt_mean_pixels_f32")
    return out


def moments_accum_f64(x: torch.Tensor, total: torch.Tensor, outer: torch.Tensor) -> None:
    """total fp64 [D] += the column sums of x fp32 [n, D] (row stride >= D), outer fp64 [D, D] += x^T x, in fp64 on the f64 MFMA
    (udt_moments_accum_f64)"""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
    n, D = x.shape
    ld = x.stride(0) if n > 1 else D
    assert ld >= D
    for t, shape in ((total, (D,)), (outer, (D, D))):
        assert t.dtype == torch.float64 and tuple(t.shape) == shape and t.is_contiguous() and t.device == x.device
    L.check(L.load().udt_moments_accum_f64(_ptr(x), _ptr(total), _ptr(outer), n, D, ld, _stream()), "udt_moments_accum_f64")


def crop_resize_aa_bwd(d_out: torch.Tensor, boxes: torch.Tensor, img_shape, mul: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the adjoint of ``crop_resize_aa`` (udt_crop_resize_aa_bwd_f32): d_out fp32 [N, C, oh, ow], the same DEVICE int32 boxes [N, 5]
    -> d_img fp32 ``img_shape`` = [B, C, H, W], every element written (zero outside the boxes and for images without one).
    Precondition: an image index appears in at most one box — validated by the caller on the host (``unique_box_images``)."""
    assert d_out.dtype == torch.float32 and d_out.dim() == 4 and d_out.is_contiguous()
    assert boxes.dtype == torch.int32 and boxes.dim() == 2 and boxes.shape[1] == 5 and boxes.is_contiguous()
    assert boxes.device == d_out.device and boxes.shape[0] == d_out.shape[0]
    B, Cc, H, W_ = (int(v) for v in img_shape)
    N, oh, ow = d_out.shape[0], d_out.shape[2], d_out.shape[3]
    assert d_out.shape[1] == Cc
    if out is None:
        out = torch.empty((B, Cc, H, W_), dtype=torch.float32, device=d_out.device)
    assert out.dtype == torch.float32 and out.shape == (B, Cc, H, W_) and out.is_contiguous()
    L.check(L.load().udt_crop_resize_aa_bwd_f32(_ptr(d_out), _ptr(boxes), _ptr(out), B, Cc, H, W_, N, oh, ow, float(mul), _stream()),
            "udt_crop_resize_aa_bwd_f32")
    return out


def unique_box_images(boxes) -> None:
    """host check of ``crop_resize_aa_bwd``'s precondition on a HOST box table [N, 5]: raises ValueError on a repeated image index"""
    seen = {}
    for n, row in enumerate(torch.as_tensor(boxes).reshape(-1, 5).tolist()):
        i = int(row[0])
        if i in seen:
            raise ValueError(f"boxes {seen[i]} and {n} both lie in image {i}: the gradient takes one box per image")
        seen[i] = n


def masked_attention_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, d_o: torch.Tensor, heads: int, scale: float,
                         mask: Optional[torch.Tensor] = None, key_padding_mask: Optional[torch.Tensor] = None, want_dq: bool = True,
                         dq: Optional[torch.Tensor] = None, dk: Optional[torch.Tensor] = None, dv: Optional[torch.Tensor] = None):
    """backward of ``masked_attention`` (udt_mattn_bwd): the same q / k / v row views and masks, d_o bf16 [B, Nq, *] -> (dq or None,
    dk, dv) bf16 [B, Nq | Lk, heads*D]; dq / dk / dv may be given as row views (column slices of one [.., 3C] or [.., 2C] buffer)"""
    _bf16(q); _bf16(k); _bf16(v); _bf16(d_o)
    B, Nq, Cq = q.shape
    Lk = k.shape[1]
    D = Cq // heads
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1 and d_o.stride(2) == 1 and d_o.shape[:2] == (B, Nq)
    new = lambda n: torch.empty((B, n, heads * D), dtype=torch.bfloat16, device=q.device)
    if want_dq and dq is None:
        dq = new(Nq)
    if not want_dq:
        dq = None
    dk = new(Lk) if dk is None else dk
    dv = new(Lk) if dv is None else dv
    for t in (dq, dk, dv):
        if t is not None:
            _bf16(t)
            assert t.stride(2) == 1
            _drop_sidecars(t)
    mask, key_padding_mask = _masks(mask, key_padding_mask, B, Nq, Lk)
    L.check(L.load().udt_mattn_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(d_o), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(mask), _ptr(key_padding_mask),
                                   B, heads, D, Nq, Lk, *_strides(q, k, v, d_o, dq, dk, dv, between=(Lk,)), scale, _stream()),
            "udt_mattn_bwd")
    return dq, dk, dv


def gelu(a: torch.Tensor) -> torch.Tensor:
    """exact-erf GELU of stored pre-activations a fp32 [rows, C] (a GEMM's fp32 output) -> bf16 [rows, C] (udt_gelu_fwd)"""
    assert a.dtype == torch.float32 and a.is_contiguous() and a.dim() == 2
    out = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device)
    L.check(L.load().udt_gelu_fwd(_ptr(a), _ptr(out), a.shape[0], a.shape[1], _stream()), "udt_gelu_fwd")
    return out


def gelu_bwd(a: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    """dy bf16 [rows, C] -> d a bf16 [rows, C] on the stored fp32 pre-activations (udt_gelu_bwd)"""
    _bf16(dy)
    assert a.dtype == torch.float32 and a.is_contiguous() and a.dim() == 2 and dy.is_contiguous() and dy.shape == a.shape
    da = torch.empty_like(dy)
    L.check(L.load().udt_gelu_bwd(_ptr(a), _ptr(dy), _ptr(da), a.shape[0], a.shape[1], _stream()), "udt_gelu_bwd")
    return da


def ocr_ce(logits: torch.Tensor, targets: torch.Tensor, n_chars: torch.Tensor, weight: Optional[torch.Tensor] = None,
           n_cls: Optional[int] = None):
    """clamped character cross entropy and its seed (udt_ocr_ce_f32): logits fp32 [N, L, >= n_cls] (a row view: the last stride 1, the
    position stride free), targets int32 [N, T], n_chars int32 [N] (1 <= n <= min(L, T): the CALLER validates on the host), weight fp32
    [N] or None -> (loss fp32 [N], d_logits fp32 [N, L, n_cls])"""
    assert logits.dtype == torch.float32 and logits.dim() == 3 and logits.stride(2) == 1
    N, Lq = logits.shape[:2]
    n_cls = logits.shape[2] if n_cls is None else int(n_cls)
    if logits.stride(0) != Lq * logits.stride(1):                   # (a size-1 dimension carries any stride: give the kernel the dense form)
        logits = logits.contiguous()
    assert n_cls <= logits.shape[2]
    assert targets.dtype == torch.int32 and targets.dim() == 2 and targets.shape[0] == N and targets.is_contiguous()
    assert n_chars.dtype == torch.int32 and n_chars.shape == (N,) and n_chars.is_contiguous()
    if weight is not None:
        assert weight.dtype == torch.float32 and weight.shape == (N,) and weight.is_contiguous()
    loss = torch.empty((N,), dtype=torch.float32, device=logits.device)
    d_logits = torch.empty((N, Lq, n_cls), dtype=torch.float32, device=logits.device)
    L.check(L.load().udt_ocr_ce_f32(_ptr(logits), _ptr(targets), _ptr(n_chars), _ptr(weight), _ptr(loss), _ptr(d_logits), N, Lq, n_cls,
                                    logits.stride(1), targets.shape[1], n_cls, _stream()), "udt_ocr_ce_f32")
    return loss, d_logits


def _ll_dims(probs: torch.Tensor, B: int, heads: int, loss: Optional[torch.Tensor], d_probs: Optional[torch.Tensor] = None,
             tiled: bool = True) -> tuple:
    """the checks of the local_loss_* wrappers -> (n, Lc): probs [n * heads, tokens, Lc] contiguous, scored against B masks (tiled:
    n a multiple of B, else n == B); loss fp32 [n] (None only next to a d_probs); d_probs fp32, like probs"""
    n = probs.shape[0] // heads
    assert probs.is_contiguous() and (n % B == 0 if tiled else probs.shape[0] == B * heads)
    assert d_probs is not None if loss is None else (loss.is_contiguous() and loss.numel() == n)
    assert d_probs is None or (d_probs.dtype == torch.float32 and d_probs.is_contiguous() and d_probs.shape == probs.shape)
    return n, probs.shape[-1]


def _ll_scratch(probs: torch.Tensor, *shape: int) -> torch.Tensor:
    """the partial sums one local-loss launch keeps per (sample, segment)"""
    return torch.empty(shape, dtype=torch.float32, device=probs.device)


def local_loss_accumulate(probs: torch.Tensor, mask: torch.Tensor, seg_mask: torch.Tensor, gk9: torch.Tensor,
                          loss: torch.Tensor, heads: int, size: int) -> None:
    """loss [n] += per-layer local-loss term of n = probs.shape[0] / heads samples; sample i is scored against
    mask[i % B] / seg_mask[i % B] (B = mask.shape[0]; n a multiple of B: tiled candidates, or the uncond ‖ cond halves)"""
    B = mask.shape[0]
    n, Lc = _ll_dims(probs, B, heads, loss)
    L.check(L.load().udt_local_loss_tiled(_ptr(probs), _ptr(mask), _ptr(seg_mask), _ptr(gk9), _ptr(loss), n, B, heads, size, Lc,
                                          seg_mask.shape[1], mask.shape[2], mask.shape[3], _stream()), "udt_local_loss_tiled")


def _check_map_hw(probs: torch.Tensor, hw, what: str):
    """(h, w) of a [b * heads, n, L] probability map; n != h * w would be scored on a wrong row pitch: refuse it"""
    h, w = int(hw[0]), int(hw[1])
    if probs.dim() != 3 or h <= 0 or w <= 0 or probs.shape[1] != h * w:
        raise ValueError(f"{what}: maps of shape {tuple(probs.shape)} do not hold h * w = {h} * {w} tokens")
    return h, w


def local_loss_accumulate_hw(probs: torch.Tensor, mask: torch.Tensor, seg_mask: torch.Tensor, gk9: torch.Tensor,
                             loss: torch.Tensor, heads: int, hw) -> None:
    """``local_loss_accumulate`` on h x w maps (tokens row-major, n = y * w + x): udt_local_loss_tiled_hw, one workgroup per
    (context token, sample)"""
    h, w = _check_map_hw(probs, hw, "local_loss_accumulate_hw")
    B = mask.shape[0]
    n, Lc = _ll_dims(probs, B, heads, loss)
    scratch = _ll_scratch(probs, n, seg_mask.shape[1], 2)
    L.check(L.load().udt_local_loss_tiled_hw(_ptr(probs), _ptr(mask), _ptr(seg_mask), _ptr(gk9), _ptr(loss), _ptr(scratch), n, B, heads,
                                             h, w, Lc, seg_mask.shape[1], mask.shape[2], mask.shape[3], _stream()),
            "udt_local_loss_tiled_hw")


def add_(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    _bf16(x); _bf16(y)
    assert x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    _drop_sidecars(x)
    L.check(L.load().udt_add_bf16(_ptr(x), _ptr(y), x.numel(), _stream()), "udt_add_bf16")
    return x


def bias_add(x: torch.Tensor, bias: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[..., c] = x[..., c] + bias[c]  (bf16 rows, fp32 bias)"""
    _bf16(x)
    Cc = x.shape[-1]
    out = _drop_sidecars(out) if out is not None else torch.empty_like(x)
    assert x.is_contiguous() and out.is_contiguous() and bias.dtype == torch.float32 and bias.numel() >= Cc
    L.check(L.load().udt_bias_add_bf16(_ptr(x), _ptr(bias), _ptr(out), x.numel() // Cc, Cc, _stream()), "udt_bias_add_bf16")
    return out


# ------------------------------------------------------------------------------------------ backward (dX only, csrc/backward.hip)
def attention_bwd(qkv: torch.Tensor, o: torch.Tensor, d_o: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """flash-attention backward of ``attention_rowv(qkv[..., :C], qkv[..., C:2C], qkv[..., 2C:], heads, scale)``:
    qkv bf16 [B, N, 3 C], o / d_o bf16 [B, N, C] -> d(qkv) bf16 [B, N, 3 C] (udt_attn_bwd: two launches, deterministic)"""
    _bf16(qkv); _bf16(o); _bf16(d_o)
    B, N, C3 = qkv.shape
    Cc = heads * 64
    assert C3 == 3 * Cc and qkv.is_contiguous() and o.is_contiguous() and d_o.is_contiguous() and o.shape == (B, N, Cc) == d_o.shape
    dqkv = torch.empty_like(qkv)
    ws = torch.empty((2, B * heads * N), dtype=torch.float32, device=qkv.device)
    es = qkv.element_size()
    L.check(L.load().udt_attn_bwd(qkv.data_ptr(), qkv.data_ptr() + Cc * es, qkv.data_ptr() + 2 * Cc * es, _ptr(o), _ptr(d_o),
                                  dqkv.data_ptr(), dqkv.data_ptr() + Cc * es, dqkv.data_ptr() + 2 * Cc * es, ws[0].data_ptr(),
                                  ws[1].data_ptr(), B, heads, N, C3, Cc, C3, scale, _stream()), "udt_attn_bwd")
    return dqkv


def attention_d512_bwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, o: torch.Tensor, d_o: torch.Tensor, scale: float,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """flash-attention backward of ``attention_d512(q, k, v, scale)`` (self-attention): q, k, v [B, N, 512] row views (e.g. the column
    ranges of one q|k|v projection), o / d_o bf16 [B, N, 512] row views -> d(q|k|v) bf16 [B, N, 1536] (``out``: a [B, N, >= 1536] row
    view to write into; its first 1536 columns are returned).  udt_attn512_bwd: two launches, deterministic, no [N, N] tensor."""
    for t in (q, k, v, o, d_o):
        _bf16(t)
        assert t.dim() == 3 and t.shape[2] == 512 and t.stride(2) == 1 and t.shape[:2] == q.shape[:2]
    B, N = q.shape[0], q.shape[1]
    if out is None:
        out = torch.empty((B, N, 1536), dtype=torch.bfloat16, device=q.device)
    _bf16(out)
    assert out.shape[:2] == (B, N) and out.shape[2] >= 1536 and out.stride(2) == 1
    _drop_sidecars(out)
    ws = torch.empty((2, B * N), dtype=torch.float32, device=q.device)
    es = out.element_size()
    L.check(L.load().udt_attn512_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(d_o), out.data_ptr(), out.data_ptr() + 512 * es,
                                     out.data_ptr() + 1024 * es, ws[0].data_ptr(), ws[1].data_ptr(), B, N, q.stride(1), k.stride(1),
                                     v.stride(1), o.stride(1), d_o.stride(1), out.stride(1), q.stride(0), k.stride(0), v.stride(0),
                                     o.stride(0), d_o.stride(0), out.stride(0), scale, _stream()), "udt_attn512_bwd")
    return out[..., :1536]


def denoised(f: torch.Tensor, noised: torch.Tensor, c_skip: torch.Tensor, c_out: torch.Tensor) -> torch.Tensor:
    """D = c_skip_b * noised + c_out_b * F, fp32 NCHW [B, 4, h, w]: f fp32 NHWC [B, h, w, ld] (the UNet head's output), noised fp32
    NCHW, c_skip / c_out fp32 [B] on the device (udt_denoised_f32, one launch)"""
    B, h, w, ld = f.shape
    assert f.dtype == torch.float32 and f.is_contiguous() and noised.dtype == torch.float32 and noised.is_contiguous()
    assert noised.shape == (B, 4, h, w)
    for t in (c_skip, c_out):
        assert t.dtype == torch.float32 and t.numel() == B and t.is_contiguous() and t.device == f.device
    out = torch.empty_like(noised)
    L.check(L.load().udt_denoised_f32(_ptr(f), _ptr(noised), _ptr(c_skip), _ptr(c_out), _ptr(out), B, h * w, ld, _stream()),
            "udt_denoised_f32")
    return out


def seed_add_(seed: torch.Tensor, g: torch.Tensor, c_out: torch.Tensor) -> torch.Tensor:
    """seed[b, y, x, c] += c_out_b * g[b, c, y, x] for the 4 latent channels, in place: seed bf16 NHWC [B, h, w, cpad] (the reverse
    pass's loss seed), g fp32 NCHW [B, 4, h, w], c_out fp32 [B] on the device (udt_seed_add_bf16, one launch)"""
    _bf16(seed)
    B, h, w, cpad = seed.shape
    assert seed.is_contiguous() and g.dtype == torch.float32 and g.is_contiguous() and g.shape == (B, 4, h, w)
    assert c_out.dtype == torch.float32 and c_out.numel() == B and c_out.is_contiguous() and c_out.device == seed.device
    _drop_sidecars(seed)
    L.check(L.load().udt_seed_add_bf16(_ptr(seed), _ptr(g), _ptr(c_out), B, h * w, cpad, _stream()), "udt_seed_add_bf16")
    return seed


def xattention_bwd(k: torch.Tensor, v: torch.Tensor, probs: torch.Tensor, d_probs: Optional[torch.Tensor],
                   d_o: Optional[torch.Tensor], heads: int, scale: float) -> torch.Tensor:
    """dq of the text cross-attention: k, v row views [B, L, *] (as ``xattention``), probs / d_probs fp32 [B * heads, Nq, L],
    d_o bf16 [B, Nq, heads * 64] -> dq bf16 [B, Nq, heads * 64]"""
    B, Lc = k.shape[0], k.shape[1]
    Nq = probs.shape[1]
    assert probs.dtype == torch.float32 and probs.is_contiguous() and probs.shape == (B * heads, Nq, Lc)
    assert k.stride(2) == 1 and v.stride(2) == 1 and k.stride(1) == v.stride(1) and k.stride(0) == Lc * k.stride(1) == v.stride(0)
    if d_probs is not None:
        assert d_probs.dtype == torch.float32 and d_probs.is_contiguous() and d_probs.shape == probs.shape
    if d_o is not None:
        _bf16(d_o)
        assert d_o.is_contiguous() and d_o.shape == (B, Nq, heads * 64)
    dq = torch.empty((B, Nq, heads * 64), dtype=torch.bfloat16, device=probs.device)
    L.check(L.load().udt_xattn_bwd(_ptr(k), _ptr(v), _ptr(probs), _ptr(d_probs), _ptr(d_o), _ptr(dq), B, heads, 64, Nq, Lc,
                                   k.stride(1), heads * 64, heads * 64, scale, _stream()), "udt_xattn_bwd")
    return dq


def local_loss_bwd(probs: torch.Tensor, mask: torch.Tensor, seg_mask: torch.Tensor, gk9: torch.Tensor, d_probs: torch.Tensor,
                   loss: Optional[torch.Tensor], heads: int, size: int, weight: float) -> None:
    """d_probs += weight * d(local-loss term of this layer) / d probs (and loss += the term): udt_local_loss_bwd"""
    B = mask.shape[0]
    n, Lc = _ll_dims(probs, B, heads, loss, d_probs)
    scratch = _ll_scratch(probs, n, seg_mask.shape[1], 2)
    L.check(L.load().udt_local_loss_bwd(_ptr(probs), _ptr(mask), _ptr(seg_mask), _ptr(gk9), _ptr(d_probs), _ptr(loss), _ptr(scratch), n, B,
                                        heads, size, Lc, seg_mask.shape[1], mask.shape[2], mask.shape[3], weight, _stream()),
            "udt_local_loss_bwd")


def local_loss_bwd_hw(probs: torch.Tensor, mask: torch.Tensor, seg_mask: torch.Tensor, gk9: torch.Tensor, d_probs: torch.Tensor,
                      loss: Optional[torch.Tensor], heads: int, hw, weight: float) -> None:
    """``local_loss_bwd`` on h x w maps: udt_local_loss_bwd_hw"""
    h, w = _check_map_hw(probs, hw, "local_loss_bwd_hw")
    B = mask.shape[0]
    n, Lc = _ll_dims(probs, B, heads, loss, d_probs)
    scratch = _ll_scratch(probs, n, seg_mask.shape[1], 2)
    L.check(L.load().udt_local_loss_bwd_hw(_ptr(probs), _ptr(mask), _ptr(seg_mask), _ptr(gk9), _ptr(d_probs), _ptr(loss), _ptr(scratch), n,
                                           B, heads, h, w, Lc, seg_mask.shape[1], mask.shape[2], mask.shape[3], weight, _stream()),
            "udt_local_loss_bwd_hw")


def layer_norm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, eps: float = 1e-5,
                   add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dX of LayerNorm (statistics recomputed from x) + ``add`` (the gradient arriving over the residual connection)"""
    _bf16(x); _bf16(dy)
    assert x.is_contiguous() and dy.is_contiguous() and dy.shape == x.shape and (add is None or (add.is_contiguous() and add.shape == x.shape))
    Cc = x.shape[-1]
    dx = torch.empty_like(x)
    L.check(L.load().udt_layernorm_bwd(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(add), _ptr(dx), x.numel() // Cc, Cc, eps, _stream()),
            "udt_layernorm_bwd")
    return dx


GN_BWD_CHUNKED = os.environ.get("UDT_GN_BWD_CHUNKED", "1") != "0"     # 0: one workgroup per (sample, group) (A/B, tests)


def group_norm_bwd(x: torch.Tensor, dy: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, groups: int, eps: float, silu: bool,
                   add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dX of GroupNorm (+ SiLU) on bf16 NHWC [B, ..., C] (statistics recomputed from x) + ``add``"""
    _bf16(x); _bf16(dy)
    assert x.is_contiguous() and dy.is_contiguous() and dy.shape == x.shape and (add is None or (add.is_contiguous() and add.shape == x.shape))
    B, Cc = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * Cc)
    dx = torch.empty_like(x)
    lib = L.load()
    part = torch.empty((2, B, lib.udt_gn_nchunks(HW, Cc), groups, 2), dtype=torch.float32, device=x.device) if GN_BWD_CHUNKED else None
    L.check(lib.udt_gn_bwd(_ptr(x), _ptr(dy), _ptr(gamma), _ptr(beta), _ptr(add), _ptr(dx), _ptr(part), B, HW, Cc, groups,
                           eps, 1 if silu else 0, _stream()), "udt_gn_bwd")
    return dx


def geglu(ag: torch.Tensor) -> torch.Tensor:
    """x * gelu(gate) of stored pre-activations ag bf16 [rows, 2 * inner] = [x | gate]"""
    _bf16(ag)
    assert ag.is_contiguous() and ag.dim() == 2
    inner = ag.shape[1] // 2
    out = torch.empty((ag.shape[0], inner), dtype=torch.bfloat16, device=ag.device)
    L.check(L.load().udt_geglu_fwd(_ptr(ag), _ptr(out), ag.shape[0], inner, _stream()), "udt_geglu_fwd")
    return out


def geglu_bwd(ag: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    _bf16(ag); _bf16(dy)
    inner = ag.shape[1] // 2
    assert ag.is_contiguous() and dy.is_contiguous() and dy.shape == (ag.shape[0], inner)
    dag = torch.empty_like(ag)
    L.check(L.load().udt_geglu_bwd(_ptr(ag), _ptr(dy), _ptr(dag), ag.shape[0], inner, _stream()), "udt_geglu_bwd")
    return dag


def sum2x2(dy: torch.Tensor) -> torch.Tensor:
    """nearest x2 upsampling backward: bf16 NHWC [B, 2H, 2W, C] -> [B, H, W, C]"""
    _bf16(dy)
    assert dy.is_contiguous() and dy.shape[1] % 2 == 0 and dy.shape[2] % 2 == 0
    B, H2, W2, Cc = dy.shape
    dx = torch.empty((B, H2 // 2, W2 // 2, Cc), dtype=torch.bfloat16, device=dy.device)
    L.check(L.load().udt_sum2x2_bf16(_ptr(dy), _ptr(dx), B, H2 // 2, W2 // 2, Cc, _stream()), "udt_sum2x2_bf16")
    return dx


def center_tokens(ctx: torch.Tensor) -> torch.Tensor:
    """fp32 [B, L, D] -> bf16 [B, L, D]: every token minus the mean over the sample's L tokens (udt_center_tokens)"""
    assert ctx.dtype == torch.float32 and ctx.is_contiguous() and ctx.dim() == 3
    B, Lc, D = ctx.shape
    out = torch.empty((B, Lc, D), dtype=torch.bfloat16, device=ctx.device)
    L.check(L.load().udt_center_tokens(_ptr(ctx), _ptr(out), B, Lc, D, _stream()), "udt_center_tokens")
    return out


def axpy_(x: torch.Tensor, y: torch.Tensor, a: float) -> torch.Tensor:
    """x += a * y (fp32, in place)"""
    assert x.dtype == torch.float32 == y.dtype and x.is_contiguous() and y.is_contiguous() and x.numel() == y.numel()
    L.check(L.load().udt_axpy_f32(_ptr(x), _ptr(y), a, x.numel(), _stream()), "udt_axpy_f32")
    return x


def aae_row_update_(x: torch.Tensor, grad: torch.Tensor, loss: torch.Tensor, state_in: torch.Tensor, state_out: torch.Tensor,
                    n_active: torch.Tensor, alpha: float, thres: float, iter_enabled: bool, max_iter: int) -> torch.Tensor:
    """the row-wise attend-and-excite update (udt_aae_row_update_f32): active rows of x fp32 [B, ...] take x -= alpha * grad, in
    place; state_in / state_out int32 [2, B] (active flags, update counts; two distinct buffers), n_active int32 [1]"""
    assert x.dtype == torch.float32 == grad.dtype == loss.dtype and x.is_contiguous() and grad.is_contiguous() and loss.is_contiguous()
    B = x.shape[0] if x.dim() else 0
    assert x.shape == grad.shape and loss.numel() == B
    for st in (state_in, state_out):
        assert st.dtype == torch.int32 and st.is_contiguous() and tuple(st.shape) == (2, B)
    assert n_active.dtype == torch.int32 and n_active.numel() == 1
    L.check(L.load().udt_aae_row_update_f32(_ptr(x), _ptr(grad), _ptr(loss), _ptr(state_in), _ptr(state_out), _ptr(n_active), B,
                                            x.numel() // max(B, 1), alpha, thres, int(bool(iter_enabled)), int(max_iter), _stream()),
            "udt_aae_row_update_f32")
    return x


# ------------------------------------------------------------------------------------------ training step (csrc/backward.hip)
def transpose(x: torch.Tensor) -> torch.Tensor:
    """bf16 [R, C] (row-strided view allowed) -> [C, Rp], Rp = R rounded up to 64, zero-padded (operand of a dW = dY^T X GEMM)"""
    _bf16(x)
    assert x.dim() == 2 and x.stride(1) == 1
    R, Cc = x.shape
    Rp = (R + 63) // 64 * 64
    out = torch.empty((Cc, Rp), dtype=torch.bfloat16, device=x.device)
    L.check(L.load().udt_transpose_bf16(_ptr(x), _ptr(out), R, Cc, x.stride(0), Rp, _stream()), "udt_transpose_bf16")
    return out


WGRAD_KERNEL = os.environ.get("UDT_WGRAD_KERNEL", "1") != "0"     # 0: transposes + the forward GEMM (A/B, tests)


def _acc_dst(out: torch.Tensor, shape) -> None:
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(shape), (out.dtype, out.shape, shape)


def weight_grad(dy: torch.Tensor, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dW fp32 [N, K] = dy^T x for dy bf16 [M, N], x bf16 [M, K] (nn.Linear: y = x W^T), contraction over the M rows with fp32
    accumulation and output: udt_wgrad_bf16 straight from the row-major operands (or, switched off / for shapes it does not take, the
    forward GEMM on the two operands transposed).  ``out``: an fp32 [N, K] view (a gradient bucket's) that the result is ADDED to —
    udt_wgrad_bf16_acc; the fallback adds its result with udt_axpy_f32"""
    _bf16(dy); _bf16(x)
    assert dy.dim() == 2 and x.dim() == 2 and dy.shape[0] == x.shape[0] and dy.stride(1) == 1 and x.stride(1) == 1
    R, N = dy.shape
    K = x.shape[1]
    lib = L.load()
    if out is not None:
        _acc_dst(out, (N, K))
    if not WGRAD_KERNEL or N % 8 or K % 8 or dy.stride(0) % 8 or x.stride(0) % 8 or (dy.data_ptr() | x.data_ptr()) & 15:
        dw = linear(transpose(dy), transpose(x), None, flags=L.GEMM_OUT_F32)
        if out is None:
            return dw
        axpy_(out.view(-1), dw.contiguous().view(-1), 1.0)
        return out
    S = lib.udt_wgrad_splits(R, N, K)
    part = torch.empty((S, N, K), dtype=torch.float32, device=dy.device) if S > 1 else None
    if out is not None:
        L.check(lib.udt_wgrad_bf16_acc(_ptr(dy), _ptr(x), _ptr(out), _ptr(part), R, N, K, dy.stride(0), x.stride(0), 1, _stream()),
                "udt_wgrad_bf16_acc")
        return out
    dw = torch.empty((N, K), dtype=torch.float32, device=dy.device)
    L.check(lib.udt_wgrad_bf16(_ptr(dy), _ptr(x), _ptr(dw), _ptr(part), R, N, K, dy.stride(0), x.stride(0), _stream()), "udt_wgrad_bf16")
    return dw


def colsum(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 [C] column sums of bf16 [rows, C] (bias gradient); ``out``: an fp32 [C] view the sums are ADDED to (udt_colsum_bf16_acc)"""
    _bf16(x)
    assert x.is_contiguous() and x.dim() == 2
    rows, Cc = x.shape
    lib = L.load()
    part = torch.empty((lib.udt_colparts(rows), Cc), dtype=torch.float32, device=x.device)
    if out is not None:
        _acc_dst(out, (Cc,))
        L.check(lib.udt_colsum_bf16_acc(_ptr(x), _ptr(part), _ptr(out), rows, Cc, 1, _stream()), "udt_colsum_bf16_acc")
        return out
    out = torch.empty((Cc,), dtype=torch.float32, device=x.device)
    L.check(lib.udt_colsum_bf16(_ptr(x), _ptr(part), _ptr(out), rows, Cc, _stream()), "udt_colsum_bf16")
    return out


def layer_norm_param_grad(x: torch.Tensor, dy: torch.Tensor, eps: float = 1e-5, out: Optional[torch.Tensor] = None):
    """(d gamma, d beta) fp32 [C] each of LayerNorm over bf16 rows x with output cotangent dy; ``out``: an fp32 [2, C] view
    (d gamma over d beta) both are ADDED to (udt_ln_param_grad_acc)"""
    _bf16(x); _bf16(dy)
    assert x.is_contiguous() and dy.is_contiguous() and x.shape == dy.shape and x.dim() == 2
    rows, Cc = x.shape
    lib = L.load()
    part = torch.empty((lib.udt_colparts(rows), 2, Cc), dtype=torch.float32, device=x.device)
    if out is not None:
        _acc_dst(out, (2, Cc))
        L.check(lib.udt_ln_param_grad_acc(_ptr(x), _ptr(dy), _ptr(part), _ptr(out), rows, Cc, eps, 1, _stream()), "udt_ln_param_grad_acc")
        return out[0], out[1]
    out = torch.empty((2, Cc), dtype=torch.float32, device=x.device)
    L.check(lib.udt_ln_param_grad(_ptr(x), _ptr(dy), _ptr(part), _ptr(out), rows, Cc, eps, _stream()), "udt_ln_param_grad")
    return out[0], out[1]


def xattention_bwd_kv(q: torch.Tensor, v: torch.Tensor, probs: torch.Tensor, d_probs: Optional[torch.Tensor],
                      d_o: Optional[torch.Tensor], heads: int, scale: float):
    """(dk, dv) bf16 [B, L, heads * 64] of the text cross-attention: q bf16 [B, Nq, C], v a row view [B, L, *]"""
    _bf16(q)
    B, Nq, Cc = q.shape
    Lc = v.shape[1]
    assert q.is_contiguous() and v.stride(2) == 1 and v.stride(0) == Lc * v.stride(1) and probs.shape == (B * heads, Nq, Lc)
    dk = torch.empty((B, Lc, Cc), dtype=torch.bfloat16, device=q.device)
    dv = torch.empty_like(dk)
    lib = L.load()
    part = torch.empty((lib.udt_xattn_kv_splits(Nq), B * Lc, Cc, 2), dtype=torch.float32, device=q.device)
    L.check(lib.udt_xattn_bwd_kv(_ptr(q), _ptr(v), _ptr(probs), _ptr(d_probs), _ptr(d_o), _ptr(dk), _ptr(dv), _ptr(part), B, heads, 64, Nq,
                                 Lc, Cc, v.stride(1), Cc, Cc, scale, _stream()), "udt_xattn_bwd_kv")
    return dk, dv


def local_loss_seg_bwd(probs: torch.Tensor, seg: torch.Tensor, seg_mask: torch.Tensor, gk9: torch.Tensor, d_probs: torch.Tensor,
                       loss: Optional[torch.Tensor], heads: int, size: int, weight: float) -> None:
    """FullLoss.get_local_loss per layer: d_probs += weight * d f / d probs, loss[b] += f_b (udt_local_loss_seg_bwd)"""
    B = seg.shape[0]
    _ll_dims(probs, B, heads, loss, d_probs, tiled=False)
    assert seg.dtype == torch.float32 and seg.is_contiguous() and seg_mask.is_contiguous() and seg.shape[1] == seg_mask.shape[1]
    scratch = _ll_scratch(probs, B, seg.shape[1])
    L.check(L.load().udt_local_loss_seg_bwd(_ptr(probs), _ptr(seg), _ptr(seg_mask), _ptr(gk9), _ptr(d_probs), _ptr(loss), _ptr(scratch), B,
                                            heads, size, probs.shape[-1], seg.shape[1], seg.shape[2], seg.shape[3], weight, _stream()),
            "udt_local_loss_seg_bwd")


def local_loss_seg_bwd_hw(probs: torch.Tensor, seg: torch.Tensor, seg_mask: torch.Tensor, gk9: torch.Tensor, d_probs: torch.Tensor,
                          loss: Optional[torch.Tensor], heads: int, hw, weight: float) -> None:
    """``local_loss_seg_bwd`` on h x w maps: udt_local_loss_seg_bwd_hw"""
    h, w = _check_map_hw(probs, hw, "local_loss_seg_bwd_hw")
    B = seg.shape[0]
    _ll_dims(probs, B, heads, loss, d_probs, tiled=False)
    assert seg.dtype == torch.float32 and seg.is_contiguous() and seg_mask.is_contiguous() and seg.shape[1] == seg_mask.shape[1]
    scratch = _ll_scratch(probs, B, seg.shape[1])
    L.check(L.load().udt_local_loss_seg_bwd_hw(_ptr(probs), _ptr(seg), _ptr(seg_mask), _ptr(gk9), _ptr(d_probs), _ptr(loss), _ptr(scratch),
                                               B, heads, h, w, probs.shape[-1], seg.shape[1], seg.shape[2], seg.shape[3], weight,
                                               _stream()), "udt_local_loss_seg_bwd_hw")


def diff_loss_grad(eps: torch.Tensor, noised: torch.Tensor, target: torch.Tensor, sigma: torch.Tensor, cpad: int = 64):
    """(loss fp32 [B], d_eps bf16 NHWC [B, h, w, cpad]) of the eps-prediction loss: eps fp32 NHWC [B, h, w, ld], noised / target fp32 NCHW"""
    B, h, w, ld = eps.shape
    assert eps.dtype == torch.float32 and eps.is_contiguous() and noised.is_contiguous() and target.is_contiguous()
    assert noised.shape == (B, 4, h, w) == target.shape and sigma.dtype == torch.float32 and sigma.numel() == B
    d_eps = torch.empty((B, h, w, cpad), dtype=torch.bfloat16, device=eps.device)
    loss = torch.empty((B,), dtype=torch.float32, device=eps.device)
    L.check(L.load().udt_diff_loss_grad(_ptr(eps), _ptr(noised), _ptr(target), _ptr(sigma), _ptr(d_eps), _ptr(loss), B, h * w, ld, cpad,
                                        _stream()), "udt_diff_loss_grad")
    return loss, d_eps


def precond_loss_grad(f: torch.Tensor, noised: torch.Tensor, target: torch.Tensor, c_skip: torch.Tensor, c_out: torch.Tensor,
                      w: torch.Tensor, cpad: int = 64):
    """(loss fp32 [B], d_f bf16 NHWC [B, h, w, cpad]) of mean(w_b (c_skip_b*noised + c_out_b*F - target)^2): udt_precond_loss_grad;
    f fp32 NHWC [B, h, w, ld], noised / target fp32 NCHW, c_skip / c_out / w fp32 [B] on the device"""
    B, h, ww, ld = f.shape
    assert f.dtype == torch.float32 and f.is_contiguous() and noised.is_contiguous() and target.is_contiguous()
    assert noised.shape == (B, 4, h, ww) == target.shape
    for t in (c_skip, c_out, w):
        assert t.dtype == torch.float32 and t.numel() == B and t.is_contiguous() and t.device == f.device
    d_f = torch.empty((B, h, ww, cpad), dtype=torch.bfloat16, device=f.device)
    loss = torch.empty((B,), dtype=torch.float32, device=f.device)
    L.check(L.load().udt_precond_loss_grad(_ptr(f), _ptr(noised), _ptr(target), _ptr(c_skip), _ptr(c_out), _ptr(w), _ptr(d_f),
                                           _ptr(loss), B, h * ww, ld, cpad, _stream()), "udt_precond_loss_grad")
    return loss, d_f


def adamw_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, step: int, lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
           weight_decay: float = 1e-2, grad_scale: float = 1.0) -> None:
    """torch.optim.AdamW's update of one fp32 tensor, in place (udt_adamw_f32); bumps the tensor's version so that cached packed
    layouts and captured graphs notice"""
    for t in (p, g, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == p.numel()
    L.check(L.load().udt_adamw_f32(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, betas[0], betas[1], eps, weight_decay, step,
                                   grad_scale, _stream()), "udt_adamw_f32")
    torch._C._increment_version(p)


def bucket_update_(segments: torch.Tensor, chunk_map: torch.Tensor, g: Optional[torch.Tensor], m: Optional[torch.Tensor],
                   v: Optional[torch.Tensor], mode: int, *, step: int = 0, lr: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                   weight_decay: float = 0.0, grad_scale: float = 1.0, one_minus_decay: float = 0.0) -> None:
    """the fused optimiser step over a device table of segments (udt_bucket_update_f32): ``segments`` uint8 [n_seg * 32] (an array of
    lib.BucketSegment), ``chunk_map`` int32 [n_chunks, 2]; mode = lib.BUCKET_ADAMW | lib.BUCKET_EMA.  The caller bumps the versions
    of the tensors behind the table's pointers"""
    assert chunk_map.dtype == torch.int32 and chunk_map.is_contiguous() and chunk_map.dim() == 2 and chunk_map.shape[1] == 2
    assert segments.dtype == torch.uint8 and segments.is_contiguous() and segments.numel() % C.sizeof(L.BucketSegment) == 0
    for t in (g, m, v):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    L.check(L.load().udt_bucket_update_f32(_ptr(segments), _ptr(chunk_map), chunk_map.shape[0], _ptr(g), _ptr(m), _ptr(v), mode, lr,
                                           betas[0], betas[1], eps, weight_decay, step, grad_scale, one_minus_decay, _stream()),
            "udt_bucket_update_f32")


def bucket_swap_(segments: torch.Tensor, chunk_map: torch.Tensor) -> None:
    """p <-> shadow over a device table of segments (udt_bucket_swap_f32)"""
    assert chunk_map.dtype == torch.int32 and chunk_map.is_contiguous() and chunk_map.dim() == 2 and chunk_map.shape[1] == 2
    assert segments.dtype == torch.uint8 and segments.is_contiguous()
    L.check(L.load().udt_bucket_swap_f32(_ptr(segments), _ptr(chunk_map), chunk_map.shape[0], _stream()), "udt_bucket_swap_f32")


# ------------------------------------------------------------------------------------------ profiling
def prof_enable(mask: int) -> None:
    L.check(L.load().udt_prof_enable(mask), "udt_prof_enable")


def prof_reset() -> None:
    L.check(L.load().udt_prof_reset(), "udt_prof_reset")


def prof_get(op_class: int):
    ms = C.c_double(0.0)
    n = C.c_int64(0)
    L.check(L.load().udt_prof_get(op_class, C.byref(ms), C.byref(n)), "udt_prof_get")
    return ms.value, n.value
