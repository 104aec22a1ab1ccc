"""A checker that localises (a helper, not a test; works on CPU and device tensors).

``check_sliced`` holds a kernel's result to its float64 reference slice by slice, where the slices follow the kernel's work
decomposition (one workgroup's / one tile's outputs), so that a defect in one unit of work lands in one slice instead of being
averaged over the tensor.  The bound of a slice is measured, not analysed: ``floor_err = emul - ref64``, where ``emul`` is the same
float64 computation rounded only where the kernel's header comment says it rounds (the stored result; for the flash-attention
backward also P and dS before the second products).  floor_err comes from the reference alone, never from the kernel's output.

    rms_s(got - ref64) <= margin_rms * rms_s(floor_err) + 2^-18 * A
    max_s|got - ref64| <= margin_max * max_s|floor_err| + 2^-18 * A          for every slice s

A (``abs_scale``) is the RMS over the whole tensor of the same formula with every summand replaced by its absolute value (the
condition-number scale; default rms(ref64)): 2^-18 A is about 64 fp32 ulps of the summands, the allowance for the kernel's fp32
arithmetic.  It is 4e-6 relative on benign inputs and keeps a correct kernel from failing on a slice whose terms cancel.
Margins 2 and 4: the recorded global ratios of kernel error to the pure output-rounding floor are 1.00 for every norm / elementwise
kernel and 1.45 for attention (before the emulation takes on the P / dS rounding), and a slice of >= 1024 elements estimates an RMS
to a few percent — so units smaller than 1024 elements are merged with their neighbours.

A slice whose ref64 is identically zero must be exactly zero in ``got``.  No slice is skipped: every element of ``got`` must be
covered exactly once (counted).

fp32 outputs of sums of exactly representable products (dW, column sums, d gamma / d beta, the fp32 row reduction) use the
element-wise form ``check_fp32_sum``:  |got - ref64| <= 16 * 2^-24 * sum|summands|  (only the accumulation rounds).

Every call appends one line to the parity report the kernel tests' ``_check`` writes (tests/test_backward_gpu.py REPORT): worst slice,
its ratio to the bound, global relative rms.
"""
import os

import torch

REPORT = None                   # None: the file tests/test_backward_gpu.py's _check appends to (one report for the whole run)
MIN_SLICE = 1024
ULP_ALLOWANCE = 2.0 ** -18
FP32_SUM_UNITS = 16.0           # units of 2^-24 of sum|summands|


def _f64(t):
    return torch.as_tensor(t).detach().double().cpu()


def _report(line, report=None):
    path = REPORT if report is None else report
    if path is None:
        import test_backward_gpu
        path = test_backward_gpu.REPORT
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "a") as f:
        f.write(line + "\n")


def _fmt(idx):
    def one(i):
        if isinstance(i, slice):
            return f"{'' if i.start is None else i.start}:{'' if i.stop is None else i.stop}"
        return str(int(i))
    return "[" + ", ".join(one(i) for i in (idx if isinstance(idx, tuple) else (idx,))) + "]"


# ------------------------------------------------------------------------------------------------ slice generators
def attn_slices(B, H, N, rows=32, head_dim=64):
    """[B, N, H * 64] (one of dq / dk / dv): (batch, head, 32-row block) — the rows one wave of udt_attn_bwd owns"""
    for b in range(B):
        for h in range(H):
            for r0 in range(0, N, rows):
                yield (b, slice(r0, min(N, r0 + rows)), slice(h * head_dim, (h + 1) * head_dim))


def row_col_slices(rows, C, rstep, cstep):
    """[rows, C]: rstep x cstep blocks (LayerNorm backward: 4-row workgroup x 512-column NCH chunk; wgrad: 128 x 128 output tiles)"""
    for r0 in range(0, rows, rstep):
        for c0 in range(0, C, cstep):
            yield (slice(r0, min(rows, r0 + rstep)), slice(c0, min(C, c0 + cstep)))


def gn_group_slices(B, C, groups):
    """[B, HW, C]: (sample, group)"""
    cpg = C // groups
    for b in range(B):
        for g in range(groups):
            yield (b, slice(None), slice(g * cpg, (g + 1) * cpg))


def gn_strip_slices(B, C, cw):
    """[B, HW, C]: (sample, strip of cw channels) — the gw consecutive groups one workgroup of the forward strip GroupNorm owns"""
    for b in range(B):
        for c0 in range(0, C, cw):
            yield (b, slice(None), slice(c0, c0 + cw))


def flat_slices(B, per_sample, step):
    """[B, per_sample] (a flattened sample): consecutive spans of ``step`` elements — GroupNorm backward's apply workgroup takes
    1024 16-byte pieces = 8192 elements"""
    for b in range(B):
        for i0 in range(0, per_sample, step):
            yield (b, slice(i0, min(per_sample, i0 + step)))


def block_slices(n, step=16):
    """[n]: blocks of ``step`` columns (the row reductions' workgroup)"""
    for i0 in range(0, n, step):
        yield (slice(i0, min(n, i0 + step)),)


def gemm_tile_slices(M, N, bm, bn, wr, wc, batch=None):
    """[M, N] (or [batch, M, N]): (M-tile, N-tile, wave row block of wr rows, wave column block of wc columns) of a bm x bn tiled GEMM,
    clipped at the ragged M and N tails — one wave's outputs of one tile"""
    for b in ([None] if batch is None else range(batch)):
        for m0 in range(0, M, bm):
            for n0 in range(0, N, bn):
                for r0 in range(m0, min(M, m0 + bm), wr):
                    for c0 in range(n0, min(N, n0 + bn), wc):
                        idx = (slice(r0, min(M, m0 + bm, r0 + wr)), slice(c0, min(N, n0 + bn, c0 + wc)))
                        yield idx if b is None else (b,) + idx


def conv_tile_slices(B, H, W, N, th, tw, bn, step=1):
    """[B, H, W, N] (NHWC output): (image, tile y, tile x, N-tile) of a convolution cut into th x tw pixel tiles and bn-column tiles;
    step 2: the phase form, whose tile of the low-resolution map owns the 2 th x 2 tw output pixels above it"""
    th, tw = th * step, tw * step
    for b in range(B):
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                for n0 in range(0, N, bn):
                    yield (b, slice(y0, min(H, y0 + th)), slice(x0, min(W, x0 + tw)), slice(n0, min(N, n0 + bn)))


def ring_slices(B, H, W):
    """[B, H, W, N]: each image's outer pixel ring (top row, bottom row, left and right columns) apart from its interior; the rings of
    all images come first so that merging short units never joins a ring to an interior"""
    for b in range(B):
        yield (b, slice(0, 1), slice(0, W), slice(None))
        if H > 1:
            yield (b, slice(H - 1, H), slice(0, W), slice(None))
        if H > 2:
            yield (b, slice(1, H - 1), slice(0, 1), slice(None))
            if W > 1:
                yield (b, slice(1, H - 1), slice(W - 1, W), slice(None))
    for b in range(B):
        if H > 2 and W > 2:
            yield (b, slice(1, H - 1), slice(1, W - 1), slice(None))


# ------------------------------------------------------------------------------------------------ the sliced check
def check_sliced(name, got, ref64, floor_err, slices, *, abs_scale=None, margin_rms=2.0, margin_max=4.0, report=None):
    """report: a file of its own for this call's line (default: the module's REPORT, see above)"""
    got, ref, floor = _f64(got), _f64(ref64), _f64(floor_err)
    assert got.shape == ref.shape == floor.shape, f"{name}: shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(floor.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    err = got - ref
    A = float(ref.pow(2).mean().sqrt()) if abs_scale is None else float(abs_scale)
    allow = ULP_ALLOWANCE * A
    cover = torch.zeros(got.shape, dtype=torch.int32)
    # units -> slices of at least MIN_SLICE elements (consecutive units merged; a short remainder joins the last slice)
    merged, cur = [], None
    for idx in slices:
        e, f, r, g = err[idx], floor[idx], ref[idx], got[idx]
        cover[idx] += 1
        unit = [e.numel(), float(e.pow(2).sum()), float(e.abs().max()) if e.numel() else 0.0, float(f.pow(2).sum()),
                float(f.abs().max()) if f.numel() else 0.0, bool((r == 0).all()), bool((g == 0).all()), idx]
        if cur is None:
            cur = unit
        else:
            cur = [cur[0] + unit[0], cur[1] + unit[1], max(cur[2], unit[2]), cur[3] + unit[3], max(cur[4], unit[4]),
                   cur[5] and unit[5], cur[6] and unit[6], cur[7]]
        if cur[0] >= MIN_SLICE:
            merged.append(cur)
            cur = None
    if cur is not None:
        if merged:
            m = merged[-1]
            merged[-1] = [m[0] + cur[0], m[1] + cur[1], max(m[2], cur[2]), m[3] + cur[3], max(m[4], cur[4]), m[5] and cur[5],
                          m[6] and cur[6], m[7]]
        else:
            merged.append(cur)
    covered = int(cover.sum())
    assert covered == got.numel() and int(cover.max()) == 1 and int(cover.min()) == 1, \
        f"{name}: the slices cover {covered} of {got.numel()} elements (each must be covered exactly once)"
    worst, worst_idx, worst_kind, failures = 0.0, None, "", []
    for n, e2, emax, f2, fmax, ref_zero, got_zero, idx in merged:
        if ref_zero:
            if not got_zero:
                failures.append(f"slice {_fmt(idx)}: the reference is identically zero, the result is not (max {emax:.3e})")
                worst, worst_idx, worst_kind = float("inf"), idx, "zero"
            continue
        b_rms = margin_rms * (f2 / n) ** 0.5 + allow
        b_max = margin_max * fmax + allow
        for kind, val, bound in (("rms", (e2 / n) ** 0.5, b_rms), ("max", emax, b_max)):
            ratio = val / bound if bound > 0 else (0.0 if val == 0 else float("inf"))
            if ratio > worst:
                worst, worst_idx, worst_kind = ratio, idx, kind
            if val > bound:
                failures.append(f"slice {_fmt(idx)} ({n} elements): {kind} error {val:.3e} > bound {bound:.3e}")
    rel = float(err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300))
    _report(f"{name:55s} sliced: {len(merged)} slices, worst {_fmt(worst_idx) if worst_idx is not None else '-'} {worst_kind} "
            f"ratio-to-bound {worst:.3f}, global rel_rms {rel:.3e}{'  FAIL' if failures else ''}", report)
    assert not failures, f"{name}: {len(failures)} of {len(merged)} slices out of bound; first: " + "; ".join(failures[:3])
    return worst


def check_fp32_sum(name, got, ref64, abs_sum, *, units=FP32_SUM_UNITS, report=None):
    """fp32 result of a sum of exact products: |got - ref64| <= units * 2^-24 * sum|summands| element by element (an element whose
    summands are all zero must be exactly zero).  Returns the worst |err| / sum|summands| in units of 2^-24."""
    got, ref, asum = _f64(got), _f64(ref64), _f64(abs_sum)
    assert got.shape == ref.shape == asum.shape, f"{name}: shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(asum.shape)}"
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values in the result"
    err = (got - ref).abs()
    bound = units * 2.0 ** -24 * asum
    ratio = torch.where(asum > 0, err / asum.clamp_min(1e-300) * 2.0 ** 24, torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                                     torch.zeros_like(err)))
    worst = float(ratio.max())
    bad = err > bound
    rel = float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300))
    at = tuple(int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)) if ratio.numel() else ()
    _report(f"{name:55s} fp32 sum: worst |err| / sum|summands| = {worst:.2f} x 2^-24 at {at} (bound {units:g}), "
            f"global rel_rms {rel:.3e}{'  FAIL' if bool(bad.any()) else ''}", report)
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {bad.numel()} elements beyond {units:g} x 2^-24 x sum|summands|; worst "
                                 f"{worst:.2f} units at {at}: got {float(got[at]):.9g}, ref {float(ref[at]):.9g}")
    return worst
