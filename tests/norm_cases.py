"""Case lists, inputs, launcher mirrors and the ``hold_*`` checks of the forward normalisation kernels (csrc/norm.hip) — a helper, not a
test; shared by tests/test_norm_ref_cpu.py (float32 restatements, planted defects) and tests/test_norm_edges_gpu.py (the kernels).

Branch of norm.hip -> the listed case that reaches it
  gn_stats_kernel, c8 <= 256 layout          every TWO_KERNEL case up to C = 2048: (2,1,64,0) R = 32 with 31 row groups idle, (1,9,320,0)
                                             R = 6 with 16 idle threads, (1,100,1024,0) R = 2 (4x unrolled loop + tail), (1,100,2048,0) R = 1
  gn_stats_kernel, strided layout (c8 > 256) (1,64,2560,0) threads 0..63 take two channel chunks; (1,16,4096,0) = GN_MAX_C
  gn_stats_kernel, empty trailing chunk      (2,289,320,0): 18 chunks of 17 rows, chunk 17 owns nothing -> partials exactly 0
  udt_gn_nchunks clamps                      HW < 16 -> 1: (2,1,64,0), (1,9,320,0);  > 128 -> 128: (1,2100,64,0), ragged last chunk
  gn_stats / gn_apply second source          (2,33,64,32) cpg 3, (2,100,320,64) cpg 12 (group straddles C1 and a 64-channel block),
                                             (1,289,1280,640) cpg 60
  gn_apply_kernel, partials table source     every TWO_KERNEL case;  scsh table source: every REC_TABLE case
  gn_apply_kernel, prefetching span          a workgroup of 1024 pieces: (1,2100,64,0) has 16 of them, (1,64,2560,0) only such
  gn_apply_kernel, tail-only span            (1,9,320,0) 360 pieces, (1,2100,64,0) the 17th workgroup (416 pieces)
  gn_apply_kernel, span of 769 .. 1023       (1,125,64,0), added to the issue's list: 1000 pieces, threads 0..231 prefetch four loads, the
                                             others walk the tail loop — the one span where both forms meet in one workgroup
    (the steady-state loop between the prefetched round and the tail cannot run: a workgroup owns 1024 pieces = one round)
  gn_strip_kernel gw 8 / 4 / 2 / 1           (2,33,64,32) / (2,9,320,0), (1,819,320,0) / (2,100,640,0), (1,64,1280,640), (1,16,3200,0) /
                                             (1,64,2560,0), (1,256,4096,0)
  gn_strip_kernel unrolled loop + tail       (1,819,320,0); unrolled, no tail: (1,256,4096,0); tail only: (1,64,1280,640); HW < pstep:
                                             (2,33,64,32), (2,9,320,0), (2,1,320,0); idle threads: (2,33,64,32) 2, (1,16,3200,0) 12
  gn_strip_groups admission                  (1,819,320,0) in / (1,820,320,0) out at cw 40; (1,256,4096,0) in / (1,257,4096,0) out at cw 128
  gn_strip_kernel with records               REC_STRIP: slots 1, 3, 7 and two sources with slots1 != slots2
  gn_finalize_kernel, records < slot lanes   (2,100,128,0) slots 3 of 64 lanes;  = lanes: (2,289,640,0) slots 12;  > lanes, ragged second
                                             round: (1,289,320,64) slots 23 of 21 lanes, (1,64,2560,0) 4 of 3, (1,16,4096,0) 5 of 2
  layernorm_kernel<1..8>                     LN_C: NCH = 1, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8; C = 8 one lane, C = 520 one lane in the second
                                             chunk; rows 1, 5, 7: the last workgroup of 4 rows part-filled
"""
import re

import torch

import norm_ref as R
import sliced_check as S

G = R.G
STRIP_LIMIT_BYTES = 64 << 10
APPLY_SPAN = 8192                       # elements one gn_apply workgroup owns: 1024 16-byte pieces

# (variant, eps, act): every case runs all five, so every kernel sees both eps values and both activations
VARIANTS = (("randn", 1e-5, 1), ("tails", 1e-6, 0), ("offset", 1e-6, 1), ("constant", 1e-5, 1), ("constant", 1e-6, 0))
LN_VARIANTS = (("randn", 1e-5), ("tails", 1e-6), ("offset", 1e-6), ("constant", 1e-5), ("constant", 1e-6))

# (B, HW, C1, C2)
TWO_KERNEL = ((2, 1, 64, 0), (1, 9, 320, 0), (2, 33, 640, 0), (2, 289, 320, 0), (1, 100, 1024, 0), (1, 100, 2048, 0), (1, 64, 2560, 0),
              (1, 16, 4096, 0), (1, 2100, 64, 0), (2, 33, 64, 32), (2, 100, 320, 64), (1, 289, 1280, 640),
              (1, 125, 64, 0))              # not in the issue's list: the apply span where prefetching and tail-only threads share a workgroup
STRIP = ((2, 1, 320, 0), (2, 33, 64, 32), (2, 9, 320, 0), (1, 819, 320, 0), (2, 100, 640, 0), (1, 64, 1280, 640), (1, 64, 2560, 0),
         (1, 16, 3200, 0), (1, 256, 4096, 0))
STRIP_GW = {(2, 1, 320, 0): 4, (2, 33, 64, 32): 8, (2, 9, 320, 0): 4, (1, 819, 320, 0): 4, (2, 100, 640, 0): 2, (1, 64, 1280, 640): 2,
            (1, 64, 2560, 0): 1, (1, 16, 3200, 0): 2, (1, 256, 4096, 0): 1}
STRIP_REFUSED = ((1, 820, 320, 0), (1, 257, 4096, 0))          # one pixel past the admission limit: must run as two kernels
# ((B, HW, C1, C2), slots1, slots2)
REC_STRIP = tuple(((s, n, 0) for s in ((2, 9, 320, 0), (2, 100, 640, 0), (1, 64, 2560, 0)) for n in (1, 3, 7))) + \
    (((2, 33, 64, 32), 3, 1), ((1, 64, 1280, 640), 2, 5))      # (2,9,320,0) at 7 slots of 2 rows: slots 5 and 6 are empty (zero records)
REC_TABLE = (((2, 100, 128, 0), 3, 0), ((2, 289, 640, 0), 12, 0), ((1, 289, 320, 64), 23, 2), ((1, 64, 2560, 0), 4, 0),
             ((1, 16, 4096, 0), 5, 0))                          # (1,16,4096,0) at 5 slots of 4 rows: slot 4 is empty
LN_C = (8, 384, 512, 520, 1024, 1280, 1536, 2048, 2560, 3072, 3584, 4096)
LN_ROWS = (1, 5, 7)


# ------------------------------------------------------------------------------------------------ mirrors of the launchers
def gn_nchunks(HW):
    """udt_gn_nchunks"""
    return max(1, min(128, HW // 16))


def gn_strip_groups(HW, C1, C2, groups=G, limit=True):
    """gn_strip_groups: groups per strip, 0 = not served (limit=False: the geometry alone, without the 64 KiB admission)"""
    C = C1 + C2
    if groups <= 0 or C % groups or C1 % 8 or C2 % 8:
        return 0
    cpg = C // groups
    gw = 1
    while (gw * cpg) % 8:
        gw *= 2
    if gw > 8 or groups % gw:
        return 0
    cw = gw * cpg
    if cw > 256:
        return 0
    if limit and HW * cw * 2 > STRIP_LIMIT_BYTES:
        return 0
    return gw


def strip_geometry(C1, C2, gw, groups=G):
    cw = gw * ((C1 + C2) // groups)
    nch = cw // 8
    pstep = R.STRIP_THREADS // nch
    return {"cw": cw, "nch": nch, "pstep": pstep, "idle": R.STRIP_THREADS - pstep * nch}


def stats_layout(C):
    """gn_stats_kernel's thread layout: (R row groups, idle threads, strided)"""
    c8 = C // 8
    if c8 <= 256:
        return 256 // c8, 256 - (256 // c8) * c8, False
    return 1, 0, True


def finalize_lanes(C, groups=G):
    return 256 // (C // groups)


def ln_nch(C):
    return (C + 511) // 512


def tags_two_kernel(B, HW, C1, C2):
    return [f"gn_stats B={B} HW={HW} C={C1 + C2}", f"gn_apply B={B} HW={HW} C={C1 + C2}"]


def tags_strip(B, HW, C1, C2, gw, records=False):
    return [f"gn_strip{'_stats' if records else ''} B={B} HW={HW} C={C1}+{C2} gw={gw}"]


def tags_table(B, HW, C1, C2, slots1):
    return [f"gn_finalize B={B} HW={HW} C={C1}+{C2} slots={slots1}", f"gn_apply_scsh B={B} HW={HW} C={C1 + C2}"]


# ------------------------------------------------------------------------------------------------ inputs
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def tail_pixels(HW, C1, C2):
    """the pixels the ``tails`` variant spikes: 0, HW - 1, the first and last pixel of every statistics chunk, and — where the strip
    kernel's geometry exists — its pstep-lane seams 4 pstep k - 1 / 4 pstep k and lane 0's first tail-loop pixel"""
    n = gn_nchunks(HW)
    rows = R.chunk_rows(HW, n)
    px = {0, HW - 1}
    for k in range(n):
        p0, p1 = k * rows, min(HW, (k + 1) * rows)
        if p0 < p1:
            px |= {p0, p1 - 1}
    gw = gn_strip_groups(HW, C1, C2, limit=False)
    if gw:
        pstep = strip_geometry(C1, C2, gw)["pstep"]
        for k in range(1, HW // (4 * pstep) + 1):
            px |= {4 * pstep * k - 1, 4 * pstep * k}
        px.add(R.strip_seam(HW, pstep))
    return sorted(p for p in px if 0 <= p < HW)


def _spike(C):
    return 16.0 * (1.0 - 2.0 * (torch.arange(C) % 2).float())            # + on even channels, - on odd ones


def _affine(C, g):
    return 1.0 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)


def gn_inputs(B, HW, C1, C2, variant):
    """-> (x [B, HW, C1], x2 [B, HW, C2] or None, gamma, beta): float32 CPU tensors, x / x2 holding bf16 values"""
    C = C1 + C2
    g = _gen(B, HW, C1, C2)
    z = torch.randn(B, HW, C, generator=g)
    x = 24.0 + 0.5 * z if variant == "offset" else 0.7 + 2.0 * z
    if variant == "tails":
        x[:, tail_pixels(HW, C1, C2), :] += _spike(C)
    elif variant == "constant":
        cpg = C // G
        x[:, :, 3 * cpg:4 * cpg] = 0.5
        x[:, :, C - cpg:] = -3.0
    else:
        assert variant in ("randn", "offset"), variant
    x = x.bfloat16().float()
    gamma, beta = _affine(C, g)
    return x[..., :C1].contiguous(), (x[..., C1:].contiguous() if C2 else None), gamma, beta


def ln_inputs(rows, C, variant):
    g = _gen(rows, C, 7)
    z = torch.randn(rows, C, generator=g)
    x = 24.0 + 0.5 * z if variant == "offset" else 0.7 + 2.0 * z
    if variant == "tails":
        cols = sorted({c for i in range(ln_nch(C)) for c in range(512 * i, min(C, 512 * i + 8))} | set(range(C - 8, C)))
        x[:, cols] += _spike(C)[cols]
    elif variant == "constant":
        x[0::3] = 0.5
    else:
        assert variant in ("randn", "offset"), variant
    gamma, beta = _affine(C, g)
    return x.bfloat16().float(), gamma, beta


def gn_records(x, x2, slots1, slots2):
    return R.records(x, slots1), (R.records(x2, slots2) if x2 is not None else None)


# ------------------------------------------------------------------------------------------------ the checks
def hold_gn(name, got, exp, unit, report=None):
    """a bf16 GroupNorm result [B, HW, C] against exp = {"ref", "emul", "A"}, twice: by (sample, group), and by the launch's own work unit —
    unit = ("span",): gn_apply's workgroup spans of 8192 elements of the flattened sample; ("strip", cw): (sample, strip of cw channels)"""
    ref, floor = exp["ref"], exp["emul"] - exp["ref"]
    B, HW, C = ref.shape
    got = got.reshape(B, HW, C)
    w = S.check_sliced(f"{name} by group", got, ref, floor, S.gn_group_slices(B, C, G), abs_scale=exp["A"], report=report)
    if unit[0] == "span":
        flat = lambda t: t.reshape(B, HW * C)
        w2 = S.check_sliced(f"{name} by span", flat(got), flat(ref), flat(floor), S.flat_slices(B, HW * C, APPLY_SPAN), abs_scale=exp["A"],
                            report=report)
    else:
        w2 = S.check_sliced(f"{name} by strip", got, ref, floor, S.gn_strip_slices(B, C, unit[1]), abs_scale=exp["A"], report=report)
    return max(w, w2)


def hold_partials(name, got, ref, ab, report=None):
    """udt_gn_stats' fp32 partials [B, nchunks, G, 2] against the float64 sums with sum|x| and sum x^2 (an empty chunk: exactly 0)"""
    w = S.check_fp32_sum(f"{name} partial sums", got[..., 0], ref[..., 0], ab[..., 0], report=report)
    return max(w, S.check_fp32_sum(f"{name} partial squares", got[..., 1], ref[..., 1], ab[..., 1], report=report))


def hold_table(name, got, t, report=None):
    """udt_gn_finalize's fp32 table [B, C/64, 2, 64] against table_from_records: scale with |sc|, shift with |beta| + |mean sc|"""
    w = S.check_fp32_sum(f"{name} table scale", got[:, :, 0], t["table"][:, :, 0], t["abs"][:, :, 0], report=report)
    return max(w, S.check_fp32_sum(f"{name} table shift", got[:, :, 1], t["table"][:, :, 1], t["abs"][:, :, 1], report=report))


def hold_ln(name, got, exp, x, beta, report=None):
    """a bf16 LayerNorm result [rows, C]: 4-row workgroup x 512-column lane chunk slices; a constant row is bf16(beta) bit for bit (every
    partial sum of <= 4096 equal bf16 values is exact in fp32, so v - mean is exactly 0)"""
    rows, C = exp["ref"].shape
    w = S.check_sliced(name, got, exp["ref"], exp["emul"] - exp["ref"], S.row_col_slices(rows, C, 4, 512), abs_scale=exp["A"], report=report)
    const = (x == x[:, :1]).all(dim=1).cpu()
    if bool(const.any()):
        want = beta.float().bfloat16().cpu()
        assert torch.equal(got.cpu()[const], want[None, :].expand(int(const.sum()), C)), f"{name}: a constant row is not bf16(beta) bit for bit"
    return w


# ------------------------------------------------------------------------------------------------ one case, any implementation
# ``impl`` is the code under test: the float32 restatement (CPU suite) or the launches (GPU suite).  It gets the inputs on ``dev`` as
# float32 tensors holding bf16 values; the references are float64 on the same device.
def _on(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


def _name(kind, shape, variant, eps, act, extra=""):
    B, HW, C1, C2 = shape
    return f"edge gn {kind} B{B} HW{HW} C{C1}+{C2}{extra} {variant} eps{eps:g} act{act}"


def case_two_kernel(shape, variant, eps, act, impl, dev="cpu", report=None):
    """impl(x, x2, gamma, beta, eps, act, nchunks) -> (y bf16 [B, HW, C], partials fp32 [B, nchunks, G, 2]); -> worst (sliced ratio, units)"""
    B, HW, C1, C2 = shape
    x, x2, gamma, beta = _on(dev, *gn_inputs(*shape, variant))
    n = gn_nchunks(HW)
    y, part = impl(x, x2, gamma, beta, eps, act, n)
    name = _name("stats+apply", shape, variant, eps, act)
    w = hold_gn(name, y, R.gn_expect(x, gamma, beta, eps, act, x2), ("span",), report)
    return w, hold_partials(name, part, *R.stats_partials(x, n, x2), report=report)


def case_strip(shape, variant, eps, act, impl, dev="cpu", report=None):
    """impl(x, x2, gamma, beta, eps, act, gw) -> y"""
    B, HW, C1, C2 = shape
    gw = gn_strip_groups(HW, C1, C2)
    assert gw == STRIP_GW[shape], (shape, gw)
    x, x2, gamma, beta = _on(dev, *gn_inputs(*shape, variant))
    y = impl(x, x2, gamma, beta, eps, act, gw)
    return hold_gn(_name("strip", shape, variant, eps, act, f" gw{gw}"), y, R.gn_expect(x, gamma, beta, eps, act, x2),
                   ("strip", strip_geometry(C1, C2, gw)["cw"]), report)


def case_records(form, shape, slots1, slots2, variant, eps, act, impl, dev="cpu", report=None):
    """form "strip" | "table"; impl(x, x2, rec1, slots1, rec2, slots2, gamma, beta, eps, act) -> (y, table fp32 [B, C/64, 2, 64] or None)"""
    B, HW, C1, C2 = shape
    x, x2, gamma, beta = _on(dev, *gn_inputs(*shape, variant))
    rec1, rec2 = gn_records(x, x2, slots1, slots2)
    y, table = impl(x, x2, rec1, slots1, rec2, slots2, gamma, beta, eps, act)
    name = _name(f"records {form}", shape, variant, eps, act, f" slots{slots1}+{slots2}")
    exp = R.gn_expect_records(x, rec1, slots1, gamma, beta, eps, act, x2, rec2, slots2)
    if form == "strip":
        gw = gn_strip_groups(HW, C1, C2)
        assert gw == STRIP_GW[shape], (shape, gw)
        return hold_gn(name, y, exp, ("strip", strip_geometry(C1, C2, gw)["cw"]), report), 0.0
    w = hold_gn(name, y, exp, ("span",), report)
    return w, hold_table(name, table, R.table_from_records(rec1, slots1, gamma, beta, HW, eps, rec2, slots2), report)


def case_ln(rows, C, variant, eps, impl, dev="cpu", report=None):
    """impl(x, gamma, beta, eps) -> y bf16 [rows, C]"""
    x, gamma, beta = _on(dev, *ln_inputs(rows, C, variant))
    y = impl(x, gamma, beta, eps)
    return hold_ln(f"edge layernorm<{ln_nch(C)}> rows{rows} C{C} {variant} eps{eps:g}", y, R.ln_expect(x, gamma, beta, eps), x, beta, report)


def failed_slices(msg):
    """(failing slices, total slices, [index ranges of the first reported slices]) from check_sliced's assertion text"""
    m = re.search(r"(\d+) of (\d+) slices out of bound", msg)
    idxs = []
    for s in re.findall(r"slice \[([^\]]*)\]", msg):
        idx = []
        for part in s.split(", "):
            if ":" in part:
                a, b = part.split(":")
                idx.append((int(a) if a else None, int(b) if b else None))
            else:
                idx.append((int(part), int(part) + 1))
        idxs.append(idx)
    return int(m.group(1)), int(m.group(2)), idxs
