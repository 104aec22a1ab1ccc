"""Inputs, shape lists, pure-Python mirrors of the planners and the shared checks of the forward GEMM / convolution edge cases (udt_gemm,
csrc/gemm.hip): tests/test_gemm_ref_cpu.py (float32 CPU evaluation, planted defects, coverage of the lists) and
tests/test_gemm_edges_gpu.py (the kernels) use the same ones.  A helper, not a test.  Every tensor is float32 holding bf16 values unless
the kernel takes fp32.  The lists are the smallest shapes that reach each branch of the dispatcher: no operand above ~4 M elements,
M N K <= 2e9 per case.

Out of scope: the MX8 / q8 forms (tests/mx8_ref.py and their own bounds), ``cu_share > 1`` plans, and anything that makes a stream-K
launch time out (UDT_ERR_ASYNC keeps its existing test; nothing here provokes it).
"""
import math
import re
import zlib
from types import SimpleNamespace

import torch

import gemm_ref as R
import sliced_check as S

MARKER = 123.0
PAD_ROWS = 3
PAD_COLS = 8                                    # (a multiple of 8 keeps every leading dimension 16-byte aligned)
BK = 64
F_F32, F_GEGLU, F_RELU, F_TRANS, F_CONV, F_SILU = 1, 2, 4, 8, 16, 32        # lib.GEMM_* (tests/test_gemm_edges_gpu.py asserts they agree)
KNOB_DEFAULTS = {"lean": -1, "lean_splitk": -1, "lean_conv": -1, "wide_conv": -1, "conv_n4": -1, "rowres": -1, "rows_epi": 1, "n_block": -1}


def _bf(t):
    return t.bfloat16().float()


# ================================================================================================ descriptors
def describe(c):
    """the udt_gemm_desc fields the planners read, from a case"""
    k = dict(KNOB_DEFAULTS)
    k.update(c.get("knobs", {}))
    d = SimpleNamespace(knobs=k, batch=c.get("batch", 1), flags=0, alpha=c.get("alpha", 1.0), residual=bool(c.get("res")),
                        rowvec=bool(c.get("rowvec")), bias=c.get("bias", True), ln=bool(c.get("ln")), in_scsh=c.get("gn") is not None,
                        colstats=bool(c.get("stats")), in_act=c.get("gn") or 0, ksize=0, stride=0, pad_t=0, pad_l=0, upsample=0,
                        C1=0, C2=0, Hin=0, Win=0, Hout=0, Wout=0, ldw=0, ld_rowvec=0)
    act = c.get("act")
    d.flags |= (F_F32 if c.get("f32") else 0) | (F_GEGLU if c.get("geglu") else 0) | (F_RELU if act == "relu" else 0) | \
        (F_SILU if act == "silu" else 0) | (F_TRANS if c.get("trans") else 0)
    if c["kind"] == "gemm":
        d.M, d.N, d.K = c["M"], c["N"], c["K"]
        la, lo, lr = c.get("ld_extra", (0, 0, 0))
        n_cols = d.N // 2 if c.get("geglu") else d.N
        d.lda, d.ldo, d.ldr = d.K + la, n_cols + lo, (n_cols + lr if d.residual else 0)
        d.rows_per_batch = c.get("trans") or c.get("rowvec") or c.get("stats") or 0
    else:
        d.flags |= F_CONV
        B, H, W = c["B"], c["H"], c["W"]
        d.ksize, d.stride, (d.pad_t, d.pad_l), d.upsample = c.get("ksize", 3), c.get("stride", 1), c.get("pad", (1, 1)), c.get("ups", 0)
        if d.ksize == 1:
            d.pad_t = d.pad_l = 0
        d.C1, d.C2, d.Hin, d.Win = c["C1"], c.get("C2", 0), H, W
        Hv, Wv = (2 * H, 2 * W) if d.upsample else (H, W)
        d.Hout, d.Wout = c.get("out_hw") or ((Hv + 2 * d.pad_t - d.ksize) // d.stride + 1, (Wv + 2 * d.pad_l - d.ksize) // d.stride + 1)
        d.M, d.N, d.K = B * d.Hout * d.Wout, c["N"], d.ksize * d.ksize * (d.C1 + d.C2)
        d.lda, d.ldo, d.ldr = 0, d.N + c.get("ld_extra", (0, 0, 0))[1], (d.N + c.get("ld_extra", (0, 0, 0))[2] if d.residual else 0)
        d.rows_per_batch = d.Hout * d.Wout
        if d.upsample == 2:
            d.ldw = 4 * d.C1
    return d


# ================================================================================================ mirrors of the planners
def round_workgroups(G):
    """gemm.hip: ``int round_workgroups(int G) { return G > 8 ? ((G + 7) & ~7) : G; }``"""
    return ((G + 7) & ~7) if G > 8 else G


def plan_tiles(d, cus):
    """gemm.hip plan_tiles (first-generation kernel; cu_share 1: ``slots = 2 * device_cus()``)"""
    tall = d.M >= 1024
    if d.N <= 64 or (tall and d.N % 128 != 0 and d.N % 128 <= 64):      # ``if (d->N <= 64 || (tall && (d->N % 128) != 0 && (d->N % 128) <= 64))``
        bm, bn = 256, 64
    else:
        bm, bn = 128, 128
    if d.flags & (F_TRANS | F_GEGLU):
        bm, bn = 128, 128
    tiles_m, tiles_n = (d.M + bm - 1) // bm, (d.N + bn - 1) // bn
    tiles = tiles_m * tiles_n * d.batch
    nkt = d.K // BK
    total = tiles * nkt
    slots = 2 * cus
    share = (total + slots - 1) // slots
    if tiles < slots // 2 and nkt >= 16:                                  # ``if (t.tiles < slots / 2 && t.nkt >= 16)``
        G = min(max(total // 8, 1), slots)
        ipw = (total + G - 1) // G
    elif tiles >= 8 * slots:
        ipw = ((tiles + slots - 1) // slots) * nkt
    elif share >= 160 and tiles % slots != 0:
        ipw = share
    else:
        ipw = nkt
    return SimpleNamespace(bm=bm, bn=bn, tiles_m=tiles_m, tiles_n=tiles_n, tiles=tiles, nkt=nkt, total=total, ipw=ipw,
                           G=(total + ipw - 1) // ipw, fixup=ipw % nkt != 0)


def use_gemm8(d):
    """gemm.hip use_gemm8: ``if (d->N <= 64) return false;`` (the 31-bit operand limits are far from these shapes)"""
    return d.N > 64


def plan_tiles8(d, cus):
    """gemm.hip plan_tiles8 (cu_share 1)"""
    gt = bool(d.flags & (F_TRANS | F_GEGLU))
    bm = 256
    bn = 160 if (not gt and d.N % 160 == 0 and d.N % 128 != 0) else 128   # ``t.bn = (!geglu_or_trans && d->N % 160 == 0 && d->N % 128 != 0) ? 160 : 128``
    tiles_m, tiles_n = (d.M + bm - 1) // bm, (d.N + bn - 1) // bn
    tiles = tiles_m * tiles_n * d.batch
    nkt = d.K // BK
    total = tiles * nkt
    whole = nkt < 24                                                     # ``const bool whole = t.nkt < 24 || prefer_whole_tiles(d, t.tiles)``
    slots = 2 * cus // 2
    G = min(max(total // 4, 1), slots)                                   # ``long long G = t.total / 4``
    ipw = (total + G - 1) // G
    if whole:
        ipw = ((ipw + nkt - 1) // nkt) * nkt
    return SimpleNamespace(bm=bm, bn=bn, tiles_m=tiles_m, tiles_n=tiles_n, tiles=tiles, nkt=nkt, total=total, ipw=ipw,
                           G=round_workgroups((total + ipw - 1) // ipw), fixup=ipw % nkt != 0)


def patch_rows(TN, gn):
    """conv3p.h: ``constexpr int patch_rows(int TN, bool GN) { return (TN == 5 && GN) ? 344 : 400; }``"""
    return 344 if (TN == 5 and gn) else 400


def conv3p_geometry(d, gn):
    """gemm.hip conv3p_geometry -> Geo or None"""
    if not gn:                                                           # ``if (!gn) return false;``
        return None
    if not (d.flags & F_CONV) or d.ksize != 3 or d.stride != 1 or d.upsample:
        return None
    if d.pad_t != 1 or d.pad_l != 1 or d.N <= 64 or d.Hout != d.Hin or d.Wout != d.Win:
        return None
    if d.flags & (F_GEGLU | F_TRANS):
        return None
    if d.C1 <= 0 or d.C1 % 64 or d.C2 < 0 or d.C2 % 64:
        return None
    H, W = d.Hout, d.Wout
    if W % 32 == 0 and H % 8 == 0:
        TW, TH, NI = 32, 8, 1
    elif W % 16 == 0 and H % 16 == 0:
        TW, TH, NI = 16, 16, 1
    elif W == 8 and H == 8:
        TW, TH, NI = 8, 8, 4
    else:
        return None
    g = SimpleNamespace(TW=TW, TH=TH, NI=NI, B=d.M // (H * W), H=H, W=W, C=d.C1 + d.C2, tiles_x=W // TW, tiles_y=H // TH)
    g.img_groups = (g.B + NI - 1) // NI
    g.prow_w = TW + 2
    g.prows_img = (TH + 2) * g.prow_w
    g.n_pieces = (NI * g.prows_img + 7) // 8
    g.chunks = g.C // 64
    bn = 160 if (d.N % 160 == 0 and d.N % 128 != 0) else 128
    # ``return ge.n_pieces * 8 <= c3p::patch_rows(bn == 160 ? 5 : 2, gn) && ge.n_pieces >= 8;``
    return g if (g.n_pieces * 8 <= patch_rows(5 if bn == 160 else 2, gn) and g.n_pieces >= 8) else None


def plan_tiles3p(d, g, cus):
    """gemm.hip plan_tiles3p (cu_share 1)"""
    bn = 160 if (d.N % 160 == 0 and d.N % 128 != 0) else 128
    tiles_m = g.img_groups * g.tiles_y * g.tiles_x
    tiles_n = (d.N + bn - 1) // bn
    tiles = tiles_m * tiles_n
    nkt = g.chunks
    total = tiles * nkt
    whole = nkt * 9 < 24                                                 # ``const bool whole = t.nkt * 9 < 24 || prefer_whole_tiles(d, t.tiles)``
    G = min(total, 2 * cus // 2)
    ipw = (total + G - 1) // G
    if whole:
        ipw = ((ipw + nkt - 1) // nkt) * nkt
    return SimpleNamespace(bm=256, bn=bn, tiles_m=tiles_m, tiles_n=tiles_n, tiles=tiles, nkt=nkt, total=total, ipw=ipw,
                           G=round_workgroups((total + ipw - 1) // ipw), fixup=ipw % nkt != 0)


def conv_n4_applies(d):
    """gemm.hip conv_n4_applies (pointers here are 16-byte aligned; knob ``conv_n4``: -1 / 1 on, 0 off)"""
    if d.knobs["conv_n4"] == 0:
        return False
    if d.flags != (F_CONV | F_F32) or d.ksize != 3 or d.stride != 1 or d.pad_t != 1 or d.pad_l != 1 or d.upsample:
        return False
    if d.N != 4 or d.C2 != 0 or d.C1 % 64 or d.C1 > 512 or d.Hout != d.Hin or d.Wout != d.Win or d.ldo % 4:
        return False
    if d.residual or d.rowvec or d.in_scsh or d.colstats or d.batch > 1 or d.alpha != 1.0:
        return False
    return d.K == 9 * d.C1 and d.lda in (0, d.C1) and d.in_act == 0


def lean_plan(d, cus, want_stats):
    """gemm.hip lean_plan, bf16 only (no MX8 operands, no emitting epilogue) -> plan or None"""
    mode = d.knobs["lean"]
    mode = -2 if mode < 0 else mode                                      # udt_debug_set("lean", v): ``g_lean.store(value < 0 ? -2 : value)``
    if mode == 0:
        return None
    if d.flags & (F_F32 | F_RELU | F_TRANS | F_SILU):                    # ``constexpr int unsupported = ...``
        return None
    conv1 = bool(d.flags & F_CONV)
    geglu = bool(d.flags & F_GEGLU)
    if conv1 and (d.ksize != 1 or d.stride != 1 or d.upsample or d.pad_t or d.pad_l or d.Hout != d.Hin or d.Wout != d.Win or
                  d.C1 % BK or d.C2 % BK or d.ln or geglu):
        return None
    if d.batch > 1 or d.in_scsh:
        return None
    ln = d.ln
    if want_stats and (geglu or ln):
        return None
    if d.N <= 64 or d.N % 8 or d.K % BK or (not conv1 and d.lda % 8) or d.ldo % 8:
        return None
    if d.residual and d.ldr % 8:
        return None
    if geglu and (d.N % 64 or d.residual or d.rowvec):
        return None
    if d.rowvec and (d.ld_rowvec if d.ld_rowvec > 0 else d.N) % 4:
        return None
    if mode > 0 and mode not in (1, 6, 7):
        return None
    t = SimpleNamespace(stats_rows=0)
    rowres_on = d.knobs["rowres"] != 0
    if mode == 7 or (mode < 0 and rowres_on):
        if ln and not want_stats and d.K == 320 and d.N % 64 == 0 and not d.residual and not d.rowvec and not conv1:
            tiles_m, chunks = (d.M + 255) // 256, d.N // 64
            ns = (cus + tiles_m - 1) // tiles_m                          # ``int ns = (device_cus() + tiles_m - 1) / tiles_m;``
            ns = min(ns, chunks // 4)
            cmax = 20 if geglu else 16
            ns = max(ns, (chunks + cmax - 1) // cmax)
            wgs = tiles_m * ns
            if ns >= 1 and (mode == 7 or (wgs * 4 >= 3 * cus if geglu else wgs >= cus)):
                t.cfg, t.bm, t.bn, t.tiles_m = 7, 256, 64, tiles_m
                t.kt_per = (chunks + ns - 1) // ns
                t.tiles_n = (chunks + t.kt_per - 1) // t.kt_per
                t.tiles, t.nkt, t.splitk, t.n_block = t.tiles_m * t.tiles_n, d.K // BK, 1, 1
                t.G = round_workgroups(t.tiles)
                return t
        if mode == 7:
            return None
    t.cfg = mode if mode > 0 else 1
    if not geglu and d.N % 160 == 0 and d.N % 128 != 0 and t.cfg == 1:
        t.cfg = 5
    if mode <= 0 and d.N >= 768 and ((d.M + 255) // 256) * ((d.N + 255) // 256) >= 2 * cus:
        t.cfg = 6
    if want_stats:
        if t.cfg not in (1, 5):
            if mode > 0:
                return None
            t.cfg = 5 if (d.N % 160 == 0 and d.N % 128 != 0) else 1
        t.stats_rows = 64 if t.cfg == 1 else 32
        rpb = d.rows_per_batch if d.rows_per_batch > 0 else d.M
        if rpb % t.stats_rows:
            return None
    t.bm, t.bn = {1: (128, 128), 5: (128, 160), 6: (256, 256)}[t.cfg]
    t.tiles_m, t.tiles_n = (d.M + t.bm - 1) // t.bm, (d.N + t.bn - 1) // t.bn
    t.tiles = t.tiles_m * t.tiles_n
    t.nkt = d.K // BK
    slots = max(cus * (2 if t.cfg in (1, 5) else 1), 1)
    sk, knob = 1, d.knobs["lean_splitk"]
    if not ln and t.tiles <= 1023:
        if knob > 1:
            sk = knob
        elif knob < 0 and t.tiles * 2 <= slots and t.nkt >= 40:           # ``else if (knob < 0 && t.tiles * 2 <= slots && t.nkt >= (mx8 ? 20 : 40))``
            sk = min(slots // t.tiles, t.nkt // 16)
        sk = min(sk, t.nkt // 4)                                         # ``if (sk > t.nkt / 4) sk = t.nkt / 4;``
        while sk > 1 and t.tiles * sk * t.bm * t.bn * 4 > (64 << 20):
            sk -= 1
        sk = max(sk, 1)
    t.kt_per = (t.nkt + sk - 1) // sk
    t.splitk = (t.nkt + t.kt_per - 1) // t.kt_per
    t.G = round_workgroups(t.tiles * t.splitk)
    nb = d.knobs["n_block"]
    if nb <= 0:
        nb = t.tiles_n if t.tiles_m <= 8 else 8
    t.n_block = min(nb, t.tiles_n)
    return t


def conv_chunk_slices(tiles, slots, chunks, knob):
    """gemm.hip conv_chunk_slices"""
    sk = 1
    if tiles <= 1023:
        if knob > 1:
            sk = min(knob, chunks)
        elif knob < 0 and tiles * 2 <= slots and chunks >= 10:
            sk = min(slots // tiles, chunks // 4)
        sk = max(sk, 1)
    return sk


def lean_conv_plan(d, cus, want_stats):
    """gemm.hip lean_conv_plan (cu_share 1) -> plan or None"""
    if d.knobs["lean_conv"] == 0 or d.knobs["lean"] == 0:                 # ``if (!on || lean_mode() == 0) return false;``
        return None
    if d.flags != F_CONV or d.ksize != 3 or d.stride != 1 or d.pad_t != 1 or d.pad_l != 1:
        return None
    if d.C2 != 0 or d.in_scsh or d.batch > 1:
        return None
    if d.N < 128 or d.N % 8 or d.C1 <= 0 or d.C1 % 64:
        return None
    phase, ups = d.upsample == 2, d.upsample == 1
    nph = 4 if phase else 1
    sh = 1 if d.upsample else 0
    if d.Hout != d.Hin << sh or d.Wout != d.Win << sh:
        return None
    Ht, Wt = (d.Hin, d.Win) if phase else (d.Hout, d.Wout)
    c = SimpleNamespace(bn=128, wgm=2)
    wide, wide_slots = False, cus
    wm = d.knobs["wide_conv"]
    knob = d.knobs["lean_splitk"]
    if wm != 0 and not ups and d.N % 160 == 0 and Wt % 16 == 0 and Ht % 16 == 0:
        wt = (d.M // 256) * (d.N // 160)
        sk = conv_chunk_slices(wt, wide_slots, d.C1 // 64, knob)
        units = wt * sk
        rounds = (units + cus - 1) // cus
        eff = units / (rounds * cus) if units > cus else (1.0 if units >= cus else units / cus)
        wide = wm > 0 or (sk <= 2 and eff >= 0.85)                       # ``wide = (wm > 0) || (sk <= 2 && eff >= ...0.85)``
    if wide:
        c.geo, c.tw, c.th, c.bn, c.wgm = (6 if phase else 3), 16, 16, 160, 4
    elif Wt % 16 == 0 and Ht % 8 == 0:
        c.geo, c.tw, c.th = (2 if ups else 4 if phase else 0), 16, 8
    elif not ups and Wt % 8 == 0 and Ht % 8 == 0:
        c.geo, c.tw, c.th = (5 if phase else 1), 8, 8
    else:
        return None
    if d.ldo % 8 or (d.residual and d.ldr % 8):
        return None
    c.nph = nph
    c.B = d.M // (d.Hout * d.Wout)
    c.tiles_x, c.tiles_y = Wt // c.tw, Ht // c.th
    c.tiles_m = c.B * c.tiles_x * c.tiles_y
    c.tiles_n = (d.N + c.bn - 1) // c.bn
    c.tiles = c.tiles_m * c.tiles_n
    c.chunks = d.C1 // 64
    slots = wide_slots if wide else 2 * cus
    sk = conv_chunk_slices(c.tiles * nph, slots, c.chunks, knob)
    while sk > 1 and c.tiles * nph * sk * c.tw * c.th * c.bn * 4 > (64 << 20):
        sk -= 1
    c.ch_per = (c.chunks + sk - 1) // sk
    c.splitk = (c.chunks + c.ch_per - 1) // c.ch_per
    c.G = round_workgroups(c.tiles * nph * c.splitk)
    patch = float(((c.tw // 2 if ups else c.tw) + 2) * ((c.th // 2 if ups else c.th) + 2)) * d.C1 * 2.0
    wtile = (4.0 if phase else 9.0) * c.bn * d.C1 * 2.0
    nb = d.knobs["n_block"]
    if nb <= 0:
        nb = int(math.sqrt(64.0 * patch / wtile) + 0.5)                   # ``nb = (int)(std::sqrt(64.0 * patch / wtile) + 0.5);``
    c.n_block = min(max(nb, 1), c.tiles_n)
    return c


def colstats_plan(d, cus):
    """gemm.hip colstats_rows / colstats_slots / lean_stats_probe -> (rows per slot, slots, layout) or None"""
    if d.flags & (F_F32 | F_GEGLU | F_TRANS) or d.batch > 1:
        return None
    rpb = d.rows_per_batch if d.rows_per_batch > 0 else d.M
    if not d.in_scsh:
        c3 = lean_conv_plan(d, cus, True)
        if c3:
            return c3.tw * c3.th // c3.wgm, c3.tiles_m * c3.wgm * c3.nph, ("conv", c3.tw, c3.th, 1, c3.wgm, c3.nph)
        if not (d.flags & F_CONV and d.ksize == 3):
            lt = lean_plan(d, cus, True)
            if lt:
                return lt.stats_rows, lt.tiles_m * (lt.bm // lt.stats_rows), ("rows",)
    g = conv3p_geometry(d, d.in_scsh)
    if g:
        rows = 32 if (d.N % 160 == 0 and d.N % 128 != 0) else 64
        if (g.TW * g.TH) % rows or rpb % rows:
            return None
        return rows, g.img_groups * g.tiles_y * g.tiles_x * (256 // rows), ("conv", g.TW, g.TH, g.NI, 256 // rows, 1)
    if use_gemm8(d) and d.knobs["rows_epi"]:
        rows = 32 if plan_tiles8(d, cus).bn == 160 else 64
        return (rows, ((d.M + 255) // 256) * (256 // rows), ("rows",)) if rpb % rows == 0 else None
    return None


def predict(c, cus):
    """udt_gemm's dispatch order -> SimpleNamespace(family, tag, tile = (kind, ...) for the slices, plan, stats)"""
    d = describe(c)
    p = SimpleNamespace(d=d, stats=colstats_plan(d, cus) if d.colstats else None)
    conv = bool(d.flags & F_CONV)
    if conv_n4_applies(d):
        p.family, p.plan = "conv_n4", None
        p.tag = f"conv_n4 M={d.M} N={d.N} K={d.K} {d.Hin}x{d.Win}"
        p.tile = ("conv", 8, 8, 4, 1)
        return p
    lt = lean_plan(d, cus, d.colstats)
    if lt:
        p.family, p.plan = f"lean{lt.cfg}", lt
        p.tag = (f"lean{lt.cfg} M={d.M} N={d.N} K={d.K} fl=0x{d.flags:x} ln={int(d.ln)} tile={lt.bm}x{lt.bn} units={lt.tiles * lt.splitk} "
                 f"splitk={lt.splitk}")
        half = 2 if d.flags & F_GEGLU else 1                              # (GEGLU: the output has N / 2 columns)
        wr, wc = {1: (64, 64), 5: (32, 160), 6: (128, 64), 7: (256, 64 * lt.kt_per)}[lt.cfg]
        p.tile = ("rows", lt.bm, (64 * lt.kt_per if lt.cfg == 7 else lt.bn) // half, wr, wc // half)
        return p
    assert not d.ln, "the LayerNorm-folded form exists on the lean kernels only"
    c3 = lean_conv_plan(d, cus, d.colstats)
    if c3:
        wide = c3.geo in (3, 6)
        p.family, p.plan = f"{'wconv3' if wide else 'lconv3'}:{c3.geo}", c3
        p.tag = (f"{'wconv3' if wide else 'lconv3'}{'+up' if (d.upsample and c3.geo != 6) else ''} M={d.M} N={d.N} K={d.K} {d.Hin}x{d.Win} "
                 f"tile={c3.tw}x{c3.th} units={c3.tiles * c3.nph * c3.splitk} splitk={c3.splitk} nb={c3.n_block}{' up4' if d.upsample == 2 else ''}")
        p.tile = ("conv", c3.th, c3.tw, c3.bn, 2 if c3.nph == 4 else 1)
        return p
    g = conv3p_geometry(d, d.in_scsh)
    if g:
        t3 = plan_tiles3p(d, g, cus)
        p.family, p.plan, p.geo = "conv3p", t3, g
        p.tag = (f"conv3p+gn M={d.M} N={d.N} K={d.K} {d.Hin}x{d.Win} tile={g.TW}x{g.TH}x{g.NI} bn={t3.bn} G={t3.G} ipw={t3.ipw}")
        p.tile = ("conv", g.TH, g.TW, t3.bn, 1)
        return p
    assert not d.in_scsh
    if use_gemm8(d):
        t8 = plan_tiles8(d, cus)
        p.family, p.plan = "gemm8", t8
        p.tag = (f"gemm8 M={d.M} N={d.N} K={d.K} conv={int(conv)} ks={d.ksize} fl=0x{d.flags:x} tile={t8.bm}x{t8.bn} G={t8.G} ipw={t8.ipw} "
                 f"b={d.batch}")
        half = 2 if d.flags & F_GEGLU else 1
        wr, wc = (32, 160) if t8.bn == 160 else (64, 64)
        p.tile = ("rows", t8.bm, t8.bn // half, wr, wc // half)
        return p
    t = plan_tiles(d, cus)
    assert t.bm == 256, "the first-generation kernel survives on 256 x 64 tiles only"
    p.family, p.plan = "gemm", t
    p.tag = (f"gemm M={d.M} N={d.N} K={d.K} conv={int(conv)} ks={d.ksize} fl=0x{d.flags:x} tile={t.bm}x{t.bn} G={t.G} ipw={t.ipw} b={d.batch}")
    p.tile = ("rows", 256, 64, 64, 64)
    return p


# ================================================================================================ the case lists
def G(M, N, K, **kw):
    return dict(kind="gemm", M=M, N=N, K=K, **kw)


def C(B, H, W, C1, N, **kw):
    return dict(kind="conv", B=B, H=H, W=W, C1=C1, N=N, **kw)


def _name(c):
    skip = ("kind",)
    return " ".join(f"{k}={v}" for k, v in c.items() if k not in skip).replace("'", "").replace(" ", "_").replace(",_", ",")


_LEAN_M, _LEAN_N, _LEAN_N5 = (8, 120, 129, 257), (72, 136, 200, 328), (160, 480)
LEAN_GEMM = (
    # configuration 1: every M against every N, K alternating between one and three K-tiles
    [G(M, N, (64, 192)[(i + j) % 2], res=bool((i + j) % 3 == 0)) for i, M in enumerate(_LEAN_M) for j, N in enumerate(_LEAN_N)] +
    # configuration 5 (N % 160 == 0 and N % 128 != 0)
    [G(M, N, (192, 64)[(i + j) % 2], res=bool(j)) for i, M in enumerate(_LEAN_M) for j, N in enumerate(_LEAN_N5)] +
    # forced configuration 6 (256 x 256, eight waves)
    [G(M, N, 192, knobs={"lean": 6}, res=True) for M, N in ((120, 136), (257, 328), (129, 72), (257, 480))] +
    # forced split-K with ragged last slices: 9 K-tiles in 5 + 4, 13 in 5 + 5 + 3
    [G(129, 136, 576, knobs={"lean_splitk": 2}, res=True), G(257, 200, 832, knobs={"lean_splitk": 3}),
     G(120, 160, 576, knobs={"lean_splitk": 2}), G(129, 480, 832, knobs={"lean_splitk": 3}, res=True),
     G(257, 328, 832, knobs={"lean": 6, "lean_splitk": 3}, res=True)] +
    # the automatic split-K rule (>= 40 K-tiles, tiles that leave the chip idle): 40 K-tiles in 20 + 20
    [G(129, 136, 2560, res=True)] +
    # operands and outputs as column ranges of wider buffers, alpha, row vectors whose period divides neither a wave block nor a tile
    [G(129, 136, 192, ld_extra=(64, 24, 40), res=True, alpha=0.75), G(257, 160, 64, ld_extra=(8, 8, 16), res=True, alpha=-1.5),
     G(257, 200, 192, rowvec=24, res=True), G(257, 160, 64, rowvec=100), G(300, 328, 64, rowvec=100, knobs={"lean": 6}, alpha=0.5)] +
    # GEGLU
    [G(129, 128, 192, geglu=True), G(257, 192, 64, geglu=True, alpha=0.5), G(120, 192, 192, geglu=True, knobs={"lean": 6})] +
    # LayerNorm-folded, plain and GEGLU (rows with a large mean and constant rows: inputs ``ln``)
    [G(129, 136, 192, ln=True), G(257, 160, 64, ln=True), G(120, 192, 192, ln=True, geglu=True), G(257, 328, 192, ln=True, knobs={"lean": 6})] +
    # the row-resident configuration 7 (K = 320), forced: one and several column splits
    [G(M, N, 320, ln=True, geglu=g, knobs={"lean": 7}) for M, N, g in ((8, 256, False), (255, 512, False), (257, 1024, False), (257, 512, True),
                                                                       (8, 1024, True))] +
    # statistics epilogue with ragged M (slots past M must be exactly zero)
    [G(192, 136, 192, stats=64, res=True), G(320, 200, 64, stats=64, rowvec=64), G(160, 160, 192, stats=32), G(288, 480, 64, stats=96, res=True)]
)
LEAN_CONV1 = [
    C(2, 8, 9, 192, 136, ksize=1, C2=64, res=True), C(3, 8, 8, 64, 160, ksize=1),
    # forced split-K (9 K-tiles in 5 + 4) whose boundary does not coincide with the source boundary (6 K-tiles | 3)
    C(2, 9, 8, 384, 136, ksize=1, C2=192, knobs={"lean_splitk": 2}, rowvec=True),
    C(3, 8, 16, 192, 200, ksize=1, C2=64, stats=True),
]
GEMM8 = [dict(c, knobs=dict(c.get("knobs", {}), lean=0)) for c in (
    # both tile widths, M on both sides of 256, whole tiles
    [G(M, N, K) for M, N, K in ((130, 136, 64), (255, 200, 192), (257, 136, 192), (300, 328, 64), (130, 160, 192), (257, 320, 64), (300, 480, 192))] +
    # stream-K whose ranges straddle a tile boundary (2 tiles x 26 K-tiles in ranges of 4; 160-wide: 2 x 26 as well)
    [G(130, 136, 1664, res=True), G(257, 160, 1664), G(300, 200, 1600, rowvec=100)] +
    # ReLU, SiLU, fp32 output
    [G(257, 136, 192, act="relu"), G(130, 160, 64, act="silu"), G(257, 200, 192, f32=True), G(130, 320, 192, f32=True, act="relu"), G(257, 136, 64, f32=True, act="silu"),
     G(130, 136, 1664, act="silu", res=True)] +
    # transposed output, batched with strides, GEGLU
    [G(144, 136, 192, trans=36, bias=True), G(288, 72, 1664, trans=36), G(130, 136, 192, batch=3, ld_extra=(64, 24, 0), bias=False),
     G(257, 72, 64, batch=3, bias=False, alpha=0.125), G(257, 192, 192, geglu=True)] +
    # tile order forced ragged (3 N-tiles in blocks of 2), both epilogue forms
    [G(600, 328, 64, knobs={"n_block": 2}), G(257, 480, 192, knobs={"n_block": 2}, res=True), G(257, 200, 192, knobs={"rows_epi": 0}, res=True),
     G(130, 160, 64, knobs={"rows_epi": 0}, rowvec=24), G(257, 136, 1664, knobs={"rows_epi": 0}, ld_extra=(8, 8, 8), res=True)] +
    # statistics forms
    [G(320, 136, 192, stats=64), G(288, 160, 64, stats=96, res=True), G(192, 200, 1664, stats=64)] +
    # gathered convolutions
    [C(2, 9, 9, 64, 136, stride=2), C(2, 10, 6, 64, 128, stride=2, pad=(0, 0), out_hw=(5, 3)), C(1, 4, 4, 64, 320, ups=1),
     C(2, 12, 20, 64, 136, res=True), C(3, 8, 8, 64, 160, C2=128, rowvec=True), C(1, 16, 20, 128, 200, stats=True),
     C(2, 9, 9, 192, 128, stride=2, act="silu"), C(1, 16, 16, 64, 72, ksize=1, f32=True)]
)]
GEN1 = (
    [G(M, N, K, res=(N == 64), rowvec=(100 if N == 12 else 0)) for M, N, K in ((130, 4, 128), (257, 12, 128), (1000, 64, 128), (257, 4, 1024),
                                                                                (1000, 12, 1024), (130, 64, 1024))] +
    [G(257, 64, 128, f32=True), G(130, 12, 1024, act="relu")] +
    # the 3x3 convolution to 4 channels with bf16 output (conv_n4 declines it), without and with the fix-up pass
    [C(3, 13, 9, 64, 4), C(2, 8, 8, 128, 4), C(1, 24, 40, 64, 4, f32=True, knobs={"conv_n4": 0})]
)
CONV_N4 = [C(3, H, W, Cc, 4, f32=True) for (H, W), Cc in (((13, 9), 64), ((8, 8), 512), ((24, 40), 64), ((13, 9), 512), ((8, 8), 64))]
LCONV = (
    # geometry 0 (16 x 8 tiles) and 1 (8 x 8): maps 8 x 8 (every pixel on the border), 16 x 8, 8 x 16, 16 x 24
    [C(3, 8, 8, 64, 128), C(1, 8, 16, 192, 136, res=True), C(3, 16, 8, 64, 320, rowvec=True), C(1, 24, 16, 64, 136, res=True, rowvec=True),
     C(1, 16, 8, 320, 128), C(3, 8, 16, 64, 136, stats=True), C(1, 8, 8, 192, 320, stats=True, res=True), C(3, 8, 8, 64, 160, alpha=0.5)] +
    # geometry 2: nearest x2 upsample, nine taps on the upsampled map
    [C(3, 4, 8, 64, 128, ups=1), C(1, 8, 8, 192, 136, ups=1, rowvec=True), C(1, 4, 8, 64, 320, ups=1, stats=True)] +
    # geometries 4 and 5: the phase form
    [C(3, 8, 16, 64, 128, ups=2), C(1, 8, 8, 192, 136, ups=2), C(3, 8, 8, 64, 320, ups=2, rowvec=True), C(1, 16, 16, 64, 136, ups=2, stats=True),
     C(1, 8, 8, 64, 128, ups=2, stats=True, res=True)] +
    # forced chunk slices with a short last slice: five chunks in 2 + 2 + 1 and 3 + 2
    [C(1, 8, 16, 320, 136, knobs={"lean_splitk": 3}, res=True), C(3, 8, 8, 320, 128, knobs={"lean_splitk": 2}, rowvec=True),
     C(1, 8, 8, 320, 136, ups=2, knobs={"lean_splitk": 3}), C(1, 4, 8, 320, 128, ups=1, knobs={"lean_splitk": 3}, stats=True)] +
    # the automatic chunk-slice rule (>= 10 chunks): 10 chunks in 5 + 5
    [C(1, 8, 8, 640, 128, res=True)] +
    # the wide kernel, forced: geometries 3 and 6
    [C(1, 16, 16, 64, 160, knobs={"wide_conv": 1}), C(3, 16, 16, 192, 320, knobs={"wide_conv": 1}, res=True, rowvec=True),
     C(1, 16, 32, 320, 160, knobs={"wide_conv": 1, "lean_splitk": 3}, stats=True), C(1, 16, 16, 64, 160, ups=2, knobs={"wide_conv": 1}),
     C(3, 16, 16, 64, 320, ups=2, knobs={"wide_conv": 1}, stats=True, res=True),
     C(1, 16, 16, 192, 160, ups=2, knobs={"wide_conv": 1, "lean_splitk": 2}, rowvec=True)]
)
CONV3P = [
    # tilings 32 x 8, 16 x 16 and 4 x (8 x 8) with ragged image groups; tile widths 128 and 160; one and two sources; in_act 0 and 1;
    # whole tiles (<= 2 chunks) and stream-K cuts between chunks; statistics
    C(1, 8, 32, 64, 128, gn=1), C(3, 8, 32, 128, 160, gn=0), C(1, 16, 16, 64, 136, gn=1, C2=64, res=True), C(3, 16, 16, 192, 160, gn=1, rowvec=True),
    C(1, 8, 8, 128, 128, gn=1), C(3, 8, 8, 64, 200, gn=0, C2=128), C(5, 8, 8, 192, 136, gn=1, stats=True), C(1, 16, 32, 64, 320, gn=1, C2=128, stats=True),
    C(5, 8, 8, 64, 128, gn=0, stats=True, res=True), C(1, 16, 16, 128, 320, gn=0, stats=True),
]
FAMILIES = {"lean": LEAN_GEMM, "lean_conv1": LEAN_CONV1, "gemm8": GEMM8, "gen1": GEN1, "conv_n4": CONV_N4, "lconv": LCONV, "conv3p": CONV3P}
CONV_VARIANTS = ("border_only", "image_steps")
GEMM_VARIANTS = ("cancel", "big_bias")
# one case per route for the value variants (indices into the lists above)
GEMM_VARIANT_CASES = [G(129, 136, 192, res=True), G(257, 160, 192, res=True), G(257, 328, 192, res=True, knobs={"lean": 6}),
                      G(257, 136, 1664, res=True, knobs={"lean": 0}), G(257, 160, 192, res=True, knobs={"lean": 0}), G(257, 64, 1024, res=True)]
CONV_VARIANT_CASES = [C(3, 8, 16, 64, 136), C(3, 8, 8, 64, 128), C(3, 4, 8, 64, 128, ups=1), C(3, 8, 16, 64, 128, ups=2), C(3, 8, 8, 64, 136, ups=2),
                      C(3, 16, 16, 64, 160, knobs={"wide_conv": 1}), C(3, 16, 16, 64, 160, ups=2, knobs={"wide_conv": 1}),
                      C(3, 8, 8, 64, 128, gn=1), C(3, 16, 16, 64, 160, gn=0), C(3, 8, 32, 64, 128, gn=1, C2=64),
                      C(3, 9, 9, 64, 136, stride=2, knobs={"lean": 0}), C(3, 12, 20, 64, 136, knobs={"lean": 0}), C(3, 8, 8, 64, 72, ksize=1, C2=64),
                      C(3, 13, 9, 64, 4), C(3, 13, 9, 64, 4, f32=True)]


def all_cases():
    """[(name, case, variant)] — every list with randn values, the variant cases with their hostile values"""
    out = []
    for fam, lst in FAMILIES.items():
        out += [(f"{fam}: {_name(c)}", c, "randn") for c in lst]
    out += [(f"variant {v}: {_name(c)}", c, v) for c in GEMM_VARIANT_CASES for v in GEMM_VARIANTS]
    out += [(f"variant {v}: {_name(c)}", c, v) for c in CONV_VARIANT_CASES for v in CONV_VARIANTS]
    return out


# ================================================================================================ inputs
def _gen(name):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(name.encode()) & 0x7fffffff)
    return g


def inputs(c, variant="randn"):
    """-> dict of CPU float32 tensors (bf16 values where the kernel reads bf16).  Weights are row- and tap-asymmetric (a swapped row
    or tap changes the result); ``ln``: rows 1, 5 carry a large mean, rows 2, 6 are constant."""
    d = describe(c)
    g = _gen(_name(c) + variant)
    rn = lambda *s: torch.randn(*s, generator=g)
    t = {}
    N, K = d.N, d.K
    n_cols = N // 2 if c.get("geglu") else N
    if c["kind"] == "gemm":
        bsh = (d.batch,) if d.batch > 1 else ()
        a = rn(*bsh, d.M, K)
        if c.get("ln"):
            a[1::8] += 8.0
            a[5::8] -= 6.0
            a[2::4] = 2.0
        t["a"] = _bf(a)
        w = rn(*bsh, N, K) / math.sqrt(K)
        w = w * (1.0 + 0.5 * torch.arange(N).reshape(N, 1) / N) * (1.0 + 0.25 * torch.arange(K).reshape(1, K) / K)
        t["w"] = _bf(w)
        M_all = d.M
    else:
        B, H, W = c["B"], c["H"], c["W"]
        Ct = d.C1 + d.C2
        x = rn(B, H, W, Ct)
        if variant == "border_only":
            x[:, 1:H - 1, 1:W - 1] = 0.0
        elif variant == "image_steps":
            x = x + 3.0 * (1.0 + torch.arange(B, dtype=torch.float32)).reshape(B, 1, 1, 1)
        t["x"] = _bf(x[..., :d.C1]).contiguous()
        if d.C2:
            t["x2"] = _bf(x[..., d.C1:]).contiguous()
        if d.upsample == 2:
            w = rn(4, N, 4 * d.C1) / math.sqrt(4 * d.C1)
            w = w * (1.0 + 0.25 * torch.arange(4).reshape(4, 1, 1)) * (1.0 + 0.5 * torch.arange(N).reshape(1, N, 1) / N) * \
                (1.0 + 0.3 * (torch.arange(4 * d.C1) // d.C1)).reshape(1, 1, -1)
        else:
            w = rn(N, K) / math.sqrt(K)
            w = w * (1.0 + 0.5 * torch.arange(N).reshape(N, 1) / N) * (1.0 + 0.3 * (torch.arange(K) // Ct)).reshape(1, K)
        t["w"] = _bf(w)
        if d.in_scsh:
            sc = 0.5 + torch.rand(B, Ct // 64, 1, 64, generator=g)
            shf = 0.75 * rn(B, Ct // 64, 1, 64) + 0.5                 # beta != 0: a padding pixel that received the shift shows
            t["scsh"] = torch.cat([sc, shf], dim=2).contiguous()
        M_all = d.M
    if d.bias:
        t["bias"] = rn(N) * (100.0 if variant == "big_bias" else 1.0)
    if d.ln:
        t["bias"] = rn(N)                                              # the folded c vector
        t["s"] = (t["w"].double().sum(dim=1)).float()                  # the folded weights' column sums, fp32 as given
    if d.rowvec:
        rpb = d.rows_per_batch
        t["rowvec"] = rn((M_all + rpb - 1) // rpb, N)
    if d.residual:
        if variant == "cancel":
            acc = (t["a"].double() @ t["w"].double().transpose(-1, -2)) * d.alpha
            t["res"] = _bf(-acc.float())
        else:
            t["res"] = _bf(rn(*((d.batch,) if d.batch > 1 else ()), M_all, n_cols))
        if c["kind"] == "conv":
            t["res"] = t["res"].reshape(c["B"], d.Hout, d.Wout, n_cols)
    return t


# ================================================================================================ references
def reference(c, t, dev="cpu", acc_hook=None):
    """-> (ref, emul, abs_terms, extra) in R's working precision; ``extra`` (or None) is an additional per-element floor (the measured
    erf error of the GEGLU forms).  acc_hook(acc) -> acc: the planted defects of the CPU test rewrite the products before the epilogue."""
    d = describe(c)
    on = lambda k: t[k].to(dev) if k in t else None
    if d.ln:                                          # (no planted defect sits in the LayerNorm-folded form)
        out = R.ln_gemm_ref(on("a"), on("w"), on("bias"), on("s"), alpha=d.alpha, geglu=bool(c.get("geglu")))
    elif c["kind"] == "gemm":
        out = R.gemm_ref(on("a"), on("w"), alpha=d.alpha, bias=on("bias"), rowvec=on("rowvec"), rows_per_batch=d.rows_per_batch,
                         residual=on("res"), act=c.get("act"), out_f32=bool(c.get("f32")), geglu=bool(c.get("geglu")),
                         transposed=bool(c.get("trans")), acc_hook=acc_hook)
    else:
        out = R.conv_ref(on("x"), on("w"), ksize=d.ksize, stride=d.stride, pad_t=d.pad_t, pad_l=d.pad_l, upsample=d.upsample,
                         out_hw=(d.Hout, d.Wout), x2=on("x2"), in_scsh=on("scsh"), in_act=d.in_act, alpha=d.alpha, bias=on("bias"),
                         rowvec=on("rowvec"), residual=on("res"), act=c.get("act"), out_f32=bool(c.get("f32")), acc_hook=acc_hook)
    return out if len(out) == 4 else out + (None,)


def eval32(c, t, acc_hook=None):
    """the float32 CPU restatement: the same op with float32 products / accumulation / epilogue and the same single roundings — what a
    correct fp32-accumulating implementation stores (the ``emul`` of the float32 evaluation)"""
    with R.restated_in(torch.float32):
        return reference(c, t, "cpu", acc_hook)[1]


# ================================================================================================ column statistics
def stats_slot_of_row(c, p):
    """slot of every output row (pixel) in the kernel's slot order, from predict()'s stats layout: GEMMs — row // rows; convolutions —
    [image (group)][phase][tile of the image][wave pixel block], a block = ``rows`` consecutive pixels of the tile in (image of the group,
    y, x) order (lean.h:1047-1049, wide.h:417, conv3p.h:693-695)"""
    d = p.d
    rows, slots, lay = p.stats
    if lay[0] == "rows":
        return torch.arange(d.M) // rows, slots
    _, tw, th, ni, wgm, nph = lay
    B = c["B"]
    Ho, Wo = d.Hout, d.Wout
    st = 2 if nph == 4 else 1
    Ht, Wt = Ho // st, Wo // st
    tx_n, ty_n = Wt // tw, Ht // th
    b, y, x = torch.meshgrid(torch.arange(B), torch.arange(Ho), torch.arange(Wo), indexing="ij")
    phase = (y % st) * 2 + (x % st) if nph == 4 else torch.zeros_like(y)
    yl, xl = y // st, x // st
    rt = (yl // th) * tx_n + (xl // tw)
    ml = (b % ni) * (tw * th) + (yl % th) * tw + (xl % tw)
    per_img = tx_n * ty_n
    tile = ((b // ni) * nph + phase) * per_img + rt
    return (tile * wgm + ml // rows).reshape(-1), slots


# ================================================================================================ the shared checks
def slices_of(c, p):
    d = p.d
    if p.tile[0] == "rows":
        _, bm, bn, wr, wc = p.tile
        n_cols = d.N // 2 if c.get("geglu") else d.N
        if c.get("trans"):
            rpb = d.rows_per_batch
            return [(b, slice(c0, min(d.N, c0 + 64)), slice(None)) for b in range(d.M // rpb) for c0 in range(0, d.N, 64)]
        # (a gathered convolution: flat pixel rows in bm-row tiles)
        return list(S.gemm_tile_slices(d.M, n_cols, bm, bn, wr, wc, batch=d.batch if d.batch > 1 else None))
    _, th, tw, bn, step = p.tile
    return list(S.conv_tile_slices(c["B"], d.Hout, d.Wout, d.N, th, tw, bn, step))


def fp32_units(c, t, exp):
    """check_fp32_sum's units for an fp32-output case: 16, or twice the float32 CPU restatement's own worst ratio where that already
    exceeds 16 (deep K) — never read off the kernel.  -> (units, the restatement's measured ratio)"""
    ref, _, ab, _ = exp
    got = eval32(c, t).double()
    r, a = ref.double().cpu(), ab.double().cpu()
    ratio = float(((got - r).abs() / a.clamp_min(1e-300) * 2.0 ** 24)[a > 0].max())
    return (S.FP32_SUM_UNITS if ratio <= S.FP32_SUM_UNITS else 2.0 * ratio), ratio


def hold(name, c, p, got, exp, t=None, report=None):
    """the checks of one result (CPU restatement or kernel): tile slices; for convolutions also border ring against interior; fp32
    outputs element-wise.  ``got`` has the reference's shape."""
    ref, emul, ab, extra = exp
    d = p.d
    if c.get("f32"):
        # an activation after the sum passes the sum's error through its slope: ReLU <= 1, SiLU <= 1.0998 (units x 1.1)
        units, ratio = fp32_units(c, t, exp)
        S.check_fp32_sum(f"{name} [restated {ratio:.1f} units]", got, ref, ab, units=units * (1.1 if c.get("act") == "silu" else 1.0),
                         report=report)
        return
    floor = (emul - ref)
    if extra is not None:
        floor = floor.abs() + extra
    A = float(ab.double().pow(2).mean().sqrt())
    view = (lambda z: z.reshape(d.M, -1)) if (c["kind"] == "conv" and p.tile[0] == "rows") else (lambda z: z)
    S.check_sliced(name, view(got), view(ref), view(floor), slices_of(c, p), abs_scale=A, report=report)
    if c["kind"] == "conv":
        sh = (c["B"], d.Hout, d.Wout, d.N)
        S.check_sliced(name + " ring", got.reshape(sh), ref.reshape(sh), floor.reshape(sh), list(S.ring_slices(c["B"], d.Hout, d.Wout)),
                       abs_scale=A, report=report)


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
