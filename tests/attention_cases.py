"""Inputs, shape lists and the shared checks of the forward attention edge cases: tests/test_attention_ref_cpu.py (float32 CPU evaluation,
planted defects, coverage of the lists) and tests/test_attention_edges_gpu.py (the kernels) use the same ones.  A helper, not a test.
Every tensor is float32 holding bf16 values unless the kernel takes fp32.  Each shape list has a pure-Python mirror of its launcher's
rule; the lists are chosen as the smallest shapes that launch what no other kernel-level test does."""
import itertools
import math

import torch

import attention_ref as R
import sliced_check as S
from backward_cases import _bf, _gen, attn_inputs

LOG2E = R.LOG2E
MARKER = 123.0                                  # rows past the result are pre-filled with it and must come back untouched


# ------------------------------------------------------------------------------------------------ flash attention: values
FLASH_VARIANTS = ("spike", "flat", "neg", "grow", "late_spike")


def flash_inputs(B, H, nq, nk, variant="randn", head_dim=64, seed=0):
    """-> q [B, nq, C], k, v [B, nk, C] (C = H * head_dim).  randn / spike / flat / neg are backward_cases.attn_inputs at
    N = max(nq, nk) (neg: every real score about -30 (-85 at head_dim 512) after scaling — a padded key scored 0 would dominate);
    grow — logits rise slowly with the key index, by about 6 in the log2 domain over ALL keys (the deferred rescale of A2_DEFER = 8
    is never taken after the first tile, P reaches 2^6); late_spike — the key whose logit leads by more than 100 is the LAST one (in
    the last, partial key tile)."""
    Hh = H * head_dim // 64
    C = H * head_dim
    N = max(nq, nk)
    base = variant if variant in ("randn", "spike", "flat", "neg") else "randn"
    qkv, _ = attn_inputs(B, Hh, N, base, seed)
    q, k, v = qkv[:, :nq, :C].clone(), qkv[:, :nk, C:2 * C].clone(), qkv[:, :nk, 2 * C:].clone()
    u = 0.125
    if variant == "spike" and N // 3 >= nk:
        k[:, nk // 3] = qkv[:, N // 3, C:2 * C]                  # (the spike key fell outside the keys in use)
    elif variant == "late_spike":
        q = 0.5 * q + 8.0 * u
        k[:, nk - 1] = 160.0 * u
    elif variant == "grow":
        q = 0.5 * q + 8.0 * u                                   # q . (u, ..., u) = 8 head_dim / 64 +- 0.5 sqrt(head_dim) / 8
        G = 6.0 / (LOG2E * head_dim ** -0.5 * 8.0 * head_dim / 64)
        k = 0.05 * k + (torch.linspace(0.0, 1.0, nk) * G * u).reshape(1, nk, 1)
    return _bf(q), _bf(k), _bf(v)


# ------------------------------------------------------------------------------------------------ d64: shapes
D64_NQ = (31, 33, 127, 129)                                     # both sides of a wave's 32 and a workgroup's 128 queries
D64_NK = (8, 64, 72, 128, 136, 192, 200, 264, 328)              # 1 .. 5 (full | partial) key tiles of 64 + one more partial
D64_NK_ROWV = D64_NK + (4, 65, 129, 193)                        # row-major V takes any key count
_BH_ONE_QTILE = ((1, 1), (7, 1), (2, 4), (3, 3))                # units 1, 7, 8, 9
_BH_TWO_QTILES = ((2, 2), (1, 1), (1, 7), (3, 3))               # units 8, 2, 14, 18


def d64_launch(B, H, nq, nk):
    """attn_fwd_impl: ``p.qtiles = (nq + 127) / 128; p.units = p.qtiles * batch * heads; p.G = (p.units + 7) / 8 * 8`` (the 1-D grid of
    attn_d64_v2_kernel; range_index permutes it when G % 8 == 0, i.e. always), ``ntiles = (p.nk + KV_TILE - 1) / KV_TILE``"""
    qtiles = (nq + 127) // 128
    units = qtiles * B * H
    return {"qtiles": qtiles, "units": units, "G": (units + 7) // 8 * 8, "ntiles": (nk + 63) // 64, "partial": nk % 64 != 0,
            "ragged_wave": nq % 32 != 0, "dead_waves": (-nq) % 128 >= 32}


def _d64_shapes(nks):
    out = []
    for (ik, nk), (iq, nq) in itertools.product(enumerate(nks), enumerate(D64_NQ)):
        B, H = (_BH_TWO_QTILES if nq > 128 else _BH_ONE_QTILE)[(ik + iq) % 4]
        out.append((B, H, nq, nk))
    return out


D64_SHAPES = {"vt": _d64_shapes(D64_NK), "rowv": _d64_shapes(D64_NK_ROWV)}      # udt_attn_fwd (V^T operand, nk % 8 == 0) | udt_attn_rowv_fwd
D64_RULE = {"vt": "d64", "rowv": "v2"}                          # the kernel each entry launches (attention_ref.flash_fwd's ``kernel``)
D64_VARIANT_SHAPES = ((2, 2, 129, 200), (1, 7, 33, 328))        # ragged queries, a partial last key tile, 4 and 6 key tiles


# ------------------------------------------------------------------------------------------------ d512: shapes
def a5_key_split(batch, nq, nk):
    """csrc/attention.hip a5_key_split"""
    wgs = (nq + 63) // 64 * batch
    if wgs >= 192:
        return 1
    ntiles = (nk + 31) // 32
    best, best_cost = 1, 1.0
    ks = 2
    while ks <= 8 and ks * 8 <= ntiles:
        cost = ((wgs * ks + 255) // 256) / ks + 0.02 * ks
        if cost < best_cost - 1e-9:
            best_cost, best = cost, ks
        ks += 1
    return best


def attn512_plan(B, nq, nk, key_split):
    """attn512_impl: -> dict(q = 32 | 64 queries per workgroup, ksplit, kt_per, last = tiles of the last slice, ntiles).  With a
    workspace ``p.kt_per = (ntiles_all + ks - 1) / ks; p.ksplit = (ntiles_all + p.kt_per - 1) / p.kt_per``;
    ``const bool two = (long long)((nq + 63) / 64) * batch * p.ksplit >= 224``"""
    ntiles = (nk + 31) // 32
    ksplit, kt_per = 1, 0
    if key_split:
        ks = a5_key_split(B, nq, nk)
        if ks > 1:
            kt_per = (ntiles + ks - 1) // ks
            ksplit = (ntiles + kt_per - 1) // kt_per
            if ksplit < 2:
                ksplit = 1
    two = (nq + 63) // 64 * B * ksplit >= 224
    last = ntiles - (ksplit - 1) * kt_per if ksplit > 1 else ntiles
    return {"q": 64 if two else 32, "ksplit": ksplit, "kt_per": kt_per if ksplit > 1 else 0, "last": last, "ntiles": ntiles}


# (B, nq, nk, key_split): batch traded for sequence so that the tensors stay small
D512_SHAPES = [
    (112, 65, 33, False), (112, 95, 31, False), (112, 97, 32, False), (112, 127, 65, False),         # q64, whole
    (3, 33, 31, False), (3, 63, 64, False), (1, 95, 33, True),                                       # q32, whole
    (30, 97, 1057, True), (56, 65, 575, True), (30, 127, 1024, True), (30, 95, 1055, True),          # q64, split 4 | 2 | 4 | 4
    (1, 33, 545, True), (3, 31, 1023, True), (2, 33, 1056, True), (1, 63, 1823, True),               # q32, split 2 | 4 | 4 | 7
]
D512_VARIANT_SHAPES = ((112, 97, 33, False), (2, 33, 1057, True))
D512_SPLIT_VARIANT_SHAPE = (30, 97, 1057, True)                 # q64 with a short last slice: neg and late_spike only (size)


def d512_slices(B, nq):
    """[B, nq, 512]: (batch, 32-query tile, 128-column quarter) — one wave of attn_d512_body"""
    for b in range(B):
        for r0 in range(0, nq, 32):
            for c0 in range(0, 512, 128):
                yield (b, slice(r0, min(nq, r0 + 32)), slice(c0, c0 + 128))


def hold_flash(name, got, exp, B, H, nq, head_dim=64, report=None):
    """the check both test files make: exp = (ref64, floor_err, abs scale) of attention_ref.flash_ref_emul"""
    ref, floor, A = exp
    slices = S.attn_slices(B, H, nq, rows=32) if head_dim == 64 else d512_slices(B, nq)
    return S.check_sliced(name, got, ref, floor, slices, abs_scale=A, report=report)


# ------------------------------------------------------------------------------------------------ short-context attention
XATTN_L = (1, 2, 12, 13, 16)
XATTN_HEAD_DIM = (64, 128)
XATTN_NQ = (1, 255, 257)                                        # the workgroup takes 256 queries
XATTN_BH = (2, 2)
XATTN_PROBS_FACTOR = 8.0


def xattn_inputs(B, H, head_dim, nq, L, seed=0):
    """-> q [B, nq, C], kv [B, L, 2 C]"""
    g = _gen(B, H, head_dim, nq, L, seed)
    C = H * head_dim
    return _bf(torch.randn((B, nq, C), generator=g)), _bf(torch.randn((B, L, 2 * C), generator=g))


def hold_xattn_out(name, got, ref, B, H, head_dim, nq, report=None):
    return S.check_sliced(name, got, ref["out"], R.bf(ref["out"]) - ref["out"], S.attn_slices(B, H, nq, rows=32, head_dim=head_dim),
                          abs_scale=ref["abs"], report=report)


def hold_xattn_probs(name, got, ref, base, report=None):
    """fp32 probabilities (no sum of exact products): element-wise |got - ref64| <= 8 x base, base = attention_ref.xattn_probs_base"""
    err = float((S._f64(got) - S._f64(ref["probs"])).abs().max())
    k = XATTN_PROBS_FACTOR * base
    S._report(f"{name:55s} probs: max |err| {err:.3e}, float32 restatement {base:.3e}, bound {k:.3e}, ratio-to-bound "
              f"{err / k if k > 0 else float('inf'):.3f}{'  FAIL' if not err <= k else ''}", report)
    assert bool(torch.isfinite(S._f64(got)).all()) and err <= k, f"{name}: probs off by {err:.3e} > {k:.3e} (8 x {base:.3e})"
    return err / k


# ------------------------------------------------------------------------------------------------ masked small attention
MATTN_D_LK = ((8, 65), (32, 63), (32, 64), (32, 129), (32, 256), (64, 128))     # keys on both sides of the 64-lane rounds
MATTN_NQ = (1, 5, 6, 7)                                         # nq % 4 = 1, 1, 2, 3 (four waves, one query each per round)
MATTN_BH = (2, 2)


def mattn_guard_ok(D, lk):
    """udt_mattn_fwd's own guards"""
    return 0 < lk <= 256 and 0 < D <= 64 and D % 8 == 0 and lk * D <= 8192


def mattn_inputs(B, H, D, nq, lk, use_mask, use_kpm, special=None, seed=0):
    """-> q [B, nq, C], k, v [B, lk, C], mask fp32 [nq, lk] | None (finite values and -inf), kpm bool [B, lk] | None.  Key 1 is never
    masked, so no row is fully masked — except special="dead": row 0 is -inf everywhere in the mask; row 2 is -inf wherever sample 1's
    key padding leaves a key (fully masked by mask + kpm for sample 1 only).  special="huge": K and V are 1e30 (as bf16) at every
    key the mask rules out for all queries or the sample's key padding ignores."""
    g = _gen(B, H, D, nq, lk, int(use_mask), int(use_kpm), seed)
    C = H * D
    q, k, v = (torch.randn((B, n, C), generator=g) for n in (nq, lk, lk))
    mask = torch.randn((nq, lk), generator=g)
    mask[torch.rand((nq, lk), generator=g) < 0.2] = -math.inf
    kpm = torch.rand((B, lk), generator=g) < 0.3
    mask[:, 1] = 0.25
    kpm[:, 1] = False
    kpm[:, 0] = True
    mask[0, 0] = -math.inf                                      # -inf in the mask AND key padding on the same key
    if special == "dead":
        assert use_mask and use_kpm and nq >= 3 and B >= 2
        mask[0] = -math.inf
        mask[2] = torch.where(kpm[1], torch.zeros(lk), torch.full((lk,), -math.inf))
    if special == "huge":
        assert use_mask and use_kpm
        mask[:, lk // 2:lk // 2 + 3] = -math.inf
        gone = kpm | torch.isinf(mask).all(dim=0)[None, :]
        k[gone] = 1e30
        v[gone] = 1e30
    return _bf(q), _bf(k), _bf(v), (mask if use_mask else None), (kpm if use_kpm else None)


def hold_mattn(name, got, ref, scale_abs, B, H, D, nq, report=None):
    return S.check_sliced(name, got, ref, R.bf(ref) - ref, S.attn_slices(B, H, nq, rows=32, head_dim=D), abs_scale=scale_abs, report=report)


# ------------------------------------------------------------------------------------------------ row softmax
SOFTMAX_COLS = (8, 2040, 2048, 2056)                            # one 16-byte piece; 255, 256, 257 pieces for 256 threads
SOFTMAX_ROWS = 6
SOFTMAX_LD_EXTRA = 24                                           # ld > cols


def softmax_inputs(cols, seed=0):
    """-> x [6, cols]: row 1 holds equal values, row 2 one value that leads by 100"""
    g = _gen(cols, seed)
    x = 3.0 * torch.randn((SOFTMAX_ROWS, cols), generator=g)
    x[1] = 1.5
    x[2] = x[2].clamp(-3.0, 3.0)
    x[2, cols // 2] = 103.0
    return _bf(x)


def hold_softmax(name, got, ref, report=None):
    return S.check_sliced(name, got, ref, R.bf(ref) - ref, S.row_col_slices(ref.shape[0], ref.shape[1], 1, ref.shape[1]), report=report)


# ------------------------------------------------------------------------------------------------ fused text cross-attention
# (heads, B, n_tok, L, zero_samples): every width with 1, 2, 4 and 8 channel splits; every width with L = 1, 5, 12 and with
# zero_samples = 0, 1, B (B: the launch gets NULL tables)
TATTN_SHAPES = [
    (5, 4, 4096, 12, 1), (5, 2, 4096, 5, 0), (5, 2, 2048, 1, 2), (5, 3, 64, 5, 1),
    (10, 2, 4096, 5, 0), (10, 2, 2048, 12, 1), (10, 2, 1024, 1, 0), (10, 2, 32, 12, 2),
    (20, 2, 4096, 1, 1), (20, 1, 4096, 12, 0), (20, 2, 1024, 5, 2), (20, 3, 96, 5, 0),
]
TATTN_EPS = 1e-5
TATTN_SCALE = 64 ** -0.5


def tattn_launch(heads, B, n_tok):
    """tattn_launch's plan: (TT, token tiles, nsplit)"""
    C = heads * 64
    TT = R.tattn_tt(C)
    return TT, B * n_tok // TT, R.tattn_nsplit(B * n_tok, TT)


def tattn_inputs(heads, B, n_tok, L, seed=0):
    """-> x [B, n_tok, C], kv [B, L, 2 C], wq, wo [C, C] (bf16 values), gamma, beta, bias [C] fp32"""
    g = _gen(heads, B, n_tok, L, seed)
    C = heads * 64
    x = torch.randn((B, n_tok, C), generator=g) * 1.5 + 0.3
    kv = torch.randn((B, L, 2 * C), generator=g)
    wq, wo = (torch.randn((C, C), generator=g) / math.sqrt(C) for _ in range(2))
    gamma = 1 + 0.2 * torch.randn((C,), generator=g)
    beta, bias = 0.2 * torch.randn((C,), generator=g), 0.3 * torch.randn((C,), generator=g)
    return _bf(x), _bf(kv), _bf(wq), _bf(wo), gamma, beta, bias


def tattn_out_slices(M, C, TT, nsplit):
    """[M, C]: (token tile of TT rows, channel split) — one workgroup of tattn_fused_kernel:
    ``ct_lo = blockIdx.y * (C >> 5) / nsplit, ct_hi = (blockIdx.y + 1) * (C >> 5) / nsplit`` 32-channel tiles"""
    for r0 in range(0, M, TT):
        for y in range(nsplit):
            yield (slice(r0, r0 + TT), slice(y * (C >> 5) // nsplit * 32, (y + 1) * (C >> 5) // nsplit * 32))


def hold_tattn_out(name, got, exp, heads, B, n_tok, report=None):
    """exp = (ref64, emul, abs scale), all [B, n_tok, C]"""
    ref, emul, A = exp
    C = heads * 64
    TT, _, nsplit = tattn_launch(heads, B, n_tok)
    flat = lambda t: t.reshape(B * n_tok, C)
    return S.check_sliced(name, flat(got), flat(ref), flat(emul - ref), tattn_out_slices(B * n_tok, C, TT, nsplit), abs_scale=A, report=report)


def hold_tattn_tables(name, got, ref, report=None):
    """got = dict(A [B, hp, C], sc [B, hp, 2], BmT [B, C, hp]) row-major (attention_ref.tattn_unpack), ref = attention_ref.tattn_prepare's
    float64 dict.  A' by (sample, score column), Bm^T by (sample, 64-channel block), s and c as fp32 sums — s against the sum of the
    A' the kernel stored (its summands ARE the stored values) — and the padded columns exactly A' = 0, s = 0, c = -1e30f."""
    B, hp, C = ref["A"].shape
    worst = S.check_sliced(name + " A'", got["A"], ref["A"], R.bf(ref["A"]) - ref["A"],
                           ((b, j, slice(None)) for b in range(B) for j in range(hp)), report=report)
    worst = max(worst, S.check_sliced(name + " Bm^T", got["BmT"], ref["BmT"], R.bf(ref["BmT"]) - ref["BmT"],
                                      ((b, slice(c0, c0 + 64), slice(None)) for b in range(B) for c0 in range(0, C, 64)), report=report))
    pad = ref["pad"].cpu()
    ga, gsc = S._f64(got["A"]), S._f64(got["sc"])
    live = ~pad
    S.check_fp32_sum(name + " s", gsc[..., 0] * live, ga.sum(dim=-1) * live, ga.abs().sum(dim=-1) * live, report=report)
    S.check_fp32_sum(name + " c", gsc[..., 1] * live, S._f64(ref["c"]) * live, S._f64(ref["c_abs"]) * live, report=report)
    assert bool((ga[pad] == 0).all()) and bool((S._f64(got["BmT"]).transpose(1, 2)[pad] == 0).all()), f"{name}: padded columns of A' / Bm^T"
    assert bool((gsc[..., 0][pad] == 0).all()), f"{name}: s of the padded columns"
    assert bool((gsc[..., 1][pad] == float(torch.tensor(-1e30, dtype=torch.float32))).all()), f"{name}: c of the padded columns"
    return worst
