"""Plain restatements of the forward attention family (csrc/attention.hip, csrc/tattn.hip) for tests/sliced_check.py (a helper, not a
test; device-agnostic plain torch).

Every function evaluates the closed form in ``dtype`` (float64: the reference; float32: the CPU evaluation that shows a bound is
attainable in the kernel's arithmetic) on bf16- or fp32-valued operands.  With ``emulate=True`` the same computation is rounded ONLY
where the kernel's own code and comments say it rounds (each docstring quotes the lines), which gives ``emul``;
``floor_err = emul - ref64``.  ``abs`` results are the same formula with every summand replaced by its absolute value, as an RMS over
the tensor (the condition-number scale A of check_sliced) or element by element (the sum|summands| of check_fp32_sum).

Planted defects (keyword arguments, for tests/test_attention_ref_cpu.py): see flash_fwd and tattn_fused.
"""
import math

import torch

F64 = torch.float64
LOG2E = 1.4426950408889634
A2_DEFER = 8.0                  # csrc/attention.hip: constexpr float A2_DEFER = 8.0f
FLASH_KERNELS = {"d64": 64, "v2": 64, "d512": 32}     # kernel -> keys per tile (KV_TILE = 64, A5_KEYS = 32)


def bf(t):
    """round to bf16, keep the dtype"""
    return t.to(torch.bfloat16).to(t.dtype)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def _heads(t, heads, hd):
    B, N, _ = t.shape
    return t[..., :heads * hd].reshape(B, N, heads, hd).permute(0, 2, 1, 3)


def _unheads(t):
    B, H, N, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * D)


# ------------------------------------------------------------------------------------------------ flash attention forward
def _flash_online(s2, v, kernel, ksplit, kt_per, skip_rescale, drop_slice):
    """the kernels' online softmax over key tiles.  s2 [B, H, nq, nk]: scores * scale * log2(e); v [B, H, nk, hd].
    All three kernels (attn_d64_kernel, attn_d64_v2_kernel, attn_d512_body) do, per tile,
        ``const float pv = fast_exp2(s * c - m);  s = pv;  psum += pv;``  then  ``pack_bf16x2(s..)`` for the P V MFMA:
    the row sum l sees the UNROUNDED fp32 P, the product sees bf16(P) — the same in all three.  They differ in the running maximum m:
      d64   ``m_new = fmaxf(m_run, mx * c)`` every tile, per query;
      v2    ``if (!__all(mxs - m_run <= A2_DEFER))`` — the 32 queries of a wave move their maxima together, and only when one of them grew
            by more than 2^8 ("the online-softmax rescale of O is skipped while the running maximum grows by less than 2^8 ... P then
            stays <= 256 ... the normaliser l sees the same P");
      d512  as d64 on tiles of 32 keys; with a key split each slice of kt_per tiles starts from m = -inf and the merge kernel computes
            ``O = sum_z 2^(m_z - m) O_z / sum_z 2^(m_z - m) l_z`` on the fp32 partials."""
    T = FLASH_KERNELS[kernel]
    B, H, nq, nk = s2.shape
    ntiles = (nk + T - 1) // T
    if ksplit <= 1:
        ksplit, kt_per = 1, ntiles
    parts = []
    for z in range(ksplit):
        m = torch.full((B, H, nq, 1), -math.inf, dtype=s2.dtype, device=s2.device)
        l = torch.zeros_like(m)
        acc = torch.zeros((B, H, nq, v.shape[-1]), dtype=s2.dtype, device=s2.device)
        for kt in range(z * kt_per, min((z + 1) * kt_per, ntiles)):
            st = s2[..., kt * T:(kt + 1) * T]
            mx = st.max(dim=-1, keepdim=True).values
            if kernel == "v2":
                grew = (mx - m) > A2_DEFER
                pad = (-nq) % 32
                g = torch.nn.functional.pad(grew, (0, 0, 0, pad)).reshape(B, H, -1, 32, 1).any(dim=3, keepdim=True)
                g = g.expand(-1, -1, -1, 32, -1).reshape(B, H, -1, 1)[:, :, :nq]
                m_new = torch.where(g, torch.maximum(m, mx), m)
            else:
                m_new = torch.maximum(m, mx)
            alpha = torch.exp2(m - m_new)
            if skip_rescale is None or kt != skip_rescale:
                l, acc = l * alpha, acc * alpha
            m = m_new
            p = torch.exp2(st - m)
            l = l + p.sum(dim=-1, keepdim=True)
            acc = acc + bf(p) @ v[..., kt * T:(kt + 1) * T, :]
        parts.append((m, l, acc))
    if drop_slice is not None:
        parts = [pz for z, pz in enumerate(parts) if z != drop_slice]
    m_all = parts[0][0]
    for m, _, _ in parts[1:]:
        m_all = torch.maximum(m_all, m)
    l_tot = sum(torch.exp2(m - m_all) * l for m, l, _ in parts)
    acc_tot = sum(torch.exp2(m - m_all) * acc for m, _, acc in parts)
    return acc_tot / l_tot


def flash_fwd(q, k, v, heads, scale, head_dim=64, dtype=F64, emulate=False, kernel="v2", ksplit=1, kt_per=0, drop_last_key=False,
              pad_score0=0, skip_rescale=None, stale_block=None, drop_slice=None):
    """softmax(q k^T scale) v per (sample, head): q [B, nq, >= heads * head_dim], k, v [B, nk, >= heads * head_dim] ->
    emulate=False: (out [B, nq, heads * head_dim] in ``dtype``, abs scale); emulate=True: the emulation (see _flash_online; softmax in
    base 2 with ``p.scale_log2e = scale * 1.4426950408889634f``, P to bf16 before P V, the normaliser from the unrounded P, and the
    output to bf16: ``pack_bf16x2(o_acc[..] * inv, ..)``); emulate="both": (exact, emulated, abs scale).  head_dim = 512 with one head
    is udt_attn512_fwd (kernel="d512"; ksplit / kt_per: the launcher's plan, see attention_cases.attn512_plan).
    Planted defects (they act on the emulation):
      drop_last_key     the last key is masked with the padding;
      pad_score0 = n    n padded keys (K = V = 0) take part in the softmax with score 0;
      skip_rescale = t  at key tile t the maximum moves but O and l are not rescaled;
      stale_block = ((b, h, r0), (b2, h2))  the 32 queries from r0 of (b, h) hold what (b2, h2) computed for those rows;
      drop_slice = z    the key-split merge leaves out slice z."""
    qh, kh, vh = (_heads(t.to(dtype), heads, head_dim) for t in (q, k, v))
    s2 = qh @ kh.transpose(-1, -2) * (scale * LOG2E)

    def exact():
        p = torch.exp2(s2 - s2.max(dim=-1, keepdim=True).values)
        l = p.sum(dim=-1, keepdim=True)
        return _unheads(p @ vh / l), rms(p @ vh.abs() / l)

    def emulated():
        s, vv = s2, vh
        if drop_last_key:
            s, vv = s[..., :-1], vv[..., :-1, :]
        if pad_score0:
            s = torch.cat((s, torch.zeros(s.shape[:-1] + (pad_score0,), dtype=dtype, device=s.device)), dim=-1)
            vv = torch.cat((vv, torch.zeros(vv.shape[:2] + (pad_score0, vv.shape[-1]), dtype=dtype, device=s.device)), dim=2)
        o = _flash_online(s, vv, kernel, ksplit, kt_per, skip_rescale, drop_slice)
        if stale_block is not None:
            (b, h, r0), (b2, h2) = stale_block
            o[b, h, r0:r0 + 32] = o[b2, h2, r0:r0 + 32]
        return bf(_unheads(o))
    if emulate == "both":
        return exact() + (emulated(),)
    return emulated() if emulate else exact()


def flash_ref_emul(q, k, v, heads, scale, head_dim=64, **kw):
    """(ref64, floor_err, abs scale)"""
    ref, a, emul = flash_fwd(q, k, v, heads, scale, head_dim, emulate="both", **kw)
    return ref, emul - ref, a


# ------------------------------------------------------------------------------------------------ short-context attention
def xattn_fwd(q, kv, heads, head_dim, scale, dtype=F64, emulate=False):
    """q [B, nq, C], kv [B, L, 2 C] (k | v), C = heads * head_dim -> dict(out [B, nq, C], probs [B * heads, nq, L][, abs]).  A single
    context token takes the sigmoid (``if (p.L == 1) ... sc[0] = 1.0f / (1.0f + __expf(-sc[0]))``).  xattn_kernel keeps K, V, the scores
    and the probabilities in fp32 (``ks[i] = bf16_bits_to_f32(p.k[off])``, ``pr[l] = sc[l]``) and rounds once:
    ``pack_bf16x2(acc[0], acc[1])`` at the store of the output — emulate rounds ``out`` to bf16 and leaves ``probs`` alone."""
    B, nq, C = q.shape
    L = kv.shape[1]
    qh = _heads(q.to(dtype), heads, head_dim)
    kh, vh = _heads(kv[..., :C].to(dtype), heads, head_dim), _heads(kv[..., C:].to(dtype), heads, head_dim)
    sim = qh @ kh.transpose(-1, -2) * scale
    p = sim.softmax(dim=-1) if L > 1 else sim.sigmoid()
    out = _unheads(p @ vh)
    res = {"out": bf(out) if emulate else out, "probs": p.reshape(B * heads, nq, L)}
    if not emulate:
        res["abs"] = rms(p @ vh.abs())
    return res


def xattn_probs_base(q, kv, heads, head_dim, scale):
    """the worst |probs32 - probs64| of the float32 torch restatement on these inputs: the measured base of the probabilities' bound
    (tests hold the kernel's fp32 probabilities to 8 x this, the factor tests/shadow_ref.py uses for "another operation order and a
    fast exp")"""
    p64 = xattn_fwd(q, kv, heads, head_dim, scale)["probs"]
    p32 = xattn_fwd(q, kv, heads, head_dim, scale, dtype=torch.float32)["probs"]
    return float((p32.double() - p64).abs().max())


# ------------------------------------------------------------------------------------------------ masked small attention
def mattn_fwd(q, k, v, heads, scale, mask=None, kpm=None, dtype=F64, emulate=False):
    """nn.MultiheadAttention's core: q [B, nq, heads * D], k, v [B, lk, >= heads * D], mask fp32 [nq, lk] additive (may hold -inf), kpm
    bool [B, lk] (true = ignore) -> emulate=False: (out, abs scale); emulate=True: out rounded to bf16 at the store
    (``p.o[..] = (uint16_t)(pack_bf16x2(acc, 0.f) & 0xffffu)``; K, V, the scores and P stay fp32 in LDS).  A fully masked row gives
    zeros: ``sc[j] = (mx == -INFINITY || sc[j] == -INFINITY) ? 0.f : __expf(sc[j] - mx)`` and
    ``const float inv = sum > 0.f ? 1.0f / sum : 0.f``."""
    B, nq, Cq = q.shape
    D = Cq // heads
    qh, kh, vh = (_heads(t.to(dtype), heads, D) for t in (q, k, v))
    s = qh @ kh.transpose(-1, -2) * scale
    if mask is not None:
        s = s + mask.to(dtype)
    if kpm is not None:
        s = s.masked_fill(kpm.bool()[:, None, None, :], -math.inf)
    mx = s.max(dim=-1, keepdim=True).values
    dead = torch.isinf(s) & (s < 0)
    zero = torch.zeros_like(s)
    e = torch.where(dead, zero, torch.exp(torch.where(dead, zero, s - torch.where(torch.isinf(mx), torch.zeros_like(mx), mx))))
    tot = e.sum(dim=-1, keepdim=True)
    p = torch.where(tot > 0, e / tot.clamp_min(1e-300), torch.zeros_like(e))
    out = _unheads(p @ vh)
    if emulate:
        return bf(out)
    return out, rms(p @ vh.abs())


# ------------------------------------------------------------------------------------------------ row softmax
def softmax_rows(x, dtype=F64, emulate=False):
    """x [rows, cols] (bf16 values) -> softmax over the row; softmax_rows_kernel: "in-place row softmax over bf16 [rows, cols]; one
    workgroup per row, fp32 math", rounded at the store: ``pack_bf16x2(__expf(bf16_lo(v[j]) - mx) * inv, ..)``"""
    out = torch.softmax(x.to(dtype), dim=-1)
    return bf(out) if emulate else out


# ------------------------------------------------------------------------------------------------ fused text cross-attention
def tattn_hp(heads):
    return (heads * 16 + 31) // 32 * 32


def tattn_tt(C):
    """tokens per workgroup: ``int tattn_tt(int C) { return C >= 640 ? 32 : 64; }``"""
    return 32 if C >= 640 else 64


def tattn_nsplit(M, TT):
    """workgroups per token tile: ``while (nsplit < 8 && grid * nsplit < target) nsplit *= 2`` with grid = M / TT, target = 256"""
    grid, n = M // TT, 1
    while n < 8 and grid * n < 256:
        n *= 2
    return n


def _a_offsets(hp, C):
    """element offsets of the logical A'[j][k] in the fragment-major table (tattn_prepare_a_kernel's ``aoff``)"""
    j = torch.arange(hp).reshape(hp, 1)
    k = torch.arange(C).reshape(1, C)
    nkt = C >> 6
    return ((((j >> 5) * nkt + (k >> 6)) * 4 + ((k >> 4) & 3)) * 64 + ((k >> 3) & 1) * 32 + (j & 31)) * 8 + (k & 7)


def _b_offsets(C, hp):
    """element offsets of the logical Bm^T[c][j] in the fragment-major table (tattn_prepare_b_kernel's ``off``)"""
    c = torch.arange(C).reshape(C, 1)
    j = torch.arange(hp).reshape(1, hp)
    return ((((c >> 5) * (hp >> 4) + (j >> 4)) * 64) + ((j >> 3) & 1) * 32 + (c & 31)) * 8 + (j & 7)


def tattn_unpack(A, BmT):
    """the kernel's fragment-major tables A [B, hp, C], BmT [B, C, hp] -> the row-major matrices A'[b][j][k], Bm^T[b][c][j]"""
    B, hp, C = A.shape
    oa, ob = _a_offsets(hp, C).to(A.device), _b_offsets(C, hp).to(A.device)
    return A.reshape(B, -1)[:, oa.reshape(-1)].reshape(B, hp, C), BmT.reshape(B, -1)[:, ob.reshape(-1)].reshape(B, C, hp)


def tattn_pack(A, BmT):
    """the inverse of tattn_unpack"""
    B, hp, C = A.shape
    oa, ob = _a_offsets(hp, C).to(A.device), _b_offsets(C, hp).to(A.device)
    pa, pb = torch.empty_like(A).reshape(B, -1), torch.empty_like(BmT).reshape(B, -1)
    pa[:, oa.reshape(-1)] = A.reshape(B, -1)
    pb[:, ob.reshape(-1)] = BmT.reshape(B, -1)
    return pa.reshape(B, hp, C), pb.reshape(B, C, hp)


def tattn_fused(x, A, sc, BmT, bias, heads, zero_samples, eps, dtype=F64, emulate=False, swap_heads=None):
    """x [B, N, C] + t_attn(LayerNorm(x)) + bias from the tables udt_tattn_prepare produced (teacher forcing: the launch's operands are
    the bf16 tables, the folding error is not this launch's error): A [B, hp, C] = A' and BmT [B, C, hp] ROW-MAJOR (tattn_unpack), sc
    [B, hp, 2] = (s_j, c_j) -> emulate=False: (out, abs scale); emulate=True: the emulation.  tattn.hip's header:
        ``S_j = rstd * (x . A'_j - mean * s_j) + c_j`` ... ``softmax over each head's 16-column group (12 real + 4 padded columns whose
        c_j = -1e30) -> P (bf16, LDS) -> out^T = Bm^T P^T on the MFMAs -> + bias + x -> store``
    so P is rounded to bf16 (``pack_bf16x2(sv[r4 * 4], sv[r4 * 4 + 1])``) and the result once at the store
    (``pack_bf16x2(v[r4 * 4 + 0], ..)``); the statistics are ``mean = s / C; var = q / C - mean * mean; if (var < 0.f) var = 0.f;
    rsqrtf(var + p.eps)`` in fp32.  The first zero_samples samples are x + bias.
    swap_heads = (h1, h2): the two heads' 16-column groups of P change places (a planted defect)."""
    B, N, C = x.shape
    hp = A.shape[1]
    x, A, sc, BmT, bias = (t.to(dtype) for t in (x, A, sc, BmT, bias[:C]))
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x * x).mean(dim=-1, keepdim=True) - mean * mean).clamp_min(0)
    rstd = (var + eps).rsqrt()
    S = rstd * (x @ A.transpose(1, 2) - mean * sc[:, None, :, 0]) + sc[:, None, :, 1]
    P = S.reshape(B, N, hp // 16, 16).softmax(dim=-1)
    if swap_heads is not None:
        h1, h2 = swap_heads
        P = P.clone()
        P[:, :, [h1, h2]] = P[:, :, [h2, h1]]
    P = P.reshape(B, N, hp)
    out = (bf(P) if emulate else P) @ BmT.transpose(1, 2) + bias + x
    out[:zero_samples] = x[:zero_samples] + bias
    if emulate:
        return bf(out)
    a = P @ BmT.abs().transpose(1, 2) + bias.abs() + x.abs()
    a[:zero_samples] = x[:zero_samples].abs() + bias.abs()
    return out, rms(a)


def tattn_prepare(kv, wq, wo, gamma, beta, heads, scale, dtype=F64, emulate=False):
    """the fold of tattn.hip's header comment, kv [B, L, 2 C] (k | v), wq, wo [>= C, >= C] row-major [out][in]:
        ``A'[b][j][k] = gamma_k * scale * sum_d Wq[h*64+d][k] K[b][i][h*64+d]``  (j = 16 h + i), stored bf16
            (``const uint32_t pk = pack_bf16x2(a * gamma[k], 0.f)``);
        ``s_j = sum_k bf16(A')``, ``c_j = scale * sum_k beta_k sum_d (...)`` in fp32;
        ``BmT[b][c][j] = sum_d V[b][i][h*64+d] Wo[c][h*64+d]``, stored bf16 (``pack_bf16x2(a, 0.f)``);
        "padded columns (i >= L): A' = 0, s = 0, c = -1e30".
    -> dict(A [B, hp, C], s, c [B, hp], BmT [B, C, hp], s_abs, c_abs [B, hp]) row-major; emulate rounds A and BmT to bf16 (s is the sum
    of the rounded A' either way)."""
    B, L, C2 = kv.shape
    C = C2 // 2
    hp = tattn_hp(heads)
    kv, wq, wo, gamma, beta = kv.to(dtype), wq[:C, :C].to(dtype), wo[:C, :C].to(dtype), gamma.to(dtype), beta.to(dtype)
    kh = kv[..., :C].reshape(B, L, heads, 64)
    vh = kv[..., C:].reshape(B, L, heads, 64)
    wqh = wq.reshape(heads, 64, C)                             # [h][d][k]
    woh = wo.reshape(C, heads, 64)                             # [c][h][d]
    a = torch.einsum("hdk,blhd->bhlk", wqh, kh) * scale        # [B, heads, L, C]
    a_abs = torch.einsum("hdk,blhd->bhlk", wqh.abs(), kh.abs()) * scale
    A = torch.zeros((B, hp // 16, 16, C), dtype=dtype, device=kv.device)
    A[:, :heads, :L] = a * gamma
    A = A.reshape(B, hp, C)
    Ar = bf(A)
    pad = torch.ones((B, hp // 16, 16), dtype=torch.bool, device=kv.device)
    pad[:, :heads, :L] = False
    pad = pad.reshape(B, hp)
    c = torch.zeros((B, hp // 16, 16), dtype=dtype, device=kv.device)
    c[:, :heads, :L] = (a * beta).sum(dim=-1)
    c = torch.where(pad, torch.full_like(c.reshape(B, hp), -1e30), c.reshape(B, hp))
    c_abs = torch.zeros((B, hp // 16, 16), dtype=dtype, device=kv.device)
    c_abs[:, :heads, :L] = (a_abs * beta.abs()).sum(dim=-1)
    Bm = torch.zeros((B, C, hp // 16, 16), dtype=dtype, device=kv.device)
    Bm[:, :, :heads, :L] = torch.einsum("blhd,chd->bchl", vh, woh)
    Bm = Bm.reshape(B, C, hp)
    return {"A": Ar if emulate else A, "s": Ar.sum(dim=-1), "c": c, "BmT": bf(Bm) if emulate else Bm, "s_abs": Ar.abs().sum(dim=-1),
            "c_abs": c_abs.reshape(B, hp), "pad": pad}
