"""The sidecar rule of udifftext_amd/ops.py: an op that writes into a caller-visible tensor drops BOTH sidecars an earlier launch may
have left on it (``gn_stats``, ``mx8``) and attaches only what its own launch emits.  Every function is called twice at the smallest
shape the library takes — into a clean tensor and into one that carries two sentinels — and the results must be bit-equal.
The attention shapes are the smallest of tests/attention_cases.py's lists (attention_mx8 has none there: the smallest of
tests/test_mx8_gpu.py's)."""
import math

import pytest
import torch

import attention_cases as K
import test_mx8_gpu

pytestmark = pytest.mark.gpu
STALE = {"gn_stats": object(), "mx8": object()}
BF16, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib, ops, packing
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)

    class Env:
        pass
    Env.ops, Env.L, Env.P, Env.dev = ops, lib, packing, cuda
    return Env


def _rand(env, shape, seed, scale=1.0, dtype=BF16):
    return (torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale).to(dtype).to(env.dev)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _hold(env, call, fresh, emits=()):
    """call(dst) writes dst and returns it; fresh() makes dst.  -> the result of the call on the tensor that carried the sentinels"""
    want = call(fresh())
    dst = fresh()
    for name, s in STALE.items():
        setattr(dst, name, s)
    got = call(dst)
    assert got is dst
    for name, kind, of in (("gn_stats", env.ops.GnStats, env.ops.gn_stats_of), ("mx8", env.ops.Mx8Act, env.ops.mx8_of)):
        if name in emits:
            new, ref = of(got), of(want)
            assert isinstance(new, kind) and isinstance(ref, kind), f"{name} was not emitted"
            for a, b in zip(new, ref):
                assert (a == b) if not isinstance(a, torch.Tensor) else torch.equal(_bits(a), _bits(b)), f"emitted {name} differs"
        else:
            assert of(got) is None and not hasattr(got, name), f"a stale {name} survived the launch"
            assert of(want) is None
    assert torch.equal(_bits(got), _bits(want)), "the result depends on the sidecars the destination carried"
    return got


def _smallest(shapes, size):
    return min(shapes, key=size)


# ------------------------------------------------------------------------------------------------ GEMM family
def _lin(env, M, N, K_, seed=1):
    w = env.P.pack_linear(torch.randn((N, K_), generator=torch.Generator().manual_seed(seed + 1)) / math.sqrt(K_)).to(env.dev)
    return _rand(env, (M, K_), seed), w, _rand(env, (N,), seed + 2, dtype=F32)


def test_linear_out(env):
    x, w, b = _lin(env, 128, 128, 128)
    _hold(env, lambda o: env.ops.linear(x, w, b, out=o), lambda: torch.empty((128, 128), dtype=BF16, device=env.dev))


MX8_EMIT_SHAPES = ((130, 256, 256), (130, 640, 640), (130, 1280, 1280))      # test_footprint_gpu._mx8_emit's candidates


def _emitting_linear(env, shapes, kw_of):
    """the first of ``shapes`` whose plan emits what ``kw_of(M)`` asks for"""
    for M, N, K_ in shapes:
        x, w, b = _lin(env, M, N, K_, seed=41)
        probe = env.ops.linear(x, w, b, **kw_of(M))
        if env.ops.gn_stats_of(probe) is not None or env.ops.mx8_of(probe) is not None:
            return x, w, b, M, N, kw_of(M)
    reason = f"the library declines an emitting plan ({kw_of(shapes[0][0])}) at every candidate of {shapes}"
    print(reason)
    pytest.skip(reason)


def test_linear_emitting_colstats(env):
    """a statistics slot holds 32 or 64 rows of ONE sample (gemm.hip colstats_rows), so no plan emits at M = 130: the candidates go
    on to the 128 x 128 x 128 of test_linear_out as two samples of 64 rows"""
    x, w, b, M, N, kw = _emitting_linear(env, MX8_EMIT_SHAPES + ((128, 128, 128),),
                                         lambda M: dict(colstats=True, rows_per_batch=M if M == 130 else 64))
    _hold(env, lambda o: env.ops.linear(x, w, b, out=o, **kw), lambda: torch.empty((M, N), dtype=BF16, device=env.dev), emits=("gn_stats",))


def test_linear_emitting_q8(env):
    x, w, b, M, N, kw = _emitting_linear(env, MX8_EMIT_SHAPES, lambda M: dict(emit_q8=True))
    _hold(env, lambda o: env.ops.linear(x, w, b, out=o, **kw), lambda: torch.empty((M, N), dtype=BF16, device=env.dev), emits=("mx8",))


def test_ln_linear(env):
    M, N, K_ = 130, 960, 320
    g = torch.Generator().manual_seed(5)
    w, bias = torch.randn((N, K_), generator=g) / math.sqrt(K_), torch.randn((N,), generator=g)
    gamma, beta = 1 + 0.2 * torch.randn((K_,), generator=g), 0.2 * torch.randn((K_,), generator=g)
    wp, c, s = (t.to(env.dev) for t in env.P.pack_ln_linear(w, bias, gamma, beta))
    x = _rand(env, (M, K_), 6)
    _hold(env, lambda o: env.ops.ln_linear(x, wp, c, s, out=o), lambda: torch.empty((M, N), dtype=BF16, device=env.dev))


def test_bmm_nt(env):
    B, M, N, K_ = 2, 70, 72, 64
    a, w = _rand(env, (B, M, K_), 51), _rand(env, (B, N, K_), 52, 1 / math.sqrt(K_))
    _hold(env, lambda o: env.ops.bmm_nt(a, w, out=o), lambda: torch.empty((B, M, N), dtype=BF16, device=env.dev))


def test_conv2d(env):
    x, w, b = _rand(env, (1, 8, 8, 64), 61), _rand(env, (64, 9 * 64), 62, 1 / 24.0), _rand(env, (64,), 63, dtype=F32)
    fresh = lambda: torch.empty((1, 8, 8, 64), dtype=BF16, device=env.dev)
    _hold(env, lambda o: env.ops.conv2d(x, w, b, out=o), fresh)
    # colstats=True: today no plan of the library emits statistics for 64 output channels (both sentinels go all the same); the
    # same input -> 128 channels is the smallest convolution that does
    emitted = []
    for N in (64, 128):
        w, b = _rand(env, (N, 9 * 64), 64, 1 / 24.0), _rand(env, (N,), 65, dtype=F32)
        emitted.append(env.ops.gn_stats_of(env.ops.conv2d(x, w, b, colstats=True)) is not None)
        print(f"conv2d 3x3 1x8x8x64 -> {N}: column statistics {'emitted' if emitted[-1] else 'declined by the library'}")
        _hold(env, lambda o: env.ops.conv2d(x, w, b, out=o, colstats=True), lambda: torch.empty((1, 8, 8, N), dtype=BF16, device=env.dev),
              emits=("gn_stats",) if emitted[-1] else ())
    assert any(emitted), "no convolution emitted column statistics"


# ------------------------------------------------------------------------------------------------ attention
def _dev(env, *ts):
    return tuple(t.bfloat16().to(env.dev).contiguous() for t in ts)


@pytest.mark.parametrize("entry", ["vt", "rowv", "rowv_q8"])
def test_flash_attention_d64(env, entry):
    shapes = K.D64_SHAPES["vt" if entry == "vt" else "rowv"]
    if entry == "rowv_q8":
        shapes = [s for s in shapes if s[1] % 2 == 0]             # (the emitting kernel takes an even head count)
    B, H, nq, nk = _smallest(shapes, lambda s: s[0] * s[1] * (s[2] + s[3]))
    q, k, v = _dev(env, *K.flash_inputs(B, H, nq, nk))
    fresh = lambda: torch.empty((B, nq, H * 64), dtype=BF16, device=env.dev)
    if entry == "vt":
        vt = v.transpose(1, 2).contiguous()
        _hold(env, lambda o: env.ops.attention(q, k, vt, H, 0.125, out=o), fresh)
    elif entry == "rowv":
        _hold(env, lambda o: env.ops.attention_rowv(q, k, v, H, 0.125, out=o), fresh)
    else:
        _hold(env, lambda o: env.ops.attention_rowv(q, k, v, H, 0.125, out=o, emit_q8=True), fresh, emits=("mx8",))


def test_attention_mx8(env):
    B, N, heads = 1, 64, 2
    data, scale = test_mx8_gpu._qkv8(env.dev, B, N, heads, seed=13)[:2]
    _hold(env, lambda o: env.ops.attention_mx8(env.ops.Mx8Act(data, scale), B, heads, 0.125, test_mx8_gpu.V_MUL, out=o),
          lambda: torch.empty((B, N, heads * 64), dtype=BF16, device=env.dev))


@pytest.mark.parametrize("key_split", [False, True])
def test_attention_d512(env, key_split):
    B, nq, nk, _ = _smallest([s for s in K.D512_SHAPES if s[3] == key_split], lambda s: s[0] * (s[1] + s[2]))
    q, k, v = _dev(env, *K.flash_inputs(B, 1, nq, nk, head_dim=512))
    _hold(env, lambda o: env.ops.attention_d512(q, k, v, 512 ** -0.5, out=o, key_split=key_split),
          lambda: torch.empty((B, nq, 512), dtype=BF16, device=env.dev))


def test_xattention(env):
    (B, H), hd, nq, L = K.XATTN_BH, min(K.XATTN_HEAD_DIM), min(K.XATTN_NQ), min(K.XATTN_L)
    q, kv = _dev(env, *K.xattn_inputs(B, H, hd, nq, L))
    C = H * hd
    _hold(env, lambda o: env.ops.xattention(q, kv[..., :C], kv[..., C:], H, hd, hd ** -0.5, out=o),
          lambda: torch.empty((B, nq, C), dtype=BF16, device=env.dev))


def test_masked_attention(env):
    (B, H), (D, lk), nq = K.MATTN_BH, min(K.MATTN_D_LK, key=lambda s: s[0] * s[1]), min(K.MATTN_NQ)
    q, k, v, mask, kpm = K.mattn_inputs(B, H, D, nq, lk, True, True)
    q, k, v = _dev(env, q, k, v)
    mask, kpm = mask.to(env.dev), kpm.to(env.dev)
    _hold(env, lambda o: env.ops.masked_attention(q, k, v, H, D ** -0.5, mask=mask, key_padding_mask=kpm, out=o),
          lambda: torch.empty((B, nq, H * D), dtype=BF16, device=env.dev))


@pytest.mark.parametrize("emit", [False, True])
def test_tattn_fused(env, emit):
    heads, B, n_tok, L, zero = _smallest(K.TATTN_SHAPES, lambda s: s[0] * s[1] * s[2])
    x, kv, wq, wo, gamma, beta, bias = K.tattn_inputs(heads, B, n_tok, L)
    xb, kvb, wqb, wob = _dev(env, x, kv, wq, wo)
    ga, be, bi = (t.to(env.dev) for t in (gamma, beta, bias))
    tabs = None if zero == B else env.ops.tattn_prepare(kvb, wqb, wob, ga, be, heads, K.TATTN_SCALE)
    if emit:
        assert env.L.load().udt_tattn_rowstat_parts(B, n_tok, heads * 64) > 0, "the smallest fused text attention emits no MX8 twin"
    _hold(env, lambda o: env.ops.tattn_fused(xb, tabs, bi, heads, zero, K.TATTN_EPS, out=o, emit_q8=emit), lambda: torch.empty_like(xb),
          emits=("mx8",) if emit else ())


# ------------------------------------------------------------------------------------------------ norms and element-wise
@pytest.mark.parametrize("strip", [True, False])
def test_group_norm(env, strip, monkeypatch):
    monkeypatch.setattr(env.ops, "GN_STRIP", strip)
    x = _rand(env, (1, 64, 64), 71)
    gamma, beta = _rand(env, (64,), 72, dtype=F32), _rand(env, (64,), 73, dtype=F32)
    fresh = lambda: torch.empty_like(x)
    _hold(env, lambda o: env.ops.group_norm(x, gamma, beta, 32, 1e-5, True, out=o), fresh)
    xf = x[0].float()
    st = env.ops.GnStats(torch.stack([xf.sum(0), (xf * xf).sum(0)], dim=-1)[None].contiguous(), 1)
    _hold(env, lambda o: env.ops.group_norm_from_stats(x, st, gamma, beta, 32, 1e-5, True, out=o), fresh)


def test_layer_norm_and_bias_add(env):
    x = _rand(env, (8, 320), 81)
    gamma, beta = _rand(env, (320,), 82, dtype=F32), _rand(env, (320,), 83, dtype=F32)
    _hold(env, lambda o: env.ops.layer_norm(x, gamma, beta, out=o), lambda: torch.empty_like(x))
    _hold(env, lambda o: env.ops.bias_add(x, beta, out=o), lambda: torch.empty_like(x))


def test_in_place_add_and_softmax(env):
    x, y = _rand(env, (8, 64), 91), _rand(env, (8, 64), 92)
    _hold(env, lambda o: env.ops.add_(o, y), x.clone)
    _hold(env, env.ops.softmax_rows_, x.clone)
