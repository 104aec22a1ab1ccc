"""Inputs of the reverse-pass edge cases, shared by tests/test_sliced_check_cpu.py (float32 CPU evaluation, planted defects) and
tests/test_backward_edges_gpu.py (the kernels).  A helper, not a test.  Every tensor is float32 holding bf16 values unless the kernel
takes fp32."""
import torch


def _bf(t):
    return t.bfloat16().float()


def _gen(*key):
    return torch.Generator().manual_seed(hash(tuple(int(k) for k in key)) % (2 ** 31))


ATTN_VARIANTS = ("spike", "flat", "alt", "neg")


def attn_inputs(B, H, N, variant="randn", seed=0):
    """-> qkv [B, N, 3 C], d_o [B, N, C].  Variants: spike — one key whose logit leads by more than 100; flat — q = 0 (uniform P);
    alt — d_o = 0 on alternate rows; neg — every real score about -30 after scaling (a padded key scored 0 would dominate)"""
    g = _gen(B, H, N, seed)
    C = H * 64
    qkv = torch.randn((B, N, 3 * C), generator=g)
    d_o = torch.randn((B, N, C), generator=g) * 0.1
    u = 0.125                                                   # the unit vector (1, ..., 1) / 8 of a head
    if variant == "spike":
        qkv[..., :C] = 0.5 * qkv[..., :C] + 8.0 * u             # q . u = 8 +- 0.5
        qkv[:, N // 3, C:2 * C] = 160.0 * u                     # scale * q . k* = 160 +- 10; every other logit is within +- 5
    elif variant == "flat":
        qkv[..., :C] = 0.0
    elif variant == "alt":
        d_o[:, 1::2] = 0.0
    elif variant == "neg":
        qkv[..., :C] = 0.25 * qkv[..., :C] + 4.0 * u
        qkv[..., C:2 * C] = 0.25 * qkv[..., C:2 * C] - 60.0 * u   # scale * q . k = -30 +- 2
    else:
        assert variant == "randn"
    return _bf(qkv), _bf(d_o)


def xattn_inputs(B, H, N, L, seed=0):
    """-> q [B, N, C], kv [B, L, 2 C], d_o [B, N, C] (bf16 values), d_p fp32 [B * H, N, L]"""
    g = _gen(B, H, N, L, seed)
    C = H * 64
    return (_bf(torch.randn((B, N, C), generator=g)), _bf(torch.randn((B, L, 2 * C), generator=g)), _bf(torch.randn((B, N, C), generator=g)),
            torch.randn((B * H, N, L), generator=g))


LN_VARIANTS = ("const_row", "offset")


def ln_inputs(rows, C, variant="randn", seed=0):
    """-> x, dy, add [rows, C], gamma [C].  const_row — row 0 (and the last) constant: variance 0; offset — mean 8, standard deviation
    2^-4 (one bf16 step at 8)"""
    g = _gen(rows, C, seed)
    x = torch.randn((rows, C), generator=g) * 2 + 0.5
    dy = torch.randn((rows, C), generator=g)
    add = torch.randn((rows, C), generator=g)
    gamma = 1 + 0.2 * torch.randn((C,), generator=g)
    if variant == "const_row":
        x[0] = 3.0
        x[-1] = -0.75
    elif variant == "offset":
        x = 8.0 + 2.0 ** -4 * torch.randn((rows, C), generator=g)
    else:
        assert variant == "randn"
    return _bf(x), _bf(dy), _bf(add), gamma


GN_VARIANTS = ("const_group", "saturated", "mean50")


def gn_inputs(B, HW, C, variant="randn", seed=0, groups=32):
    """-> x, dy, add [B, HW, C], gamma, beta [C], silu.  const_group — group 1 of every sample nearly constant; saturated — gamma = 20
    under SiLU; mean50 — mean 50"""
    g = _gen(B, HW, C, seed)
    x = torch.randn((B, HW, C), generator=g) * 1.5 + 0.3
    dy = torch.randn((B, HW, C), generator=g)
    add = torch.randn((B, HW, C), generator=g)
    gamma = 1 + 0.2 * torch.randn((C,), generator=g)
    beta = 0.1 * torch.randn((C,), generator=g)
    silu = True
    cpg = C // groups
    if variant == "const_group":
        x[:, :, cpg:2 * cpg] = 2.0 + 2.0 ** -6 * torch.randn((B, HW, cpg), generator=g).sign()     # 2 +- 2^-6
    elif variant == "saturated":
        gamma = torch.full((C,), 20.0)
    elif variant == "mean50":
        x = x + 50.0
    else:
        assert variant == "randn"
    return _bf(x), _bf(dy), _bf(add), gamma, beta, silu


def geglu_inputs(rows, inner, seed=0):
    """-> ag [rows, 2 inner], dy [rows, inner]; gates at +-30 and 0 among ordinary ones"""
    g = _gen(rows, inner, seed)
    ag = torch.randn((rows, 2 * inner), generator=g) * 1.5
    dy = torch.randn((rows, inner), generator=g)
    gate = ag[:, inner:]
    gate[:, 0::8] = 30.0
    gate[:, 1::8] = -30.0
    gate[:, 2::8] = 0.0
    return _bf(ag), _bf(dy)


def pair_inputs(R, N, K, seed=0):
    """-> dy [R, N], x [R, K] (the weight gradient's operands; dy alone for column sums)"""
    g = _gen(R, N, K, seed)
    return _bf(torch.randn((R, N), generator=g)), _bf(torch.randn((R, K), generator=g))


def seed_inputs(B, h, w, seed=0):
    """-> f fp32 NHWC [B, h, w, 4], noised, target fp32 NCHW [B, 4, h, w]"""
    g = _gen(B, h, w, seed)
    return torch.randn((B, h, w, 4), generator=g), torch.randn((B, 4, h, w), generator=g), torch.randn((B, 4, h, w), generator=g)
