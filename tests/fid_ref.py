"""float64 restatement of FID as udifftext_amd/fid_inception.py defines it, in plain torch on NCHW tensors and numpy, with
the per-element bounds the kernels of csrc/fid.hip are held to.  u = 2^-24 is the unit roundoff of fp32, v = 2^-53 that of fp64.
The architecture is written out here as a literal conv -> BatchNorm -> ReLU network; nothing is imported from the module under test.

Convolution (``conv``).  The same arithmetic as udt_conv2d_f32 (K rounded products, K additions, the bias), so lpips_ref.conv's bound
holds with K = kh kw Cin:  |got - ref| <= (K + 2) u (sum |w||x| + |b|) (1 + 2^-10)  per output element, for any summation order.

Average pool (``avg_pool``).  The taps inside the image (t of them, 1 <= t <= 9) are added one by one and divided by t: at most eight
rounded additions and one rounded division, |got - ref| <= 9 u (sum |x| / t) (1 + 2^-10).  The max-pool does not round.

Input stage (``input_stage``).  The 8-bit value q (or the clamped continuous value) is restated in fp32 exactly as the kernel computes
it.  From there on the kernel rounds p = q/255 (1), the column weight (1), one product and one fused multiply-add per row pair (2), the
row weight (1), one product and one fused multiply-add (2): at most 7 <= 8 roundings of non-negative terms on the way to r, then
out = 2 r - 1 with 2 r exact and one rounding:  |got - ref| <= (2 * 8 u r + u |2 r - 1|) (1 + 2^-10).

Global mean (``mean_pixels``).  P rounded additions and one division: |got - ref| <= (P + 1) u mean|x| (1 + 2^-10).

Moments (``moments``).  fp32 -> fp64 is exact; an element of X^T X is a chain of n fp64 fused multiply-adds (n roundings) added to the
stored value (one more when that is not zero):  |got - ref| <= n v sum_r |x_ri x_rj| (+ v |result| in the accumulating call), and
n v sum_r |x_ri| for the sum.  Integers below 2^53 are exact.

Blocks and the whole network: no simple bound exists; tests run this restatement in fp32 on the CPU on their own inputs, take its
largest relative distance from the float64 run, and allow the GPU 8 times that (tests/test_fid_gpu.py; DESIGN §20's rule).
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
V = 2.0 ** -53
SLACK = 1.0 + 2.0 ** -10
EPS = 1e-3
SIZE = 299


# ------------------------------------------------------------------------------------------------ kernels
def conv(x, w, b, stride, pad, relu):
    """x [N, Cin, H, W], w [Cout, Cin, kh, kw], b [Cout] or None, pad = (pad_h, pad_w) -> (float64 reference, float64 bound)"""
    xd, wd = x.double(), w.double()
    bd = None if b is None else b.double()
    ref = F.conv2d(xd, wd, bd, stride=stride, padding=pad)
    mag = F.conv2d(xd.abs(), wd.abs(), None if bd is None else bd.abs(), stride=stride, padding=pad)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return (ref.clamp_min(0.0) if relu else ref), (K + 2) * U * mag * SLACK


def avg_pool(x, stride, pad):
    xd = x.double()
    ref = F.avg_pool2d(xd, 3, stride, pad, count_include_pad=False)
    return ref, 9 * U * F.avg_pool2d(xd.abs(), 3, stride, pad, count_include_pad=False) * SLACK


def max_pool(x, stride, pad):
    return F.max_pool2d(x, 3, stride, pad)


def saved_values(samples, images, quantise=True):
    """fp32 [2 N, 3, H, W]: the clamped (and truncated) 8-bit values, bit for bit what the kernel states (torch's CPU elementwise
    operations do not contract)"""
    s, x = samples.float(), images.float()
    v = torch.cat((s * 255.0, ((x + 1.0) * 0.5) * 255.0), 0)
    assert v.dtype == torch.float32
    v = v.clamp(0.0, 255.0)
    return v.trunc() if quantise else v


def _taps(n_in, n_out):
    """output i reads source coordinate max(0, (i + 0.5) n_in / n_out - 0.5) = max(0, (2 i + 1) n_in - n_out) / (2 n_out)"""
    i = torch.arange(n_out, dtype=torch.int64)
    num = ((2 * i + 1) * n_in - n_out).clamp_min(0)
    den = 2 * n_out
    q = torch.div(num, den, rounding_mode="floor")
    i0 = q.clamp_max(n_in - 1)
    i1 = (i0 + 1).clamp_max(n_in - 1)
    w1 = (num - q * den).double() / den
    return i0, i1, 1.0 - w1, w1


def resize(p, size=SIZE):
    """float64 bilinear resize (align_corners=False, no antialiasing) of p [..., H, W] to size x size"""
    y0, y1, wy0, wy1 = _taps(p.shape[-2], size)
    x0, x1, wx0, wx1 = _taps(p.shape[-1], size)
    rows = p[..., y0, :] * wy0.reshape(-1, 1) + p[..., y1, :] * wy1.reshape(-1, 1)
    return rows[..., x0] * wx0 + rows[..., x1] * wx1


def input_stage(samples, images, quantise=True, size=SIZE):
    """-> (float64 [2 N, 3, size, size] in [-1, 1], its bound)"""
    r = resize(saved_values(samples, images, quantise).double() / 255.0, size)
    out = 2.0 * r - 1.0
    return out, (16.0 * U * r + U * out.abs()) * SLACK


def mean_pixels(x):
    xd = x.double()
    P = x.shape[2] * x.shape[3]
    return xd.mean((2, 3)), (P + 1) * U * xd.abs().mean((2, 3)) * SLACK


def moments(x):
    """x fp32 [n, D] -> (sum float64 [D], outer float64 [D, D], bound of sum, bound of outer) for one call from zero"""
    xd = x.double()
    n = x.shape[0]
    return xd.sum(0), xd.t() @ xd, n * V * xd.abs().sum(0), n * V * (xd.abs().t() @ xd.abs())


# ------------------------------------------------------------------------------------------------ the network, unfolded
def basic(x, sd, name, stride=1, padding=0):
    """BasicConv2d: conv (no bias) -> BatchNorm(eps 1e-3), inference form -> ReLU, in x's dtype"""
    t = lambda k: sd[f"{name}.{k}"].to(x.dtype)
    y = F.conv2d(x, t("conv.weight"), None, stride=stride, padding=padding)
    y = F.batch_norm(y, t("bn.running_mean"), t("bn.running_var"), t("bn.weight"), t("bn.bias"), training=False, eps=EPS)
    return F.relu(y)


def _avg(x):
    return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)


def inception_a(x, sd, n):
    b1 = basic(x, sd, f"{n}.branch1x1")
    b5 = basic(basic(x, sd, f"{n}.branch5x5_1"), sd, f"{n}.branch5x5_2", padding=2)
    b3 = basic(basic(basic(x, sd, f"{n}.branch3x3dbl_1"), sd, f"{n}.branch3x3dbl_2", padding=1), sd, f"{n}.branch3x3dbl_3", padding=1)
    bp = basic(_avg(x), sd, f"{n}.branch_pool")
    return torch.cat((b1, b5, b3, bp), 1)


def inception_b(x, sd, n):
    b3 = basic(x, sd, f"{n}.branch3x3", stride=2)
    bd = basic(basic(basic(x, sd, f"{n}.branch3x3dbl_1"), sd, f"{n}.branch3x3dbl_2", padding=1), sd, f"{n}.branch3x3dbl_3", stride=2)
    return torch.cat((b3, bd, F.max_pool2d(x, 3, 2)), 1)


def inception_c(x, sd, n):
    b1 = basic(x, sd, f"{n}.branch1x1")
    b7 = basic(x, sd, f"{n}.branch7x7_1")
    b7 = basic(b7, sd, f"{n}.branch7x7_2", padding=(0, 3))
    b7 = basic(b7, sd, f"{n}.branch7x7_3", padding=(3, 0))
    bd = basic(x, sd, f"{n}.branch7x7dbl_1")
    bd = basic(bd, sd, f"{n}.branch7x7dbl_2", padding=(3, 0))
    bd = basic(bd, sd, f"{n}.branch7x7dbl_3", padding=(0, 3))
    bd = basic(bd, sd, f"{n}.branch7x7dbl_4", padding=(3, 0))
    bd = basic(bd, sd, f"{n}.branch7x7dbl_5", padding=(0, 3))
    bp = basic(_avg(x), sd, f"{n}.branch_pool")
    return torch.cat((b1, b7, bd, bp), 1)


def inception_d(x, sd, n):
    b3 = basic(basic(x, sd, f"{n}.branch3x3_1"), sd, f"{n}.branch3x3_2", stride=2)
    b7 = basic(x, sd, f"{n}.branch7x7x3_1")
    b7 = basic(b7, sd, f"{n}.branch7x7x3_2", padding=(0, 3))
    b7 = basic(b7, sd, f"{n}.branch7x7x3_3", padding=(3, 0))
    b7 = basic(b7, sd, f"{n}.branch7x7x3_4", stride=2)
    return torch.cat((b3, b7, F.max_pool2d(x, 3, 2)), 1)


def inception_e(x, sd, n, pool):
    b1 = basic(x, sd, f"{n}.branch1x1")
    b3 = basic(x, sd, f"{n}.branch3x3_1")
    b3 = torch.cat((basic(b3, sd, f"{n}.branch3x3_2a", padding=(0, 1)), basic(b3, sd, f"{n}.branch3x3_2b", padding=(1, 0))), 1)
    bd = basic(basic(x, sd, f"{n}.branch3x3dbl_1"), sd, f"{n}.branch3x3dbl_2", padding=1)
    bd = torch.cat((basic(bd, sd, f"{n}.branch3x3dbl_3a", padding=(0, 1)), basic(bd, sd, f"{n}.branch3x3dbl_3b", padding=(1, 0))), 1)
    pooled = _avg(x) if pool == "avg" else F.max_pool2d(x, 3, 1, 1)
    return torch.cat((b1, b3, bd, basic(pooled, sd, f"{n}.branch_pool")), 1)


# name -> function of (x, sd); Mixed_7c's branch pool is a max-pool (the FID variant)
BLOCKS = {
    "Mixed_5b": lambda x, sd: inception_a(x, sd, "Mixed_5b"), "Mixed_5c": lambda x, sd: inception_a(x, sd, "Mixed_5c"),
    "Mixed_5d": lambda x, sd: inception_a(x, sd, "Mixed_5d"), "Mixed_6a": lambda x, sd: inception_b(x, sd, "Mixed_6a"),
    "Mixed_6b": lambda x, sd: inception_c(x, sd, "Mixed_6b"), "Mixed_6c": lambda x, sd: inception_c(x, sd, "Mixed_6c"),
    "Mixed_6d": lambda x, sd: inception_c(x, sd, "Mixed_6d"), "Mixed_6e": lambda x, sd: inception_c(x, sd, "Mixed_6e"),
    "Mixed_7a": lambda x, sd: inception_d(x, sd, "Mixed_7a"),
    "Mixed_7b": lambda x, sd: inception_e(x, sd, "Mixed_7b", "avg"), "Mixed_7c": lambda x, sd: inception_e(x, sd, "Mixed_7c", "max"),
}
# the widths the issue's table states, and the spatial chain of a 299 x 299 input
BLOCK_WIDTHS = {"Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768,
                "Mixed_6e": 768, "Mixed_7a": 1280, "Mixed_7b": 2048, "Mixed_7c": 2048}
SPATIAL_CHAIN = (299, 149, 147, 147, 73, 73, 71, 35, 17, 8)


def stem(x, sd, sizes=None):
    note = (lambda t: sizes.append(t.shape[-1])) if sizes is not None else (lambda t: None)
    for name, kw in (("Conv2d_1a_3x3", dict(stride=2)), ("Conv2d_2a_3x3", {}), ("Conv2d_2b_3x3", dict(padding=1)), ("pool", None),
                     ("Conv2d_3b_1x1", {}), ("Conv2d_4a_3x3", {}), ("pool", None)):
        x = F.max_pool2d(x, 3, 2) if kw is None else basic(x, sd, name, **kw)
        note(x)
    return x


def trunk(x, sd, dtype=torch.float64):
    """network input [N, 3, 299, 299] -> pool features [N, 2048] in ``dtype``"""
    x = stem(x.to(dtype), sd)
    for fn in BLOCKS.values():
        x = fn(x, sd)
    return x.mean((2, 3))


def features(samples, images, sd, quantise=True, dtype=torch.float64):
    """[2 N, 2048] in ``dtype``: the fake frames' features, then the real ones'"""
    return trunk(input_stage(samples, images, quantise)[0], sd, dtype)


# ------------------------------------------------------------------------------------------------ statistics and distance
def statistics(f):
    """features [n, D] -> (mu, Sigma) float64 numpy, Sigma = np.cov(rowvar=False)"""
    a = f.double().numpy()
    if a.shape[0] < 2:
        raise ValueError("n < 2")
    return a.mean(0), np.cov(a, rowvar=False)


def frechet(mu1, s1, mu2, s2):
    """step 4, restated: sum sqrt(max(eig(A S2 A), 0)) with A = S1^(1/2) from eigh, negative eigenvalues clamped"""
    lam, q = np.linalg.eigh(s1)
    a = q @ np.diag(np.sqrt(lam.clip(min=0.0))) @ q.T
    m = a @ s2 @ a
    tr = np.sqrt(np.linalg.eigvalsh((m + m.T) / 2).clip(min=0.0)).sum()
    return float(((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2.0 * tr)


def frechet_zero_bound(s):
    """|FID(S, S)| bound: the exact value is 0 = 2 tr S - 2 sum l_i with l_i the eigenvalues of S.  eigh returns eigenvalues within
    c D v |S|_2 of those of a nearby matrix (backward stable, c a small constant: 8 here), twice (S, then A S A whose norm is |S|_2^2
    and whose square-rooted eigenvalues move by at most sqrt(delta) each), and two D x D products add D v |S|_2^2 each:
    |FID| <= 2 D sqrt(delta), delta = (8 D + 2 D) v |S|_2^2 ... taken with 16 D for slack."""
    D = s.shape[0]
    norm = float(np.linalg.norm(s, 2))
    return 2.0 * D * (16.0 * D * V) ** 0.5 * norm
