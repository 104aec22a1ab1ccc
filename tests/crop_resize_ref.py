"""float64 restatement of udt_crop_resize_aa_f32 (include/udt_kernels.h): F.interpolate(crop[None], size, mode="bicubic",
antialias=True, align_corners=False) as two dense weight tables, out = Wy . crop . Wx^T.

Along an axis of n_in input and n_out output samples, output i uses scale = n_in / n_out, support = 2 scale and inv = 1 / scale
when scale >= 1 (else 2 and 1), centre = scale (i + 0.5), the taps lo = max(0, int(centre - support + 0.5)) <= j <
hi = min(n_in, int(centre + support + 0.5)) and the weights k((j - centre + 0.5) inv) divided by their sum; k is the Keys cubic
with a = -0.5 (ATen's value when antialiasing, not the -0.75 of plain bicubic).  Python floats are IEEE doubles throughout.
tests/test_crop_resize_cpu.py pins this against ATen's float64 result.
"""
import torch

A = -0.5


def cubic(x: float) -> float:
    x = abs(x)
    if x < 1.0:
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    if x < 2.0:
        return A * (((x - 5.0) * x + 8.0) * x - 4.0)
    return 0.0


def axis_table(n_in: int, n_out: int):
    """-> (W float64 [n_out, n_in], K: the largest tap count of a row, S: the largest row sum of |w|)"""
    scale = n_in / n_out
    support = 2.0 * scale if scale >= 1.0 else 2.0
    inv = 1.0 / scale if scale >= 1.0 else 1.0
    Wt = torch.zeros((n_out, n_in), dtype=torch.float64)
    K = 0
    for i in range(n_out):
        centre = scale * (i + 0.5)
        lo = max(0, int(centre - support + 0.5))
        hi = min(n_in, int(centre + support + 0.5))
        w = [cubic((j - centre + 0.5) * inv) for j in range(lo, hi)]
        total = sum(w)
        Wt[i, lo:hi] = torch.tensor(w, dtype=torch.float64) / total
        K = max(K, hi - lo)
    return Wt, K, float(Wt.abs().sum(1).max())


_TABLES: dict = {}


def tables(n_in: int, n_out: int):
    key = (n_in, n_out)
    if key not in _TABLES:
        _TABLES[key] = axis_table(n_in, n_out)
    return _TABLES[key]


def resize(crop: torch.Tensor, out_hw):
    """crop [..., h, w] -> (float64 [..., oh, ow], info): info = {"Ky", "Kx", "Sy", "Sx"} of the two axes"""
    oh, ow = out_hw
    Wy, Ky, Sy = tables(crop.shape[-2], oh)
    Wx, Kx, Sx = tables(crop.shape[-1], ow)
    out = Wy @ crop.double() @ Wx.T
    return out, {"Ky": Ky, "Kx": Kx, "Sy": Sy, "Sx": Sx}


def crop_resize(img: torch.Tensor, boxes, out_hw, mul: float = 1.0, add: float = 0.0):
    """img [B, C, H, W], boxes [N, 5] (image index, top, bottom, left, right) -> (float64 [N, C, oh, ow], bound float64 [N, 1, 1, 1]):
    the kernel's stated bound per output element of box n,
        |got - ref| <= (Ky + Kx + 16) 2^-23 Sy Sx max|box| |mul|
    (fp32 accumulation of K products in any order costs at most about K 2^-24 relative to sum |w x| per pass; the additive 16 covers
    the fp32 rounding and normalisation of the weights; a tap that flips in or out at an exact support boundary carries k(+-2) = 0)"""
    outs, bounds = [], []
    for i, t, b, l, r in torch.as_tensor(boxes).reshape(-1, 5).tolist():
        crop = img[i, :, t:b, l:r]
        o, nf = resize(crop, out_hw)
        outs.append(mul * o + add)
        bounds.append((nf["Ky"] + nf["Kx"] + 16) * 2.0 ** -23 * nf["Sy"] * nf["Sx"] * float(crop.abs().max()) * abs(mul))
    return torch.stack(outs), torch.tensor(bounds, dtype=torch.float64).reshape(-1, 1, 1, 1)
