"""float64 restatement of LPIPS-Alex as udifftext_amd/lpips_alex.py defines it, in plain torch on NCHW tensors, with the
per-element bounds the kernels of csrc/lpips.hip are held to.  u = 2^-24 is the unit roundoff of fp32 below.

Convolution (``conv``).  The kernel adds K fp32 products in one chain and then the bias: K + 1 rounded additions and K rounded
products, so for ANY summation order  |got - ref| <= (K + 2) u (sum |w||x| + |b|) (1 + 2^-10)  per output element — the last factor
covers the second-order terms, (1 + u)^(K + 2) - 1 <= (K + 2) u (1 + 2^-10) for K <= 2^13.  sum |w||x| is the float64 convolution of
|x| with |w|, so every output has its own bound: a tap that wrapped into the neighbouring row or image would show up at an output
whose own window is small.  ReLU is 1-Lipschitz and does not enlarge it.

Layer distance (``layer``).  Per pixel and image the kernel computes s = sum_c f_c^2 (C products, C - 1 additions in some order:
relative error <= (C + 1) u), sqrt (halves it, one rounding), + 1e-10 (one rounding, and fp32(1e-10) is within u of 1e-10), the division
(one rounding):  |u_c' - u_c| <= ((C + 1)/2 + 4) u |u_c| <= (C + 6) u |u_c|  for C >= 3.  The difference u0_c - u1_c adds one rounding,
u |u0_c - u1_c| <= u (|u0_c| + |u1_c|), so the computed difference is off by at most
    e_c = (C + 7) u (|u0_c| + |u1_c|).
Then (diff + e)^2 - diff^2 <= 2 |diff| e + e^2 per channel, weighted by |w_c|; the two products, the C - 1 channel additions, the
P - 1 pixel additions (any order) and the division by P are at most C + P + 2 more roundings of non-negative terms (their sum is
d_abs, d with |w|).  So
    |got - d| <= [ mean_p sum_c |w_c| (2 |u0_c - u1_c| e_c + e_c^2) + (C + P + 4) u d_abs ] (1 + 2^-10)
and, in the accumulating form, one more rounding of the sum: + u |previous + d|.

Whole network: no simple bound exists (the taps' errors pass through four more convolutions and a normalisation); tests measure the
distance of this restatement run in fp32 on the CPU from its float64 run and allow the GPU 8 times that
(tests/test_lpips_gpu.py).
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
# (state-dict prefix, Cin, Cout, kernel, stride, padding, pooled before) — written out here, not imported from the module under test
CONVS = (("net.slice1.0", 3, 64, 11, 4, 2, False), ("net.slice2.3", 64, 192, 5, 1, 2, True), ("net.slice3.6", 192, 384, 3, 1, 1, True),
         ("net.slice4.8", 384, 256, 3, 1, 1, False), ("net.slice5.10", 256, 256, 3, 1, 1, False))
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)


def input_stage(samples: torch.Tensor, images: torch.Tensor, quantise: bool = True, shift=SHIFT, scale=SCALE) -> torch.Tensor:
    """fp32 [2 N, 3, H, W], bit for bit what the kernel states: every fp32 operation on its own (torch's CPU elementwise operations
    do not contract), v / 127.5 - 1 in float64 and rounded once"""
    s, x = samples.float(), images.float()
    v = torch.cat((s * 255.0, ((x + 1.0) * 0.5) * 255.0), 0)
    assert v.dtype == torch.float32
    v = v.clamp(0.0, 255.0)
    if quantise:
        v = v.trunc()
    t = (v.double() / 127.5 - 1.0).float()
    sh = torch.tensor(shift, dtype=torch.float32).reshape(1, 3, 1, 1)
    sc = torch.tensor(scale, dtype=torch.float32).reshape(1, 3, 1, 1)
    return (t - sh) / sc


def conv(x, w, b, stride, pad, relu):
    """x [N, Cin, H, W], w [Cout, Cin, k, k], b [Cout] or None -> (float64 reference, float64 bound per element)"""
    xd, wd = x.double(), w.double()
    bd = None if b is None else b.double()
    ref = F.conv2d(xd, wd, bd, stride=stride, padding=pad)
    mag = F.conv2d(xd.abs(), wd.abs(), None if bd is None else bd.abs(), stride=stride, padding=pad)
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return (ref.clamp_min(0.0) if relu else ref), (K + 2) * U * mag * SLACK


def pool(x):
    return F.max_pool2d(x, 3, 2)


def layer(f, w, prev=None):
    """f [2 N, C, h, w] (pair n = frames n and N + n), w [C], prev [N] or None -> (float64 [N] = prev + mean_p d, its bound [N])"""
    fd, wd = f.double(), w.double().reshape(1, -1, 1, 1)
    N, C, P = f.shape[0] // 2, f.shape[1], f.shape[2] * f.shape[3]
    un = fd / (fd.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    u0, u1 = un[:N], un[N:]
    diff = (u0 - u1).abs()
    d = (wd * diff.pow(2)).sum(1).mean((1, 2))
    d_abs = (wd.abs() * diff.pow(2)).sum(1).mean((1, 2))
    e = (C + 7) * U * (u0.abs() + u1.abs())
    bound = ((wd.abs() * (2.0 * diff * e + e * e)).sum(1).mean((1, 2)) + (C + P + 4) * U * d_abs) * SLACK
    if prev is not None:
        d = prev.double() + d
        bound = bound + U * d.abs() * SLACK
    return d, bound


def features(x, sd, dtype=torch.float64):
    """the five taps (after each ReLU) of AlexNet features[0:12] of x [n, 3, H, W], in ``dtype``"""
    taps, f = [], x.to(dtype)
    for name, _, _, _, stride, pad, pooled in CONVS:
        if pooled:
            f = pool(f)
        f = F.relu(F.conv2d(f, sd[name + ".weight"].to(dtype), sd[name + ".bias"].to(dtype), stride=stride, padding=pad))
        taps.append(f)
    return taps


def lpips(samples, images, sd, quantise=True, dtype=torch.float64):
    """LPIPS of every (sample, image) pair -> [N] in ``dtype``; fake and real go through the network as one batch"""
    shift = tuple(sd["scaling_layer.shift"].reshape(-1).tolist()) if "scaling_layer.shift" in sd else SHIFT
    scale = tuple(sd["scaling_layer.scale"].reshape(-1).tolist()) if "scaling_layer.scale" in sd else SCALE
    x = input_stage(samples, images, quantise, shift, scale)
    N = samples.shape[0]
    total = torch.zeros((N,), dtype=dtype)
    for k, f in enumerate(features(x, sd, dtype)):
        w = sd[f"lin{k}.model.1.weight"].to(dtype).reshape(1, -1, 1, 1)
        un = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        total = total + (w * (un[:N] - un[N:]).pow(2)).sum(1).mean((1, 2))
    return total
