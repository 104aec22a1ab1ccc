"""LPIPS-Alex on the fp32 kernels of csrc/lpips.hip: the perceptual distance the reference reports next to OCR accuracy
(test.py:122-124, metrics.py:12-30: ``lpips.LPIPS(net='alex')`` between every saved fake frame and the real image it was made from).

Definition, for one pair (fake, real) of [3, H, W] frames:
  1. input: the 8-bit PNG values test.py:94,102,110-113 saves — fake q = trunc(s*255) for the [0, 1] sample s, real
     q = trunc(((x + 1)*0.5)*255) for the [-1, 1] image x, fp32 products in that order, clamped to [0, 255] — then lpips.im2tensor's
     t = q/127.5 - 1 and the scaling layer (t - shift)/scale.  ``quantise=False`` skips the trunc: LPIPS of the continuous frames.
  2. features: torchvision AlexNet ``features[0:12]``, a tap after each of the five ReLUs.
  3. distance: per tap and pixel u = f/(sqrt(sum_c f^2) + 1e-10), d = sum_c w_c (u0_c - u1_c)^2; LPIPS = sum over taps of the pixel mean.

PER IMAGE: every pair is measured on its own frame.  The reference concatenates a batch's frames along the width before saving
(test.py:95,104), so at its batch size 1 the two agree, and at larger batches the reference's number includes the seam pixels.

Fake and real run through the network as ONE batch of 2 N frames, so LPIPS(x, x) is exactly 0.0.  Everything is fp32 (a metric quoted
to three or four digits is not computed in bf16) and deterministic.  There is no fallback: without a gfx950 device the calls raise.

This file is lpips_alex.py, not lpips.py: the package's directory is first on sys.path (for the ``sgm`` mirror), and a top-level
``lpips`` here would shadow the real package that the reference's metrics.py imports.

State-dict names are those of the published packages AS WE KNOW THEM — neither ``lpips`` nor ``torchvision`` is available to this
project's tests, so ``KEY_TABLE`` below is the one place that states them and is unverified against the packages.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.nn as nn

from . import ops, packing, synth

# (slice, index in torchvision's ``features``, Cin, Cout, kernel, stride, padding); a 3x3 / 2 max-pool precedes convolutions 2 and 3
ALEX_CONVS = (("slice1", 0, 3, 64, 11, 4, 2), ("slice2", 3, 64, 192, 5, 1, 2), ("slice3", 6, 192, 384, 3, 1, 1),
              ("slice4", 8, 384, 256, 3, 1, 1), ("slice5", 10, 256, 256, 3, 1, 1))
POOL_BEFORE = (False, True, True, False, False)
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)

# our state-dict name -> the other names a checkpoint may use for the same tensor: torchvision's AlexNet for the backbone, the
# ``lins`` ModuleList that later releases of the lpips package register next to lin0 .. lin4
KEY_TABLE: Dict[str, Tuple[str, ...]] = {}
for _slice, _idx, *_ in ALEX_CONVS:
    for _leaf in ("weight", "bias"):
        KEY_TABLE[f"net.{_slice}.{_idx}.{_leaf}"] = (f"features.{_idx}.{_leaf}",)
for _k in range(5):
    KEY_TABLE[f"lin{_k}.model.1.weight"] = (f"lins.{_k}.model.1.weight",)
KEY_TABLE["scaling_layer.shift"] = ()
KEY_TABLE["scaling_layer.scale"] = ()


def map_sizes(H: int, W: int) -> List[Tuple[int, int]]:
    """the five tap sizes of an H x W frame (host arithmetic); ValueError when a tap would have no pixel"""
    sizes, h, w = [], int(H), int(W)
    for (_, _, _, _, ks, stride, pad), pool in zip(ALEX_CONVS, POOL_BEFORE):
        if pool:
            h, w = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if h >= 3 and w >= 3 else (0, 0)
        if h >= 1 and w >= 1:
            h, w = packing.conv_out_hw(h, w, ks, stride, (pad, pad))
        if h < 1 or w < 1:
            raise ValueError(f"LPIPS: a {H} x {W} frame is too small: tap {len(sizes) + 1} of the AlexNet features would have no pixel")
        sizes.append((h, w))
    return sizes


class _Weights(nn.Module):
    def __init__(self, shape, bias: bool):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(shape), requires_grad=False)
        if bias:
            self.bias = nn.Parameter(torch.zeros((shape[0],)), requires_grad=False)


class LPIPS(nn.Module):
    """``LPIPS(net="alex")``; ``forward(samples, images, quantise=True) -> [N]`` fp32 on the device.  Built with zero weights:
    ``load_weights`` (the published alex.pth + an AlexNet checkpoint, or one lpips state dict) or ``fill_synthetic_`` fills them."""

    def __init__(self, net: str = "alex", ckpt_path=None):
        super().__init__()
        if net != "alex":
            raise NotImplementedError(f"LPIPS(net={net!r}): only the AlexNet variant the reference measures with is built")
        self.net = nn.Module()
        for name, idx, cin, cout, ks, _, _ in ALEX_CONVS:
            sl = nn.Module()
            sl.add_module(str(idx), _Weights((cout, cin, ks, ks), bias=True))
            self.net.add_module(name, sl)
        for k, (_, _, _, cout, *_rest) in enumerate(ALEX_CONVS):
            lin = nn.Module()
            lin.model = nn.Module()
            lin.model.add_module("1", _Weights((1, cout, 1, 1), bias=False))
            self.add_module(f"lin{k}", lin)
        self.scaling_layer = nn.Module()
        self.scaling_layer.register_buffer("shift", torch.tensor(SHIFT).reshape(1, 3, 1, 1))
        self.scaling_layer.register_buffer("scale", torch.tensor(SCALE).reshape(1, 3, 1, 1))
        if ckpt_path is not None:
            paths = [ckpt_path] if isinstance(ckpt_path, str) else list(ckpt_path)
            self.load_weights(*[torch.load(p, map_location="cpu") for p in paths])

    map_sizes = staticmethod(map_sizes)

    # ---- weights
    def load_weights(self, *state_dicts) -> None:
        """fill every tensor from the given state dicts (later ones win), each name looked up under ours and under its KEY_TABLE
        aliases; KeyError names what no dict holds (the scaling layer's constants may be absent)"""
        merged = {}
        for sd in state_dicts:
            merged.update(sd)
        own = self.state_dict()
        assert set(own) == set(KEY_TABLE)
        new, missing = {}, []
        for name, aliases in KEY_TABLE.items():
            hit = next((merged[n] for n in (name, *aliases) if n in merged), None)
            if hit is None:
                if name.startswith("scaling_layer."):
                    new[name] = own[name]
                else:
                    missing.append(name)
                continue
            if tuple(hit.shape) != tuple(own[name].shape):
                raise ValueError(f"LPIPS: {name} has shape {tuple(hit.shape)} in the checkpoint, {tuple(own[name].shape)} here")
            new[name] = hit
        if missing:
            raise KeyError(f"LPIPS: no checkpoint tensor for {missing}")
        self.load_state_dict(new, strict=True)

    def fill_synthetic_(self, prefix: str = "lpips.") -> "LPIPS":
        """synth.py's name-and-shape recipe; the lin weights made non-negative (as the trained ones are)"""
        sd = {}
        for name, t in self.state_dict().items():
            if name.startswith("scaling_layer."):
                continue
            v = synth.synthetic_tensor(prefix + name, tuple(t.shape))
            sd[name] = v.abs() if name.startswith("lin") else v
        self.load_weights(sd)
        return self

    def _sources(self):
        return [*self.parameters(), *self.buffers()]

    def _pack(self):
        convs = []
        for name, idx, _, cout, ks, stride, pad in ALEX_CONVS:
            m = getattr(getattr(self.net, name), str(idx))
            convs.append((packing.pack_conv_f32(m.weight), m.bias.float().contiguous(), cout, ks, stride, pad))
        lins = [getattr(self, f"lin{k}").model.get_submodule("1").weight.float().reshape(-1).contiguous() for k in range(5)]
        return convs, lins, self.scaling_layer.shift.float().reshape(-1).contiguous(), self.scaling_layer.scale.float().reshape(-1).contiguous()

    def packed(self):
        """the kernels' layouts, in the per-module cache (rebuilt when a weight changes pointer, version or device)"""
        from sgm.modules import hipnn
        return hipnn.layout(self, "lpips_f32", self._pack)

    # ---- the measurement
    @torch.no_grad()
    def forward(self, samples: torch.Tensor, images: torch.Tensor, quantise: bool = True) -> torch.Tensor:
        """samples [N, 3, H, W] in [0, 1] (what ``predict`` returns), images [N, 3, H, W] in [-1, 1] (batch["image"]) -> LPIPS of every
        pair, fp32 [N] on the device, no synchronisation.  ValueError before any launch when the shapes differ or the frame is too
        small for the five taps.  Any H, W that leaves every tap a pixel works."""
        if samples.dim() != 4 or samples.shape[1] != 3 or tuple(samples.shape) != tuple(images.shape):
            raise ValueError(f"LPIPS: samples {tuple(samples.shape)} and images {tuple(images.shape)} must both be [N, 3, H, W]")
        N, _, H, W = samples.shape
        if N < 1:
            raise ValueError("LPIPS: no pair")
        sizes = map_sizes(H, W)
        convs, lins, shift, scale = self.packed()
        dev = shift.device
        f = ops.lpips_input(samples.to(dev, torch.float32).contiguous(), images.to(dev, torch.float32).contiguous(), shift, scale, quantise)
        out = torch.empty((N,), dtype=torch.float32, device=dev)
        scratch = torch.empty((max(ops.lpips_layer_scratch_bytes(N, h * w) for h, w in sizes),), dtype=torch.uint8, device=dev)
        for k, (w, b, cout, ks, stride, pad) in enumerate(convs):
            if POOL_BEFORE[k]:
                f = ops.maxpool3s2_f32(f)
            f = ops.conv2d_f32(f, w, b, cout, ks, stride, pad, relu=True)
            assert tuple(f.shape[1:3]) == sizes[k]
            ops.lpips_layer(f, lins[k], out, accumulate=k > 0, scratch=scratch)
        return out
