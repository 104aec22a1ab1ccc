"""Torch restatement of the t_attn map consumers on h x w maps (tokens row-major, n = y * w + x).

The reference's get_min_local_loss / get_local_loss (loss.py:192-286) reshape the maps to ``size x size`` with
``size = int(n ** 0.5)`` and raise for h != w, so there is nothing of the reference to record for rectangular maps.  This file is the
reference's formula with ``size, size`` replaced by ``h, w``: head mean, reshape to (h, w), depth-wise 3x3 blur, nearest mask
(F.interpolate(..., size=(h, w))), max over the pixels, ``+ 1 - seg``, min over the tokens, negate, mean over the scored layers; and
the ``seg`` form of get_local_loss.  For h == w it equals oracle.sampling.min_local_loss / oracle.training.local_loss (pinned to the
reference by tests/test_oracle_golden.py) — tests/test_rect_cpu.py holds it to that.

A layer is scored when min(h, w) >= min_attn_size ("Rectangular images").  Sample i of the maps is scored against
mask[i % B] / seg_mask[i % B] (tiled candidates; the per-sample rule for B > 1).
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn.functional as F


def scores_map(hw, min_attn_size: int = 16) -> bool:
    return min(int(hw[0]), int(hw[1])) >= min_attn_size


def blurred_maps(item: dict, seg_l: int, g_kernel: torch.Tensor) -> torch.Tensor:
    """[b, seg_l, h * w]: head mean of the first seg_l tokens' maps, blurred 3x3 per token"""
    heads, (h, w), am = item["heads"], item["hw"], item["attn_map"]
    bh, n, l = am.shape
    assert n == h * w
    am = am.reshape(-1, heads, n, l)[..., :seg_l].permute(0, 1, 3, 2).mean(dim=1)            # b, l, n
    return F.conv2d(am.reshape(-1, seg_l, h, w), g_kernel[:seg_l], padding=1, groups=seg_l).reshape(-1, seg_l, n)


def min_local_loss(attn_maps: List[dict], mask: torch.Tensor, seg_mask: torch.Tensor, g_kernel: torch.Tensor,
                   min_attn_size: int = 16) -> torch.Tensor:
    """maps [b * heads, n, L] with b a multiple of B = mask.shape[0]; mask [B, 1, Hm, Wm]; seg_mask [B, seg_l] -> fp32 [b]"""
    loss, count = 0, 0
    B, seg_l = mask.shape[0], seg_mask.shape[1]
    for item in attn_maps:
        if not item["name"].endswith("t_attn") or not scores_map(item["hw"], min_attn_size):
            continue
        h, w = item["hw"]
        am = blurred_maps(item, seg_l, g_kernel)
        reps = am.shape[0] // B
        mm = F.interpolate(mask, (h, w)).tile((reps, seg_l, 1, 1)).reshape(-1, seg_l, h * w)
        p = (mm * am).max(dim=-1)[0] + (1 - seg_mask.tile((reps, 1)))
        loss = loss + (-p.min(dim=-1)[0])
        count += 1
    return loss / count


def local_loss(attn_maps: List[dict], seg: torch.Tensor, seg_mask: torch.Tensor, g_kernel: torch.Tensor,
               min_attn_size: int = 16) -> torch.Tensor:
    """the training step's get_local_loss: seg [B, seg_l, Hs, Ws] character segment maps -> fp32 [B]"""
    loss, count = 0, 0
    seg_l = seg_mask.shape[1]
    for item in attn_maps:
        if not item["name"].endswith("t_attn") or not scores_map(item["hw"], min_attn_size):
            continue
        h, w = item["hw"]
        am = blurred_maps(item, seg_l, g_kernel)
        sm = F.interpolate(seg, (h, w)).reshape(-1, seg_l, h * w)
        p = (sm * am).max(dim=-1)[0] * seg_mask
        nn_ = ((1 - sm) * am).max(dim=-1)[0] * seg_mask
        loss = loss + (nn_.sum(dim=-1) / seg_mask.sum(dim=-1) - p.sum(dim=-1) / seg_mask.sum(dim=-1))
        count += 1
    return loss / count
