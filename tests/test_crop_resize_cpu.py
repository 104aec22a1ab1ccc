"""The float64 restatement of udt_crop_resize_aa_f32 (tests/crop_resize_ref.py) against ATen, and the entry point's registration."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import crop_resize_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))

BOXES = [(1, 1), (5, 5), (7, 300), (200, 9), (31, 127), (32, 128), (33, 129), (64, 64), (128, 384), (512, 768)]
OUT = (32, 128)


def _crop(h, w, seed=0):
    return torch.rand((3, h, w), generator=torch.Generator().manual_seed(1000 * h + w + seed), dtype=torch.float64)


@pytest.mark.parametrize("h,w", BOXES)
def test_helper_matches_aten_float64(h, w):
    crop = _crop(h, w)
    want = F.interpolate(crop[None], size=OUT, mode="bicubic", antialias=True, align_corners=False)[0]
    got, info = R.resize(crop, OUT)
    err = float((got - want).abs().max())
    print(f"{h}x{w}: max |helper - ATen float64| {err:.3e}; K {info['Ky']}, {info['Kx']}; S {info['Sy']:.4f}, {info['Sx']:.4f}")
    assert err <= 1e-12


def test_helper_matches_the_oracle_transform_in_float32():
    """(helper - 0.5) / 0.5 against oracle.parseq.predictor_transform (ATen in fp32, which stays within 4.5e-7 of float64)"""
    from oracle import parseq as OP
    crops = [_crop(h, w).float() for h, w in BOXES]
    want = OP.predictor_transform(crops).double()
    got = torch.stack([(R.resize(c, OUT)[0] - 0.5) / 0.5 for c in crops])
    err = float((got - want).abs().max())
    print(f"max |helper - oracle fp32 transform| {err:.3e}")
    assert err <= 2e-6


def test_same_size_tables_are_the_identity():
    for n in OUT:
        Wt, K, S = R.tables(n, n)
        assert torch.equal(Wt, torch.eye(n, dtype=torch.float64)) and S == 1.0 and K <= 4


def test_crop_resize_matches_slicing_and_affine():
    img = torch.rand((2, 3, 20, 40), generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    boxes = [[1, 2, 17, 3, 39], [0, 0, 20, 0, 40]]
    got, bound = R.crop_resize(img, boxes, (8, 16), mul=2.0, add=-1.0)
    for n, (i, t, b, l, r) in enumerate(boxes):
        want = F.interpolate(img[i:i + 1, :, t:b, l:r], size=(8, 16), mode="bicubic", antialias=True, align_corners=False)[0]
        assert float((got[n] - (2.0 * want - 1.0)).abs().max()) <= 1e-12
    assert bound.shape == (2, 1, 1, 1) and bool((bound > 0).all())


def test_crop_resize_is_declared_typed_and_in_the_footprint_table():
    import test_crop_resize_footprint_gpu  # noqa: F401  (appends its cases to the table)
    import test_footprint_gpu as table
    from udifftext_amd import lib, ops
    name = "udt_crop_resize_aa_f32"
    root = os.path.dirname(HERE)
    text = open(os.path.join(root, "include", "udt_kernels.h")).read()
    assert name in text.split("#ifndef UDT_KERNELS_H")[0], "the header's overview comment does not list the entry point"
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", code)
    assert m, f"{name} is not declared in include/udt_kernels.h"
    assert len(m.group(1).split(",")) == 13 == len(lib.SYMBOLS[name][1])
    covering = [n for n, _, covers in table.CASES if name in covers]
    assert len(covering) >= 2 and name not in table.EXEMPT
    assert callable(ops.crop_resize_aa)
    from udifftext_amd.build import SOURCES
    assert "resample.hip" in SOURCES
