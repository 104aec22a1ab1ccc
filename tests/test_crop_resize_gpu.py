"""udt_crop_resize_aa_f32 through the C ABI against the float64 restatement (tests/crop_resize_ref.py, pinned against ATen by
tests/test_crop_resize_cpu.py).

Bound, per output element of a box (derived, not measured; crop_resize_ref.crop_resize returns it):
    |got - ref| <= (Ky + Kx + 16) 2^-23 Sy Sx max|box| |mul|
K and S are the axes' tap counts and absolute row sums.  fp32 accumulation of K products in any order costs at most about K 2^-24
relative to sum |w x| per pass; the additive 16 covers the fp32 rounding and normalisation of the weights; a tap that flips in or out
at an exact support boundary carries weight k(+-2) = 0.  The shapes are the smallest at which each thing can go wrong: boxes smaller
and larger than the output on either axis, sizes one off the output's, more than one 64-row chunk, more than one 32 x 32 output tile and
partial tiles, several boxes and images per launch, boxes on every edge and corner."""
import pytest
import torch

import crop_resize_ref as R

pytestmark = pytest.mark.gpu

NAME = "udt_crop_resize_aa_f32"
# on (2, C, 96, 320) images: 1x1, 5x5, 7x300, 31x127, 33x129 — a corner pixel, the top-left corner, the bottom edge up to the right
# corner, the interior, the top-right corner
BOXES_A = [[0, 95, 96, 319, 320], [0, 0, 5, 0, 5], [1, 89, 96, 20, 320], [1, 10, 41, 100, 227], [0, 0, 33, 191, 320]]
# 32x128 top-left, 64x64 bottom-right, 32x128 bottom-left, 31x127 on the left edge, the whole image
BOXES_B = [[1, 0, 32, 0, 128], [0, 32, 96, 256, 320], [0, 64, 96, 0, 128], [1, 33, 64, 0, 127], [1, 0, 96, 0, 320]]
CASES = {
    "A 32x128": ((2, 3, 96, 320), BOXES_A, (32, 128)),
    "B 32x128": ((2, 3, 96, 320), BOXES_B, (32, 128)),
    "A 8x16": ((2, 3, 96, 320), BOXES_A, (8, 16)),
    "B 32x130": ((2, 3, 96, 320), BOXES_B, (32, 130)),
    "C=1 N=5": ((2, 1, 96, 320), BOXES_A, (32, 128)),
    "C=1 N=1 200x9": ((1, 1, 208, 16), [[0, 4, 204, 3, 12]], (32, 128)),
    "N=1 64x64": ((1, 3, 70, 70), [[0, 6, 70, 0, 64]], (32, 128)),
    "one box 128x384": ((1, 3, 130, 390), [[0, 1, 129, 3, 387]], (32, 128)),
    "one box 512x768": ((1, 3, 512, 768), [[0, 0, 512, 0, 768]], (32, 128)),
}


@pytest.fixture(scope="module")
def lib(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib as L
    so = L.load()
    assert so.udt_device_arch_ok() == 1
    return so


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _launch(lib, img, boxes, out_hw, mul=1.0, add=0.0):
    B, C, H, W = img.shape
    bx = torch.tensor(boxes, dtype=torch.int32, device=img.device)
    for i, t, b, l, r in boxes:                                   # (no test passes a box that lies outside its image)
        assert 0 <= i < B and 0 <= t < b <= H and 0 <= l < r <= W
    out = torch.full((len(boxes), C) + tuple(out_hw), float("nan"), dtype=torch.float32, device=img.device)
    assert img.is_contiguous() and img.dtype == torch.float32
    rc = lib.udt_crop_resize_aa_f32(img.data_ptr(), bx.data_ptr(), out.data_ptr(), B, C, H, W, len(boxes), out_hw[0], out_hw[1], mul, add,
                                    _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _check(name, got, img, boxes, out_hw, mul, add):
    ref, bound = R.crop_resize(img.cpu(), boxes, out_hw, mul, add)
    err = (got.double().cpu() - ref).abs()
    for n, bx in enumerate(boxes):
        print(f"{name} box {n} {bx[2] - bx[1]}x{bx[4] - bx[3]} -> {out_hw[0]}x{out_hw[1]}: max |err| {float(err[n].max()):.3e}, "
              f"bound {float(bound[n]):.3e}, ratio {float(err[n].max() / bound[n]):.3f}")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= bound).all()), name


@pytest.mark.parametrize("name", list(CASES))
def test_against_float64(lib, cuda, name):
    shape, boxes, out_hw = CASES[name]
    img = torch.randn(shape, generator=torch.Generator().manual_seed(len(name) + shape[2]))
    got = _launch(lib, img.to(cuda), boxes, out_hw, 2.0, -1.0)
    _check(name, got, img, boxes, out_hw, 2.0, -1.0)


def test_taps_clamp_at_the_box_not_at_the_image(lib, cuda):
    """every pixel outside the box is +-1e6: one escaped tap shows as an error of about 1e4; the result equals, bit for bit, the
    result on the cropped tensor as an image of its own"""
    g = torch.Generator().manual_seed(77)
    box = [0, 10, 43, 30, 159]                                    # 33 x 129, strictly inside
    img = (torch.randint(0, 2, (1, 3, 64, 200), generator=g).float() * 2.0 - 1.0) * 1e6
    crop = torch.rand((3, 33, 129), generator=g)
    img[0, :, 10:43, 30:159] = crop
    for out_hw in ((32, 128), (8, 16)):
        got = _launch(lib, img.to(cuda), [box], out_hw, 2.0, -1.0)
        alone = _launch(lib, crop[None].contiguous().to(cuda), [[0, 0, 33, 0, 129]], out_hw, 2.0, -1.0)
        assert torch.equal(got, alone)
        _check("inside +-1e6", got, img, [box], out_hw, 2.0, -1.0)


def test_same_size_is_bit_equal_to_the_box(lib, cuda):
    img = torch.randn((2, 3, 96, 320), generator=torch.Generator().manual_seed(9))
    boxes = [[1, 64, 96, 192, 320], [0, 5, 37, 7, 135]]
    got = _launch(lib, img.to(cuda), boxes, (32, 128), 1.0, 0.0).cpu()
    for n, (i, t, b, l, r) in enumerate(boxes):
        assert torch.equal(got[n], img[i, :, t:b, l:r])


def test_ops_wrapper(lib, cuda):
    from udifftext_amd import ops
    img = torch.rand((2, 3, 40, 64), generator=torch.Generator().manual_seed(4)).to(cuda)
    boxes = [[1, 3, 30, 2, 60], [0, 0, 40, 0, 64]]
    got = ops.crop_resize_aa(img, torch.tensor(boxes, dtype=torch.int32, device=cuda), (32, 128), mul=2.0, add=-1.0)
    assert got.shape == (2, 3, 32, 128) and got.dtype == torch.float32
    assert torch.equal(got, _launch(lib, img, boxes, (32, 128), 2.0, -1.0))


def test_error_returns_launch_nothing(lib, cuda):
    from udifftext_amd import lib as L
    img = torch.rand((1, 3, 8, 8)).to(cuda)
    bx = torch.tensor([[0, 0, 8, 0, 8]], dtype=torch.int32, device=cuda)
    out = torch.full((1, 3, 32, 128), 7.0, device=cuda)
    p = (img.data_ptr(), bx.data_ptr(), out.data_ptr())
    dims = dict(B=1, C=3, H=8, W=8, N=1, out_h=32, out_w=128)

    def call(ptrs, **kw):
        d = dict(dims, **kw)
        return lib.udt_crop_resize_aa_f32(*ptrs, d["B"], d["C"], d["H"], d["W"], d["N"], d["out_h"], d["out_w"], 1.0, 0.0, _stream())
    for k in range(3):
        assert call(tuple(None if j == k else v for j, v in enumerate(p))) == -2          # UDT_ERR_BAD_ARG
    for key in dims:
        for v in (0, -1):
            assert call(p, **{key: v}) == -1, key                                           # UDT_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(ValueError):
        L.check(call(p, N=0), NAME)
    assert call(p) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7.0).any())
