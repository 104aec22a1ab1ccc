"""Memory footprint of udt_crop_resize_aa_f32 (crop + antialiased bicubic resize + normalise of every box in one launch), as cases of
tests/test_footprint_gpu.py's table.

The cases are appended to that module's ``CASES`` when this module is imported, as tests/test_aae_rows_footprint_gpu.py does it, and
run here through the table's own ``_run_case``: img and boxes guarded inputs inside poisoned arenas (a tap that leaves the image reads a
NaN), out a guarded output, against compact buffers, bit-equal, no guard byte touched, no output element left unwritten.
"""
import pytest
import torch

import test_footprint_gpu as table
from test_footprint_gpu import F32, _chk, _mods, _p, _rand, env  # noqa: F401  (env: the table's fixture)

pytestmark = pytest.mark.gpu

NAME = "udt_crop_resize_aa_f32"
OWN = []


def case(name, covers):
    def deco(fn):
        if name not in [c[0] for c in table.CASES]:           # (a re-import must not register twice)
            table.case(name, covers)(fn)
        OWN.append((name, fn))
        return fn
    return deco


def _crop_resize(B, Cc, H, W, boxes, out_hw, seed):
    def fn(b):
        O, L, lib, P = _mods()
        img = b.inp(_rand((B, Cc, H, W), seed), name="img")
        bx = b.inp(torch.tensor(boxes, dtype=torch.int32), name="boxes")
        out = b.out((len(boxes), Cc) + tuple(out_hw), F32, name="out")
        assert img.is_contiguous() and bx.is_contiguous() and out.is_contiguous()
        _chk(lib.udt_crop_resize_aa_f32(_p(img), _p(bx), _p(out), B, Cc, H, W, len(boxes), out_hw[0], out_hw[1], 2.0, -1.0, O._stream()),
             NAME)
        assert not bool(torch.isnan(out).any()), "a tap read the poison around the image"
        return {"out": out}
    return fn


# the four corners of the first and the last image (down-scaling, up-scaling, both), and the whole of one
case("crop_resize_aa 5 boxes at the corners of (2,3,70,131) images -> 32x128", [NAME])(
    _crop_resize(2, 3, 70, 131, [[0, 0, 33, 0, 129], [0, 0, 7, 120, 131], [1, 60, 70, 0, 5], [1, 38, 70, 2, 131], [1, 0, 70, 0, 131]],
                 (32, 128), 811))
case("crop_resize_aa a 1x1 box of a (1,1,1,1) image -> 32x128", [NAME])(_crop_resize(1, 1, 1, 1, [[0, 0, 1, 0, 1]], (32, 128), 812))


@pytest.mark.parametrize("idx", range(len(OWN)), ids=[c[0] for c in OWN])
def test_crop_resize_footprint(env, idx):
    name, fn = OWN[idx]
    table._run_case(name, fn, env.dev)
