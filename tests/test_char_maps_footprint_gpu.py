"""Memory footprint of the two character-map kernels — udt_tattn_fused_maps (the fused text attention that also writes the head mean of
its probabilities) and udt_resize_bilinear_f32 — as cases of tests/test_footprint_gpu.py's table.

The cases are appended to that module's ``CASES`` when this module is imported, as tests/test_crop_resize_footprint_gpu.py does it, and
run here through the table's own ``_run_case``: every input guarded inside a poisoned arena, every output guarded and pre-filled with the
sentinel, against compact buffers, bit-equal, no guard byte touched, no output element left unwritten.  The ``maps`` buffer has EXACTLY
[B - map_from, L, n_tok] elements between its guards: a plane for a sample below map_from, or for one of the 16 - L padded score columns
of a head, would land in a guard.
"""
import math

import pytest
import torch

import test_footprint_gpu as table
from test_footprint_gpu import BF16, F32, I32, U8, _chk, _mods, _p, _rand, env  # noqa: F401  (env: the table's fixture)

pytestmark = pytest.mark.gpu

MAPS = "udt_tattn_fused_maps"
RESIZE = "udt_resize_bilinear_f32"
OWN = []


def case(name, covers):
    def deco(fn):
        if name not in [c[0] for c in table.CASES]:           # (a re-import must not register twice)
            table.case(name, covers)(fn)
        OWN.append((name, fn))
        return fn
    return deco


def _maps_case(heads, q8, Lc, map_from, accumulate):
    def fn(b):
        O, L, lib, P = _mods()
        B, n_tok, zero = 3, 64, 1
        Cc = heads * 64
        hp = lib.udt_tattn_hp(heads)
        x = b.inp(_rand((B, n_tok, Cc), 81, 1.5, 0.3).bfloat16(), name="x")
        kv = b.inp(_rand((B, Lc, 2 * Cc), 82).bfloat16(), name="k|v")
        wq = b.inp(P.pack_linear(_rand((Cc, Cc), 83, 1 / math.sqrt(Cc))), name="wq")
        wo = b.inp(P.pack_linear(_rand((Cc, Cc), 84, 1 / math.sqrt(Cc))), name="wo")
        gamma, beta = b.inp(_rand((Cc,), 85, 0.2, 1.0), name="gamma"), b.inp(_rand((Cc,), 86, 0.2), name="beta")
        bias = b.inp(_rand((Cc,), 87, 0.3), name="bias")
        tabs = O.TattnTables(b.out((B, hp, Cc), BF16, name="A'"), b.out((B, hp, 2), F32, name="sc"), b.out((B, Cc, hp), BF16, name="BmT"))
        O.tattn_prepare(kv, wq, wo, gamma, beta, heads, 0.125, out=tabs)
        out = b.out((B, n_tok, Cc), BF16)
        shape = (B - map_from, Lc, n_tok)
        maps = b.inout(_rand(shape, 88), name="maps") if accumulate else b.out(shape, F32, name="maps")
        assert maps.is_contiguous()
        res = {"out": out, "maps": maps, "~A'": tabs.A, "~sc": tabs.sc, "~BmT": tabs.BmT}
        extra = (None, None, None)
        if q8:
            parts = lib.udt_tattn_rowstat_parts(B, n_tok, Cc)
            assert parts > 0
            M = B * n_tok
            q8o, q8s = b.out((M, Cc), U8, name="q8_out"), b.out((Cc // 128, M), I32, name="q8_scale")
            rs = b.out((parts, M, 2), F32, name="rowstat_out")
            extra = (_p(q8o), _p(q8s), _p(rs))
            res.update({"q8": q8o, "q8_scale": q8s, "rowstat": rs})
        _chk(lib.udt_tattn_fused_maps(_p(x), _p(out), _p(tabs.A), _p(tabs.sc), _p(tabs.BmT), _p(bias), B, n_tok, Cc, heads, zero, 1e-5,
                                      _p(maps), Lc, map_from, 0.5, int(accumulate), *extra, O._stream()), MAPS)
        assert not bool(torch.isnan(maps).any()), "a map read something that is not a probability"
        return res
    return fn


case("tattn_fused_maps heads 5 n_tok 64 B3 zero 1 map_from 2 L 5: maps exactly [1, 5, 64]", ["udt_tattn_prepare", MAPS])(
    _maps_case(5, False, 5, 2, False))
case("tattn_fused_maps heads 20 L 12 map_from 1, accumulate into maps [2, 12, 64]", ["udt_tattn_prepare", MAPS])(
    _maps_case(20, False, 12, 1, True))
case("tattn_fused_maps + MX8 twin C=640 L 2 map_from 1: four extra outputs guarded", ["udt_tattn_prepare", MAPS])(
    _maps_case(10, True, 2, 1, False))


def _resize_case(planes, hw, HW, seed):
    def fn(b):
        O, L, lib, P = _mods()
        x = b.inp(_rand((planes,) + hw, seed), name="in")
        out = b.out((planes,) + HW, F32, name="out")
        assert x.is_contiguous() and out.is_contiguous()
        _chk(lib.udt_resize_bilinear_f32(_p(x), _p(out), planes, hw[0], hw[1], HW[0], HW[1], O._stream()), RESIZE)
        assert not bool(torch.isnan(out).any()), "a tap read the poison around the planes"
        return {"out": out}
    return fn


case("resize_bilinear 3 planes 3x5 -> 7x4 (down and up, clamped edges)", [RESIZE])(_resize_case(3, (3, 5), (7, 4), 821))
case("resize_bilinear 2 planes 1x1 -> 5x5", [RESIZE])(_resize_case(2, (1, 1), (5, 5), 822))
case("resize_bilinear 5 planes 8x12 -> 64x96 (more than one workgroup)", [RESIZE])(_resize_case(5, (8, 12), (64, 96), 823))


@pytest.mark.parametrize("idx", range(len(OWN)), ids=[c[0] for c in OWN])
def test_char_maps_footprint(env, idx):
    name, fn = OWN[idx]
    table._run_case(name, fn, env.dev)
