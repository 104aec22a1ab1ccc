"""Memory footprint of the OCR-loss entry points (udt_mattn_bwd, udt_gelu_fwd / _bwd, udt_ocr_ce_f32, udt_crop_resize_aa_bwd_f32), one
ragged shape each, as further cases of the table of tests/test_footprint_gpu.py: they are registered through that module's own ``case``
decorator, as tests/test_crop_resize_footprint_gpu.py does it (so tests/test_footprint_cpu.py's "every entry point of the header has a case" sees them once this module is imported — the
collection of the suite does that) and run through its ``_run_case``: once on guarded / poisoned buffers, once on compact ones,

  * payloads bit-equal between the two layouts: a poisoned ld gap or guard that reached a result would have made it NaN;
  * no guard and no ld gap byte touched;
  * no output element left unwritten — for d_img that is the contract "every element is written exactly once, the caller clears
    nothing", also for a box table that breaks the one-box-per-image precondition.

None of the new entry points takes a scratch buffer or a workspace, so ``exact_scratch`` has nothing to hold here.
"""
import pytest
import torch

import test_footprint_gpu as T
from test_footprint_gpu import BF16, F32, I32, U8, _chk, _mods, _p, _rand, env  # noqa: F401  (env: the table's fixture)

pytestmark = pytest.mark.gpu

CASES = []                                                  # (name, fn, covered entry points): this module's own


def case(name, covers):
    def deco(fn):
        if name not in [c[0] for c in T.CASES]:             # (a re-import must not register twice)
            T.case(name, covers)(fn)
        CASES.append((name, fn, tuple(covers)))
        return fn
    return deco


def _mattn_bwd_case(b, masks, want_dq):
    O, L, lib, P = _mods()
    B, H, D, nq, lk = 2, 3, 24, 19, 37                      # nothing a multiple of a tile: 19 = 16 + 3 query rows, 37 keys, 3 pieces a row
    C = H * D
    q = b.inp(_rand((B, nq, C), 301).bfloat16(), ld=80, name="q")
    k = b.inp(_rand((B, lk, C), 302).bfloat16(), ld=88, name="k")
    v = b.inp(_rand((B, lk, C), 303).bfloat16(), ld=96, name="v")
    g = b.inp(_rand((B, nq, C), 304).bfloat16(), ld=80, name="d_o")
    mask = kpm = None
    if masks:
        mask = b.inp(torch.triu(torch.full((nq, lk), float("-inf")), 5), ld=40, name="mask")
        pad = torch.zeros((B, lk), dtype=U8)
        pad[0, 30:] = 1
        pad[1, :] = 1                                       # every key of sample 1 is padding: zeros
        kpm = b.inp(pad, name="kpm")
    dq = b.out((B, nq, C), BF16, ld=80, name="dq") if want_dq else None
    dk = b.out((B, lk, C), BF16, ld=88, name="dk")
    dv = b.out((B, lk, C), BF16, ld=80, name="dv")
    _chk(lib.udt_mattn_bwd(_p(q), _p(k), _p(v), _p(g), _p(dq), _p(dk), _p(dv), _p(mask), _p(kpm), B, H, D, nq, lk,
                           q.stride(1), k.stride(1), v.stride(1), g.stride(1), dq.stride(1) if want_dq else 0, dk.stride(1), dv.stride(1),
                           mask.stride(0) if masks else 0, q.stride(0), k.stride(0), v.stride(0), g.stride(0),
                           dq.stride(0) if want_dq else 0, dk.stride(0), dv.stride(0), D ** -0.5, O._stream()), "udt_mattn_bwd")
    if masks:
        torch.cuda.synchronize()
        assert bool((dk[1] == 0).all()) and bool((dv[1] == 0).all()) and bool((dq[1] == 0).all())
        assert bool(torch.isfinite(dk.float()).all()) and bool((dk[0] != 0).any())
    out = {"dk": dk, "dv": dv}
    if want_dq:
        out["dq"] = dq
    return out


@case("mattn_bwd 2x3x24 19x37 masks, ld gaps", ["udt_mattn_bwd"])
def _mattn_bwd_masked(b):
    return _mattn_bwd_case(b, True, True)


@case("mattn_bwd 2x3x24 19x37 dq null", ["udt_mattn_bwd"])
def _mattn_bwd_plain(b):
    return _mattn_bwd_case(b, False, False)


@case("gelu_fwd / gelu_bwd rows 3 C 40", ["udt_gelu_fwd", "udt_gelu_bwd"])
def _gelu(b):
    O, L, lib, P = _mods()
    a = b.inp(_rand((3, 40), 311, 2.0), name="a")
    dy = b.inp(_rand((3, 40), 312).bfloat16(), name="dy")
    out, da = b.out((3, 40), BF16, name="out"), b.out((3, 40), BF16, name="da")
    _chk(lib.udt_gelu_fwd(_p(a), _p(out), 3, 40, O._stream()), "udt_gelu_fwd")
    _chk(lib.udt_gelu_bwd(_p(a), _p(dy), _p(da), 3, 40, O._stream()), "udt_gelu_bwd")
    return {"out": out, "da": da}


@case("ocr_ce N 3 L 5, ld gaps", ["udt_ocr_ce_f32"])
def _ocr_ce(b):
    O, L, lib, P = _mods()
    N, Lq, T_, ncls = 3, 5, 7, 95
    x = _rand((N, Lq, ncls), 321, 3.0)
    tg = torch.randint(0, ncls, (N, T_), generator=torch.Generator().manual_seed(322)).to(I32)
    x[0, torch.arange(Lq), tg[0, :Lq].long()] += 25.0       # row 0 flows; rows 1 and 2 clamp
    logits = b.inp(x, ld=104, name="logits")
    targets = b.inp(tg, name="targets")
    n_chars = b.inp(torch.tensor([2, 5, 1], dtype=I32), name="n_chars")
    weight = b.inp(torch.tensor([0.5, 2.0, 1.0]), name="weight")
    loss = b.out((N,), F32, name="loss")
    d = b.out((N, Lq, ncls), F32, ld=96, name="d_logits")
    _chk(lib.udt_ocr_ce_f32(_p(logits), _p(targets), _p(n_chars), _p(weight), _p(loss), _p(d), N, Lq, ncls, logits.stride(1), T_,
                            d.stride(1), O._stream()), "udt_ocr_ce_f32")
    torch.cuda.synchronize()
    assert float(loss[0]) < 1.0 and float(loss[1]) == 1.0 and float(loss[2]) == 1.0
    assert bool((d[0, :2] != 0).any()) and bool((d[0, 2:] == 0).all()) and bool((d[1:] == 0).all())
    return {"loss": loss, "d_logits": d}


def _adjoint_case(b, boxes):
    O, L, lib, P = _mods()
    B, Cc, H, W = 3, 3, 37, 300                             # two 256-column segments per row, the second ragged
    d_out = b.inp(_rand((len(boxes), Cc, 32, 128), 331), name="d_out")
    bx = b.inp(torch.tensor(boxes, dtype=I32), name="boxes")
    d_img = b.out((B, Cc, H, W), F32, name="d_img")
    _chk(lib.udt_crop_resize_aa_bwd_f32(_p(d_out), _p(bx), _p(d_img), B, Cc, H, W, len(boxes), 32, 128, 2.0, O._stream()),
         "udt_crop_resize_aa_bwd_f32")
    return d_img


@case("crop_resize_aa_bwd 3x3x37x300, a box and a corner pixel", ["udt_crop_resize_aa_bwd_f32"])
def _adjoint(b):
    d_img = _adjoint_case(b, [[0, 3, 30, 10, 290], [2, 36, 37, 299, 300]])
    torch.cuda.synchronize()
    assert bool((d_img[1] == 0).all()) and bool((d_img[0, :, :3] == 0).all()) and bool((d_img[0, :, 3:30, 10:290] != 0).any())
    assert bool((d_img[2, :, 36, 299] != 0).all()) and int((d_img[2] != 0).sum()) == 3
    return {"d_img": d_img}


@case("crop_resize_aa_bwd with a repeated image index", ["udt_crop_resize_aa_bwd_f32"])
def _adjoint_repeated(b):
    """the precondition (one box per image) broken: the first box of the image is used, nothing outside d_img is touched"""
    d_img = _adjoint_case(b, [[1, 0, 20, 0, 100], [1, 10, 37, 50, 300]])
    torch.cuda.synchronize()
    assert bool((d_img[0] == 0).all()) and bool((d_img[2] == 0).all()) and bool((d_img[1, :, 20:] == 0).all())
    return {"d_img": d_img}


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[c[0] for c in CASES])
def test_ocr_loss_footprint(env, idx):
    name, fn, _ = CASES[idx]
    T._run_case(name, fn, env.dev)
