"""Memory footprint of the accumulating gradient kernels and the bucket optimiser step, as cases of tests/test_footprint_gpu.py's table.

The cases are appended to that module's ``CASES`` when this module is imported (pytest imports every test module before it runs the
first test), so ``test_every_entry_point_of_the_header_is_in_the_table_or_exempt`` (tests/test_footprint_cpu.py) finds them there; they
run here, through the table's own ``_run_case``: guarded / poisoned buffers against compact ones, bit-equal, no guard byte touched.
The segment tables of udt_bucket_update_f32 / udt_bucket_swap_f32 point INTO guarded buffers — every parameter and every shadow its
own arena, the flat g / m / v one arena each — and the padding between the segments inside g / m / v holds poison (g) or the output
sentinel (m, v): a kernel that walks a segment past its end, or touches padding, lands in a guard or is caught by the case.
"""
import ctypes as C

import pytest
import torch

import footprint as fp
import test_footprint_gpu as table
from test_footprint_gpu import BF16, F32, _chk, _mods, _p, _rand, env  # noqa: F401  (env: the table's fixture)

pytestmark = pytest.mark.gpu

OWN = []


def case(name, covers):
    def deco(fn):
        if name not in [c[0] for c in table.CASES]:           # (a re-import must not register twice)
            table.case(name, covers)(fn)
        OWN.append((name, fn))
        return fn
    return deco


def _wgrad_acc(R, N, K):
    def fn(b):
        O, L, lib, P = _mods()
        S = lib.udt_wgrad_splits(R, N, K)
        part = b.scratch(S * N * K * 4, name=f"wgrad partials ({S} splits)") if S > 1 else None
        dw = b.inout(_rand((N, K), 401, 3.0), name="dw (accumulate)")
        dy, x = b.inp(_rand((R, N), 402).bfloat16(), ld=N + 8, name="dy"), b.inp(_rand((R, K), 403).bfloat16(), ld=K + 8, name="x")
        _chk(lib.udt_wgrad_bf16_acc(_p(dy), _p(x), _p(dw), _p(part), R, N, K, dy.stride(0), x.stride(0), 1, O._stream()), "udt_wgrad_bf16_acc")
        over = b.out((N, K), F32, name="dw (accumulate 0)")
        _chk(lib.udt_wgrad_bf16_acc(_p(dy), _p(x), _p(over), _p(part), R, N, K, dy.stride(0), x.stride(0), 0, O._stream()), "udt_wgrad_bf16_acc")
        return {"dw": dw, "over": over}
    return fn


case("wgrad_acc (1000,648,72) split, ldy/ldx wider, partials exact", ["udt_wgrad_bf16_acc"])(_wgrad_acc(1000, 648, 72))
case("wgrad_acc (40,136,72) one range: add in the epilogue, no partials", ["udt_wgrad_bf16_acc"])(_wgrad_acc(40, 136, 72))


@case("colsum_acc rows 70 C 72, partials exact", ["udt_colsum_bf16_acc"])
def _colsum_acc(b):
    O, L, lib, P = _mods()
    part = b.scratch(lib.udt_colparts(70) * 72 * 4, name="colsum partials")
    out = b.inout(_rand((72,), 404, 3.0), name="out (accumulate)")
    _chk(lib.udt_colsum_bf16_acc(_p(b.inp(_rand((70, 72), 405).bfloat16(), name="x")), _p(part), _p(out), 70, 72, 1, O._stream()),
         "udt_colsum_bf16_acc")
    return {"out": out}


@case("ln_param_grad_acc rows 70 C 320, partials exact", ["udt_ln_param_grad_acc"])
def _ln_pg_acc(b):
    O, L, lib, P = _mods()
    part = b.scratch(lib.udt_colparts(70) * 2 * 320 * 4, name="ln_param_grad partials")
    out = b.inout(_rand((2, 320), 406, 3.0), name="dgamma_dbeta (accumulate)")
    _chk(lib.udt_ln_param_grad_acc(_p(b.inp(_rand((70, 320), 407, 2.0, 0.5).bfloat16(), name="x")),
                                   _p(b.inp(_rand((70, 320), 408).bfloat16(), name="dy")), _p(part), _p(out), 70, 320, 1e-5, 1, O._stream()),
         "udt_ln_param_grad_acc")
    return {"out": out}


SIZES = [1, 3, 4, 5, 255, 257, 4096, 4097, 9000]          # one chunk exactly, one element into the next, ragged ends


def _bucket(b, with_flat):
    """the operands of a bucket launch inside guarded buffers; returns (table, chunk map, ps, shadows, g, m, v, padding mask)"""
    O, L, lib, P = _mods()
    offs, o = [], 0
    for n in SIZES:
        offs.append(o)
        o += (n + 3) // 4 * 4
    total = (o + 63) // 64 * 64
    ps = [b.inout(_rand((n,), 410 + i, 0.05), name=f"p[{i}]") for i, n in enumerate(SIZES)]
    shs = [b.inout(_rand((n,), 430 + i, 0.05), name=f"shadow[{i}]") for i, n in enumerate(SIZES)]
    pad = torch.ones((total,), dtype=torch.bool)
    for n, off in zip(SIZES, offs):
        pad[off:off + n] = False
    g = m = v = None
    if with_flat:
        gh, mh, vh = _rand((total,), 450, 2e-3), _rand((total,), 451, 1e-3), _rand((total,), 452, 1e-3).abs() * 1e-3
        gi, mi, vi = gh.view(torch.int32), mh.view(torch.int32), vh.view(torch.int32)
        gi[pad] = fp._signed(fp.in_poison(F32), 4)
        mi[pad] = fp._signed(fp.out_sentinel(F32), 4)
        vi[pad] = fp._signed(fp.out_sentinel(F32), 4)
        g, m, v = b.inp(gh, name="g (bucket)"), b.inout(mh, name="m"), b.inout(vh, name="v")
    arr = (L.BucketSegment * len(SIZES))()
    seg_ids, chunk_ids = [], []
    for i, n in enumerate(SIZES):
        arr[i].p, arr[i].shadow, arr[i].offset, arr[i].n = ps[i].data_ptr(), shs[i].data_ptr(), offs[i], n
        k = (n + L.BUCKET_CHUNK - 1) // L.BUCKET_CHUNK
        seg_ids += [i] * k
        chunk_ids += list(range(k))
    tab = b.inp(torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).clone(), name="segment table")
    cmap = b.inp(torch.tensor(list(zip(seg_ids, chunk_ids)), dtype=torch.int32), name="chunk map")
    assert C.sizeof(L.BucketSegment) == 32 and cmap.is_contiguous()
    return tab, cmap, ps, shs, g, m, v, pad.to(b.dev)


def _bucket_update(mode):
    def fn(b):
        O, L, lib, P = _mods()
        tab, cmap, ps, shs, g, m, v, pad = _bucket(b, True)
        _chk(lib.udt_bucket_update_f32(_p(tab), _p(cmap), cmap.shape[0], _p(g), _p(m), _p(v), mode, 1e-3, 0.9, 0.999, 1e-3, 1e-2, 3, 0.5, 0.25,
                                       O._stream()), "udt_bucket_update_f32")
        for name, t in (("m", m), ("v", v)):
            assert fp.all_sentinel(t[pad]), f"padding of {name} was written"
            assert not fp.holds_sentinel(t[~pad])
        assert not bool(torch.isnan(torch.cat(ps + shs + [m[~pad], v[~pad]])).any()), "padding of g was read"
        return {"p": torch.cat(ps), "shadow": torch.cat(shs), "~m": m, "~v": v}
    return fn


case("bucket_update AdamW: 9 segments in their own arenas, padding poisoned", ["udt_bucket_update_f32"])(_bucket_update(1))
case("bucket_update AdamW + EMA: 9 segments in their own arenas, padding poisoned", ["udt_bucket_update_f32"])(_bucket_update(3))


@case("bucket_update EMA only: no g / m / v", ["udt_bucket_update_f32"])
def _bucket_ema(b):
    O, L, lib, P = _mods()
    tab, cmap, ps, shs, g, m, v, pad = _bucket(b, False)
    _chk(lib.udt_bucket_update_f32(_p(tab), _p(cmap), cmap.shape[0], None, None, None, 2, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 1.0, 0.25, O._stream()),
         "udt_bucket_update_f32 EMA")
    return {"p": torch.cat(ps), "shadow": torch.cat(shs)}


@case("bucket_swap: 9 segments in their own arenas", ["udt_bucket_swap_f32"])
def _bucket_swap(b):
    O, L, lib, P = _mods()
    tab, cmap, ps, shs, g, m, v, pad = _bucket(b, False)
    _chk(lib.udt_bucket_swap_f32(_p(tab), _p(cmap), cmap.shape[0], O._stream()), "udt_bucket_swap_f32")
    return {"p": torch.cat(ps), "shadow": torch.cat(shs)}


@pytest.mark.parametrize("idx", range(len(OWN)), ids=[c[0] for c in OWN])
def test_optim_footprint(env, idx):
    name, fn = OWN[idx]
    table._run_case(name, fn, env.dev)
