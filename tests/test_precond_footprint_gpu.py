"""Memory footprint of the udt_precond_* entry points, as cases of tests/test_footprint_gpu.py's table.

The cases are appended to that module's ``CASES`` when this module is imported (pytest imports every test module before it runs the
first test), so ``test_every_entry_point_of_the_header_is_in_the_table_or_exempt`` (tests/test_footprint_cpu.py) finds them there; they
run here, through the table's own ``_run_case``: guarded / poisoned buffers against compact ones, bit-equal, no guard byte touched.
The unguided forms (pair = 0) get B rows of network output and B rows of xin inside their guards: a read or write of the rows a CFG
pair would have lands in poison or in a guard and is reported.
"""
import pytest
import torch

import footprint as fp
import test_footprint_gpu as table
from test_footprint_gpu import B3, BF16, F32, HW35, _chk, _mods, _p, _rand, env  # noqa: F401  (env: the table's fixture)

pytestmark = pytest.mark.gpu

OWN = []


def case(name, covers):
    def deco(fn):
        if name not in [c[0] for c in table.CASES]:           # (a re-import must not register twice)
            table.case(name, covers)(fn)
        OWN.append((name, fn))
        return fn
    return deco


def _f8(b, rows, seed):
    return b.inp(_rand((rows * HW35, 4), seed), ld=8, name="network output (channels 4..7 poisoned)")


def _euler(pair):
    def fn(b):
        O, L, lib, P = _mods()
        x = b.inout(_rand((B3, 4, HW35), 311, 10.0), name="x")
        den = b.out((B3, 4, HW35), F32, name="den_out")
        f = _f8(b, (2 if pair else 1) * B3, 312)
        _chk(lib.udt_precond_euler_step(_p(x), _p(f), _p(den), B3, HW35, f.stride(0), 0.09, -0.95, 3.2, 2.9, 5.0, pair, O._stream()),
             "udt_precond_euler_step")
        return {"x": x, "den": den}
    return fn


def _sampler(pair):
    def fn(b):
        O, L, lib, P = _mods()
        xin, aux, prev, noise = (b.inp(_rand((B3, 4, HW35), 313 + i, 3.0), name=n) for i, n in enumerate(("xin", "aux", "prev", "noise")))
        xout, den = b.out((B3, 4, HW35), F32, name="xout"), b.out((B3, 4, HW35), F32, name="den_out")
        k = L.SamplerCoefs(0.9, 0.2, -0.1, 0.05, 0.3, -0.95, 5.0)
        f = _f8(b, (2 if pair else 1) * B3, 317)
        _chk(lib.udt_precond_sampler_step(_p(xin), _p(f), _p(aux), _p(prev), _p(noise), _p(xout), _p(den), B3, HW35, f.stride(0), k, 0.09,
                                          pair, O._stream()), "udt_precond_sampler_step")
        x2 = b.inout(xin.clone(), name="xout = xin")                      # the alias the header allows
        _chk(lib.udt_precond_sampler_step(_p(x2), _p(f), _p(aux), _p(prev), _p(noise), _p(x2), None, B3, HW35, f.stride(0), k, 0.09,
                                          pair, O._stream()), "udt_precond_sampler_step in place")
        assert fp.bit_equal(x2, xout)
        return {"xout": xout, "den": den, "inplace": x2}
    return fn


def _multistep(pair):
    def fn(b):
        O, L, lib, P = _mods()
        xin, h1, h2 = (b.inp(_rand((B3, 4, HW35), 318 + i, 3.0), name=n) for i, n in enumerate(("xin", "hist1", "hist2")))
        xout, dout = b.out((B3, 4, HW35), F32, name="xout"), b.out((B3, 4, HW35), F32, name="d_out")
        k = L.MultistepCoefs(-0.95, 5.0, 3.2, 3)
        for j, cf in enumerate((-0.5, 0.2, -0.05)):
            k.k[j] = cf
        k.hist[1], k.hist[2] = _p(h1), _p(h2)
        f = _f8(b, (2 if pair else 1) * B3, 321)
        _chk(lib.udt_precond_multistep_step(_p(xin), _p(f), _p(xout), _p(dout), B3, HW35, f.stride(0), k, 0.09, pair, O._stream()),
             "udt_precond_multistep_step")
        return {"xout": xout, "d_out": dout}
    return fn


def _unet_input(pair, churn):
    def fn(b):
        O, L, lib, P = _mods()
        cpad = 64
        x = b.inout(_rand((B3, 4, HW35), 322, 10.0), name="x")
        xin = b.out(((2 if pair else 1) * B3 * HW35, cpad), BF16, name="xin")
        noise = b.inp(_rand((B3, 4, HW35), 323), name="noise") if churn else None
        _chk(lib.udt_precond_unet_input(_p(x), _p(noise), _p(xin), B3, HW35, cpad, 0.37, 0.8 if churn else 0.0, pair, O._stream()),
             "udt_precond_unet_input")
        assert not fp.holds_sentinel(xin[:, :4])
        assert fp.all_sentinel(xin[:, 4:]), "channels >= 4 of xin were touched"
        return {"x": x, "~xin": xin}
    return fn


for _pair in (1, 0):
    _tag = "pair" if _pair else "unguided"
    case(f"precond_euler_step {_tag} ld_f 8, den_out guarded", ["udt_precond_euler_step"])(_euler(_pair))
    case(f"precond_sampler_step {_tag} ld_f 8, all terms, xout / den_out guarded", ["udt_precond_sampler_step"])(_sampler(_pair))
    case(f"precond_multistep_step {_tag} ld_f 8, n 3, xout / d_out guarded", ["udt_precond_multistep_step"])(_multistep(_pair))
    for _churn in (False, True):
        case(f"precond_unet_input {_tag}{' churned' if _churn else ''} cpad 64: channels >= 4 keep their sentinel",
             ["udt_precond_unet_input"])(_unet_input(_pair, _churn))


@case("precond_loss_grad B 2 hw 35 ld_f 8 poisoned cpad 64: channels >= 4 exact zeros", ["udt_precond_loss_grad"])
def _loss(b):
    O, L, lib, P = _mods()
    B, hw = 2, 35
    f = b.inp(_rand((B * hw, 4), 392), ld=8, name="network output")
    noised, target = b.inp(_rand((B, 4, hw), 393, 3.0), name="noised"), b.inp(_rand((B, 4, hw), 394), name="target")
    c_skip, c_out, w = (b.inp(torch.tensor(v), name=n) for v, n in (([0.09, 0.67], "c_skip"), ([-0.95, -0.57], "c_out"),
                                                                     ([1.1, 3.0], "w")))
    d_f, loss = b.out((B * hw, 64), BF16, name="d_f"), b.out((B,), F32, name="loss")
    _chk(lib.udt_precond_loss_grad(_p(f), _p(noised), _p(target), _p(c_skip), _p(c_out), _p(w), _p(d_f), _p(loss), B, hw, f.stride(0), 64,
                                   O._stream()), "udt_precond_loss_grad")
    assert bool((fp.bits(d_f[:, 4:]) == 0).all()), "channels >= 4 of d_f are not exact (+0) zeros"
    return {"d_f": d_f, "loss": loss}


@pytest.mark.parametrize("idx", range(len(OWN)), ids=[c[0] for c in OWN])
def test_precond_footprint(env, idx):
    name, fn = OWN[idx]
    table._run_case(name, fn, env.dev)
