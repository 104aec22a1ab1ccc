"""Memory footprint of udt_aae_row_update_f32 (the row-wise attend-and-excite update), as cases of tests/test_footprint_gpu.py's table.

The cases are appended to that module's ``CASES`` when this module is imported, as tests/test_optim_footprint_gpu.py does it, and run
here through the table's own ``_run_case``: x updated in place inside a guarded arena, grad / loss / state_in guarded inputs, state_out
and n_active guarded outputs, every buffer against a compact one, bit-equal, no guard byte touched.  The frozen rows' grad and loss
hold the input poison (a NaN): the kernel must not let them reach anything it writes.
"""
import pytest
import torch

import footprint as fp
import test_footprint_gpu as table
from test_footprint_gpu import F32, I32, _chk, _mods, _p, _rand, env  # noqa: F401  (env: the table's fixture)

pytestmark = pytest.mark.gpu

OWN = []


def case(name, covers):
    def deco(fn):
        if name not in [c[0] for c in table.CASES]:           # (a re-import must not register twice)
            table.case(name, covers)(fn)
        OWN.append((name, fn))
        return fn
    return deco


def _row_update(B, n, active, counts, loss, thres=-0.5, max_iter=20):
    def fn(b):
        O, L, lib, P = _mods()
        act = torch.tensor(active, dtype=torch.bool)
        x0 = _rand((B, n), 701)
        gh, lh = _rand((B, n), 702, 0.1), torch.tensor(loss, dtype=torch.float32)
        poison = fp._signed(fp.in_poison(F32), 4)
        gh.view(torch.int32)[~act] = poison                  # frozen rows: NaN poison in grad and loss
        lh.view(torch.int32)[~act] = poison
        x = b.inout(x0, name="x")
        grad, ls = b.inp(gh, name="grad"), b.inp(lh, name="loss")
        st = b.inp(torch.tensor([active, counts], dtype=torch.int32), name="state_in")
        so, na = b.out((2, B), I32, name="state_out"), b.out((1,), I32, name="n_active")
        assert x.is_contiguous() and grad.is_contiguous() and st.is_contiguous() and so.is_contiguous()
        _chk(lib.udt_aae_row_update_f32(_p(x), _p(grad), _p(ls), _p(st), _p(so), _p(na), B, n, 1.5, thres, 1, max_iter, O._stream()),
             "udt_aae_row_update_f32")
        assert fp.bit_equal(x[~act.to(b.dev)], x0.to(b.dev)[~act.to(b.dev)]), "a frozen row of x was written"
        assert not bool(torch.isnan(x).any()), "a frozen row's poisoned grad reached x"
        return {"x": x, "state_out": so, "n_active": na}
    return fn


case("aae_row_update (3,1028) mixed: frozen rows' grad / loss poisoned", ["udt_aae_row_update_f32"])(
    _row_update(3, 1028, [1, 0, 7], [2, 5, 20], [0.3, 0.0, -0.9]))
case("aae_row_update (1,4) one active row", ["udt_aae_row_update_f32"])(_row_update(1, 4, [1], [0], [0.3]))


@pytest.mark.parametrize("idx", range(len(OWN)), ids=[c[0] for c in OWN])
def test_aae_rows_footprint(env, idx):
    name, fn = OWN[idx]
    table._run_case(name, fn, env.dev)
