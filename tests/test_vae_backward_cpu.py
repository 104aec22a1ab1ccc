"""CPU-side checks of the VAE decoder's reverse pass and the OCR term of the training step:

  * the attention reference the GPU test leans on: ``backward_ref.attn_bwd_head`` at head_dim 512 equals torch.autograd of
    softmax(q k^T scale) v in float64, and its ``emulate=True`` form differs from it by no more than the bf16 rounding of P, dS and
    the results;
  * the ABI: include/udt_kernels.h declares udt_attn512_bwd, udt_denoised_f32 and udt_seed_add_bf16, the built library exports them
    with the expected argument counts, and the footprint table covers them;
  * ``training.check_trainable`` accepts ``ocr_enabled`` with a predictor and refuses ``style_enabled``; ``get_ocr_loss`` without a
    predictor and ``training_loss_and_grads`` without r_bbox / label raise ValueError before any launch;
  * tests/golden/vae_backward_golden.npz (the real reference in float64) agrees with float64 autograd of ``oracle.nets.vae_decode``
    to 1e-9 relative: the oracle the per-layer GPU tests use and the reference are the same function;
  * the conditions of tests/test_ocr_train_gpu.py's fixture (tests/ocr_train_ref.py), from the float64 references alone: every "live"
    row's float64 cross entropy is <= 0.8 and the "clamped" row's is >= 1.2, and the reading survives decode-sized noise;
  * after ``prepare(free_masters=True)`` (frozen layouts) the reverse pass's layouts raise ``hipnn.layout``'s UdtError.
"""
import os
import re
import types

import pytest
import torch

import backward_ref as R
import vae_backward_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the attention reference
def _attn_inputs(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((n, 512), generator=g).bfloat16().float() for _ in range(4)]


@pytest.mark.parametrize("n", [1, 33, 97])
def test_attention_reference_at_head_dim_512_is_autograd(n):
    q, k, v, d_o = _attn_inputs(n, n)
    scale = 512 ** -0.5
    with torch.enable_grad():
        qg, kg, vg = (t.double().requires_grad_(True) for t in (q, k, v))
        o = torch.softmax(qg @ kg.t() * scale, dim=-1) @ vg
        want = torch.autograd.grad((o * d_o.double()).sum(), [qg, kg, vg])
    got = R.attn_bwd_head(q, k, v, d_o, scale, R.F64)
    for nm, w in zip(("dq", "dk", "dv"), want):
        assert got[nm].dtype == torch.float64
        assert float((got[nm] - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), nm
    # with the forward's output handed in as an operand the result is the same (D = rowsum(dO o O))
    given = R.attn_bwd_head(q, k, v, d_o, scale, R.F64, o=o.detach())
    for nm in ("dq", "dk", "dv"):
        assert float((given[nm] - got[nm]).abs().max()) <= 1e-12 * max(1.0, float(got[nm].abs().max()))


@pytest.mark.parametrize("n", [33, 97])
def test_attention_emulation_differs_by_the_stated_roundings_only(n):
    """P and dS rounded to bf16 (2^-9 relative each, summand by summand: 2^-9 of the sum of |summands|, the "abs" output), the
    result rounded to bf16 (2^-9 of itself): |emulated - exact| <= 2^-8 abs, element by element — and the roundings are there"""
    q, k, v, d_o = _attn_inputs(n, 100 + n)
    scale = 512 ** -0.5
    o = (torch.softmax(q.double() @ k.double().t() * scale, dim=-1) @ v.double()).bfloat16().double()
    exact, emul = R.attn_bwd_head(q, k, v, d_o, scale, R.F64, emulate="both", o=o)
    for nm in ("dq", "dk", "dv"):
        err = (emul[nm] - exact[nm]).abs()
        assert bool((err <= 2.0 ** -8 * exact["abs"][nm] + 1e-300).all()), nm
        assert float(err.max()) > 0
        assert torch.equal(emul[nm], emul[nm].bfloat16().double()), f"{nm}: the emulated result is a bf16 value"


# ------------------------------------------------------------------------------------------------ the ABI
NEW = {"udt_attn512_bwd": 26, "udt_denoised_f32": 9, "udt_seed_add_bf16": 7}


def test_new_entry_points_are_declared_typed_built_and_in_the_footprint_table():
    import test_footprint_gpu as table
    import test_vae_backward_footprint_gpu  # noqa: F401  (registers its cases in the table)
    from udifftext_amd import lib, ops
    header = open(os.path.join(ROOT, "include", "udt_kernels.h")).read()
    so = lib.load()
    covered = {name for _, _, covers in table.CASES for name in covers}
    for name, n_args in NEW.items():
        m = re.search(r"int\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"include/udt_kernels.h does not declare {name}"
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args == len(lib.SYMBOLS[name][1]), name
        assert hasattr(so, name), f"libudt_kernels.so does not export {name}"
        assert name in covered, f"{name} has no footprint case"
    assert callable(ops.attention_d512_bwd) and callable(ops.denoised) and callable(ops.seed_add_)


def test_attn512_bwd_refuses_its_domain_without_a_gpu():
    """the host checks come before anything touches the device: null pointers, n < 1, ld % 8, misaligned pointers"""
    from udifftext_amd import lib
    so = lib.load()
    p = 1 << 20                                                # (an aligned non-null address; never dereferenced)
    ok = [p] * 10 + [1, 40, 512, 512, 512, 512, 512, 1536, 0, 0, 0, 0, 0, 0, 0.1, None]
    def call(i, val):
        a = list(ok)
        a[i] = val
        return so.udt_attn512_bwd(*a)
    for i in range(10):
        assert call(i, None) == -2
    for i in range(8):
        assert call(i, p + 8) == -2
    assert call(11, 0) == -1 and call(10, 0) == -1
    for i in range(12, 18):
        assert call(i, 516) == -1 and call(i, 504) == -1
    for i in range(18, 24):
        assert call(i, 4) == -1


# ------------------------------------------------------------------------------------------------ the interface's refusals
def _loss_fn(**over):
    import udifftext_amd  # noqa: F401
    from sgm.util import instantiate_from_config
    from udifftext_amd import config as C
    cfg = C.default_model_config().model.params.loss_fn_config
    params = {k: v for k, v in cfg["params"].items() if k != "predictor_config"}
    params.update(over)
    return instantiate_from_config({"target": cfg["target"], "params": params})


def _engine(loss_fn):
    from sgm.util import instantiate_from_config
    from udifftext_amd import config as C
    den = instantiate_from_config(C.default_model_config().model.params.denoiser_config)
    return types.SimpleNamespace(loss_fn=loss_fn, denoiser=den,
                                 conditioner=types.SimpleNamespace(embedders=[types.SimpleNamespace(is_trainable=False)]))


def test_check_trainable_accepts_the_ocr_loss_with_a_predictor_and_refuses_the_style_loss():
    from udifftext_amd import training
    loss_fn = _loss_fn()
    loss_fn.ocr_enabled = True
    loss_fn.predictor = torch.nn.Identity()                    # (check_trainable asks whether there is one, nothing more)
    training.check_trainable(_engine(loss_fn))
    with pytest.raises(NotImplementedError, match="get_style_local_loss"):
        training.check_trainable(_engine(_loss_fn(style_enabled=True)))
    both = _loss_fn(style_enabled=True)
    both.ocr_enabled, both.predictor = True, torch.nn.Identity()
    with pytest.raises(NotImplementedError, match="style"):
        training.check_trainable(_engine(both))


def test_ocr_interface_raises_value_errors_before_any_launch():
    from udifftext_amd import training
    z = torch.zeros((1, 4, 8, 8))
    with pytest.raises(ValueError, match="predictor"):
        _loss_fn().get_ocr_loss(z, [[0, 8, 0, 8]], ["a"], None, 0.18215)
    loss_fn = _loss_fn()
    loss_fn.ocr_enabled, loss_fn.predictor = True, torch.nn.Identity()
    for kw in (dict(), dict(r_bbox=[[0, 8, 0, 8]]), dict(label=["a"])):
        with pytest.raises(ValueError, match="r_bbox and label"):
            training.training_loss_and_grads(_engine(loss_fn), z, {}, None, None, **kw)


# ------------------------------------------------------------------------------------------------ golden vs oracle
@pytest.mark.parametrize("case", list(V.CASES))
def test_golden_agrees_with_float64_autograd_of_the_oracle(case):
    G = V.golden()
    B, h, w = V.CASES[case]
    z, d_frames = torch.from_numpy(G[f"{case}_z"]), torch.from_numpy(G[f"{case}_d_frames"])
    assert z.shape == (B, 4, h, w) and d_frames.shape == (B, 3, 8 * h, 8 * w)
    _, sd = V.build_vae()
    frames, d_z = V.vjp64(V.decode_fn(sd), z, d_frames)
    assert V.rel_rms(frames, G[f"{case}_frames"]) <= 1e-9
    assert V.rel_rms(d_z, G[f"{case}_d_z"]) <= 1e-9
    twin_rel = [V.rel_rms(G[f"{case}_twin_d_z"][b], G[f"{case}_d_z"][b]) for b in range(B)]
    assert twin_rel == pytest.approx(list(G[f"{case}_twin_rel"]), rel=1e-6)
    assert all(1e-3 < r < 3e-2 for r in twin_rel), twin_rel     # (a bf16 twin: neither exact nor beyond the stated TOL_UNET)


# ------------------------------------------------------------------------------------------------ the end-to-end fixture
def test_fixture_rows_keep_their_distance_from_the_clamp():
    import ocr_train_ref as T
    fx = T.fixture()
    raw = fx["raw64"]
    assert raw.dtype == torch.float64 and raw.shape == (T.B,)
    assert fx["live"] == [b for b in range(T.B) if b != T.WRONG_ROW] and len(fx["live"]) == 2
    for b in fx["live"]:
        assert 0.0 < float(raw[b]) <= 0.8, (b, float(raw[b]))
    assert float(raw[T.WRONG_ROW]) >= 1.2 and fx["labels"][T.WRONG_ROW] == T.WRONG_LABEL
    assert fx["frames64"].shape == (T.B, 3, 64, 64) and fx["model_output"].shape == (T.B, 4, 8, 8)
    for (t, b, l, r) in T.BOXES:
        assert 0 <= t < b <= 64 and 0 <= l < r <= 64


def test_fixture_reading_survives_decode_sized_noise():
    import ocr_train_ref as T
    fx = T.fixture()
    for k in range(2):
        same, raw = T.perturbed(fx, k)
        assert same, f"noise draw {k} changes the greedy tokens"
        for b in fx["live"]:
            assert abs(float(raw[b]) - float(fx["raw64"][b])) <= 1.5e-2, (k, b, float(raw[b]), float(fx["raw64"][b]))


# ------------------------------------------------------------------------------------------------ frozen layouts
def test_reverse_pass_layouts_raise_the_clean_error_once_the_masters_are_released():
    from sgm.modules import hipnn as H
    from udifftext_amd import backward, lib, vae_backward
    vae, _ = V.build_vae()
    attn, conv = vae.decoder.mid.attn_1, vae.decoder.mid.block_1.conv1
    H.freeze_layouts(attn)
    H.freeze_layouts(conv)
    with pytest.raises(lib.UdtError, match="free_masters"):
        vae_backward._attn_wT(attn)
    with pytest.raises(lib.UdtError, match="free_masters"):
        backward._conv_wt(conv)
