"""The OCR term of the training loss through its public interface, on the GPU (``pytest -m gpu``).

``FullLoss.get_ocr_loss`` on the fixture of tests/ocr_train_ref.py (latent 8 x 8, B = 3, one box per image, labels = the float64
oracle's reading of the float64-decoded crops, one row made wrong; tests/test_vae_backward_cpu.py pins its distances from the clamp):
the composition bit for bit, the losses within LOSS_TOL = 3e-2 of float64 (the float64-decoded frames and the float64 scorer, teacher-
forced with the GPU's own greedy tokens, as tests/test_ocr_loss_gpu.py takes its end-to-end reference: on the first GPU run the two
autoregressive loops disagreed in one token of one row, and the float64 cross entropy under the oracle's tokens, 0.0720, became
0.3132 under the GPU's — the loss was 0.3137), the clamped row exactly 1 with an exactly zero gradient.
``training.training_loss_and_grads`` with ``ocr_enabled`` on the batch of the training goldens: the loss dict, lambda_ocr_loss = 0
bit-equal to the term switched off, the seed handed to the reverse pass on the eps path and on a udt_precond_* path (VScaling).
``DiffusionEngine.training_step`` on a batch carrying r_bbox and label, on both optimisers.
"""
import contextlib
import os

import pytest
import torch

import ocr_loss_ref as O
import ocr_train_ref as T

pytestmark = pytest.mark.gpu
LOSS_TOL = 3e-2


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib, ops, training, vae_backward
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)

    class Env:
        pass
    Env.ops, Env.training, Env.vb, Env.dev = ops, training, vae_backward, cuda
    return Env


@pytest.fixture(scope="module")
def engine(cuda):
    from udifftext_amd import pipeline
    return pipeline.build_engine(cuda)


@pytest.fixture(scope="module")
def predictor(cuda):
    return O.load_predictor(O.sharpened_weights(), cuda)


def _loss_fn(predictor, **over):
    from sgm.util import instantiate_from_config
    from udifftext_amd import config as C
    cfg = C.default_model_config().model.params.loss_fn_config
    params = {k: v for k, v in cfg["params"].items() if k != "predictor_config"}
    params.update(over)
    loss_fn = instantiate_from_config({"target": cfg["target"], "params": params})
    loss_fn.predictor = predictor
    loss_fn.ocr_enabled = True
    return loss_fn


# ------------------------------------------------------------------------------------------------ get_ocr_loss
def test_get_ocr_loss_composition_losses_and_the_clamp(env, engine, predictor):
    fx = T.fixture()
    fsm = engine.first_stage_model
    loss_fn = _loss_fn(predictor)
    mo = fx["model_output"].to(env.dev)
    loss, d_mo = loss_fn.get_ocr_loss(mo, T.BOXES, fx["labels"], fsm, T.SCALER)
    assert loss.shape == (T.B,) and loss.dtype == torch.float32 and d_mo.shape == mo.shape and d_mo.dtype == torch.float32
    # the composition, bit for bit: decode_tape's bwd(get_ocr_loss_decoded(frames)[1]) / scaler on the same frames
    z = (mo.float() * (1.0 / T.SCALER)).contiguous()
    frames, bwd = env.vb.decode_tape(fsm, z)
    loss_d, d_frames = loss_fn.get_ocr_loss_decoded(frames, T.BOXES, fx["labels"])
    assert torch.equal(loss, loss_d) and torch.equal(d_mo, bwd(d_frames) / T.SCALER)
    # a weight passes through to get_ocr_loss_decoded; without want_grad there is no gradient (and no tape)
    loss_w, d_w = loss_fn.get_ocr_loss(mo, T.BOXES, fx["labels"], fsm, T.SCALER, weight=0.25)
    _, d_frames_w = loss_fn.get_ocr_loss_decoded(frames, T.BOXES, fx["labels"], weight=0.25)
    assert torch.equal(loss_w, loss) and torch.equal(d_w, bwd(d_frames_w) / T.SCALER)
    loss_n, none = loss_fn.get_ocr_loss(mo, T.BOXES, fx["labels"], fsm, T.SCALER, want_grad=False)
    assert none is None and loss_n.shape == loss.shape
    # the losses: float64 of the whole chain (the float64-decoded frames, the float64 scorer) under the GPU's OWN greedy tokens, as
    # tests/test_ocr_loss_gpu.py's end-to-end test takes its reference: the refinement pass is teacher-forced with the tokens of the
    # autoregressive loop, and a greedy near-tie between the two loops must not enter the comparison
    import crop_resize_ref as R
    loss_fn.get_ocr_loss(mo, T.BOXES, fx["labels"], fsm, T.SCALER)
    toks = predictor.parseq.last_refine_tokens.cpu()
    x64, _ = R.crop_resize(fx["frames64"], T.boxes5(), (32, 128), 2.0, -1.0)
    raw64, _ = O.chain_ref(fx["psd"], x64, toks, fx["labels"], torch.float64)
    x_gpu, _ = R.crop_resize(frames.double().cpu(), T.boxes5(), (32, 128), 2.0, -1.0)
    raw_gpu_frames, _ = O.chain_ref(fx["psd"], x_gpu, toks, fx["labels"], torch.float64)
    same = toks.shape == fx["tgt_in"].shape and bool((toks == fx["tgt_in"]).all())
    print(f"greedy tokens equal to the oracle's: {same}; GPU {toks.tolist()}; oracle {fx['tgt_in'].tolist()}")
    for b in fx["live"]:
        print(f"row {b} ({fx['labels'][b]!r}): loss {float(loss[b]):.4f}, float64 under the GPU's tokens {float(raw64[b]):.4f}, under the "
              f"oracle's {float(fx['raw64'][b]):.4f}, float64 scorer on the GPU's frames {float(raw_gpu_frames[b]):.4f}")
    for b in fx["live"]:
        assert float(loss[b]) < 1.0, f"row {b} drifted into the clamp: {float(loss[b])}"
        assert abs(float(loss[b]) - float(raw64[b])) <= LOSS_TOL, (b, float(loss[b]), float(raw64[b]))
    assert float(loss[T.WRONG_ROW]) == 1.0 and bool((d_mo[T.WRONG_ROW] == 0).all()), "the clamped row: loss 1 and a zero gradient, exactly"
    assert any(bool((d_mo[b] != 0).any()) for b in fx["live"]) and bool(torch.isfinite(d_mo).all())


# ------------------------------------------------------------------------------------------------ training_loss_and_grads
@contextlib.contextmanager
def _ocr_engine(engine, predictor, lam, denoiser=None):
    """the engine with an OCR-enabled loss (and, optionally, another denoiser) for the duration"""
    from sgm.util import instantiate_from_config
    from udifftext_amd import config as C
    old_loss, old_den = engine.loss_fn, engine.denoiser
    lf = _loss_fn(predictor, lambda_ocr_loss=lam)
    lf.to(next(engine.parameters()).device)
    engine.loss_fn = lf
    if denoiser is not None:
        engine.denoiser = instantiate_from_config(C.denoiser_config(denoiser, discrete=True)).to(next(engine.parameters()).device)
    try:
        yield engine
    finally:
        engine.loss_fn, engine.denoiser = old_loss, old_den


def _train_inputs(dev):
    import numpy as np
    from aae_fixture import train_batch
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_golden.npz"))
    batch = train_batch()
    z, idx, noise = (torch.from_numpy(g[k]).to(dev) for k in ("g14_z", "g14_sigma_idx", "g14_noise"))
    cond = {"concat": torch.from_numpy(g["g14_c_concat"]).to(dev), "t_crossattn": torch.from_numpy(g["g14_c_txt"]).to(dev)}
    return batch, z, idx, noise, cond, batch["seg"].to(dev), batch["seg_mask"].to(dev)


def _own_reading(predictor, frames, boxes):
    """the labels the scorer itself reads off the boxes (first 6 characters), so that rows stay below the clamp and carry a gradient"""
    return [(y[:6] or "a") for y in predictor.img2txt_boxes(frames, [[i] + list(bb) for i, bb in enumerate(boxes)])]


@pytest.mark.parametrize("denoiser", [None, "v"])
def test_training_loss_and_grads_with_the_ocr_term(env, engine, predictor, denoiser, monkeypatch):
    from udifftext_amd import backward
    tr, dev = env.training, env.dev
    batch, z, idx, noise, cond, seg, segm = _train_inputs(dev)
    B = z.shape[0]
    r_bbox = batch["r_bbox"]
    kw = dict(sigma_idx=idx, noise=noise)
    seen = {}
    real_add, real_bwd = env.ops.seed_add_, backward.UNetTape.backward

    def spy_add(seed, g, c_out):
        seen["before"], seen["g"], seen["c_out"] = seed.clone(), g.clone(), c_out.clone()
        return real_add(seed, g, c_out)

    def spy_bwd(self, d_eps=None, param_grads=None):
        seen["seed"] = d_eps.clone()
        return real_bwd(self, d_eps, param_grads=param_grads)
    with _ocr_engine(engine, predictor, 0.0, denoiser) as e:
        # labels that flow: the scorer's own reading of the decoded denoiser output at these draws
        tape, noised, sigma = tr.training_tape(e, z, cond, idx, noise)
        if tape.precond is None:
            c_skip, c_out = torch.ones_like(sigma), -sigma
        else:
            c_skip, c_out = tape.precond[0], tape.precond[1]
            assert denoiser == "v"
        den = env.ops.denoised(tape.eps, noised, c_skip, c_out)
        frames, _ = env.vb.decode_tape(e.first_stage_model, (den.float() * (1.0 / float(e.scale_factor))).contiguous())
        labels = _own_reading(predictor, frames, r_bbox.tolist())             # (the frames get_ocr_loss will score, bit for bit)
        del frames
        del tape
        # lambda_ocr_loss = 0: the loss dict gains the term, the gradients are bit-equal to the term switched off
        ld0, g0 = tr.training_loss_and_grads(e, z, cond, seg, segm, r_bbox=r_bbox, label=labels, **kw)
        e.loss_fn.ocr_enabled = False
        ld_off, g_off = tr.training_loss_and_grads(e, z, cond, seg, segm, **kw)
        e.loss_fn.ocr_enabled = True
        assert "loss/ocr_loss" in ld0 and "loss/ocr_loss" not in ld_off
        assert torch.equal(ld0["loss/full_loss"], ld_off["loss/full_loss"]) and set(g0) == set(g_off)
        for n in g0:
            assert torch.equal(g0[n], g_off[n]), n
        # lambda_ocr_loss > 0
        lam = 0.5
        e.loss_fn.lambda_ocr_loss = lam
        monkeypatch.setattr(env.ops, "seed_add_", spy_add)
        monkeypatch.setattr(backward.UNetTape, "backward", spy_bwd)
        ld, grads = tr.training_loss_and_grads(e, z, cond, seg, segm, r_bbox=r_bbox, label=labels, **kw)
        monkeypatch.undo()
        lam_local = float(e.loss_fn.lambda_local_loss)
        want = ld["loss/diff_loss"] + lam_local * ld["loss/local_loss"] + lam * ld["loss/ocr_loss"]
        size = abs(float(ld["loss/diff_loss"])) + abs(lam_local * float(ld["loss/local_loss"])) + abs(lam * float(ld["loss/ocr_loss"]))
        assert abs(float(ld["loss/full_loss"]) - float(want)) <= 2.0 ** -22 * size, (float(ld["loss/full_loss"]), float(want))
        assert torch.equal(ld["loss/ocr_loss"], ld0["loss/ocr_loss"]) and torch.equal(ld["loss/diff_loss"], ld0["loss/diff_loss"])
        assert 0.0 < float(ld["loss/ocr_loss"]) < 1.0, "no row flows: the seed check below would be vacuous"
        # the seed: diff seed + c_out[b] d_D, to one rounding of the seed's type (bf16), d_D = get_ocr_loss's gradient at weight lam / B
        assert torch.equal(seen["c_out"], c_out)
        if denoiser is None:
            assert torch.equal(seen["c_out"], -e.denoiser.sigmas.to(dev).float()[idx.to(dev)])
        _, d_den = e.loss_fn.get_ocr_loss(den, r_bbox, labels, e.first_stage_model, e.scale_factor, weight=lam / B)
        assert torch.equal(seen["g"], d_den) and bool((d_den != 0).any())
        exact = seen["before"].double()[..., :4] + (c_out.double().view(B, 1, 1, 1) * d_den.double()).permute(0, 2, 3, 1)
        got = seen["seed"].double()
        assert torch.equal(seen["seed"][..., 4:], seen["before"][..., 4:])
        assert bool(((got[..., :4] - exact).abs() <= 2.0 ** -8 * exact.abs() + 1e-30).all())
        assert not torch.equal(seen["seed"], seen["before"])
        assert any(not torch.equal(grads[n], g0[n]) for n in grads)


def test_missing_boxes_or_labels_are_refused_before_any_launch(env, engine, predictor):
    batch, z, idx, noise, cond, seg, segm = _train_inputs(env.dev)
    with _ocr_engine(engine, predictor, 0.5) as e:
        with pytest.raises(ValueError, match="r_bbox and label"):
            env.training.training_loss_and_grads(e, z, cond, seg, segm, sigma_idx=idx, noise=noise, label=["a", "b"])


# ------------------------------------------------------------------------------------------------ DiffusionEngine.training_step
@pytest.mark.parametrize("fused", [False, True])
def test_engine_training_step_with_the_ocr_term(env, engine, predictor, cuda, fused):
    from aae_fixture import train_batch
    tr = env.training
    prev_keys = engine.opt_keys
    engine.opt_keys = ["t_attn", "t_norm"]
    named = tr.trainable_parameters(engine)
    before = {n: p.detach().clone() for n, p in named}
    frozen = {n: p.detach().clone() for n, p in list(engine.first_stage_model.named_parameters())[:8]}
    scorer = {n: p.detach().clone() for n, p in list(predictor.named_parameters())[:8]}
    try:
        with _ocr_engine(engine, predictor, 0.5) as e:
            batch = {k: (v.to(cuda) if isinstance(v, torch.Tensor) and k != "r_bbox" else v) for k, v in train_batch().items()}
            assert "r_bbox" in batch and "label" in batch
            opt = e.configure_optimizers(5e-5 * 16, fused=fused)
            torch.manual_seed(77)
            ld = e.training_step(batch, opt)
            assert "loss/ocr_loss" in ld and bool(torch.isfinite(ld["loss/full_loss"])) and 0.0 < float(ld["loss/ocr_loss"]) <= 1.0
            changed = sum(int(not torch.equal(p.detach(), before[n])) for n, p in named)
            assert changed >= 100, changed
            for n, p in list(e.first_stage_model.named_parameters())[:8]:
                assert torch.equal(p.detach(), frozen[n]), n
            for n, p in list(predictor.named_parameters())[:8]:
                assert torch.equal(p.detach(), scorer[n]), n
    finally:
        engine.opt_keys = prev_keys
        with torch.no_grad():
            for n, p in named:
                p.copy_(before[n])
