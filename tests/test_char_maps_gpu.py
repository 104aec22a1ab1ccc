"""Character attention maps at throughput (``pytest -m gpu``).

Kernel level — udt_tattn_fused_maps (csrc/tattn.hip) on tests/attention_cases.py's inputs: ``out`` (and the MX8 twin with its row
statistics) bit-equal to the plain entry point's, ``maps`` repeated bit for bit and held slice by slice (one token tile x one sample) to
the float64 map of tests/char_maps_ref.py by tests/sliced_check.py with its margins 2 and 4 — the floor from the emulation that rounds P
to bf16 and nothing else (the header's ROUNDING paragraph), the abs scale the softmax's sensitivity to the fp32 rounding of its scores;
store mode, and two launches at weight 0.5 that accumulate.  udt_resize_bilinear_f32 (csrc/resample.hip) element by element within
16 x 2^-24 of the sum of its absolute summands.  One line per check goes to char_maps_report.txt next to the run's parity report;
profiles/char_maps_report.txt is a passing run's.

Product level — one UNet call against the real reference's maps (tests/golden/char_maps_golden.npz, make_char_maps_golden.py);
``pipeline.predict_many`` with ``cfgs.detailed``: the image does not change by a bit, an image's maps do not depend on its batch mates,
they agree with the maps ``predict`` dumps through the unfused route, ``map_size`` is kernel 2 applied to them, and the contract holds
under attend-and-excite and through ``evaluate``.
"""
import os

import numpy as np
import pytest
import torch

import attention_cases as K
import attention_ref as R
import char_maps_ref as M
import sliced_check as S
import test_backward_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(os.path.dirname(test_backward_gpu.REPORT), "char_maps_report.txt")        # a file of its own, same directory
GOLD = os.path.join(ROOT, "tests", "golden", "char_maps_golden.npz")


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib, ops
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)

    class Env:
        pass
    Env.ops, Env.L, Env.lib, Env.dev = ops, lib, lib.load(), cuda
    return Env


def _line(text):
    S._report(text, REPORT)


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return float((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300))


def _hold(name, got, ref, bound):
    r = _rel(got, ref)
    _line(f"{name:70s} rel_rms {r:.3e} (bound {bound:.1e}){'  FAIL' if not r <= bound else ''}")
    assert r <= bound, f"{name}: rel_rms {r:.3e} > {bound}"


# ================================================================================================ kernel 1: the maps
# (heads, B, n_tok, L, zero, map_from): every width at one and two token tiles (all of them channel-split: nsplit = 8, only split 0
# writes), B = 3 with zero_samples 1 and map_from 1 and 2, L = 2 and 12 — and one shape per width without a channel split
_SMALL = [(heads, 3, tiles * (64 if heads == 5 else 32), L, 1, map_from)
          for heads in (5, 10, 20) for tiles in (1, 2) for L in (2, 12) for map_from in (1, 2)]
_WHOLE = [(5, 4, 4096, 12, 1, 1), (10, 2, 4096, 5, 0, 0), (20, 2, 4096, 12, 1, 1)]
MAP_SHAPES = _SMALL + _WHOLE


def _map_slices(Bm, n_tok, TT):
    """maps [Bm, L, n_tok]: (sample, every context token, one token tile) — what one workgroup writes"""
    for b in range(Bm):
        for t0 in range(0, n_tok, TT):
            yield (b, slice(None), slice(t0, t0 + TT))


def _prepared(env, heads, B, n_tok, L, seed=0):
    x, kv, wq, wo, gamma, beta, bias = K.tattn_inputs(heads, B, n_tok, L, seed=seed)
    xb, kvb, wqb, wob = (t.bfloat16().to(env.dev).contiguous() for t in (x, kv, wq, wo))
    ga, be, bi = (t.to(env.dev) for t in (gamma, beta, bias))
    tabs = env.ops.tattn_prepare(kvb, wqb, wob, ga, be, heads, K.TATTN_SCALE)
    A, _ = R.tattn_unpack(tabs.A.float(), tabs.BmT.float())
    return x.to(env.dev), xb, tabs, A, tabs.sc.clone(), bi


@pytest.mark.parametrize("heads,B,n_tok,L,zero,map_from", MAP_SHAPES)
def test_fused_text_attention_maps(env, heads, B, n_tok, L, zero, map_from):
    TT, tiles, nsplit = K.tattn_launch(heads, B, n_tok)
    assert (nsplit > 1) == ((heads, B, n_tok, L, zero, map_from) in _SMALL)
    name = f"heads{heads} B{B} n{n_tok} L{L} zero{zero} map_from{map_from} ({tiles} tiles of {TT} x {nsplit} channel splits)"
    ops = env.ops
    xd, xb, tabs, A, sc, bi = _prepared(env, heads, B, n_tok, L)
    q8 = heads != 5                                                           # (the MX8-emitting form exists for C = 640 / 1280)
    for emit_q8 in ((False, True) if q8 else (False,)):
        want = ops.tattn_fused(xb, tabs, bi, heads, zero, K.TATTN_EPS, emit_q8=emit_q8)
        maps = torch.full((B - map_from, L, n_tok), float("nan"), dtype=torch.float32, device=env.dev)
        got = ops.tattn_fused_maps(xb, tabs, bi, heads, zero, K.TATTN_EPS, maps, map_from, emit_q8=emit_q8)
        assert torch.equal(got, want), f"{name}: out differs from udt_tattn_fused{'_q8' if emit_q8 else ''}"
        if emit_q8:
            a, b = ops.mx8_of(got), ops.mx8_of(want)
            assert a is not None and b is not None
            assert torch.equal(a.data, b.data) and torch.equal(a.scale, b.scale) and torch.equal(a.stats, b.stats), f"{name}: MX8 twin"
        again = torch.full_like(maps, float("nan"))
        ops.tattn_fused_maps(xb, tabs, bi, heads, zero, K.TATTN_EPS, again, map_from, emit_q8=emit_q8)
        assert torch.equal(maps, again), f"{name}: maps are not deterministic"
        if emit_q8:
            assert torch.equal(maps, first), f"{name}: the MX8 form writes other maps than the bf16 form"
        first = maps
    ref, a = M.tattn_maps(xd, A, sc, heads, L, map_from, K.TATTN_EPS)
    emul = M.tattn_maps(xd, A, sc, heads, L, map_from, K.TATTN_EPS, emulate=True)
    worst = S.check_sliced(f"char maps store {name}", first, ref, emul - ref, _map_slices(B - map_from, n_tok, TT), abs_scale=M.rms(a),
                           report=REPORT)
    # accumulate: two launches at weight 0.5 (other rows, the same tables), the first stores and the second adds
    xd2, xb2 = _prepared(env, heads, B, n_tok, L, seed=1)[:2]
    acc = torch.full_like(first, float("nan"))
    ops.tattn_fused_maps(xb, tabs, bi, heads, zero, K.TATTN_EPS, acc, map_from, weight=0.5)
    ops.tattn_fused_maps(xb2, tabs, bi, heads, zero, K.TATTN_EPS, acc, map_from, weight=0.5, accumulate=True)
    r2, a2 = M.tattn_maps(xd2, A, sc, heads, L, map_from, K.TATTN_EPS, weight=0.5)
    e2 = M.tattn_maps(xd2, A, sc, heads, L, map_from, K.TATTN_EPS, weight=0.5, emulate=True)
    worst2 = S.check_sliced(f"char maps accumulate {name}", acc, 0.5 * ref + r2, 0.5 * (emul - ref) + (e2 - r2),
                            _map_slices(B - map_from, n_tok, TT), abs_scale=M.rms(0.5 * a + a2), report=REPORT)
    _line(f"char maps {name}: worst ratio-to-bound store {worst:.3f}, accumulate {worst2:.3f}")
    # every token's L probabilities of a head sum to one: so do their head means (bf16 P: to 2^-9 per head at the most)
    assert float((first.double().sum(dim=1) - 1).abs().max()) <= 12 * 2.0 ** -9


def test_fused_text_attention_maps_bad_arguments_launch_nothing(env):
    heads, B, n_tok, L, zero = 5, 3, 64, 5, 1
    _, xb, tabs, _, _, bi = _prepared(env, heads, B, n_tok, L)
    lib, p = env.lib, (lambda t: None if t is None else t.data_ptr())
    out = torch.full_like(xb, K.MARKER)
    maps = torch.full((B, 12, n_tok), K.MARKER, dtype=torch.float32, device=env.dev)

    def call(maps_t, Lc, map_from, x=xb):
        return lib.udt_tattn_fused_maps(p(x), p(out), p(tabs.A), p(tabs.sc), p(tabs.BmT), p(bi), B, n_tok, heads * 64, heads, zero,
                                        K.TATTN_EPS, p(maps_t), Lc, map_from, 1.0, 0, None, None, None, env.ops._stream())
    BAD_ARG, BAD_SHAPE = -2, -1                                               # (include/udt_kernels.h udt_status)
    assert lib.udt_status_string(BAD_ARG) and call(None, L, 1) == BAD_ARG and call(maps, L, 1, x=None) == BAD_ARG
    for Lc, map_from in ((0, 1), (13, 1), (-1, 1), (L, 0), (L, B + 1), (L, -1)):
        assert call(maps, Lc, map_from) == BAD_SHAPE, (Lc, map_from)
    torch.cuda.synchronize()
    assert bool((out == K.MARKER).all()) and bool((maps == K.MARKER).all()), "a refused call launched something"
    assert call(maps, L, B) == 0                                              # map_from == B: no plane, the plain result
    torch.cuda.synchronize()
    assert bool((maps == K.MARKER).all()) and torch.equal(out, env.ops.tattn_fused(xb, tabs, bi, heads, zero, K.TATTN_EPS))


# ================================================================================================ kernel 2: bilinear resize
RESIZE_SHAPES = [(6, (8, 8), (64, 64)), (6, (8, 12), (64, 96)), (6, (3, 5), (7, 4)), (6, (1, 1), (5, 5)), (24, (64, 64), (512, 512))]


@pytest.mark.parametrize("planes,hw,HW", RESIZE_SHAPES)
def test_resize_bilinear(env, planes, hw, HW):
    g = torch.Generator().manual_seed(hw[0] * 1000 + HW[1])
    x = torch.randn((2, planes // 2) + hw, generator=g).to(env.dev)
    got = env.ops.resize_bilinear(x, HW)
    assert got.shape == (2, planes // 2) + HW and got.dtype == torch.float32
    ref, asum = M.bilinear(x, *HW)
    S.check_fp32_sum(f"resize_bilinear {planes} planes {hw} -> {HW}", got, ref, asum, report=REPORT)
    assert torch.equal(got, env.ops.resize_bilinear(x, HW)), "resize_bilinear: not deterministic"
    want = torch.nn.functional.interpolate(x.double(), size=HW, mode="bilinear", align_corners=False)
    assert float((ref - want).abs().max()) <= 1e-12                          # (the restatement IS F.interpolate, here too)
    lib = env.lib
    assert lib.udt_resize_bilinear_f32(None, got.data_ptr(), planes, *hw, *HW, env.ops._stream()) == -2                  # UDT_ERR_BAD_ARG
    assert lib.udt_resize_bilinear_f32(x.data_ptr(), got.data_ptr(), planes, hw[0], hw[1], 0, HW[1], env.ops._stream()) == -1     # _BAD_SHAPE


# ================================================================================================ product level
@pytest.fixture(scope="module")
def engine(cuda):
    from udifftext_amd import lib, pipeline
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)
    return pipeline.build_engine(cuda)


def _copy(batch):
    return {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in batch.items()}


def test_unet_maps_against_the_reference(engine, cuda):
    """the G7 setup (tests/golden/make_golden.py): one UNet call of the CFG pair at t = 999, made as the sampling loop makes it, asking
    for each fixture layer's maps — relative RMS <= 3e-2, the project's bound for a single t_attn map (tests/test_engine_gpu.py)"""
    from udifftext_amd import ops, pipeline, synth
    from sgm.modules.diffusionmodules.openaimodel import CPAD
    gold = np.load(GOLD)
    unet = engine.model.diffusion_model
    batch = synth.synthetic_batch(1, 256, 256, 4, seed=0)
    torch.manual_seed(1234)
    batch, buc = pipeline.prepare_batch(batch, cuda)
    c, uc = engine.conditioner.get_unconditional_conditioning(batch, batch_uc=buc, force_uc_zero_embeddings=["label"])
    x7 = torch.randn((1, 4, 32, 32), generator=torch.Generator().manual_seed(7)).to(cuda)
    x = torch.cat([torch.cat([x7, x7]), torch.cat([uc["concat"], c["concat"]])], dim=1)
    tctx = torch.cat([uc["t_crossattn"], c["t_crossattn"]])
    xin = ops.nchw_to_nhwc(x.float().contiguous(), CPAD)
    emb = unet.time_embedding_rows(torch.tensor([999.0, 999.0], device=cuda))
    t_kv = unet.project_context(tctx)
    t_fused = unet.prepare_fused_tattn(t_kv)
    plain = unet.forward_nhwc(xin, emb, t_kv, zero_ctx_rows=1, t_fused=t_fused)
    for layers, key in [((str(n),), f"maps_{n}") for n in gold["layers"]] + [(tuple(str(n) for n in gold["pair"]), "maps_two_layers")]:
        want = torch.from_numpy(gold[key])
        maps = torch.full(tuple(want.shape), float("nan"), dtype=torch.float32, device=cuda)
        eps = unet.forward_nhwc(xin, emb, t_kv, zero_ctx_rows=1, t_fused=t_fused, char_maps=maps, map_from=1, map_layers=layers)
        assert torch.equal(eps, plain), f"{layers}: eps changed with the maps"
        _hold(f"UNet call: head-mean maps of {'+'.join(layers)} vs the reference", maps, want, 3e-2)
    # what is not covered says so: the 4x4 level of a 32x32 latent (16 tokens), and a selection of two map sizes
    maps = torch.zeros((1, 12, 16), dtype=torch.float32, device=cuda)
    with pytest.raises(NotImplementedError, match="middle_block.1.*16 tokens"):
        unet.forward_nhwc(xin, emb, t_kv, zero_ctx_rows=1, t_fused=t_fused, char_maps=maps, map_from=1, map_layers=("middle_block.1",))
    with pytest.raises(RuntimeError, match="different map sizes"):
        unet.char_map_plan(32, 32, 12, ("output_blocks.6.1", "input_blocks.1.1"))
    with pytest.raises(RuntimeError, match="select no attention layer"):
        unet.char_map_plan(32, 32, 12, ("nowhere",))
    with pytest.raises(NotImplementedError, match="context of 1 tokens"):
        unet.char_map_plan(32, 32, 1)
    assert [n for n, _, _ in unet.char_map_blocks()] == ["output_blocks.6.1.transformer_blocks.0.t_attn"]      # the shipped selection
    assert all(blk.char_map is None for _, blk, _ in unet.char_map_blocks(("input_blocks", "middle_block", "output_blocks")))


def _many(engine, cuda, name, detailed, H, W, in_flight, steps=4, batches=2, per=2, **kw):
    from udifftext_amd import config as C, pipeline, synth
    cfgs = C.default_runtime_config(steps=steps, batch_size=per, noise_iters=0, detailed=detailed)
    bs = [synth.synthetic_batch(per, H, W, 4, seed=40 + i) for i in range(batches)]
    seeds = [[900 + per * i + j for j in range(per)] for i in range(batches)]
    sampler = pipeline.init_sampling(steps, 5.0, cuda, sampler=name)
    outs = pipeline.predict_many(cfgs, engine, sampler, bs, in_flight=in_flight, fuse=1, image_seeds=seeds, **kw)
    return outs, sampler, bs


@pytest.mark.parametrize("name,H,W,in_flight,dual", [("euler", 128, 128, 2, False), ("heun", 128, 128, 2, False),
                                                     ("euler", 128, 128, 1, True), ("heun", 128, 128, 1, True),
                                                     ("heun", 128, 192, 1, False), ("euler", 128, 192, 2, False)])
def test_the_image_does_not_change(engine, cuda, monkeypatch, name, H, W, in_flight, dual):
    """predict_many with and without cfgs.detailed: samples and z bit-equal — on the lanes (in_flight 2), alone on one stream and alone
    on the two-stream runner (the conditional half writes the maps from the side stream), square and not"""
    from sgm.modules.diffusionmodules import sampling
    monkeypatch.setattr(sampling, "DUAL_STREAM", dual)
    plain, _, _ = _many(engine, cuda, name, False, H, W, in_flight)
    outs, sampler, _ = _many(engine, cuda, name, True, H, W, in_flight)
    assert sampler.use_graphs, "graph capture fell back to eager launches"
    if in_flight == 1:
        runner = next(iter(sampler._graphed.values()))
        assert runner.st.dual == dual and runner.maps is not None
    assert len(outs) == len(plain) == 2
    h, w = H // 16, W // 16                                                  # output_blocks.6.1: half the latent's grid
    for k, ((img, z, maps), (img0, z0)) in enumerate(zip(outs, plain)):
        assert torch.equal(z, z0) and torch.equal(img, img0), f"{name} {H}x{W} in_flight {in_flight}: batch {k} changed with detailed"
        assert maps.shape == (2, 12, h, w) and maps.dtype == torch.float32 and bool(torch.isfinite(maps).all())
        assert float((maps.double().sum(dim=1) - 1).abs().max()) <= 12 * 2.0 ** -9
        assert not torch.equal(maps[0], maps[1])


@pytest.mark.parametrize("name", ["dpmpp2m", "euler_a", "dpmpp2s_a", "linear_multistep", "heun"])
def test_every_sampler_hands_back_maps(engine, cuda, name):
    """``sampler(..., detailed=True)`` of the five samplers that used to refuse: x as without, the maps on ``last_char_maps``"""
    from udifftext_amd import pipeline, synth
    batch, buc = pipeline.prepare_batch(synth.synthetic_batch(2, 128, 128, 4, seed=5), cuda)
    torch.manual_seed(3)
    c, uc = engine.conditioner.get_unconditional_conditioning(batch, batch_uc=buc, force_uc_zero_embeddings=["label"])
    x0 = torch.randn((2, 4, 16, 16), generator=torch.Generator().manual_seed(8)).to(cuda)
    s = pipeline.init_sampling(4, 5.0, cuda, sampler=name)
    noise = s.draw_step_noise(x0.shape, x0.device)
    z0 = s(engine, x0.clone(), cond=c, uc=uc, noise=noise)
    z1 = s(engine, x0.clone(), cond=c, uc=uc, noise=noise, detailed=True)
    assert torch.equal(z0, z1), f"{name}: the latent changed with detailed"
    maps = s.last_char_maps
    assert maps.shape == (2, 12, 8, 8) and float((maps.double().sum(dim=1) - 1).abs().max()) <= 12 * 2.0 ** -9
    with pytest.raises(ValueError, match="init_step"):
        s(engine, x0.clone(), cond=c, uc=uc, noise=noise, detailed=True, init_step=3)
    # eager launches (graphs off) hand back the same
    e = pipeline.init_sampling(4, 5.0, cuda, sampler=name)
    e.use_graphs = False
    z2 = e(engine, x0.clone(), cond=c, uc=uc, noise=noise, detailed=True)
    assert torch.equal(z2, z1) and torch.equal(e.last_char_maps, maps), f"{name}: eager and replayed runs differ"


def test_maps_do_not_depend_on_the_batch(engine, cuda):
    """image 1 of a fused batch of 4 against the same image sampled alone under its per-image seed: the project's stated batch
    dependence (1.1e-2 in bf16) — the latent itself moves by that much"""
    from udifftext_amd import config as C, parallel, pipeline, synth
    gb = synth.synthetic_batch(4, 128, 128, 4, seed=21)
    seeds = [31, 32, 33, 34]
    s = pipeline.init_sampling(4, 5.0, cuda)
    cfg = lambda n: C.default_runtime_config(steps=4, batch_size=n, noise_iters=0, detailed=True)
    (_, _, m4), = pipeline.predict_many(cfg(4), engine, s, [_copy(gb)], in_flight=1, fuse=1, image_seeds=[seeds])
    (_, _, m1), = pipeline.predict_many(cfg(1), engine, s, [parallel.slice_batch(gb, 1, 2)], in_flight=1, fuse=1, image_seeds=[seeds[1:2]])
    assert m4.shape == (4, 12, 8, 8) and m1.shape == (1, 12, 8, 8)
    _hold("maps of image 1: batch of 4 vs alone", m4[1:2], m1, 1.1e-2)
    assert _rel(m4[0:1], m1) > 2 * _rel(m4[1:2], m1)                          # (another image's maps are farther away)


def test_maps_agree_with_the_unfused_route(engine, cuda, tmp_path, monkeypatch):
    """one Euler image through ``predict`` with detailed (the unfused map-emitting step, save_segment_map's array) and through
    predict_many: each side within the single-map bound of the truth, the steps before the middle one are the same fast steps"""
    from udifftext_amd import config as C, pipeline, synth
    monkeypatch.chdir(tmp_path)
    steps = 4
    batch = synth.synthetic_batch(1, 128, 128, 4, seed=9)
    label, name = batch["label"][0], batch["name"][0]
    cfgs = C.default_runtime_config(steps=steps, batch_size=1, noise_iters=0, detailed=True)
    sampler = pipeline.init_sampling(steps, 5.0, cuda)
    torch.manual_seed(11)
    pipeline.predict(cfgs, engine, sampler, _copy(batch))
    seg = np.load(tmp_path / "temp" / "seg_map" / f"seg_{name}.npy")
    torch.manual_seed(11)
    (_, _, maps), = pipeline.predict_many(cfgs, engine, sampler, [_copy(batch)], in_flight=1, fuse=1)
    assert seg.shape == (len(label), 8, 8) and maps.shape == (1, 12, 8, 8)
    _hold("predict_many maps vs predict's seg_map (unfused route)", maps[0, :len(label)], torch.from_numpy(seg), 2 * 3e-2)
    paths = pipeline.save_char_maps(maps, [label], [name], out_dir=str(tmp_path / "many"))
    assert np.load(paths[0]).shape == seg.shape


def test_resized_maps_are_kernel_two_applied(engine, cuda):
    from udifftext_amd import ops
    outs, _, _ = _many(engine, cuda, "euler", True, 128, 192, 2)
    big, _, _ = _many(engine, cuda, "euler", True, 128, 192, 2, map_size="image")
    for (img, _, maps), (_, _, mb) in zip(outs, big):
        assert mb.shape == (2, 12, 128, 192) == maps.shape[:2] + img.shape[-2:]
        assert torch.equal(mb, ops.resize_bilinear(maps, (128, 192)))
    small, _, _ = _many(engine, cuda, "euler", True, 128, 192, 2, map_size=(5, 7))
    assert torch.equal(small[0][2], ops.resize_bilinear(outs[0][2], (5, 7)))


def test_with_attend_and_excite_and_through_evaluate(engine, cuda):
    from udifftext_amd import config as C, pipeline, synth
    bs = [synth.synthetic_batch(2, 128, 128, 4, seed=70 + i) for i in range(2)]
    seeds = [[1, 2], [3, 4]]

    class Predictor:                                                         # (evaluate is duck-typed: the samples go through)
        def transform_boxes(self, samples, boxes):
            return samples[:, :, :8, :8]

        def txt_of(self, x):
            return ["?"] * x.shape[0]

    for b in bs:
        b["r_bbox"] = torch.tensor([[0, 64, 0, 64]] * 2)
    cfgs = C.default_runtime_config(steps=4, batch_size=2, noise_iters=0, detailed=True)
    sampler = pipeline.init_sampling(4, 5.0, cuda)
    res = pipeline.evaluate(cfgs, engine, sampler, [_copy(b) for b in bs], Predictor(), in_flight=2, fuse=1, image_seeds=seeds,
                            return_samples=True)
    assert res["total"] == 4 and all(len(o) == 3 and o[2].shape == (2, 12, 8, 8) for o in res["outputs"])
    ref = pipeline.predict_many(cfgs, engine, sampler, [_copy(b) for b in bs], in_flight=2, fuse=1, image_seeds=seeds)
    assert all(torch.equal(a[2], b[2]) and torch.equal(a[0], b[0]) for a, b in zip(res["outputs"], ref))
    # attend-and-excite: the rows path, its maps from what the middle step cached (record_losses) or from its fused step (without)
    cfg2 = C.default_runtime_config(steps=2, batch_size=2, noise_iters=0, detailed=True, aae_enabled=True)
    s2 = pipeline.init_sampling(2, 5.0, cuda)
    for record in (True, False):
        outs = pipeline.predict_many(cfg2, engine, s2, [_copy(b) for b in bs], in_flight=1, fuse=1, image_seeds=seeds, record_losses=record)
        for img, z, maps in outs:
            assert img.shape[0] == z.shape[0] == 2 and maps.shape == (2, 12, 8, 8) and bool(torch.isfinite(maps).all())
            assert float((maps.double().sum(dim=1) - 1).abs().max()) <= 2e-3
