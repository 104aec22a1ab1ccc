"""Character attention maps at throughput, host side (no GPU):

* ``pipeline.predict_many`` with ``cfgs.detailed`` and a stub engine / sampler (the style of tests/test_parallel_cpu.py): triples in input
  order, split per batch; pairs without it; the init_step refusal before any sampler call; ``predict_sharded`` refuses;
* the plans of all six samplers carry the flag on exactly one evaluation, the first of the middle step;
* the float64 restatements the GPU tests use (tests/char_maps_ref.py) equal the reference's own reduction of full probabilities and
  ``F.interpolate(mode="bilinear", align_corners=False)``;
* ``save_char_maps`` writes the reference's file; the header declares the new entry points and ``lib.SYMBOLS`` types them.
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import udifftext_amd  # noqa: F401  (puts the sgm mirror on sys.path)
import attention_cases as K
import attention_ref as R
import char_maps_ref as M
from udifftext_amd import config as C
from udifftext_amd import lib, parallel, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_CTX, HM, WM = 5, 2, 3


# ------------------------------------------------------------------------------------------------ predict_many with stubs
class _StubConditioner:
    def get_unconditional_conditioning(self, batch, batch_uc=None, force_uc_zero_embeddings=None):
        from udifftext_amd import rng
        B = batch["image"].shape[0]
        feat = batch["image"].mean(dim=(1, 2, 3)).reshape(B, 1, 1, 1)
        return {"concat": rng.randn((B, 4, 2, 2)) + feat}, {"concat": rng.randn((B, 4, 2, 2)) + feat}


class _StubModel:
    conditioner = _StubConditioner()

    def decode_first_stage(self, z):
        return z[:, :3].repeat_interleave(2, -1).repeat_interleave(2, -2) * 0.1


def _stub_maps(x):
    """per-image maps [B, L, h, w] that identify the image they belong to"""
    ramp = torch.arange(L_CTX * HM * WM, dtype=torch.float32).reshape(1, L_CTX, HM, WM)
    return x.mean(dim=(1, 2, 3)).reshape(-1, 1, 1, 1) + ramp


class _StubSampler:
    num_sigmas = 5                                                        # 4 steps

    def __init__(self):
        self.calls = []

    def get_init_noise(self, cfgs, model, cond, batch, uc=None):
        from udifftext_amd import rng
        return rng.randn((cfgs.batch_size, 4, 2, 2))

    def char_map_step(self, init_step=0, num_steps=None):
        from sgm.modules.diffusionmodules.sampling import char_map_step
        return char_map_step(self.num_sigmas, init_step)

    def sample_in_flight(self, model, xs, conds, ucs, init_step=0, deferred_checks=None, streams=None, char_maps=False):
        self.calls.append((xs[0].shape[0], char_maps))
        zs = [x + 0.5 * c["concat"] - 0.25 * u["concat"] for x, c, u in zip(xs, conds, ucs)]
        return [(z, _stub_maps(x)) for z, x in zip(zs, xs)] if char_maps else zs


def _batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand((n, 3, 8, 8), generator=g), "label": [f"img{i}" for i in range(n)], "txt": [f"t{i}" for i in range(n)]}


def _cfgs(**kw):
    cfgs = C.default_runtime_config(steps=4, batch_size=2, noise_iters=0)
    for k, v in kw.items():
        setattr(cfgs, k, v)
    return cfgs


def _run(detailed, fuse, in_flight=2, sampler=None, **kw):
    torch.manual_seed(5)
    sm = sampler or _StubSampler()
    outs = pipeline.predict_many(_cfgs(detailed=detailed), _StubModel(), sm, [_batch(2, 300 + i) for i in range(5)], torch.device("cpu"),
                                 in_flight=in_flight, fuse=fuse, **kw)
    return outs, sm


@pytest.mark.parametrize("fuse,units", [(1, [2, 2, 2, 2, 2]), (0, [6, 4])])
def test_predict_many_detailed_returns_triples_in_input_order(fuse, units):
    plain, _ = _run(False, fuse)
    outs, sm = _run(True, fuse)
    assert [c[0] for c in sm.calls] == units and all(c[1] is True for c in sm.calls)
    assert len(outs) == len(plain) == 5
    for k, ((img, z, maps), (img0, z0)) in enumerate(zip(outs, plain)):
        assert torch.equal(img, img0) and torch.equal(z, z0), k            # the image does not depend on asking for maps
        assert maps.shape == (2, L_CTX, HM, WM) and maps.dtype == torch.float32
    # the maps of image i of batch k are those of ITS latent: the fused batch was split where the inputs were joined
    single, _ = _run(True, 1)
    for (_, _, a), (_, _, b) in zip(outs, single):
        assert torch.equal(a, b)


def test_predict_many_without_detailed_still_yields_pairs():
    outs, sm = _run(False, 0)
    assert all(isinstance(o, tuple) and len(o) == 2 for o in outs) and all(c[1] is False for c in sm.calls)
    with pytest.raises(ValueError, match="map_size"):
        _run(False, 0, map_size="image")


def test_predict_many_detailed_refuses_a_late_start_before_any_sampler_call():
    sm = _StubSampler()
    assert sm.char_map_step(2) == 2
    with pytest.raises(ValueError, match="init_step"):
        pipeline.predict_many(_cfgs(detailed=True, init_step=3), _StubModel(), sm, [_batch(2, 1)], torch.device("cpu"))
    assert sm.calls == []

    class NoMaps:
        get_init_noise = _StubSampler.get_init_noise

    with pytest.raises(NotImplementedError, match="detailed"):
        pipeline.predict_many(_cfgs(detailed=True), _StubModel(), NoMaps(), [_batch(2, 1)], torch.device("cpu"))
    with pytest.raises(ValueError, match="map_size"):
        pipeline.predict_many(_cfgs(detailed=True), _StubModel(), sm, [_batch(2, 1)], torch.device("cpu"), map_size="latent")
    assert sm.calls == []


def test_predict_sharded_refuses_detailed():
    gb = dict(_batch(4, 9), name=[str(i) for i in range(4)])
    with pytest.raises(NotImplementedError, match="detailed"):
        parallel.predict_sharded(_cfgs(detailed=True), _StubModel(), _StubSampler(), [gb], [11], dist=None, micro_batch=2,
                                 device=torch.device("cpu"))


def test_evaluate_tolerates_triples():
    class Predictor:
        def transform_boxes(self, samples, boxes):
            return samples[:, :, :2, :2]

        def txt_of(self, x):
            return ["img0"] * x.shape[0]

    batches = [dict(_batch(2, 400 + i), r_bbox=torch.tensor([[0, 2, 0, 2]] * 2)) for i in range(2)]
    torch.manual_seed(5)
    res = pipeline.evaluate(_cfgs(detailed=True), _StubModel(), _StubSampler(), batches, Predictor(), torch.device("cpu"), in_flight=1,
                            fuse=1, return_samples=True)
    assert res["total"] == 4 and res["correct"] == 2
    assert all(len(o) == 3 and o[2].shape == (2, L_CTX, HM, WM) for o in res["outputs"])


# ------------------------------------------------------------------------------------------------ plans
@pytest.mark.parametrize("steps", [4, 5])
@pytest.mark.parametrize("name", sorted(pipeline.SAMPLERS))
def test_exactly_one_evaluation_carries_the_flag(name, steps):
    from sgm.modules.diffusionmodules import sampling as S
    s = pipeline.init_sampling(steps, 5.0, "cpu", sampler=name)
    sig = s._host_sigmas()
    assert len(sig) == steps + 1
    plain, plans = s.plans(sig, 0), s.plans(sig, 0, char_maps=True)
    assert not S.plans_emit_maps(plain) and S.plans_emit_maps(plans)
    flagged = [(i, k) for i, plan in plans for k, e in enumerate(plan) if e.maps]
    assert flagged == [(steps // 2, 0)] and s.char_map_step(0) == steps // 2
    # nothing else about the plans changes, and the flag makes them another runner's key
    assert [(i, tuple(e._replace(maps=False) for e in plan)) for i, plan in plans] == plain and tuple(plans) != tuple(plain)
    assert S.plans_emit_maps(s.plans(sig, steps // 2, char_maps=True))
    with pytest.raises(ValueError, match="init_step"):
        s.plans(sig, steps // 2 + 1, char_maps=True)
    with pytest.raises(ValueError, match="init_step"):
        s.char_map_step(steps // 2 + 1)


@pytest.mark.parametrize("name", sorted(set(pipeline.SAMPLERS) - {"euler"}))
def test_detailed_needs_an_engine_and_no_longer_a_euler_sampler(name):
    s = pipeline.init_sampling(4, 5.0, "cpu", sampler=name)
    with pytest.raises(NotImplementedError, match="no engine"):
        s(None, torch.zeros((1, 4, 8, 8)), {}, {}, detailed=True)
    with pytest.raises(ValueError, match="init_step"):                        # past the engine check: the plan is made, nothing launched
        s(object(), torch.zeros((1, 4, 8, 8)), {}, {}, detailed=True, init_step=3)


# ------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("heads,B,n_tok,L,map_from", [(5, 3, 64, 12, 1), (10, 2, 32, 2, 0)])
def test_map_restatement_equals_the_reference_reduction(heads, B, n_tok, L, map_from):
    """two layers' full probabilities [b * heads, n, l] through the reference's stack / mean / reshape / mean / permute, against the two
    launches at weight 0.5 the kernel tests make (store, then accumulate)"""
    layers, maps = [], 0
    for seed in (0, 1):
        x, kv, wq, wo, gamma, beta, bias = K.tattn_inputs(heads, B, n_tok, L, seed=seed)
        t = R.tattn_prepare(kv, wq, wo, gamma, beta, heads, K.TATTN_SCALE, emulate=True)
        sc = torch.stack((t["s"], t["c"]), dim=-1)
        m, a = M.tattn_maps(x, t["A"], sc, heads, L, map_from, K.TATTN_EPS, weight=0.5)
        assert m.shape == a.shape == (B - map_from, L, n_tok) and M.rms(a) > 0 and bool((a >= m).all())
        maps = maps + m
        P, _ = M.tattn_probs(x, t["A"], sc, K.TATTN_EPS)
        assert float(P[:, :, :heads, L:].abs().max()) == 0.0                 # the padded columns hold no probability
        layers.append(P[map_from:, :, :heads, :L].permute(0, 2, 1, 3).reshape(-1, n_tok, L))      # [b * heads, n, l]
        emul = M.tattn_maps(x, t["A"], sc, heads, L, map_from, K.TATTN_EPS, weight=0.5, emulate=True)
        assert 0 < float((emul - m).abs().max()) <= 2.0 ** -9 * 0.5          # bf16 P: half an ulp of a value <= 1, per head, averaged
    ref = M.reference_reduction(layers, heads)
    assert ref.shape == maps.shape
    torch.testing.assert_close(maps, ref, rtol=0, atol=1e-15)
    torch.testing.assert_close(maps.sum(dim=1), torch.ones_like(maps[:, 0]), rtol=0, atol=1e-12)   # softmax rows sum to one


@pytest.mark.parametrize("hw,HW", [((8, 8), (64, 64)), ((8, 12), (64, 96)), ((3, 5), (7, 4)), ((1, 1), (5, 5))])
def test_bilinear_restatement_equals_interpolate(hw, HW):
    g = torch.Generator().manual_seed(hw[0] * 100 + HW[1])
    x = torch.randn((2, 3) + hw, generator=g, dtype=torch.float64)
    got, asum = M.bilinear(x, *HW)
    want = F.interpolate(x, size=HW, mode="bilinear", align_corners=False)
    torch.testing.assert_close(got, want, rtol=0, atol=1e-14)
    assert bool((asum >= got.abs() - 1e-15).all())


# ------------------------------------------------------------------------------------------------ files and ABI
def test_save_char_maps_writes_the_reference_file(tmp_path):
    maps = torch.arange(2 * 12 * 4 * 6, dtype=torch.float32).reshape(2, 12, 4, 6)
    paths = pipeline.save_char_maps(maps, ["abc", "hello"], ["n0", "n1"], out_dir=str(tmp_path))
    assert [os.path.basename(p) for p in paths] == ["seg_n0.npy", "seg_n1.npy"]
    for p, m, label in zip(paths, maps, ["abc", "hello"]):
        a = np.load(p)
        assert a.shape == (len(label), 4, 6) and a.dtype == np.float32 and np.array_equal(a, m[:len(label)].numpy())
    with pytest.raises(ValueError):
        pipeline.save_char_maps(maps, ["abc"], ["n0", "n1"], out_dir=str(tmp_path))
    with pytest.raises(ValueError):
        pipeline.save_char_maps(maps, ["a" * 13, "b"], ["n0", "n1"], out_dir=str(tmp_path))


def test_abi_declares_and_types_the_new_entry_points():
    import test_char_maps_footprint_gpu  # noqa: F401  (appends its cases to the table)
    import test_footprint_gpu as table
    text = open(os.path.join(ROOT, "include", "udt_kernels.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n in (("udt_tattn_fused_maps", 21), ("udt_resize_bilinear_f32", 8)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m and len(m.group(1).split(",")) == n == len(lib.SYMBOLS[name][1]), name
        assert name in {c for _, _, covers in table.CASES for c in covers}, name
    # the plain entry points keep their signatures: the map variant is theirs + (maps, L, map_from, weight, accumulate)
    assert len(lib.SYMBOLS["udt_tattn_fused"][1]) == 13 and len(lib.SYMBOLS["udt_tattn_fused_q8"][1]) == 16
    assert lib.SYMBOLS["udt_tattn_fused_maps"][1][:12] == lib.SYMBOLS["udt_tattn_fused"][1][:12]
    for word in ("ROUNDING (maps)", "UDT_ERR_BAD_ARG: a null maps"):
        assert word in text
