"""Rectangular images (H != W), host side: the torch restatement of the map consumers against the oracle at h == w, the ``hw`` key of
the attention-map items, the layer-selection rule, the argument checks of the ``_hw`` ops and ``predict_many`` over mixed sizes."""
import pytest
import torch

import rect_ref
from oracle import sampling as osamp, training as otrain
from test_parallel_cpu import _StubModel, _StubSampler


def _probs(g, b, heads, n, L=12):
    return torch.softmax(torch.randn((b * heads, n, L), generator=g) * 2.0, dim=-1)


@pytest.mark.parametrize("B,reps,heads,size", [(1, 1, 5, 16), (2, 1, 10, 32), (1, 3, 5, 24)])
def test_restatement_equals_the_oracle_on_square_maps(B, reps, heads, size):
    """tests/rect_ref.py at h == w against oracle.sampling.min_local_loss / oracle.training.local_loss (pinned to the reference by
    tests/test_oracle_golden.py), on random probabilities, to fp32 rounding; two layers so that the mean over layers is covered.
    (reps > 1 with B == 1: the oracle broadcasts the one mask over the candidates, the restatement tiles it.)"""
    g = torch.Generator().manual_seed(100 * size + B)
    gk = osamp.gaussian_kernel(3, 1.0, 12)
    mask = (torch.rand((B, 1, 64, 64), generator=g) > 0.5).float()
    segm = torch.zeros((B, 12)); segm[:, :5] = 1.0
    maps = []
    for k, s in enumerate((size, size // 2)):
        maps.append({"name": f"b{k}.t_attn", "heads": heads, "size": s, "hw": (s, s), "attn_map": _probs(g, B * reps, heads, s * s)})
    got = rect_ref.min_local_loss(maps, mask, segm, gk, 8)
    ref = osamp.min_local_loss(maps, mask, segm, gk, 8)
    assert got.shape == (B * reps,)
    torch.testing.assert_close(got, ref, rtol=1e-6, atol=0)
    if reps == 1:
        seg = (torch.rand((B, 12, 64, 64), generator=g) > 0.6).float()
        torch.testing.assert_close(rect_ref.local_loss(maps, seg, segm, gk, 8), otrain.local_loss(maps, seg, segm, gk, 8), rtol=1e-6, atol=0)
    # the selection: with the default threshold the 16-wide layer counts, the 8-wide one does not — in both
    if size == 16:
        torch.testing.assert_close(rect_ref.min_local_loss(maps, mask, segm, gk), osamp.min_local_loss(maps, mask, segm, gk), rtol=1e-6, atol=0)


@pytest.mark.parametrize("hw,scored", [((64, 64), True), ((16, 16), True), ((8, 8), False), ((16, 24), True), ((24, 16), True),
                                       ((32, 48), True), ((64, 96), True), ((96, 64), True), ((8, 12), False), ((12, 36), False),
                                       ((36, 12), False), ((15, 120), False), ((16, 120), True)])
def test_a_layer_is_scored_when_its_shorter_side_reaches_min_attn_size(hw, scored):
    """min(h, w) >= min_attn_size (16): the reference's rule for h == w, and never a 3x3 blur + mask over a map fewer than 16 pixels
    high or wide — 12x36 has int(sqrt(h w)) = 20 but is not scored"""
    from sgm.modules.diffusionmodules.loss import FullLoss
    assert FullLoss.scores_map(type("L", (), {"min_attn_size": 16})(), hw) is scored
    assert rect_ref.scores_map(hw, 16) is scored


def test_levels_scored_for_the_fixture_shapes():
    """the four levels of a latent (x1, x1/2, x1/4, x1/8): 64x96 scores its first three as 64x64 does; 32x48 and 48x32 the first two"""
    for (h, w), n in (((64, 96), 3), ((96, 64), 3), ((64, 64), 3), ((32, 48), 2), ((48, 32), 2), ((32, 32), 2), ((16, 24), 1)):
        levels = [(h >> k, w >> k) for k in range(4)]
        assert [rect_ref.scores_map(l) for l in levels] == [True] * n + [False] * (4 - n)
        assert all(rect_ref.scores_map(l) == (int((l[0] * l[1]) ** 0.5) >= 16) for l in levels)     # both readings agree here


def test_map_items_carry_hw_and_keep_size(monkeypatch):
    """CrossAttention records (h, w) next to the reference's ``size = int(n ** 0.5)``; bare token rows can only mean a square map"""
    import sgm.modules.hipnn as H
    from sgm.modules import attention as A
    from sgm.util import skip_param_init
    monkeypatch.setattr(H.Linear, "forward", lambda self, x, residual=None, out=None, **k: torch.zeros((x.shape[0], self.out_features)))
    monkeypatch.setattr(A.ops, "linear", lambda x, w, *a, **k: torch.zeros((x.shape[0], 256)))
    monkeypatch.setattr(A.ops, "xattention", lambda q, k, v, heads, dh, scale, probs=None: torch.zeros_like(q))
    with skip_param_init():
        ca = A.CrossAttention(128, context_dim=64, heads=2, dim_head=64)
    monkeypatch.setattr(ca, "packed", lambda: None)
    ca.attn_map_cache = {"name": "x.t_attn", "heads": 2, "size": None, "hw": None, "attn_map": None}
    ctx = torch.zeros((1, 12, 64))
    ca(torch.zeros((1, 24, 128)), context=ctx, emit_map=True, hw=(4, 6))
    assert ca.attn_map_cache["hw"] == (4, 6) and ca.attn_map_cache["size"] == 4
    assert tuple(ca.attn_map_cache["attn_map"].shape) == (2, 24, 12)
    ca(torch.zeros((1, 24, 128)), context=ctx, emit_map=True, hw=(6, 4))
    assert ca.attn_map_cache["hw"] == (6, 4) and ca.attn_map_cache["size"] == 4
    ca(torch.zeros((1, 16, 128)), context=ctx, emit_map=True)
    assert ca.attn_map_cache["hw"] == (4, 4) and ca.attn_map_cache["size"] == 4
    with pytest.raises(ValueError):
        ca(torch.zeros((1, 24, 128)), context=ctx, emit_map=True)                   # 24 tokens, no geometry: not guessed
    with pytest.raises(ValueError):
        ca(torch.zeros((1, 24, 128)), context=ctx, emit_map=True, hw=(5, 5))
    assert A.map_hw(1536, (32, 48)) == (32, 48) and A.map_hw(1024) == (32, 32)


def test_unet_cache_items_have_the_hw_key():
    from udifftext_amd import config as C
    from sgm.util import instantiate_from_config, skip_param_init
    with skip_param_init():
        unet = instantiate_from_config(C.default_model_config().model).model.diffusion_model
    assert len(unet.attn_map_cache) == 16
    assert all(set(item) >= {"name", "heads", "size", "hw", "attn_map"} and item["hw"] is None for item in unet.attn_map_cache)


def test_hw_ops_refuse_maps_that_do_not_hold_h_times_w_tokens():
    """n != h * w would be scored on a wrong row pitch (39 x 39 for a 32x48 map through the old entry points): ValueError, before any
    launch"""
    from udifftext_amd import ops
    heads = 5
    probs = torch.zeros((heads, 1536, 12))
    mask, segm, gk, loss = torch.zeros((1, 1, 64, 96)), torch.zeros((1, 12)), torch.zeros((9,)), torch.zeros((1,))
    seg = torch.zeros((1, 12, 64, 96))
    for hw in ((39, 39), (32, 32), (48, 48), (0, 1536), (32, -48)):
        with pytest.raises(ValueError):
            ops.local_loss_accumulate_hw(probs, mask, segm, gk, loss, heads, hw)
        with pytest.raises(ValueError):
            ops.local_loss_bwd_hw(probs, mask, segm, gk, torch.zeros_like(probs), loss, heads, hw, 1.0)
        with pytest.raises(ValueError):
            ops.local_loss_seg_bwd_hw(probs, seg, segm, gk, torch.zeros_like(probs), loss, heads, hw, 1.0)


def test_hw_symbols_are_declared_with_h_and_w():
    from udifftext_amd import lib
    for old, new in (("udt_local_loss_tiled", "udt_local_loss_tiled_hw"), ("udt_local_loss_bwd", "udt_local_loss_bwd_hw"),
                     ("udt_local_loss_seg_bwd", "udt_local_loss_seg_bwd_hw")):
        extra = 2 if new == "udt_local_loss_tiled_hw" else 1           # (h, w for size; the forward also takes the scratch)
        assert len(lib.SYMBOLS[new][1]) == len(lib.SYMBOLS[old][1]) + extra


# ---- pipeline.predict_many over mixed image sizes (host logic, stub engine as tests/test_parallel_cpu.py) -------------------------
class _SizedConditioner:
    def get_unconditional_conditioning(self, batch, batch_uc=None, force_uc_zero_embeddings=None):
        from udifftext_amd import rng
        B, _, H, W = batch["image"].shape
        feat = batch["image"].mean(dim=(1, 2, 3)).reshape(B, 1, 1, 1)
        return {"concat": rng.randn((B, 4, H // 8, W // 8)) + feat}, {"concat": rng.randn((B, 4, H // 8, W // 8)) + feat}


class _SizedModel(_StubModel):
    conditioner = _SizedConditioner()


class _SizedSampler(_StubSampler):
    calls = []

    def get_init_noise(self, cfgs, model, cond, batch, uc=None):
        from udifftext_amd import rng
        return rng.randn(tuple(cond["concat"].shape))

    def sample_in_flight(self, model, xs, conds, ucs, init_step=0, deferred_checks=None, streams=None):
        type(self).calls.append(tuple(xs[0].shape))
        return super().sample_in_flight(model, xs, conds, ucs, init_step, deferred_checks, streams)


def _sized_batch(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand((n, 3, H, W), generator=g), "label": [f"img{i}" for i in range(n)], "txt": ["" for _ in range(n)],
            "target_size_as_tuple": torch.tensor([[H, W]] * n)}


def test_predict_many_fuses_only_batches_of_one_image_size():
    from udifftext_amd import config as C, pipeline
    sizes = [(256, 256), (256, 256), (256, 384), (256, 384), (256, 384), (256, 256), (384, 256)]
    mk = lambda: [_sized_batch(2, H, W, 50 + i) for i, (H, W) in enumerate(sizes)]
    cfgs = C.default_runtime_config(steps=4, batch_size=2, noise_iters=0)
    _SizedSampler.calls = []
    torch.manual_seed(3)
    outs = pipeline.predict_many(cfgs, _SizedModel(), _SizedSampler(), mk(), torch.device("cpu"), in_flight=2, fuse=0)
    # 7 batches on 2 lanes: up to 4 per sampling batch, cut where the size changes
    assert _SizedSampler.calls == [(4, 4, 32, 32), (6, 4, 32, 48), (2, 4, 32, 32), (2, 4, 48, 32)]
    torch.manual_seed(3)
    seq = pipeline.predict_many(cfgs, _SizedModel(), _SizedSampler(), mk(), torch.device("cpu"), in_flight=1, fuse=1)
    assert len(outs) == len(sizes)
    for (img, z), (img1, z1), (H, W) in zip(outs, seq, sizes):
        assert tuple(z.shape) == (2, 4, H // 8, W // 8) and tuple(img.shape) == (2, 3, H // 4, W // 4)   # (the stub decoder: x2)
        assert torch.equal(img, img1) and torch.equal(z, z1)                                             # input order, per-batch draws
    with pytest.raises(ValueError):
        pipeline.predict_many(cfgs, _SizedModel(), _SizedSampler(), mk(), torch.device("cpu"), in_flight=2, fuse=2)
    # one size: automatic fusing groups exactly as before
    _SizedSampler.calls = []
    pipeline.predict_many(cfgs, _SizedModel(), _SizedSampler(), [_sized_batch(2, 256, 384, i) for i in range(5)], torch.device("cpu"),
                          in_flight=2, fuse=0)
    assert _SizedSampler.calls == [(6, 4, 32, 48), (4, 4, 32, 48)]
