"""Every launch of the forward product OUTSIDE the five square calls of tests/test_shadow_gpu.py, teacher-forced against float64
(tests/shadow_ref.py): the rectangular plans, the VAE encoder, the conditioner and the OCR scorer.

Same rule as test_shadow_gpu.py: each ``ops`` call of a real model call is checked on the inputs the HIP path really produced, at the
shape and plan it really runs, against its own per-op bound, and every traced class 0-3 launch must belong to a checked call.  The
runs (eager, no graph capture):
  1. one sampler call at a 64 x 96 latent, B = 1 (a CFG pair): DESIGN section 12's table — lconv3 on the 8 x 8 tile at 16 x 24, the
     fifteen stream-K gemm8 convolutions of the 8 x 12 level, attn at 6144 / 1536 / 384 / 96 query rows, tattn_fused at n = 96;
  2. one sampler call at a 48 x 32 latent, B = 3 (6 samples), in bf16 and in config #5: 1536, 384, 96 and 24 rows per sample — sample
     boundaries inside every tile of the GroupNorm-statistics and row-vector epilogues;
  3. the in-flight plan at a 32 x 48 latent: 16 samples under launch_context(cu_share=2) on a side stream with its own workspace;
  4. the map-emitting path ``unet(x, t, ctx)`` at 32 x 48, B = 2: every attn_map_cache item carries the (h, w) of its token count;
  5. encode_first_stage at 512 x 512 (B = 4, the benchmark's) and at 256 x 384: the stride-2 convolutions with bottom / right padding,
     the encoder's attention_d512, quant_conv with fp32 output, posterior_sample;
  6. decode_first_stage at a 64 x 96 latent (512 x 768);
  7. conditioner.get_unconditional_conditioning on synthetic batches at 512 x 512 (B = 4) and 256 x 384 (B = 2): mask_downsample,
     embed_tokens, the label encoder's linear / xattention / layer_norm, the masked-image encoder pass;
  8. ParseqPredictor on four crops of different sizes: ViT encoder, autoregressive decoding, the refinement pass, and the
     teacher-forced decode of four labels of different lengths — masked_attention with the additive mask and with a key-padding mask
     that really pads.
No run may pass vacuously: each asserts that the ops it exists for were seen by the shadow (``Shadow.saw``).
The union of the plan families of these runs is pinned (PINNED_FAMILIES_PATHS).  Measured values next to their bounds and each run's
wall time go to the parity report that test_engine_gpu.py writes (its REPORT).
"""
import os
import time

import numpy as np
import pytest
import torch

import shadow_ref
from test_engine_gpu import REPORT          # (one parity report for the end-to-end and the per-op checks)

pytestmark = pytest.mark.gpu

# The plan families (first word of the profiler tag of each class 0-3 launch) that runs 1-8 take, as observed on the MI355X.
# A heuristic change that moves these calls off one of them or onto a new one fails test_plan_families_of_the_other_paths: if the
# move is intended, replace this set by the "observed" set that test prints (every family in it has then been shadow-checked).
PINNED_FAMILIES_PATHS = {"attn", "attn-mx8", "attn-mx8+q8", "attn512", "conv_n4", "gemm", "gemm8", "lconv3", "lconv3+up", "lean1", "lean1+q8",
                         "lean1-mx8", "lean1-mx8+q8", "lean5", "lean7", "lean7+q8", "tattn_fused", "tattn_fused+q8", "tattn_prepare",
                         "wconv3", "xattention"}

_FAMILIES: dict = {}
_OP_FAMILIES: dict = {}
_TIMES: dict = {}


@pytest.fixture(scope="module")
def engine(cuda):
    from udifftext_amd import lib, pipeline
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)
    return pipeline.build_engine(cuda)


@pytest.fixture(scope="module")
def predictor(cuda):
    import udifftext_amd  # noqa: F401
    from sgm.modules.predictors.model import ParseqPredictor
    from sgm.util import skip_param_init
    from udifftext_amd import synth
    torch.set_grad_enabled(False)
    G = np.load(os.path.join(os.path.dirname(__file__), "golden", "parseq_golden.npz"))
    keys, shapes = list(G["state_dict_keys"]), [eval(s) for s in G["state_dict_shapes"]]
    sd = {k: synth.synthetic_tensor("parseq." + k, sh) for k, sh in zip(keys, shapes)}
    with skip_param_init():
        m = ParseqPredictor(ckpt_path=None)
    missing, unexpected = m.parseq.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    return m.to(cuda).eval()


def _ctx(engine, B, seed):
    from udifftext_amd import synth
    le = engine.conditioner.embedders[0]
    ctx = le(synth.synthetic_batch(B, 512, 512, 9, seed=seed)["label"])
    return torch.cat([torch.zeros_like(ctx), ctx])


def _sampler_call(unet, x, ts, tctx, zero_rows):
    from test_engine_gpu import _sampler_call as call
    return call(unet, x, ts, tctx, zero_rows)


def _shadow(name, tmp_path, fn):
    """(test_shadow_gpu._shadow, with this module's own family and time records) -> (what fn returned, the Shadow)"""
    torch.cuda.synchronize()
    t0 = time.time()
    with shadow_ref.Shadow(name, report=REPORT, trace_dir=str(tmp_path)) as sh:
        out = fn()
        torch.cuda.synchronize()
    dt = time.time() - t0
    with open(REPORT, "a") as f:
        f.write(f"  shadow run '{name}': {dt:.1f} s\n")
    _TIMES[name] = dt
    for fam, n in sh.families.items():
        _FAMILIES[fam] = _FAMILIES.get(fam, 0) + n
    for key, n in sh.op_families.items():
        _OP_FAMILIES[key] = _OP_FAMILIES.get(key, 0) + n
    print(f"shadow '{name}': {sh.calls} calls, {sh.traced} traced launches, {dt:.1f} s, families {dict(sh.families)}")
    assert not sh.failures, f"{name}: {len(sh.failures)} ops calls off their bounds:\n  " + "\n  ".join(sh.failures[:40])
    assert sh.calls > 0
    assert sh.unchecked_launches == 0, f"{name}: {sh.unchecked_launches} class 0-3 launches outside shadow-checked ops calls"
    return out, sh


# --------------------------------------------------------------------------------------------------------- 1-4: the UNet
def test_shadow_sampler_call_at_64x96(engine, cuda, tmp_path):
    torch.manual_seed(41)
    B = 1
    tctx = _ctx(engine, B, 11)
    x = torch.randn((2 * B, 9, 64, 96), device=cuda)
    ts = torch.full((2 * B,), 441, device=cuda)
    eps, sh = _shadow("sampler call 64x96 x2", tmp_path, lambda: _sampler_call(engine.model.diffusion_model, x, ts, tctx, B))
    assert eps.shape == (2 * B, 4, 64, 96) and torch.isfinite(eps).all()
    assert sh.saw("conv2d", lambda n: n.startswith("8x12 ")) > 0, sorted(sh.seen)
    assert sh.saw("conv2d", lambda n: n.startswith("16x24 ")) > 0
    assert sh.saw("attention_rowv", lambda n: " N=6144 " in n) > 0, sorted(sh.seen)
    assert sh.saw("tattn_fused", lambda n: " N=96 " in n) > 0
    # the fifteen 3x3 convolutions of the 8 x 12 level are served by the stream-K gemm8
    assert sh.saw("conv2d", lambda n: n.startswith("8x12 ") and " k3 s1" in n) >= 15, sorted(sh.seen)
    assert sh.op_families[("conv2d", "gemm8")] >= 15, dict(sh.op_families)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "config5"])
def test_shadow_sampler_call_at_48x32(engine, cuda, tmp_path, monkeypatch, fp8):
    import sgm.modules.hipnn as H
    monkeypatch.setattr(H, "FP8_LINEARS", fp8)
    monkeypatch.setattr(H, "FP8_ATTENTION", fp8)
    torch.manual_seed(42)
    B = 3
    tctx = _ctx(engine, B, 12)
    x = torch.randn((2 * B, 9, 48, 32), device=cuda)
    ts = torch.full((2 * B,), 441, device=cuda)
    eps, sh = _shadow(f"sampler call 48x32 x6 {'config #5' if fp8 else 'bf16'}", tmp_path,
                      lambda: _sampler_call(engine.model.diffusion_model, x, ts, tctx, B))
    assert eps.shape == (2 * B, 4, 48, 32) and torch.isfinite(eps).all()
    assert sh.saw("conv2d", lambda n: n.startswith("6x4 ")) > 0, sorted(sh.seen)       # 24 rows per sample
    assert sh.saw("conv2d", lambda n: n.startswith("12x8 ")) > 0                        # 96 rows per sample
    if fp8:
        assert sh.saw("linear_mx8") > 0 and sh.saw("attention_mx8") > 0, sorted(sh.seen)
    else:
        assert sh.saw("linear_mx8") == 0 and sh.saw("attention_mx8") == 0


def test_shadow_in_flight_call_at_32x48(engine, cuda, tmp_path):
    from udifftext_amd import ops, packing
    torch.manual_seed(43)
    unet = engine.model.diffusion_model
    n = 8
    tctx = _ctx(engine, n, 13)
    x = torch.randn((2 * n, 9, 32, 48), device=cuda)
    ts = torch.full((2 * n,), 701.0, device=cuda)
    xin = ops.nchw_to_nhwc(x.float().contiguous(), packing.KPAD)
    emb = unet.time_embedding_rows(ts)
    t_kv = unet.project_context(tctx)
    s1 = torch.cuda.Stream(device=cuda)
    w1 = ops.Workspace(cuda)
    torch.cuda.synchronize()

    def run():
        with torch.cuda.stream(s1), ops.launch_context(cu_share=2, workspace=w1):
            out = unet.forward_nhwc(xin, emb, t_kv, zero_ctx_rows=n)
        torch.cuda.synchronize()
        return out
    eps, sh = _shadow("in-flight call 32x48 x16 cu_share 2", tmp_path, run)
    w1.check()
    assert torch.isfinite(eps).all()
    assert sh.saw("conv2d", lambda n: n.startswith("4x6 ")) > 0, sorted(sh.seen)


def test_shadow_map_emitting_call_at_32x48(engine, cuda, tmp_path):
    torch.manual_seed(44)
    B = 2
    tctx = _ctx(engine, B, 14)
    x = torch.randn((2 * B, 9, 32, 48), device=cuda)
    ts = torch.full((2 * B,), 300, device=cuda)
    unet = engine.model.diffusion_model
    eps, sh = _shadow("map-emitting call 32x48 x4", tmp_path, lambda: unet(x, timesteps=ts, t_context=tctx))
    assert torch.isfinite(eps).all() and len(unet.attn_map_cache) > 0
    assert sh.saw("xattention", lambda n: True) > 0
    levels = set()
    for it in unet.attn_map_cache:
        h, w = it["hw"]
        assert it["attn_map"].shape[1] == h * w and 3 * h == 2 * w, (it["name"], tuple(it["attn_map"].shape), it["hw"])
        levels.add((h, w))
    assert (32, 48) in levels and (16, 24) in levels, levels


# ---------------------------------------------------------------------------------------------------------- 5-6: the VAE
@pytest.mark.parametrize("B,H,W", [(4, 512, 512), (1, 256, 384)])
def test_shadow_vae_encode(engine, cuda, tmp_path, B, H, W):
    torch.manual_seed(45)
    img = torch.rand((B, 3, H, W), device=cuda) * 2.0 - 1.0
    z, sh = _shadow(f"encode_first_stage {H}x{W} x{B}", tmp_path, lambda: engine.encode_first_stage(img))
    assert z.shape == (B, 4, H // 8, W // 8) and torch.isfinite(z).all()
    assert sh.saw("conv2d", lambda n: " s2" in n) > 0, sorted(sh.seen)
    assert sh.saw("conv2d", lambda n: n.endswith(" f32")) > 0                           # quant_conv
    assert sh.saw("attention_d512") > 0 and sh.saw("posterior_sample") > 0, sorted(sh.seen)


def test_shadow_vae_decode_at_512x768(engine, cuda, tmp_path):
    torch.manual_seed(46)
    z = torch.randn((1, 4, 64, 96), device=cuda) * 3.0
    dec, sh = _shadow("decode_first_stage 512x768", tmp_path, lambda: engine.decode_first_stage(z))
    assert dec.shape == (1, 3, 512, 768) and torch.isfinite(dec).all()
    assert sh.saw("attention_d512", lambda n: "N=6144" in n) > 0, sorted(sh.seen)
    assert sh.saw("conv2d", lambda n: n.startswith("512x768 ")) > 0


# ---------------------------------------------------------------------------------------------------- 7: the conditioner
@pytest.mark.parametrize("B,H,W", [(4, 512, 512), (2, 256, 384)])
def test_shadow_conditioner(engine, cuda, tmp_path, B, H, W):
    from udifftext_amd import pipeline, synth
    torch.manual_seed(47)
    batch, buc = pipeline.prepare_batch(synth.synthetic_batch(B, H, W, 9, seed=15), cuda)
    (c, uc), sh = _shadow(f"conditioner {H}x{W} x{B}", tmp_path, lambda: engine.conditioner.get_unconditional_conditioning(
        batch, batch_uc=buc, force_uc_zero_embeddings=["label"]))
    assert all(torch.isfinite(v).all() for v in list(c.values()) + list(uc.values()))
    assert sh.saw("mask_downsample", lambda n: n == str((B, 1, H, W))) > 0, sorted(sh.seen)
    assert sh.saw("embed_tokens") > 0 and sh.saw("xattention") > 0 and sh.saw("layer_norm") > 0, sorted(sh.seen)
    assert sh.saw("posterior_sample") > 0 and sh.saw("attention_d512") > 0                # (the masked-image encoder pass)


# --------------------------------------------------------------------------------------------------- 8: the OCR scorer
def test_shadow_parseq_predictor(predictor, cuda, tmp_path):
    """four crops of different sizes through the full inference path — transform, ViT encoder, the autoregressive loop (additive masks
    only), the refinement pass (additive mask + key-padding mask) — and, on the same memory, the teacher-forced decode of four labels
    of different lengths: its key-padding mask differs per sample and really pads (the synthetic network rarely emits an EOS, so
    the refinement pass's mask may be all false)"""
    P = predictor.parseq
    g = torch.Generator().manual_seed(48)
    crops = [torch.rand((3, 40, 100), generator=g), torch.rand((3, 25, 90), generator=g), torch.rand((3, 32, 128), generator=g),
             torch.rand((3, 64, 48), generator=g)]
    crops = [c.to(cuda) for c in crops]
    labels = ["a", "MI355", "gfx950-hip", "UDiffText-on-CDNA4-(2026)"]
    tgt = P.tokenizer.encode(labels, device=cuda)[:, :-1]           # (the decoder's input, as in training: the last position dropped)
    Lt = tgt.shape[1]
    mask = torch.triu(torch.full((Lt, Lt), float("-inf"), device=cuda), 1)
    kpm = (tgt == P.pad_id) | (tgt == P.eos_id)
    assert Lt == 26 and sorted(int(n) for n in kpm.sum(-1)) == [0, 15, 20, 24]

    def run():
        logits = predictor(crops)
        mem = P.encode(predictor.transform(crops))
        out = P.decode(tgt, P.decoder.memory_kv(mem), mask, kpm, tgt_query_mask=mask)
        return logits, P.logits_of(out)
    (logits, tf_logits), sh = _shadow("ParseqPredictor x4", tmp_path, run)
    assert logits.shape[0] == 4 and logits.shape[2] == 95 and torch.isfinite(logits).all()
    assert tf_logits.shape == (4, Lt, 95) and torch.isfinite(tf_logits).all()
    toks = P.last_ar_tokens
    assert toks.shape[1] == logits.shape[1] >= 2
    print("decoded:", P.tokenizer.decode(logits.softmax(-1))[0])
    assert sh.saw("masked_attention", lambda n: "mask=1" in n) > 0, sorted(sh.seen)
    assert sh.saw("masked_attention", lambda n: "kpm=1" in n) > 0, sorted(sh.seen)
    assert sh.saw("masked_attention", lambda n: f"Nq={Lt} Lk={Lt} " in n and "mask=1 kpm=1" in n) > 0, sorted(sh.seen)
    assert sh.saw("masked_attention", lambda n: "Nq=128 Lk=128" in n and "mask=0 kpm=0" in n) > 0       # the ViT at 128 tokens
    assert sh.saw("linear", lambda n: n.startswith("M=512 ")) > 0                       # its linears (4 x 128 rows)


# ------------------------------------------------------------------------------------------------------- plan families
def test_plan_families_of_the_other_paths(engine, predictor, cuda, tmp_path, monkeypatch):
    """(runs last in this module) the union of plan families over runs 1-8 equals PINNED_FAMILIES_PATHS"""
    if len(_FAMILIES) == 0:
        test_shadow_sampler_call_at_64x96(engine, cuda, tmp_path)
        for fp8 in (False, True):
            test_shadow_sampler_call_at_48x32(engine, cuda, tmp_path, monkeypatch, fp8)
        test_shadow_in_flight_call_at_32x48(engine, cuda, tmp_path)
        test_shadow_map_emitting_call_at_32x48(engine, cuda, tmp_path)
        for B, H, W in ((4, 512, 512), (1, 256, 384)):
            test_shadow_vae_encode(engine, cuda, tmp_path, B, H, W)
        test_shadow_vae_decode_at_512x768(engine, cuda, tmp_path)
        for B, H, W in ((4, 512, 512), (2, 256, 384)):
            test_shadow_conditioner(engine, cuda, tmp_path, B, H, W)
        test_shadow_parseq_predictor(predictor, cuda, tmp_path)
    from test_shadow_gpu import PINNED_FAMILIES
    observed = sorted(_FAMILIES)
    with open(REPORT, "a") as f:
        f.write("# shadow paths: plan families over runs 1-8 (launches; * = not among the five square runs' families)\n")
        for fam in observed:
            f.write(f"  {fam:24s} {_FAMILIES[fam]:6d}{' *' if fam not in PINNED_FAMILIES else ''}\n")
        f.write("  plans " + ", ".join(f"{op}:{fam} {n}" for (op, fam), n in sorted(_OP_FAMILIES.items())) + "\n")
        f.write(f"# shadow paths: {len(_TIMES)} runs, {sum(_TIMES.values()):.1f} s in all\n")
    print("observed plan families:", observed)
    print("first shadow-checked here:", sorted(set(observed) - set(PINNED_FAMILIES)))
    print(f"shadow paths: {len(_TIMES)} runs, {sum(_TIMES.values()):.1f} s in all")
    assert PINNED_FAMILIES_PATHS is not None and set(observed) == set(PINNED_FAMILIES_PATHS), \
        f"plan families changed: observed {observed}, pinned {sorted(PINNED_FAMILIES_PATHS or [])}"
