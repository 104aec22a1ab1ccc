"""Rectangular images (H != W) on the MI355X path, ``pytest -m gpu``, everything through the C ABI.

  * the ``_hw`` local-loss kernels (forward score, its gradient, the training step's ``seg`` form) against the torch restatement
    tests/rect_ref.py and its autograd; old and new entry points bit-equal at h == w;
  * r1 / r2 / r3 of tests/golden/rect_golden.npz (the REAL reference at 256x384, 384x256, 512x768): conditioner, one UNet call, the
    VAE, the 10-step latent and the decoded image; graph replay, predict_many over mixed sizes;
  * the consumers of the text-attention maps at H != W, where the reference raises: noise search, reverse pass, attend-and-excite,
    the ``detailed`` dumps — against the restatement / the CPU oracle.

Every tolerance is the one the square counterpart states (tests/test_engine_gpu.py, tests/test_backward_gpu.py): the arithmetic is
the same.  single network call rel_rms <= 2e-2, rel_max <= 8e-2; maps 3e-2; 10-step latent 6e-2; decoded image 4e-2; predict_many vs
predict 3e-2; local-loss kernels on given probabilities: loss rtol 1e-5 / atol 1e-6, gradients rtol 1e-5 / atol 1e-8; whole-UNet
reverse pass 3e-2.
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import rect_ref
from oracle import sampling as osamp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _metrics(got, ref):
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    err = (got - ref)
    rms = ref.pow(2).mean().sqrt().item()
    return err.pow(2).mean().sqrt().item() / max(rms, 1e-30), err.abs().max().item() / max(ref.abs().max().item(), 1e-30)


def _check(name, got, ref, rel_rms, rel_max=None):
    r, m = _metrics(got, ref)
    print(f"{name}: rel_rms {r:.3e} (tol {rel_rms:.1e}) rel_max {m:.3e}")
    assert r <= rel_rms, f"{name}: rel_rms {r:.3e} > {rel_rms}"
    if rel_max is not None:
        assert m <= rel_max, f"{name}: rel_max {m:.3e} > {rel_max}"


@pytest.fixture(scope="module")
def rg():
    return np.load(os.path.join(GOLD, "rect_golden.npz"))


@pytest.fixture(scope="module")
def engine(cuda):
    from udifftext_amd import lib, pipeline
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)
    return pipeline.build_engine(cuda)


@pytest.fixture(scope="module")
def ops(cuda):
    from udifftext_amd import lib, ops
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)
    return ops


def _cond(engine, cuda, H, W, n_chars, seed, batch_size=1, torch_seed=1234):
    from udifftext_amd import pipeline, synth
    batch = synth.synthetic_batch(batch_size, H, W, n_chars, seed=seed)
    torch.manual_seed(torch_seed)
    batch, buc = pipeline.prepare_batch(batch, cuda)
    c, uc = engine.conditioner.get_unconditional_conditioning(batch, batch_uc=buc, force_uc_zero_embeddings=["label"])
    return batch, c, uc


# ------------------------------------------------------------------------------------------------ kernels
HW_CASES = [(16, 24), (24, 16), (32, 48), (64, 96), (96, 64)]


def _kernel_inputs(h, w, heads, B, reps, seed):
    g = torch.Generator().manual_seed(seed)
    n, L, seg_l = h * w, 12, 12
    probs = torch.softmax(torch.randn((B * reps * heads, n, L), generator=g) * 2.0, dim=-1)
    mask = (torch.rand((B, 1, 8 * h, 8 * w), generator=g) > 0.5).float()
    segm = torch.zeros((B, seg_l))
    segm[:, :5] = 1.0
    gk = osamp.gaussian_kernel(3, 1.0, 12)
    return probs, mask, segm, gk


@pytest.mark.parametrize("heads", [5, 10])
@pytest.mark.parametrize("h,w", HW_CASES)
def test_local_loss_hw_forward_and_backward_vs_restatement(ops, cuda, h, w, heads):
    """udt_local_loss_tiled_hw and udt_local_loss_bwd_hw on h x w maps with tiled candidates (n_samples = 3 * mask_batch, mask_batch 2;
    image-sized masks, so the per-axis nearest resize is exercised) against tests/rect_ref.py and its autograd"""
    B, reps = 2, 3
    probs, mask, segm, gk = _kernel_inputs(h, w, heads, B, reps, 1000 * h + w + heads)
    item = lambda t: [{"name": "x.t_attn", "heads": heads, "size": int((h * w) ** 0.5), "hw": (h, w), "attn_map": t}]
    with torch.enable_grad():
        t = probs.clone().requires_grad_(True)
        ll = rect_ref.min_local_loss(item(t), mask, segm, gk, 1)
        (ref,) = torch.autograd.grad(ll.sum(), [t])
    dev = cuda
    gk9 = gk[0, 0].reshape(9).contiguous().to(dev)
    pd, md, sd = probs.to(dev), mask.to(dev), segm.to(dev)
    fwd = torch.zeros((B * reps,), device=dev)
    ops.local_loss_accumulate_hw(pd, md, sd, gk9, fwd, heads, (h, w))
    dp = torch.zeros_like(pd)
    loss = torch.zeros((B * reps,), device=dev)
    ops.local_loss_bwd_hw(pd, md, sd, gk9, dp, loss, heads, (h, w), 1.0)
    print(f"local loss {h}x{w} heads {heads}: fwd max err {(fwd.cpu() - ll).abs().max().item():.3e}, "
          f"grad max err {(dp.cpu() - ref).abs().max().item():.3e} of {ref.abs().max().item():.3e}")
    assert torch.allclose(fwd.cpu(), ll, rtol=1e-5, atol=1e-6)
    assert torch.equal(loss, fwd)                                    # the same kernels score both
    assert torch.allclose(dp.cpu(), ref, rtol=1e-5, atol=1e-8)
    assert int((ref != 0).sum()) > 0
    # accumulation: a second layer adds to the same loss
    ops.local_loss_accumulate_hw(pd, md, sd, gk9, fwd, heads, (h, w))
    assert torch.allclose(fwd.cpu(), 2 * ll, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("heads", [5, 10])
@pytest.mark.parametrize("h,w", HW_CASES)
def test_local_loss_seg_hw_vs_restatement(ops, cuda, h, w, heads):
    """udt_local_loss_seg_bwd_hw (the training step's get_local_loss and its gradient) on h x w maps"""
    B = 2
    g = torch.Generator().manual_seed(77 * h + w + heads)
    probs = torch.softmax(torch.randn((B * heads, h * w, 12), generator=g) * 2.0, dim=-1)
    seg = (torch.rand((B, 12, 8 * h, 8 * w), generator=g) > 0.6).float()
    segm = torch.zeros((B, 12))
    segm[:, :5] = 1.0
    gk = osamp.gaussian_kernel(3, 1.0, 12)
    with torch.enable_grad():
        t = probs.clone().requires_grad_(True)
        ll = rect_ref.local_loss([{"name": "x.t_attn", "heads": heads, "hw": (h, w), "attn_map": t}], seg, segm, gk, 1)
        (ref,) = torch.autograd.grad(ll.sum() * 0.37, [t])
    dev = cuda
    dp = torch.zeros_like(probs).to(dev)
    loss = torch.zeros((B,), device=dev)
    ops.local_loss_seg_bwd_hw(probs.to(dev), seg.to(dev), segm.to(dev), gk[0, 0].reshape(9).contiguous().to(dev), dp, loss, heads, (h, w),
                              0.37)
    print(f"seg local loss {h}x{w} heads {heads}: loss max err {(loss.cpu() - ll).abs().max().item():.3e}, "
          f"grad max err {(dp.cpu() - ref).abs().max().item():.3e} of {ref.abs().max().item():.3e}")
    assert torch.allclose(loss.cpu(), ll, rtol=1e-5, atol=1e-6)
    assert torch.allclose(dp.cpu(), ref, rtol=1e-5, atol=1e-8) and int((ref != 0).sum()) > 0


@pytest.mark.parametrize("h,w", [(16, 24), (96, 64)])
def test_local_loss_hw_takes_the_first_extremum(ops, cuda, h, w):
    """exact ties: two identical isolated spikes (the blur adds exact zeros around them) in the maps of two identical tokens — the
    arg-max is the spike with the lower row-major index y * w + x, the arg-min the lower token, as torch.max / torch.min"""
    heads, L = 5, 12
    n = h * w
    first, second = 2 * w + 3, (h - 3) * w + (w - 2)
    probs = torch.zeros((heads, n, L))
    probs[:, first, :2] = 0.5
    probs[:, second, :2] = 0.5
    mask = torch.ones((1, 1, 8 * h, 8 * w))
    segm = torch.zeros((1, L))
    segm[:, :2] = 1.0
    gk = osamp.gaussian_kernel(3, 1.0, 12)
    with torch.enable_grad():
        t = probs.clone().requires_grad_(True)
        ll = rect_ref.min_local_loss([{"name": "x.t_attn", "heads": heads, "hw": (h, w), "attn_map": t}], mask, segm, gk, 1)
        (ref,) = torch.autograd.grad(ll.sum(), [t])
    dev = cuda
    dp = torch.zeros_like(probs).to(dev)
    loss = torch.zeros((1,), device=dev)
    ops.local_loss_bwd_hw(probs.to(dev), mask.to(dev), segm.to(dev), gk[0, 0].reshape(9).contiguous().to(dev), dp, loss, heads, (h, w), 1.0)
    dp = dp.cpu()
    assert torch.allclose(loss.cpu(), ll, rtol=1e-5, atol=1e-6)
    centre = float(-gk[0, 0, 1, 1] / heads)
    assert dp[0, first, 0].item() == pytest.approx(centre, rel=1e-6) and dp[0, first - w, 0].item() != 0 and dp[0, first + 1, 0].item() != 0
    assert not bool(dp[:, second - w - 1:second + w + 2].any()) and not bool(dp[:, :, 1:].any())
    assert int((dp != 0).sum()) == 9 * heads
    assert torch.allclose(dp, ref, rtol=1e-5, atol=1e-8)


@pytest.mark.parametrize("size", [16, 32, 64])
def test_old_and_new_entry_points_are_bit_equal_on_square_maps(ops, cuda, size):
    """udt_local_loss_tiled / _bwd / _seg_bwd (size) against the _hw entry points at h = w = size: the same bits"""
    heads, B, reps = 5, 2, 3
    probs, mask, segm, gk = _kernel_inputs(size, size, heads, B, reps, 31 * size)
    dev = cuda
    gk9 = gk[0, 0].reshape(9).contiguous().to(dev)
    pd, md, sd = probs.to(dev), mask.to(dev), segm.to(dev)
    a, b = torch.zeros((B * reps,), device=dev), torch.zeros((B * reps,), device=dev)
    ops.local_loss_accumulate(pd, md, sd, gk9, a, heads, size)
    ops.local_loss_accumulate_hw(pd, md, sd, gk9, b, heads, (size, size))
    assert torch.equal(a, b) and bool(a.abs().sum() > 0)
    da, db = torch.zeros_like(pd), torch.zeros_like(pd)
    la, lb = torch.zeros_like(a), torch.zeros_like(a)
    ops.local_loss_bwd(pd, md, sd, gk9, da, la, heads, size, 0.25)
    ops.local_loss_bwd_hw(pd, md, sd, gk9, db, lb, heads, (size, size), 0.25)
    assert torch.equal(da, db) and torch.equal(la, lb) and torch.equal(la, a) and bool(da.abs().sum() > 0)
    g = torch.Generator().manual_seed(size)
    seg = (torch.rand((B * reps, 12, 64, 64), generator=g) > 0.6).float().to(dev)
    sm = sd.tile((reps, 1)).contiguous()
    da.zero_(); db.zero_(); la.zero_(); lb.zero_()
    ops.local_loss_seg_bwd(pd, seg, sm, gk9, da, la, heads, size, 0.37)
    ops.local_loss_seg_bwd_hw(pd, seg, sm, gk9, db, lb, heads, (size, size), 0.37)
    assert torch.equal(da, db) and torch.equal(la, lb) and bool(da.abs().sum() > 0)


def test_hw_entry_points_refuse_bad_shapes_through_the_c_abi(ops, cuda):
    """h * w above the LDS bound (120 * 120) answers UDT_ERR_BAD_SHAPE (lib.check: ValueError); 100 x 144 = 14400 is inside it"""
    heads = 1
    for (h, w), ok in (((100, 144), True), ((121, 120), False), ((8, 1801), False)):
        probs = torch.softmax(torch.randn((heads, h * w, 12), device=cuda), dim=-1)
        mask, segm = torch.ones((1, 1, h, w), device=cuda), torch.ones((1, 12), device=cuda)
        gk9 = osamp.gaussian_kernel(3, 1.0, 12)[0, 0].reshape(9).contiguous().to(cuda)
        loss = torch.zeros((1,), device=cuda)
        if ok:
            ops.local_loss_accumulate_hw(probs, mask, segm, gk9, loss, heads, (h, w))
            assert bool(torch.isfinite(loss).all()) and float(loss) < 0
        else:
            with pytest.raises(ValueError, match="unsupported shape"):
                ops.local_loss_accumulate_hw(probs, mask, segm, gk9, loss, heads, (h, w))


# ------------------------------------------------------------------------------------------------ r1 / r2: the reference at 32x48, 48x32
@pytest.mark.parametrize("case,H,W", [("r1", 256, 384), ("r2", 384, 256)])
def test_conditioner_unet_call_and_sampling_vs_reference_golden(engine, rg, cuda, case, H, W):
    from udifftext_amd import config as C, ops, pipeline
    h, w = H // 8, W // 8
    batch, c, uc = _cond(engine, cuda, H, W, 4, 0)
    assert c["concat"].shape == (1, 5, h, w) and uc["t_crossattn"].abs().max().item() == 0.0
    _check(f"{case} conditioner c.concat vs reference", c["concat"].cpu(), rg[f"{case}_c_concat"], 2e-2, 8e-2)
    _check(f"{case} conditioner uc.concat vs reference", uc["concat"].cpu(), rg[f"{case}_uc_concat"], 2e-2, 8e-2)
    _check(f"{case} conditioner c.t_crossattn vs reference", c["t_crossattn"][:, :, ::16].cpu(), rg[f"{case}_c_txt_sub"], 2e-2, 8e-2)
    np.testing.assert_allclose(c["concat"][:, :1].cpu().numpy(), rg[f"{case}_c_concat"][:, :1], atol=1e-6)   # mask: exact
    # one UNet call on the REFERENCE's conditioning
    x7 = torch.from_numpy(rg[f"{case}_x"]).to(cuda)
    ucc, cc = torch.from_numpy(rg[f"{case}_uc_concat"]).to(cuda), torch.from_numpy(rg[f"{case}_c_concat"]).to(cuda)
    le = engine.conditioner.embedders[0]
    tctx = torch.cat([torch.zeros((1, 12, 2048), device=cuda), le(batch["label"])])
    xin = torch.cat([torch.cat([x7, x7]), torch.cat([ucc, cc])], dim=1)
    unet = engine.model.diffusion_model
    eps = unet(xin, timesteps=torch.tensor([999, 999], device=cuda), t_context=tctx)
    assert eps.shape == (2, 4, h, w) and eps.dtype == torch.float32
    _check(f"{case} UNet eps (CFG pair, {h}x{w} latent) vs reference", eps.cpu(), rg[f"{case}_eps"], 2e-2, 8e-2)
    # hw of all 16 cache items: the four levels of the latent, row-major tokens
    assert len(unet.attn_map_cache) == 16
    for i, item in enumerate(unet.attn_map_cache):
        hh, ww = item["hw"]
        assert hh * ww == item["attn_map"].shape[1] and hh * w == ww * h and h % hh == 0, (item["name"], item["hw"])
        assert item["size"] == int((hh * ww) ** 0.5)
    assert sorted({it["hw"] for it in unet.attn_map_cache}, reverse=True) == [(h >> k, w >> k) for k in range(4)]
    if case == "r1":
        names = [str(n) for n in rg["r1_attn_names"]]
        for i, (item, name) in enumerate(zip(unet.attn_map_cache, names)):
            heads, size, *shape = (int(v) for v in rg[f"r1_attn_{i:02d}_meta"])
            assert item["name"] == name and item["heads"] == heads and item["size"] == size and list(item["attn_map"].shape) == shape
            f = item["attn_map"].float().reshape(-1)
            step = max(1, f.numel() // 2048)
            _check(f"r1 t_attn map {name}", f[::step][:2048].cpu(), rg[f"r1_attn_{i:02d}_sub"], 3e-2)
        mom = engine.first_stage_model.encode_moments(batch["image"])
        _check("r1 VAE encoder moments 256x384 vs reference", ops.nhwc_to_nchw(mom, 8).cpu(), rg["r1_moments"], 2e-2, 8e-2)
    # 10 deterministic Euler steps + decode
    sampler = pipeline.init_sampling(10, 5.0, cuda)
    cfgs = C.default_runtime_config(steps=10, batch_size=1, noise_iters=0)
    torch.manual_seed(99)
    x0 = sampler.get_init_noise(cfgs, engine, cond=c, batch=batch, uc=uc)
    np.testing.assert_array_equal(x0.cpu().numpy(), rg[f"{case}_x0"])
    z = sampler(engine, x0.clone(), cond=c, batch=batch, uc=uc)
    assert z.shape == (1, 4, h, w)
    _check(f"{case} 10-step latent vs reference", z.cpu(), rg[f"{case}_latent"], 6e-2)
    dec = engine.decode_first_stage(z)
    assert dec.shape == (1, 3, H, W)
    _check(f"{case} decoded image of the 10-step latent vs reference", dec[:, :, ::8, ::8].cpu(), rg[f"{case}_decoded_sub"], 4e-2)


# ------------------------------------------------------------------------------------------------ r3: 512x768
def test_r3_512x768_sampling_vs_reference_golden_and_graph_replay(engine, rg, cuda):
    """the production-size kernels on a 64x96 latent (wide convolution, 6144-token attention): x0 bit-equal, the 10-step latent and
    the decoded image against the REAL reference; hipGraph replay bit-equal to eager launches"""
    from udifftext_amd import config as C, pipeline
    batch, c, uc = _cond(engine, cuda, 512, 768, 9, 12)
    assert batch["label"][0] == "Diffusion"
    _check("r3 conditioner c.concat vs reference", c["concat"].cpu(), rg["r3_c_concat"], 2e-2, 8e-2)
    sampler = pipeline.init_sampling(10, 5.0, cuda)
    sampler.use_graphs = True
    cfgs = C.default_runtime_config(steps=10, batch_size=1, noise_iters=0)
    torch.manual_seed(99)
    x0 = sampler.get_init_noise(cfgs, engine, cond=c, batch=batch, uc=uc)
    np.testing.assert_array_equal(x0.cpu().numpy(), rg["r3_x0"])
    z = sampler(engine, x0.clone(), cond=c, batch=batch, uc=uc)
    assert z.shape == (1, 4, 64, 96)
    assert len(sampler._graphed) == 1, "graph capture fell back to eager launches"
    _check("r3 10-step latent (512x768) vs reference", z.cpu(), rg["r3_latent"], 6e-2)
    dec = engine.decode_first_stage(z)
    assert dec.shape == (1, 3, 512, 768)
    _check("r3 decoded image of the 10-step latent vs reference", dec[:, :, ::8, ::8].cpu(), rg["r3_decoded_sub"], 4e-2)
    eager = pipeline.init_sampling(10, 5.0, cuda)
    eager.use_graphs = False
    ze = eager(engine, x0.clone(), cond=c, batch=batch, uc=uc)
    assert torch.equal(ze, z)
    # a 96x64 latent next to it: its own runner, replay again bit-equal to eager launches
    b2, c2, uc2 = _cond(engine, cuda, 768, 512, 9, 12)
    torch.manual_seed(5)
    x2 = torch.randn((1, 4, 96, 64), device=cuda)
    four, four_e = pipeline.init_sampling(4, 5.0, cuda), pipeline.init_sampling(4, 5.0, cuda)
    four_e.use_graphs = False
    zg2 = four(engine, x2.clone(), cond=c2, batch=b2, uc=uc2)
    assert len(four._graphed) == 1 and torch.equal(zg2, four_e(engine, x2.clone(), cond=c2, batch=b2, uc=uc2))


def test_predict_many_over_mixed_sizes_matches_predict(engine, cuda):
    """three lanes, mixed 512x512 and 512x768 batches, automatic fusing: against predict() batch by batch"""
    from udifftext_amd import config as C, pipeline, synth
    cfgs = C.default_runtime_config(steps=3, batch_size=1, noise_iters=0)
    sizes = [(512, 512), (512, 768), (512, 768), (512, 512), (512, 512), (512, 768), (512, 512)]
    mk = lambda: [synth.synthetic_batch(1, H, W, 9, seed=60 + i) for i, (H, W) in enumerate(sizes)]
    seq = pipeline.init_sampling(3, 5.0, cuda)
    torch.manual_seed(8)
    ref = [pipeline.predict(cfgs, engine, seq, b) for b in mk()]
    par = pipeline.init_sampling(3, 5.0, cuda)
    torch.manual_seed(8)
    got = pipeline.predict_many(cfgs, engine, par, mk(), in_flight=3, fuse=0)
    assert len(got) == len(ref)
    for i, ((s_ref, z_ref), (s_got, z_got), (H, W)) in enumerate(zip(ref, got, sizes)):
        assert s_got.shape == s_ref.shape == (1, 3, H, W) and z_got.shape == z_ref.shape == (1, 4, H // 8, W // 8)
        _check(f"mixed sizes: predict_many latent of batch {i} ({H}x{W}) vs predict", z_got.cpu(), z_ref.cpu(), 3e-2)
        _check(f"mixed sizes: predict_many image of batch {i} ({H}x{W}) vs predict", s_got.cpu(), s_ref.cpu(), 3e-2)
    with pytest.raises(ValueError):
        pipeline.predict_many(cfgs, engine, par, mk()[:2], in_flight=1, fuse=2)


# ------------------------------------------------------------------------------------------------ map consumers at H != W
@pytest.mark.parametrize("H,W", [(256, 384), (384, 256)])
def test_noise_search_scores_rectangular_maps_per_sample(engine, cuda, monkeypatch, H, W):
    """B = 2, noise_iters = 4: the scores the search used equal the restatement evaluated on the maps of the same calls, and each
    sample gets the candidate with its own smallest score"""
    from udifftext_amd import config as C, pipeline, rng
    h, w = H // 8, W // 8
    batch, c, uc = _cond(engine, cuda, H, W, 6, 31, batch_size=2, torch_seed=77)
    sampler = pipeline.init_sampling(50, 5.0, cuda)
    cfgs = C.default_runtime_config(steps=50, batch_size=2, noise_iters=4)
    loss_fn = engine.loss_fn
    gk = loss_fn.g_kernel.detach().float().cpu()
    used, want = [], []
    orig = loss_fn.get_min_local_loss

    def recording(cache, mask, seg, cond_only=False):
        out = orig(cache, mask, seg, cond_only=cond_only)
        assert cond_only
        items = []
        for it in cache:
            assert it["hw"] in [(h >> k, w >> k) for k in range(4)]
            am = it["attn_map"].detach().float().cpu()
            items.append({"name": it["name"], "heads": it["heads"], "hw": it["hw"], "attn_map": am[am.shape[0] // 2:]})
        assert sum(rect_ref.scores_map(it["hw"]) for it in items) == 10        # the 32x48 and 16x24 levels
        used.append(out.detach().cpu())
        want.append(rect_ref.min_local_loss(items, mask.float().cpu(), seg.float().cpu(), gk, loss_fn.min_attn_size))
        return out

    monkeypatch.setattr(loss_fn, "get_min_local_loss", recording)
    torch.manual_seed(4321)
    with contextlib.redirect_stdout(io.StringIO()):
        x0 = sampler.get_init_noise(cfgs, engine, cond=c, batch=batch, uc=uc)
    assert x0.shape == (2, 4, h, w) and len(used) == 2                          # 4 candidates x 2 images in one chunk, 2 Euler steps
    for k, (u, v) in enumerate(zip(used, want)):
        assert u.shape == v.shape == (8,)
        _check(f"noise search {H}x{W}: scores after step {k} vs restatement on the same maps", u, v, 3e-2)
    score = used[-1].reshape(4, 2)
    torch.manual_seed(4321)
    cands = [rng.randn_on((2, 4, h, w), cuda) for _ in range(5)][:4]
    best = score.argmin(dim=0)
    assert len(set(score[:, 0].tolist())) == 4 and len(set(score[:, 1].tolist())) == 4
    for b in range(2):
        assert torch.equal(x0[b], cands[int(best[b])][b])
        assert float(score[int(best[b]), b]) == float(score[:, b].min())


def test_reverse_pass_at_a_48x32_latent_vs_oracle_autograd(engine, cuda):
    """backward.unet_maps_vjp with the dense cotangents of aae_fixture.aae_functional_weights against oracle.backward.maps_functional_grad
    (B = 1; min(h, w) >= 16 picks the ten maps the oracle's int(sqrt(n)) >= 16 picks); then the hard loss: unet_local_loss_grad eager and
    replayed bit-equal, its loss equal to get_min_local_loss on the same maps"""
    from aae_fixture import aae_functional_weights
    from oracle import backward as obw, spec
    from udifftext_amd import backward as bw, pipeline
    dev = cuda
    batch, c, uc = _cond(engine, dev, 384, 256, 4, 6, torch_seed=17)
    x = torch.randn((1, 4, 48, 32), device=dev) * 3.0
    sigma = torch.full((1,), 2.5, device=dev)
    sampler = pipeline.init_sampling(10, 5.0, dev)
    c_noise = sampler.get_c_noise(x, engine, sigma)
    unet, loss_fn = engine.model.diffusion_model, engine.loss_fn

    def maps_grad(rec):
        used = [it for it in rec if loss_fn.scores_map(it["hw"])]
        assert [it["hw"] for it in used] == [(48, 32)] * 2 + [(24, 16)] * 2 + [(24, 16)] * 3 + [(48, 32)] * 3
        assert [it["size"] for it in used] == [39] * 2 + [19] * 5 + [39] * 3 and len(rec) == 16
        for k, it in enumerate(used):
            it["d_probs"] = (aae_functional_weights(it["attn_map"].shape, k).to(dev) / len(used)).contiguous()
    got = bw.unet_maps_vjp(unet, x, c_noise.float(), c["concat"], c["t_crossattn"], maps_grad).cpu()
    sd = {k: v.detach().float().cpu() for k, v in engine.state_dict().items()}
    cond = {"concat": c["concat"].float().cpu(), "t_crossattn": c["t_crossattn"].float().cpu()}
    _, ref = obw.maps_functional_grad(sd, spec.EngineConfig(), x.cpu(), sigma.cpu(), cond, aae_functional_weights, loss_fn.min_attn_size)
    assert got.shape == ref.shape == (1, 4, 48, 32)
    _check("reverse pass at a 48x32 latent (dense map cotangents) vs oracle autograd", got, ref, 3e-2)
    # the hard loss
    args = (c_noise.float(), c["concat"], c["t_crossattn"], batch["mask"], batch["seg_mask"])
    l_e, g_e = bw.unet_local_loss_grad(unet, loss_fn, x, *args)
    assert bool(torch.isfinite(g_e).all()) and bool(g_e.abs().sum() > 0)
    runner = bw.GraphedLocalLossGrad(unet, loss_fn, x, *args)
    for xx in (x, x * 0.5):
        l_g, g_g = runner(xx, *args)
        l_e2, g_e2 = bw.unet_local_loss_grad(unet, loss_fn, xx, *args)
        assert torch.equal(g_g, g_e2) and torch.allclose(l_g, l_e2, rtol=1e-5, atol=1e-6)
    runner.check()
    seen = {}

    def score_only(rec):
        seen["ll"] = loss_fn.get_min_local_loss(rec, batch["mask"], batch["seg_mask"])
        for it in rec:
            if loss_fn.scores_map(it["hw"]):
                it["d_probs"] = torch.zeros_like(it["attn_map"])
    bw.unet_maps_vjp(unet, x, *args[:3], score_only)
    print(f"hard local loss at 48x32: reverse pass {l_e.tolist()} get_min_local_loss {seen['ll'].tolist()}")
    assert torch.allclose(l_e, seen["ll"], rtol=1e-5, atol=0)


def test_attend_and_excite_at_256x384(engine, cuda):
    """aae_enabled through the sampler on a 32x48 latent: finite latent, one local loss and one decoded intermediate per step, the
    scheduled gradient evaluations (4 steps, none in iter_lst: one each), a trajectory that differs from the plain one"""
    from udifftext_amd import config as C, pipeline
    batch, c, uc = _cond(engine, cuda, 256, 384, 4, 14, torch_seed=99)
    sampler = pipeline.init_sampling(4, 5.0, cuda)
    cfgs = C.default_runtime_config(steps=4, batch_size=1, noise_iters=0)
    torch.manual_seed(5)
    x0 = sampler.get_init_noise(cfgs, engine, cond=c, batch=batch, uc=uc)
    evals0 = getattr(sampler, "aae_evaluations", 0)
    z = sampler(engine, x0.clone(), cond=c, batch=batch, uc=uc, aae_enabled=True)
    assert z.shape == (1, 4, 32, 48) and bool(torch.isfinite(z).all())
    assert len(sampler.last_local_losses) == 4 and len(sampler.last_inters) == 4 and all(np.isfinite(sampler.last_local_losses))
    assert sampler.aae_evaluations - evals0 == 4
    assert sampler.last_inters[0].shape == (256, 384, 3)
    z_plain = sampler(engine, x0.clone(), cond=c, batch=batch, uc=uc, aae_enabled=False)
    assert not torch.equal(z, z_plain)


@pytest.mark.parametrize("H,W,steps", [(256, 384, 6), (512, 768, 2)])
def test_detailed_dumps_rectangular_maps(engine, cuda, tmp_path, monkeypatch, H, W, steps):
    """``detailed: True`` at H != W: the dumped per-character maps are [len(label), h', w'] of the configured layer
    (save_attn_layers = output_blocks.6.1: the half-resolution level of the latent — [L, 16, 24] for a 256x384 image, [L, 32, 48] for
    512x768), row-major, equal to the cached probabilities of that layer"""
    from udifftext_amd import config as C, pipeline, synth
    monkeypatch.chdir(tmp_path)
    hm, wm = H // 16, W // 16
    batch = synth.synthetic_batch(1, H, W, 4, seed=9)
    label, name = batch["label"][0], batch["name"][0]
    sampler = pipeline.init_sampling(steps, 5.0, cuda)
    torch.manual_seed(11)
    s0, z0 = pipeline.predict(C.default_runtime_config(steps=steps, batch_size=1, noise_iters=0),
                              engine, sampler, {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in batch.items()})
    torch.manual_seed(11)
    s1, z1 = pipeline.predict(C.default_runtime_config(steps=steps, batch_size=1, noise_iters=0, detailed=True),
                              engine, sampler, {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in batch.items()})
    assert z1.shape == (1, 4, H // 8, W // 8) and bool(torch.isfinite(z1).all())
    _check(f"detailed=True latent at {H}x{W} vs the plain sampler", z1.cpu(), z0.cpu(), 1.5e-2)
    seg = np.load(tmp_path / "temp" / "seg_map" / f"seg_{name}.npy")
    assert seg.shape == (len(label), hm, wm) and np.isfinite(seg).all()
    unet = engine.model.diffusion_model
    full = unet.save_attn_map(save_name="again", tokens=label, out_dir=str(tmp_path / "again"))
    assert full.shape == (12, hm, wm)
    np.testing.assert_allclose(full.sum(axis=0), 1.0, atol=2e-3)
    np.testing.assert_array_equal(full[:len(label)], seg)
    items = [it for it in unet.attn_map_cache if it["name"].startswith("output_blocks.6.1") and it["name"].endswith("t_attn")]
    assert len(items) == 1 and items[0]["hw"] == (hm, wm)
    m = items[0]["attn_map"].float().reshape(-1, items[0]["heads"], hm * wm, 12).mean(dim=1)[-1].t().reshape(12, hm, wm).cpu().numpy()
    np.testing.assert_allclose(full, m, atol=1e-6)
