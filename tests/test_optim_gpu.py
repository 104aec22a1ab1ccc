"""Gradient accumulation and EMA on the fused bucket optimiser step, on the GPU.  ``pytest -m gpu``.

Kernel level (exact): the accumulating forms of the three parameter-gradient kernels against ``prefill + parent``; the bucket update
against the per-tensor udt_adamw_f32 on the same data (bit-equal: both kernels inline ONE device function with its fused operations
written out) and its EMA against
float64 at the derived bound |err| <= 4 * 2^-24 (|shadow| + |p|) — three roundings (the difference, the product, the subtraction)
on operands no larger than that sum, plus one of slack; the swap; the padding between segments.

G16 (tests/golden/optim_golden.npz, tests/golden/make_optim_golden.py): two windows of two micro-batches through
``engine.training_step`` against the REAL reference's FullLoss + torch.optim.AdamW + LitEma.  Tolerances are tests/test_iterated_gpu.py's
for the same model and optimiser: window 1 is one evaluation deep (TOL_LOSS, TOL_STEP), window 2 sits where G15c's step 2 sits — one
update behind it, the same lr and eps — and borrows its free-running bounds (TOL_LOSS_FREE, TOL_GRAD_FREE, TOL_DP_FREE).  A mean of two
gradients injects no more error than one: an error of TOL per evaluation is at most ``ratio`` x TOL of the mean, ratio = (rms g_a +
rms g_b) / 2 / rms(mean), stored by the generator (1.01 / 1.03); a shadow displacement is a fixed combination of the p_k - p_0, with
the analogous stored ratio (<= 1.011).  The first shadow displacement is exactly zero (no optimiser step yet) and is checked as such.

Setting UDT_PARITY_REPORT to a file path makes the G16 test also write every measured value to that file (profiles/optim_parity.txt).
"""
import os

import numpy as np
import pytest
import torch

import optim_ref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REPORT = os.environ.get("UDT_PARITY_REPORT")
# tests/test_iterated_gpu.py (derived there)
TOL_STEP, TOL_LOSS = 3e-2, 6e-4
G_LOSS, G_GRAD, G_DP = 0.204, 1.481, 1.008
TOL_LOSS_FREE = TOL_LOSS + G_LOSS * TOL_STEP
TOL_GRAD_FREE = TOL_STEP + G_GRAD * TOL_STEP
TOL_DP_FREE = max(1.0, G_DP) * TOL_STEP
F32, BF16 = torch.float32, torch.bfloat16


def _report(line):
    print(line)
    if REPORT:
        os.makedirs(os.path.dirname(os.path.abspath(REPORT)), exist_ok=True)
        with open(REPORT, "a") as f:
            f.write(line + "\n")


def _rand(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(tuple(shape), generator=g) * scale + shift


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import backward, lib, ops, pipeline, training
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)

    class Env:
        pass
    Env.ops, Env.L, Env.lib, Env.bw, Env.pipeline, Env.training, Env.dev = ops, lib, lib.load(), backward, pipeline, training, cuda
    return Env


@pytest.fixture(scope="module")
def engine(env):
    return env.pipeline.build_engine(env.dev)


def _chk(env, rc, what):
    env.L.check(rc, what)


# ------------------------------------------------------------------------------------------------ the accumulating forms
@pytest.mark.parametrize("R", [40, 64, 1000], ids=["R40-one-range-ragged", "R64-one-range", "R1000-split"])
def test_wgrad_acc_is_prefill_plus_parent(env, R):
    """N = 136, K = 72 (neither a multiple of the 128 tile): R = 40 / 64 take the S_used == 1 branch (the add in the kernel's
    epilogue), R = 1000 the split one (the add in the reduction); R = 40 and 1000 are no multiples of 64"""
    lib, st, dev = env.lib, env.ops._stream(), env.dev
    N, K = 136, 72
    dy, x = _rand((R, N), 1).to(dev, BF16), _rand((R, K), 2).to(dev, BF16)
    S = lib.udt_wgrad_splits(R, N, K)
    rps = ((R + S - 1) // S + 31) // 32 * 32
    assert ((R + rps - 1) // rps == 1) == (R <= 64)
    part = torch.empty((max(S, 1), N, K), dtype=F32, device=dev)
    parent = torch.full((N, K), float("nan"), device=dev)
    _chk(env, lib.udt_wgrad_bf16(dy.data_ptr(), x.data_ptr(), parent.data_ptr(), part.data_ptr(), R, N, K, N, K, st), "udt_wgrad_bf16")
    prefill = _rand((N, K), 3, 5.0).to(dev)
    acc = prefill.clone()
    _chk(env, lib.udt_wgrad_bf16_acc(dy.data_ptr(), x.data_ptr(), acc.data_ptr(), part.data_ptr(), R, N, K, N, K, 1, st), "udt_wgrad_bf16_acc")
    assert torch.equal(acc, prefill + parent)
    over = prefill.clone()
    _chk(env, lib.udt_wgrad_bf16_acc(dy.data_ptr(), x.data_ptr(), over.data_ptr(), part.data_ptr(), R, N, K, N, K, 0, st), "udt_wgrad_bf16_acc")
    assert torch.equal(over, parent)
    # the wrapper: the accumulating form on a view
    view = prefill.clone()
    assert env.ops.weight_grad(dy, x, out=view) is view and torch.equal(view, acc)
    assert torch.equal(env.ops.weight_grad(dy, x), parent)


@pytest.mark.parametrize("C", [8, 320, 1280])
@pytest.mark.parametrize("rows", [1, 65, 4100])
def test_colsum_and_ln_param_grad_acc_are_prefill_plus_parent(env, rows, C):
    lib, st, dev = env.lib, env.ops._stream(), env.dev
    x, dy = _rand((rows, C), 4, 2.0, 0.5).to(dev, BF16), _rand((rows, C), 5).to(dev, BF16)
    parts = lib.udt_colparts(rows)
    part = torch.empty((parts, 2, C), dtype=F32, device=dev)
    # column sums
    parent = torch.full((C,), float("nan"), device=dev)
    _chk(env, lib.udt_colsum_bf16(dy.data_ptr(), part.data_ptr(), parent.data_ptr(), rows, C, st), "udt_colsum_bf16")
    prefill = _rand((C,), 6, 3.0).to(dev)
    acc, over = prefill.clone(), prefill.clone()
    _chk(env, lib.udt_colsum_bf16_acc(dy.data_ptr(), part.data_ptr(), acc.data_ptr(), rows, C, 1, st), "udt_colsum_bf16_acc")
    _chk(env, lib.udt_colsum_bf16_acc(dy.data_ptr(), part.data_ptr(), over.data_ptr(), rows, C, 0, st), "udt_colsum_bf16_acc")
    assert torch.equal(acc, prefill + parent) and torch.equal(over, parent)
    view = prefill.clone()
    assert env.ops.colsum(dy, out=view) is view and torch.equal(view, acc)
    # LayerNorm parameter gradients
    parent2 = torch.full((2, C), float("nan"), device=dev)
    _chk(env, lib.udt_ln_param_grad(x.data_ptr(), dy.data_ptr(), part.data_ptr(), parent2.data_ptr(), rows, C, 1e-5, st), "udt_ln_param_grad")
    prefill2 = _rand((2, C), 7, 3.0).to(dev)
    acc2, over2 = prefill2.clone(), prefill2.clone()
    _chk(env, lib.udt_ln_param_grad_acc(x.data_ptr(), dy.data_ptr(), part.data_ptr(), acc2.data_ptr(), rows, C, 1e-5, 1, st), "udt_ln_param_grad_acc")
    _chk(env, lib.udt_ln_param_grad_acc(x.data_ptr(), dy.data_ptr(), part.data_ptr(), over2.data_ptr(), rows, C, 1e-5, 0, st), "udt_ln_param_grad_acc")
    assert torch.equal(acc2, prefill2 + parent2) and torch.equal(over2, parent2)
    view2 = prefill2.clone()
    env.ops.layer_norm_param_grad(x, dy, 1e-5, out=view2)
    assert torch.equal(view2, acc2)


# ------------------------------------------------------------------------------------------------ the bucket update
SIZES = [1, 3, 4, 5, 255, 257, 320, 1280 * 1280]
HYPER = dict(lr=1.6e-2, betas=(0.9, 0.999), eps=1e-3, weight_decay=1e-2)
GRAD_SCALE = 0.37


@pytest.fixture(scope="module")
def bucket_case(env):
    """eight segments (the last one 400 chunks), segment 5's parameter only 4-byte aligned, the padding of g / m / v NaN; two fused
    steps (AdamW + EMA) next to the per-tensor udt_adamw_f32 on copies of the same data.  Computed once, shared, left unchanged."""
    tr, dev = env.training, env.dev
    named = []
    for i, n in enumerate(SIZES):
        if i == 5:
            buf = torch.empty((n + 1,), dtype=F32, device=dev)
            t = buf[1:]
            assert t.data_ptr() % 16 == 4
        else:
            t = torch.empty((n,), dtype=F32, device=dev)
        t.copy_(_rand((n,), 20 + i, 0.05))
        named.append((f"model.seg{i}.weight", t))
    opt = tr.BucketAdamW(named, accumulate_grad_batches=1, **HYPER)
    ema = tr.Ema(named, decay=0.9999)
    for i, sh in enumerate(ema.shadows()):
        sh.copy_(_rand((SIZES[i],), 40 + i, 0.05))
    bucket = opt.bucket
    nan = float("nan")
    pad = torch.ones((bucket.total,), dtype=torch.bool, device=dev)
    for (n, p) in named:
        pad[bucket.offsets[n]:bucket.offsets[n] + p.numel()] = False
    assert int(pad.sum()) > 0
    for flat in (bucket.flat, opt.m, opt.v):
        flat.fill_(nan)
    for i, (n, p) in enumerate(named):
        o = bucket.offsets[n]
        assert o % 4 == 0
        bucket.flat[o:o + p.numel()] = _rand((p.numel(),), 60 + i, 2e-3).to(dev)
        opt.m[o:o + p.numel()] = 0.0
        opt.v[o:o + p.numel()] = 0.0
    # the per-tensor route on copies
    ref = {n: (p.clone(), torch.zeros_like(p), torch.zeros_like(p)) for n, p in named}
    states = []
    for step in (1, 2):
        sh_before = [s.clone() for s in ema.shadows()]
        versions = [p._version for _, p in named]
        opt.step(bucket, grad_scale=GRAD_SCALE, ema=ema)
        assert all(p._version > v0 for (_, p), v0 in zip(named, versions)), "the step did not bump the parameters' versions"
        for n, p in named:
            rp, rm, rv = ref[n]
            env.ops.adamw_(rp, bucket.views[n].contiguous(), rm, rv, step, HYPER["lr"], HYPER["betas"], HYPER["eps"], HYPER["weight_decay"],
                           GRAD_SCALE)
        states.append({"p": [p.clone() for _, p in named], "m": opt.m.clone(), "v": opt.v.clone(), "g": bucket.flat.clone(),
                       "ref": {n: tuple(t.clone() for t in ref[n]) for n in ref}, "sh_before": sh_before,
                       "sh": [s.clone() for s in ema.shadows()], "omd": optim_ref.one_minus_decay(step)})
    torch.cuda.synchronize()

    class Case:
        pass
    Case.named, Case.opt, Case.ema, Case.bucket, Case.pad, Case.states = named, opt, ema, bucket, pad, states
    return Case


def test_bucket_update_is_bit_equal_to_the_per_tensor_adamw(env, bucket_case):
    """p, m, v after steps 1 and 2 (grad_scale 0.37) against udt_adamw_f32 on the same data: both kernels inline the ONE device
    function ``adamw_element``, whose fused multiply-adds are written out with contraction off, so they round alike.  (With the
    contraction left to the compiler the 16-byte path fused other products than adamw_kernel: m and v were 1 ulp apart at step 2.)"""
    c = bucket_case
    assert c.opt.step_count == 2 and int(c.ema.num_updates) == 2
    for k, st in enumerate(c.states):
        for i, (n, p) in enumerate(c.named):
            o = c.bucket.offsets[n]
            rp, rm, rv = st["ref"][n]
            assert torch.equal(st["m"][o:o + p.numel()], rm), (k + 1, n, "m")
            assert torch.equal(st["v"][o:o + p.numel()], rv), (k + 1, n, "v")
            assert torch.equal(st["p"][i], rp), (k + 1, n, "p")
        if k:
            assert not torch.equal(st["p"][-1], c.states[k - 1]["p"][-1])


def test_bucket_update_leaves_the_padding_alone(env, bucket_case):
    c = bucket_case
    for st in c.states:
        for key in ("g", "m", "v"):
            assert bool(torch.isnan(st[key][c.pad]).all()), f"padding of {key} was written"
            assert not bool(torch.isnan(st[key][~c.pad]).any()), f"a payload element of {key} is NaN: padding was read"
        assert all(not bool(torch.isnan(t).any()) for t in st["p"] + st["sh"])


def test_bucket_ema_vs_float64(env, bucket_case):
    """shadow' = shadow - omd (shadow - p') on the UPDATED p'; |err| <= 4 * 2^-24 (|shadow| + |p'|)"""
    c = bucket_case
    assert np.allclose([st["omd"] for st in c.states], [9 / 11, 9 / 12], rtol=1e-6)            # ema.py:36-38, updates 1 and 2
    for st in c.states:
        for i in range(len(c.named)):
            s0, p1, s1 = st["sh_before"][i].double(), st["p"][i].double(), st["sh"][i].double()
            want = s0 - st["omd"] * (s0 - p1)
            bound = 4 * 2.0 ** -24 * (s0.abs() + p1.abs())
            assert bool(((s1 - want).abs() <= bound).all()), (i, float(((s1 - want).abs() - bound).max()))
            assert not torch.equal(st["sh"][i], st["sh_before"][i])


def test_bucket_modes_touch_only_their_own_tensors(env, bucket_case):
    """on copies: EMA-only leaves p, m, v, g bit-untouched; AdamW-only leaves the shadows untouched"""
    tr, L, dev = env.training, env.L, env.dev
    c = bucket_case
    named = [(n, p.clone()) for n, p in c.named]
    shadows = [s.clone() for s in c.ema.shadows()]
    g, m, v = c.bucket.flat.clone(), c.opt.m.clone(), c.opt.v.clone()
    seg = tr._Segments(named, c.bucket.offsets)
    tab, cmap = seg.tables(shadows)
    keep = lambda: ([p.clone() for _, p in named], [s.clone() for s in shadows], g.clone(), m.clone(), v.clone())
    bits = lambda t: t.view(torch.int32)
    same = lambda a, b: all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))
    p0, s0, g0, m0, v0 = keep()
    env.ops.bucket_update_(tab, cmap, g, m, v, L.BUCKET_EMA, one_minus_decay=0.25)
    p1, s1, g1, m1, v1 = keep()
    assert same(p0, p1) and same([g0, m0, v0], [g1, m1, v1]) and not any(torch.equal(a, b) for a, b in zip(s0, s1))
    env.ops.bucket_update_(tab, cmap, g, m, v, L.BUCKET_ADAMW, step=3, grad_scale=GRAD_SCALE, **HYPER)
    p2, s2, g2, m2, v2 = keep()
    assert same(s1, s2) and same([g1], [g2]) and not any(torch.equal(a, b) for a, b in zip(p1, p2))
    # the EMA-only launch needs no g / m / v at all
    env.ops.bucket_update_(tab, cmap, None, None, None, L.BUCKET_EMA, one_minus_decay=0.25)
    # the swap: once exchanges, twice is the identity
    pb, sb = keep()[:2]
    env.ops.bucket_swap_(tab, cmap)
    p3, s3 = keep()[:2]
    env.ops.bucket_swap_(tab, cmap)
    p4, s4 = keep()[:2]
    assert same(p3, sb) and same(s3, pb) and not any(torch.equal(a, b) for a, b in zip(p3, pb))
    assert same(p4, pb) and same(s4, sb)


def test_ema_swap_bumps_versions_and_is_its_own_inverse(env, bucket_case):
    tr = env.training
    named = [(n, p.clone()) for n, p in bucket_case.named]
    ema = tr.Ema(named)
    for i, sh in enumerate(ema.shadows()):
        sh.copy_(_rand((SIZES[i],), 80 + i))
    p0, s0 = [p.clone() for _, p in named], [s.clone() for s in ema.shadows()]
    v0 = [p._version for _, p in named]
    ema.store()
    ema.copy_to()
    assert all(torch.equal(p, s) for (_, p), s in zip(named, s0)) and all(torch.equal(s, p) for s, p in zip(ema.shadows(), p0))
    assert all(p._version > v for (_, p), v in zip(named, v0))
    with pytest.raises(RuntimeError):
        ema.update()
    v1 = [p._version for _, p in named]
    ema.restore()
    assert all(torch.equal(p, q) for (_, p), q in zip(named, p0)) and all(torch.equal(s, q) for s, q in zip(ema.shadows(), s0))
    assert all(p._version > v for (_, p), v in zip(named, v1))


def test_bucket_average_in_a_world_of_one_on_rccl(env):
    """the in-place reduce-scatter + all-gather of GradBucket.average, forced in a world of one: the bucket is unchanged"""
    import socket

    import torch.distributed as dist
    tr, dev = env.training, env.dev
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    named = [("a.weight", torch.zeros((7, 5), device=dev)), ("a.bias", torch.zeros((5,), device=dev))]
    b = tr.GradBucket(named)
    b.flat.copy_(_rand((b.total,), 90))
    want = b.flat.clone()
    mine = not dist.is_initialized()
    if mine:
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    calls = []
    real_rs, real_ag = dist.reduce_scatter_tensor, dist.all_gather_into_tensor
    try:
        dist.reduce_scatter_tensor = lambda out, inp, **k: (calls.append(("rs", inp.data_ptr(), out.data_ptr())), real_rs(out, inp, **k))[1]
        dist.all_gather_into_tensor = lambda out, inp, **k: (calls.append(("ag", out.data_ptr(), inp.data_ptr())), real_ag(out, inp, **k))[1]
        ptr = b.flat.data_ptr()
        b.average(dist, force=True)
        torch.cuda.synchronize()
        assert calls == [("rs", ptr, ptr), ("ag", ptr, ptr)], calls          # on the buffer itself: no concatenation, no copy back
        assert torch.equal(b.flat, want)
        b.average(dist)                                                      # a world of one, not forced: nothing runs
        assert len(calls) == 2
    finally:
        dist.reduce_scatter_tensor, dist.all_gather_into_tensor = real_rs, real_ag
        if mine:
            dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------ the reverse pass into the bucket
def _train_inputs(env):
    from aae_fixture import train_batch
    dev = env.dev
    g16 = np.load(os.path.join(GOLD, "optim_golden.npz"))
    g14 = np.load(os.path.join(GOLD, "train_golden.npz"))
    g15 = np.load(os.path.join(GOLD, "iterated_golden.npz"))
    tb = train_batch()
    z = torch.from_numpy(g15["g15c_z"]).to(dev)
    cond = {"concat": torch.from_numpy(g14["g14_c_concat"]).to(dev), "t_crossattn": torch.from_numpy(g14["g14_c_txt"]).to(dev)}
    draws = [(torch.from_numpy(g16["g16_sigma_idx"][k]).to(dev), torch.from_numpy(g16["g16_noise"][k]).to(dev)) for k in range(4)]
    return g16, z, cond, tb["seg"].to(dev), tb["seg_mask"].to(dev), draws


def test_reverse_pass_into_the_bucket_equals_the_dict_route(engine, env):
    """one micro-batch from a zeroed bucket = the dict route's gradients; two = g_a + g_b (the full loss, local loss included)"""
    tr = env.training
    g16, z, cond, seg, segm, draws = _train_inputs(env)
    named = tr.trainable_parameters(engine, ["t_attn", "t_norm"])
    bucket = tr.GradBucket(named)
    assert bucket.names == [str(n) for n in g16["g16_names"]]
    ld_a, ga = tr.training_loss_and_grads(engine, z, cond, seg, segm, sigma_idx=draws[0][0], noise=draws[0][1])
    ld_b, gb = tr.training_loss_and_grads(engine, z, cond, seg, segm, sigma_idx=draws[1][0], noise=draws[1][1])
    assert sorted(ga) == sorted(bucket.names)
    bucket.zero_()
    ld, got = tr.training_loss_and_grads(engine, z, cond, seg, segm, sigma_idx=draws[0][0], noise=draws[0][1], bucket=bucket)
    assert got is bucket and all(torch.equal(ld[k], ld_a[k]) for k in ld_a)
    bad = [n for n in bucket.names if not torch.equal(bucket.views[n], ga[n])]
    assert not bad, f"{len(bad)} gradients differ after one micro-batch, first {bad[0]}"
    assert any(bool(ga[n].any()) for n in ga)
    tr.training_loss_and_grads(engine, z, cond, seg, segm, sigma_idx=draws[1][0], noise=draws[1][1], bucket=bucket)
    bad = [n for n in bucket.names if not torch.equal(bucket.views[n], ga[n] + gb[n])]
    assert not bad, f"{len(bad)} gradients differ after two micro-batches, first {bad[0]}"


# ------------------------------------------------------------------------------------------------ G16
def _check_sub(tag, tensors, ref_sub, names, tol):
    r, worst, wname = optim_ref.rel_sub(tensors, ref_sub, names)
    _report(f"{tag:58s} rel_rms {r:.3e} (tol {tol:.2e})  worst tensor {worst:.3e} {wname}")
    assert r <= tol, (tag, r, tol)


def _check_scalar(tag, got, ref, rtol):
    err, tol = abs(float(got) - float(ref)), rtol * abs(float(ref))
    _report(f"{tag:58s} |err| {err:.3e} (tol {tol:.1e}; value {float(ref):.6f})")
    assert err <= tol, (tag, float(got), float(ref))


def test_g16_two_windows_through_training_step_vs_reference(engine, env):
    """engine.training_step with the fused optimiser, accumulate_grad_batches = 2, use_ema: the golden's draws reach the step through
    ``shared_step`` (replaced on the instance: the latents, conditioning and draws are the golden's, not the first stage's)"""
    tr = env.training
    g16, z, cond, seg, segm, draws = _train_inputs(env)
    names = [str(n) for n in g16["g16_names"]]
    N = int(g16["g16_accumulate"][0])
    saved = (engine.use_ema, engine.opt_keys, engine.optimizer_config, engine.model_ema, engine.loss_fn.lambda_local_loss)
    named = tr.trainable_parameters(engine, ["t_attn", "t_norm"])
    before = {n: p.detach().clone() for n, p in named}
    try:
        engine.use_ema, engine.opt_keys = True, ["t_attn", "t_norm"]
        engine.optimizer_config = {"target": "torch.optim.AdamW", "params": {"eps": float(g16["g16_eps"][0]),
                                                                             "weight_decay": float(g16["g16_weight_decay"][0])}}
        engine.loss_fn.lambda_local_loss = 0.0
        opt = engine.configure_optimizers(float(g16["g16_lr"][0]), fused=True, accumulate_grad_batches=N)
        assert isinstance(opt, tr.BucketAdamW) and [n for n, _ in opt.named] == names
        ema = engine.model_ema
        assert isinstance(ema, tr.Ema) and ["model_ema." + k for k in ema.state_dict()] == [str(k) for k in g16["g16_ema_keys"]]
        engine.shared_step = lambda batch, bucket=None: tr.training_loss_and_grads(
            engine, z, cond, seg, segm, sigma_idx=batch["sigma_idx"], noise=batch["noise"], bucket=bucket)
        acc = []
        real_step = opt.step
        opt.step = lambda bucket=None, **kw: (acc.append((opt.bucket.flat.clone(), kw["grad_scale"])), real_step(bucket, **kw))[1]
        shadow_of = lambda: dict(zip(names, ema.shadows()))
        for k, (idx, noise) in enumerate(draws):
            w = k // N
            ld = engine.training_step({"sigma_idx": idx, "noise": noise}, opt)
            for key in ("loss/diff_loss", "loss/full_loss"):
                _check_scalar(f"G16 micro-batch {k + 1} {key}", ld[key], g16[f"g16_{k + 1}_" + key.replace("/", "_")][0],
                              TOL_LOSS if w == 0 else TOL_LOSS_FREE)
            assert opt.step_count == (k + 1) // N and int(ema.num_updates) == k + 1
            if (k + 1) % N == 0:
                flat, scale = acc[-1]
                assert scale == 1.0 / N and not bool(opt.bucket.flat.any()), "grad_scale / the bucket is not zeroed after the step"
                gacc = {n: flat[opt.bucket.offsets[n]:opt.bucket.offsets[n] + p.numel()] * scale for n, p in named}
                ratio = float(g16["g16_grad_ratio"][w])
                _check_sub(f"G16 window {w + 1} accumulated gradient vs reference", gacc, g16[f"g16_w{w + 1}_grad_sub"], names,
                           (TOL_STEP if w == 0 else TOL_GRAD_FREE) * ratio)
                dp = {n: p.detach() - before[n] for n, p in named}
                _check_sub(f"G16 window {w + 1} p_k - p_0 vs reference", dp, g16[f"g16_w{w + 1}_dp_sub"], names,
                           TOL_STEP if w == 0 else TOL_DP_FREE)
            disp = {n: s - before[n] for n, s in shadow_of().items()}
            if k == 0:
                assert not g16["g16_1_shadow_sub"].any() and all(not bool(d.any()) for d in disp.values()), "EMA moved before any step"
                _report(f"{'G16 shadow - p_0 after EMA update 1':58s} exactly zero, as the reference's")
            else:
                _check_sub(f"G16 shadow - p_0 after EMA update {k + 1} vs reference", disp, g16[f"g16_{k + 1}_shadow_sub"], names,
                           TOL_DP_FREE * float(g16["g16_shadow_ratio"][k]))
        assert opt.step_count == 2 and len(acc) == 2 and int(ema.num_updates) == 4
    finally:
        engine.__dict__.pop("shared_step", None)
        engine.use_ema, engine.opt_keys, engine.optimizer_config, engine.model_ema, engine.loss_fn.lambda_local_loss = saved
        with torch.no_grad():
            for n, p in named:
                p.copy_(before[n])


# ------------------------------------------------------------------------------------------------ ema_scope
def test_ema_scope_runs_on_the_shadows_and_restores_bit_for_bit(engine, env):
    tr, dev = env.training, env.dev
    g15 = np.load(os.path.join(GOLD, "iterated_golden.npz"))
    g13 = np.load(os.path.join(GOLD, "aae_golden.npz"))
    x0 = torch.from_numpy(g15["g15a_ii_x"][0]).to(dev)                       # [1, 4, 16, 16]
    xin = torch.cat([x0, torch.from_numpy(g13["g13_c_concat"]).to(dev)], dim=1)
    ts = torch.tensor([981], device=dev)
    tctx = torch.from_numpy(g13["g13_c_txt"]).to(dev)
    unet = engine.model.diffusion_model
    call = lambda: unet(xin, timesteps=ts, t_context=tctx).clone()
    saved = (engine.use_ema, engine.opt_keys, engine.model_ema)
    named = tr.trainable_parameters(engine, ["t_attn", "t_norm"])
    before = {n: p.detach().clone() for n, p in named}
    try:
        engine.use_ema, engine.opt_keys = False, ["t_attn", "t_norm"]
        out0 = call()
        with engine.ema_scope():                                         # without use_ema: a no-op
            assert torch.equal(call(), out0)
        engine.use_ema = True
        engine.configure_optimizers(fused=True)
        ema = engine.model_ema
        for i, sh in enumerate(ema.shadows()):
            sh.mul_(0.5 + 0.25 * (i % 3))
        shadows = [s.clone() for s in ema.shadows()]
        with engine.ema_scope():
            out_in = call()
            assert all(torch.equal(p, s) for (_, p), s in zip(named, shadows))
        out_after = call()
        assert torch.equal(out_after, out0), "after ema_scope the UNet's output is not bit-equal to before"
        assert all(torch.equal(p, before[n]) for n, p in named) and all(torch.equal(s, q) for s, q in zip(ema.shadows(), shadows))
        assert not torch.equal(out_in, out0), "inside ema_scope the UNet still ran on the training weights (a stale layout)"
        with torch.no_grad():
            for (_, p), s in zip(named, shadows):
                p.copy_(s)
        assert torch.equal(call(), out_in), "inside ema_scope differs from the same engine with its trained tensors set to the shadows"
    finally:
        engine.use_ema, engine.opt_keys, engine.model_ema = saved
        with torch.no_grad():
            for n, p in named:
                p.copy_(before[n])
