"""Gradient accumulation and EMA on the fused bucket optimiser step: what holds without a GPU.

  * the torch restatement of the window loop (tests/optim_ref.py: accumulate, AdamW, LitEma, in that order), fed with the fp32
    oracle's gradients (oracle/training.py), reproduces every quantity of G16 (tests/golden/optim_golden.npz, the REAL reference's
    loop) to fp32 accuracy — which validates the golden and the order of operations the GPU path is held to;
  * the bucket's layout, the window logic on a stub (launches recorded, none made), ``Ema``'s decays / keys / state dict, the engine
    surface, the in-place collective on gloo, the ABI.

Distances of the restatement from the golden, measured on the build host (fp32 oracle vs fp32 reference, different association
orders; the test prints them), and the pins at 3x:
    losses (worst, relative)                   measured 1.84e-7                       pin 5.6e-7
    accumulated gradients, windows 1 / 2       measured 1.07e-6 / 1.43e-6 rel rms     pin 3.3e-6 / 4.3e-6
    p_k - p_0, windows 1 / 2                   measured 1.51e-6 / 1.02e-6             pin 4.6e-6 / 3.1e-6
    shadow - p_0, updates 2 / 3 / 4            measured 1.58e-6 / 1.63e-6 / 1.05e-6   pin 4.8e-6 / 4.9e-6 / 3.2e-6
(update 1's shadow displacement is exactly zero on both sides.)
"""
import os
import re
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import optim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

PIN_LOSS = 5.6e-7
PIN_GRAD = (3.3e-6, 4.3e-6)
PIN_DP = (4.6e-6, 3.1e-6)
PIN_SHADOW = (0.0, 4.8e-6, 4.9e-6, 3.2e-6)


@pytest.fixture(scope="module")
def g16():
    return np.load(os.path.join(GOLD, "optim_golden.npz"))


# ------------------------------------------------------------------------------------------------ the restatement
def test_restated_window_loop_on_oracle_gradients_reproduces_the_golden(g16):
    from aae_fixture import train_batch
    from oracle import sampling, spec, training as otr
    from udifftext_amd import synth
    torch.set_grad_enabled(False)
    cfg = spec.EngineConfig()
    sd = synth.synthetic_state_dict([(k, s) for k, s in spec.engine_param_shapes(cfg) if k.startswith("model.")])
    sd["denoiser.sigmas"] = sampling.denoiser_sigma_table(1000)
    sd["loss_fn.g_kernel"] = sampling.gaussian_kernel(3, 1.0, 12)
    g14 = np.load(os.path.join(GOLD, "train_golden.npz"))
    tb = train_batch()
    z = torch.from_numpy(g14["g14_z"])
    cond = {"concat": torch.from_numpy(g14["g14_c_concat"]), "t_crossattn": torch.from_numpy(g14["g14_c_txt"])}
    names = [str(n) for n in g16["g16_names"]]
    assert names == otr.trainable_names(sd)
    N = int(g16["g16_accumulate"][0])
    p = {n: sd[n] for n in names}                                      # (updated in place: the oracle reads the same tensors)

    def grad_fn(p_, k):
        idx, noise = torch.from_numpy(g16["g16_sigma_idx"][k]), torch.from_numpy(g16["g16_noise"][k])
        return otr.training_grads(sd, cfg, z, cond, tb["seg"], tb["seg_mask"], idx, noise, lambda_local=0.0)

    out = optim_ref.window_loop(p, grad_fn, 2 * N, N, float(g16["g16_lr"][0]), float(g16["g16_eps"][0]), float(g16["g16_weight_decay"][0]))
    assert out["steps"] == [N, 2 * N]
    np.testing.assert_allclose(out["omd"], g16["g16_one_minus_decay"], rtol=1e-6)
    figures = []                                                        # (name, measured, pin): all printed before any is asserted
    worst = 0.0
    for k, ld in enumerate(out["losses"]):
        for key in ("loss/diff_loss", "loss/full_loss"):
            ref = float(g16[f"g16_{k + 1}_" + key.replace("/", "_")][0])
            worst = max(worst, abs(float(ld[key]) - ref) / abs(ref))
    figures.append(("losses, worst relative distance", worst, PIN_LOSS))
    for w in range(2):
        figures.append((f"window {w + 1} accumulated gradient", optim_ref.rel_sub(out["grads"][w], g16[f"g16_w{w + 1}_grad_sub"], names)[0],
                        PIN_GRAD[w]))
        figures.append((f"window {w + 1} p_k - p_0", optim_ref.rel_sub(out["dp"][w], g16[f"g16_w{w + 1}_dp_sub"], names)[0], PIN_DP[w]))
    assert all(not bool(t.any()) for t in out["shadow"][0].values()) and not g16["g16_1_shadow_sub"].any()
    for j in range(1, 2 * N):
        figures.append((f"EMA update {j + 1} shadow - p_0", optim_ref.rel_sub(out["shadow"][j], g16[f"g16_{j + 1}_shadow_sub"], names)[0],
                        PIN_SHADOW[j]))
    for name, got, pin in figures:
        print(f"{name:40s} {got:.3e} (pin {pin:.1e})")
    for name, got, pin in figures:
        assert got <= pin, (name, got, pin)
    # what the GPU test leans on: the stored conditions
    assert (g16["g16_grad_ratio"] <= 1.5).all() and (g16["g16_shadow_ratio"] <= 1.5).all()


# ------------------------------------------------------------------------------------------------ the bucket's layout
def _named():
    g = torch.Generator().manual_seed(3)
    shapes = (("model.b.weight", (3, 3, 3)), ("model.a.weight", (7, 5)), ("model.a.bias", (5,)), ("model.c.weight", (1280,)))
    return [(n, torch.nn.Parameter(torch.randn(s, generator=g))) for n, s in shapes]


def test_bucket_layout_order_alignment_and_aliasing():
    from udifftext_amd import training
    named = _named()
    b = training.GradBucket(named)
    assert b.names == [n for n, _ in named]
    assert [b.offsets[n] for n in b.names] == [0, 28, 64, 72] and b.total == 1408
    assert all(o % 4 == 0 for o in b.offsets.values()) and b.total % 64 == 0
    assert b.flat.dtype == torch.float32 and not bool(b.flat.any())
    for n, p in named:
        v = b.views[n]
        assert v.shape == p.shape and v.data_ptr() == b.flat.data_ptr() + 4 * b.offsets[n]
        v.fill_(1.0)
    assert float(b.flat.sum()) == sum(p.numel() for _, p in named)           # the views alias the flat buffer; the padding stayed zero
    assert b.zero_() is b and not bool(b.flat.any())


# ------------------------------------------------------------------------------------------------ the window logic
class _Dist:
    def __init__(self, world):
        self.world, self.reduced = world, 0

    def is_initialized(self):
        return True

    def get_world_size(self):
        return self.world

    def get_rank(self):
        return 0

    def get_backend(self):
        return "gloo"

    class ReduceOp:
        SUM = "sum"

    def all_reduce(self, t, op=None):
        self.reduced += 1
        t.mul_(self.world)                                             # every rank holds the same bucket: the sum is world x it


@pytest.mark.parametrize("world", [1, 2])
def test_window_logic_on_a_stub(world):
    """N = 3: the optimiser steps on calls 3 and 6 only, with grad_scale = 1 / (3 * world) on the bucket summed over the ranks; the
    EMA counts 1 .. 6 — fused into the step's launch on calls 3 and 6, the EMA-only launch on the others; the bucket is zero again
    after each step.  (The launches are recorded, not made.)"""
    from udifftext_amd import lib as L, training
    named = _named()
    opt = training.BucketAdamW(named, lr=1e-3, accumulate_grad_batches=3)
    ema = training.Ema(named)
    log = []
    opt._launch = lambda bucket, mode, grad_scale, omd, ema_: log.append(("step", mode, grad_scale, omd, float(bucket.flat.sum()),
                                                                        ema_ is ema))
    ema._launch_update = lambda omd: log.append(("ema", omd))
    dist = _Dist(world)

    def micro(bucket):
        assert bucket is opt.bucket
        for v in bucket.views.values():
            v.add_(1.0)                                                # what the reverse pass does: ADD this micro-batch's gradient
        return {"loss/full_loss": torch.tensor(float(opt.micro_batches))}
    n_el = sum(p.numel() for _, p in named)
    for k in range(6):
        ld = training.window_step(opt, micro, dist, ema=ema)
        assert float(ld["loss/full_loss"]) == k and int(ema.num_updates) == k + 1
        assert opt.step_count == (k + 1) // 3
        if (k + 1) % 3 == 0:
            assert not bool(opt.bucket.flat.any()), "the bucket is not zeroed after the step"
    omd = [optim_ref.one_minus_decay(j + 1) for j in range(6)]
    both = L.BUCKET_ADAMW | L.BUCKET_EMA
    assert log == [("ema", omd[0]), ("ema", omd[1]), ("step", both, 1.0 / (3 * world), omd[2], 3.0 * n_el * world, True),
                   ("ema", omd[3]), ("ema", omd[4]), ("step", both, 1.0 / (3 * world), omd[5], 3.0 * n_el * world, True)]
    assert dist.reduced == (2 if world > 1 else 0)
    # without an EMA: AdamW-only launches, nothing in between
    log.clear()
    opt2 = training.BucketAdamW(named, lr=1e-3, accumulate_grad_batches=3)
    opt2._launch = lambda bucket, mode, grad_scale, omd, ema_: log.append((mode, grad_scale, ema_))
    for k in range(6):
        training.window_step(opt2, lambda b: {}, None)
    assert log == [(L.BUCKET_ADAMW, 1.0 / 3, None)] * 2
    with pytest.raises(ValueError):
        training.BucketAdamW(named, lr=1e-3, accumulate_grad_batches=0)


# ------------------------------------------------------------------------------------------------ Ema
def test_ema_decays_keys_and_state_dict_round_trip(g16):
    from udifftext_amd import training
    named = _named()
    ema = training.Ema(named, decay=0.9999)
    assert list(ema.state_dict()) == ["decay", "num_updates", "bweight", "aweight", "abias", "cweight"]
    assert ema.m_name2s_name == {"b.weight": "bweight", "a.weight": "aweight", "a.bias": "abias", "c.weight": "cweight"}
    assert all(torch.equal(s, p) and s.data_ptr() != p.data_ptr() for s, (_, p) in zip(ema.shadows(), named))
    got = [ema.next_one_minus_decay() for _ in range(4)]
    np.testing.assert_allclose(got, g16["g16_one_minus_decay"], rtol=1e-7)               # LitEma's own, recorded by the generator
    np.testing.assert_allclose(got, [9 / 11, 9 / 12, 9 / 13, 9 / 14], rtol=1e-6)
    assert int(ema.num_updates) == 4 and ema.num_updates.dtype == torch.int32
    ema._host = (ema._host[0], 200_000)                                  # far along: the configured decay caps the warm-up
    assert ema.next_one_minus_decay() == pytest.approx(1e-4, rel=2e-3)
    fixed = training.Ema(named, decay=0.5, use_num_updates=False)
    assert int(fixed.num_updates) == -1 and fixed.next_one_minus_decay() == 0.5 and int(fixed.num_updates) == -1
    with pytest.raises(ValueError):
        training.Ema(named, decay=1.5)
    # the golden's key list (the reference's LitEma over the trained tensors) is what the real names produce
    names = [str(n) for n in g16["g16_names"]]
    big = training.Ema([(n, torch.nn.Parameter(torch.zeros(1))) for n in names])
    keys = ["model_ema." + k for k in big.state_dict()]
    assert keys == [str(k) for k in g16["g16_ema_keys"]] and int(g16["g16_ema_trained"].sum()) == len(names) == 112
    # round trip under the engine's prefix, num_updates included; shadows of untrained tensors in a checkpoint are ignored
    holder = torch.nn.Module()
    holder.model_ema = training.Ema(named)
    holder.model_ema.next_one_minus_decay()
    for s in holder.model_ema.shadows():
        s.add_(1.0)
    sd = holder.state_dict()
    assert list(sd) == ["model_ema." + k for k in ("decay", "num_updates", "bweight", "aweight", "abias", "cweight")]
    other = torch.nn.Module()
    other.model_ema = training.Ema(named, untrained_names=["model.untrained.weight"])
    assert other.model_ema.names == [n for n, _ in named]
    sd["model_ema.untrainedweight"] = torch.zeros(3)                      # a shadow of one of the model's untrained tensors: ignored
    missing, unexpected = other.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    sd["model_ema.aweigth"] = torch.zeros(3)                              # a name the model does not have: reported
    with pytest.raises(RuntimeError, match="model_ema.aweigth"):
        other.load_state_dict(sd, strict=True)
    assert other.load_state_dict(sd, strict=False).unexpected_keys == ["model_ema.aweigth"]
    assert all(torch.equal(a, b) for a, b in zip(other.model_ema.shadows(), holder.model_ema.shadows()))
    assert int(other.model_ema.num_updates) == 1 and other.model_ema.next_one_minus_decay() == optim_ref.one_minus_decay(2)


def test_ema_copy_to_without_store_overwrites_as_litema_does():
    from udifftext_amd import training
    named = _named()
    ema = training.Ema(named)
    for s in ema.shadows():
        s.mul_(2.0)
    want = [s.clone() for s in ema.shadows()]
    v0 = [p._version for _, p in named]
    ema.copy_to()
    assert all(torch.equal(p, w) for (_, p), w in zip(named, want)) and all(torch.equal(s, w) for s, w in zip(ema.shadows(), want))
    assert all(p._version > v for (_, p), v in zip(named, v0))


def test_ema_store_keeps_no_copy_and_copy_to_refuses_changed_parameters():
    from udifftext_amd import training
    named = _named()
    ema = training.Ema(named)
    ema.store()
    with torch.no_grad():
        named[0][1].add_(1.0)
    with pytest.raises(RuntimeError, match="changed between"):
        ema.copy_to()
    ema.restore()                                                      # nothing was swapped: nothing to undo
    assert not ema._stored and not ema._swapped


# ------------------------------------------------------------------------------------------------ the engine surface
def test_engine_constructs_with_use_ema_and_ema_scope_without_it_is_a_no_op():
    import udifftext_amd  # noqa: F401
    from sgm.util import instantiate_from_config, skip_param_init
    from udifftext_amd import config as C, training
    cfg = C.default_model_config()
    cfg.model.params.use_ema = True
    cfg.model.params.opt_keys = ["t_attn", "t_norm"]
    with skip_param_init():
        eng = instantiate_from_config(cfg.model)
    assert eng.use_ema and isinstance(eng.model_ema, training.Ema)
    named = training.trainable_parameters(eng)
    assert len(named) == 112 and len(eng.model_ema.shadows()) == 112
    keys = [k for k in eng.state_dict() if k.startswith("model_ema.")]
    assert len(keys) == 114 and keys[:2] == ["model_ema.decay", "model_ema.num_updates"]
    opt = eng.configure_optimizers(1e-4, fused=True, accumulate_grad_batches=4)
    assert isinstance(opt, training.BucketAdamW) and opt.accumulate_grad_batches == 4 and opt.bucket.total >= 75_936_320
    assert training.engine_ema(eng) is eng.model_ema
    assert type(eng.configure_optimizers(1e-4)) is training.AdamW          # the default is what it returned before
    with pytest.raises(NotImplementedError):
        eng.configure_optimizers(1e-4, accumulate_grad_batches=2)
    # the per-tensor route's training_step moves the EMA as well (one hook, one contract): once per call
    log = []
    eng.model_ema._launch_update = lambda omd: log.append(omd)
    eng.shared_step = lambda batch, bucket=None: ({"loss/full_loss": torch.tensor(0.0)}, {})
    stub = types.SimpleNamespace(named=[], step=lambda grads: log.append("step"))
    eng.training_step({}, stub)
    eng.training_step({}, stub)
    assert log == ["step", optim_ref.one_minus_decay(1), "step", optim_ref.one_minus_decay(2)] and int(eng.model_ema.num_updates) == 2
    del eng.__dict__["shared_step"]
    # without use_ema: no shadows, ema_scope and on_train_batch_end do nothing
    eng.use_ema, eng.model_ema = False, None
    assert training.engine_ema(eng) is None
    p = named[0][1]
    with torch.no_grad():
        p.fill_(1.0)                                                   # (skip_param_init left the memory as it was: it may hold NaN)
    v0, before = p._version, p.detach().clone()
    with eng.ema_scope("test"):
        assert torch.equal(p, before)
    eng.on_train_batch_end()
    assert p._version == v0 and not [k for k in eng.state_dict() if k.startswith("model_ema.")]


def test_pretrained_sd2_mapping_still_drops_model_ema():
    """a pretrained SD-2 file's shadows are not UDiffText's: the mapper drops them even when the engine has keys of that name"""
    from udifftext_amd import ckpt
    sd = {"model_ema.decay": torch.zeros(()), "model_ema.diffusion_modelx": torch.zeros(2), "model.diffusion_model.out.2.bias": torch.ones(4)}
    out, rep = ckpt.map_sd2_inpainting(sd, ["model.diffusion_model.out.2.bias", "model_ema.decay", "model_ema.diffusion_modelx"])
    assert list(out) == ["model.diffusion_model.out.2.bias"]
    assert set(rep["dropped_other"]) == {"model_ema.decay", "model_ema.diffusion_modelx"}


# ------------------------------------------------------------------------------------------------ the collective
def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from udifftext_amd import training
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda t, *a, **k: (calls.append(t.data_ptr()), real(t, *a, **k))[1]
    named = [("b.weight", torch.zeros((3, 3, 3))), ("a.weight", torch.zeros((7, 5))), ("a.bias", torch.zeros((5,)))]
    b = training.GradBucket(named)
    g = torch.Generator().manual_seed(100 + rank)
    for n, _ in named:
        b.views[n].copy_(torch.randn(b.views[n].shape, generator=g))
    ptr = b.flat.data_ptr()
    b.average(dist)
    out[rank] = ({k: v.clone() for k, v in b.views.items()}, calls == [ptr], b.flat.data_ptr() == ptr)
    dist.barrier()
    dist.destroy_process_group()


def test_bucket_average_over_two_ranks_is_one_in_place_sum():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(2, port, out), nprocs=2, join=True)
    ref = {}
    for r in range(2):
        g = torch.Generator().manual_seed(100 + r)
        for k, shp in (("b.weight", (3, 3, 3)), ("a.weight", (7, 5)), ("a.bias", (5,))):
            ref[k] = ref.get(k, 0) + torch.randn(shp, generator=g)           # the SUM: 1 / world is the update's grad_scale
    for r in range(2):
        views, one_call_on_the_buffer, same_buffer = out[r]
        assert one_call_on_the_buffer and same_buffer
        for k in ref:
            assert torch.allclose(views[k], ref[k], rtol=1e-6, atol=1e-7), (r, k)


# ------------------------------------------------------------------------------------------------ the ABI
def test_new_entry_points_are_declared_and_the_parents_keep_their_signatures():
    from udifftext_amd import lib as L
    text = open(os.path.join(ROOT, "include", "udt_kernels.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def n_args(name):
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, name
        return len([a for a in m.group(1).split(",") if a.strip()])
    new = {"udt_wgrad_bf16_acc": 11, "udt_colsum_bf16_acc": 7, "udt_ln_param_grad_acc": 9, "udt_bucket_update_f32": 16, "udt_bucket_swap_f32": 4}
    parents = {"udt_wgrad_bf16": 10, "udt_colsum_bf16": 6, "udt_ln_param_grad": 8, "udt_adamw_f32": 13}
    for name, n in {**new, **parents}.items():
        assert name in L.SYMBOLS and n_args(name) == n == len(L.SYMBOLS[name][1]), name
    for parent in ("udt_wgrad_bf16", "udt_colsum_bf16", "udt_ln_param_grad"):           # the parent plus one int32 before the stream
        a, b = L.SYMBOLS[parent][1], L.SYMBOLS[parent + "_acc"][1]
        assert b == a[:-1] + [L._i32, a[-1]]
    import ctypes
    assert ctypes.sizeof(L.BucketSegment) == 32 and L.BUCKET_CHUNK == int(re.search(r"#define UDT_BUCKET_CHUNK (\d+)", text).group(1))
