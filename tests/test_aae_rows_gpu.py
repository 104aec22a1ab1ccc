"""The row-wise attend-and-excite loop on the MI355X: udt_aae_row_update_f32 against the restated rule (tests/aae_rows_ref.py) and the real
reference's B = 1 loop (tests/golden/aae_rows_golden.npz), EulerEDMSampler.attend_and_excite_rows against attend_and_excite at B = 1 and
against the written-out row-wise loop at B = 2, independence of a row from its batch mate, attend_and_excite at B = 2 against its
restated rule, results that alias neither the runner's static latent nor the caller's x, the sampler's schedule
(sample_rows_with_attend_and_excite) and pipeline.predict_many with cfgs.aae_enabled end to end.

Reference: sgm/modules/diffusionmodules/sampling.py:233-252,355-420.
"""
import os

import numpy as np
import pytest
import torch

import aae_rows_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I32 = torch.int32


def _rel(got, ref):
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300)).item()


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import backward, lib, ops, pipeline
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)

    class Env:
        pass
    Env.ops, Env.bw, Env.pipeline, Env.lib, Env.L, Env.dev = ops, backward, pipeline, lib.load(), lib, cuda
    return Env


@pytest.fixture(scope="module")
def engine(env):
    return env.pipeline.build_engine(env.dev)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "aae_rows_golden.npz"))


@pytest.fixture(scope="module")
def g15():
    return np.load(os.path.join(GOLD, "iterated_golden.npz"))


# ------------------------------------------------------------------------------------------------ the kernel
MAX_ITER, THRES, ALPHA = 20, -0.5, 1.75
NAN = float("nan")


def _patterns(B):
    """name -> (active, counts, loss, poisoned (frozen) rows, iter_enabled)"""
    alt = [(b + 1) % 2 for b in range(B)]                                 # row 0 active, row 1 frozen, ...
    above, mixed_loss = [0.25] * B, [0.25 if b % 3 != 2 else -0.75 for b in range(B)]
    return {
        "all active": ([1] * B, [b % 5 for b in range(B)], mixed_loss, [], 1),
        "all frozen": ([0] * B, [3] * B, above, [], 1),
        "mixed": (alt, [2] * B, mixed_loss, [], 1),
        "NaN loss in an active row": ([1] * B, [3] * B, [NAN] + above[1:], [], 1),
        "NaN in a frozen row's grad and loss": ([0] + [1] * (B - 1), [4] * B, above, [0], 1),
        "it exactly at max_iter": ([1] * B, [MAX_ITER - 1] * B, above, [], 1),
        "it at max_iter + 1": ([1] * B, [MAX_ITER] * B, above, [], 1),
        "iter_enabled 0": ([1] * B, [0] * B, above, [], 0),
        "active value 7": ([7] * B, [1] * B, mixed_loss, [], 1),
    }


@pytest.mark.parametrize("B,n", [(1, 4), (1, 1024), (1, 1028), (3, 1028), (5, 1024), (2, 6144)])
def test_kernel_vs_the_restated_rule(env, B, n):
    """active rows bit-equal to ops.axpy_ on the row, frozen rows bit-equal to their input, state_out and n_active exactly the rule's"""
    dev, ops = env.dev, env.ops
    g = torch.Generator().manual_seed(1000 * B + n)
    for name, (active, counts, loss, poisoned, en) in _patterns(B).items():
        x0, grad = torch.randn((B, n), generator=g), torch.randn((B, n), generator=g) * 0.1
        ls = torch.tensor(loss, dtype=torch.float32)
        for b in poisoned:
            grad[b] = NAN
            ls[b] = NAN
        st = torch.tensor([active, counts], dtype=I32)
        _, so_ref, na_ref = R.row_update(x0, grad, ls, st, ALPHA, THRES, en, MAX_ITER)
        x, gd = x0.to(dev), grad.to(dev)
        so, na = torch.full((2, B), -77, dtype=I32, device=dev), torch.full((1,), -77, dtype=I32, device=dev)
        ops.aae_row_update_(x, gd, ls.to(dev), st.to(dev), so, na, ALPHA, THRES, en, MAX_ITER)
        for b in range(B):
            if active[b]:
                want = ops.axpy_(x0[b].to(dev).contiguous(), gd[b].contiguous(), -ALPHA)
            else:
                want = x0[b].to(dev)
            assert torch.equal(x[b].view(I32), want.view(I32)), (name, b, "active" if active[b] else "frozen")
        assert so.cpu().tolist() == so_ref.tolist(), (name, so.cpu().tolist(), so_ref.tolist())
        assert int(na.cpu()[0]) == na_ref, (name, int(na.cpu()[0]), na_ref)
    # what the patterns are there for, stated once on the rule itself
    p = _patterns(B)
    ref = lambda k: R.row_update(torch.zeros((B, n)), torch.zeros((B, n)), torch.tensor(p[k][2]), torch.tensor(p[k][:2], dtype=I32),
                                 ALPHA, THRES, p[k][4], MAX_ITER)
    assert ref("NaN loss in an active row")[1][0, 0] == 1 and ref("it exactly at max_iter")[2] == B
    assert ref("it at max_iter + 1")[2] == 0 and ref("iter_enabled 0")[2] == 0 and ref("all frozen")[2] == 0


def test_kernel_refusals(env):
    dev, lib = env.dev, env.lib
    x, gr, ls = torch.zeros((2, 8), device=dev), torch.zeros((2, 8), device=dev), torch.zeros((2,), device=dev)
    s0, s1, na = torch.ones((2, 2), dtype=I32, device=dev), torch.full((2, 2), -5, dtype=I32, device=dev), torch.full((1,), -5, dtype=I32, device=dev)
    p = lambda t: t.data_ptr()
    call = lambda x_, s_in, s_out, B, n, max_iter=20: lib.udt_aae_row_update_f32(p(x_), p(gr), p(ls), p(s_in), p(s_out), p(na), B, n, 1.0, 0.0,
                                                                                 1, max_iter, None)
    assert call(x, s0, s1, 1, 6) == -1                                     # n % 4 != 0
    assert call(x.view(-1)[1:], s0, s1, 1, 4) == -1                        # x not 16-byte aligned
    assert call(x, s0, s1, 1025, 4) == -1
    assert call(x, s0, s0, 2, 8) == -2                                     # aliased state buffers
    assert call(x, s0, s0.view(-1)[1:], 1, 8) == -2                        # overlapping by one word ([2, 1] at s0 and at s0 + 1 word)
    assert call(x, s0, s1, 0, 8) == -2
    assert call(x, s0, s1, 2, 0) == -2
    assert call(x, s0, s1, 2, 8, max_iter=-1) == -2
    assert lib.udt_aae_row_update_f32(None, p(gr), p(ls), p(s0), p(s1), p(na), 2, 8, 1.0, 0.0, 1, 20, None) == -2
    torch.cuda.synchronize()
    assert not bool(x.any()) and bool((s1 == -5).all()) and int(na[0]) == -5, "a refused call launched"
    with pytest.raises(ValueError):
        env.ops.aae_row_update_(torch.zeros((1, 6), device=dev), torch.zeros((1, 6), device=dev), ls[:1], s0[:, :1].contiguous(),
                                s1[:, :1].contiguous(), na, 1.0, 0.0, True, 20)


def _device_loop(env, x0, evaluate, alpha, thres, en, max_iter):
    """the row loop through ops.aae_row_update_ with ping-pong state buffers -> (x, counts, evaluations)"""
    dev, B = env.dev, x0.shape[0]
    x = x0.clone()
    s_in, s_out = torch.zeros((2, B), dtype=I32, device=dev), torch.zeros((2, B), dtype=I32, device=dev)
    s_in[0] = 1
    na = torch.zeros((1,), dtype=I32, device=dev)
    evals = 0
    while True:
        loss, grad = evaluate(x)
        env.ops.aae_row_update_(x, grad.contiguous(), loss.contiguous(), s_in, s_out, na, alpha, thres, en, max_iter)
        s_in, s_out = s_out, s_in
        evals += 1
        assert evals <= max_iter + 1
        if int(na.item()) == 0:
            break
    return x, s_in[1].cpu(), evals


def test_golden_through_the_kernel(env, gold):
    """the golden's samples, each group stacked into one batch, driven through ops.aae_row_update_ with the toy's loss and gradient
    computed by torch on the device: the reference's counts exactly; x_final within aae_rows_ref.displacement_bound (as on the CPU) plus
    what the toy's device arithmetic adds — k updates of alpha * (device gradient - CPU gradient), that difference measured here on
    x0 and itself held to 8 roundings of the gradient's size (the 4 fp32 operations a side displacement_bound assumes)."""
    dev, alpha = env.dev, float(gold["alpha"][0])
    for g in range(gold["group_thres"].shape[0]):
        rows = np.nonzero(gold["group"] == g)[0]
        x0, w, t = (torch.from_numpy(gold[k][rows]) for k in ("x0", "toy_w", "toy_t"))
        c = torch.from_numpy(gold["toy_c"][rows])
        thres, max_iter, en = float(gold["group_thres"][g]), int(gold["group_max_iter"][g]), bool(gold["group_iter_enabled"][g])
        wd, td, cd = w.to(dev), t.to(dev), c.to(dev)
        l_cpu, g_cpu = R.toy_loss_grad(x0, w, t, c)
        l_dev, g_dev = R.toy_loss_grad(x0.to(dev), wd, td, cd)
        dg = float((g_dev.cpu() - g_cpu).abs().max())
        dl = float((l_dev.cpu() - l_cpu).abs().max())
        print(f"group {g}: toy device vs CPU on x0: max |d grad| {dg:.3e} (max |grad| {float(g_cpu.abs().max()):.3e}), max |d loss| {dl:.3e}")
        assert dg <= 8 * 2.0 ** -24 * float(g_cpu.abs().max()) and dl <= 1e-4          # (loss: a tenth of the golden's margin)
        xf, counts, evals = _device_loop(env, x0.to(dev), lambda x: R.toy_loss_grad(x, wd, td, cd), alpha, thres, en, max_iter)
        assert counts.tolist() == gold["counts"][rows].tolist(), (g, counts.tolist(), gold["counts"][rows].tolist())
        assert evals == int(gold["counts"][rows].max())
        for r, s in enumerate(rows):
            k = int(gold["counts"][s])
            ref = torch.from_numpy(gold["x_final"][s])
            bound = R.displacement_bound(k, alpha, x0[r], ref, g_cpu[r]) + k * alpha * dg
            err = float((xf[r].cpu() - ref).abs().max())
            print(f"group {g} sample {s}: {k} updates, max |x_final - reference| {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (g, s, err, bound)


# ------------------------------------------------------------------------------------------------ the loop
def _g13_cond(dev):
    g13 = np.load(os.path.join(GOLD, "aae_golden.npz"))
    return {"concat": torch.from_numpy(g13["g13_c_concat"]).to(dev), "t_crossattn": torch.from_numpy(g13["g13_c_txt"]).to(dev)}


def _aae_point(env, g):
    """the G13 point of G15a: x_0, sigma, alpha, the golden's conditioning, the masks of aae_batch()"""
    from aae_fixture import aae_batch
    dev = env.dev
    b = aae_batch()
    batch = {"mask": b["mask"].to(dev), "seg_mask": b["seg_mask"].to(dev)}
    x0 = torch.from_numpy(g["g15a_ii_x"][0]).to(dev)
    sigma = torch.from_numpy(g["g15a_sigma"]).to(dev)
    return x0, sigma, float(g["g15a_alpha"][0]), _g13_cond(dev), batch


class _graph_mode:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        import sgm.modules.diffusionmodules.sampling as S
        S.AAE_GRAPH = self.on

    def __exit__(self, *a):
        import sgm.modules.diffusionmodules.sampling as S
        S.AAE_GRAPH = True


@pytest.mark.parametrize("case,thres,max_iter,n_updates", [("i", 1e3, 20, 1), ("ii", -1e3, 2, 3)])
def test_rows_loop_equals_attend_and_excite_at_batch_1(engine, env, g15, case, thres, max_iter, n_updates):
    """B = 1 at the G13 point, G15a's two exits: attend_and_excite_rows is attend_and_excite bit for bit, with the same number of
    evaluations — through the captured runner (one runner serves both methods) and through eager launches"""
    x0, sigma, alpha, c, batch = _aae_point(env, g15)
    outs = []
    for graph in (True, False):
        with _graph_mode(graph):
            sampler = env.pipeline.init_sampling(10, 5.0, env.dev)
            ref = sampler.attend_and_excite(x0, engine, sigma, c, batch, alpha, True, thres, max_iter=max_iter)
            n_ref = sampler.aae_evaluations
            runner = getattr(sampler, "_aae_runner", None)
            assert (runner is not None) == graph
            x, iters = sampler.attend_and_excite_rows(x0, engine, sigma, c, batch, alpha, True, thres, max_iter=max_iter)
            assert getattr(sampler, "_aae_runner", None) is runner               # (the same captured evaluation)
        assert n_ref == n_updates and sampler.aae_evaluations - n_ref == n_updates, (graph, n_ref, sampler.aae_evaluations)
        assert iters.dtype == torch.int32 and iters.is_cuda and iters.tolist() == [n_updates]
        assert sampler.aae_row_updates.tolist() == [n_updates] and sampler.aae_frozen_row_evaluations == 0
        assert torch.equal(x, ref), (case, graph)
        outs.append(x)
    assert torch.equal(outs[0], outs[1]), "hipGraph runner and eager launches differ"
    # iter_enabled off: one evaluation, whatever thres says
    sampler = env.pipeline.init_sampling(10, 5.0, env.dev)
    ref = sampler.attend_and_excite(x0, engine, sigma, c, batch, alpha, False, thres, max_iter=max_iter)
    x, iters = sampler.attend_and_excite_rows(x0, engine, sigma, c, batch, alpha, False, thres, max_iter=max_iter)
    assert torch.equal(x, ref) and iters.tolist() == [1] and sampler.aae_evaluations == 2


@pytest.fixture(scope="module")
def pair(engine, env, g15):
    """the B = 2 construction of test_attend_and_excite_loop_is_per_sample_at_batch_2 (tests/test_iterated_gpu.py): the G13 sample
    stacked with a second one (another latent, the mask on another cell), thres between the two first losses"""
    x0, sigma, alpha, c, batch = _aae_point(env, g15)
    dev = env.dev
    x1 = torch.randn((1, 4, 16, 16), generator=torch.Generator().manual_seed(77)) * float(sigma[0])
    mask1 = torch.zeros_like(batch["mask"].cpu())
    mask1[:, :, 24:32, 80:88] = 1.0                                        # latent cell (3, 10)
    x = torch.cat([x0, x1.to(dev)])
    s2 = sigma.reshape(1).repeat(2)
    c2 = {k: v.repeat((2,) + (1,) * (v.dim() - 1)) for k, v in c.items()}
    b2 = {"mask": torch.cat([batch["mask"], mask1.to(dev)]), "seg_mask": batch["seg_mask"].repeat(2, 1)}
    sampler = env.pipeline.init_sampling(10, 5.0, dev)
    c_noise = sampler.get_c_noise(x, engine, s2).float()
    unet = engine.model.diffusion_model
    ev = lambda xx, bb=b2: env.bw.unet_local_loss_grad(unet, engine.loss_fn, xx, c_noise, c2["concat"], c2["t_crossattn"], bb["mask"],
                                                       bb["seg_mask"])
    loss, grad = ev(x)
    l0 = [float(v) for v in loss]
    assert l0[0] != l0[1]

    class P:
        pass
    P.x, P.s2, P.c2, P.b2, P.alpha, P.ev, P.loss0, P.grad0 = x, s2, c2, b2, alpha, ev, loss.clone(), grad.clone()
    P.thres, P.max_iter, P.low = 0.5 * (l0[0] + l0[1]), 2, int(l0[1] < l0[0])
    return P


def _rows_run(env, engine, graph, P, x=None, b2=None):
    with _graph_mode(graph):
        sampler = env.pipeline.init_sampling(10, 5.0, env.dev)
        xr, iters = sampler.attend_and_excite_rows(P.x if x is None else x, engine, P.s2, P.c2, P.b2 if b2 is None else b2, P.alpha, True,
                                                   P.thres, max_iter=P.max_iter)
    assert (getattr(sampler, "_aae_runner", None) is not None) == graph
    return sampler, xr, iters.cpu().tolist()


def test_rows_loop_freezes_each_row_on_its_own_at_batch_2(engine, env, pair):
    """thres between the two first losses: the row below it takes exactly ONE update and keeps that value, bit for bit, while the
    other row goes on; both rows match the row-wise loop written out on the eager batched evaluation (atol 1e-6, as
    test_attend_and_excite_loop_is_per_sample_at_batch_2 holds the .all() loop), with equal counts; captured == eager, bit for bit"""
    P = pair
    xm, active, cnt, evals, frozen = P.x.clone(), [True, True], [0, 0], 0, 0
    while any(active):
        lk, gk = P.ev(xm)
        evals += 1
        frozen += active.count(False)
        for b in range(2):
            if active[b]:
                xm[b] = xm[b] - P.alpha * gk[b]
                cnt[b] += 1
                active[b] = not (float(lk[b]) <= P.thres) and not (cnt[b] > P.max_iter)
    assert cnt[P.low] == 1 and cnt[1 - P.low] >= 2, ("precondition: one row freezes at once, the other goes on", cnt)
    one = env.ops.axpy_(P.x[P.low].clone().contiguous(), P.grad0[P.low].contiguous(), -P.alpha)
    outs = []
    for graph in (True, False):
        sm, xr, iters = _rows_run(env, engine, graph, P)
        assert iters == cnt, (graph, iters, cnt)
        assert sm.aae_evaluations == evals and sm.aae_row_updates.tolist() == cnt and sm.aae_frozen_row_evaluations == frozen
        assert torch.equal(xr[P.low], one), (graph, "the frozen row moved after its one update")
        assert torch.allclose(xr, xm, rtol=0, atol=1e-6)
        outs.append(xr)
    assert torch.equal(outs[0], outs[1]), "hipGraph runner and eager launches differ"


def test_a_row_owes_nothing_to_its_batch_mate(engine, env, pair):
    """the B = 2 run again with ONE row's latent and mask replaced so that the replaced row freezes at another iteration: the kept
    row's x and count are the same, bit for bit (DESIGN.md §5's "a sample owes nothing to its mates' values at a fixed batch size",
    extended to the reverse pass and the loop).  Both ways round: row 1 replaced and row 0 kept (as the loop test has it), and row 0
    replaced with the row that runs to the cap kept — three updates beside a mate that freezes after one in one run and runs on in
    the other.  Candidates for the new row are tried in order until one's first loss lies on the other side of thres than the old
    row's (the last, a copy of the kept row, does by construction)."""
    P, dev = pair, env.dev
    sig = float(P.s2[0])
    base = {graph: _rows_run(env, engine, graph, P)[1:] for graph in (True, False)}
    for keep in (0, 1):
        swap = 1 - keep
        cands = []
        for seed, (r0, c0) in ((78 + 10 * keep, (80, 24)), (79 + 10 * keep, (96, 96))):
            m = torch.zeros_like(P.b2["mask"][:1])
            m[:, :, r0:r0 + 8, c0:c0 + 8] = 1.0
            cands.append((torch.randn((1, 4, 16, 16), generator=torch.Generator().manual_seed(seed)).to(dev) * sig, m))
        cands.append((P.x[keep:keep + 1].clone(), P.b2["mask"][keep:keep + 1].clone()))
        was_below = float(P.loss0[swap]) <= P.thres
        for xn, mn in cands:
            xv, mv = P.x.clone(), P.b2["mask"].clone()
            xv[swap], mv[swap] = xn[0], mn[0]
            bv = {"mask": mv, "seg_mask": P.b2["seg_mask"]}
            lv, _ = P.ev(xv, bv)
            if (float(lv[swap]) <= P.thres) != was_below:
                break
        else:
            raise AssertionError("precondition: no candidate row freezes at another iteration")
        assert torch.equal(lv[keep], P.loss0[keep]), "the kept row's loss moved with its mate's values (eager evaluation)"
        for graph in (True, False):
            xa, ia = base[graph]
            _, xb, ib = _rows_run(env, engine, graph, P, x=xv, b2=bv)
            assert ia[swap] != ib[swap], ("precondition: the replaced row freezes at another iteration", ia, ib)
            assert ia[keep] == ib[keep], (graph, keep, ia, ib)
            d = float((xa[keep] - xb[keep]).abs().max())
            print(f"graph {graph}: row {keep} with row {swap} replaced: counts {ia} -> {ib}, max |d x[{keep}]| {d:.3e}")
            assert torch.equal(xa[keep], xb[keep]), (graph, keep, d)


# ------------------------------------------------------------------------------------------------ the joint loop at B = 2
@pytest.fixture(scope="module")
def joint(engine, env, g15):
    """the G13 sample stacked with a second row: the same conditioning and masks, 0.5 * x; the eager batched evaluation and the two
    rows' losses at the start"""
    x0, sigma, alpha, c, batch = _aae_point(env, g15)
    two = lambda v: v.repeat((2,) + (1,) * (v.dim() - 1))
    x = torch.cat([x0, 0.5 * x0])
    s2, c2, b2 = sigma.reshape(1).repeat(2), {k: two(v) for k, v in c.items()}, {k: two(v) for k, v in batch.items()}
    sampler = env.pipeline.init_sampling(10, 5.0, env.dev)
    c_noise = sampler.get_c_noise(x, engine, s2).float()
    unet = engine.model.diffusion_model
    ev = lambda xx: env.bw.unet_local_loss_grad(unet, engine.loss_fn, xx, c_noise, c2["concat"], c2["t_crossattn"], b2["mask"], b2["seg_mask"])

    class P:
        pass
    P.x, P.s2, P.c2, P.b2, P.alpha, P.ev, P.loss0 = x, s2, c2, b2, alpha, ev, [float(v) for v in ev(x)[0]]
    return P


def test_joint_loop_equals_its_restated_rule_at_batch_2(engine, env, joint):
    """attend_and_excite at B = 2 against its rule written out on public pieces (backward.unet_local_loss_grad, ops.axpy_, the stop
    rule ``not iter_enabled or (loss <= thres).all() or iters > max_iter`` over all rows jointly): bit-equal latents and the same
    number added to aae_evaluations, through the captured runner (the loop runs on its static latent) and through eager launches.
    thres +1e9: one update; -1e9: to the cap, max_iter + 1 updates; the mean of the two rows' first losses: whatever the rule gives
    (printed)."""
    P, max_iter = joint, 3
    samplers = {graph: env.pipeline.init_sampling(10, 5.0, env.dev) for graph in (True, False)}
    for name, thres in (("+1e9", 1e9), ("-1e9", -1e9), ("mean of the first losses", 0.5 * (P.loss0[0] + P.loss0[1]))):
        x, iters = P.x.clone(), 0
        while True:
            loss, grad = P.ev(x)
            env.ops.axpy_(x, grad, -P.alpha)
            iters += 1
            if bool((loss <= thres).all()) or iters > max_iter:
                break
        print(f"thres {name} ({thres:.6g}; first losses {P.loss0}): the restated rule takes {iters} updates")
        if name != "mean of the first losses":
            assert iters == (1 if thres > 0 else max_iter + 1), (name, iters)
        for graph, sampler in samplers.items():
            n0 = getattr(sampler, "aae_evaluations", 0)
            with _graph_mode(graph):
                got = sampler.attend_and_excite(P.x, engine, P.s2, P.c2, P.b2, P.alpha, True, thres, max_iter=max_iter)
            assert (getattr(sampler, "_aae_runner", None) is not None) == graph
            assert sampler.aae_evaluations - n0 == iters, (name, graph, sampler.aae_evaluations - n0, iters)
            assert torch.equal(got.view(I32), x.view(I32)), (name, graph, float((got - x).abs().max()))


def test_update_results_alias_neither_the_runner_nor_the_input(engine, env, joint):
    """both update functions through the captured runner: a result keeps its bits when the next call reloads and updates the runner's
    static latent, the callers' x are not written, and no result shares storage with the static buffer"""
    P = joint
    sampler = env.pipeline.init_sampling(10, 5.0, env.dev)
    updates = {"attend_and_excite": sampler.attend_and_excite, "attend_and_excite_rows": lambda *a, **k: sampler.attend_and_excite_rows(*a, **k)[0]}
    for name, update in updates.items():
        x_a, x_b = P.x.clone(), (0.75 * P.x).contiguous()
        a0, b0 = x_a.clone(), x_b.clone()
        r_a = update(x_a, engine, P.s2, P.c2, P.b2, P.alpha, True, -1e9, max_iter=1)          # (two updates of every row)
        bits = r_a.clone()
        r_b = update(x_b, engine, P.s2, P.c2, P.b2, P.alpha, True, -1e9, max_iter=1)
        static = sampler._aae_runner.x
        assert torch.equal(r_a.view(I32), bits.view(I32)), (name, "the first result changed with the second call")
        assert not torch.equal(r_a, r_b) and not torch.equal(r_a, a0), (name, "precondition: the calls update, and differ")
        assert torch.equal(x_a.view(I32), a0.view(I32)) and torch.equal(x_b.view(I32), b0.view(I32)), (name, "a caller's x was written")
        ptrs = [t.untyped_storage().data_ptr() for t in (static, r_a, r_b, x_a, x_b)]
        assert len(set(ptrs)) == len(ptrs), (name, "shared storage", ptrs)
        assert torch.equal(static.view(I32), r_b.view(I32))                  # (the static latent is where the last call left it)


# ------------------------------------------------------------------------------------------------ the sampler and predict_many
def _decided_pair(engine, env):
    """two 128 x 128 images (16 x 16 latents) with masks that decide the loss's hard selections (tests/aae_fixture.py): one mask cell
    and one scored token per row"""
    from udifftext_amd import synth
    b = synth.synthetic_batch(2, 128, 128, 4, seed=13)
    mask = torch.zeros_like(b["mask"])
    mask[0, :, 56:64, 40:48] = 1.0
    mask[1, :, 24:32, 80:88] = 1.0
    b["mask"], b["masked"] = mask, b["image"] * (1.0 - mask)
    seg = torch.zeros_like(b["seg_mask"])
    seg[:, 0] = 1.0
    b["seg_mask"] = seg
    batch, buc = env.pipeline.prepare_batch(b, env.dev)
    c, uc = engine.conditioner.get_unconditional_conditioning(batch, batch_uc=buc, force_uc_zero_embeddings=["label"])
    return batch, c, uc


def test_sampler_rows_schedule_at_batch_2(engine, env, capsys):
    batch, c, uc = _decided_pair(engine, env)
    x0 = torch.randn((2, 4, 16, 16), generator=torch.Generator().manual_seed(5)).to(env.dev)
    sampler = env.pipeline.init_sampling(10, 5.0, env.dev)
    z = sampler.sample_rows_with_attend_and_excite(engine, x0.clone(), c, batch, uc)
    assert capsys.readouterr().out == ""                                   # no print
    assert bool(torch.isfinite(z).all()) and z.shape == x0.shape
    ll = sampler.last_row_losses
    assert tuple(ll.shape) == (10, 2) and not ll.is_cuda and bool(torch.isfinite(ll).all())
    rows, evals = sampler.aae_row_updates.tolist(), sampler.aae_evaluations
    print(f"10 steps, B = 2: {evals} evaluations, row updates {rows}, frozen-row evaluations {sampler.aae_frozen_row_evaluations}")
    assert all(10 <= r <= 10 + 2 * 20 for r in rows) and max(rows) <= evals <= 10 + 2 * 20
    assert 2 * evals - sum(rows) == sampler.aae_frozen_row_evaluations
    plain = sampler(engine, x0.clone(), cond=c, batch=batch, uc=uc)
    assert _rel(z, plain) > 1e-3, "attend-and-excite changed nothing"
    fast = env.pipeline.init_sampling(10, 5.0, env.dev)
    z2 = fast.sample_rows_with_attend_and_excite(engine, x0.clone(), c, batch, uc, record_losses=False)
    assert not hasattr(fast, "last_row_losses")
    r = _rel(z2, z)
    print(f"record_losses False vs True: latent rel_rms {r:.3e} (bound 1.5e-2), row updates {fast.aae_row_updates.tolist()} vs {rows}")
    assert r <= 1.5e-2


def test_predict_many_with_attend_and_excite_end_to_end(engine, env):
    """two one-image batches at 128 x 128 under image_seeds, fused into one sampling batch: finite, in range, in input order (each
    output is the nearer to its own image sampled alone), different from the run without attend-and-excite, and a second call
    bit-identical"""
    from udifftext_amd import config as C, synth
    cfgs = C.default_runtime_config(steps=10, batch_size=1, noise_iters=0)
    cfgs.aae_enabled = True
    mk = lambda: [synth.synthetic_batch(1, 128, 128, 4, seed=40 + i) for i in range(2)]
    seeds = [[900], [901]]
    sampler = env.pipeline.init_sampling(10, 5.0, env.dev)
    run = lambda cf, bs, sd, **kw: env.pipeline.predict_many(cf, engine, sampler, bs, env.dev, image_seeds=sd, **kw)
    got = run(cfgs, mk(), seeds, fuse=2)
    assert len(got) == 2
    for img, z in got:
        assert img.shape == (1, 3, 128, 128) and z.shape == (1, 4, 16, 16)
        assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(z).all()) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    again = run(cfgs, mk(), seeds, fuse=2)
    for (a, za), (b, zb) in zip(got, again):
        assert torch.equal(a, b) and torch.equal(za, zb), "a second identical call differs"
    alone = [run(cfgs, [mk()[i]], [seeds[i]], fuse=1)[0][1] for i in range(2)]
    for i in range(2):
        own, other = _rel(got[i][1], alone[i]), _rel(got[i][1], alone[1 - i])
        print(f"image {i}: latent vs itself alone {own:.3e}, vs the other image alone {other:.3e}")
        assert own < other
    plain_cfgs = C.default_runtime_config(steps=10, batch_size=1, noise_iters=0)
    plain = run(plain_cfgs, mk(), seeds, fuse=2, in_flight=1)
    for i in range(2):
        assert _rel(got[i][1], plain[i][1]) > 1e-3, "attend-and-excite changed nothing"
