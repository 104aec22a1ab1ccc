"""The row-wise attend-and-excite loop without a GPU: the restated update rule (tests/aae_rows_ref.py) against the real reference's B = 1
loop (tests/golden/aae_rows_golden.npz, tests/golden/make_aae_rows_golden.py), the host logic of pipeline.predict_many with
cfgs.aae_enabled on a stub engine, and the registration of udt_aae_row_update_f32."""
import os
import re

import numpy as np
import pytest
import torch

import aae_rows_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "aae_rows_golden.npz"))


def test_golden_covers_the_stated_counts(gold):
    counts, group = gold["counts"], gold["group"]
    g0 = sorted(int(c) for c, g in zip(counts, group) if g == 0)
    assert gold["x0"].shape[0] >= 5 and gold["x0"].shape[1:] == (4, 8, 8)
    assert g0[0] == 1 and g0[-1] == int(gold["group_max_iter"][0]) + 1 == 21 and len({g0[1], g0[2]} - {1, 21}) == 2
    assert int(gold["group_max_iter"][1]) == 2 and 3 in [int(c) for c, g in zip(counts, group) if g == 1]
    assert not bool(gold["group_iter_enabled"][2]) and all(int(c) == 1 for c, g in zip(counts, group) if g == 2)
    for s in range(counts.shape[0]):                          # the generator's margin: no fp32 reordering flips a count
        if gold["group_iter_enabled"][group[s]]:
            thres = float(gold["group_thres"][group[s]])
            ll = gold["losses"][s, :counts[s]]
            assert not np.isnan(ll).any() and np.isnan(gold["losses"][s, counts[s]:]).all()
            assert (np.abs(ll - thres) >= 1e-3 * max(abs(thres), 1.0) * (1 - 1e-6)).all()


def test_row_rule_reproduces_the_reference_loop_of_every_sample_in_one_batch(gold):
    """all samples of a group stacked into ONE batch and driven by the restated rule: every row ends with the reference's count — rows
    that freeze early are not disturbed by the ones that run on, the ones that run on not stopped by the early ones — its losses at
    every iteration within 1e-4 of the golden's margin, and its x_final within ``aae_rows_ref.displacement_bound`` (one fma per
    update; derived there)."""
    alpha = float(gold["alpha"][0])
    for g in range(gold["group_thres"].shape[0]):
        rows = np.nonzero(gold["group"] == g)[0]
        x0, w, t = (torch.from_numpy(gold[k][rows]) for k in ("x0", "toy_w", "toy_t"))
        c = torch.from_numpy(gold["toy_c"][rows])
        thres, max_iter, en = float(gold["group_thres"][g]), int(gold["group_max_iter"][g]), bool(gold["group_iter_enabled"][g])
        xf, counts, evals, losses = R.row_loop(x0, lambda x: R.toy_loss_grad(x, w, t, c), alpha, thres, en, max_iter)
        assert counts.tolist() == gold["counts"][rows].tolist(), (g, counts.tolist(), gold["counts"][rows].tolist())
        assert evals == int(gold["counts"][rows].max())
        g0 = R.toy_loss_grad(x0, w, t, c)[1]
        for r, s in enumerate(rows):
            k = int(gold["counts"][s])
            ref = torch.from_numpy(gold["x_final"][s])
            bound = R.displacement_bound(k, alpha, x0[r], ref, g0[r])
            err = float((xf[r] - ref).abs().max())
            print(f"group {g} sample {s}: {k} updates, max |x_final - reference| {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (g, s, err, bound)
            got_l = np.array([float(l[r]) for l in losses[:k]])
            assert np.abs(got_l - gold["losses"][s, :k]).max() <= 1e-4          # (a tenth of the golden's margin)


def test_row_rule_edges():
    """the rule's corners on hand-made states: NaN loss runs to the cap, frozen rows ignore NaN inputs, counts at the cap, an active
    flag of 7, iter_enabled off"""
    nan = float("nan")
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    grad = torch.ones((3, 4))
    grad[1] = nan
    loss = torch.tensor([nan, nan, -1.0])
    state = torch.tensor([[7, 0, 1], [19, 4, 20]], dtype=torch.int32)
    xn, so, na = R.row_update(x, grad, loss, state, 0.5, -0.5, True, 20)
    assert torch.equal(xn[0], x[0] - 0.5) and torch.equal(xn[1], x[1]) and torch.equal(xn[2], x[2] - 0.5)
    assert so.tolist() == [[1, 0, 0], [20, 4, 21]] and na == 1                 # row 0: it = max_iter, NaN loss: stays; row 2: loss <= thres
    _, so, na = R.row_update(x, grad, loss, torch.tensor([[1, 0, 1], [20, 4, 3]], dtype=torch.int32), 0.5, -2.0, True, 20)
    assert so.tolist() == [[0, 0, 1], [21, 4, 4]] and na == 1                  # row 0: it = max_iter + 1: out
    _, so, na = R.row_update(x, grad, loss, torch.tensor([[1, 0, 1], [0, 0, 0]], dtype=torch.int32), 0.5, -2.0, False, 20)
    assert so.tolist() == [[0, 0, 0], [1, 0, 1]] and na == 0


# ------------------------------------------------------------------------------------------------ predict_many, host logic
class _StubConditioner:
    def get_unconditional_conditioning(self, batch, batch_uc=None, force_uc_zero_embeddings=None):
        from udifftext_amd import rng
        B = batch["image"].shape[0]
        feat = batch["image"].mean(dim=(1, 2, 3)).reshape(B, 1, 1, 1)
        return {"concat": rng.randn((B, 4, 2, 2)) + feat}, {"concat": rng.randn((B, 4, 2, 2)) + feat}


class _StubModel:
    conditioner = _StubConditioner()

    def parameters(self):
        return iter([torch.zeros(1)])

    def decode_first_stage(self, z):
        return z[:, :3].repeat_interleave(2, -1).repeat_interleave(2, -2) * 0.1


class _StubSampler:
    """the stub sampler of tests/test_parallel_cpu.py with the rows method; records what it is called with"""
    uses_churn = False

    def __init__(self):
        self.calls, self.draws = [], []

    def get_init_noise(self, cfgs, model, cond, batch, uc=None):
        from udifftext_amd import rng
        self.draws.append("init")
        return rng.randn((cfgs.batch_size, 4, 2, 2))

    def draw_step_noise(self, shape, device, num_steps=None, init_step=0):
        from udifftext_amd import rng
        self.draws.append("step")
        return rng.randn((2,) + tuple(shape))

    def _combine(self, x, cond, uc, noise):
        return x + 0.5 * cond["concat"] - 0.25 * uc["concat"] + 0.125 * noise.sum(0)

    def sample_rows_with_attend_and_excite(self, model, x, cond, batch, uc, num_steps=None, init_step=0, noise=None, record_losses=True):
        self.calls.append((x.shape[0], batch["mask"].clone(), batch["seg_mask"].clone(), record_losses))
        return self._combine(x, cond, uc, noise) + batch["mask"].mean(dim=(1, 2, 3)).reshape(-1, 1, 1, 1)

    def __call__(self, model, x, cond, batch=None, uc=None, init_step=0, aae_enabled=False, detailed=False):
        assert aae_enabled
        noise = self.draw_step_noise(x.shape, x.device, None, init_step)
        return self._combine(x, cond, uc, noise) + batch["mask"].mean(dim=(1, 2, 3)).reshape(-1, 1, 1, 1)


def _batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    return {"image": torch.rand((n, 3, 8, 8), generator=g), "mask": torch.rand((n, 1, 8, 8), generator=g),
            "seg_mask": torch.rand((n, 12), generator=g), "label": [f"img{i}" for i in range(n)], "txt": [f"t{i}" for i in range(n)]}


def _cfgs(**kw):
    from udifftext_amd import config as C
    cfgs = C.default_runtime_config(steps=2, batch_size=2, noise_iters=0)
    cfgs.aae_enabled = True
    for k, v in kw.items():
        setattr(cfgs, k, v)
    return cfgs


@pytest.mark.parametrize("n_batches,in_flight,fuse,units", [(5, 3, 2, [2, 2, 1]), (3, 2, 1, [1, 1, 1]), (4, 1, 0, [4])])
def test_predict_many_aae_runs_units_in_sequence_with_concatenated_masks(n_batches, in_flight, fuse, units):
    """cfgs.aae_enabled: the units are formed as without it and handed to sample_rows_with_attend_and_excite one after the other, the
    fused batch holding mask / seg_mask concatenated over the unit; outputs in input order; and every draw — conditioning, initial
    noise, step noise, batch by batch — equals ``predict`` batch by batch from the same generator state"""
    from udifftext_amd import pipeline
    sm = _StubSampler()
    torch.manual_seed(7)
    outs = pipeline.predict_many(_cfgs(), _StubModel(), sm, [_batch(2, 100 + i) for i in range(n_batches)], torch.device("cpu"),
                                 in_flight=in_flight, fuse=fuse, record_losses=False)
    assert [c[0] for c in sm.calls] == [2 * u for u in units] and len(outs) == n_batches
    assert all(c[3] is False for c in sm.calls)
    assert sm.draws == ["init", "step"] * n_batches
    i = 0
    for (nb, mask, seg, _), u in zip(sm.calls, units):
        ref = [_batch(2, 100 + j) for j in range(i, i + u)]
        assert torch.equal(mask, torch.cat([b["mask"] for b in ref])) and torch.equal(seg, torch.cat([b["seg_mask"] for b in ref]))
        i += u
    sp = _StubSampler()
    torch.manual_seed(7)
    for i in range(n_batches):
        img, z = pipeline.predict(_cfgs(), _StubModel(), sp, _batch(2, 100 + i), torch.device("cpu"))
        assert torch.equal(outs[i][0], img) and torch.equal(outs[i][1], z), i


def test_predict_many_aae_image_seeds_are_batching_independent():
    from udifftext_amd import pipeline
    seeds = [[11, 12], [13, 14], [15, 16]]
    run = lambda fuse: pipeline.predict_many(_cfgs(), _StubModel(), _StubSampler(), [_batch(2, 200 + i) for i in range(3)],
                                             torch.device("cpu"), in_flight=1, fuse=fuse, image_seeds=seeds)
    for (a, za), (b, zb) in zip(run(1), run(3)):
        assert torch.equal(a, b) and torch.equal(za, zb)


def test_predict_many_aae_refusals():
    from udifftext_amd import pipeline
    with pytest.raises(NotImplementedError, match="detailed"):
        pipeline.predict_many(_cfgs(detailed=True), _StubModel(), _StubSampler(), [_batch(2, 1)], torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="detailed"):
        pipeline.predict_many(_cfgs(detailed=True, aae_enabled=False), _StubModel(), _StubSampler(), [_batch(2, 1)], torch.device("cpu"))

    class NoRows:
        get_init_noise = _StubSampler.get_init_noise

    with pytest.raises(NotImplementedError, match="attend-and-excite"):
        pipeline.predict_many(_cfgs(), _StubModel(), NoRows(), [_batch(2, 1)], torch.device("cpu"))


# ------------------------------------------------------------------------------------------------ registration
def test_aae_row_update_is_declared_typed_and_in_the_footprint_table():
    import test_aae_rows_footprint_gpu  # noqa: F401  (appends its cases to the table)
    import test_footprint_gpu as table
    from udifftext_amd import lib
    root = os.path.dirname(HERE)
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "udt_kernels.h")).read(), flags=re.S)
    m = re.search(r"int\s+udt_aae_row_update_f32\s*\(([^)]*)\)", code)
    assert m, "udt_aae_row_update_f32 is not declared in include/udt_kernels.h"
    assert len(m.group(1).split(",")) == 13 == len(lib.SYMBOLS["udt_aae_row_update_f32"][1])
    covering = [name for name, _, covers in table.CASES if "udt_aae_row_update_f32" in covers]
    assert len(covering) >= 2 and "udt_aae_row_update_f32" not in table.EXEMPT
    from udifftext_amd import ops
    assert callable(ops.aae_row_update_)
