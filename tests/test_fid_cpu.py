"""FID, host side (no GPU):

* the float64 restatement the GPU tests use (tests/fid_ref.py): its block widths and the spatial chain 299 -> ... -> 8 against the
  issue's table and the module's own plan, its resize against F.interpolate in float64, its saved 8-bit values against numpy's
  ``astype(np.uint8)`` path of the reference's test.py:94,102;
* the module's key table (every tensor once; fc.*, AuxLogits.*, num_batches_tracked ignored), BatchNorm folding against the unfolded
  form in float64, its refusals (before any launch: without a GPU a launch raises lib.UdtError);
* ``frechet_distance``: identical statistics, diagonal covariances against the closed form, a rank-deficient pair, scipy's sqrtm where
  scipy exists;
* ``FIDStats``: merge of two halves equals one pass, n < 2 raises, the state round trip;
* ``pipeline.fid_of`` / ``pipeline.evaluate(fid=...)`` on the stub engine of tests/test_evaluate_cpu.py with stub statistics;
* the header declares the new entry points, ``lib.SYMBOLS`` types them, the footprint table covers them; no top-level name of the
  package shadows an import of the reference.
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import udifftext_amd  # noqa: F401
import evaluate_standin as S
import fid_ref as R
from test_evaluate_cpu import SEEDS, N_BATCHES, PER, _Model, _Sampler, _batch, _cfgs
from udifftext_amd import lib, pipeline
from udifftext_amd import fid_inception as M
from udifftext_amd.fid_inception import FID, FIDStats, KEY_TABLE, frechet_distance

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sd():
    return FID().fill_synthetic_().state_dict()


def _rand(shape, seed, scale=1.0):
    return torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


# ------------------------------------------------------------------------------------------------ the restatement
def test_block_widths_of_the_restatement_and_of_the_plan(sd):
    assert list(R.BLOCKS) == list(M.BLOCKS) == list(R.BLOCK_WIDTHS)
    for name, fn in R.BLOCKS.items():
        cin, branches = M.BLOCKS[name]
        launches, c_out, c_tmp, stride = M.block_plan(cin, branches)
        y = fn(_rand((1, cin, 3, 3), 3).abs(), sd)
        assert y.shape == (1, R.BLOCK_WIDTHS[name], *((1, 1) if stride == 2 else (3, 3))), name
        assert c_out == R.BLOCK_WIDTHS[name] and float(y.max()) > 0.0
        # every channel of the concatenation and of the scratch map is written exactly once
        for buf, width in (("out", c_out), ("tmp", c_tmp)):
            spans = sorted((d0, d1) for _, _, (b, d0, d1) in launches if b == buf)
            assert [s[0] for s in spans] == [0] + [s[1] for s in spans[:-1]] and (spans[-1][1] if spans else 0) == width, (name, buf)
    widths = [R.BLOCK_WIDTHS[n] for n in R.BLOCKS]
    assert [M.BLOCKS[n][0] for n in R.BLOCKS] == [192] + widths[:-1]        # each block reads what the one before it wrote


def test_spatial_chain_299_to_8(sd):
    sizes = []
    x = R.stem(_rand((1, 3, 299, 299), 4), sd, sizes)
    assert x.shape == (1, 192, 35, 35)
    x6 = R.BLOCKS["Mixed_6a"](_rand((1, 288, 35, 35), 5).abs(), sd)
    x7 = R.BLOCKS["Mixed_7a"](_rand((1, 768, 17, 17), 6).abs(), sd)
    assert tuple(sizes + [x6.shape[-1], x7.shape[-1]]) == R.SPATIAL_CHAIN[1:]
    want = [(s, s) for s in (149, 147, 147, 73, 73, 71, 35, 35, 17, 17, 8, 8)]
    assert M.map_sizes() == M.map_sizes(299, 299) == want
    with pytest.raises(ValueError, match="too small"):
        M.map_sizes(74, 299)


def test_resize_equals_interpolate_in_float64():
    for h, w in ((8, 8), (5, 13), (512, 384), (300, 299), (1, 1), (299, 299), (600, 2)):
        p = torch.rand((2, 3, h, w), generator=torch.Generator().manual_seed(h * w), dtype=torch.float64)
        want = F.interpolate(p, size=(299, 299), mode="bilinear", align_corners=False)
        got = R.resize(p)
        # F.interpolate forms the coordinate (i + 0.5) (in / out) - 0.5 in floating point: up to 4 roundings at magnitude <= in, which
        # move a weight by as much; the restatement's rational coordinate is exact
        assert got.shape == want.shape and float((got - want).abs().max()) <= 4 * max(h, w) * 2.0 ** -52 + 4e-16, (h, w)
    assert torch.equal(R.resize(p := torch.rand((1, 1, 299, 299), dtype=torch.float64)), p)        # the same size: the identity


def test_saved_values_equal_the_uint8_path_and_exact_levels_quantise_to_themselves():
    ks = torch.arange(0, 256, dtype=torch.float64)
    s = torch.cat(((ks / 255.0).float(), torch.rand(3 * 4 * 100 - 256, generator=torch.Generator().manual_seed(1)))).reshape(1, 3, 4, 100)
    x = (s * 2.0 - 1.0).clamp(-1.0, 1.0)
    fake = (s.numpy().transpose(0, 2, 3, 1) * 255).astype(np.uint8)
    real = (((x + 1.0) / 2.0).numpy().transpose(0, 2, 3, 1) * 255).astype(np.uint8)
    v = R.saved_values(s, x)
    assert v.dtype == torch.float32 and v.shape == (2, 3, 4, 100)
    assert np.array_equal(v[0].numpy().transpose(1, 2, 0), fake[0].astype(np.float32))
    assert np.array_equal(v[1].numpy().transpose(1, 2, 0), real[0].astype(np.float32))
    assert torch.equal(v[0].reshape(-1)[:256], ks.float())                 # a frame value exactly on k/255 quantises to k
    cont = R.saved_values(s, x, quantise=False)
    assert not torch.equal(cont, v) and float((cont - v).max()) < 1.0 and float((cont - v).min()) >= 0.0
    out, bound = R.input_stage(s, x)
    assert out.shape == (2, 3, 299, 299) and float(out.min()) >= -1.0 and float(out.max()) <= 1.0
    assert float(bound.max()) <= 17 * R.U * R.SLACK and float(bound.min()) > 0.0


# ------------------------------------------------------------------------------------------------ the module, on the host
def test_key_table_covers_every_tensor_once_and_ignores_the_classifier(sd):
    convs = M.all_convs()
    assert len(convs) == 94 and len({p for p, _ in convs}) == 94
    assert set(KEY_TABLE) == set(FID().state_dict()) == set(sd) and len(KEY_TABLE) == 94 * 5 and FID.KEY_TABLE is KEY_TABLE
    names = {n for k, aliases in KEY_TABLE.items() for n in (k, *aliases)}
    assert len(names) == sum(1 + len(a) for a in KEY_TABLE.values())       # no name stands for two tensors
    for k in ("Conv2d_1a_3x3.conv.weight", "Mixed_5b.branch5x5_2.bn.running_var", "Mixed_6e.branch7x7dbl_5.bn.weight",
              "Mixed_7a.branch7x7x3_4.bn.bias", "Mixed_7c.branch3x3dbl_3b.bn.running_mean"):
        assert k in KEY_TABLE
    assert tuple(sd["Mixed_6b.branch7x7_2.conv.weight"].shape) == (128, 128, 1, 7)
    assert tuple(sd["Mixed_6b.branch7x7_3.conv.weight"].shape) == (192, 128, 7, 1)
    assert tuple(sd["Mixed_7b.branch3x3_2b.conv.weight"].shape) == (384, 384, 3, 1)
    assert all(float(v.min()) >= 0.5 for k, v in sd.items() if k.endswith("running_var"))
    # a torchvision-style checkpoint: the classifier, the auxiliary head and the BatchNorm counters are ignored
    tv = dict(sd)
    tv.update({"fc.weight": torch.zeros(4, 4), "fc.bias": torch.zeros(4), "AuxLogits.conv0.conv.weight": torch.zeros(2, 2, 1, 1),
               "Mixed_5b.branch1x1.bn.num_batches_tracked": torch.tensor(7)})
    a = FID()
    a.load_weights(tv)
    for k, v in a.state_dict().items():
        assert torch.equal(v, sd[k]), k
    short = dict(sd)
    del short["Mixed_7c.branch_pool.bn.running_var"]
    with pytest.raises(KeyError, match="Mixed_7c.branch_pool.bn.running_var"):
        FID().load_weights(short)
    with pytest.raises(ValueError, match="shape"):
        FID().load_weights({**sd, "Conv2d_1a_3x3.conv.weight": torch.zeros(32, 3, 3, 2)})
    with pytest.raises(ValueError, match="does not know"):
        FID().load_weights({**sd, "Mixed_8a.branch1x1.conv.weight": torch.zeros(1)})
    from sgm.util import instantiate_from_config
    assert isinstance(instantiate_from_config({"target": "udifftext_amd.fid_inception.FID"}), FID)


def test_bn_folding_equals_the_unfolded_form_in_float64(sd):
    for prefix, op in (("Conv2d_1a_3x3", None), ("Mixed_6b.branch7x7_2", None), ("Mixed_7c.branch3x3dbl_3b", None)):
        op = dict(M.all_convs())[prefix]
        x = _rand((2, op.cin, 9, 9), 11)
        want = R.basic(x, sd, prefix, stride=op.stride, padding=op.pad)
        w, b = M.fold_bn(*(sd[f"{prefix}.{k}"] for k in ("conv.weight", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")))
        assert w.dtype == b.dtype == torch.float64
        got = F.relu(F.conv2d(x, w, b, stride=op.stride, padding=op.pad))
        assert float(want.max()) > 0 and torch.allclose(got, want, rtol=1e-12, atol=1e-14), prefix
    # eps is 1e-3, not nn.BatchNorm2d's default 1e-5
    one = torch.ones(1)
    w, b = M.fold_bn(torch.ones(1, 1, 1, 1), 2 * one, 3 * one, 5 * one, 0 * one)
    assert abs(float(w) - 2.0 / 1e-3 ** 0.5) < 1e-9 and abs(float(b) - (3.0 - 5.0 * 2.0 / 1e-3 ** 0.5)) < 1e-9


def test_refusals_fire_before_any_launch():
    m = FID()
    s = torch.rand(2, 3, 8, 8)
    for bad in ((s, s[:, :, :4]), (s[:, :2], s[:, :2]), s[0], (s[:0], s[:0])):
        with pytest.raises(ValueError, match=r"\[N >= 1, 3, H, W\]"):
            m.features(bad)
    with pytest.raises(ValueError, match="needs the FID module"):
        FIDStats().update(s, s)
    with pytest.raises(ValueError, match="are not"):
        FIDStats(dim=8).update_features(torch.zeros(3, 8))
    if not torch.cuda.is_available():
        with pytest.raises(lib.UdtError):                                  # and no CPU fallback behind them
            m.features((s, s * 2 - 1))


# ------------------------------------------------------------------------------------------------ the distance
def _cov_pair(n, D, seed):
    a, b = _rand((n, D), seed).numpy(), (_rand((n, D), seed + 1) * 1.3 + 0.2).numpy()
    return (a.mean(0), np.cov(a, rowvar=False)), (b.mean(0), np.cov(b, rowvar=False))


def test_frechet_of_identical_statistics_is_zero_within_the_eigh_bound():
    for n, D in ((200, 32), (8, 32), (500, 64)):
        (mu, s), _ = _cov_pair(n, D, 21)
        got = frechet_distance(mu, s, mu, s)
        bound = R.frechet_zero_bound(s)
        print(f"FID(S, S), n {n}, D {D}: {got:.3e}, bound {bound:.3e}")
        assert abs(got) <= bound < 1e-3 * np.trace(s)


def test_frechet_of_diagonal_covariances_is_the_closed_form():
    g = np.random.default_rng(5)
    a, b = g.uniform(0.1, 4.0, 32), g.uniform(0.1, 4.0, 32)
    b[:3] = 0.0                                                              # a singular one as well
    mu1, mu2 = g.normal(size=32), g.normal(size=32)
    want = ((mu1 - mu2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    got = frechet_distance(mu1, np.diag(a), mu2, np.diag(b))
    assert abs(got - want) <= 1e-12 * want
    assert abs(frechet_distance(mu2, np.diag(b), mu1, np.diag(a)) - want) <= 1e-12 * want          # symmetric in its two sets
    assert abs(got - R.frechet(mu1, np.diag(a), mu2, np.diag(b))) <= 1e-12 * want
    with pytest.raises(ValueError, match="do not fit"):
        frechet_distance(mu1, np.diag(a), mu2[:5], np.diag(b))


def test_frechet_of_a_rank_deficient_pair_is_finite_and_not_negative():
    (mu1, s1), (mu2, s2) = _cov_pair(8, 32, 31)
    assert np.linalg.matrix_rank(s1) == 7
    got = frechet_distance(mu1, s1, mu2, s2)
    assert np.isfinite(got) and got > 0.0
    assert abs(got - R.frechet(mu1, s1, mu2, s2)) <= 1e-9 * got


def test_frechet_against_scipy_sqrtm_on_a_well_conditioned_pair():
    linalg = pytest.importorskip("scipy.linalg")
    (mu1, s1), (mu2, s2) = _cov_pair(400, 24, 41)
    covmean = linalg.sqrtm(s1.dot(s2))
    covmean = covmean[0] if isinstance(covmean, tuple) else covmean
    want = float(((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2.0 * np.trace(np.real(covmean)))
    assert abs(frechet_distance(mu1, s1, mu2, s2) - want) <= 1e-8 * want


# ------------------------------------------------------------------------------------------------ the statistics
def _state(f_fake, f_real):
    return {"n": f_fake.shape[0], "sum": torch.stack((f_fake.sum(0), f_real.sum(0))), "outer": torch.stack((f_fake.t() @ f_fake, f_real.t() @ f_real))}


def test_stats_merge_of_two_halves_equals_one_pass_and_n_below_two_raises():
    fa, fb = _rand((40, 16), 51), _rand((40, 16), 52) * 0.7 + 0.1         # (full rank: the square roots are well conditioned)
    whole = FIDStats.from_state(_state(fa, fb))
    halves = FIDStats.from_state(_state(fa[:17], fb[:17])).merge(FIDStats.from_state(_state(fa[17:], fb[17:])))
    assert halves.n == whole.n == 40 and halves.dim == 16
    assert torch.allclose(halves.sum, whole.sum, rtol=1e-14, atol=1e-14) and torch.allclose(halves.outer, whole.outer, rtol=1e-14, atol=1e-14)
    (mu1, s1), (mu2, s2) = whole.moments()
    assert np.allclose(mu1, fa.numpy().mean(0), rtol=1e-13) and np.allclose(s2, np.cov(fb.numpy(), rowvar=False), rtol=1e-11, atol=1e-13)
    want = R.frechet(*R.statistics(fa), *R.statistics(fb))
    assert abs(whole.compute() - want) <= 1e-9 * want and abs(halves.compute() - want) <= 1e-9 * want
    back = FIDStats.from_state(whole.state())
    assert back.n == 40 and torch.equal(back.sum, whole.sum) and torch.equal(back.outer, whole.outer)
    st = whole.state()
    assert st["sum"].dtype == st["outer"].dtype == torch.float64 and st["sum"].device.type == "cpu" and st["outer"].shape == (2, 16, 16)
    for n in (0, 1):
        with pytest.raises(ValueError, match="at least 2 images"):
            FIDStats.from_state(_state(fa[:n], fb[:n])).compute()
    with pytest.raises(ValueError, match="features against"):
        whole.merge(FIDStats(dim=8))
    with pytest.raises(ValueError, match="from_state"):
        FIDStats.from_state({"n": 2, "sum": torch.zeros(2, 4), "outer": torch.zeros(2, 4, 4)})


# ------------------------------------------------------------------------------------------------ fid_of / evaluate with stubs
class _StubStats(FIDStats):
    """features that identify the frame: the 3 channel means and the 3 channel means of the squares, added on the host"""

    def __init__(self, chunks, repeat=1):
        super().__init__(None, dim=6 * repeat)
        self.chunks, self.repeat = chunks, repeat

    def update(self, samples, images, quantise=True):
        self.chunks.append((int(samples.shape[0]), tuple(samples.shape[-2:])))
        for k, x in enumerate((samples, (images + 1.0) * 0.5)):
            f = torch.cat((x.double().mean((2, 3)), x.double().pow(2).mean((2, 3))), 1).repeat(1, self.repeat)
            self.sum[k] += f.sum(0)
            self.outer[k] += f.t() @ f
        self.n += samples.shape[0]
        return self


class _StubFID:
    def __init__(self, repeat=1):
        self.chunks, self.repeat = [], repeat

    def stats(self):
        return _StubStats(self.chunks, self.repeat)


def test_evaluate_with_and_without_fid():
    batches = lambda: [_batch(k) for k in range(N_BATCHES)]
    run = lambda **kw: pipeline.evaluate(_cfgs(), _Model(), _Sampler(), batches(), S.MeanReader(), CPU, in_flight=2, fuse=0,
                                         image_seeds=SEEDS, return_samples=True, **kw)
    plain = run()
    assert set(plain) == {"accuracy", "correct", "total", "pred", "label", "outputs"}                 # the parent's keys
    assert set(pipeline.evaluate(_cfgs(), _Model(), _Sampler(), batches(), S.MeanReader(), CPU, image_seeds=SEEDS)) == {
        "accuracy", "correct", "total", "pred", "label"}
    m = _StubFID()
    res = run(fid=m, fid_chunk=4)
    assert set(res) == set(plain) | {"fid", "fid_stats"}                     # (10 images for 6 features: no note)
    for key in ("accuracy", "correct", "total", "pred", "label"):
        assert res[key] == plain[key]
    for (a, za), (b, zb) in zip(res["outputs"], plain["outputs"]):
        assert torch.equal(a, b) and torch.equal(za, zb)
    total = N_BATCHES * PER
    assert sum(n for n, _ in m.chunks) == total and max(n for n, _ in m.chunks) <= 4
    assert res["fid_stats"]["n"] == total
    wide = run(fid=_StubFID(repeat=2))                                       # 10 images for 12 features: the note pytorch_fid's warning is
    assert "rank-deficient" in wide["fid_note"] and isinstance(wide["fid"], float) and wide["fid_stats"]["sum"].shape == (2, 12)
    fake = torch.cat([o[0] for o in plain["outputs"]])
    real = torch.cat([(b["image"] + 1.0) * 0.5 for b in batches()])
    feats = [torch.cat((x.double().mean((2, 3)), x.double().pow(2).mean((2, 3))), 1) for x in (fake, real)]
    want = R.frechet(*R.statistics(feats[0]), *R.statistics(feats[1]))
    assert isinstance(res["fid"], float) and abs(res["fid"] - want) <= 1e-9 * abs(want) + 1e-12
    assert abs(FIDStats.from_state(res["fid_stats"]).compute() - res["fid"]) == 0.0
    # with the second measurement as well
    both = run(fid=_StubFID(), lpips=lambda s, x: (s - (x + 1.0) * 0.5).abs().mean((1, 2, 3)))
    assert set(both) == set(res) | {"lpips", "lpips_sum", "lpips_per_image"} 
    assert abs(both["fid"] - res["fid"]) <= 1e-12 * res["fid"]              # (chunks of 32 here, of 4 there: another order of the fp64 sums)
    # one image: no covariance
    one = _batch(0)
    one = {k: (v[:1] if isinstance(v, (torch.Tensor, list)) else v) for k, v in one.items()}
    from udifftext_amd import config as C
    single = pipeline.evaluate(C.default_runtime_config(steps=2, batch_size=1, noise_iters=0), _Model(), _Sampler(), [one], S.MeanReader(), CPU, image_seeds=[SEEDS[0][:1]], fid=_StubFID())
    assert single["total"] == 1 and single["fid"] is None and "at least 2 images" in single["fid_note"] and single["fid_stats"]["n"] == 1
    with pytest.raises(ValueError, match="fid_chunk"):
        run(fid=_StubFID(), fid_chunk=0)


# ------------------------------------------------------------------------------------------------ the drop-in stays a drop-in
# the top-level names the reference's test.py, metrics.py and util.py import, and the packages FID is usually taken from
REFERENCE_IMPORTS = {"torch", "random", "numpy", "os", "PIL", "tqdm", "contextlib", "torchvision", "omegaconf", "pytorch_lightning",
                     "dataset", "util", "metrics", "lpips", "glob", "sgm", "pytorch_fid", "fid", "scipy"}


def test_no_module_of_the_package_shadows_an_import_of_the_reference():
    pkg = os.path.dirname(os.path.abspath(udifftext_amd.__file__))
    own = {os.path.splitext(n)[0] for n in os.listdir(pkg)
           if n.endswith(".py") or os.path.isfile(os.path.join(pkg, n, "__init__.py"))} - {"__init__"}
    assert "fid_inception" in own and "sgm" in own
    assert own & REFERENCE_IMPORTS == {"sgm"}, own & REFERENCE_IMPORTS


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_declares_types_and_covers_the_new_entry_points():
    import test_fid_footprint_gpu  # noqa: F401  (appends its cases to the table)
    import test_footprint_gpu as table
    text = open(os.path.join(ROOT, "include", "udt_kernels.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    covered = {c for _, _, covers in table.CASES for c in covers}
    for name, n in (("udt_conv2d_rect_f32", 18), ("udt_pool3_f32", 12), ("udt_fid_input_f32", 10), ("udt_mean_pixels_f32", 8),
                    ("udt_moments_accum_f64", 7)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m and len(m.group(1).split(",")) == n == len(lib.SYMBOLS[name][1]), name
        assert name in covered and name not in table.EXEMPT, name
        assert lib.SYMBOLS[name][1][-1] == lib.C.c_void_p                                          # the stream is the last argument
    assert hasattr(lib.load(), "udt_moments_accum_f64")
    assert lib.SYMBOLS["udt_conv2d_f32"][1] == [lib._fp] * 4 + [lib._i32] * 11 + [lib._vp]          # the square entry point keeps its signature
    for word in ("v_mfma_f64_16x16x4_f64", "count_include_pad=False", "kh x kw"):
        assert word in text
