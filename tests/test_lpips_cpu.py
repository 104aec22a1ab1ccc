"""LPIPS, host side (no GPU):

* the float64 restatement the GPU tests use (tests/lpips_ref.py) against a literal ``nn.Sequential`` spelling of torchvision's AlexNet
  ``features[0:12]`` (tap positions, state-dict indices), and its input stage against the numpy ``astype(np.uint8)`` path of the
  reference's test.py:94,102 followed by lpips.im2tensor, bit for bit;
* LPIPS(x, x) == 0 and symmetry of the restatement;
* the module's key table, its loader under both packages' names, its refusals (they fire before any launch: without a GPU a launch raises lib.UdtError);
* ``pipeline.lpips_of`` / ``pipeline.evaluate(lpips=...)`` on the stub engine of tests/test_evaluate_cpu.py with a stub LPIPS;
* the header declares the new entry points, ``lib.SYMBOLS`` types them, the footprint table covers them.
"""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

import udifftext_amd  # noqa: F401
import evaluate_standin as S
import lpips_ref as R
from test_evaluate_cpu import SEEDS, N_BATCHES, PER, _Model, _Sampler, _batch, _cfgs
from udifftext_amd import lib, pipeline
from udifftext_amd.lpips_alex import ALEX_CONVS, KEY_TABLE, LPIPS, map_sizes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def sd():
    return LPIPS().fill_synthetic_().state_dict()


def _frames(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3, H, W), generator=g), torch.rand((n, 3, H, W), generator=g) * 2.0 - 1.0


# ------------------------------------------------------------------------------------------------ the restatement
def test_features_equal_a_literal_alexnet(sd):
    net = nn.Sequential(
        nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(), nn.MaxPool2d(kernel_size=3, stride=2),
        nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(),
        nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(),
        nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU()).double()
    tv = {f"{idx}.{leaf}": sd[f"net.{sl}.{idx}.{leaf}"].double() for sl, idx, *_ in ALEX_CONVS for leaf in ("weight", "bias")}
    net.load_state_dict(tv, strict=True)                                  # the indices 0, 3, 6, 8, 10 are exactly the Sequential's convolutions
    x = torch.rand((2, 3, 67, 99), generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 4.0 - 2.0
    taps, f = [], x
    with torch.no_grad():
        for i, m in enumerate(net):
            f = m(f)
            if i in (1, 4, 7, 9, 11):                                     # after each ReLU: the ends of lpips' slice1 .. slice5
                taps.append(f)
    got = R.features(x, sd)
    assert [tuple(t.shape[1:]) for t in got] == [(64, 16, 24), (192, 7, 11), (384, 3, 5), (256, 3, 5), (256, 3, 5)]
    for a, b in zip(got, taps):
        assert a.dtype == torch.float64 and torch.allclose(a, b, rtol=1e-12, atol=1e-13)
        assert float(a.max()) > 0.0


def _edge_values():
    """[0, 1] samples on both sides of every integer boundary of s * 255, and the ends"""
    ks = torch.arange(0, 256, dtype=torch.float64)
    base = (ks / 255.0).float()
    vals = torch.cat((base, torch.nextafter(base, torch.tensor(2.0)), torch.nextafter(base, torch.tensor(-1.0)).clamp_min(0.0),
                      torch.tensor([0.0, 1.0, 0.5, 0.999999, 1e-7])))
    return vals.clamp(0.0, 1.0)


def test_input_stage_equals_the_saved_png_path_bit_for_bit():
    s = _edge_values()
    n = s.numel()
    pad = (-n) % 12
    s = torch.cat((s, torch.rand(pad + 24, generator=torch.Generator().manual_seed(1))))
    samples = s.reshape(1, 3, 4, -1).contiguous()
    x = (samples * 2.0 - 1.0)
    x.view(-1)[:4] = torch.tensor([-1.0, 1.0, 0.0, -0.9999999])
    images = x.clamp(-1.0, 1.0)
    # test.py:94 / :102 and :110-113, then lpips.load_image + lpips.im2tensor, then the scaling layer
    fake = (samples.numpy().transpose(0, 2, 3, 1) * 255).astype(np.uint8)
    real = (((images + 1.0) / 2.0).numpy().transpose(0, 2, 3, 1) * 255).astype(np.uint8)
    assert fake.min() == 0 and fake.max() == 255 and real.min() == 0 and real.max() == 255
    want = []
    for img in (fake[0], real[0]):
        t = torch.Tensor((img / (255.0 / 2.0) - 1.0)[:, :, :, np.newaxis].transpose((3, 2, 0, 1)))
        sh = torch.Tensor([-.030, -.088, -.188])[None, :, None, None]
        sc = torch.Tensor([.458, .448, .450])[None, :, None, None]
        want.append((t - sh) / sc)
    got = R.input_stage(samples, images, quantise=True)
    assert got.dtype == torch.float32 and got.shape == (2, 3, 4, samples.shape[-1])
    assert torch.equal(got.view(torch.int32), torch.cat(want, 0).view(torch.int32))
    cont = R.input_stage(samples, images, quantise=False)
    assert not torch.equal(cont, got) and float((cont - got).abs().max()) <= (1.0 / 127.5) / 0.448 * (1 + 1e-5)


def test_identity_is_zero_and_the_distance_is_symmetric(sd):
    sa, xb = _frames(2, 64, 96, 11)
    xa = sa * 2.0 - 1.0
    sb = (xb + 1.0) * 0.5
    assert torch.equal(R.lpips((xa + 1.0) * 0.5, xa, sd), torch.zeros(2, dtype=torch.float64))
    d_ab, d_ba = R.lpips((xa + 1.0) * 0.5, xb, sd), R.lpips(sb, xa, sd)
    assert float(d_ab.min()) > 0.0 and torch.allclose(d_ab, d_ba, rtol=1e-12, atol=0.0)
    d32 = R.lpips((xa + 1.0) * 0.5, xb, sd, dtype=torch.float32)
    assert d32.dtype == torch.float32 and torch.allclose(d32.double(), d_ab, rtol=1e-4)
    assert not torch.equal(R.lpips(sb, xa, sd, quantise=False), d_ba)


def test_layer_bound_is_finite_for_zero_pixels():
    f = torch.rand((4, 8, 2, 3), generator=torch.Generator().manual_seed(2))
    f[:, :, 0, 0] = 0.0                     # zero in both images of every pair
    f[0, :, 1, 1] = 0.0                     # zero in one image only
    d, b = R.layer(f, torch.rand(8, generator=torch.Generator().manual_seed(3)))
    assert bool(torch.isfinite(d).all()) and bool(torch.isfinite(b).all()) and bool((b > 0).all()) and bool((b < 1e-4 * d).all())


# ------------------------------------------------------------------------------------------------ the module, on the host
def test_key_table_and_the_two_packages_names(sd):
    assert set(KEY_TABLE) == set(LPIPS().state_dict()) == set(sd)
    assert KEY_TABLE["net.slice1.0.weight"] == ("features.0.weight",) and KEY_TABLE["net.slice5.10.bias"] == ("features.10.bias",)
    assert KEY_TABLE["lin3.model.1.weight"] == ("lins.3.model.1.weight",)
    assert [tuple(sd[f"lin{k}.model.1.weight"].shape) for k in range(5)] == [(1, c, 1, 1) for c in (64, 192, 384, 256, 256)]
    assert all(bool((sd[f"lin{k}.model.1.weight"] >= 0).all()) for k in range(5))
    assert tuple(sd["scaling_layer.shift"].shape) == (1, 3, 1, 1)
    # the published alex.pth (lin layers only) + a torchvision AlexNet checkpoint (features.N.*, with its classifier)
    lins = {k: v for k, v in sd.items() if k.startswith("lin")}
    alexnet = {alias[0]: sd[k] for k, alias in KEY_TABLE.items() if k.startswith("net.")}
    alexnet["classifier.1.weight"] = torch.zeros(4, 4)
    a, b = LPIPS(), LPIPS()
    a.load_weights(sd)
    b.load_weights(alexnet, lins)
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]) and torch.equal(v, sd[k]), k
    with pytest.raises(KeyError, match="lin0.model.1.weight"):
        LPIPS().load_weights(alexnet)
    with pytest.raises(ValueError, match="shape"):
        LPIPS().load_weights({**sd, "lin0.model.1.weight": torch.zeros(1, 63, 1, 1)})
    with pytest.raises(NotImplementedError):
        LPIPS(net="vgg")
    from sgm.util import instantiate_from_config
    assert isinstance(instantiate_from_config({"target": "udifftext_amd.lpips_alex.LPIPS", "params": {"net": "alex"}}), LPIPS)


def test_map_sizes_and_refusals():
    assert map_sizes(64, 96) == [(15, 23), (7, 11), (3, 5), (3, 5), (3, 5)]
    assert map_sizes(96, 64) == [(23, 15), (11, 7), (5, 3), (5, 3), (5, 3)]
    assert map_sizes(512, 512) == [(127, 127), (63, 63), (31, 31), (31, 31), (31, 31)]
    assert map_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    for hw in ((30, 64), (64, 30), (6, 6), (14, 200)):
        with pytest.raises(ValueError, match="too small"):
            map_sizes(*hw)
    m = LPIPS().fill_synthetic_()
    s, x = _frames(2, 64, 96, 3)
    # ValueError BEFORE any launch: without a GPU a launch would raise lib.UdtError instead
    with pytest.raises(ValueError, match="too small"):
        m(s[:, :, :30], x[:, :, :30])
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        m(s, x[:, :, :32])
    with pytest.raises(ValueError, match=r"\[N, 3, H, W\]"):
        m(s[:, :2], x[:, :2])
    if not torch.cuda.is_available():
        with pytest.raises(lib.UdtError):                                 # and no CPU fallback behind them
            m(s, x)


# ------------------------------------------------------------------------------------------------ lpips_of / evaluate with stubs
class _StubLPIPS:
    """a value that identifies the pair: mean |sample - (image + 1) / 2|; records the chunks it is handed"""

    def __init__(self):
        self.chunks = []

    def __call__(self, samples, images):
        assert samples.shape == images.shape
        self.chunks.append((int(samples.shape[0]), tuple(samples.shape[-2:])))
        return (samples - (images + 1.0) * 0.5).abs().mean(dim=(1, 2, 3))


def _pairs(sizes):
    outs, batches = [], []
    for k, (n, hw) in enumerate(sizes):
        s, x = _frames(n, *hw, seed=40 + k)
        outs.append((s, torch.zeros(n, 4, 1, 1)))
        batches.append({"image": x})
    return outs, batches


def test_lpips_of_order_and_chunks_over_two_image_sizes():
    sizes = [(2, (8, 8)), (3, (8, 8)), (2, (8, 12)), (1, (8, 12)), (2, (8, 8))]
    outs, batches = _pairs(sizes)
    want = [_StubLPIPS()(o[0], b["image"]).tolist() for o, b in zip(outs, batches)]
    for chunk, chunks in ((32, [(5, (8, 8)), (3, (8, 12)), (2, (8, 8))]),
                          (2, [(2, (8, 8)), (2, (8, 8)), (1, (8, 8)), (2, (8, 12)), (1, (8, 12)), (2, (8, 8))]),
                          (4, [(4, (8, 8)), (1, (8, 8)), (3, (8, 12)), (2, (8, 8))])):
        m = _StubLPIPS()
        got = pipeline.lpips_of(outs, batches, m, chunk=chunk)
        assert m.chunks == chunks, chunk
        assert [len(g) for g in got] == [n for n, _ in sizes]
        for g, w in zip(got, want):
            assert all(isinstance(v, float) for v in g) and np.allclose(g, w, rtol=1e-6, atol=0)
    assert pipeline.lpips_of([], [], _StubLPIPS()) == []
    with pytest.raises(ValueError, match="chunk"):
        pipeline.lpips_of(outs, batches, _StubLPIPS(), chunk=0)
    with pytest.raises(ValueError, match="differ in shape"):
        pipeline.lpips_of(outs[:1], [{"image": torch.zeros(2, 3, 8, 9)}], _StubLPIPS())
    with pytest.raises(ValueError, match="outputs for"):
        pipeline.lpips_of(outs, batches[:2], _StubLPIPS())


def test_evaluate_with_and_without_lpips():
    batches = lambda: [_batch(k) for k in range(N_BATCHES)]
    plain = pipeline.evaluate(_cfgs(), _Model(), _Sampler(), batches(), S.MeanReader(), CPU, in_flight=2, fuse=0, image_seeds=SEEDS,
                              return_samples=True)
    assert set(plain) == {"accuracy", "correct", "total", "pred", "label", "outputs"}
    assert set(pipeline.evaluate(_cfgs(), _Model(), _Sampler(), batches(), S.MeanReader(), CPU, image_seeds=SEEDS)) == {
        "accuracy", "correct", "total", "pred", "label"}
    m = _StubLPIPS()
    res = pipeline.evaluate(_cfgs(), _Model(), _Sampler(), batches(), S.MeanReader(), CPU, in_flight=2, fuse=0, image_seeds=SEEDS,
                            return_samples=True, lpips=m, lpips_chunk=4)
    assert set(res) == set(plain) | {"lpips", "lpips_sum", "lpips_per_image"}
    for key in ("accuracy", "correct", "total", "pred", "label"):
        assert res[key] == plain[key]
    for (a, za), (b, zb) in zip(res["outputs"], plain["outputs"]):
        assert torch.equal(a, b) and torch.equal(za, zb)
    assert m.chunks == [(4, (8, 8)), (4, (8, 8)), (2, (8, 8))]
    want = [_StubLPIPS()(o[0], b["image"]).tolist() for o, b in zip(plain["outputs"], batches())]
    assert [len(p) for p in res["lpips_per_image"]] == [PER] * N_BATCHES
    assert np.allclose(sum(res["lpips_per_image"], []), sum(want, []), rtol=1e-6, atol=0)
    assert len({round(v, 9) for v in sum(res["lpips_per_image"], [])}) == N_BATCHES * PER       # (the values do tell the pairs apart)
    assert res["lpips_sum"] == sum(sum(res["lpips_per_image"], [])) and res["total"] == N_BATCHES * PER
    assert math.isclose(res["lpips"], res["lpips_sum"] / res["total"], rel_tol=0, abs_tol=0)


def test_evaluate_refuses_lpips_inputs_before_any_sampling():
    sm, reader = _Sampler(), S.MeanReader()
    bad = _batch(1)
    del bad["image"]
    with pytest.raises(ValueError, match="batch 1 has no"):
        pipeline.evaluate(_cfgs(), _Model(), sm, [_batch(0), bad], reader, CPU, image_seeds=SEEDS[:2], lpips=_StubLPIPS())
    with pytest.raises(ValueError, match="too small"):                    # the real module's map sizes, on the host
        pipeline.evaluate(_cfgs(), _Model(), sm, [_batch(0)], reader, CPU, image_seeds=SEEDS[:1], lpips=LPIPS())
    with pytest.raises(ValueError, match="lpips_chunk"):
        pipeline.evaluate(_cfgs(), _Model(), sm, [_batch(0)], reader, CPU, image_seeds=SEEDS[:1], lpips=_StubLPIPS(), lpips_chunk=0)
    assert sm.n_calls == 0 and not reader.boxes and not reader.chunks


# ------------------------------------------------------------------------------------------------ the drop-in stays a drop-in
# the top-level names the reference's test.py, metrics.py and util.py import (test.py:1-16, metrics.py:1-3, util.py:1-4)
REFERENCE_IMPORTS = {"torch", "random", "numpy", "os", "PIL", "tqdm", "contextlib", "torchvision", "omegaconf", "pytorch_lightning",
                     "dataset", "util", "metrics", "lpips", "glob", "sgm"}


def test_no_module_of_the_package_shadows_an_import_of_the_reference():
    """``import udifftext_amd`` puts its directory first on sys.path (for the ``sgm`` mirror), so every top-level name in it is
    importable bare and wins over an installed package: none may equal a name the reference's drivers import — ``sgm``, the mirror
    that is meant to win, excepted.  (The module is lpips_alex.py, not lpips.py: metrics.py:1 does ``import lpips``.)"""
    import importlib.util
    pkg = os.path.dirname(os.path.abspath(udifftext_amd.__file__))
    assert pkg in __import__("sys").path
    own = {os.path.splitext(n)[0] for n in os.listdir(pkg)
           if n.endswith(".py") or os.path.isfile(os.path.join(pkg, n, "__init__.py"))} - {"__init__"}
    assert "lpips_alex" in own and "sgm" in own
    assert own & REFERENCE_IMPORTS == {"sgm"}, own & REFERENCE_IMPORTS
    spec = importlib.util.find_spec("lpips")                  # the caller's package or nothing, never a file of ours
    assert spec is None or not os.path.abspath(spec.origin or "").startswith(pkg + os.sep)


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_declares_types_and_covers_the_new_entry_points():
    import test_lpips_footprint_gpu  # noqa: F401  (appends its cases to the table)
    import test_footprint_gpu as table
    text = open(os.path.join(ROOT, "include", "udt_kernels.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    covered = {c for _, _, covers in table.CASES for c in covers}
    for name, n in (("udt_conv2d_f32", 16), ("udt_maxpool3s2_f32", 9), ("udt_lpips_input_f32", 11), ("udt_lpips_layer_f32", 11),
                    ("udt_lpips_layer_scratch_bytes", 2)):
        m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)", code)
        assert m and len(m.group(1).split(",")) == n == len(lib.SYMBOLS[name][1]), name
        assert name in covered and name not in table.EXEMPT, name
        assert lib.SYMBOLS[name][1][-1] == lib.C.c_void_p or name.endswith("scratch_bytes")          # the stream is the last argument
    layer_cases = [covers for _, _, covers in table.CASES if "udt_lpips_layer_f32" in covers]
    assert layer_cases and all("udt_lpips_layer_scratch_bytes" in c for c in layer_cases)
    assert hasattr(lib.load(), "udt_conv2d_f32")
    for word in ("Kp = K rounded up to a multiple of 16", "channels-last", "v_mfma_f32_32x32x2_f32"):
        assert word in text
