"""pipeline.evaluate and the box-based entry points of ParseqPredictor on the GPU.

PARSeq on synthetic weights has near-tied logits (tests/test_parseq_gpu.py), so nothing here compares OCR strings between two
different computations: the predictor is checked for its interface and for determinism, the plumbing with a stand-in reader whose
text is a fixed function of the resampled crop's mean (tests/evaluate_standin.py), the numerics of the resampling against the float64
restatement at the kernel's bound (tests/crop_resize_ref.py)."""
import os

import numpy as np
import pytest
import torch

import crop_resize_ref as R
import evaluate_standin as S

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "parseq_golden.npz"))
H, W, STEPS = 64, 128, 2
SEEDS = [[31, 32], [33, 34]]


@pytest.fixture(scope="module")
def predictor(cuda):
    """synthetic PARSeq weights, as tests/test_parseq_gpu.py builds them"""
    import udifftext_amd  # noqa: F401
    from sgm.modules.predictors.model import ParseqPredictor
    from sgm.util import skip_param_init
    from udifftext_amd import synth
    keys, shapes = list(G["state_dict_keys"]), [eval(s) for s in G["state_dict_shapes"]]
    sd = {k: synth.synthetic_tensor("parseq." + k, sh) for k, sh in zip(keys, shapes)}
    with skip_param_init():
        m = ParseqPredictor(ckpt_path=None)
    missing, unexpected = m.parseq.load_state_dict(sd, strict=True)
    assert not missing and not unexpected
    torch.set_grad_enabled(False)
    return m.to(cuda).eval()


@pytest.fixture(scope="module")
def engine(cuda):
    from udifftext_amd import lib, pipeline
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)
    return pipeline.build_engine(cuda)


def test_transform_boxes_against_float64_and_the_list_transform(predictor, cuda):
    samples = torch.rand((2, 3, H, W), generator=torch.Generator().manual_seed(12))
    boxes = [[0, 16, 32, 16, 112], [1, 0, 64, 0, 128], [1, 40, 47, 3, 90]]
    x = predictor.transform_boxes(samples.to(cuda), boxes)
    assert x.shape == (3, 3, 32, 128) and x.dtype == torch.float32 and x.is_cuda
    ref, bound = R.crop_resize(samples, boxes, (32, 128), 2.0, -1.0)
    err = (x.double().cpu() - ref).abs()
    print(f"transform_boxes: max |err| per box {[float(e.max()) for e in err]}, bounds {bound.flatten().tolist()}")
    assert bool((err <= bound).all())
    old = predictor.transform([samples[i, :, t:b, l:r].to(cuda) for i, t, b, l, r in boxes])
    rel = float((x - old).double().pow(2).mean().sqrt() / old.double().pow(2).mean().sqrt())
    print(f"transform_boxes vs transform on hand-sliced crops: rel {rel:.3e}")
    assert rel <= 1e-5
    assert torch.equal(predictor.transform_boxes(samples.to(cuda), torch.tensor(boxes)), x)          # (a host tensor as well as a list)
    txt = predictor.img2txt_boxes(samples.to(cuda), boxes)
    assert len(txt) == 3 and all(isinstance(t, str) for t in txt)
    for bad in ([[2, 0, 8, 0, 8]], [[0, 8, 8, 0, 8]], [[0, 0, 65, 0, 8]], [[0, 0, 8, -1, 8]], [[0, 0, 8, 0, 129]]):
        with pytest.raises(ValueError, match="box 0"):
            predictor.transform_boxes(samples.to(cuda), bad)


def test_txt_of_is_deterministic(predictor, cuda):
    x = torch.rand((5, 3, 32, 128), generator=torch.Generator().manual_seed(2)).to(cuda) * 2.0 - 1.0
    a, b = predictor.txt_of(x), predictor.txt_of(x)
    assert len(a) == 5 and all(isinstance(t, str) for t in a) and a == b


def _batches():
    from udifftext_amd import synth
    out = []
    for k in range(2):
        b = synth.synthetic_batch(2, H, W, 4, seed=70 + k)
        b["r_bbox"] = torch.tensor([[24, 40, 16, 112], [8 * k, 33 + 8 * k, 5, 128 - 7 * k]])      # 16x96 (synthetic_batch's), and a ragged one
        out.append(b)
    return out


def test_evaluate_end_to_end(engine, predictor, cuda):
    from udifftext_amd import config as C, pipeline
    cfgs = C.default_runtime_config(steps=STEPS, batch_size=2, noise_iters=0)
    boxes = [torch.cat((torch.arange(2).reshape(-1, 1), b["r_bbox"]), 1) for b in _batches()]
    ref_out = pipeline.predict_many(cfgs, engine, pipeline.init_sampling(STEPS, 5.0, cuda), _batches(), cuda, in_flight=2, fuse=1,
                                    image_seeds=SEEDS)
    reader = S.KernelMeanReader(predictor)
    res = pipeline.evaluate(cfgs, engine, pipeline.init_sampling(STEPS, 5.0, cuda), _batches(), reader, cuda, in_flight=2, fuse=1,
                            image_seeds=SEEDS, ocr_batch=3, return_samples=True)
    assert len(res["outputs"]) == 2 and reader.chunks == [3, 1]
    for (a, za), (b, zb) in zip(res["outputs"], ref_out):
        assert a.shape == (2, 3, H, W) and torch.equal(a, b) and torch.equal(za, zb)
    want = []
    for (img, _), bx in zip(ref_out, boxes):
        ref, bound = R.crop_resize(img.cpu(), bx, (32, 128), 2.0, -1.0)
        means = ((ref + 1.0) / 2.0).mean(dim=(1, 2, 3))
        for m, bd in zip(means.tolist(), bound.flatten().tolist()):       # (the inputs' own validity: no mean within the bound of a bin edge)
            assert S.margin_to_bin_edge(m) > bd, (m, bd)
        want.append([S.text_of_mean(m) for m in means.tolist()])
    assert res["pred"] == want
    assert res["label"] == [b["label"] for b in _batches()] and res["total"] == 4
    assert res["correct"] == sum(p.lower() == t.lower() for ps, ts in zip(want, res["label"]) for p, t in zip(ps, ts))
    # the real predictor: interface only
    res = pipeline.evaluate(cfgs, engine, pipeline.init_sampling(STEPS, 5.0, cuda), _batches(), predictor, cuda, in_flight=2, fuse=1,
                            image_seeds=SEEDS)
    assert set(res) == {"accuracy", "correct", "total", "pred", "label"}
    assert res["total"] == 4 and 0 <= res["correct"] <= res["total"] and res["accuracy"] == res["correct"] / 4
    assert [len(p) for p in res["pred"]] == [2, 2] and all(isinstance(t, str) for p in res["pred"] for t in p)
