"""Host logic of pipeline.evaluate on the stub engine and sampler of tests/test_parallel_cpu.py with a stand-in reader
(tests/evaluate_standin.py): order and grouping of the predictions, the chunks the reader sees, the counts, the refusals."""
import pytest
import torch

import evaluate_standin as S
from test_parallel_cpu import _StubModel, _StubSampler

CPU = torch.device("cpu")
N_BATCHES, PER = 5, 2
SEEDS = [[100 + 2 * k, 101 + 2 * k] for k in range(N_BATCHES)]


class _Model(_StubModel):
    def parameters(self):
        return iter([torch.zeros(1)])

    def decode_first_stage(self, z):                      # (8 x 8 frames: the size of the batch's images, which the boxes refer to)
        return z[:, :3].repeat_interleave(4, -1).repeat_interleave(4, -2) * 0.1


class _Sampler(_StubSampler):
    def __init__(self):
        self.n_calls = 0

    def get_init_noise(self, *a, **k):
        self.n_calls += 1
        return super().get_init_noise(*a, **k)

    def sample_in_flight(self, *a, **k):
        self.n_calls += 1
        return super().sample_in_flight(*a, **k)


def _boxes(k):
    """two different boxes per batch, different from batch to batch, touching edges and corners of the 8 x 8 image"""
    return torch.tensor([[0, 1 + k, 0, 8 - k], [k, 8, 3, 4 + k % 4 + 1]])


def _batch(k, labels=None, boxes=None):
    g = torch.Generator().manual_seed(300 + k)
    b = {"image": torch.rand((PER, 3, 8, 8), generator=g), "label": list(labels or [f"x{k}{i}" for i in range(PER)]),
         "txt": [f"t{i}" for i in range(PER)], "name": [str(i) for i in range(PER)]}
    if boxes is not False:
        b["r_bbox"] = _boxes(k) if boxes is None else boxes
    return b


def _cfgs():
    from udifftext_amd import config as C
    return C.default_runtime_config(steps=2, batch_size=PER, noise_iters=0)


@pytest.fixture(scope="module")
def expected():
    """the samples of every batch (image seeds: independent of fuse and in_flight) and the table's text of every box"""
    from udifftext_amd import pipeline
    outs = pipeline.predict_many(_cfgs(), _Model(), _Sampler(), [_batch(k) for k in range(N_BATCHES)], CPU, in_flight=1, fuse=1,
                                 image_seeds=SEEDS)
    pred = []
    for k, (img, _) in enumerate(outs):
        assert img.shape == (PER, 3, 8, 8)
        bx = torch.cat((torch.arange(PER).reshape(-1, 1), _boxes(k)), 1)
        pred.append([S.text_of_mean(m) for m in S.box_means(img, bx).tolist()])
    assert len({p for ps in pred for p in ps}) >= 3, "the stand-in's strings do not tell the boxes apart"
    return outs, pred


@pytest.mark.parametrize("ocr_batch,chunks", [(1, [1] * 10), (3, [3, 3, 3, 1]), (64, [10]), (None, [2] * 5)])
@pytest.mark.parametrize("in_flight,fuse", [(1, 1), (3, 2), (2, 0)])
def test_order_and_grouping(expected, ocr_batch, chunks, in_flight, fuse):
    from udifftext_amd import pipeline
    outs, pred = expected
    reader = S.MeanReader()
    res = pipeline.evaluate(_cfgs(), _Model(), _Sampler(), [_batch(k) for k in range(N_BATCHES)], reader, CPU, in_flight=in_flight,
                            fuse=fuse, image_seeds=SEEDS, ocr_batch=ocr_batch)
    assert res["pred"] == pred
    assert res["label"] == [[f"x{k}{i}" for i in range(PER)] for k in range(N_BATCHES)]
    assert reader.chunks == chunks
    assert len(reader.boxes) == N_BATCHES                                     # one transform_boxes per returned batch
    for k, bx in enumerate(reader.boxes):
        assert bx.tolist() == torch.cat((torch.arange(PER).reshape(-1, 1), _boxes(k)), 1).tolist()
    assert "outputs" not in res and res["total"] == N_BATCHES * PER and res["correct"] == 0 and res["accuracy"] == 0.0


def test_counts_and_case_insensitive_match(expected):
    from udifftext_amd import pipeline
    _, pred = expected
    labels = [[p.swapcase() if (k + i) % 3 != 0 else p + "x" for i, p in enumerate(ps)] for k, ps in enumerate(pred)]
    n_right = sum((k + i) % 3 != 0 for k in range(N_BATCHES) for i in range(PER))
    assert 0 < n_right < N_BATCHES * PER
    assert any(l != p for ls, ps in zip(labels, pred) for l, p in zip(ls, ps) if l.lower() == p.lower())     # (case does differ)
    res = pipeline.evaluate(_cfgs(), _Model(), _Sampler(), [_batch(k, labels=labels[k]) for k in range(N_BATCHES)], S.MeanReader(), CPU,
                            image_seeds=SEEDS)
    assert res["correct"] == n_right and res["total"] == N_BATCHES * PER and res["accuracy"] == n_right / (N_BATCHES * PER)
    assert res["pred"] == pred and res["label"] == labels
    assert set(res) == {"accuracy", "correct", "total", "pred", "label"}


@pytest.mark.parametrize("bad,match", [(False, "r_bbox"),
                                       (torch.tensor([[0, 4, 0, 8], [3, 3, 0, 8]]), "image 1"),            # empty box
                                       (torch.tensor([[0, 4, 0, 9], [0, 4, 0, 8]]), "image 0"),            # past the right edge
                                       (torch.tensor([[0, 4, 0, 8], [-1, 4, 0, 8]]), "image 1")])          # past the top edge
def test_refusals_fire_before_any_sampling(bad, match):
    from udifftext_amd import pipeline
    sm, reader = _Sampler(), S.MeanReader()
    batches = [_batch(0), _batch(1), _batch(2, boxes=bad)]
    with pytest.raises(ValueError, match=match):
        pipeline.evaluate(_cfgs(), _Model(), sm, batches, reader, CPU, image_seeds=SEEDS[:3])
    assert sm.n_calls == 0 and not reader.boxes and not reader.chunks


def test_return_samples_is_the_predict_many_list(expected):
    from udifftext_amd import pipeline
    outs, _ = expected
    sm = _Sampler()
    res = pipeline.evaluate(_cfgs(), _Model(), sm, [_batch(k) for k in range(N_BATCHES)], S.MeanReader(), CPU, in_flight=3, fuse=2,
                            image_seeds=SEEDS, return_samples=True)
    assert sm.n_calls > 0 and len(res["outputs"]) == N_BATCHES
    for (a, za), (b, zb) in zip(res["outputs"], outs):
        assert torch.equal(a, b) and torch.equal(za, zb)
