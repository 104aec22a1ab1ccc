"""Stand-in OCR readers for the tests of pipeline.evaluate: the text of a crop is a fixed function of the MEAN of its pixels, so what
``evaluate`` returns can be predicted exactly from the samples (PARSeq on synthetic weights has near-tied logits: its strings say
nothing about plumbing).  ``evaluate`` uses ``transform_boxes`` and ``txt_of`` only."""
import torch

TABLE = ["alpha", "Bravo", "charlie", "DELTA", "echo", "Foxtrot", "golf", "HOTEL", "india", "Juliett", "kilo", "LIMA", "mike",
         "November", "oscar", "PAPA"]
BINS = 256                      # a mean in [0, 1] falls into bin int(mean * 256); the table repeats every 16 bins


def text_of_mean(mean: float) -> str:
    return TABLE[int(float(mean) * BINS) % len(TABLE)]


def margin_to_bin_edge(mean: float) -> float:
    v = float(mean) * BINS
    return min(v - int(v), int(v) + 1 - v) / BINS


def box_means(samples: torch.Tensor, boxes) -> torch.Tensor:
    """per box (image index, top, bottom, left, right) the float64 mean of samples[index, :, top:bottom, left:right]"""
    return torch.stack([samples[i, :, t:b, l:r].double().mean() for i, t, b, l, r in torch.as_tensor(boxes).reshape(-1, 5).tolist()])


class MeanReader:
    """plain torch on any device: transform_boxes -> [N] box means; records the boxes and the chunk sizes it is handed"""

    def __init__(self):
        self.boxes, self.chunks = [], []

    def transform_boxes(self, samples, boxes):
        self.boxes.append(torch.as_tensor(boxes).clone())
        return box_means(samples, boxes)

    def txt_of(self, x):
        self.chunks.append(int(x.shape[0]))
        return [text_of_mean(m) for m in x.tolist()]


class KernelMeanReader:
    """transform_boxes is the real predictor's (one udt_crop_resize_aa_f32 launch, normalised to [-1, 1]); txt_of reads the table at
    the mean of the resampled crop"""

    def __init__(self, predictor):
        self.predictor, self.chunks = predictor, []

    def transform_boxes(self, samples, boxes):
        return self.predictor.transform_boxes(samples, boxes)

    def txt_of(self, x):
        self.chunks.append(int(x.shape[0]))
        return [text_of_mean(m) for m in ((x.double() + 1.0) / 2.0).mean(dim=(1, 2, 3)).tolist()]
