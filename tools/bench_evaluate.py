"""What scoring costs next to generating: pipeline.evaluate against predict_many alone and against the route that
existed before it.  One MI355X, synthetic weights (UDiffText engine and PARSeq), 16 batches of 4 images at 512 x 512, 50 steps; per
mode one warm-up run and ``--runs`` timed ones, the modes alternating; each run timed with device events around it plus one final
synchronisation:

    a   pipeline.predict_many alone
    b   pipeline.evaluate: predict_many, one crop / resize / normalise launch per batch, PARSeq on chunks of 64 crops
    c   predict_many, then per batch: slice the crops, predictor.img2txt (one F.interpolate per crop, one PARSeq call per batch)

and the preprocessing alone for 64 boxes of 128 x 384 pixels: one udt_crop_resize_aa_f32 launch against the 64 F.interpolate calls of
ParseqPredictor.transform.  On synthetic weights the strings PARSeq returns are noise: the accuracy printed is not a quality figure.

    python tools/bench_evaluate.py --commit <hash> [--out FILE] [--runs 3] [--batches 16] [--steps 50]
"""
import argparse
import contextlib
import io
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import udifftext_amd  # noqa: E402,F401
from udifftext_amd import config as C, pipeline, synth  # noqa: E402


def timed(fn):
    """fn() between two device events on the current stream, one synchronisation after it -> (seconds, fn's result)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    with contextlib.redirect_stdout(io.StringIO()):
        res = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocr_evaluate.txt"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--ocr-batch", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    from sgm.modules.predictors.model import ParseqPredictor
    from sgm.util import skip_param_init
    engine = pipeline.build_engine(dev)
    with skip_param_init():
        predictor = ParseqPredictor(ckpt_path=None)
    synth.fill_module_(predictor.parseq, prefix="parseq.")
    predictor = predictor.to(dev).eval()
    nb, bsz, n_img = args.batches, args.batch_size, args.batches * args.batch_size
    seeds = [[9000 + bsz * k + i for i in range(bsz)] for k in range(nb)]
    batches = lambda: [synth.synthetic_batch(bsz, args.size, args.size, 9, seed=30 + k) for k in range(nb)]
    cfgs = C.default_runtime_config(steps=args.steps, batch_size=bsz, noise_iters=0)
    sampler = pipeline.init_sampling(args.steps, 5.0, dev)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"OCR accuracy at throughput: {nb} batches of {bsz} images of {args.size} x {args.size}, {args.steps} steps, synthetic weights "
        f"(engine and PARSeq), fixed per-image seeds; one warm-up and {args.runs} timed runs per mode, modes alternating; device events "
        f"around each run + one final synchronisation")
    say(f"measured at commit {args.commit}")
    say()

    def mode_a():
        return pipeline.predict_many(cfgs, engine, sampler, batches(), dev, image_seeds=seeds)

    def mode_b():
        return pipeline.evaluate(cfgs, engine, sampler, batches(), predictor, dev, image_seeds=seeds, ocr_batch=args.ocr_batch)

    def mode_c():
        bs = batches()
        boxes = [b["r_bbox"].tolist() for b in bs]                 # (host values, taken before the batch moves to the device)
        labels = [list(b["label"]) for b in bs]
        outs = pipeline.predict_many(cfgs, engine, sampler, bs, dev, image_seeds=seeds)
        correct = 0
        for (samples, _), bx, lb in zip(outs, boxes, labels):
            pred = predictor.img2txt([samples[i, :, t:b, l:r] for i, (t, b, l, r) in enumerate(bx)])
            correct += sum(p.lower() == t.lower() for p, t in zip(pred, lb))
        return correct

    modes = {"a": ("predict_many alone", mode_a), "b": (f"evaluate (ocr_batch {args.ocr_batch})", mode_b),
             "c": ("predict_many + per-batch slicing + img2txt", mode_c)}
    times = {m: [] for m in modes}
    for run in range(args.runs + 1):
        for m, (what, fn) in modes.items():
            dt, res = timed(fn)
            tag = "warm-up" if run == 0 else f"run {run}"
            extra = ""
            if m == "b":
                extra = f"; {res['correct']} of {res['total']} strings equal their label"
            elif m == "c":
                extra = f"; {res} of {n_img} strings equal their label"
            say(f"mode {m} {tag}: {dt:.3f} s = {n_img / dt:.2f} images/s ({what}){extra}")
            if run:
                times[m].append(dt)
    say()
    for m, (what, _) in modes.items():
        ts = times[m]
        say(f"mode {m} ({what}): fastest {min(ts):.3f} s, slowest {max(ts):.3f} s, median {statistics.median(ts):.3f} s = "
            f"{n_img / statistics.median(ts):.2f} images/s")
    med = {m: statistics.median(times[m]) for m in modes}
    say(f"scoring on top of generating (medians): evaluate + {med['b'] - med['a']:.3f} s = {1e3 * (med['b'] - med['a']) / n_img:.2f} ms per "
        f"image; the per-batch route + {med['c'] - med['a']:.3f} s = {1e3 * (med['c'] - med['a']) / n_img:.2f} ms per image")
    say()

    # ---- the preprocessing alone: 64 boxes of 128 x 384 (synthetic_batch's box at 512 x 512) out of 16 batches of 4 images
    g = torch.Generator().manual_seed(1)
    imgs = [torch.rand((4, 3, 512, 512), generator=g).to(dev) for _ in range(16)]
    box = [192, 320, 64, 448]
    per_batch = [[i] + box for i in range(4)]
    reps = 20

    def new_route():
        return torch.cat([predictor.transform_boxes(s, per_batch) for s in imgs])

    def new_one_launch(stack=torch.cat(imgs), bx=[[i] + box for i in range(64)]):
        return predictor.transform_boxes(stack, bx)

    def old_route():
        t, b, l, r = box
        return torch.cat([predictor.transform([s[i, :, t:b, l:r] for i in range(4)]) for s in imgs])

    routes = {"one launch for the 64 boxes (transform_boxes on the stacked images, host validation and box upload included)": new_one_launch,
              "16 launches of 4 boxes (transform_boxes per batch, as evaluate issues them)": new_route,
              "64 F.interpolate calls (transform on hand-sliced crops, 4 per call)": old_route}
    pt = {k: [] for k in routes}
    for rep in range(reps + 2):
        for k, fn in routes.items():
            dt, _ = timed(fn)
            if rep >= 2:
                pt[k].append(dt)
    say(f"preprocessing alone, 64 boxes of 128 x 384 -> 32 x 128, 2 warm-up and {reps} timed repetitions, routes alternating "
        f"(host time of the launches included: each repetition ends in a synchronisation):")
    for k, ts in pt.items():
        say(f"  {k}: median {1e6 * statistics.median(ts):.0f} us, fastest {1e6 * min(ts):.0f} us, slowest {1e6 * max(ts):.0f} us")
    a, b = new_one_launch(), old_route()
    say(f"  largest difference between the two routes' outputs: {float((a - b).abs().max()):.3e}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
