"""Attend-and-excite throughput: predict one image at a time against predict_many over the same images fused into one sampling batch
(EulerEDMSampler.sample_rows_with_attend_and_excite).  One MI355X, 512 x 512, 50 steps, synthetic weights, fixed
per-image seeds; per mode one warm-up run and three timed runs:

    a   pipeline.predict with aae_enabled, one image after the other                      (runs on any commit: the baseline)
    b   pipeline.predict_many(aae_enabled) over the images as one-image batches fused into one unit, record_losses on
    c   the same with record_losses off

    python tools/bench_aae_rows.py --commit <hash> [--modes a,b,c] [--baseline <report of mode a at the parent commit>] [--out FILE]

Per mode: seconds per image of every run, evaluations, per-row update counts, and the frozen-row evaluations as a share of B x
evaluations.  With --baseline the report quotes that file and states the acceptance comparison: the slowest (b) run against the fastest
baseline (a) run, per image.  On synthetic weights every iterated step runs to its cap (the t_attn maps are nearly uniform, the loss
never reaches the thresholds), so the frozen share is zero here; with trained weights it is unmeasured.
"""
import argparse
import contextlib
import io
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import udifftext_amd  # noqa: E402,F401
from udifftext_amd import config as C, pipeline, rng, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="a,b,c")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aae_rows.txt"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    engine = pipeline.build_engine(dev)
    n, seeds = args.images, [[5000 + i] for i in range(args.images)]
    batches = lambda: [synth.synthetic_batch(1, args.size, args.size, 9, seed=30 + i) for i in range(n)]
    lines = [f"attend-and-excite, {n} images of {args.size} x {args.size}, {args.steps} steps, synthetic weights, per-image seeds "
             f"{[s[0] for s in seeds]}; one warm-up and {args.runs} timed runs per mode", f"measured at commit {args.commit}", ""]
    results = {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for mode in args.modes.split(","):
        cfgs = C.default_runtime_config(steps=args.steps, batch_size=1, noise_iters=0)
        cfgs.aae_enabled = True
        sampler = pipeline.init_sampling(args.steps, 5.0, dev)
        per_image = []
        for run in range(args.runs + 1):
            bs = batches()
            e0 = getattr(sampler, "aae_evaluations", 0)
            f0 = getattr(sampler, "aae_frozen_row_evaluations", 0)
            sampler.__dict__.pop("aae_row_updates", None)
            rows = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                if mode == "a":
                    for b, s in zip(bs, seeds):
                        ei = getattr(sampler, "aae_evaluations", 0)
                        with rng.per_image(s):
                            pipeline.predict(cfgs, engine, sampler, b, dev)
                        rows.append(sampler.aae_evaluations - ei)          # (B = 1: every evaluation is an update of the row)
                else:
                    pipeline.predict_many(cfgs, engine, sampler, bs, dev, in_flight=1, fuse=n, image_seeds=seeds,
                                          record_losses=(mode == "b"))
                    rows = sampler.aae_row_updates.tolist()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / n
            evals = sampler.aae_evaluations - e0
            frozen = getattr(sampler, "aae_frozen_row_evaluations", 0) - f0
            B = 1 if mode == "a" else n
            tag = "warm-up" if run == 0 else f"run {run}"
            say(f"mode {mode} {tag}: {dt:.3f} s per image; {evals} evaluations at B = {B}; row updates {rows}; frozen-row evaluations "
                f"{frozen} = {100.0 * frozen / max(1, B * evals):.1f} % of B x evaluations")
            if run:
                per_image.append(dt)
        results[mode] = per_image
        say(f"mode {mode}: fastest {min(per_image):.3f}, slowest {max(per_image):.3f} s per image")
        say("")
    if args.baseline:
        text = open(args.baseline).read()
        base = [float(v) for v in re.findall(r"^mode a run \d+: ([0-9.]+) s per image", text, flags=re.M)]
        say("---- baseline: mode a measured at the parent commit ----")
        for ln in text.strip().splitlines():
            say("  " + ln)
        say("")
        if base and "b" in results:
            ok = max(results["b"]) < min(base)
            say(f"acceptance: slowest (b) run {max(results['b']):.3f} s per image against the fastest parent-commit (a) run {min(base):.3f} s "
                f"per image: {'met' if ok else 'NOT met'} ({min(base) / max(results['b']):.2f}x)")
            if "c" in results:
                say(f"record_losses off (c): slowest run {max(results['c']):.3f} s per image ({min(base) / max(results['c']):.2f}x)")
    say("On synthetic weights every iterated step runs to its cap, so no row freezes before its mates and the frozen share is zero; "
        "the share with trained weights is unmeasured.")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
