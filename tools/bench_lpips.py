"""What LPIPS costs: every launch of udifftext_amd.lpips_alex.LPIPS for one chunk of 32 pairs of 512 x 512 frames, the
convolutions' share of the 157 TFLOP/s fp32 peak, and pipeline.evaluate on 16 batches of 4 images at 512 x 512, 50 steps (the workload
of profiles/ocr_evaluate.txt) with and without the module.  One MI355X, synthetic weights; device events around every timed piece.

    python tools/bench_lpips.py --commit <hash> [--out FILE] [--runs 2] [--pairs 32] [--skip-evaluate]
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
from udifftext_amd import config as C, ops, pipeline, synth  # noqa: E402
from udifftext_amd.lpips_alex import ALEX_CONVS, LPIPS, POOL_BEFORE, map_sizes  # noqa: E402

PEAK_F32 = 157e12


def timed(fn, reps=1):
    """fn() ``reps`` times between two device events -> (seconds per call, the last result)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    with contextlib.redirect_stdout(io.StringIO()):
        for _ in range(reps):
            res = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips.txt"))
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--pairs", type=int, default=32)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--skip-evaluate", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    m = LPIPS().fill_synthetic_().to(dev)
    N, S = args.pairs, args.size
    g = torch.Generator().manual_seed(3)
    samples = torch.rand((N, 3, S, S), generator=g).to(dev)
    images = (torch.rand((N, 3, S, S), generator=g) * 2.0 - 1.0).to(dev)
    convs, lins, shift, scale = m.packed()
    sizes = map_sizes(S, S)
    say(f"LPIPS-Alex in fp32, one chunk of {N} pairs of {S} x {S} frames ({2 * N} frames through the network), synthetic weights; per launch: "
        f"2 warm-up calls, then 5 calls between two device events")
    say(f"measured on {args.commit}")
    say()
    out = torch.empty((N,), dtype=torch.float32, device=dev)
    scratch = torch.empty((max(ops.lpips_layer_scratch_bytes(N, h * w) for h, w in sizes),), dtype=torch.uint8, device=dev)
    total_us = conv_us = conv_flop = 0.0

    def piece(name, fn, flop=0.0):
        nonlocal total_us, conv_us, conv_flop
        timed(fn, 2)
        dt, res = timed(fn, 5)
        total_us += dt * 1e6
        extra = ""
        if flop:
            conv_us += dt * 1e6
            conv_flop += flop
            extra = f", {flop / 1e9:.1f} GFLOP, {flop / dt / 1e12:.1f} TFLOP/s = {100 * flop / dt / PEAK_F32:.1f} % of the 157 TFLOP/s fp32 peak"
        say(f"  {name}: {dt * 1e6:.0f} us{extra}")
        return res

    f = piece("udt_lpips_input_f32", lambda: ops.lpips_input(samples, images, shift, scale, True))
    for k, (w, b, cout, ks, stride, pad) in enumerate(convs):
        if POOL_BEFORE[k]:
            f = piece(f"udt_maxpool3s2_f32 {tuple(f.shape)}", lambda f=f: ops.maxpool3s2_f32(f))
        cin = f.shape[3]
        h, wd = sizes[k]
        flop = 2.0 * 2 * N * h * wd * cout * ks * ks * cin
        f = piece(f"udt_conv2d_f32 conv{k + 1} {tuple(f.shape)} -> {cout}, {ks}x{ks} / {stride}", lambda f=f: ops.conv2d_f32(f, w, b, cout, ks, stride, pad, relu=True),
                  flop)
        piece(f"udt_lpips_layer_f32 tap {k + 1} ({h * wd} pixels, C {cout}; two launches)", lambda f=f, k=k: ops.lpips_layer(f, lins[k], out, k > 0, scratch))
    say(f"  sum of the launches: {total_us:.0f} us; the five convolutions {conv_us:.0f} us for {conv_flop / 1e9:.1f} GFLOP = "
        f"{conv_flop / conv_us / 1e6:.1f} TFLOP/s = {100 * conv_flop / conv_us * 1e6 / PEAK_F32:.1f} % of peak")
    timed(lambda: m(samples, images), 1)
    dt, val = timed(lambda: m(samples, images), 3)
    say(f"  LPIPS.forward on the chunk (allocations included): {dt * 1e3:.2f} ms = {dt * 1e3 / N:.3f} ms per pair; mean value {float(val.mean()):.6f}")
    del f, samples, images
    say()
    if not args.skip_evaluate:
        from sgm.modules.predictors.model import ParseqPredictor
        from sgm.util import skip_param_init
        engine = pipeline.build_engine(dev)
        with skip_param_init():
            predictor = ParseqPredictor(ckpt_path=None)
        synth.fill_module_(predictor.parseq, prefix="parseq.")
        predictor = predictor.to(dev).eval()
        nb, bsz, n_img = args.batches, args.batch_size, args.batches * args.batch_size
        seeds = [[9000 + bsz * k + i for i in range(bsz)] for k in range(nb)]
        batches = lambda: [synth.synthetic_batch(bsz, S, S, 9, seed=30 + k) for k in range(nb)]
        cfgs = C.default_runtime_config(steps=args.steps, batch_size=bsz, noise_iters=0)
        sampler = pipeline.init_sampling(args.steps, 5.0, dev)
        modes = {"plain": lambda: pipeline.evaluate(cfgs, engine, sampler, batches(), predictor, dev, image_seeds=seeds),
                 "lpips": lambda: pipeline.evaluate(cfgs, engine, sampler, batches(), predictor, dev, image_seeds=seeds, lpips=m)}
        say(f"pipeline.evaluate, {nb} batches of {bsz} images of {S} x {S}, {args.steps} steps (the workload of profiles/ocr_evaluate.txt, whose "
            f"evaluate took 5.71 s at its commit); one warm-up and {args.runs} timed runs per mode, modes alternating")
        times = {k: [] for k in modes}
        for run in range(args.runs + 1):
            for k, fn in modes.items():
                dt, res = timed(fn)
                extra = f"; lpips {res['lpips']:.6f}" if k == "lpips" else ""
                say(f"  {k} {'warm-up' if run == 0 else f'run {run}'}: {dt:.3f} s = {n_img / dt:.2f} images/s{extra}")
                if run:
                    times[k].append(dt)
        a, b = statistics.median(times["plain"]), statistics.median(times["lpips"])
        say(f"  medians: without lpips {a:.3f} s, with lpips {b:.3f} s: + {b - a:.3f} s = {100 * (b - a) / a:.2f} % = {1e3 * (b - a) / n_img:.2f} ms "
            f"per image")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
