"""What FID costs: every launch of udifftext_amd.fid_inception.FID for one chunk of 32 pairs of 512 x 512 frames, split
into input stage, convolutions by block, pools and moments, the convolutions' share of the 157 TFLOP/s fp32 peak, and
pipeline.evaluate on 16 batches of 4 images at 512 x 512, 50 steps (the workload of profiles/lpips.txt) with and without the module.
One MI355X, synthetic weights; device events around every timed piece.  64 images is a TIMING workload: an FID of 64 images against
2048 features is not a meaningful number.

    python tools/bench_fid.py --commit <hash> [--out FILE] [--runs 2] [--pairs 32] [--skip-evaluate]
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import udifftext_amd  # noqa: E402,F401
from udifftext_amd import config as C, ops, pipeline, synth  # noqa: E402
from udifftext_amd.fid_inception import BLOCKS, FID, SIZE, STEM, Conv, FIDStats, block_plan  # noqa: E402

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fid.txt"))
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

    m = FID().fill_synthetic_().to(dev)
    N, S = args.pairs, args.size
    g = torch.Generator().manual_seed(3)
    samples = torch.rand((N, 3, S, S), generator=g).to(dev)
    images = (torch.rand((N, 3, S, S), generator=g) * 2.0 - 1.0).to(dev)
    packed = m.packed()
    say(f"FID InceptionV3 in fp32, one chunk of {N} pairs of {S} x {S} frames ({2 * N} frames of {SIZE} x {SIZE} through the network), synthetic "
        f"weights; per launch: 2 warm-up calls, then 5 calls between two device events")
    say(f"measured on {args.commit}")
    say()
    groups = {}                                                # group -> [conv us, conv flop, pool us, launches]

    def piece(group, fn, flop=0.0):
        timed(fn, 2)
        dt, res = timed(fn, 5)
        rec = groups.setdefault(group, [0.0, 0.0, 0.0, 0])
        rec[0 if flop else 2] += dt * 1e6
        rec[1] += flop
        rec[3] += 1
        return dt, res

    def conv(group, x, op, wb, out=None):
        n, h, w, _ = x.shape
        ho, wo = (h + 2 * op.pad[0] - op.kernel[0]) // op.stride + 1, (w + 2 * op.pad[1] - op.kernel[1]) // op.stride + 1
        flop = 2.0 * n * ho * wo * op.cout * op.kernel[0] * op.kernel[1] * op.cin
        dt, res = piece(group, lambda: ops.conv2d_rect_f32(x, wb[0], wb[1], op.cout, op.kernel, op.stride, op.pad, relu=True, out=out), flop)
        return dt, flop, res

    dt_in, x = piece("input stage", lambda: ops.fid_input(samples, images, True, SIZE))
    say(f"  udt_fid_input_f32 {tuple(samples.shape)} x 2 -> {tuple(x.shape)}: {dt_in * 1e6:.0f} us")
    for op in STEM:
        if isinstance(op, Conv):
            shape = tuple(x.shape)
            dt, flop, x = conv("stem", x, op, packed[op.name])
            say(f"  stem {op.name} {shape} -> {op.cout}, {op.kernel[0]}x{op.kernel[1]} / {op.stride}: {dt * 1e6:.0f} us, {flop / 1e9:.1f} GFLOP, "
                f"{flop / dt / 1e12:.1f} TFLOP/s = {100 * flop / dt / PEAK_F32:.1f} % of peak")
        else:
            shape = tuple(x.shape)
            dt, x = piece("stem", lambda x=x: ops.pool3_f32(x, op.stride, op.pad, op.average))
            say(f"  stem max-pool 3 / 2 {shape}: {dt * 1e6:.0f} us")
    worst = []
    for name, (cin, branches) in BLOCKS.items():
        launches, c_out, c_tmp, stride = block_plan(cin, branches)
        n, h, w, _ = x.shape
        ho, wo = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if stride == 2 else (h, w)
        bufs = {"x": x, "out": torch.empty((n, ho, wo, c_out), dtype=torch.float32, device=dev),
                "tmp": torch.empty((n, h, w, max(c_tmp, 1)), dtype=torch.float32, device=dev)}
        for op, (sb, s0, s1), (db, d0, d1) in launches:
            src, dst = bufs[sb][..., s0:s1], bufs[db][..., d0:d1]
            if isinstance(op, Conv):
                dt, flop, _ = conv(name, src, op, packed[f"{name}.{op.name}"], out=dst)
                worst.append((flop / dt, f"{name}.{op.name} {op.kernel[0]}x{op.kernel[1]} / {op.stride}, {op.cin} -> {op.cout} on {h} x {w}", dt))
            else:
                piece(name, lambda: ops.pool3_f32(src, op.stride, op.pad, op.average, out=dst))
        x = bufs["out"]
    dt_mean, feats = piece("head", lambda: ops.mean_pixels_f32(x))
    total = torch.zeros((feats.shape[1],), dtype=torch.float64, device=dev)
    outer = torch.zeros((feats.shape[1], feats.shape[1]), dtype=torch.float64, device=dev)
    dt_mom, _ = piece("moments", lambda: [ops.moments_accum_f64(feats[k * N:(k + 1) * N], total, outer) for k in range(2)])
    say()
    say("  group: launches, convolutions (time, GFLOP, TFLOP/s, share of the 157 TFLOP/s fp32 peak), other launches")
    conv_us = conv_flop = other_us = 0.0
    for name, (cu, cf, pu, nl) in groups.items():
        conv_us, conv_flop, other_us = conv_us + cu, conv_flop + cf, other_us + pu
        rate = f"{cu:.0f} us, {cf / 1e9:.1f} GFLOP, {cf / cu / 1e6:.1f} TFLOP/s = {100 * cf / cu * 1e6 / PEAK_F32:.1f} %" if cf else "-"
        say(f"  {name}: {nl} launches; convolutions {rate}; pools and the rest {pu:.0f} us")
    say(f"  sum of the launches: {conv_us + other_us:.0f} us; the 94 convolutions {conv_us:.0f} us for {conv_flop / 1e9:.1f} GFLOP = "
        f"{conv_flop / conv_us / 1e6:.1f} TFLOP/s = {100 * conv_flop / conv_us * 1e6 / PEAK_F32:.1f} % of peak (LPIPS's five, the same kernel: "
        f"63.1 TFLOP/s = 40.2 %, profiles/lpips.txt)")
    say(f"  udt_mean_pixels_f32: {dt_mean * 1e6:.0f} us; udt_moments_accum_f64, both sets ({N} rows x 2048 each, 2 x 32 MiB read and written): "
        f"{dt_mom * 1e6:.0f} us")
    worst.sort()
    say("  the five slowest convolutions by rate: " + "; ".join(f"{n}: {r / 1e12:.1f} TFLOP/s, {d * 1e6:.0f} us" for r, n, d in worst[:5]))
    say("  the five longest convolutions: " + "; ".join(f"{n}: {d * 1e6:.0f} us, {r / 1e12:.1f} TFLOP/s"
                                                        for r, n, d in sorted(worst, key=lambda t: -t[2])[:5]))
    st = FIDStats(m)
    timed(lambda: st.update(samples, images), 1)
    dt, _ = timed(lambda: st.update(samples, images), 3)
    say(f"  FIDStats.update on the chunk (allocations included): {dt * 1e3:.2f} ms = {dt * 1e3 / N:.3f} ms per pair")
    t0 = time.perf_counter()
    val = st.compute()
    say(f"  FIDStats.compute on the host (two 2048 x 2048 eigendecompositions, numpy float64): {time.perf_counter() - t0:.2f} s; value {val:.6e} "
        f"({st.n} images: a timing workload, not a meaningful FID)")
    del x, samples, images, bufs, st
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
                 "fid": lambda: pipeline.evaluate(cfgs, engine, sampler, batches(), predictor, dev, image_seeds=seeds, fid=m)}
        say(f"pipeline.evaluate, {nb} batches of {bsz} images of {S} x {S}, {args.steps} steps (the workload of profiles/lpips.txt, whose evaluate "
            f"without LPIPS took 5.74 s at the parent commit); one warm-up and {args.runs} timed runs per mode, modes alternating.  {n_img} images "
            f"is a timing workload, not a meaningful FID")
        times = {k: [] for k in modes}
        for run in range(args.runs + 1):
            for k, fn in modes.items():
                dt, res = timed(fn)
                extra = f"; fid {res['fid']:.6e}" if k == "fid" else ""
                say(f"  {k} {'warm-up' if run == 0 else f'run {run}'}: {dt:.3f} s = {n_img / dt:.2f} images/s{extra}")
                if run:
                    times[k].append(dt)
        a, b = statistics.median(times["plain"]), statistics.median(times["fid"])
        say(f"  medians: without fid {a:.3f} s, with fid {b:.3f} s: + {b - a:.3f} s = {100 * (b - a) / a:.2f} % = {1e3 * (b - a) / n_img:.2f} ms "
            f"per image (the host's eigendecompositions above are part of it, once per evaluate)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
