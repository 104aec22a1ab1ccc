#!/usr/bin/env python
"""Cost of the optimiser step over the 112 trained tensors at their real sizes (75.9 M values, 304 MB), on one GPU, in one process.

    python tools/bench_optimizer.py [--runs 30] [--warmup 5] [--out profiles/optimizer_step.txt] [--commit <id>]

Measured, each the median of ``--runs`` (>= 20) device-event timings after ``--warmup``, the routes alternating inside one loop:

  per-tensor route   training.allreduce_gradients(force=True) + training.AdamW.step          (one concatenated bucket, a copy back and
                     a scale per tensor, one udt_adamw_f32 launch per tensor)
  bucket route       GradBucket.average(force=True) + BucketAdamW.step + GradBucket.zero_()  (collectives in place, ONE launch)
  the two steps      the same without the collectives (AdamW.step; BucketAdamW.step + zero_)
  update kernel      udt_bucket_update_f32 alone: AdamW, AdamW + EMA, EMA only

The collectives run on RCCL in a world of one (``force``), as tests/test_training_gpu.py does: their traffic is local, what differs
between the routes is the concatenation / copy back around them.  GB/s figures count the bytes the update itself must move
(AdamW: read p, g, m, v, write p, m, v = 7 x 4 B per value; + EMA: read and write the shadow = 9 x; EMA only: 3 x) against the
roughly 6.3 TB/s a streaming kernel reaches on the MI355X.  Exit status 1 if the bucket route is slower than the per-tensor route.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 6.3


def trained_shapes():
    """(state-dict name, shape) of the tensors configure_optimizers selects, from the model config (no weights are filled)"""
    import udifftext_amd  # noqa: F401
    from sgm.util import instantiate_from_config, skip_param_init
    from udifftext_amd import config as C, training
    cfg = C.default_model_config()
    with skip_param_init():
        eng = instantiate_from_config(cfg.model)
    return [(n, tuple(p.shape)) for n, p in training.trainable_parameters(eng, ["t_attn", "t_norm"])]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_optimizer needs a GPU: a CPU run gives no time")
    import torch.distributed as dist
    from udifftext_amd import lib as L, ops, training
    dev = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    shapes = trained_shapes()
    n_val = sum(int(torch.Size(s).numel()) for _, s in shapes)
    g = torch.Generator(device="cpu").manual_seed(0)
    mk = lambda s, scale: (torch.randn(s, generator=g) * scale).to(dev)
    named_a = [(n, mk(s, 0.05)) for n, s in shapes]                     # the per-tensor route's parameters
    named_b = [(n, p.clone()) for n, p in named_a]                      # the bucket route's
    grads = {n: mk(s, 1e-3) for n, s in shapes}
    names = [n for n, _ in shapes]
    hyper = dict(lr=5e-5, eps=1e-8, weight_decay=1e-2)
    opt_a = training.AdamW(named_a, **hyper)
    opt_b = training.BucketAdamW(named_b, **hyper)
    ema = training.Ema(named_b)
    for n in names:
        opt_b.bucket.views[n].copy_(grads[n])
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    seg, cmap = opt_b._segments.tables(ema.shadows())
    bucket = opt_b.bucket

    def route_a():
        training.allreduce_gradients(grads, names, dist, force=True)
        opt_a.step(grads)

    def route_b():
        bucket.average(dist, force=True)
        opt_b.step(bucket, grad_scale=1.0)
        bucket.zero_()

    def kernel(mode):
        def run():
            ops.bucket_update_(seg, cmap, bucket.flat, opt_b.m, opt_b.v, mode, step=3, grad_scale=1.0, one_minus_decay=1e-4, **hyper)
        return run
    def step_a():
        opt_a.step(grads)

    def step_b():
        opt_b.step(bucket, grad_scale=1.0)
        bucket.zero_()
    work = [("per-tensor route: allreduce_gradients + AdamW.step", route_a, 7), ("bucket route: average + BucketAdamW.step + zero_", route_b, 7),
            ("  without the collectives: AdamW.step", step_a, 7), ("  without the collectives: BucketAdamW.step + zero_", step_b, 7),
            ("udt_bucket_update_f32 AdamW", kernel(L.BUCKET_ADAMW), 7), ("udt_bucket_update_f32 AdamW + EMA", kernel(L.BUCKET_ADAMW | L.BUCKET_EMA), 9),
            ("udt_bucket_update_f32 EMA only", kernel(L.BUCKET_EMA), 3)]
    times = {name: [] for name, _, _ in work}
    try:
        for it in range(args.warmup + args.runs):
            for name, fn, _ in work:                                        # alternating: every route sees the same machine state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
    finally:
        dist.destroy_process_group()
    lines = [f"# optimiser step over {len(shapes)} trained tensors, {n_val / 1e6:.1f} M values ({4 * n_val / 1e6:.0f} MB fp32); median of {args.runs} "
             f"runs after {args.warmup} warm-up, device events, one process, routes alternating" + (f"; commit {args.commit}" if args.commit else ""),
             f"# GB/s: the bytes the update must move (7 / 9 / 3 x 4 B per value) over the time; a streaming kernel reaches ~{STREAM_TBS} TB/s"]
    result = {"tensors": len(shapes), "values": n_val, "runs": args.runs, "commit": args.commit, "ms": {}}
    for name, _, k in work:
        ms = statistics.median(times[name])
        gbs = k * 4 * n_val / (ms * 1e-3) / 1e9
        result["ms"][name] = ms
        lines.append(f"{name:58s} {ms:8.3f} ms  (min {min(times[name]):.3f}, max {max(times[name]):.3f})  {gbs:8.0f} GB/s  "
                     f"{100 * gbs / (STREAM_TBS * 1e3):5.1f} % of streaming")
    a, b = result["ms"][work[0][0]], result["ms"][work[1][0]]
    lines.append(f"bucket route / per-tensor route: {b / a:.3f} ({'no slower' if b <= a else 'SLOWER'})")
    print("\n".join(lines))
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if b <= a else 1


if __name__ == "__main__":
    sys.exit(main())
