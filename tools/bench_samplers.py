"""images/s of the sampler family at bench.py's workload: 512x512, batches of 4, the predict_many default lanes
(parallel.predict_sharded on one GPU, pipeline.IN_FLIGHT lanes, fuse 1), CFG 5, no noise search.

    python tools/bench_samplers.py [--steps K] [--warmup W] [--configs euler_50,dpmpp2m_20,...]

One JSON line per configuration on stdout (``name``, ``sampler``, ``sampler_steps``, ``unet_evaluations``, ``images_per_s``).
Euler 50 is bench.py's ``value`` measured the same way.  For the step kernel's time per launch run one configuration under
``rocprofv3 --kernel-trace --stats`` and read ``cfg_sampler_kernel`` (``cfg_multistep_kernel`` for linear_multistep) from the
stats file.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"euler_50": ("euler", 50), "dpmpp2m_20": ("dpmpp2m", 20), "euler_a_20": ("euler_a", 20), "heun_10": ("heun", 10),
           "dpmpp2s_a_10": ("dpmpp2s_a", 10), "linear_multistep_20": ("linear_multistep", 20)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6, help="timed batches of --batch images")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--chars", type=int, default=9)
    ap.add_argument("--configs", default=",".join(CONFIGS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_samplers.py needs an MI355X")
    import udifftext_amd  # noqa: F401
    from udifftext_amd import config as C, parallel, pipeline, synth
    dev = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    with contextlib.redirect_stdout(sys.stderr):
        model = pipeline.build_engine(dev)
    n_b = args.warmup + args.steps
    batches = [{k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in
                synth.synthetic_batch(args.batch, args.size, args.size, args.chars, seed=1000 + i).items()} for i in range(n_b)]
    seeds = [77 + i for i in range(n_b)]
    for name in args.configs.split(","):
        kind, n = CONFIGS[name]
        sampler = pipeline.init_sampling(n, 5.0, dev, sampler=kind)
        cfgs = C.default_runtime_config(steps=n, batch_size=args.batch, noise_iters=0)
        sig = [float(s) for s in sampler.discretization(n, device="cpu")]
        evals = sum(len(p) for _, p in sampler.plans(sig))

        def run(idx):
            return parallel.predict_sharded(cfgs, model, sampler, [batches[i] for i in idx], [seeds[i] for i in idx],
                                            micro_batch=args.batch, fuse=1, device=dev)
        if args.warmup > 0:            # as bench.py: every grouping of the timed region has captured its graphs
            run([i % args.warmup for i in range(max(args.warmup, args.steps))])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = run(list(range(args.warmup, n_b)))[-1]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert bool(torch.isfinite(frames).all())
        print(json.dumps({"name": name, "sampler": type(sampler).__name__, "sampler_steps": n, "unet_evaluations": evals,
                          "images_per_s": args.batch * args.steps / dt, "s_per_batch": dt / args.steps,
                          "batch": args.batch, "size": args.size, "in_flight": pipeline.IN_FLIGHT}), flush=True)
        del sampler
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
