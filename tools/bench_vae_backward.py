"""What the VAE decoder's reverse pass costs, on one MI355X with synthetic weights.  Every repetition is timed with
device events around it plus one synchronisation; variants alternate; 3 warm-up and ``--reps`` timed repetitions each; random operands.

    kernel   udt_attn512_bwd at n = 4096, B = 4 and B = 1: time and TFLOP/s at 5 products of 2 n^2 512 FLOPs per sample, next to
             udt_attn512_fwd on the same operands (2 products) and its recorded figure (profiles/r03_attn512.txt)
    decoder  decode_tape forward + reverse at 512 x 512, B = 4, against first_stage_model.decode alone
    step     training_loss_and_grads at 512 x 512, B = 4 with and without ocr_enabled (``--step``: builds the whole engine)

The launch counts are the library's own (udt_prof_*).  The result is written below the "# ---- timing" line of
profiles/vae_backward.txt (the part above it belongs to tests/test_vae_backward_gpu.py).

    python tools/bench_vae_backward.py --commit <hash> [--reps 20] [--step]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import udifftext_amd  # noqa: E402,F401
from udifftext_amd import ops, synth, vae_backward  # noqa: E402

MARK = "# ---- timing"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, res


def launches(fn):
    ops.prof_enable(0x3f)
    ops.prof_reset()
    fn()
    torch.cuda.synchronize()
    n = sum(int(ops.prof_get(c)[1]) for c in range(6))
    ops.prof_enable(0)
    ops.prof_reset()
    return n


def alternate(modes, reps):
    times = {m: [] for m in modes}
    for rep in range(reps + 3):
        for m, fn in modes.items():
            dt, _ = timed(fn)
            if rep >= 3:
                times[m].append(dt)
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_backward.txt"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    lines = []

    def say(line=""):
        print(line, flush=True)
        lines.append(line)

    def report(tag, ts, flops=None):
        med = statistics.median(ts)
        rate = f", {flops / med * 1e-12:.1f} TFLOP/s at the median" if flops else ""
        say(f"{tag}: median {1e3 * med:.3f} ms, fastest {1e3 * min(ts):.3f} ms, slowest {1e3 * max(ts):.3f} ms{rate}")
        return med

    say(MARK + f": measured once, at commit {args.commit}")
    say(f"3 warm-up and {args.reps} timed repetitions per variant, variants alternating; device events around a repetition + one "
        "synchronisation (host launch time included); random operands")
    # ---- the kernel
    n, scale = 4096, 512 ** -0.5
    for B in (4, 1):
        g = torch.Generator().manual_seed(B)
        qkv = torch.randn((B, n, 1536), generator=g).bfloat16().to(dev)
        d_o = torch.randn((B, n, 512), generator=g).bfloat16().to(dev)
        q, k, v = qkv[..., :512], qkv[..., 512:1024], qkv[..., 1024:]
        o = ops.attention_d512(q, k, v, scale)
        out = torch.empty_like(qkv)
        t = alternate({"fwd": lambda: ops.attention_d512(q, k, v, scale), "bwd": lambda: ops.attention_d512_bwd(q, k, v, o, d_o, scale, out=out)},
                      args.reps)
        report(f"udt_attn512_fwd n {n} B {B} (2 products)", t["fwd"], 2 * 2.0 * n * n * 512 * B)
        report(f"udt_attn512_bwd n {n} B {B} (5 products)", t["bwd"], 5 * 2.0 * n * n * 512 * B)
    say("(profiles/r03_attn512.txt records the forward at B 4: 282 us)")
    # ---- the decoder
    from sgm.util import instantiate_from_config, skip_param_init
    from udifftext_amd import config as C
    with skip_param_init():
        vae = instantiate_from_config(C.default_model_config().model.params.first_stage_config)
    synth.fill_module_(vae, prefix="first_stage_model.")
    vae = vae.to(dev).eval()
    B = 4
    z = (torch.randn((B, 4, 64, 64), generator=torch.Generator().manual_seed(9)) * 3.0).to(dev)
    d_frames = torch.randn((B, 3, 512, 512), generator=torch.Generator().manual_seed(10)).to(dev)

    def both():
        frames, bwd = vae_backward.decode_tape(vae, z)
        return bwd(d_frames)
    t = alternate({"decode": lambda: vae.decode(z), "tape": lambda: vae_backward.decode_tape(vae, z)[0], "both": both}, args.reps)
    report(f"first_stage_model.decode 512 x 512 B {B}", t["decode"])
    report("decode_tape forward", t["tape"])
    report("decode_tape forward + reverse", t["both"])
    n_dec, n_tape, n_both = launches(lambda: vae.decode(z)), launches(lambda: vae_backward.decode_tape(vae, z)), launches(both)
    say(f"library launches: decode {n_dec}, decode_tape forward {n_tape}, forward + reverse {n_both}: the added reverse pass is {n_both - n_tape} launches")
    torch.cuda.synchronize()
    say(f"peak device memory during forward + reverse: {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")
    # ---- the training step
    if args.step:
        from sgm.modules.predictors.model import ParseqPredictor
        from udifftext_amd import pipeline, training
        engine = pipeline.build_engine(dev)
        with skip_param_init():
            predictor = ParseqPredictor(ckpt_path=None)
        synth.fill_module_(predictor.parseq, prefix="parseq.")
        predictor = predictor.to(dev).eval()
        batch = synth.synthetic_batch(B, 512, 512, 9, seed=8)
        torch.manual_seed(1234)
        batch_d, _ = pipeline.prepare_batch(dict(batch), dev)
        cond = engine.conditioner(batch_d)
        zt = (torch.randn((B, 4, 64, 64), generator=torch.Generator().manual_seed(11))).to(dev)
        seg = torch.zeros((B, 12, 512, 512), device=dev)
        seg[:, :9, 192:320, 64:448] = 1.0
        segm = batch["seg_mask"].to(dev)
        idx = torch.full((B,), 500, dtype=torch.long)
        noise = torch.randn((B, 4, 64, 64), generator=torch.Generator().manual_seed(12)).to(dev)
        engine.opt_keys = ["t_attn", "t_norm"]
        lf = engine.loss_fn
        lf.predictor, lf.lambda_ocr_loss = predictor, 0.01
        kw = dict(sigma_idx=idx, noise=noise)

        def step(on):
            lf.ocr_enabled = on
            extra = dict(r_bbox=batch["r_bbox"], label=batch["label"]) if on else {}
            return training.training_loss_and_grads(engine, zt, cond, seg, segm, **kw, **extra)
        t = alternate({"off": lambda: step(False), "on": lambda: step(True)}, max(5, args.reps // 2))
        report(f"training_loss_and_grads 512 x 512 B {B}, ocr_enabled False", t["off"])
        report(f"training_loss_and_grads 512 x 512 B {B}, ocr_enabled True", t["on"])
        n_off, n_on = launches(lambda: step(False)), launches(lambda: step(True))
        say(f"library launches: {n_off} without the OCR term, {n_on} with it")
    head = ""
    if os.path.exists(args.out):
        text = open(args.out).read()
        i = text.find(MARK)
        head = text if i < 0 else text[:i]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(head + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
