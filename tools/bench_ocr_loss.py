"""What the OCR loss's gradient costs: ``ParseqPredictor.calc_loss_boxes`` with and without the reverse pass, next to
``calc_loss`` on the same crops — the only form the parent commit has.  One MI355X, synthetic PARSeq weights with the sharpened head of
tests/ocr_loss_ref.py, 16 frames of 512 x 512 with one 128 x 384 box each; the three modes alternate, every repetition is timed with
device events around it plus one synchronisation (so the host time of issuing the launches is inside the figure: the pass is
launch-bound), 3 warm-up and ``--reps`` timed repetitions per mode.

    a   calc_loss_boxes(want_grad=True)     crop + resize, AR loop, taped refinement pass, loss + seed, reverse pass, crop-resize adjoint
    b   calc_loss_boxes(want_grad=False)    the same without the reverse pass
    c   calc_loss on the hand-sliced crops  one F.interpolate per crop, the untaped inference forward (the parent's route)

The launch counts are the library's own (udt_prof_*: every entry point but udt_mattn_fwd brackets its launches); torch's copies and
casts are not in them.  The result is written below the "# ---- timing" line of profiles/ocr_loss_grad.txt (the part above it belongs to
tests/test_ocr_loss_gpu.py).

    python tools/bench_ocr_loss.py --commit <hash> [--reps 20]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import udifftext_amd  # noqa: E402,F401
from udifftext_amd import ops, synth  # noqa: E402

MARK = "# ---- timing"
SHARPEN = 16.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    res = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, res


def launches(fn):
    """library launches of fn(), summed over the profiling classes"""
    ops.prof_enable(0x3f)
    ops.prof_reset()
    fn()
    torch.cuda.synchronize()
    n = sum(int(ops.prof_get(c)[1]) for c in range(6))
    ops.prof_enable(0)
    ops.prof_reset()
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ocr_loss_grad.txt"))
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.set_grad_enabled(False)
    from sgm.modules.predictors.model import ParseqPredictor
    from sgm.util import skip_param_init
    with skip_param_init():
        predictor = ParseqPredictor(ckpt_path=None)
    synth.fill_module_(predictor.parseq, prefix="parseq.")
    with torch.no_grad():
        predictor.parseq.head.weight.mul_(SHARPEN)
        predictor.parseq.head.bias.mul_(SHARPEN)
    predictor = predictor.to(dev).eval()
    n, s = args.frames, args.size
    frames = (torch.rand((n, 3, s, s), generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)     # a decoder's output range
    t, b, l, r = s * 3 // 8, s * 5 // 8, s // 8, s * 7 // 8                                              # 128 x 384 at 512 x 512
    boxes = [[i, t, b, l, r] for i in range(n)]
    # labels the scorer itself reads off the boxes (first 6 characters), so that most rows stay below the clamp and carry a gradient
    labels = [(y[:6] or "a") for y in predictor.img2txt_boxes(frames, boxes)]
    lines = []

    def say(line=""):
        print(line, flush=True)
        lines.append(line)

    modes = {"a": ("calc_loss_boxes(want_grad=True)", lambda: predictor.calc_loss_boxes(frames, boxes, labels)),
             "b": ("calc_loss_boxes(want_grad=False)", lambda: predictor.calc_loss_boxes(frames, boxes, labels, want_grad=False)),
             "c": ("calc_loss on sliced crops (the parent's route)", lambda: predictor.calc_loss([frames[i, :, t:b, l:r] for i in range(n)], labels))}
    say(MARK + f": measured once, at commit {args.commit}")
    say(f"{n} frames of {s} x {s}, one {b - t} x {r - l} box each, synthetic PARSeq weights (head x {SHARPEN:g}); modes alternating, 3 warm-up and "
        f"{args.reps} timed repetitions each; device events around a repetition + one synchronisation (host launch time included)")
    times = {m: [] for m in modes}
    for rep in range(args.reps + 3):
        for m, (_, fn) in modes.items():
            dt, res = timed(fn)
            if rep >= 3:
                times[m].append(dt)
    loss, grad = modes["a"][1]()
    say(f"rows below the clamp (carrying a gradient): {int((loss < 1).sum())} of {n}; decoded length {predictor.parseq.last_refine_tokens.shape[1]}; "
        f"max |gradient| {float(grad.abs().max()):.3e}")
    for m, (what, _) in modes.items():
        ts = times[m]
        say(f"mode {m} {what}: median {1e3 * statistics.median(ts):.2f} ms, fastest {1e3 * min(ts):.2f} ms, slowest {1e3 * max(ts):.2f} ms")
    na, nb = launches(modes["a"][1]), launches(modes["b"][1])
    say(f"library launches: {na} with the reverse pass, {nb} without: the reverse pass (tape.backward + the crop-resize adjoint) is {na - nb} launches")
    med = {m: statistics.median(times[m]) for m in modes}
    say(f"the reverse pass costs {1e3 * (med['a'] - med['b']):.2f} ms on top of the taped forward; the taped forward against the parent's "
        f"inference forward: {1e3 * (med['b'] - med['c']):+.2f} ms")
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
