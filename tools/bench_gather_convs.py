"""The UNet's gathered 3x3 convolutions (nearest x2 upsampling folded into the gather, stride 2) next to a staged-patch
convolution of the same FLOPs — how much the gather form (gemm8<CONV>) costs against conv3p.

``python tools/bench_gather_convs.py phase``: only the second table — the six upsampling convolutions of the benchmarked workload
(three of a UNet call on 8 samples, three of the VAE decoder on a batch of 4) on the nine-tap instance (upsample = 1) and in the
phase form (four 2x2 phase convolutions on packing.pack_conv_up4 weights) on the lean and, where its geometry admits the shape,
the wide kernel; per launch from the library's own events (udt_prof_get), planned alone and for three launch streams."""
import math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from udifftext_amd import ops, packing

dev = torch.device("cuda", 0)


def timed(fn, iters=30):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


for share in (() if "phase" in sys.argv[1:] else (1, 3)):
    print(f"cu_share {share}")
    for B, Hin, C, N, mode in [(8, 32, 640, 640, "up"), (8, 16, 1280, 1280, "up"), (8, 8, 1280, 1280, "up"),
                               (8, 64, 320, 320, "s2"), (8, 32, 640, 640, "s2"), (8, 16, 1280, 1280, "s2")]:
        x = torch.randn((B, Hin, Hin, C), device=dev).bfloat16()
        w = packing.pack_conv(torch.randn((N, C, 3, 3), device=dev) / math.sqrt(C * 9))
        b = torch.zeros((N,), device=dev)
        with ops.launch_context(cu_share=share):
            if mode == "up":
                Ho = 2 * Hin
                us = timed(lambda: ops.conv2d(x, w, b, upsample=True))
                xr = torch.randn((B, Ho, Ho, C), device=dev).bfloat16()
                ref = timed(lambda: ops.conv2d(xr, w, b))
            else:
                Ho = Hin // 2
                us = timed(lambda: ops.conv2d(x, w, b, stride=2))
                xr = torch.randn((B, Ho, Ho, C), device=dev).bfloat16()
                ref = timed(lambda: ops.conv2d(xr, w, b))
        fl = 2.0 * B * Ho * Ho * N * C * 9
        print(f"  {mode} {B}x{Hin}x{Hin} {C}->{N} (out {Ho}x{Ho}): this launch {us:7.1f} us {fl/us/1e6:5.0f} TF | staged-patch conv of the same output {ref:7.1f} us {fl/ref/1e6:5.0f} TF", flush=True)


def launch_us(fn, iters=20):
    """(us per launch from the library's events around it, the launch's tag)"""
    from udifftext_amd import lib as L
    lib = L.load()
    for _ in range(3): fn()
    torch.cuda.synchronize()
    ops.prof_reset(); lib.udt_prof_trace(1); ops.prof_enable(1)
    fn()
    torch.cuda.synchronize()
    ops.prof_enable(0)
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "udt_bench_gather_trace.csv")
    lib.udt_prof_dump(path.encode()); lib.udt_prof_trace(0)
    tag = open(path).read().splitlines()[1].split(",", 2)[2]
    ops.prof_reset(); ops.prof_enable(1)
    for _ in range(iters): fn()
    torch.cuda.synchronize()
    ms, n = ops.prof_get(0)
    ops.prof_enable(0)
    return ms / n * 1e3, tag


PHASE_SHAPES = [(8, 8, 1280, 1280), (8, 16, 1280, 1280), (8, 32, 640, 640),          # UNet call on 8 samples: 8->16, 16->32, 32->64
                (4, 64, 512, 512), (4, 128, 512, 512), (4, 256, 256, 256)]           # VAE decoder, batch of 4
for share in (1, 3):
    from udifftext_amd import lib as L
    print(f"upsampling convolutions, nine taps against the phase form; cu_share {share}")
    for B, Hin, C, N in PHASE_SHAPES:
        x = torch.randn((B, Hin, Hin, C), device=dev).bfloat16()
        w4 = torch.randn((N, C, 3, 3), device=dev) / math.sqrt(C * 9)
        w, wu, b = packing.pack_conv(w4), packing.pack_conv_up4(w4), torch.zeros((N,), device=dev)
        fl = 2.0 * B * 4 * Hin * Hin * N * C * 9                     # the reference formulation's nine taps
        row = []
        with ops.launch_context(cu_share=share):
            row.append(("nine-tap",) + launch_us(lambda: ops.conv2d(x, w, b, upsample=True)))
            for name, knob in (("phase", -1), ("phase lean", 0), ("phase wide", 1)):
                if knob == 1 and (N % 160 or Hin % 16):
                    continue
                L.check(L.load().udt_debug_set(b"wide_conv", knob), "udt_debug_set")
                try:
                    row.append((name,) + launch_us(lambda: ops.conv2d(x, w, b, upsample=True, w_up4=wu)))
                finally:
                    L.check(L.load().udt_debug_set(b"wide_conv", -1), "udt_debug_set")
        print(f"  {B}x{Hin}x{Hin} {C}->{N}:")
        for name, us, tag in row:
            print(f"    {name:10s} {us:8.1f} us {fl / us / 1e6:5.0f} TF  [{tag}]", flush=True)
        del x, w4, w, wu
