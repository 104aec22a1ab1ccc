"""Generate tests/golden/vae_backward_golden.npz: the REAL reference's AutoencoderKL decoder under torch.autograd, on the CPU.

    UDT_REFERENCE=<reference checkout> python tests/golden/make_vae_backward_golden.py        # under a minute

make_golden.py's import recipe; the first stage of configs/test/textdesign_sd_2.yaml (ch 128, ch_mult (1, 2, 4, 4), 2 res blocks,
``attn_type: vanilla`` — the exact softmax attention of the reference's AttnBlock) with udifftext_amd.synth weights, in float64.

  d8     latent 8 x 8,  B = 2
  d8x16  latent 8 x 16, B = 1

Stored per case: z (fp32 values), a fixed random d_frames (fp32 values), frames = decode(z) and d_z = d <d_frames, frames> / d z in
float64, and the bf16 twin's d_z — the same module run in torch.bfloat16 under the same autograd — with its per-sample relative RMS
error against the float64 d_z (the yardstick of tests/test_vae_backward_gpu.py).  Only arrays are stored.
"""
from __future__ import annotations

import copy
import os
import sys
import time

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (import_reference / strip_ckpt; exits without UDT_REFERENCE)
from make_rect_golden import save_npz_deterministic  # noqa: E402

from udifftext_amd import synth  # noqa: E402

CASES = {"d8": (2, 8, 8, 31), "d8x16": (1, 8, 16, 32)}       # case -> (B, h, w, seed)


def rel_rms(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).pow(2).mean().sqrt() / b.double().pow(2).mean().sqrt())


def main():
    t0 = time.time()
    MG.import_reference()
    from sgm.util import instantiate_from_config
    cfg = yaml.safe_load(open(os.path.join(MG.REF, "configs/test/textdesign_sd_2.yaml")))
    MG.strip_ckpt(cfg)
    fcfg = cfg["model"]["params"]["first_stage_config"]
    fcfg["params"]["ddconfig"]["attn_type"] = "vanilla"
    with torch.no_grad():
        vae = instantiate_from_config(fcfg).eval()
        for name, p in vae.state_dict().items():
            full = "first_stage_model." + name
            if not synth.is_computed_buffer(full):
                p.copy_(synth.synthetic_tensor(full, tuple(p.shape)))
    for p in vae.parameters():
        p.requires_grad_(False)
    vae64 = copy.deepcopy(vae).double()
    twin = copy.deepcopy(vae).to(torch.bfloat16)
    out = {}
    for case, (B, h, w, seed) in CASES.items():
        g = torch.Generator().manual_seed(seed)
        z = torch.randn((B, 4, h, w), generator=g)
        d_frames = torch.randn((B, 3, 8 * h, 8 * w), generator=g)
        with torch.enable_grad():
            z64 = z.double().requires_grad_(True)
            frames = vae64.decode(z64)
            (d_z,) = torch.autograd.grad((frames * d_frames.double()).sum(), [z64])
            zb = z.bfloat16().requires_grad_(True)
            fb = twin.decode(zb)
            (d_zb,) = torch.autograd.grad((fb.float() * d_frames.bfloat16().float()).sum(), [zb])
        assert tuple(frames.shape) == (B, 3, 8 * h, 8 * w)
        out[f"{case}_z"] = z.numpy()
        out[f"{case}_d_frames"] = d_frames.numpy()
        out[f"{case}_frames"] = frames.detach().numpy()
        out[f"{case}_d_z"] = d_z.numpy()
        out[f"{case}_twin_d_z"] = d_zb.float().numpy()
        out[f"{case}_twin_rel"] = np.array([rel_rms(d_zb[b], d_z[b]) for b in range(B)], dtype=np.float64)
        print(f"[vae backward golden] {case}: twin relRMS {out[f'{case}_twin_rel']} ({time.time() - t0:.1f}s)")
    save_npz_deterministic(os.path.join(HERE, "vae_backward_golden.npz"), out)
    print(f"[vae backward golden] written ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
