"""Generate tests/golden/char_maps_golden.npz: the REAL reference's head-mean character maps of one UNet call, on the CPU.

    UDT_REFERENCE=<reference checkout> python tests/golden/make_char_maps_golden.py        # ~1 minute

make_golden.py's import recipe, stubs and synthetic weights; the G7 setup (256x256 "TEXT" batch under torch.manual_seed(1234), the
CFG pair at t = 999 on torch.Generator().manual_seed(7) 32x32 latents).  Per selected layer the reference's own reduction
(openaimodel.py:559-591 save_attn_map) of the probabilities the call cached — reshape (-1, heads, n, l), mean over heads, permute — for
the CONDITIONAL row only, fp32 [1, 12, n]:

  maps_<layer>      output_blocks.6.1 (the shipped save_attn_layers) and one layer of every width the fused text attention covers
  maps_two_layers   the layer mean of output_blocks.6.1 and output_blocks.7.1 (stack -> mean, as save_attn_map with two layers)

The archive is written with fixed zip timestamps (make_rect_golden.py): a re-run is byte-identical.
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (install_stubs / import_reference / strip_ckpt; exits without UDT_REFERENCE)
from make_rect_golden import save_npz_deterministic  # noqa: E402

from udifftext_amd import synth  # noqa: E402

LAYERS = ("output_blocks.6.1", "input_blocks.1.1", "input_blocks.7.1")      # C = 640 (16x16), 320 (32x32), 1280 (8x8)
PAIR = ("output_blocks.6.1", "output_blocks.7.1")


def head_mean(item):
    """[b * heads, n, l] -> the conditional row's [1, l, n]"""
    m = item["attn_map"].float()
    _, n, l = m.shape
    return m.reshape(-1, int(item["heads"]), n, l).mean(dim=1)[1:].permute(0, 2, 1).contiguous()


def main():
    t0 = time.time()
    torch.set_grad_enabled(False)
    MG.import_reference()
    from sgm.util import instantiate_from_config

    cfg = yaml.safe_load(open(os.path.join(MG.REF, "configs/test/textdesign_sd_2.yaml")))
    MG.strip_ckpt(cfg)
    model = instantiate_from_config(cfg["model"]).eval()
    torch.nn.Module.train(model.conditioner.embedders[0], False)      # (make_golden.py: the LabelEncoder dropout quirk)
    for name, p in model.state_dict().items():
        if not synth.is_computed_buffer(name):
            p.copy_(synth.synthetic_tensor(name, tuple(p.shape)))
    print(f"[char maps golden] reference engine ready ({time.time() - t0:.1f}s)")
    batch = synth.synthetic_batch(1, 256, 256, 4, seed=0)
    torch.manual_seed(1234)
    buc = {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in batch.items()}
    buc["label"] = ["" for _ in batch["label"]]
    buc["txt"] = ["" for _ in batch["txt"]]
    c, uc = model.conditioner.get_unconditional_conditioning(batch, batch_uc=buc, force_uc_zero_embeddings=["label"])
    unet = model.model.diffusion_model
    x7 = torch.randn((1, 4, 32, 32), generator=torch.Generator().manual_seed(7))
    xin = torch.cat([torch.cat([x7, x7]), torch.cat([uc["concat"], c["concat"]])], dim=1)
    tctx = torch.cat([uc["t_crossattn"], c["t_crossattn"]])
    unet(xin, timesteps=torch.tensor([999, 999]), t_context=tctx)
    items = {it["name"]: it for it in unet.attn_map_cache}
    find = lambda layer: items[f"{layer}.transformer_blocks.0.t_attn"]
    out = {"layers": np.array(LAYERS), "pair": np.array(PAIR)}
    for layer in LAYERS:
        out[f"maps_{layer}"] = head_mean(find(layer)).numpy()
    # two layers: stack -> mean -> head mean (the reductions commute; this is the reference's order)
    stacked = torch.stack([find(layer)["attn_map"].float() for layer in PAIR], dim=0).mean(dim=0)
    out["maps_two_layers"] = head_mean({"attn_map": stacked, "heads": find(PAIR[0])["heads"]}).numpy()
    for k, v in out.items():
        print(f"[char maps golden] {k}: {v.shape} {v.dtype}")
    save_npz_deterministic(os.path.join(HERE, "char_maps_golden.npz"), out)
    print(f"[char maps golden] written ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
