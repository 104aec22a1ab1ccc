"""Generate tests/golden/rect_golden.npz: the REAL reference on rectangular images (H != W), on the CPU.

    UDT_REFERENCE=<reference checkout> python tests/golden/make_rect_golden.py        # ~4 minutes

make_golden.py's import recipe and synthetic weights, CFG 5, deterministic Euler (10 steps), batch 1.  The reference's plain path
(conditioner, UNet, EulerEDMSampler.__call__, decode_first_stage) takes H and W separately; its map consumers (get_min_local_loss,
save_attn_map) raise for H != W, so nothing of them is recorded here (tests/rect_ref.py restates them).

  r1  256x384 (latent 32x48), "TEXT":       c / uc concat and a sub-sample of c.t_crossattn, one UNet call of the CFG pair at t = 999
                                            (eps; name, heads, shape and a strided sub-sample of the 16 t_attn maps), the VAE
                                            moments of the image, x0, the 10-step latent, a decoded sub-sample
  r2  384x256 (latent 48x32), "TEXT":       c / uc concat, one UNet call (eps), x0, the 10-step latent, a decoded sub-sample
  r3  512x768 (latent 64x96), "Diffusion":  c / uc concat, x0, the 10-step latent, a decoded sub-sample

Seeds: the conditioner runs under torch.manual_seed(1234) (draw order pinned, as G6), the UNet input is
torch.Generator().manual_seed(7) (as G7), x0 is drawn under torch.manual_seed(99) (as G9).  The archive is written with fixed
zip timestamps: a re-run is byte-identical.
"""
from __future__ import annotations

import io
import os
import sys
import time
import types
import zipfile

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (install_stubs / import_reference / strip_ckpt / sub; exits without UDT_REFERENCE)

from udifftext_amd import synth  # noqa: E402

# case -> (H, W, characters of the label, seed of the synthetic batch, one UNet call?, maps / moments?)
CASES = {"r1": (256, 384, 4, 0, True, True), "r2": (384, 256, 4, 0, True, False), "r3": (512, 768, 9, 12, False, False)}


def save_npz_deterministic(path: str, arrays: dict) -> None:
    """np.savez_compressed with fixed member timestamps (numpy stamps the members with the wall clock)"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    t0 = time.time()
    torch.set_grad_enabled(False)
    MG.import_reference()
    from sgm.util import instantiate_from_config
    import sgm.modules.diffusionmodules.sampling as S

    cfg = yaml.safe_load(open(os.path.join(MG.REF, "configs/test/textdesign_sd_2.yaml")))
    MG.strip_ckpt(cfg)
    model = instantiate_from_config(cfg["model"]).eval()
    torch.nn.Module.train(model.conditioner.embedders[0], False)      # (make_golden.py: the LabelEncoder dropout quirk)
    for name, p in model.state_dict().items():
        if not synth.is_computed_buffer(name):
            p.copy_(synth.synthetic_tensor(name, tuple(p.shape)))
    print(f"[rect golden] reference engine ready ({time.time() - t0:.1f}s)")

    class _TorchProxy:                                     # (make_golden.py: the samplers' torch.device on the CPU)
        def __getattr__(self, n):
            return getattr(torch, n)

        @staticmethod
        def device(*a, **k):
            return torch.device("cpu")

    S.torch = _TorchProxy()
    unet = model.model.diffusion_model
    out = {}
    for case, (Hh, Ww, n_chars, seed, one_call, maps) in CASES.items():
        h, w = Hh // 8, Ww // 8
        batch = synth.synthetic_batch(1, Hh, Ww, n_chars, seed=seed)
        torch.manual_seed(1234)
        buc = {k: (v.clone() if isinstance(v, torch.Tensor) else list(v)) for k, v in batch.items()}
        buc["label"] = ["" for _ in batch["label"]]
        buc["txt"] = ["" for _ in batch["txt"]]
        c, uc = model.conditioner.get_unconditional_conditioning(batch, batch_uc=buc, force_uc_zero_embeddings=["label"])
        assert tuple(c["concat"].shape) == (1, 5, h, w)
        out[f"{case}_c_concat"] = c["concat"].numpy()
        out[f"{case}_uc_concat"] = uc["concat"].numpy()
        out[f"{case}_c_txt_sub"] = c["t_crossattn"][:, :, ::16].numpy()
        if one_call:
            x7 = torch.randn((1, 4, h, w), generator=torch.Generator().manual_seed(7))
            xin = torch.cat([torch.cat([x7, x7]), torch.cat([uc["concat"], c["concat"]])], dim=1)
            tctx = torch.cat([uc["t_crossattn"], c["t_crossattn"]])
            eps = unet(xin, timesteps=torch.tensor([999, 999]), t_context=tctx)
            out[f"{case}_x"] = x7.numpy()
            out[f"{case}_eps"] = eps.numpy()
            if maps:
                names = []
                for i, item in enumerate(unet.attn_map_cache):
                    names.append(item["name"])
                    out[f"{case}_attn_{i:02d}_meta"] = np.array([int(item["heads"]), int(item["size"])] + list(item["attn_map"].shape))
                    out[f"{case}_attn_{i:02d}_sub"] = MG.sub(item["attn_map"], 2048)
                out[f"{case}_attn_names"] = np.array(names)
                fs = model.first_stage_model
                out[f"{case}_moments"] = fs.quant_conv(fs.encoder(batch["image"])).numpy()
        sampler = S.EulerEDMSampler(
            num_steps=10,
            discretization_config={"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"},
            guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": 5.0}},
            s_churn=0.0, s_tmin=0.0, s_tmax=999.0, s_noise=1.0, verbose=False, device="cpu")
        cfgs = types.SimpleNamespace(batch_size=1, channel=4, factor=8, gpu=0, noise_iters=0)
        torch.manual_seed(99)
        x0 = sampler.get_init_noise(cfgs, model, cond=c, batch=batch, uc=uc)
        assert tuple(x0.shape) == (1, 4, h, w)
        out[f"{case}_x0"] = x0.numpy()
        z = sampler(model, x0.clone(), cond=c, batch=batch, uc=uc, init_step=0, aae_enabled=False, detailed=False)
        out[f"{case}_latent"] = z.numpy()
        dec = model.decode_first_stage(z)
        assert tuple(dec.shape) == (1, 3, Hh, Ww)
        out[f"{case}_decoded_sub"] = dec[:, :, ::8, ::8].numpy()
        print(f"[rect golden] {case} {Hh}x{Ww} done ({time.time() - t0:.1f}s)")
    save_npz_deterministic(os.path.join(HERE, "rect_golden.npz"), out)
    print(f"[rect golden] written ({time.time() - t0:.1f}s)")


if __name__ == "__main__":
    main()
