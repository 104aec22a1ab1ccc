"""The fixture of tests/test_ocr_train_gpu.py, chosen on the CPU from float64 references alone (a helper, not a test).

Latent 8 x 8, B = 3, one box per image.  The latents are decoded by the float64 oracle (tests/vae_backward_ref.py), the boxes are
cropped and resized by tests/crop_resize_ref.py, and the labels are the float64 oracle scorer's own greedy reading of those crops —
how tests/ocr_loss_ref.py builds its fixture, with the same sharpened scorer.  Row WRONG_ROW gets a wrong label, so it is clamped.
tests/test_vae_backward_cpu.py pins the conditions: every live row's float64 cross entropy <= 0.8, the clamped row's >= 1.2, and the
reading is stable: under noise of twice the decoder's stated forward tolerance on the frames the float64 scorer reads the same
greedy tokens and the live rows' cross entropy moves by less than half of LOSS_TOL (the sharpened head makes most draws fragile:
a greedy near-tie turns one character of a label into a wrong one).
"""
import torch

import crop_resize_ref as R
import ocr_loss_ref as O
import vae_backward_ref as V

B, LAT = 3, (8, 8)
BOXES = [[16, 48, 0, 64], [8, 40, 4, 60], [24, 56, 0, 64]]           # (top, bottom, left, right) per image
WRONG_ROW, WRONG_LABEL = 1, "ZZ~"
SEED = 11               # of seeds 0 .. 23, one of the few whose reading survives decode-sized noise (``perturbed``): seed 2's does not
LATENT_SCALE = 3.0                                                    # (latents of the size the VAE tests decode)
SCALER = 0.18215

_FIXTURE = {}


def boxes5():
    return [[i] + list(bb) for i, bb in enumerate(BOXES)]


def fixture(seed=None):
    """dict(z [3, 4, 8, 8] = model_output / SCALER, model_output, frames64, labels, tgt_in, raw64 [3], live rows) — once per process"""
    if _FIXTURE and seed is None:
        return _FIXTURE
    from oracle import parseq as OP
    _, sd = V.build_vae()
    z = torch.randn((B, 4, *LAT), generator=torch.Generator().manual_seed(SEED if seed is None else seed)) * LATENT_SCALE
    with torch.no_grad(), V.f64_nets():
        frames64 = V.decode_fn(sd)(z.double())
    psd = O.sharpened_weights()
    psd64 = {k: v.double() for k, v in psd.items()}
    x64, _ = R.crop_resize(frames64, boxes5(), (32, 128), 2.0, -1.0)
    tok = OP.Tokenizer()
    with torch.no_grad():
        ar = OP.parseq_forward(psd64, x64, refine_iters=0)
        tgt_in = torch.cat([torch.full((B, 1), tok.bos_id, dtype=torch.long), ar[:, :-1].argmax(-1)], dim=1)
        labels = [(y[:6] or "a") for y in tok.decode(O.refine_logits(psd64, x64, tgt_in).softmax(-1))[0]]
    labels[WRONG_ROW] = WRONG_LABEL
    raw64, _ = O.chain_ref(psd, x64, tgt_in, labels, torch.float64)
    out = dict(z=z, model_output=z * SCALER, frames64=frames64, labels=labels, tgt_in=tgt_in, raw64=raw64, psd=psd,
               live=[b for b in range(B) if b != WRONG_ROW])
    if seed is None:
        _FIXTURE.update(out)
    return out


def perturbed(fx, k, rel=2 * 2e-2):
    """(same greedy tokens?, float64 cross entropy [3]) of the fixture's labels on frames64 + noise draw k of relative RMS ``rel``"""
    from oracle import parseq as OP
    f = fx["frames64"]
    noise = torch.randn(f.shape, generator=torch.Generator().manual_seed(100 + k), dtype=torch.float64) * f.pow(2).mean().sqrt() * rel
    x, _ = R.crop_resize(f + noise, boxes5(), (32, 128), 2.0, -1.0)
    psd64 = {n: v.double() for n, v in fx["psd"].items()}
    tok = OP.Tokenizer()
    with torch.no_grad():
        ar = OP.parseq_forward(psd64, x, refine_iters=0)
        tgt = torch.cat([torch.full((B, 1), tok.bos_id, dtype=torch.long), ar[:, :-1].argmax(-1)], dim=1)
    same = tgt.shape == fx["tgt_in"].shape and bool((tgt == fx["tgt_in"]).all())
    raw, _ = O.chain_ref(fx["psd"], x, fx["tgt_in"] if not same else tgt, fx["labels"], torch.float64)
    return same, raw
