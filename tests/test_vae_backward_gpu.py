"""The AutoencoderKL decoder on a tape (udifftext_amd/vae_backward.py) on the GPU (``pytest -m gpu``).

Per layer — ``vae_resnet_fwd`` 512 -> 512 and 512 -> 256 (shortcut) at 8 x 8, ``vae_attn_fwd`` at 8 x 8 and 8 x 16, the Upsample pair
at 4 x 4 -> 8 x 8 — against float64 autograd of the matching ``oracle.nets`` function (tests/vae_backward_ref.py), relRMS under
TOL_SLICE = 3e-2, the project's stated bound for a two-block slice (tests/test_backward_gpu.py; these are shorter); each layer's tape
forward agrees with its inference forward to the forward's stated tolerance (TOL_FWD = 2e-2, tests/test_engine_gpu.py).

The decoder — ``decode_tape`` on the cases of tests/golden/vae_backward_golden.npz (the real reference in float64): frames within
TOL_FWD of the golden; per sample relRMS(d_z - golden) <= TWIN_FACTOR x the bf16 twin's relRMS and in any case <= TOL_UNET = 3e-2
(TWIN_FACTOR = 2 as in tests/test_ocr_loss_gpu.py, for the reason recorded there: kernels and twin are two draws of the same
rounding noise); the dot-product identity <d_frames, J dz> = <d_z, dz> with J dz from float64; a sample whose d_frames is zero gets a
d_z that is exactly zero.  Both numbers per sample go to profiles/vae_backward.txt.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import vae_backward_ref as V

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "vae_backward.txt")
TOL_SLICE = 3e-2
TOL_UNET = 3e-2
TOL_FWD = 2e-2
TWIN_FACTOR = 2.0
DEC = V.PREFIX + "decoder."


def _note(line):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a") as f:
        f.write(line + "\n")
    print(line)


@pytest.fixture(scope="module")
def env(cuda):
    import udifftext_amd  # noqa: F401
    from udifftext_amd import lib, ops, vae_backward
    assert lib.load().udt_device_arch_ok() == 1
    torch.set_grad_enabled(False)
    vae, sd = V.build_vae(cuda)

    class Env:
        pass
    Env.ops, Env.vb, Env.dev, Env.vae, Env.sd = ops, vae_backward, cuda, vae, sd
    return Env


def _nhwc(env, t):
    """NCHW fp32 (CPU) -> bf16 NHWC on the device"""
    return t.permute(0, 2, 3, 1).contiguous().bfloat16().to(env.dev)


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2).double()


def _rand(shape, seed, scale=1.0):
    return (torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed)) * scale).bfloat16().float()


def _layer(env, name, fwd, module, ref_fn, x, d_out, infer):
    """x, d_out: NCHW fp32 holding bf16 values"""
    out, bwd = fwd(module, _nhwc(env, x))
    d_x = bwd(_nhwc(env, d_out))
    assert bwd(None) is None
    ref_out, ref_dx = V.vjp64(ref_fn, x, d_out)
    r_fwd, r_bwd = V.rel_rms(_nchw(out), ref_out), V.rel_rms(_nchw(d_x), ref_dx)
    r_inf = V.rel_rms(_nchw(out), _nchw(infer(_nhwc(env, x))))
    _note(f"{name:44s} forward vs float64 {r_fwd:.3e}, tape vs inference forward {r_inf:.3e}, d_x vs float64 autograd {r_bwd:.3e}")
    assert r_fwd <= TOL_FWD and r_inf <= TOL_FWD, (r_fwd, r_inf)
    assert r_bwd <= TOL_SLICE, r_bwd


@pytest.mark.parametrize("which,cin,cout", [("mid.block_1", 512, 512), ("up.1.block.0", 512, 256)])
def test_resnet_block(env, which, cin, cout):
    from oracle import nets
    dec = env.vae.decoder
    module = dec.mid.block_1 if which == "mid.block_1" else dec.up[1].block[0]
    assert (module.in_channels, module.out_channels) == (cin, cout)
    x, d_out = _rand((2, cin, 8, 8), 11), _rand((2, cout, 8, 8), 12)
    _layer(env, f"vae_resnet_fwd {cin}->{cout} 8x8", env.vb.vae_resnet_fwd, module,
           lambda t: nets._vae_resnet(env.sd, DEC + which + ".", t), x, d_out, module)


@pytest.mark.parametrize("h,w", [(8, 8), (8, 16)])
def test_attention_block(env, h, w):
    from oracle import nets
    module = env.vae.decoder.mid.attn_1
    x, d_out = _rand((2, 512, h, w), 21), _rand((2, 512, h, w), 22)
    _layer(env, f"vae_attn_fwd {h}x{w}", env.vb.vae_attn_fwd, module, lambda t: nets._vae_attn(env.sd, DEC + "mid.attn_1.", t), x, d_out,
           module)


def test_attention_block_other_widths_are_refused(env):
    from sgm.modules.diffusionmodules.model import MemoryEfficientAttnBlock
    with pytest.raises(NotImplementedError, match="512"):
        env.vb.vae_attn_fwd(MemoryEfficientAttnBlock(64), torch.zeros((1, 4, 4, 64), dtype=torch.bfloat16, device=env.dev))


def test_upsample(env):
    from oracle import nets
    module = env.vae.decoder.up[3].upsample
    x, d_out = _rand((2, 512, 4, 4), 31), _rand((2, 512, 8, 8), 32)
    _layer(env, "upsample 512 4x4 -> 8x8", env.vb.vae_upsample_fwd, module,
           lambda t: nets._conv(env.sd, DEC + "up.3.upsample.conv.", F.interpolate(t, scale_factor=2.0, mode="nearest")), x, d_out, module)


# ------------------------------------------------------------------------------------------------ the decoder
@pytest.fixture(scope="module")
def taped(env):
    """case -> (z, d_frames, frames, d_z) of decode_tape on the golden's inputs, computed once"""
    G = V.golden()
    out = {}
    for case in V.CASES:
        z, d_frames = torch.from_numpy(G[f"{case}_z"]), torch.from_numpy(G[f"{case}_d_frames"])
        frames, bwd = env.vb.decode_tape(env.vae, z.to(env.dev))
        out[case] = (z, d_frames, frames, bwd(d_frames.to(env.dev)), bwd)
    return G, out


@pytest.mark.parametrize("case", list(V.CASES))
def test_decode_tape_vs_golden(env, taped, case):
    G, res = taped
    B, h, w = V.CASES[case]
    z, d_frames, frames, d_z, bwd = res[case]
    assert frames.shape == (B, 3, 8 * h, 8 * w) and frames.dtype == torch.float32
    assert d_z.shape == (B, 4, h, w) and d_z.dtype == torch.float32
    assert bwd(None) is None
    r_frames = V.rel_rms(frames, G[f"{case}_frames"])
    r_inf = V.rel_rms(frames, env.vae.decode(z.to(env.dev)))
    _note(f"decode_tape {case}: frames vs golden {r_frames:.3e}, vs first_stage_model.decode {r_inf:.3e}")
    assert r_frames <= TOL_FWD and r_inf <= TOL_FWD
    bad = []
    for b in range(B):
        got, twin = V.rel_rms(d_z[b], G[f"{case}_d_z"][b]), float(G[f"{case}_twin_rel"][b])
        _note(f"decode_tape {case} sample {b}: relRMS(d_z - golden) {got:.3e}, bf16 twin {twin:.3e} (bound {min(TWIN_FACTOR * twin, TOL_UNET):.3e})")
        if not (got <= TWIN_FACTOR * twin and got <= TOL_UNET):
            bad.append((b, got, twin))
    assert not bad, f"(sample, kernels, twin): {bad}"


@pytest.mark.parametrize("case", list(V.CASES))
def test_dot_product_identity(env, taped, case):
    """<d_frames, J dz> = <d_z, dz> for two random perturbations, J dz from the float64 oracle (tied to the golden at 1e-9 by
    tests/test_vae_backward_cpu.py).  The left side is exact; the right side carries d_z's error e, |e| <= TOL_UNET |d_z|, against a
    direction drawn independently of it: <e, dz> is normal with standard deviation |e| |dz| / sqrt(numel), so
    |difference| <= 5 TOL_UNET |d_z| |dz| / sqrt(numel) (five standard deviations).  <d_z, dz> itself is of the size
    |d_z| |dz| / sqrt(numel): a d_z that is zero, or the gradient of something else, misses the bound by a factor 1 / (5 TOL_UNET)."""
    G, res = taped
    z, d_frames, frames, d_z, _ = res[case]
    fn = V.decode_fn(env.sd)
    for k in range(2):
        dz = torch.randn(z.shape, generator=torch.Generator().manual_seed(70 + k), dtype=torch.float64)
        lhs = float((d_frames.double() * V.jvp64(fn, z, dz)).sum())
        rhs = float((d_z.double().cpu() * dz).sum())
        exact = float((torch.from_numpy(G[f"{case}_d_z"]) * dz).sum())
        bound = 5 * TOL_UNET * float(d_z.double().norm()) * float(dz.norm()) / dz.numel() ** 0.5
        _note(f"dot-product identity {case} draw {k}: <d_frames, J dz> {lhs:.6e}, <d_z, dz> {rhs:.6e}, golden {exact:.6e}, bound on the difference {bound:.3e}")
        assert abs(lhs - exact) <= 1e-6 * float(torch.from_numpy(G[f"{case}_d_z"]).norm()) * float(dz.norm())
        assert abs(lhs - rhs) <= bound


def test_a_sample_without_gradient_gets_exactly_zero(env, taped):
    G, res = taped
    z, d_frames, _, d_z, bwd = res["d8"]
    d = d_frames.clone()
    d[1] = 0
    got = bwd(d.to(env.dev))
    assert bool((got[1] == 0).all()), "d_frames == 0 for the sample, d_z is not exactly zero"
    assert bool((got[0] != 0).any())
