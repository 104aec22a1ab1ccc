"""The AutoencoderKL decoder on a tape: ``first_stage_model.decode`` with its reverse pass.

The OCR term of the training loss (reference loss.py:178-190) decodes the denoiser's output and scores the crops; its gradient
reaches the UNet through the decoder.  As in ``udifftext_amd.backward``, every layer has a ``*_fwd`` that runs the forward through
the same ops as inference — unfused where the fused form keeps no intermediate: ``ops.group_norm``, then the convolution — keeps
what the reverse pass reads and returns ``(out, bwd)`` with ``bwd(d_out) -> d_in``.  Only activations are differentiated (the first
stage is frozen):

  * convolution backward-data = the forward kernels on rotated taps (``backward.conv_bwd``);
  * GroupNorm (+ SiLU) backward = udt_gn_bwd, the residual's gradient fused in as ``add``;
  * nearest x2 backward = udt_sum2x2_bf16 behind the convolution's backward-data at the high resolution;
  * the mid-block attention (one head of 512 dims) = udt_attn512_bwd between two GEMMs on transposed weights.

Nothing is recomputed: at 512 x 512, B = 4 the kept activations come to a few GB.  A cotangent of ``None`` means "exactly zero".
"""
from __future__ import annotations

from typing import Optional

import torch
from sgm.modules import hipnn as H

from . import ops, packing
from .backward import _conv_wt, conv_bwd


def _gn(norm, x: torch.Tensor, silu: bool) -> torch.Tensor:
    return ops.group_norm(x, norm.weight, norm.bias, norm.num_groups, norm.eps, silu)


def _gn_bwd(norm, x: torch.Tensor, dy: torch.Tensor, silu: bool, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    return ops.group_norm_bwd(x, dy, norm.weight, norm.bias, norm.num_groups, norm.eps, silu, add=add)


def vae_resnet_fwd(rb, x: torch.Tensor):
    """ResnetBlock (reference model.py:91-148, temb_channels = 0) on bf16 NHWC: GN(eps 1e-6) + SiLU -> conv3x3 -> GN + SiLU ->
    conv3x3, plus the 1x1 nin_shortcut where the channel count changes.  Keeps x and h1."""
    a1 = _gn(rb.norm1, x, True)
    w1, b1 = rb.conv1.packed()
    h1 = ops.conv2d(a1, w1, b1, ksize=3, n_out=w1.shape[0])
    a2 = _gn(rb.norm2, h1, True)
    ident = rb.in_channels == rb.out_channels
    if ident:
        skip = x
    else:
        ws, bs = rb.nin_shortcut.packed()
        skip = ops.conv2d(x, ws, bs, ksize=1, pad=(0, 0), n_out=ws.shape[0])
    w2, b2 = rb.conv2.packed()
    out = ops.conv2d(a2, w2, b2, ksize=3, residual=skip, n_out=w2.shape[0])
    del a1, a2, skip

    def bwd(d_out):
        if d_out is None:
            return None
        d_a2 = conv_bwd(rb.conv2, d_out)
        d_h1 = _gn_bwd(rb.norm2, h1, d_a2, True)
        d_a1 = conv_bwd(rb.conv1, d_h1)
        d_skip = d_out if ident else conv_bwd(rb.nin_shortcut, d_out)
        return _gn_bwd(rb.norm1, x, d_a1, True, add=d_skip)
    return out, bwd


def _attn_wT(attn):
    """backward-data weights of the attention block (layouts of the module): proj_out^T, and the fused [q|k|v]^T as one [C, 3 C] GEMM"""
    c = attn.in_channels
    f = lambda m: m.weight.detach().reshape(c, c)
    wo_t = H.layout(attn, "woT", lambda: packing.pack_linear(f(attn.proj_out).t().contiguous()))
    wqkv_t = H.layout(attn, "wqkvT", lambda: packing.pack_linear(torch.cat([f(attn.q), f(attn.k), f(attn.v)], dim=0).t().contiguous()))
    return wo_t, wqkv_t


def vae_attn_fwd(attn, x: torch.Tensor):
    """MemoryEfficientAttnBlock (reference model.py:201-262) on bf16 NHWC, C = 512: GN without SiLU, the fused q|k|v linear,
    udt_attn512_fwd, proj_out with the residual.  Keeps x, q|k|v and o."""
    B, Hh, Ww, C = x.shape
    if C != 512:
        raise NotImplementedError(f"the VAE attention's reverse pass is built for one head of 512 dims (udt_attn512_bwd), not {C}")
    N = Hh * Ww
    scale = C ** -0.5
    wqkv, bqkv, _, _, wo, bo = attn.packed()
    hn = _gn(attn.norm, x, False).reshape(B * N, C)
    qkv = ops.linear(hn, wqkv, bqkv).reshape(B, N, 3 * C)
    del hn
    o = ops.attention_d512(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], scale)
    out = ops.linear(o.reshape(B * N, C), wo, bo, residual=x.reshape(B * N, C), rows_per_batch=N).reshape(B, Hh, Ww, C)

    def bwd(d_out):
        if d_out is None:
            return None
        wo_t, wqkv_t = _attn_wT(attn)
        d_o = ops.linear(d_out.reshape(B * N, C), wo_t, None).reshape(B, N, C)
        d_qkv = ops.attention_d512_bwd(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], o, d_o, scale)
        d_hn = ops.linear(d_qkv.reshape(B * N, 3 * C), wqkv_t, None).reshape(B, Hh, Ww, C)
        return _gn_bwd(attn.norm, x, d_hn, False, add=d_out)
    return out, bwd


def vae_upsample_fwd(up, x: torch.Tensor):
    """Upsample (reference model.py:55-68): the module's own nearest x2 + conv3x3; reverse: the convolution's backward-data at
    2H x 2W, then 2 x 2 block sums.  Keeps nothing."""
    out = up.conv(x, upsample=True)

    def bwd(d_out):
        if d_out is None:
            return None
        return ops.sum2x2(conv_bwd(up.conv, d_out))
    return out, bwd


def decode_tape(first_stage_model, z: torch.Tensor):
    """``first_stage_model.decode(z)`` with its reverse pass: z fp32 [B, 4, h, w] on the GPU -> (frames fp32 [B, 3, 8h, 8w], bwd);
    bwd(d_frames fp32 [B, 3, 8h, 8w]) -> d_z fp32 [B, 4, h, w] (None for None).  post_quant_conv, conv_in, the mid block, the four
    levels, norm_out and conv_out; h != w works.  After ``prepare(free_masters=True)`` the transposed layouts cannot be built and
    ``hipnn.layout`` raises its UdtError."""
    from sgm.util import require_gpu
    require_gpu(z, "vae_backward.decode_tape")
    dec = first_stage_model.decoder
    pqc = first_stage_model.post_quant_conv
    zin = ops.nchw_to_nhwc(z.float().contiguous(), packing.KPAD)
    h = dec.conv_in(pqc(zin))
    del zin
    tape = []
    for fwd, mod in ((vae_resnet_fwd, dec.mid.block_1), (vae_attn_fwd, dec.mid.attn_1), (vae_resnet_fwd, dec.mid.block_2)):
        h, b = fwd(mod, h)
        tape.append(b)
    for lv in reversed(range(dec.num_resolutions)):
        for blk in dec.up[lv].block:
            h, b = vae_resnet_fwd(blk, h)
            tape.append(b)
        if lv != 0:
            h, b = vae_upsample_fwd(dec.up[lv].upsample, h)
            tape.append(b)
    a = _gn(dec.norm_out, h, True)
    w, bb = dec.conv_out.packed()
    frames = ops.nhwc_to_nchw(ops.conv2d(a, w, bb, ksize=3, flags=H.GEMM_OUT_F32, n_out=w.shape[0]), dec.out_ch)
    del a
    h_last = h

    def bwd(d_frames):
        if d_frames is None:
            return None
        assert d_frames.shape == frames.shape, f"d_frames {tuple(d_frames.shape)}, frames {tuple(frames.shape)}"
        d = ops.nchw_to_nhwc(d_frames.float().contiguous(), packing.KPAD)
        d = _gn_bwd(dec.norm_out, h_last, conv_bwd(dec.conv_out, d), True)
        for b in reversed(tape):
            d = b(d)
        d = conv_bwd(dec.conv_in, d, n_pad=packing.KPAD)                 # (post_quant_conv is a GEMM: its K is padded to 64)
        wt = _conv_wt(pqc)
        d_z = ops.conv2d(d, wt, None, ksize=1, pad=(0, 0), flags=H.GEMM_OUT_F32, n_out=wt.shape[0])
        return ops.nhwc_to_nchw(d_z, z.shape[1])
    return frames, bwd
