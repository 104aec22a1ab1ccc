"""The OCR scorer under differentiation: d loss / d image through PARSeq's last refinement pass.

The reference obtains the OCR term's gradient from ``torch.autograd`` through ``ParseqPredictor.calc_loss`` (reference
sgm/modules/diffusionmodules/loss.py:178-190, sgm/modules/predictors/model.py:40-58).  The scorer here is launches into
libudt_kernels.so, so the reverse pass is written out in the style of ``udifftext_amd.backward.UNetTape``: every layer has a ``*_fwd``
that runs the forward through the same ops as inference — unfused where the fused inference kernel keeps no intermediate (the MLPs: a
plain GEMM with fp32 output, udt_gelu_fwd on the stored pre-activations) — and returns a closure ``bwd(d_out) -> d_in``.

What is differentiated.  The autoregressive logits reach the result only through ``argmax``; the gradient path is the LAST refinement
pass -> memory -> the ViT encoder -> the image.  With one decoder layer (the ``parseq`` hub configuration) the content stream is not
updated and the query stream's self-attention sees ``pos_queries`` and token embeddings only, so everything up to the
cross-attention's QUERY is constant with respect to the image: the decoder's reverse pass is head, decoder.norm, linear2 / GELU /
linear1 / norm2 (+ residual), cross_attn.out_proj, masked attention dK / dV, the k|v projection.  All weights are frozen: dX only.

  * linear backward-data = the forward GEMM on W^T (``backward.linear_bwd``; layouts in the per-module cache ``hipnn.layout``);
  * LayerNorm: udt_layernorm_bwd, the residual's gradient goes in through ``add``;
  * attention: udt_mattn_bwd (encoder: dq, dk, dv written into the column thirds of one d_qkv buffer; decoder: dk | dv only);
  * patch embedding backward-data: one GEMM with fp32 output, then the un-patchify (a view change).

torch is used for memory only (allocation, views, the bf16 cast of the fp32 seed, the un-patchify permutation).
"""
from __future__ import annotations

from typing import Callable, List, Tuple

import torch
from sgm.modules import hipnn as H

from . import ops, packing
from .backward import linear_bwd

Bwd = Callable[[torch.Tensor], torch.Tensor]


def check_supported(parseq) -> None:
    """the configurations the reverse pass is written for; anything else raises instead of differentiating something else"""
    if parseq.refine_iters < 1:
        raise NotImplementedError("the OCR gradient flows through the last refinement pass: refine_iters must be >= 1")
    if len(parseq.decoder.layers) != 1:
        raise NotImplementedError(f"dec_depth = {len(parseq.decoder.layers)}: the decoder's reverse pass is written for one layer "
                                  "(the parseq hub configuration), where the cross-attention queries are constants")


# ------------------------------------------------------------------------------------------------ layers
def _plain(gl) -> Tuple[torch.Tensor, torch.Tensor]:
    """the plain (no GEGLU epilogue) layout of a _GeluLinear: tape mode needs its pre-activations"""
    return H.layout(gl, "plain_fc", lambda: (packing.pack_linear(gl.weight), packing.pad_bias(gl.bias)))


def mlp_fwd(fc1, fc2, xn: torch.Tensor, residual: torch.Tensor, tape: bool = True):
    """fc2(gelu(fc1(xn))) + residual on bf16 rows [M, C]; bwd(d_out) -> d_xn (the residual's gradient is d_out itself).
    tape=False (every ``*_fwd``): the same launches, the same bits, but nothing is kept and ``bwd`` is None"""
    w1, b1 = _plain(fc1)
    a = ops.linear(xn, w1, b1, flags=H.GEMM_OUT_F32)                # stored pre-activations, fp32 [M, hidden]: rounded once, after the GELU
    out = fc2(ops.gelu(a), residual=residual)
    if not tape:
        return out, None

    def bwd(d_out):
        d_a = ops.gelu_bwd(a, linear_bwd(fc2, d_out))
        return linear_bwd(fc1, d_a)
    return out, bwd


def vit_block_fwd(blk, x: torch.Tensor, B: int, tape: bool = True):
    """_VitBlock (pre-LN, eps 1e-6) on bf16 rows x [B * N, C]; bwd(d_out) -> d_x"""
    M, Cc = x.shape
    N = M // B
    at = blk.attn
    scale = (Cc // at.heads) ** -0.5
    n1 = ops.layer_norm(x, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
    qkv = at.qkv(n1).reshape(B, N, 3 * Cc)
    q, k, v = qkv[..., :Cc], qkv[..., Cc:2 * Cc], qkv[..., 2 * Cc:]
    o = ops.masked_attention(q, k, v, at.heads, scale)
    x1 = at.proj(o.reshape(M, Cc), residual=x)
    n2 = ops.layer_norm(x1, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
    x2, mlp_bwd = mlp_fwd(blk.mlp.fc1, blk.mlp.fc2, n2, x1, tape)
    del n1, n2, o
    if not tape:
        return x2, None

    def bwd(d_x2):
        d_x1 = ops.layer_norm_bwd(x1, mlp_bwd(d_x2), blk.norm2.weight, blk.norm2.eps, add=d_x2)
        d_o = linear_bwd(at.proj, d_x1).reshape(B, N, Cc)
        d_qkv = torch.empty_like(qkv)
        ops.masked_attention_bwd(q, k, v, d_o, at.heads, scale, dq=d_qkv[..., :Cc], dk=d_qkv[..., Cc:2 * Cc], dv=d_qkv[..., 2 * Cc:])
        d_n1 = linear_bwd(at.qkv, d_qkv.reshape(M, 3 * Cc))
        return ops.layer_norm_bwd(x, d_n1, blk.norm1.weight, blk.norm1.eps, add=d_x1)
    return x2, bwd


def encoder_fwd(enc, img: torch.Tensor, tape: bool = True):
    """Encoder (the ViT) on img fp32 [B, 3, H, W] -> (memory bf16 [B, N, C], bwd(d_memory [B, N, C]) -> d_img fp32 [B, 3, H, W])"""
    B, Cin, Hh, Ww = img.shape
    pe = enc.patch_embed
    ph, pw = pe.patch_size
    x = pe(img)
    x = (x.float() + enc.pos_embed).to(torch.bfloat16)              # (an addition of a constant: the gradient passes through)
    _, N, Cc = x.shape
    x = x.reshape(B * N, Cc)
    bwds: List[Bwd] = []
    for blk in enc.blocks:
        x, b = vit_block_fwd(blk, x, B, tape)
        bwds.append(b)
    memory = ops.layer_norm(x, enc.norm.weight, enc.norm.bias, enc.norm.eps).reshape(B, N, Cc)
    if not tape:
        return memory, None
    x_last = x

    def bwd(d_memory):
        d = ops.layer_norm_bwd(x_last, d_memory.reshape(B * N, Cc).contiguous(), enc.norm.weight, enc.norm.eps)
        for b in reversed(bwds):
            d = b(d)
        # backward-data of the patch embedding: d cols = d tokens . W (fp32 out), then the un-patchify
        K = Cin * ph * pw
        wt = H.layout(pe, "wT", lambda: packing.pack_linear(pe.proj.weight.detach().reshape(Cc, K).t().contiguous()))
        d_cols = ops.linear(d, wt, None, flags=H.GEMM_OUT_F32)[:, :K]
        return d_cols.reshape(B, Hh // ph, Ww // pw, Cin, ph, pw).permute(0, 3, 1, 4, 2, 5).reshape(B, Cin, Hh, Ww).contiguous()
    return memory, bwd


def refine_fwd(parseq, memory: torch.Tensor, tgt_in: torch.Tensor, tape: bool = True):
    """one teacher-forced refinement pass of PARSeq on tokens tgt_in [N, L] (masks and key padding as PARSeq.forward's refinement)
    -> (logits fp32 [N, L, n_cls], bwd(d_logits fp32 [N, L, n_cls]) -> d_memory bf16 [N, Lm, C])"""
    check_supported(parseq)
    dev = memory.device
    N, Lt = tgt_in.shape
    Lm, Cc = memory.shape[1], memory.shape[2]
    layer = parseq.decoder.layers[0]
    ca = layer.cross_attn
    n_cls = len(parseq.tokenizer) - 2
    tgt_mask = torch.triu(torch.full((Lt, Lt), float("-inf"), device=dev), 1)
    query_mask = tgt_mask.clone()
    query_mask[torch.triu(torch.ones(Lt, Lt, dtype=torch.bool, device=dev), 2)] = 0
    kpm = (tgt_in == parseq.eos_id).int().cumsum(-1) > 0
    # ---- constant with respect to the image: the embeddings, the query stream's self-attention, the cross-attention's queries
    null_ctx = parseq.text_embed(tgt_in[:, :1])
    content = torch.cat([null_ctx, parseq.pos_queries[:, :Lt - 1] + parseq.text_embed(tgt_in[:, 1:])], dim=1).to(torch.bfloat16).contiguous()
    query = parseq.pos_queries[:, :Lt].expand(N, -1, -1).to(torch.bfloat16).contiguous()
    tgt = layer.self_attn(layer.norm_q(query), kv=layer.norm_c(content), attn_mask=query_mask, key_padding_mask=kpm, residual=query)
    wq, bq, _, _ = ca.packed()
    M = N * Lt
    q = ops.linear(layer.norm1(tgt).reshape(M, Cc), wq, bq).reshape(N, Lt, Cc)
    # ---- the differentiated part
    scale = (Cc // ca.heads) ** -0.5
    kv = ca.project_kv(memory)                                      # [N, Lm, 2C]
    k, v = kv[..., :Cc], kv[..., Cc:]
    o = ops.masked_attention(q, k, v, ca.heads, scale)
    t2 = ca.out_proj(o.reshape(M, Cc), residual=tgt.reshape(M, Cc))
    n2 = ops.layer_norm(t2, layer.norm2.weight, layer.norm2.bias, layer.norm2.eps)
    t3, mlp_bwd = mlp_fwd(layer.linear1, layer.linear2, n2, t2, tape)
    dn = parseq.decoder.norm
    out = ops.layer_norm(t3, dn.weight, dn.bias, dn.eps)
    logits = parseq.head(out, flags=H.GEMM_OUT_F32)[:, :n_cls].reshape(N, Lt, n_cls)
    del n2, o, out
    if not tape:
        return logits, None

    def bwd(d_logits):
        head = parseq.head
        wt = H.layout(head, "wT", lambda: packing.pack_linear(head.weight.detach().t().contiguous()))     # [C, n_cls padded to 64]
        dl = torch.zeros((M, wt.shape[1]), dtype=torch.bfloat16, device=dev)
        dl[:, :n_cls] = d_logits.reshape(M, n_cls)
        d_t3 = ops.layer_norm_bwd(t3, ops.linear(dl, wt, None), dn.weight, dn.eps)
        d_t2 = ops.layer_norm_bwd(t2, mlp_bwd(d_t3), layer.norm2.weight, layer.norm2.eps, add=d_t3)
        d_o = linear_bwd(ca.out_proj, d_t2).reshape(N, Lt, Cc)
        d_kv = torch.empty_like(kv)
        ops.masked_attention_bwd(q, k, v, d_o, ca.heads, scale, want_dq=False, dk=d_kv[..., :Cc], dv=d_kv[..., Cc:])
        wkv_t = H.layout(ca, "wkvT", lambda: packing.pack_linear(ca.in_proj_weight.detach()[Cc:].t().contiguous()))
        return ops.linear(d_kv.reshape(N * Lm, 2 * Cc), wkv_t, None).reshape(N, Lm, Cc)
    return logits, bwd


class RefineTape:
    """the reversible teacher-forced pass: ``backward(d_logits fp32 [N, L, n_cls]) -> d_images fp32 [N, 3, h, w]``"""

    def __init__(self, enc_bwd: Bwd, dec_bwd: Bwd):
        self._enc_bwd, self._dec_bwd = enc_bwd, dec_bwd

    def backward(self, d_logits: torch.Tensor) -> torch.Tensor:
        return self._enc_bwd(self._dec_bwd(d_logits.float().contiguous()))
