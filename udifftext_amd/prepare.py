"""Load-time preparation of a ``DiffusionEngine`` (SURVEY.md §8b "Checkpoint contract": internal repacking happens
after load, in a prepare step; §8f rank 3: checkpoint ingestion & weight packing).

``prepare(engine)`` does, once, what the first forward would otherwise do lazily:

* **dedup of the twin VAE** — the reference engine holds two copies of the autoencoder, ``first_stage_model.*`` and
  ``conditioner.embedders.2.model.*``, loaded from the same file (configs/test/textdesign_sd_2.yaml:70,91;
  sgm/models/diffusion.py:87-105).  When every tensor of the two is equal the LatentEncoder is pointed at
  ``first_stage_model``: one set of masters, one set of packed weights (the state dict keeps both prefixes).
* **packing** — every layout the forward pass reads (``hipnn.layout``: bf16 K-contiguous packs, fused q|k|v / k|v / GEGLU
  blocks, the LayerNorm-folded packs, the ``[W_po W_2 | W_po]`` fold, the 22 ``emb_layers`` as one matrix; with UDT_FP8 the
  e4m3 packs too) is built now; modules whose weights are consumed only through a parent's fused pack are skipped.
* **free_masters=True** — then, in one pass, every module that can own layouts is frozen (``hipnn.freeze_layouts``: it
  serves the layouts it has built and raises UdtError for any other) and the fp32 checkpoint-layout parameters of the
  packed modules are released (5.4 GB of the engine's 8.1 GB on the device).  The engine then serves inference only — no
  attend-and-excite, no training: its state dict no longer holds those weights, so reload the checkpoint into a fresh
  engine to change them or the launch path.
"""
from __future__ import annotations

from typing import Dict

import torch


def _same_weights(a: torch.nn.Module, b: torch.nn.Module) -> bool:
    sa, sb = a.state_dict(), b.state_dict()
    if list(sa.keys()) != list(sb.keys()):
        return False
    return all(sa[k].shape == sb[k].shape and sa[k].device == sb[k].device and bool(torch.equal(sa[k], sb[k])) for k in sa)


def prepare(engine, free_masters: bool = False, dedup_vae: bool = True) -> Dict[str, float]:
    """returns a report: {"vae_deduplicated", "packed_modules", "packed_bytes", "freed_bytes"}"""
    from sgm.modules import hipnn as H
    from sgm.modules.encoders.modules import LatentEncoder
    report = {"vae_deduplicated": 0, "packed_modules": 0, "packed_bytes": 0, "freed_bytes": 0}
    with torch.no_grad():
        # ---- twin VAE
        if dedup_vae and getattr(engine, "conditioner", None) is not None:
            for emb in engine.conditioner.embedders:
                if isinstance(emb, LatentEncoder) and emb.model is not engine.first_stage_model \
                        and _same_weights(emb.model, engine.first_stage_model):
                    emb.model = engine.first_stage_model
                    report["vae_deduplicated"] += 1
                    engine._vae_alias_prefixes = ("first_stage_model.", "conditioner.embedders.%d.model." % list(engine.conditioner.embedders).index(emb))
        # ---- pack roots (a fused child is packed through its parent only)
        fused = set()
        for m in engine.modules():
            if isinstance(m, H._Packed):
                fused.update(id(c) for c in m.fused_children())
        unet = engine.model.diffusion_model
        fused.update(id(rb.emb_layers[1]) for rb in unet._resblocks)
        roots = [m for m in engine.modules() if isinstance(m, H._Packed) and id(m) not in fused]
        # where the LayerNorm-folded layouts serve the forward pass (BasicTransformerBlock: fold = LN_GEMM and not fp8), the plain
        # q|k|v and GEGLU layouts of the UNet's blocks are never read: not packed (~270 MB of bf16 for the SD-2 UNet)
        from sgm.modules.attention import BasicTransformerBlock as _BTB
        fold_on = H.LN_GEMM
        ln_only = set()
        if fold_on:
            for m in unet.modules():
                if isinstance(m, _BTB):
                    ln_only.update((id(m.attn1), id(m.ff.net[0])))
            roots = [m for m in roots if id(m) not in ln_only]
        seen = set()
        for m in roots:
            if id(m) in seen:
                continue
            seen.add(id(m))
            report["packed_modules"] += 1
            report["packed_bytes"] += H.nbytes(m.packed())
            if getattr(m, "upsamples", False):          # Upsample.conv: the phase layout of its 3x3 weights
                report["packed_bytes"] += H.nbytes(m.packed_up4())
        report["packed_bytes"] += H.nbytes(unet._emb_pack())
        # ---- LayerNorm-folded layouts of the q|k|v and GEGLU projections (udt_ln_gemm_fwd)
        from sgm.modules.attention import BasicTransformerBlock
        # (in config #5 — UDT_FP8=1 — prepare_ln / prepare_mx8 also build the e4m3 layouts of the blocks whose linears run on MX8
        #  operands: ahead of the release of the masters)
        if H.LN_GEMM:
            from sgm.modules.attention import SpatialTransformer
            for m in unet.modules():
                if isinstance(m, BasicTransformerBlock):
                    report["packed_bytes"] += m.prepare_ln()
                elif isinstance(m, SpatialTransformer):
                    report["packed_bytes"] += m.prepare_mx8()
                    report["packed_bytes"] += m.prepare_ffproj()      # (round 6: [W_po W_2 | W_po], attention.FF_PROJ)
        # ---- freeze every module that can own layouts (it serves what it has built), release the masters of the packed ones
        if free_masters:
            victims = []
            for m in engine.modules():
                if hasattr(m, "_sources"):
                    H.freeze_layouts(m)
                if isinstance(m, H._Packed):
                    victims += list(m.parameters(recurse=False))
                    if hasattr(m, "own_masters"):
                        victims += m.own_masters()
            done = set()
            for p in victims:
                if id(p) in done:
                    continue
                done.add(id(p))
                report["freed_bytes"] += p.numel() * p.element_size()
                p.data = torch.empty(0, dtype=p.dtype, device=p.device)
    return report
