"""One training step of the text cross-attention on the HIP path (second half).

Reference: ``DiffusionEngine.forward / shared_step / training_step / configure_optimizers`` (sgm/models/diffusion.py:138-172,202-222)
with ``FullLoss.__call__`` (sgm/modules/diffusionmodules/loss.py:131-176): noise the latent at a sampled sigma, run the denoiser,

    loss = mean_b mean(w (D(x + n sigma) - x)^2)  +  lambda_local_loss * mean_b get_local_loss(t_attn maps, seg, seg_mask),

back-propagate to the parameters whose names contain an ``opt_keys`` entry (configs/train/textdesign_sd_2.yaml:4-6: ``t_attn``,
``t_norm`` — 75.9 M of the UNet's 866 M), average the gradients over the data-parallel ranks, AdamW step, lr = base * 0.95^epoch.

Here: the tape-mode forward and the written-out reverse pass of ``udifftext_amd.backward`` (dX through every layer, dW only where
the reference trains), the two loss seeds and the optimiser update as HIP kernels (csrc/backward.hip), one flat fp32 bucket per step
through ``torch.distributed`` (RCCL on the GPUs: reduce-scatter + all-gather, the bandwidth-optimal form on the xGMI mesh; gloo's
all_reduce in the CPU tests).  The OCR loss (ocr_enabled; False in every shipped config) runs through the VAE decoder's reverse pass
(udifftext_amd.vae_backward).  The style loss (style_enabled) cannot be built — the reference calls
``get_style_local_loss``, which it never defines — and the Lightning loop itself stays out of scope.

Gradient accumulation and EMA (configs/train.yaml:21 ``accumulate_grad_batches``; diffusion.py:75-78,178-195 with sgm/modules/ema.py)
run on the fused route: the trained tensors' gradients live in ONE persistent flat bucket (``GradBucket``), the reverse pass ADDS into
its views (udt_*_acc), the collectives run on it in place, and ONE launch (udt_bucket_update_f32) takes the AdamW step over all 112
tensors and moves the EMA shadows (``BucketAdamW``, ``Ema``).  ``window_step`` is Lightning's order for a window of N micro-batches:
backward; on the N-th the optimiser step with grad_scale = 1 / (N * world); then, after EVERY micro-batch, on_train_batch_end — the
EMA update, which therefore counts num_updates per micro-batch, not per optimiser step (diffusion.py:178-180).  The per-tensor
``AdamW`` + ``allreduce_gradients`` route stays what configure_optimizers returns by default.

The denoiser is the engine's: c_in, c_noise, c_skip, c_out per sample from ``precond_coefs`` (EpsScaling, VScaling,
EDMScaling under DiscreteDenoiser or the continuous Denoiser), w from ``denoiser.w``, the sigmas from ``loss_fn.sigma_sampler``
(DiscreteSampling or EDMSampling).  DiscreteDenoiser + EpsScaling + EpsWeighting keeps its own seed kernel (udt_diff_loss_grad);
every other pair seeds the reverse pass with udt_precond_loss_grad.  What is not built raises (``check_trainable``).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from . import backward, lib as L, ops, rng


# ------------------------------------------------------------------------------------------------ the loss and its gradients
def check_trainable(engine) -> None:
    """raise NotImplementedError for the parts of FullLoss.__call__ / DiffusionEngine.forward this path does not compute, instead of
    computing something else"""
    from sgm.modules.diffusionmodules.sigma_sampling import DiscreteSampling, EDMSampling
    loss_fn = engine.loss_fn
    if loss_fn.type != "l2":
        raise NotImplementedError(f"loss type {loss_fn.type!r}: the loss seed kernels implement the l2 loss")
    if loss_fn.offset_noise_level > 0:
        raise NotImplementedError("offset_noise_level > 0 is not implemented")
    if loss_fn.style_enabled:
        raise NotImplementedError("the style loss (style_enabled) is not implemented: the reference's FullLoss.__call__ calls "
                                  "get_style_local_loss, which the reference has no definition of")
    if loss_fn.ocr_enabled and getattr(loss_fn, "predictor", None) is None:
        raise NotImplementedError("ocr_enabled without an OCR predictor: construct FullLoss with a predictor_config")
    if type(loss_fn.sigma_sampler) not in (DiscreteSampling, EDMSampling):
        raise NotImplementedError(f"sigma sampler {type(loss_fn.sigma_sampler).__name__}: DiscreteSampling and EDMSampling are implemented")
    conditioner = getattr(engine, "conditioner", None)
    if any(getattr(e, "is_trainable", False) for e in getattr(conditioner, "embedders", ())):
        raise NotImplementedError("a trainable conditioner embedder: the reverse pass ends at the UNet's inputs")


def _eps_path(engine) -> bool:
    """DiscreteDenoiser + EpsScaling + EpsWeighting: the path of udt_diff_loss_grad (sigma^-2 weighting in the kernel)"""
    from sgm.modules.diffusionmodules.denoiser import DiscreteDenoiser
    from sgm.modules.diffusionmodules.denoiser_scaling import EpsScaling
    from sgm.modules.diffusionmodules.denoiser_weighting import EpsWeighting
    den = engine.denoiser
    return type(den) is DiscreteDenoiser and type(den.scaling) is EpsScaling and type(den.weighting) is EpsWeighting


def training_loss_and_grads(engine, z: torch.Tensor, cond: dict, seg: torch.Tensor, seg_mask: torch.Tensor,
                            sigma_idx: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                            want_grads: bool = True, sigma: Optional[torch.Tensor] = None, bucket: Optional["GradBucket"] = None,
                            r_bbox=None, label=None, first_stage_model=None, scaler: Optional[float] = None):
    """FullLoss.__call__ on latents z fp32 [B, 4, h, w] with conditioning ``cond`` ({"concat": [B, 5, h, w], "t_crossattn":
    [B, L, Dc]}), character segment maps seg fp32 [B, seg_l, Hs, Ws] and seg_mask [B, seg_l].
    sigma_idx int64 [B] (default: DiscreteSampling's torch.randint draw; EDMSampling: one CPU torch.randn((B,))), or ``sigma``
    fp32 [B] (continuous sigmas, instead of a draw), and noise [B, 4, h, w] (default: one CPU-generator randn, rng.randn_on) are
    the step's random draws.  Returns (loss_dict, grads): loss_dict as the reference's (``loss/diff_loss``,
    ``loss/local_loss``, ``loss/full_loss``: 0-dim fp32 tensors), grads = {state-dict name: fp32 gradient of loss/full_loss} for the
    t_attn / t_norm parameters (None when want_grads is False).  ``bucket``: a GradBucket the gradients are ADDED to instead (one
    micro-batch of an accumulation window); grads is then the bucket.
    With ``loss_fn.ocr_enabled`` (reference loss.py:159-166): r_bbox (per image (top, bottom, left, right), on the host) and label (B
    strings) are required; first_stage_model / scaler default to the engine's.  The denoiser's output D = c_skip noised + c_out F
    is materialised in fp32, ``loss_fn.get_ocr_loss`` runs with weight lambda_ocr_loss / B, and c_out[b] * d_D is added into the
    loss seed before the reverse pass; the loss dict gains ``loss/ocr_loss`` and full_loss lambda_ocr_loss * ocr_loss."""
    loss_fn = engine.loss_fn
    ocr = bool(loss_fn.ocr_enabled)
    if ocr and (r_bbox is None or label is None):
        raise ValueError("ocr_enabled: training_loss_and_grads needs r_bbox and label (batch['r_bbox'], batch['label'])")
    B = z.shape[0]
    dev = z.device
    tape, noised, sigma = training_tape(engine, z, cond, sigma_idx, noise, sigma)
    z = z.float().contiguous()
    if tape.precond is None:
        loss_diff, d_eps = ops.diff_loss_grad(tape.eps, noised, z, sigma)
    else:
        loss_diff, d_eps = ops.precond_loss_grad(tape.eps, noised, z, *tape.precond)
    used = [it for it in tape.maps if loss_fn.scores_map(it["hw"])]
    lam = float(loss_fn.lambda_local_loss)
    loss_local = torch.zeros((B,), dtype=torch.float32, device=dev)
    if used:
        segf, segm = seg.float().contiguous(), seg_mask.float().contiguous()
        gk = loss_fn.g_kernel[0, 0].reshape(9).float().contiguous()
        for it in used:
            it["d_probs"] = torch.zeros_like(it["attn_map"])
            ops.local_loss_seg_bwd_hw(it["attn_map"], segf, segm, gk, it["d_probs"], loss_local, it["heads"], it["hw"],
                                      lam / (len(used) * B))
    diff = loss_diff.mean()
    local = loss_local.mean() / max(len(used), 1)
    loss_dict = {"loss/diff_loss": diff, "loss/local_loss": local, "loss/full_loss": diff + lam * local}
    if ocr:
        lam_ocr = float(loss_fn.lambda_ocr_loss)
        if tape.precond is None:                                         # eps path: D = noised - sigma eps
            c_skip, c_out = torch.ones_like(sigma), -sigma
        else:
            c_skip, c_out = tape.precond[0], tape.precond[1]
        den = ops.denoised(tape.eps, noised, c_skip, c_out)
        fsm = first_stage_model if first_stage_model is not None else engine.first_stage_model
        sc = float(scaler if scaler is not None else engine.scale_factor)
        loss_ocr, d_den = loss_fn.get_ocr_loss(den, r_bbox, label, fsm, sc, want_grad=want_grads, weight=lam_ocr / B)
        if d_den is not None:
            ops.seed_add_(d_eps, d_den.contiguous(), c_out.contiguous())
        ocr_mean = loss_ocr.mean()
        loss_dict["loss/ocr_loss"] = ocr_mean
        loss_dict["loss/full_loss"] = loss_dict["loss/full_loss"] + lam_ocr * ocr_mean
    if not want_grads:
        return loss_dict, None
    if bucket is not None:
        tape.backward(d_eps, param_grads=bucket)
        return loss_dict, bucket
    grads: Dict[str, torch.Tensor] = {}
    tape.backward(d_eps, param_grads=grads)
    return loss_dict, grads


def training_tape(engine, z: torch.Tensor, cond: dict, sigma_idx: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                  sigma: Optional[torch.Tensor] = None):
    """the training forward: noise z at the sampled sigmas, the denoiser's input scaling and timestep input, tape-mode UNet with
    its output head.  Returns (tape, noised fp32 [B, 4, h, w], sigma fp32 [B]); ``tape.precond`` is None on the eps path, else the
    device fp32 [B] triple (c_skip, c_out, w) of udt_precond_loss_grad"""
    from sgm.modules.diffusionmodules.openaimodel import CPAD
    from sgm.modules.diffusionmodules.sampling import precond_coefs
    from sgm.modules.diffusionmodules.sigma_sampling import DiscreteSampling
    check_trainable(engine)
    dev = z.device
    B, _, h, w = z.shape
    den = engine.denoiser
    unet = engine.model.diffusion_model
    sampler = engine.loss_fn.sigma_sampler
    eps_path = _eps_path(engine)
    den_table = getattr(den, "sigmas", None)
    if sigma is not None:
        if sigma_idx is not None:
            raise ValueError("give sigma_idx or sigma, not both")
        sigma = sigma.to(dev).float().contiguous()
    elif sigma_idx is not None or type(sampler) is DiscreteSampling:
        table = (den_table if den_table is not None else sampler.sigmas).to(dev).float()
        if sigma_idx is None:
            sigma_idx = torch.randint(0, table.numel(), (B,))           # DiscreteSampling.__call__ (CPU draw, reference order)
        sigma_idx = sigma_idx.to(dev).long()
        sigma = table[sigma_idx].contiguous()                            # (the sampled sigmas lie on the denoiser's table)
    else:
        sigma = sampler(B).to(dev).float().contiguous()                  # EDMSampling: one CPU torch.randn((B,)), same generator
    if noise is None:
        noise = rng.randn_on((B, 4, h, w), dev)
    z = z.float().contiguous()
    noised = z.clone()
    sig_host = [float(s) for s in sigma.cpu()]
    for b in range(B):                                                   # noised = z + n sigma_b
        ops.axpy_(noised[b], noise[b].float().contiguous(), sig_host[b])
    if eps_path and sigma_idx is not None:
        c_in = [1.0 / (s ** 2 + 1.0) ** 0.5 for s in sig_host]
        c_noise = sigma_idx.float()
        precond = None
    else:
        host_table = den_table.detach().float().cpu() if den_table is not None else None
        ks = [precond_coefs(den, s, host_table) for s in sig_host]
        c_in = [k.c_in for k in ks]
        c_noise = torch.tensor([k.c_noise for k in ks], dtype=torch.float32, device=dev)
        wgt = den.w(torch.tensor(sig_host, dtype=torch.float64))
        mk = lambda v: torch.as_tensor(v, dtype=torch.float64).float().to(dev).contiguous()
        precond = (mk([k.c_skip for k in ks]), mk([k.c_out for k in ks]), mk(wgt))
    scaled = noised.clone()
    for b in range(B):                                                   # network input = noised * c_in(sigma_b)
        ops.axpy_(scaled[b], scaled[b], c_in[b] - 1.0)
    xin = ops.nchw_to_nhwc(torch.cat((scaled, cond["concat"].float()), dim=1).contiguous(), CPAD)
    tape = backward.UNetTape(unet, xin, c_noise, cond["t_crossattn"], with_head=True)
    tape.precond = precond
    return tape, noised, sigma


def trainable_parameters(engine, opt_keys: Optional[List[str]] = None) -> List[Tuple[str, torch.nn.Parameter]]:
    """the (state-dict name, parameter) pairs DiffusionEngine.configure_optimizers selects (diffusion.py:204-217): names under
    ``model.`` that contain an opt_keys entry, in module order"""
    keys = opt_keys if opt_keys is not None else (engine.opt_keys or [])
    return [("model." + n, p) for n, p in engine.model.named_parameters() if any(k in n for k in keys)]


# ------------------------------------------------------------------------------------------------ data-parallel gradient average
def allreduce_gradients(grads: Dict[str, torch.Tensor], names: List[str], dist=None, force: bool = False) -> None:
    """average the gradients over the ranks, in place: ONE flat fp32 bucket in the order ``names`` (the same on every rank).  On RCCL:
    reduce-scatter + all-gather of the padded bucket — on the xGMI full mesh both are direct peer exchanges, 2 (N - 1) / N of the
    bucket per GPU; with gloo (CPU tests): all_reduce."""
    if dist is None or not dist.is_initialized() or (dist.get_world_size() == 1 and not force):
        return                                                           # (force: run the collectives in a world of one — tests)
    world = dist.get_world_size()
    flat = torch.cat([grads[n].reshape(-1) for n in names])
    n = flat.numel()
    if dist.get_backend() == "nccl":
        pad = (-n) % world
        if pad:
            flat = torch.cat([flat, flat.new_zeros(pad)])
        shard = torch.empty((flat.numel() // world,), dtype=flat.dtype, device=flat.device)
        dist.reduce_scatter_tensor(shard, flat, op=dist.ReduceOp.SUM)
        dist.all_gather_into_tensor(flat, shard)
    else:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM)
    o = 0
    for nm in names:
        g = grads[nm]
        g.copy_(flat[o:o + g.numel()].reshape(g.shape))
        o += g.numel()
        if g.is_cuda:
            ops.axpy_(g.reshape(-1), g.reshape(-1), 1.0 / world - 1.0)     # g *= 1 / world
        else:
            g.mul_(1.0 / world)                                          # (CPU tests: no HIP kernels)


# ------------------------------------------------------------------------------------------------ optimiser
class AdamW:
    """torch.optim.AdamW (the reference's default optimiser, diffusion.py:49-51) over named fp32 parameters, stepped by udt_adamw_f32;
    ``set_epoch`` applies configure_optimizers' LambdaLR (lr = base * 0.95^epoch, diffusion.py:220)"""

    def __init__(self, named_params: List[Tuple[str, torch.nn.Parameter]], lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2):
        self.named = list(named_params)
        self.base_lr, self.lr, self.betas, self.eps, self.weight_decay = lr, lr, betas, eps, weight_decay
        self.step_count = 0
        self.state = {n: (torch.zeros_like(p.data, dtype=torch.float32), torch.zeros_like(p.data, dtype=torch.float32)) for n, p in self.named}

    def set_epoch(self, epoch: int) -> None:
        self.lr = self.base_lr * 0.95 ** epoch

    def step(self, grads: Dict[str, torch.Tensor], grad_scale: float = 1.0) -> None:
        self.step_count += 1
        for n, p in self.named:
            m, v = self.state[n]
            ops.adamw_(p, grads[n].contiguous(), m, v, self.step_count, self.lr, self.betas, self.eps, self.weight_decay, grad_scale)


def training_step(engine, optimizer, z: torch.Tensor, cond: dict, seg: torch.Tensor, seg_mask: torch.Tensor, dist=None,
                  sigma_idx: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                  sigma: Optional[torch.Tensor] = None) -> dict:
    """loss + gradients + rank average + AdamW update of the t_attn / t_norm parameters; returns the loss dict.  With a BucketAdamW:
    one micro-batch of its accumulation window (``window_step``), EMA included when the engine keeps one"""
    if isinstance(optimizer, BucketAdamW):
        run = lambda bucket: training_loss_and_grads(engine, z, cond, seg, seg_mask, sigma_idx=sigma_idx, noise=noise, sigma=sigma,
                                                     bucket=bucket)[0]
        return window_step(optimizer, run, dist, ema=engine_ema(engine))
    loss_dict, grads = training_loss_and_grads(engine, z, cond, seg, seg_mask, sigma_idx=sigma_idx, noise=noise, sigma=sigma)
    names = [n for n, _ in optimizer.named]
    allreduce_gradients(grads, names, dist)
    optimizer.step(grads)
    ema = engine_ema(engine)
    if ema is not None:                                                  # on_train_batch_end (diffusion.py:178-180): the EMA-only launch
        ema.update()
    return loss_dict


# ------------------------------------------------------------------------------------------------ the gradient bucket
BUCKET_ALIGN = 4                  # floats: every view starts 16-byte aligned in the flat buffer (udt_bucket_segment.offset)
BUCKET_PAD = 64                   # floats: the flat buffer's length divides by every world size up to 64 (reduce-scatter shards)


def bucket_layout(named_params) -> Tuple[Dict[str, int], int]:
    """({state-dict name: offset in floats}, total floats) of a flat buffer holding one view per tensor, in the order given"""
    offsets, o = {}, 0
    for n, p in named_params:
        offsets[n] = o
        o += (p.numel() + BUCKET_ALIGN - 1) // BUCKET_ALIGN * BUCKET_ALIGN
    return offsets, max(BUCKET_PAD, (o + BUCKET_PAD - 1) // BUCKET_PAD * BUCKET_PAD)


class GradBucket:
    """ONE persistent flat fp32 buffer with a view per trained tensor (``views[name]``, the tensor's shape), in ``trainable_parameters``
    order: the reverse pass accumulates into the views (UNetTape.backward(param_grads=bucket)), ``average`` runs the collectives on
    the buffer itself, udt_bucket_update_f32 consumes it.  A window of micro-batches starts from ``zero_()``."""

    def __init__(self, named_params, device=None):
        named_params = list(named_params)
        self.names = [n for n, _ in named_params]
        self.offsets, self.total = bucket_layout(named_params)
        dev = device if device is not None else named_params[0][1].device
        self.flat = torch.zeros((self.total,), dtype=torch.float32, device=dev)
        self.views = {n: self.flat[self.offsets[n]:self.offsets[n] + p.numel()].view(p.shape) for n, p in named_params}

    def zero_(self) -> "GradBucket":
        self.flat.zero_()
        return self

    def average(self, dist=None, force: bool = False) -> None:
        """SUM the bucket over the ranks, in place — no concatenation, no copy back, and no scaling: the 1 / world factor is the update's
        grad_scale.  RCCL: reduce-scatter into this rank's shard of the buffer + all-gather from it (both in place; 2 (N - 1) / N of
        the bucket per GPU on the xGMI mesh); gloo: all_reduce.  (force: run the collectives in a world of one — tests)"""
        if dist is None or not dist.is_initialized() or (dist.get_world_size() == 1 and not force):
            return
        world = dist.get_world_size()
        if dist.get_backend() == "nccl" and self.total % world == 0:
            n = self.total // world
            shard = self.flat[dist.get_rank() * n:(dist.get_rank() + 1) * n]
            dist.reduce_scatter_tensor(shard, self.flat, op=dist.ReduceOp.SUM)
            dist.all_gather_into_tensor(self.flat, shard)
        else:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM)


class _Segments:
    """the device tables of udt_bucket_update_f32 / udt_bucket_swap_f32 for a list of tensors: the segment table (parameter, shadow,
    offset, length) and the chunk map; rebuilt when any data_ptr changed (a module moved, a state dict replaced a tensor)"""

    def __init__(self, named_params, offsets: Dict[str, int]):
        self.named = list(named_params)
        self.offsets = offsets
        self._key = None
        self._tables = None

    def tables(self, shadows: Optional[List[torch.Tensor]] = None):
        params = [p for _, p in self.named]
        key = tuple(p.data_ptr() for p in params) + tuple(t.data_ptr() for t in (shadows or ()))
        if key != self._key:
            dev = params[0].device
            for t in params + list(shadows or ()):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise ValueError("the fused optimiser step takes contiguous fp32 tensors on one device")
            if shadows is not None and [t.numel() for t in shadows] != [p.numel() for p in params]:
                raise ValueError("EMA shadows do not match the trained tensors")
            arr = (L.BucketSegment * len(params))()
            seg_ids, chunk_ids = [], []
            for i, (n, p) in enumerate(self.named):
                arr[i].p, arr[i].shadow = p.data_ptr(), (shadows[i].data_ptr() if shadows is not None else None)
                arr[i].offset, arr[i].n = self.offsets[n], p.numel()
                k = (p.numel() + L.BUCKET_CHUNK - 1) // L.BUCKET_CHUNK
                seg_ids.append(torch.full((k,), i, dtype=torch.int32))
                chunk_ids.append(torch.arange(k, dtype=torch.int32))
            seg = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            cmap = torch.stack([torch.cat(seg_ids), torch.cat(chunk_ids)], dim=1).contiguous().to(dev)
            self._key, self._tables = key, (seg, cmap)
        return self._tables

    def bump_versions(self) -> None:
        # host only, no launch: packed layouts and captured graphs notice.  ONE call on the list: handed a single 2-D tensor the
        # function walks its rows (2.6 ms for a 1280 x 1280 weight, 30 ms of host time over the 112 tensors)
        torch._C._increment_version([p for _, p in self.named])


# ------------------------------------------------------------------------------------------------ EMA
class Ema(nn.Module):
    """LitEma (sgm/modules/ema.py) over the trained tensors: one fp32 buffer per tensor, named as LitEma names it (the name below
    ``model.`` with the dots removed), plus ``decay`` and ``num_updates`` — under the engine's ``model_ema.`` prefix the reference's keys.
    Tensors that are not trained keep no shadow: LitEma moves only tensors that require a gradient (ema.py:46-52), and asserts that
    the others have none (:53-54); a checkpoint that also carries shadows of the model's untrained tensors (``untrained_names``) loads
    with those ignored, any other unknown ``model_ema.*`` key is reported as unexpected.  ``update`` is
    LitEma.forward: decay = min(decay, (1 + n) / (10 + n)) (ema.py:36-38, in fp32 as there), shadow -= (1 - decay) (shadow - p) in
    ONE launch (udt_bucket_update_f32, EMA mode; BucketAdamW.step fuses it with the optimiser step).  ``store`` / ``copy_to`` /
    ``restore`` are ema_scope's calls (diffusion.py:182-195) on udt_bucket_swap_f32: parameters and shadows trade places and trade
    back, no copy of the 304 MB is kept — so ``store`` must be followed by ``copy_to`` before the parameters change."""

    def __init__(self, named_params, decay: float = 0.9999, use_num_updates: bool = True, prefix: str = "model.",
                 untrained_names=()):
        """``untrained_names``: names (as ``named_params``') of the model's other parameters — the shadows a LitEma built over the
        whole model would also hold; a state dict may carry them, they are not kept.  Any OTHER unknown key stays unexpected."""
        super().__init__()
        if decay < 0.0 or decay > 1.0:
            raise ValueError("Decay must be between 0 and 1")
        named_params = list(named_params)
        self.m_name2s_name: Dict[str, str] = {}
        self.register_buffer("decay", torch.tensor(decay, dtype=torch.float32))
        self.register_buffer("num_updates", torch.tensor(0 if use_num_updates else -1, dtype=torch.int))
        for n, p in named_params:
            rel = n[len(prefix):] if n.startswith(prefix) else n
            s_name = rel.replace(".", "")
            self.m_name2s_name[rel] = s_name
            self.register_buffer(s_name, p.detach().clone().float())
        self._s_names = [self.m_name2s_name[n[len(prefix):] if n.startswith(prefix) else n] for n, _ in named_params]
        self.names = [n for n, _ in named_params]                        # the trained tensors, in the bucket's order
        self._ignorable = {(n[len(prefix):] if n.startswith(prefix) else n).replace(".", "") for n in untrained_names}
        self._stored_versions: Optional[List[int]] = None
        self._segments = _Segments(named_params, bucket_layout(named_params)[0])
        self._host: Optional[Tuple[float, int]] = None                   # (decay, num_updates) mirrored on the host: no sync per update
        self._stored = self._swapped = False

    # -- state
    def shadows(self) -> List[torch.Tensor]:
        return [getattr(self, s) for s in self._s_names]

    def _apply(self, fn, *a, **k):
        self._host = None
        return super()._apply(fn, *a, **k)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        self._host = None
        before = len(unexpected_keys)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)
        # shadows of the model's tensors that are not trained (a LitEma built while every parameter required a gradient): never moved,
        # not kept.  A key that names neither a trained nor an untrained tensor of the model stays unexpected (strict loads fail on it).
        unexpected_keys[before:] = [k for k in unexpected_keys[before:]
                                    if not (k.startswith(prefix) and k[len(prefix):] in self._ignorable)]

    def reset_num_updates(self) -> None:
        self.num_updates.zero_()
        self._host = None

    def next_one_minus_decay(self) -> float:
        """count one update and return its 1 - decay, in LitEma's fp32 arithmetic (ema.py:34-40)"""
        if self._host is None:
            self._host = (float(self.decay), int(self.num_updates))
        decay, n = self._host
        d = torch.tensor(decay, dtype=torch.float32)
        if n >= 0:
            n += 1
            self.num_updates += 1
            d = torch.minimum(d, (1 + torch.tensor(n, dtype=torch.int)) / (10 + torch.tensor(n, dtype=torch.int)))
        self._host = (decay, n)
        return float(1.0 - d)

    # -- the launches
    def tables(self):
        return self._segments.tables(self.shadows())

    def _launch_update(self, one_minus_decay: float) -> None:
        seg, cmap = self.tables()
        ops.bucket_update_(seg, cmap, None, None, None, L.BUCKET_EMA, one_minus_decay=one_minus_decay)

    def _launch_swap(self) -> None:
        seg, cmap = self.tables()
        ops.bucket_swap_(seg, cmap)
        self._segments.bump_versions()

    def update(self, model=None) -> None:
        """LitEma.forward (the engine's on_train_batch_end): the shadows follow the parameters"""
        if self._swapped:
            raise RuntimeError("EMA update inside ema_scope: the parameters hold the shadows")
        self._launch_update(self.next_one_minus_decay())

    forward = update

    def store(self, parameters=None) -> None:
        """mark the parameters as stored: ``copy_to`` then keeps them in the shadow slots (the swap).  Nothing is copied, so the
        parameters must not change between ``store`` and ``copy_to`` — ``copy_to`` checks their versions and refuses otherwise"""
        self._stored = True
        self._stored_versions = [p._version for _, p in self._segments.named]

    def copy_to(self, model=None) -> None:
        """parameters <- shadows.  After ``store()``: by the swap (the shadow slots keep the training weights until ``restore``);
        without it the training weights are overwritten, as LitEma.copy_to does"""
        if self._swapped:
            return
        if self._stored:
            if self._stored_versions != [p._version for _, p in self._segments.named]:
                raise RuntimeError("the parameters changed between Ema.store() and copy_to(): store() keeps no copy (use ema_scope)")
            self._launch_swap()
            self._swapped = True
            return
        with torch.no_grad():
            for (_, p), sh in zip(self._segments.named, self.shadows()):
                p.copy_(sh)                                               # (bumps p's version, as the swap does)

    def restore(self, parameters=None) -> None:
        if self._swapped:
            self._launch_swap()
        self._stored = self._swapped = False
        self._stored_versions = None


def engine_ema(engine) -> Optional[Ema]:
    return getattr(engine, "model_ema", None) if getattr(engine, "use_ema", False) else None


# ------------------------------------------------------------------------------------------------ the fused optimiser
class BucketAdamW:
    """``AdamW`` on the fused route: the same hyper-parameters and ``set_epoch``, the moments m / v flat in the bucket's layout, and
    ``step`` ONE launch of udt_bucket_update_f32 over all trained tensors (with ``ema``: the shadows move in the same launch, after
    the step, as on_train_batch_end follows optimizer.step()).  ``accumulate_grad_batches`` = N is the window ``window_step`` keeps."""

    def __init__(self, named_params: List[Tuple[str, torch.nn.Parameter]], lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, accumulate_grad_batches: int = 1, device=None):
        if accumulate_grad_batches < 1:
            raise ValueError("accumulate_grad_batches must be >= 1")
        self.named = list(named_params)
        self.base_lr, self.lr, self.betas, self.eps, self.weight_decay = lr, lr, betas, eps, weight_decay
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        self.step_count = 0
        self.micro_batches = 0
        self.bucket = GradBucket(self.named, device=device)
        self.m = torch.zeros_like(self.bucket.flat)
        self.v = torch.zeros_like(self.bucket.flat)
        self._segments = _Segments(self.named, self.bucket.offsets)

    def set_epoch(self, epoch: int) -> None:
        self.lr = self.base_lr * 0.95 ** epoch

    def _launch(self, bucket: GradBucket, mode: int, grad_scale: float, one_minus_decay: float, ema: Optional[Ema]) -> None:
        seg, cmap = self._segments.tables(ema.shadows() if ema is not None else None)
        ops.bucket_update_(seg, cmap, bucket.flat, self.m, self.v, mode, step=self.step_count, lr=self.lr, betas=self.betas, eps=self.eps,
                           weight_decay=self.weight_decay, grad_scale=grad_scale, one_minus_decay=one_minus_decay)
        self._segments.bump_versions()

    def step(self, bucket: Optional[GradBucket] = None, grad_scale: float = 1.0, ema: Optional[Ema] = None) -> None:
        bucket = self.bucket if bucket is None else bucket
        if bucket.offsets != self.bucket.offsets or bucket.flat.device != self.m.device:
            raise ValueError("the bucket's layout is not this optimiser's")
        if ema is not None and ema._swapped:
            raise RuntimeError("optimiser step inside ema_scope: the parameters hold the shadows")
        self.step_count += 1
        omd = ema.next_one_minus_decay() if ema is not None else 0.0
        self._launch(bucket, L.BUCKET_ADAMW | (L.BUCKET_EMA if ema is not None else 0), grad_scale, omd, ema)


def window_step(optimizer: BucketAdamW, run_micro_batch: Callable[[GradBucket], dict], dist=None, ema: Optional[Ema] = None) -> dict:
    """one micro-batch of an accumulation window, in Lightning's order (configs/train.yaml:21; diffusion.py:151-180):
      1. ``run_micro_batch(bucket)``: the loss, and the reverse pass ADDED to the bucket;
      2. on every N-th call: the rank sum in place, the update with grad_scale = 1 / (N * world), the bucket zeroed;
      3. on EVERY call: on_train_batch_end — the EMA update (per micro-batch, as the reference counts num_updates).
    On the stepping call 2 and 3 are the ONE fused launch; on the others 3 is the kernel's EMA-only mode.  Returns the loss dict."""
    bucket = optimizer.bucket
    loss_dict = run_micro_batch(bucket)
    optimizer.micro_batches += 1
    if optimizer.micro_batches % optimizer.accumulate_grad_batches == 0:
        world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
        bucket.average(dist)
        optimizer.step(bucket, grad_scale=1.0 / (optimizer.accumulate_grad_batches * world), ema=ema)
        bucket.zero_()
    elif ema is not None:
        ema.update()
    return loss_dict
