"""Loss objects instantiated by ``loss_fn_config`` (configs/test/textdesign_sd_2.yaml:109-131).

Only what inference touches is implemented (reference sgm/modules/diffusionmodules/loss.py):
``FullLoss.__init__`` (:73-101, builds the sigma sampler and the ``g_kernel`` buffer — a state-dict entry),
``get_gaussian_kernel`` (:103-129) and ``get_min_local_loss`` (:192-235, scores how well the t_attn maps of the
characters land inside the mask; used by the initial-noise search), and the OCR term ``get_ocr_loss`` (:178-190) with its
gradient.  ``FullLoss.__call__`` itself is udifftext_amd.training.training_loss_and_grads.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from udifftext_amd import ops

from ...util import instantiate_from_config


class StandardDiffusionLoss(nn.Module):
    def __init__(self, sigma_sampler_config, type="l2", offset_noise_level=0.0, batch2model_keys=None):
        super().__init__()
        assert type in ["l2", "l1"]
        self.sigma_sampler = instantiate_from_config(sigma_sampler_config)
        self.type = type
        self.offset_noise_level = offset_noise_level

    def __call__(self, *args, **kwargs):
        raise NotImplementedError("training losses are out of scope of the MI355X inference path")


class FullLoss(StandardDiffusionLoss):
    def __init__(self, seq_len=12, kernel_size=3, gaussian_sigma=0.5, min_attn_size=16, lambda_local_loss=0.0,
                 lambda_ocr_loss=0.0, lambda_style_loss=0.0, ocr_enabled=False, style_enabled=False,
                 predictor_config=None, *args, **kwarg):
        super().__init__(*args, **kwarg)
        if kernel_size != 3:
            raise NotImplementedError("udt_local_loss implements the 3x3 blur of the UDiffText config")
        self.gaussian_kernel_size = kernel_size
        self.register_buffer("g_kernel", self.get_gaussian_kernel(kernel_size, gaussian_sigma, seq_len))
        self.min_attn_size = min_attn_size
        self.lambda_local_loss, self.lambda_ocr_loss, self.lambda_style_loss = lambda_local_loss, lambda_ocr_loss, lambda_style_loss
        self.style_enabled, self.ocr_enabled = style_enabled, ocr_enabled
        if ocr_enabled:
            self.predictor = instantiate_from_config(predictor_config)

    @staticmethod
    def get_gaussian_kernel(kernel_size=3, sigma=1, out_channels=3):
        ax = torch.arange(kernel_size).float() - (kernel_size - 1) / 2.0
        g = torch.exp(-(ax[:, None] ** 2 + ax[None, :] ** 2) / (2 * sigma ** 2.)) / (2. * torch.pi * sigma ** 2.)
        g = g / g.sum()
        return g.view(1, 1, kernel_size, kernel_size).tile(out_channels, 1, 1, 1)

    def get_ocr_loss_decoded(self, decoded, r_bbox, label, weight=None, want_grad: bool = True):
        """The part of ``get_ocr_loss`` (reference loss.py:178-190) AFTER ``first_stage_model.decode``: decoded fp32 [B, 3, H, W] on the
        GPU (the decoder's output as it is, in [-1, 1]: the reference does not remap it), r_bbox: per image (top, bottom, left, right) on
        the host, label: B strings -> ``self.predictor.calc_loss_boxes`` on the boxes (i, *r_bbox[i]): (ocr loss fp32 [B], its gradient
        with respect to ``decoded`` fp32 [B, 3, H, W], or None without ``want_grad``).
        The other half — ``model_output / scaler`` and the VAE decoder's reverse pass, which carries this gradient to the UNet's
        output — is ``get_ocr_loss``.
        ValueError when there is no predictor (``ocr_enabled`` was false at construction)."""
        predictor = getattr(self, "predictor", None)
        if predictor is None:
            raise ValueError("get_ocr_loss_decoded needs the OCR predictor: construct FullLoss with ocr_enabled=True and a predictor_config")
        if isinstance(r_bbox, torch.Tensor) and r_bbox.is_cuda:
            raise ValueError("r_bbox is read on the host: pass it as a host tensor or a list")
        rows = torch.as_tensor(r_bbox).reshape(-1, 4).tolist()
        boxes = [[i] + list(bb) for i, bb in enumerate(rows)]
        return predictor.calc_loss_boxes(decoded, boxes, label, weight=weight, want_grad=want_grad)

    def get_ocr_loss(self, model_output, r_bbox, label, first_stage_model, scaler, want_grad: bool = True, weight=None):
        """reference loss.py:178-190, its arguments in its order: ``model_output / scaler`` -> ``first_stage_model.decode`` -> the crop
        of every image's box -> ``predictor.calc_loss``.  model_output fp32 [B, 4, h, w] on the GPU (the denoiser's output D).
        -> (ocr loss fp32 [B], d_model_output fp32 [B, 4, h, w] or None without ``want_grad``):
        d_model_output = (1 / scaler) * decoder_vjp(d_decoded), d_decoded from ``get_ocr_loss_decoded`` (``weight``: the upstream
        cotangent of each row's loss, passed through to it).  The decoder runs on a tape (vae_backward.decode_tape) only when the
        gradient is wanted.  ``lambda_ocr_loss * mean`` is the caller's (training.training_loss_and_grads).
        ValueError when there is no predictor."""
        if getattr(self, "predictor", None) is None:
            raise ValueError("get_ocr_loss needs the OCR predictor: construct FullLoss with ocr_enabled=True and a predictor_config")
        from udifftext_amd import vae_backward
        z = (model_output.float() * (1.0 / float(scaler))).contiguous()
        if not want_grad:
            loss, _ = self.get_ocr_loss_decoded(first_stage_model.decode(z), r_bbox, label, weight=weight, want_grad=False)
            return loss, None
        frames, bwd = vae_backward.decode_tape(first_stage_model, z)
        loss, d_frames = self.get_ocr_loss_decoded(frames, r_bbox, label, weight=weight, want_grad=True)
        return loss, bwd(d_frames) / float(scaler)

    def scores_map(self, hw) -> bool:
        """a t_attn layer is scored when min(h, w) >= min_attn_size: the reference's ``size >= min_attn_size`` for h == w (it
        raises for h != w), and never a blur over a map fewer than min_attn_size pixels high or wide"""
        return min(int(hw[0]), int(hw[1])) >= self.min_attn_size

    def get_min_local_loss(self, attn_map_cache, mask, seg_mask, cond_only: bool = False):
        """-> fp32 [n], n = batch of the attention maps (uncond ‖ cond).  mask [B,1,H,W], seg_mask [B, seg_l] with
        n a multiple of B: sample i of the maps is scored against mask[i % B] (for B = 1 this is the reference's
        broadcast; for B > 1 the reference is undefined — SURVEY.md §8a row N — and this is the per-sample rule).
        cond_only: score only the conditional half (the half every caller keeps, reference sampling.py: ``local_loss[B:]``)
        -> fp32 [n / 2].  The maps are h x w (``item["hw"]``, tokens row-major), the mask is resized per axis; a layer counts
        when ``scores_map(hw)``.  Two launches per scored attention map, whatever n is."""
        mask = mask.float().contiguous()
        seg = seg_mask.float().contiguous()
        B = mask.shape[0]
        gk = self.g_kernel[0, 0].reshape(9).float().contiguous()
        loss, count = None, 0
        for item in attn_map_cache:
            if not item["name"].endswith("t_attn") or item["attn_map"] is None:
                continue
            heads, hw, am = item["heads"], item["hw"], item["attn_map"]
            if not self.scores_map(hw):
                continue
            n = am.shape[0] // heads
            assert n % B == 0 and seg.shape[1] <= am.shape[2]
            first = n // 2 if cond_only else 0
            assert first % B == 0
            if loss is None:
                loss = torch.zeros((n - first,), dtype=torch.float32, device=am.device)
            ops.local_loss_accumulate_hw(am[first * heads:], mask, seg, gk, loss, heads, hw)
            count += 1
        return loss / count
