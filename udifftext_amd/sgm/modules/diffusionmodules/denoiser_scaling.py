"""Preconditioning coefficients (reference sgm/modules/diffusionmodules/denoiser_scaling.py:4-31)."""
import torch


class EDMScaling:
    def __init__(self, sigma_data=0.5):
        self.sigma_data = sigma_data

    def __call__(self, sigma: torch.Tensor):
        denom = sigma ** 2 + self.sigma_data ** 2
        return self.sigma_data ** 2 / denom, sigma * self.sigma_data / denom ** 0.5, 1 / denom ** 0.5, 0.25 * sigma.log()


class EpsScaling:
    """eps-prediction: c_skip = 1, c_out = -sigma, c_in = (sigma^2 + 1)^-1/2, c_noise = sigma"""

    def __call__(self, sigma: torch.Tensor):
        return torch.ones_like(sigma), -sigma, 1 / (sigma ** 2 + 1.0) ** 0.5, sigma.clone()


class VScaling:
    def __call__(self, sigma: torch.Tensor):
        denom = sigma ** 2 + 1.0
        return 1.0 / denom, -sigma / denom ** 0.5, 1.0 / denom ** 0.5, sigma.clone()
