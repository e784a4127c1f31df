"""The likelihoods that the spectra and the downsampler share (reference permutect/utils/stats_utils.py), and what their fits share:
torch's optimizer defaults and the rule for where a fit runs.  Needs torch alone: no built library."""
from __future__ import annotations

import os

import torch
from torch import Tensor

# torch.optim.Adam's defaults, which the reference takes as they are; AdamW's are the same plus the weight decay.  The device fits
# are given these numbers; the torch loops build their optimizers with them.
ADAM_DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
ADAMW_DEFAULTS = dict(ADAM_DEFAULTS, weight_decay=1e-2)


def fits_on_device(param: Tensor, switch_env_name: str) -> bool:
    """Whether a fit of `param`'s module makes its library calls or runs its torch loop: a float32 module on a ROCm device uses the
    library, unless the environment variable `switch_env_name` says `torch`."""
    return param.device.type == "cuda" and param.dtype == torch.float32 and os.environ.get(switch_env_name, "") != "torch"


def log_binomial_coefficient(n: Tensor, k: Tensor) -> Tensor:
    return torch.lgamma(n + 1) - torch.lgamma(n - k + 1) - torch.lgamma(k + 1)


def binomial_log_lk(n: Tensor, k: Tensor, p: Tensor) -> Tensor:
    """reference utils/stats_utils.py:21-25"""
    return log_binomial_coefficient(n, k) + k * torch.log(p) + (n - k) * torch.log(1 - p)


def beta_binomial_log_lk(n: Tensor, k: Tensor, alpha: Tensor, beta: Tensor) -> Tensor:
    """log P(k | n, alpha, beta), normalised (reference utils/stats_utils.py:28-40)"""
    return (log_binomial_coefficient(n, k) + torch.lgamma(k + alpha) + torch.lgamma(n - k + beta) + torch.lgamma(alpha + beta)
            - torch.lgamma(n + alpha + beta) - torch.lgamma(alpha) - torch.lgamma(beta))
