"""`ArtifactSpectra`: a beta-binomial allele-fraction spectrum of artifacts per (depth bin, variant type) cell (reference
permutect/architecture/spectra/artifact_spectra.py:17-75), what `refine_artifact_model --learn_artifact_spectra` stores in the model
file for the posterior stage.  Same parameters, same `state_dict` keys (`parametrizations.alpha_dv.original`,
`parametrizations.beta_dv.original`: the logs of alpha and beta), same `forward` and `fit` signatures; the plots are out of scope.

`fit` is the reference's loop -- epochs of batch-64 torch.optim.Adam steps on minus the mean log-likelihood of the minibatch -- and
where it runs decides how:

  * a float32 module on a ROCm device makes ONE library call (pmt_spectra_fit, csrc/pmt_spectra_fit.hip): the 15 cells are
    independent problems under an element-wise optimizer, a wavefront each runs every step with its parameters in registers;
  * a module on the CPU -- or any module under PMT_SPECTRA_FIT=torch, or one that is not float32 -- runs the torch loop.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor, nn
from torch.nn.utils import parametrize

from permutect_amd.architecture.modules import PositiveNumber
from permutect_amd.engine import lib as L
from permutect_amd.enums import Variation
from permutect_amd.stats_utils import ADAM_DEFAULTS, beta_binomial_log_lk, fits_on_device

DEPTH_CUTOFFS = [10, 20]
NUM_DEPTH_BINS = len(DEPTH_CUTOFFS) + 1


def depths_to_depth_bins(depths_b: Tensor) -> Tensor:
    """the bin is the number of cutoffs that are met or exceeded (reference :22-24)"""
    return (depths_b >= DEPTH_CUTOFFS[0]).long() + (depths_b >= DEPTH_CUTOFFS[1]).long()


def check_fit_inputs(types_b: Tensor, depths_b: Tensor, alt_counts_b: Tensor) -> None:
    """What the reference would turn into NaN parameters is refused before anything is launched."""
    if not (types_b.dim() == 1 and types_b.shape == depths_b.shape == alt_counts_b.shape):
        raise ValueError(f"ArtifactSpectra.fit: three 1-D tensors of one length, not {tuple(types_b.shape)}, {tuple(depths_b.shape)}, "
                         f"{tuple(alt_counts_b.shape)}")
    if types_b.numel() == 0:
        return
    if bool(((types_b < 0) | (types_b >= len(Variation))).any()):
        raise ValueError(f"ArtifactSpectra.fit: a variant type outside 0 .. {len(Variation) - 1}")
    if bool((alt_counts_b < 0).any()):
        raise ValueError("ArtifactSpectra.fit: a negative alt count")
    if bool((alt_counts_b > depths_b).any()):
        raise ValueError("ArtifactSpectra.fit: an alt count above its depth")


class ArtifactSpectra(nn.Module):
    def __init__(self):
        super().__init__()
        self.V = len(Variation)
        self.D = NUM_DEPTH_BINS
        self.alpha_dv = nn.Parameter(2 * torch.ones(self.D, self.V))
        parametrize.register_parametrization(self, "alpha_dv", PositiveNumber())
        self.beta_dv = nn.Parameter(30 * torch.ones(self.D, self.V))
        parametrize.register_parametrization(self, "beta_dv", PositiveNumber())

    def raw_parameters(self):
        """(log alpha, log beta) [3][5]: the `.original` tensors"""
        return self.parametrizations.alpha_dv.original, self.parametrizations.beta_dv.original

    def forward(self, variant_types_b: Tensor, depths_b: Tensor, alt_counts_b: Tensor) -> Tensor:
        """log-likelihood of each variant's alt count given its depth under its cell's beta-binomial (reference :48-55)"""
        var_types_b = variant_types_b.long()
        depth_bins_b = depths_to_depth_bins(depths_b)
        cells_b = depth_bins_b * self.V + var_types_b  # (a flat index, like the reference's index_tensor)
        alpha_b = self.alpha_dv.reshape(-1)[cells_b]
        beta_b = self.beta_dv.reshape(-1)[cells_b]
        return beta_binomial_log_lk(n=depths_b, k=alt_counts_b, alpha=alpha_b, beta=beta_b)

    def fit(self, num_epochs: int, types_b: Tensor, depths_b: Tensor, alt_counts_b: Tensor, batch_size: int = 64):
        """Reference :58-75.  The minibatches are consecutive slices of the three tensors in the order given, every epoch the same;
        the last one of an epoch may be short.  Nothing is clipped (the reference's `backpropagate` is given no parameters to clip)."""
        if num_epochs < 0 or batch_size < 1:
            raise ValueError(f"ArtifactSpectra.fit: num_epochs {num_epochs}, batch_size {batch_size}")
        raw = self.raw_parameters()
        dev, dtype = raw[0].device, raw[0].dtype
        types_b, depths_b, alt_counts_b = types_b.to(dev), depths_b.to(dev), alt_counts_b.to(dev)  # (one upload each, wherever they were)
        check_fit_inputs(types_b, depths_b, alt_counts_b)
        if fits_on_device(raw[0], "PMT_SPECTRA_FIT"):
            return self._fit_on_device(num_epochs, types_b, depths_b, alt_counts_b, batch_size)
        types_b, depths_b, alt_counts_b = types_b.long(), depths_b.to(dtype), alt_counts_b.to(dtype)
        optimizer = torch.optim.Adam(self.parameters(), **ADAM_DEFAULTS)
        n = len(alt_counts_b)
        num_batches = math.ceil(n / batch_size)
        for _ in range(num_epochs):
            for batch in range(num_batches):
                sl = slice(batch * batch_size, min((batch + 1) * batch_size, n))
                loss = -torch.mean(self.forward(types_b[sl], depths_b[sl], alt_counts_b[sl]))
                optimizer.zero_grad(set_to_none=True)
                loss.backward()
                optimizer.step()

    def _fit_on_device(self, num_epochs: int, types_b: Tensor, depths_b: Tensor, alt_counts_b: Tensor, batch_size: int):
        o_a, o_b = self.raw_parameters()
        dev = o_a.device
        n = int(types_b.numel())
        if n == 0 or num_epochs == 0:  # no step, as in the reference
            return
        if n >= 2 ** 31:
            raise ValueError(f"ArtifactSpectra.fit: {n} rows; the device fit indexes them with 32 bits")
        types, depths, alts = (t.to(device=dev, dtype=torch.int32).contiguous() for t in (types_b, depths_b, alt_counts_b))
        la, lb = o_a.detach().clone(memory_format=torch.contiguous_format), o_b.detach().clone(memory_format=torch.contiguous_format)
        hyper = ADAM_DEFAULTS
        with torch.cuda.device(dev):
            L.check(L.load().pmt_spectra_fit(types.data_ptr(), depths.data_ptr(), alts.data_ptr(), n, la.data_ptr(), lb.data_ptr(),
                                             int(batch_size), int(num_epochs), hyper["lr"], hyper["betas"][0], hyper["betas"][1], hyper["eps"],
                                             L.raw_stream(dev)), "pmt_spectra_fit")
            with torch.no_grad():
                o_a.copy_(la)
                o_b.copy_(lb)
