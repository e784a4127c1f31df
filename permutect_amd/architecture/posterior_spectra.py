"""The spectra of the posterior model: everything that turns alt and ref read counts into a likelihood (reference
permutect/architecture/spectra/somatic_spectrum.py:45-96, normal_artifact_spectrum.py:24-58, posterior_model_spectra.py:18-124).  Same
parameters, same `state_dict` keys, same constants; `forward` only -- neither the stand-alone `fit` of the somatic spectrum nor plots.

These modules are the torch form of the posterior stage: what runs on the CPU, in float64 and under PMT_POSTERIOR=torch, and what
csrc/pmt_posterior.hip was written from.  They take the columns of a `PosteriorRows` (architecture/posterior_model.py) as tensors of
the module's dtype (counts included: the reference's integer counts are promoted to it by the first arithmetic that touches them).
"""
from __future__ import annotations

import math

import torch
from torch import Tensor, nn
from torch.nn.utils import parametrize

from permutect_amd.architecture.artifact_spectra import ArtifactSpectra
from permutect_amd.architecture.modules import BoundedNumber, LogWeights, PositiveNumber
from permutect_amd.enums import Call, Variation
from permutect_amd.stats_utils import beta_binomial_log_lk, binomial_log_lk

NUM_SOMATIC_COMPONENTS = 5
NUM_MIXTURE_POINTS = 100  # len(torch.arange(0.001, 0.999, 0.01)): the binomial mixture that stands for the uniform-binomial integral


def uniform_binomial_log_lk(n: Tensor, k: Tensor, x1: Tensor, x2: Tensor) -> Tensor:
    """log of the mean over 100 points p between x1 and x2 of Binomial(k | n, p) (reference utils/stats_utils.py:160-175)"""
    interp = torch.arange(start=0.001, end=0.999, step=0.01, dtype=n.dtype).to(device=n.device)  # (the reference's, in torch's default dtype)
    assert len(interp) == NUM_MIXTURE_POINTS
    x1_x, x2_x = x1.unsqueeze(-1), x2.unsqueeze(-1)
    n_x, k_x = n.unsqueeze(-1), k.unsqueeze(-1)
    interp_x = interp.view(*([1] * x1.dim()), -1)
    p_x = x2_x * interp_x + x1_x * (1 - interp_x)
    return torch.logsumexp(binomial_log_lk(n_x, k_x, p_x), dim=-1) - math.log(NUM_MIXTURE_POINTS)


def add_in_log_space(x: Tensor, y: Tensor) -> Tensor:
    """reference utils/math_utils.py:40-49"""
    m = torch.maximum(x, y)
    return m + torch.log(torch.exp(x - m) + torch.exp(y - m))


class SomaticSpectrum(nn.Module):
    """K uniform-binomial clusters c_k * Uniform[maf, 1 - maf] with learned cell fractions and weights, plus a background cluster (a flat
    beta-binomial of fixed weight 1e-4) without learned parameters (reference somatic_spectrum.py:45-96)."""

    def __init__(self, num_components: int):
        super().__init__()
        self.K = num_components
        self.cf_k = nn.Parameter(torch.sigmoid((6 * ((torch.arange(num_components) / num_components) - 0.5))))
        parametrize.register_parametrization(self, "cf_k", BoundedNumber(0, 1))
        self.log_weights_k = nn.Parameter(torch.log(torch.square(self.cf_k.detach())))
        parametrize.register_parametrization(self, "log_weights_k", LogWeights())
        background_weight = 0.0001
        self.log_background_weight = nn.Parameter(torch.log(torch.tensor(background_weight)), requires_grad=False)
        self.log_non_background_weight = nn.Parameter(torch.log(torch.tensor(1 - background_weight)), requires_grad=False)
        self.background_alpha = nn.Parameter(torch.tensor([1]), requires_grad=False)
        self.background_beta = nn.Parameter(torch.tensor([1]), requires_grad=False)

    def forward(self, depths_b: Tensor, alt_counts_b: Tensor, mafs_b: Tensor) -> Tensor:
        alt_counts_bk = alt_counts_b.view(-1, 1)
        depths_bk = depths_b.view(-1, 1)
        mafs_bk = torch.clamp(mafs_b, max=0.49).view(-1, 1)  # maf = 0.5 exactly would make x1 = x2
        cf_bk = self.cf_k.view(1, -1)
        x1_bk, x2_bk = mafs_bk * cf_bk, (1 - mafs_bk) * cf_bk
        uniform_binomial_log_lks_bk = uniform_binomial_log_lk(n=depths_bk, k=alt_counts_bk, x1=x1_bk, x2=x2_bk)
        log_weights_bk = self.log_weights_k.view(1, -1)
        non_background_log_lks_b = torch.logsumexp(log_weights_bk + uniform_binomial_log_lks_bk, dim=-1)
        background_log_lks_b = beta_binomial_log_lk(n=depths_b, k=alt_counts_b, alpha=self.background_alpha, beta=self.background_beta)
        return add_in_log_space(self.log_non_background_weight + non_background_log_lks_b, self.log_background_weight + background_log_lks_b)


class NormalArtifactSpectrum(nn.Module):
    """P(normal alt | normal depth) by an ArtifactSpectra of its own, times P(tumor alt | normal allele fraction, tumor depth): a
    beta-binomial whose mean is a type-dependent multiple of the normal's allele fraction (reference normal_artifact_spectrum.py:24-58)."""

    def __init__(self):
        super().__init__()
        V = len(Variation)
        self.normal_spectrum = ArtifactSpectra()
        self.mean_multiplier_v = nn.Parameter(0.5 * torch.ones(V))
        parametrize.register_parametrization(self, "mean_multiplier_v", BoundedNumber(0, 1))
        self.concentration_v = nn.Parameter(30 * torch.ones(V))  # alpha + beta
        parametrize.register_parametrization(self, "concentration_v", PositiveNumber())

    def forward(self, var_types_b: Tensor, tumor_alt_counts_b: Tensor, tumor_depths_b: Tensor, normal_alt_counts_b: Tensor,
                normal_depths_b: Tensor):
        normal_log_lks_b = self.normal_spectrum.forward(var_types_b, normal_depths_b, normal_alt_counts_b)
        mean_multiplier_b = self.mean_multiplier_v[var_types_b]
        concentration_b = self.concentration_v[var_types_b]
        normal_af_b = normal_alt_counts_b / (normal_depths_b + 0.001)
        tumor_mean_b = normal_af_b * mean_multiplier_b
        alpha_b = 0.001 + tumor_mean_b * concentration_b
        beta_b = torch.clamp(concentration_b - alpha_b, min=0.001)
        tumor_log_lks_b = beta_binomial_log_lk(n=tumor_depths_b, k=tumor_alt_counts_b, alpha=alpha_b, beta=beta_b)
        return tumor_log_lks_b, normal_log_lks_b


def germline_log_likelihood(afs: Tensor, mafs: Tensor, alt_counts: Tensor, depths: Tensor, het_beta: float = None) -> Tensor:
    """given germline, the likelihood of these counts: het with the alt on the minor or on the major allele, or hom alt (reference
    posterior_model_spectra.py:18-54)"""
    dt = dict(device=depths.device, dtype=depths.dtype)
    hom_alpha, hom_beta = torch.tensor([98.0], **dt), torch.tensor([2.0], **dt)
    het_probs = 2 * afs * (1 - afs)
    hom_probs = afs * afs
    het_proportion = het_probs / (het_probs + hom_probs)
    hom_proportion = 1 - het_proportion
    log_mafs = torch.log(mafs)
    log_1m_mafs = torch.log(1 - mafs)
    log_half_het_prop = torch.log(het_proportion / 2)
    ref_counts = depths - alt_counts
    if het_beta is None:
        combinatorial_term = torch.lgamma(depths + 1) - torch.lgamma(alt_counts + 1) - torch.lgamma(ref_counts + 1)
        alt_minor = combinatorial_term + alt_counts * log_mafs + ref_counts * log_1m_mafs
        alt_major = combinatorial_term + ref_counts * log_mafs + alt_counts * log_1m_mafs
    else:
        hb = torch.tensor([het_beta], **dt)
        alt_minor = alt_major = beta_binomial_log_lk(depths, alt_counts, hb, hb)
    alt_minor_ll = log_half_het_prop + alt_minor
    alt_major_ll = log_half_het_prop + alt_major
    hom_ll = torch.log(hom_proportion) + beta_binomial_log_lk(depths, alt_counts, hom_alpha, hom_beta)
    return torch.logsumexp(torch.vstack((alt_minor_ll, alt_major_ll, hom_ll)), dim=0)


class PosteriorModelSpectra(nn.Module):
    """the somatic spectrum, the tumor artifact spectra, the normal artifact spectrum and the germline likelihoods (reference
    posterior_model_spectra.py:57-124)"""

    def __init__(self, het_beta: float = None):
        super().__init__()
        self.het_beta = het_beta
        self.somatic_spectrum = SomaticSpectrum(num_components=NUM_SOMATIC_COMPONENTS)
        self.artifact_spectra = ArtifactSpectra()
        self.normal_artifact_spectra = NormalArtifactSpectrum()

    def spectra_log_likelihoods_bc(self, rows) -> tuple[Tensor, Tensor]:
        """`rows`: anything with the columns of a PosteriorRows as tensors (variant types integer, the rest of this module's dtype)"""
        dtype = self.artifact_spectra.raw_parameters()[0].dtype
        var_types_b = rows.variant_types.long()
        afs_b, mafs_b = rows.allele_frequencies.to(dtype), rows.mafs.to(dtype)
        depths_b, alt_counts_b = rows.depths.to(dtype), rows.alt_counts.to(dtype)
        normal_depths_b, normal_alt_counts_b = rows.normal_depths.to(dtype), rows.normal_alt_counts.to(dtype)

        na_tumor_log_lks_b, na_normal_log_lks_b = self.normal_artifact_spectra.forward(
            var_types_b=var_types_b, tumor_alt_counts_b=alt_counts_b, tumor_depths_b=depths_b, normal_alt_counts_b=normal_alt_counts_b,
            normal_depths_b=normal_depths_b)
        spectra_log_lks_bc = torch.zeros((len(var_types_b), len(Call)), device=depths_b.device, dtype=dtype)
        spectra_log_lks_bc[:, Call.SOMATIC] = self.somatic_spectrum.forward(depths_b, alt_counts_b, mafs_b)
        spectra_log_lks_bc[:, Call.ARTIFACT] = self.artifact_spectra.forward(var_types_b, depths_b, alt_counts_b)
        spectra_log_lks_bc[:, Call.NORMAL_ARTIFACT] = na_tumor_log_lks_b
        spectra_log_lks_bc[:, Call.SEQ_ERROR] = rows.seq_error_log_lks.to(dtype)
        spectra_log_lks_bc[:, Call.GERMLINE] = germline_log_likelihood(afs_b, mafs_b, alt_counts_b, depths_b, self.het_beta)

        normal_seq_error_log_lks = rows.normal_seq_error_log_lks.to(dtype)
        normal_log_lks_bc = torch.zeros_like(spectra_log_lks_bc)
        normal_log_lks_bc[:, Call.SOMATIC] = normal_seq_error_log_lks
        normal_log_lks_bc[:, Call.ARTIFACT] = normal_seq_error_log_lks
        normal_log_lks_bc[:, Call.SEQ_ERROR] = normal_seq_error_log_lks
        normal_log_lks_bc[:, Call.NORMAL_ARTIFACT] = torch.where(normal_alt_counts_b < 1, -9999, na_normal_log_lks_b)
        normal_log_lks_bc[:, Call.GERMLINE] = germline_log_likelihood(afs_b, rows.normal_mafs.to(dtype), normal_alt_counts_b, normal_depths_b,
                                                                      self.het_beta)
        return spectra_log_lks_bc, normal_log_lks_bc
