"""The priors of the posterior model (reference permutect/architecture/posterior_model_priors.py:21-52, :71-145, :147-225).  Same
parameters and `state_dict` keys.

The context-dependent M step of the reference (:169-222) fits per-context SNV mutation rates with pymc: a mean-field ADVI run and the
mean of 1000 draws, stochastic and unseeded.  That fit is NOT reproduced here and no parity with its numbers is claimed.  What is built is
a DETERMINISTIC estimator of the SAME generative model (`context_objective`, `fit_context_rates`; on a ROCm device one persistent launch,
csrc/pmt_context_fit.hip): the maximiser of the model's log joint -- Beta(1, 1e6) overall rate, Gamma(4, 5) concentrations, a
Dirichlet over the 12 substitutions, twelve Dirichlets over the 16 flanking contexts, Binomial counts -- with every prior density taken in
its unconstrained coordinate (logit, log, softmax basis), in which the mode of each conjugate piece equals its posterior mean
(theta_i ~ k_i + kappa, kappa = 4 / 5): the closest deterministic stand-in for the posterior mean the reference reports, and strictly
positive everywhere.  Everything around the fit -- the rrra -> sc conversion, the two roundings, the write-back -- is the reference's
arithmetic, pinned against its own code (tests/golden/context_priors.npz).
"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch import Tensor, nn

from permutect_amd.engine import lib as L
from permutect_amd.enums import Call, Variation
from permutect_amd.stats_utils import ADAM_DEFAULTS, fits_on_device

NUM_SUBSTITUTIONS, NUM_FLANKS = 12, 16
CONTEXT_FIT_STEPS, CONTEXT_FIT_LR = 2000, 0.05
LOG_RATE_CAP = math.log1p(-1e-6)


def _sc_to_rrra_index() -> Tensor:
    """[12][16] flat indices into a 5 x 5 x 5 x 5 table: substitution s = ref * 4 + alt without the ref == alt entries (A>C = 0 ..
    T>G = 11), flanks c = left * 4 + right, entry [left][ref][right][alt]"""
    index = torch.zeros(NUM_SUBSTITUTIONS, NUM_FLANKS, dtype=torch.long)
    s = 0
    for ref in range(4):
        for alt in range(4):
            if ref == alt:
                continue
            for left in range(4):
                for right in range(4):
                    index[s, left * 4 + right] = ((left * 5 + ref) * 5 + right) * 5 + alt
            s += 1
    return index


SC_TO_RRRA = _sc_to_rrra_index()


def convert_rrra_tensor_to_sc(input_rrra: Tensor) -> Tensor:
    """the 12 x 16 SNV cells of a 5 x 5 x 5 x 5 table (reference :34-52); bins with a deletion code and ref == alt entries are dropped"""
    return input_rrra.reshape(-1)[SC_TO_RRRA.to(input_rrra.device)]


def context_fit_counts(somatic_snv_totals_rrra: Tensor, snv_context_totals_rrra: Tensor, posterior_totals_vc: Tensor, ratio: float):
    """(n_sc, k_sc) of the reference (:158-171), as float tensors holding integers: rounded to even in the totals' dtype"""
    total_nonignored = torch.sum(posterior_totals_vc).item()
    total_ignored_per_context = ratio * total_nonignored / 64
    n_sc = torch.round(convert_rrra_tensor_to_sc(snv_context_totals_rrra) + total_ignored_per_context)
    k_sc = torch.round(convert_rrra_tensor_to_sc(somatic_snv_totals_rrra))
    return n_sc, torch.minimum(k_sc, n_sc)  # (a posterior is at most 1: the cap only guards the Binomial against a caller's totals)


def context_start(n_sc: Tensor, k_sc: Tensor) -> Tensor:
    """the 207 unknowns [u, a, b, x (12), y (12 x 16)] at the start: x = y = 0, kappa = 0.8, R = (sum k + 1) / (sum n + 1e6 + 1)"""
    p = torch.zeros(3 + NUM_SUBSTITUTIONS * (1 + NUM_FLANKS), dtype=n_sc.dtype)
    r = (k_sc.double().sum() + 1) / (n_sc.double().sum() + 1e6 + 1)
    p[0] = torch.log(r) - torch.log1p(-r)
    p[1] = p[2] = math.log(0.8)
    return p


def context_log_rates(p: Tensor) -> Tensor:
    """log p_sc [12][16] of the unknowns, capped at log(1 - 1e-6)"""
    u, x, y = p[0], p[3:15], p[15:].view(NUM_SUBSTITUTIONS, NUM_FLANKS)
    log_p = torch.nn.functional.logsigmoid(u) + math.log(192.0) + torch.log_softmax(x, 0)[:, None] + torch.log_softmax(y, 1)
    return torch.clamp(log_p, max=LOG_RATE_CAP)


def context_objective(p: Tensor, n_sc: Tensor, k_sc: Tensor) -> Tensor:
    """F: the log joint of the reference's model (:173-201) with the Beta prior in the logit, the Gamma priors in the log and the
    Dirichlet priors in the softmax basis (differentiable: the gradient test's yardstick)"""
    u, a, b, x, y = p[0], p[1], p[2], p[3:15], p[15:].view(NUM_SUBSTITUTIONS, NUM_FLANKS)
    log_r, log_1mr = torch.nn.functional.logsigmoid(u), torch.nn.functional.logsigmoid(-u)
    lts, ltsc = torch.log_softmax(x, 0), torch.log_softmax(y, 1)
    log_p = context_log_rates(p)
    ks, kc = torch.exp(a), torch.exp(b)
    f = (k_sc * log_p + (n_sc - k_sc) * torch.log1p(-torch.exp(log_p))).sum()
    f = f + log_r + 1e6 * log_1mr + 4 * a - 5 * ks + 4 * b - 5 * kc
    f = f + torch.lgamma(12 * ks) - 12 * torch.lgamma(ks) + ks * lts.sum()
    return f + 12 * (torch.lgamma(16 * kc) - 16 * torch.lgamma(kc)) + kc * ltsc.sum()


def context_gradient(p: Tensor, n_sc: Tensor, k_sc: Tensor) -> Tensor:
    """dF / dp in closed form (what the kernel evaluates)"""
    u, a, b, x, y = p[0], p[1], p[2], p[3:15], p[15:].view(NUM_SUBSTITUTIONS, NUM_FLANKS)
    r, ks, kc = torch.sigmoid(u), torch.exp(a), torch.exp(b)
    lts, ltsc = torch.log_softmax(x, 0), torch.log_softmax(y, 1)
    ts, tsc = torch.exp(lts), torch.exp(ltsc)
    log_p = torch.nn.functional.logsigmoid(u) + math.log(192.0) + lts[:, None] + ltsc
    capped = log_p >= LOG_RATE_CAP
    rate = torch.exp(torch.clamp(log_p, max=LOG_RATE_CAP))
    w = torch.where(capped, torch.zeros_like(rate), k_sc - (n_sc - k_sc) * rate / (1 - rate))
    w_s = w.sum(1)
    w_all = w_s.sum()
    g = torch.empty_like(p)
    g[0] = (1 - r) * (w_all + 1) - 1e6 * r
    g[1] = 4 - 5 * ks + ks * (12 * torch.digamma(12 * ks) - 12 * torch.digamma(ks) + lts.sum())
    g[2] = 4 - 5 * kc + kc * (12 * (16 * torch.digamma(16 * kc) - 16 * torch.digamma(kc)) + ltsc.sum())
    g[3:15] = w_s + ks - ts * (w_all + 12 * ks)
    g[15:] = (w + kc - tsc * (w_s[:, None] + 16 * kc)).reshape(-1)
    return g


@torch.no_grad()
def fit_context_rates(n_sc: Tensor, k_sc: Tensor, steps: int = CONTEXT_FIT_STEPS, lr: float = CONTEXT_FIT_LR, dtype=None):
    """The torch mirror of pmt_context_priors_fit, on the CPU in `dtype` (default: the counts'): `steps` steps of torch.optim.Adam on
    -F / max(sum k, 1) from `context_start` with the learning rate lr (1 - t / steps).  Returns (log p_sc [12][16], the last step's
    largest |dF| / max(sum k, 1))."""
    dtype = dtype or n_sc.dtype
    n_sc, k_sc = n_sc.detach().to("cpu", dtype), k_sc.detach().to("cpu", dtype)
    p = context_start(n_sc, k_sc)
    (beta1, beta2), eps = ADAM_DEFAULTS["betas"], ADAM_DEFAULTS["eps"]
    exp_avg, exp_avg_sq = torch.zeros_like(p), torch.zeros_like(p)
    scale = max(float(k_sc.double().sum()), 1.0)
    last = 0.0
    for t in range(steps):  # torch.optim.Adam's single-tensor update, written out (a tenth of the optimizer object's overhead)
        g = context_gradient(p, n_sc, k_sc)
        if t == steps - 1:
            last = float(g.abs().max()) / scale
        g.mul_(-1 / scale)
        exp_avg.lerp_(g, 1 - beta1)
        exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
        step_size = lr * (1 - t / steps) / (1 - beta1 ** (t + 1))
        denom = (exp_avg_sq.sqrt() / math.sqrt(1 - beta2 ** (t + 1))).add_(eps)
        p.addcdiv_(exp_avg, denom, value=-step_size)
    return context_log_rates(p), last


def pack_contexts(haplotypes_bs: Tensor) -> Tensor:
    """((i0 * 5 + i1) * 5 + i2) * 5 + i3 of the four centre bases of each haplotype row (ref sequence then alt sequence, A C G T
    deletion = 0 .. 4): left flank, ref base, right flank, alt base (reference `get_ref_contexts_and_alt_bases`, :21-31)"""
    seq_length = haplotypes_bs.shape[-1] // 2
    ref_center_idx = (seq_length - 1) // 2
    alt_center_idx = ref_center_idx + seq_length
    h = haplotypes_bs.long()
    return ((h[:, ref_center_idx - 1] * 5 + h[:, ref_center_idx]) * 5 + h[:, ref_center_idx + 1]) * 5 + h[:, alt_center_idx]


class PosteriorModelPriors(nn.Module):
    """Log priors of the somatic, artifact and normal-artifact calls per variant type.  The germline prior is the variant's population
    allele frequency (1 minus the hom-ref probability; -9999 in no-germline mode) and the sequencing-error prior is log 1."""

    def __init__(self, variant_log_prior: float, artifact_log_prior: float, no_germline_mode: bool, device=torch.device("cpu")):
        super().__init__()
        self.no_germline_mode = no_germline_mode
        self._device = device
        self.use_context_dependent_snv_priors = True
        self.log_priors_vc = nn.Parameter(torch.zeros(len(Variation), len(Call)))
        with torch.no_grad():
            self.log_priors_vc[:, Call.SOMATIC] = variant_log_prior
            self.log_priors_vc[:, Call.ARTIFACT] = artifact_log_prior
            self.log_priors_vc[:, Call.GERMLINE] = -9999 if self.no_germline_mode else 0
            self.log_priors_vc[:, Call.NORMAL_ARTIFACT] = artifact_log_prior
        self.somatic_snv_log_priors_rrra = nn.Parameter(variant_log_prior * torch.ones((5, 5, 5, 5), device=self._device))

    def enable_context_dependent_snv_priors(self) -> None:
        self.use_context_dependent_snv_priors = True

    def disable_context_dependent_snv_priors(self) -> None:
        self.use_context_dependent_snv_priors = False

    def somatic_snv_log_priors(self, rows) -> Tensor:
        return self.somatic_snv_log_priors_rrra.view(-1)[rows.contexts.long()]

    def log_priors_bc(self, rows) -> Tensor:
        variant_types_b = rows.variant_types.long()
        dtype = self.log_priors_vc.dtype
        allele_frequencies_b = rows.allele_frequencies.to(dtype)
        is_snv_b = (variant_types_b == Variation.SNV).to(dtype)
        log_priors_bc = self.log_priors_vc[variant_types_b, :]
        log_priors_bc[:, Call.SEQ_ERROR] = 0
        log_priors_bc[:, Call.GERMLINE] = -9999 if self.no_germline_mode else torch.log(1 - torch.square(1 - allele_frequencies_b))
        if self.use_context_dependent_snv_priors:
            log_priors_bc[:, Call.SOMATIC] = is_snv_b * self.somatic_snv_log_priors(rows) + (1 - is_snv_b) * log_priors_bc[:, Call.SOMATIC]
        return torch.nn.functional.log_softmax(log_priors_bc, dim=-1)

    # ---- the E step's totals of the context-dependent priors (reference :112-123) -----------------------------------------------
    @classmethod
    def initialize_snv_context_totals_rrra(cls, device=torch.device("cpu"), dtype=torch.float32) -> Tensor:
        return torch.zeros(5, 5, 5, 5, device=device, dtype=dtype)

    @classmethod
    def increment_somatic_snv_context_totals_rrra(cls, snv_totals_rrra: Tensor, context_totals_rrra: Tensor, rows, posteriors_bc: Tensor) -> None:
        """for every SNV row: its somatic posterior into `snv_totals_rrra`, 1 into `context_totals_rrra`, at the row's context"""
        is_snv = (rows.variant_types.long() == Variation.SNV).to(posteriors_bc.dtype)
        contexts = rows.contexts.long()
        snv_totals_rrra.view(-1).index_add_(0, contexts, (posteriors_bc[:, Call.SOMATIC] * is_snv).to(snv_totals_rrra.dtype))
        context_totals_rrra.view(-1).index_add_(0, contexts, is_snv.to(context_totals_rrra.dtype))

    @staticmethod
    def snv_context_counts_rrra(rows) -> Tensor:
        """int64 [5][5][5][5]: the number of SNV rows per context bin (data alone: counted once per fit)"""
        snv = rows.variant_types.long().clamp(0, len(Variation) - 1) == Variation.SNV
        return torch.bincount(rows.contexts.long().clamp(0, 624)[snv], minlength=625).view(5, 5, 5, 5)

    def update_priors_m_step(self, posterior_totals_vc: Tensor, ignored_to_non_ignored_ratio: float, somatic_snv_totals_rrra: Tensor = None,
                             snv_context_totals_rrra: Tensor = None) -> None:
        """The EM-style M step: the prior of a call is its share of ALL sites, the ones that never became candidates included.  A variant
        type without posterior mass gets log 0 = -inf, as in the reference.  Torch ops on the totals' device, nothing read back.

        With context dependence on, the two context totals of the E step are needed (without them: NotImplementedError, as before this
        estimator existed): the 192 SNV entries of `somatic_snv_log_priors_rrra` become the log rates of the deterministic estimator
        described in this module's docstring -- NOT the reference's ADVI fit -- and the other 433 entries keep their bits.
        `somatic_snv_totals_rrra` is either a floating tensor of summed posteriors or, from pmt_posterior_step_context, an int64 tensor
        in 2^-30 fixed point; on a ROCm device the latter is fitted by pmt_context_priors_fit in one launch, nothing read back.
        `self.context_fit_steps` and `self.context_fit_lr` set the schedule."""
        context = self.use_context_dependent_snv_priors
        if context and (somatic_snv_totals_rrra is None or snv_context_totals_rrra is None):
            raise NotImplementedError("the context-dependent M step needs the E step's somatic_snv_totals_rrra and snv_context_totals_rrra")
        total_nonignored = torch.sum(posterior_totals_vc).double()  # (the reference's `.item()`: a Python float from here on)
        overall_total = ignored_to_non_ignored_ratio * total_nonignored + total_nonignored
        with torch.no_grad():
            self.log_priors_vc.copy_(torch.log(posterior_totals_vc / (posterior_totals_vc + overall_total)))
            self.log_priors_vc[:, Call.SEQ_ERROR] = 0
            self.log_priors_vc[:, Call.GERMLINE] = -9999 if self.no_germline_mode else 0
            if not context:
                self.somatic_snv_log_priors_rrra.fill_(self.log_priors_vc[Variation.SNV, Call.SOMATIC])
            elif somatic_snv_totals_rrra.dtype == torch.int64 and fits_on_device(self.somatic_snv_log_priors_rrra, "PMT_POSTERIOR"):
                self._context_m_step_on_device(posterior_totals_vc, ignored_to_non_ignored_ratio, somatic_snv_totals_rrra, snv_context_totals_rrra)
            else:
                self._context_m_step_mirror(posterior_totals_vc, ignored_to_non_ignored_ratio, somatic_snv_totals_rrra, snv_context_totals_rrra)

    context_fit_steps, context_fit_lr = CONTEXT_FIT_STEPS, CONTEXT_FIT_LR
    last_context_fit = None  # after a context M step: {"n_sc", "k_sc", "max_grad"} (mirror) or {"diagnostics"} (device tensor, PMT_CONTEXT_FIT_DIAG)

    def _context_m_step_mirror(self, posterior_totals_vc, ratio, somatic_snv_totals_rrra, snv_context_totals_rrra) -> None:
        dtype = self.somatic_snv_log_priors_rrra.dtype
        if somatic_snv_totals_rrra.dtype == torch.int64:
            somatic_snv_totals_rrra = (somatic_snv_totals_rrra.double() / L.CONTEXT_FIXED_ONE).to(dtype)
        n_sc, k_sc = context_fit_counts(somatic_snv_totals_rrra, snv_context_totals_rrra.to(somatic_snv_totals_rrra.dtype), posterior_totals_vc, ratio)
        log_rates_sc, max_grad = fit_context_rates(n_sc, k_sc, self.context_fit_steps, self.context_fit_lr, dtype=dtype)
        table = self.somatic_snv_log_priors_rrra
        table.view(-1)[SC_TO_RRRA.to(table.device)] = log_rates_sc.to(table.device, table.dtype)
        self.last_context_fit = {"n_sc": n_sc.cpu(), "k_sc": k_sc.cpu(), "max_grad": max_grad}

    def _context_m_step_on_device(self, posterior_totals_vc, ratio, fixed_rrra, counts_rrra) -> None:
        table = self.somatic_snv_log_priors_rrra
        dev = table.device
        assert table.is_contiguous() and fixed_rrra.is_contiguous() and fixed_rrra.numel() == 625 and fixed_rrra.device == dev
        counts, totals = counts_rrra.to(dev, torch.int64).contiguous(), posterior_totals_vc.to(dev, torch.float32).contiguous()
        assert counts.numel() == 625 and totals.numel() == len(Variation) * len(Call)
        diagnostics = torch.zeros(L.CONTEXT_FIT_DIAG, dtype=torch.float32, device=dev)
        (beta1, beta2), eps = ADAM_DEFAULTS["betas"], ADAM_DEFAULTS["eps"]
        with torch.cuda.device(dev):
            L.check(L.load().pmt_context_priors_fit(fixed_rrra.data_ptr(), counts.data_ptr(), totals.data_ptr(), float(ratio), table.data_ptr(),
                                                    int(self.context_fit_steps), float(self.context_fit_lr), beta1, beta2, eps,
                                                    diagnostics.data_ptr(), L.raw_stream(dev)), "pmt_context_priors_fit")
        self.last_context_fit = {"diagnostics": diagnostics}

    def last_context_fit_max_grad(self):
        """the last context fit's largest |dF / d unknown| / max(sum k, 1) at its last step (None without a fit; reads the device)"""
        fit = self.last_context_fit
        if fit is None:
            return None
        return float(fit["diagnostics"][0]) if "diagnostics" in fit else fit["max_grad"]
