"""Generate tests/golden/context_priors.npz by running the REFERENCE's posterior model with context-dependent SNV priors (build container
only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_context_priors_golden.py

Imports the reference with the three in-process stubs for I/O-only modules that make_golden.py uses (cyvcf2, intervaltree,
torch.utils.tensorboard; none carries arithmetic) and a RECORDING stand-in for `pymc`.  The reference's context M step
(posterior_model_priors.py:169-222) hands its integer counts to a pymc model, fits it by mean-field ADVI and averages 1000 draws: stochastic,
unseeded, and pymc is not installed.  The stand-in keeps what `pm.Binomial` is given (`n`, `observed`) and makes
`pm.fit(...).sample(...).posterior["rate_sc"]` return PRESCRIBED rates, so that the reference's OWN code does everything around the fit:
the rrra -> sc conversion, the two roundings, and the loop that writes the log rates back into the 5 x 5 x 5 x 5 table.  The prescribed
rates are the maximiser of F, the model's log joint with every prior in its unconstrained coordinate (include/permutect_amd.h:
pmt_context_priors_fit), found here by float64 L-BFGS and checked by its gradient.  No parity with ADVI is claimed anywhere.

The reference's `learn_priors_and_spectra` itself runs (its loader replaced by a list of consecutive batches in dataset order, its
prefetcher by `iter`: no arithmetic in either) for num_iterations = 1, 2, 4 at batch 64, in float32 and float64; the M step is wrapped to
keep its arguments and what it leaves behind after every epoch.

Rows: 64 * 18 + 29 = 1181 seeded candidates of their own: mostly SNVs over all 192 context bins, at most 16 per bin, half of them with
somatic-looking evidence; a few SNV rows with a deletion code in the context (their bins are dropped); the other variant types too.

The seed is searched until, in every context epoch of every case and in both precisions, no context bin's somatic total lies within
2e-3 of a half-integer, nor does the number of ignored sites per context: then the integers the fit is given are the same for every
implementation whose log priors are within 1e-4 of these (16 rows x 1e-4 / 4 = 4e-4 per bin).

Only data is written.
"""
import os
import sys
import types

REFERENCE = os.environ.get("PERMUTECT_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402

cy = types.ModuleType("cyvcf2"); cy.VCF = cy.Variant = cy.Writer = object; sys.modules["cyvcf2"] = cy
it = types.ModuleType("intervaltree"); it.IntervalTree = dict; sys.modules["intervaltree"] = it
tb = types.ModuleType("torch.utils.tensorboard")


class SummaryWriter:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, n):
        return lambda *a, **k: None


tb.SummaryWriter = SummaryWriter
sys.modules["torch.utils.tensorboard"] = tb

# ---- the estimator: F, its maximiser ----------------------------------------------------------------------------------------------------
LOG_CAP = float(np.log1p(-1e-6))


def log_rates(p):
    u, x, y = p[0], p[3:15], p[15:].view(12, 16)
    return torch.clamp(torch.nn.functional.logsigmoid(u) + float(np.log(192.0)) + torch.log_softmax(x, 0)[:, None] + torch.log_softmax(y, 1), max=LOG_CAP)


def objective(p, n, k):
    u, a, b, x, y = p[0], p[1], p[2], p[3:15], p[15:].view(12, 16)
    lts, ltsc = torch.log_softmax(x, 0), torch.log_softmax(y, 1)
    lp = log_rates(p)
    ks, kc = torch.exp(a), torch.exp(b)
    f = (k * lp + (n - k) * torch.log1p(-torch.exp(lp))).sum()
    f = f + torch.nn.functional.logsigmoid(u) + 1e6 * torch.nn.functional.logsigmoid(-u) + 4 * a - 5 * ks + 4 * b - 5 * kc
    f = f + torch.lgamma(12 * ks) - 12 * torch.lgamma(ks) + ks * lts.sum()
    return f + 12 * (torch.lgamma(16 * kc) - 16 * torch.lgamma(kc)) + kc * ltsc.sum()


def maximise(n, k):
    """(log p_sc at the maximiser of F, max |dF| / max(sum k, 1) there) by float64 L-BFGS from the estimator's start"""
    with torch.enable_grad():
        n, k = torch.as_tensor(n, dtype=torch.float64).reshape(12, 16), torch.as_tensor(k, dtype=torch.float64).reshape(12, 16)
        p = torch.zeros(207, dtype=torch.float64)
        r = (k.sum() + 1) / (n.sum() + 1e6 + 1)
        p[0] = torch.log(r) - torch.log1p(-r)
        p[1] = p[2] = float(np.log(0.8))
        p.requires_grad_()
        scale = max(float(k.sum()), 1.0)
        for _ in range(4):  # (restarts: a fresh curvature history where the line search gave up)
            opt = torch.optim.LBFGS([p], lr=1, max_iter=5000, tolerance_grad=1e-13, tolerance_change=1e-18, history_size=50, line_search_fn="strong_wolfe")

            def closure():
                opt.zero_grad()
                loss = -objective(p, n, k) / scale
                loss.backward()
                return loss

            opt.step(closure)

        def gradient(q):
            q = q.detach().clone().requires_grad_()
            return torch.autograd.grad(-objective(q, n, k) / scale, q)[0]

        # Newton steps to finish (the Hessian is singular along the softmax's shifts: pseudo-inverse), kept while the gradient shrinks
        p = p.detach()
        for _ in range(20):
            g = gradient(p)
            if float(g.abs().max()) <= 1e-10:
                break
            hessian = torch.autograd.functional.hessian(lambda q: -objective(q, n, k) / scale, p)
            candidate = p - torch.linalg.pinv(hessian, hermitian=True, rtol=1e-12) @ g
            if not float(gradient(candidate).abs().max()) < float(g.abs().max()):
                break
            p = candidate
        grad = float(gradient(p).abs().max())
        assert grad <= 1e-6, grad
        return log_rates(p.detach()).numpy().copy(), grad


# ---- the recording stand-in for pymc ----------------------------------------------------------------------------------------------------
class Sym:
    """a symbolic random variable: absorbs the arithmetic the reference builds its model with"""

    def _same(self, *a, **k):
        return self

    __mul__ = __rmul__ = __add__ = __radd__ = reshape = flatten = _same


class Mean:
    def __init__(self, a):
        self.a = a

    def to_numpy(self):
        return self.a


class Draws:
    def __init__(self, rates):
        self.rates = rates

    def mean(self, axis=None, dtype=None, out=None, **kw):  # np.mean(draws, axis=(0, 1))
        assert axis == (0, 1)
        return Mean(self.rates)


class Recorder:
    fits = []  # one entry per context M step: {"n", "k", "log_p", "grad"}
    pending = None


class ModelContext:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def binomial(name, n, p, observed):
    Recorder.pending = (np.asarray(n).copy(), np.asarray(observed).copy())
    return Sym()


class Approximation:
    def sample(self, draws):
        n, k = Recorder.pending
        assert n.shape == (192,) and k.shape == (192,) and np.issubdtype(n.dtype, np.integer) and (k <= n).all() and (k >= 0).all()
        log_p, grad = maximise(n, k)
        Recorder.fits.append({"n": n.reshape(12, 16), "k": k.reshape(12, 16), "log_p": log_p, "grad": grad})
        return types.SimpleNamespace(posterior={"rate_sc": Draws(np.exp(log_p))})


pm = types.ModuleType("pymc")
pm.Model = ModelContext
pm.Beta = pm.Gamma = pm.Dirichlet = pm.Deterministic = lambda *a, **k: Sym()
pm.Binomial = binomial
pm.math = types.SimpleNamespace(ones=lambda shape: Sym())
pm.fit = lambda method: Approximation()
sys.modules["pymc"] = pm

import permutect.architecture.posterior_model as ref_pm  # noqa: E402
import permutect.architecture.posterior_model_priors as ref_priors  # noqa: E402
from permutect.architecture.posterior_model import PosteriorModel  # noqa: E402
from permutect.architecture.posterior_model_priors import get_ref_contexts_and_alt_bases  # noqa: E402
from permutect.data.batch import Batch  # noqa: E402
from permutect.data.datum import Data, Datum  # noqa: E402

N = 64 * 18 + 29
SEQ = 11
GENOMIC_SPAN = 1e6
MAX_PER_BIN = 16
MARGIN = 2e-3
ITERATIONS = (1, 2, 4)
CPU = torch.device("cpu")


class RecordingAverage(ref_pm.StreamingAverage):
    made = []

    def __init__(self):
        super().__init__()
        RecordingAverage.made.append(self)


ref_pm.StreamingAverage = RecordingAverage
ref_pm.prefetch_generator = iter  # (the reference's prefetcher copies a batch to the default device and dtype: no arithmetic)
# (the float64 run: the reference's `is_snv` is `.float()` whatever the totals' dtype, which index_add_ refuses to add into float64
#  totals; 0 and 1 are the same numbers in both)
_add_at_index = ref_priors.add_at_index
ref_priors.add_at_index = lambda tens, idx, values: _add_at_index(tens=tens, idx=idx, values=values.to(tens.dtype))
ref_pm.trange = lambda a, b, **k: range(a, b)
ref_pm.tqdm = lambda x, **k: x


def inputs(seed):
    rng = np.random.default_rng(seed)
    types_b = np.where(rng.random(N) < 0.86, 0, rng.choice([1, 2, 3, 4], N))
    somatic = rng.random(N) < 0.5  # rows whose evidence looks somatic
    depths = rng.integers(20, 200, N)
    alts = np.where(somatic, rng.binomial(depths, rng.uniform(0.12, 0.5, N)), rng.integers(1, 5, N))
    alts = np.clip(alts, 1, depths)
    ndepths = rng.integers(15, 120, N)
    nalts = np.where(rng.random(N) < 0.85, 0, rng.integers(1, 3, N))
    logits = np.where(somatic, -rng.uniform(0.5, 8, N), rng.uniform(-2, 8, N))
    afs = np.exp(rng.uniform(np.log(1e-4), np.log(3e-2), N))
    mafs, nmafs = np.full(N, 0.5), np.full(N, 0.5)
    low = rng.random(N) < 0.2
    mafs[low] = rng.uniform(0.1, 0.5, int(low.sum()))
    seq = -alts * rng.uniform(1.0, 5.0, N)
    nseq = -nalts * rng.uniform(2, 6, N)
    haps = rng.integers(0, 4, (N, 2 * SEQ))
    haps[rng.random((N, 2 * SEQ)) < 0.02] = 4
    # the SNV rows' contexts: a skewed distribution over the 192 bins, every bin at least once, none more than MAX_PER_BIN times
    centre, alt_centre = (SEQ - 1) // 2, (SEQ - 1) // 2 + SEQ
    bins = [(lf, ref, rf, alt) for lf in range(4) for ref in range(4) for rf in range(4) for alt in range(4) if ref != alt]
    weight = np.exp(0.8 * rng.standard_normal(len(bins)))
    snv_rows = np.flatnonzero(types_b == 0)
    assert len(snv_rows) >= len(bins)
    chosen = list(rng.permutation(len(bins)))
    used = np.ones(len(bins), dtype=np.int64)
    while len(chosen) < len(snv_rows):
        j = int(rng.choice(len(bins), p=weight / weight.sum()))
        if used[j] < MAX_PER_BIN:
            used[j] += 1
            chosen.append(j)
    for row, j in zip(snv_rows, rng.permutation(np.array(chosen))):
        haps[row, centre - 1], haps[row, centre], haps[row, centre + 1], haps[row, alt_centre] = bins[j]
    for row, pos in zip(snv_rows[:12], [centre - 1, centre, centre + 1, alt_centre] * 3):  # SNV rows whose bin the conversion drops
        haps[row, pos] = 4
    ints = np.zeros((N, 16 + 2 * SEQ), dtype=np.int16)
    floats = np.zeros((N, 6 + 2), dtype=np.float16)
    for field, col in ((Data.VARIANT_TYPE, types_b), (Data.ORIGINAL_DEPTH, depths), (Data.ORIGINAL_ALT_COUNT, alts),
                       (Data.ORIGINAL_NORMAL_DEPTH, ndepths), (Data.ORIGINAL_NORMAL_ALT_COUNT, nalts)):
        ints[:, field.idx] = col
    ints[:, Data.ALT_COUNT.idx] = 1
    ints[:, 16:] = haps
    for field, col in ((Data.SEQ_ERROR_LOG_LK, seq), (Data.NORMAL_SEQ_ERROR_LOG_LK, nseq), (Data.ALLELE_FREQUENCY, afs), (Data.MAF, mafs),
                       (Data.NORMAL_MAF, nmafs), (Data.CACHED_ARTIFACT_LOGIT, logits)):
        floats[:, field.idx] = col
    assert set(np.unique(types_b)) == {0, 1, 2, 3, 4} and (nalts <= ndepths).all() and np.isfinite(floats.astype(np.float64)).all()
    return ints, floats


def batches_of(data, batch_size, dtype):
    out = []
    for first in range(0, N, batch_size):
        b = Batch(data[first:min(first + batch_size, N)])
        b.float_tensor = b.float_tensor.to(dtype)
        out.append(b)
    return out


def raw_parameters(model):
    s = model.spectra
    som, art, na = s.somatic_spectrum.parametrizations, s.artifact_spectra.parametrizations, s.normal_artifact_spectra
    return [som.cf_k.original, som.log_weights_k.original, art.alpha_dv.original, art.beta_dv.original,
            na.normal_spectrum.parametrizations.alpha_dv.original, na.normal_spectrum.parametrizations.beta_dv.original,
            na.parametrizations.mean_multiplier_v.original, na.parametrizations.concentration_v.original]


def flat_raw(model):
    return torch.cat([p.detach().reshape(-1) for p in raw_parameters(model)]).numpy().copy()


def make_model(dtype):
    torch.set_default_dtype(torch.float32)  # the parameters start as the reference's float32 ones, whatever they become
    model = PosteriorModel(-10.0, -10.0, no_germline_mode=False, device=CPU, het_beta=None)
    model = model.to(dtype)
    model._dtype = model.spectra._dtype = dtype
    torch.set_default_dtype(dtype)
    return model


def near_half_integer(x):
    return float(np.abs(np.abs(x - np.floor(x)) - 0.5).min())


def run_case(data, iterations, dtype, ratio):
    """the reference's learn_priors_and_spectra; returns what every epoch's M step was given and left behind, or None if a total of a
    context epoch is too close to a half-integer"""
    model = make_model(dtype)
    rec = {k: [] for k in ("totals_tc", "log_priors_vc", "raw", "table", "context_epochs", "somatic_totals", "context_totals", "n_sc", "k_sc",
                           "log_rates", "grad")}
    original = model.priors.update_priors_m_step
    state = {"ok": True, "margin": 1.0}
    from permutect.architecture.posterior_model_priors import convert_rrra_tensor_to_sc

    def recording(posterior_totals_vc, somatic_snv_totals_rrra, snv_context_totals_rrra, ignored_to_non_ignored_ratio):
        context = model.priors.use_context_dependent_snv_priors
        fits_before = len(Recorder.fits)
        rec["totals_tc"].append(posterior_totals_vc.detach().numpy().copy())
        if context:
            som = convert_rrra_tensor_to_sc(somatic_snv_totals_rrra).numpy().astype(np.float64)
            ignored = ignored_to_non_ignored_ratio * torch.sum(posterior_totals_vc).item() / 64
            margin = min(near_half_integer(som), near_half_integer(np.array([ignored])))
            state["margin"] = min(state["margin"], margin)
            if margin < MARGIN:
                state["ok"] = False
            rec["context_epochs"].append(len(rec["totals_tc"]) - 1)
            rec["somatic_totals"].append(somatic_snv_totals_rrra.numpy().copy())
            rec["context_totals"].append(snv_context_totals_rrra.numpy().copy())
        original(posterior_totals_vc, somatic_snv_totals_rrra, snv_context_totals_rrra, ignored_to_non_ignored_ratio)
        if context:
            assert len(Recorder.fits) == fits_before + 1
            fit = Recorder.fits[-1]
            rec["n_sc"].append(fit["n"]), rec["k_sc"].append(fit["k"]), rec["log_rates"].append(fit["log_p"]), rec["grad"].append(fit["grad"])
        rec["log_priors_vc"].append(model.priors.log_priors_vc.detach().numpy().copy())
        rec["raw"].append(flat_raw(model))
        rec["table"].append(model.priors.somatic_snv_log_priors_rrra.detach().numpy().copy())

    model.priors.update_priors_m_step = recording
    first_average = len(RecordingAverage.made)
    model.learn_priors_and_spectra(batches_of(data, 64, dtype), iterations, ratio, summary_writer=None, learning_rate=0.001)
    averages = RecordingAverage.made[first_average:]
    assert len(averages) == iterations and all(a._count == N for a in averages)
    rec["losses"] = [a._sum / a._count for a in averages]
    assert rec["context_epochs"] == [e for e in range(iterations) if e + 1 > iterations / 2], rec["context_epochs"]
    assert model.priors.use_context_dependent_snv_priors
    return (rec if state["ok"] else None), state["margin"]


def synthetic(seed, exposure, rate, het, zero_cells=0):
    rng = np.random.default_rng(seed)
    true = rate * np.exp(het * rng.standard_normal((12, 16))) * np.exp(het * rng.standard_normal((12, 1)))
    n = np.round(exposure * rng.uniform(0.5, 1.5, (12, 16)))
    if zero_cells:
        n.reshape(-1)[rng.choice(192, zero_cells, replace=False)] = 0
    k = rng.binomial(n.astype(np.int64), np.minimum(true, 1))
    return n.astype(np.int64), k.astype(np.int64)


def main():
    torch.set_num_threads(4)
    ratio = (GENOMIC_SPAN - N) / N
    seed = int(os.environ.get("CONTEXT_GOLDEN_FIRST_SEED", 20250101))
    while True:
        ints, floats = inputs(seed)
        data = [Datum(ints[i], floats[i], np.zeros((1, 12), dtype=np.uint8), compressed=True) for i in range(N)]
        cases, ok = {}, True
        for iterations in ITERATIONS:
            for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                cases[iterations, tag], margin = run_case(data, iterations, dtype, ratio)
                print(f"seed {seed}: {iterations} iteration(s) {tag}: nearest half-integer {margin:.2e}", flush=True)
                if cases[iterations, tag] is None:
                    ok = False
                    break
            if not ok:
                break
        if ok:
            break
        seed += 1
    torch.set_default_dtype(torch.float32)

    whole = Batch(data)
    idx = get_ref_contexts_and_alt_bases(whole)
    out = {"seed": np.int64(seed), "ratio": np.float64(ratio), "genomic_span": np.float64(GENOMIC_SPAN), "margin": np.float64(MARGIN),
           "contexts": (((idx[0] * 5 + idx[1].long()) * 5 + idx[2]) * 5 + idx[3]).numpy().astype(np.int32)}
    for name, field in (("variant_types", Data.VARIANT_TYPE), ("depths", Data.ORIGINAL_DEPTH), ("alt_counts", Data.ORIGINAL_ALT_COUNT),
                        ("normal_depths", Data.ORIGINAL_NORMAL_DEPTH), ("normal_alt_counts", Data.ORIGINAL_NORMAL_ALT_COUNT)):
        out[name] = whole.get(field).numpy().astype(np.int32)
    for name, field in (("seq_error_log_lks", Data.SEQ_ERROR_LOG_LK), ("normal_seq_error_log_lks", Data.NORMAL_SEQ_ERROR_LOG_LK),
                        ("allele_frequencies", Data.ALLELE_FREQUENCY), ("mafs", Data.MAF), ("normal_mafs", Data.NORMAL_MAF),
                        ("artifact_logits", Data.CACHED_ARTIFACT_LOGIT)):
        out[name] = whole.get(field).float().numpy().astype(np.float32)
    snv = out["variant_types"] == 0
    per_bin = np.bincount(out["contexts"][snv], minlength=625)
    assert per_bin.max() <= MAX_PER_BIN and (np.array([(c // 125 == 4) or (c // 25 % 5 == 4) or (c // 5 % 5 == 4) or (c % 5 == 4)
                                                       for c in out["contexts"][snv]])).sum() >= 12
    out["iterations"] = np.array(ITERATIONS, dtype=np.int64)
    for (iterations, tag), rec in cases.items():
        for key, value in rec.items():
            out[f"it{iterations}_{tag}_{key}"] = np.array(value, dtype=np.int64 if key in ("context_epochs", "n_sc", "k_sc") else np.float64)
        k_last = rec["k_sc"][-1]
        print(f"{iterations} iteration(s) {tag}: losses {rec['losses']}; last fit: sum k {int(k_last.sum())}, cells with k >= 1: {int((k_last >= 1).sum())}, "
              f"max |dF| / sum k {rec['grad'][-1]:.1e}")
        assert (k_last >= 1).sum() >= 48

    # ---- six fit problems of their own: the captured counts of the three float64 cases' last context epoch, a WGS-like one, one
    # without a single somatic SNV, one with cells that no site falls into
    problems = {f"captured{iterations}": (cases[iterations, "f64"]["n_sc"][-1], cases[iterations, "f64"]["k_sc"][-1]) for iterations in ITERATIONS}
    problems["wgs"] = synthetic(1, 4.7e7, 2e-6, 0.7)
    n_zero = synthetic(3, 1e5, 0.0, 0.0)
    problems["all_zero"] = (n_zero[0], np.zeros_like(n_zero[1]))
    problems["empty_cells"] = synthetic(2, 2e4, 5e-5, 0.7, zero_cells=9)
    out["fit_names"] = np.array(list(problems))
    for name, (n, k) in problems.items():
        log_p, grad = maximise(n, k)
        out[f"fit_{name}_n"], out[f"fit_{name}_k"], out[f"fit_{name}_log_p"], out[f"fit_{name}_grad"] = n, k, log_p, np.float64(grad)
        print(f"fit {name}: sum n {int(n.sum())}, sum k {int(k.sum())}, cells with n = 0: {int((n == 0).sum())}, log p in [{log_p.min():.3f}, {log_p.max():.3f}], "
              f"max |dF| / max(sum k, 1) {grad:.1e}")
    path = os.path.join(HERE, "context_priors.npz")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes; seed", seed)


if __name__ == "__main__":
    main()
