"""The reference side of tests/test_step_kernels_gpu.py, without a GPU (tests/step_kernel_cases.py holds the tables).

Held here: (1) each float64 reference equals the real thing to 1e-12 -- the phi reference against
torch.nn.utils.parametrizations.orthogonal(orthogonal_map="matrix_exp", use_trivialization=True) on a float64 nn.Linear whose base has
been advanced once, the optimizer reference against clip_grad_norm_ + torch.optim.AdamW in float64 over five steps, the losses'
restatement against the closed forms written out in numpy, the recorder's index against a loop; (2) every MIRROR (the kernels' own
arithmetic in numpy) stays within HALF of the bound the GPU test uses, on every case of the tables, so that the bounds can be met by correct
arithmetic; (3) teeth: with 7 Taylor terms instead of 12, and separately with one squaring too few, the phi mirror fails the new forward
bound on a table case, while the 7-term mutant stays inside the old 2e-6 on the old test's case (N = 10, 0.3 sigma); (4) the guard of
`expm_inplace`: a non-finite rotation parameter gives zero squarings and a non-finite result, not a loop of 2^31 products; (5) the float32
yardstick of the losses breaks a bound on at most 2 % of the edge block.

Measured here (the mirrors, as error / bound; a bound is never tightened to these, `pytest -s` prints them): orthogonal forward 0.25, adjoint
0.24, Q Q^T - I 0.11; EXP 0.38 / 0.10 and BOUNDED 0.33 / 0.50 against the plain bound + 2 x the float32 yardstick (against the plain bounds
their float32 chains reach 0.57 / 0.97 forward and BOUNDED's saturated adjoint far more, step_kernel_cases.PHI_F32_YARDSTICKS); UNIT_ROWS 0.30 /
0.18, LOG_SOFTMAX 0.37 / 0.09; the optimizer's norm 0.13, and against the issue's 4 x 2^-24 / 2 ulp + 2e-5 forms m 0.73, v 1.20, theta 0.60,
hence the widened 6 / 10 x 2^-24 and x 1.25 (0.49, 0.48, 0.48 of those).  The 7-term mutant breaks the new forward bound on 20 of the 73 orthogonal
(N, X) cases, each of them inside the old 2e-6, and is 2.9e-8 off on the old test's own case; one squaring short breaks it on 50.  The losses'
float32 yardstick breaks no bound on any row of any shape."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from tests import step_kernel_cases as K

f32, f64 = np.float32, np.float64


# ---- references equal the real thing -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 10, 32])
def test_phi_reference_is_torchs_orthogonal_parametrization(n):
    torch.manual_seed(n)
    lin = nn.Linear(n, n, bias=False, dtype=torch.float64)
    nn.utils.parametrizations.orthogonal(lin, orthogonal_map="matrix_exp", use_trivialization=True)
    orth = lin.parametrizations.weight[0]
    with torch.no_grad():
        lin.parametrizations.weight.original.copy_(0.4 * torch.randn(n, n, dtype=torch.float64))
    with nn.utils.parametrize.cached():
        _ = lin.weight
    # advance the base once: torch's own step of the trivialization (base <- the current weight, original <- 0), then move away again
    with torch.no_grad():
        w_now = lin.weight.detach().clone()
        lin.weight = w_now  # right_inverse: base <- w_now, original <- 0 (-I below the diagonal is not used by matrix_exp)
        lin.parametrizations.weight.original.copy_(0.3 * torch.randn(n, n, dtype=torch.float64))
    assert torch.allclose(orth.base, w_now, atol=1e-12) and (n == 1 or not torch.allclose(orth.base, torch.eye(n, dtype=torch.float64)))
    x = lin.parametrizations.weight.original
    gy = torch.randn(n, n, dtype=torch.float64)
    w = lin.weight
    (g_torch,) = torch.autograd.grad(w, x, gy)
    seg = K.Seg(K.PHI_ORTHOGONAL, x.detach().numpy(), gy.numpy(), base=orth.base.detach().numpy())
    y_ref, g_ref = K.phi_torch(seg, torch.float64)
    assert np.abs(y_ref - w.detach().numpy()).max() <= 1e-12
    assert np.abs(g_ref - g_torch.numpy()).max() <= 1e-12 * max(1.0, np.abs(g_ref).max())
    assert np.abs(np.triu(g_ref)).max() == 0.0  # nothing on or above the diagonal


def test_optimizer_reference_is_clip_grad_norm_and_adamw_in_float64():
    for case in (K.OptCase(1025), K.OptCase(257, lr=1e-2, weight_decay=0.0), K.OptCase(257, norm="below"), K.OptCase(257, norm="off")):
        theta, g, m, v, hyper, _ = K.opt_inputs(case)
        p = nn.Parameter(torch.tensor(theta, dtype=torch.float64))
        opt = torch.optim.AdamW([p], lr=hyper["lr"], betas=(hyper["beta1"], hyper["beta2"]), eps=hyper["eps"], weight_decay=hyper["weight_decay"])
        th, m_, v_ = theta.astype(f64), np.zeros_like(theta, f64), np.zeros_like(theta, f64)
        rng = K.rng_of("five steps", case.id)
        for step in range(1, 6):
            grad = g.astype(f64) * rng.uniform(0.5, 2.0, len(g))
            p.grad = torch.tensor(grad)
            norm = torch.sqrt((p.grad ** 2).sum()).item()
            if hyper["max_grad_norm"] > 0:
                norm = nn.utils.clip_grad_norm_([p], hyper["max_grad_norm"]).item()
            opt.step()
            ref = K.adamw_reference(th, grad, m_, v_, hyper, step)
            th, m_, v_ = ref["theta"], ref["m"], ref["v"]
            assert abs(ref["norm"] - norm) <= 1e-12 * norm
            assert np.abs(th - p.detach().numpy()).max() <= 1e-12
            assert np.abs(m_ - opt.state[p]["exp_avg"].numpy()).max() <= 1e-12
            assert np.abs(v_ - opt.state[p]["exp_avg_sq"].numpy()).max() <= 1e-12
        # and adamw_torch (one step from a given state) is the same thing
        th1, m1, v1, norm1 = K.adamw_torch(theta, g, m, v, hyper, 7, torch.float64)
        ref = K.adamw_reference(theta, g, m, v, hyper, 7)
        assert max(np.abs(th1 - ref["theta"]).max(), np.abs(m1 - ref["m"]).max(), np.abs(v1 - ref["v"]).max()) <= 1e-12
        assert abs(norm1 - ref["norm"]) <= 1e-12 * ref["norm"]


def test_losses_reference_is_the_closed_form():
    li = K.loss_inputs(257, 3, 3)
    vecs, _ = K.losses_torch(li, torch.float64)
    rows = slice(li.edge_rows, None)  # the random rows: the closed forms below are written without the overflow guards
    x, bk, raw, sl = (a.astype(f64)[rows] for a in (li.logits_b, li.logits_bk, li.alt_count_raw, li.source_logits))
    lab = li.labels[rows]
    target, labeled = 1.0 * (lab == 0) + 0.5 * (lab == 2), 1.0 * (lab != 2)
    sup = labeled * (np.log1p(np.exp(x)) - x * target)
    o = bk[:, 1] - np.log(np.exp(bk[:, 0]) + np.exp(bk[:, 2:]).sum(axis=1))
    unsup = (1 - labeled) * np.log1p(np.exp(np.minimum(o, K.MAX_OUTLIER_LOGIT)))
    alt = (1 / (1 + np.exp(-raw)) - li.alt_counts[rows] / K.MAX_ALT_COUNT) ** 2
    p = np.exp(sl) / np.exp(sl).sum(axis=1, keepdims=True)
    src = ((p - np.eye(li.s)[li.sources[rows]]) ** 2).sum(axis=1)
    total = li.weights[rows].astype(f64) * (sup + unsup + alt) + li.source_weights[rows].astype(f64) * src
    for got, want in zip(vecs, (sup, unsup, alt, src, total)):
        assert np.abs(got[rows] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    # source_logits = NULL and S = 1: the source loss is zero
    assert not K.losses_torch(li, torch.float64, with_sources=False)[0][3].any()
    assert not K.losses_torch(K.loss_inputs(257, 3, 1), torch.float64)[0][3].any()


def test_recorder_reference_index_is_the_loop():
    cols, vecs = K.record_inputs(257, 6)
    hist = K.record_reference(cols, vecs, 6)
    loop = np.zeros_like(hist)
    for i in range(257):
        r, a = min(int(cols[K.Data.REF_COUNT][i]), 10) // 3, (min(int(cols[K.Data.ALT_COUNT][i]), 15) - 1) // 3
        j = (((int(cols[K.Data.SOURCE][i]) * 3 + int(cols[K.Data.LABEL][i])) * 5 + int(cols[K.Data.VARIANT_TYPE][i])) * 4 + r) * 5 + a
        loop[3, j] += float(vecs["weights"][i])
        loop[5, j] += float(vecs["source_weights"][i])
    assert np.abs(hist[3] - loop[3]).max() <= 1e-12 and np.abs(hist[5] - loop[5]).max() <= 1e-12
    assert abs(hist[1].sum() - hist[3].sum()) <= 1e-9  # labeled + unlabeled weights are the weights
    assert K.REC_BINS_PER_SOURCE == 300


# ---- mirrors within half of every bound ------------------------------------------------------------------------------------------------
def all_phi_segs():
    segs = [s for n in K.ORTHO_NS for layout in K.ORTHO_BASES for s in K.ortho_segs(n, layout)]
    return segs + K.elementwise_segs()


def test_phi_mirror_within_half_of_every_bound():
    worst = {}
    for seg in all_phi_segs():
        y, g = K.phi_mirror(seg)
        ref = K.phi_torch(seg, torch.float64)
        fwd, fwd_bound, bwd, bwd_bound = K.phi_errors(seg, y, g, ref, K.phi_yardstick(seg, ref))
        name = K.KIND_NAMES[seg.kind]
        w = worst.setdefault(name, [0.0, 0.0, 0.0])
        w[0], w[1] = max(w[0], fwd / fwd_bound), max(w[1], (bwd / bwd_bound) if bwd_bound > 0 else float(bwd > 0))
        if seg.kind == K.PHI_ORTHOGONAL:
            q = y.astype(f64) if seg.base is None else seg.base.astype(f64).T @ y.astype(f64)
            w[2] = max(w[2], np.abs(q @ q.T - np.eye(seg.rows)).max() / (K.PHI_ORTH_TOL * seg.rows))
            if seg.id.split("-")[2] == "zero":  # X = 0: exactly the identity, or exactly base
                assert np.array_equal(y, np.eye(seg.rows, dtype=f32) if seg.base is None else seg.base), seg.id
    print("phi mirror, worst error / bound (forward, backward, orthogonality):", {k: [f"{v:.3f}" for v in w] for k, w in worst.items()})
    # EXP and BOUNDED against the plain bound + 2 x the float32 yardstick (step_kernel_cases.PHI_F32_YARDSTICKS says why); the rest
    # against the plain bounds
    for name in K.KIND_NAMES:
        assert max(worst[name]) <= 0.5, (name, worst[name])


def test_phi_mutants_are_caught_by_the_new_bound_and_missed_by_the_old_one():
    caught, missed_by_old = {"terms7": 0, "short": 0}, 0
    old_case = K.ortho_seg(10, "0.3", 1.0, "row_major")  # the old test: the model's feature_dim, 0.3 sigma, a row-major base
    for seg in [s for n in K.ORTHO_NS for s in K.ortho_segs(n, "none") if s.id.endswith("g1-none")]:
        ref = K.phi_torch(seg, torch.float64)
        for name, kw in (("terms7", dict(terms=7)), ("short", dict(squarings_short=1))):
            y, g = K.phi_mirror(seg, **kw)
            fwd, bound, _, _ = K.phi_errors(seg, y, g, ref)
            caught[name] += fwd > bound
            missed_by_old += name == "terms7" and bound < fwd <= K.PHI_OLD_FWD_TOL
    assert caught["terms7"] >= 1 and caught["short"] >= 1, caught
    assert missed_by_old >= 1  # table cases on which the 7-term series breaks the new bound and would have passed the old 2e-6
    y, g = K.phi_mirror(old_case, terms=7)
    fwd, bound, _, _ = K.phi_errors(old_case, y, g)
    print(f"7-term mutant on the old test's case: {fwd:.3e} (new bound {bound:.3e}, old bound {K.PHI_OLD_FWD_TOL:.1e}); caught on", caught, "of which inside the old bound", missed_by_old)
    assert fwd <= K.PHI_OLD_FWD_TOL  # and on the old test's own case the old bound sees nothing


def test_expm_guard_on_the_mirror():
    for bad in (np.inf, -np.inf, np.nan):
        a = np.zeros((4, 4))
        a[2, 1], a[1, 2] = bad, -bad
        out, s = K.expm_mirror(a)
        assert s == 0 and not np.isfinite(out).all()
    big = np.zeros((2, 2))
    big[1, 0], big[0, 1] = 1e300, -1e300  # finite norms stay below the cap ...
    assert K.expm_mirror(big)[1] == 998 < K.EXPM_MAX_SQUARINGS
    big[1, 0], big[0, 1] = 1e308, -1e308  # ... except where norm / 0.5 itself overflows: the cap, taken on the double before it is converted
    assert K.expm_mirror(big)[1] == K.EXPM_MAX_SQUARINGS
    assert K.expm_mirror(np.full((2, 2), 0.25))[1] == 0 and K.expm_mirror(np.full((2, 2), 0.2500001))[1] == 1


OPT_MIRROR = {}


@pytest.mark.parametrize("case", K.opt_cases(), ids=lambda c: c.id)
def test_adamw_mirror_within_half_of_every_bound(case):
    theta, g, m, v, hyper, step = K.opt_inputs(case)
    ref = K.adamw_reference(theta, g, m, v, hyper, step)
    errs = K.opt_errors(ref, theta, *K.adamw_mirror(theta, g, m, v, hyper, step))
    print("adamw mirror error / bound:", {k: f"{e:.3f}" for k, e in errs.items()})
    for k, e in errs.items():
        assert e <= 0.5, (k, e)
    if case.state == "zero_grad" and case.n:
        th, m2, v2, norm = K.adamw_mirror(theta, g, m, v, hyper, step)
        assert norm == 0 and not m2.any() and not v2.any() and np.isfinite(th).all()


# ---- the losses' float32 yardstick ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.loss_shapes(), ids=str)
def test_losses_yardstick_breaks_a_bound_on_at_most_two_percent_of_the_edge_block(shape):
    li = K.loss_inputs(*shape)
    if li.n == 0:
        return
    ref = K.losses_torch(li, torch.float64)
    yard = K.losses_torch(li, torch.float32)
    bad, worst_loss, worst_grad = K.loss_violations(li, yard[0], yard[1], ref)
    print(f"losses yardstick {shape}: dropped {int(bad.sum())} rows, worst error / bound {worst_loss:.3f} (losses) {worst_grad:.3f} (gradients)")
    assert not bad[li.edge_rows:].any()
    assert bad[:li.edge_rows].sum() <= math.floor(K.LOSS_MAX_DROPPED * li.edge_rows)
    for v in ref[0] + ref[1]:
        assert np.isfinite(v).all()
