"""The training step's small kernels alone -- pmt_phi_forward / pmt_phi_backward (csrc/pmt_phi.hip), pmt_clip_adamw (csrc/pmt_optim.hip),
pmt_losses_forward / pmt_losses_backward and pmt_record_losses (csrc/pmt_losses.hip) -- through the C ABI, against float64, at the edges
of their launch arithmetic and of their inputs.  tests/step_kernel_cases.py holds the tables, the references, the float32 yardsticks and
the mirrors; tests/test_step_kernels_cpu.py holds the references against torch itself and the mirrors against these bounds.

The harness owns every buffer: each output and each in-place buffer sits between guard words (SENTINEL) that must still stand after every
call, the integer columns are columns of an [n, 19] int64 array full of junk (or dense, or int32), the segments of a phi program lie apart
from each other with sentinels in the gaps of `phi` and `grad_theta`, `scratch` is 1024 sentinels of which only the launched workgroups'
slots and the step slot may change, the histogram table has guard words before and behind its 6 x bins floats.  Refused calls leave
every buffer untouched.

Held to what (tests/step_kernel_cases.py derives each bound; none is read off a device):
  phi        forward |err| <= 2^-23 x max(1, max|ref|) per segment, adjoint |err| <= 2^-22 x max|g_ref|, |Q Q^T - I| <= 4 x 2^-23 x N; EXP and
             BOUNDED, float32 chains behind `expf`, + 2 x the float32 yardstick.  Orthogonal N = 1 .. 32 (33 refused), X = 0 (exactly the
             identity / `base`), |A|_1 exactly 0.5 and one float above (s = 0 / 1), exactly 1 and 8 (the scaled norm exactly 0.5 under one and
             four squarings: the series' worst case, which is where the 7-term mutant of the CPU test is caught), 0.3 and 3 sigma; upstream
             1e-3, 1, 1e3; base NULL, row-major, a transposed view.  The adjoint accumulates: into a prefilled grad_theta the result is
             prefill + increment to one ulp of the larger of the sum and its terms (`gx += gy * y` may contract into one fused
             multiply-add), twice gives twice, an orthogonal segment's diagonal and upper triangle are never written.
  clip+AdamW grad_norm 5e-7 relative; m, v within 6 / 10 x 2^-24 of the sum of the magnitudes of their two terms; theta within
             1.25 x (2 ulp32 + 2e-5 |Adam term|): n = 0 .. 600 001 (one workgroup, a partial last one, the 256-workgroup cap, the grid-stride
             second pass), steps 1 .. 100 000 from a non-zero state, lr, weight decay, norms below and above the clip, no clip, no norm out,
             a zero gradient; PMT_STEP_ON_DEVICE bit for bit the explicit steps 1, 2, 3; n = 0 leaves the step slot alone.
  losses     rtol 2e-5, atol 2e-6 x max(1, largest |input logit| of the row); input gradients rtol 2e-4, atol 2e-6 x max|upstream| x the same:
             n = 0 .. 1000, K = 0 .. 16 (17 refused), S = 1 .. 7, strided and dense int64 columns, an edge block of ninety rows, each
             upstream pointer NULL in turn; the rows that must be exactly zero are exactly zero.
  recorder   every cell rtol 1e-5 + 1e-5 of its histogram's largest cell, every count histogram's total 1e-6: n = 1 .. 5000 (twenty
             workgroups into one table, twice), 300 / 600 / 1800 bins (2100 refused), int32 dense and int64 strided columns.

What the table found: no defect of the four kernels' arithmetic.  Two things it made visible without a device: BOUNDED's adjoint
`s * (1 - s)` loses every digit where the sigmoid saturates (x = 16.2: 28 % off a gradient of 7.9e-7; float32 torch does the same bit for
bit, so it is parity with the reference and not changed), and float32 torch's own gradient norm is 3e-5 off on 600 001 heavy-tailed
gradients where the kernel's float64 partial sums are exact to float32 rounding.  One guard came with it: `expm_inplace` now takes no
squarings for a non-finite norm and at most 1100 (never fed on a device: the mirror and the CPU test carry that case).

Measured on an MI355X (the bounds are not tightened to these): the matrix exponential at most 3.0e-8 from float64 (N = 32, 3 sigma: 0.25 of its
bound) where float32 torch.linalg.matrix_exp is up to 2.5e-5 off, its adjoint at most 5.7e-8 of the gradient's largest entry (0.24 of its bound;
float32 torch up to 9.7e-4), Q Q^T - I at most 0.11 of its bound; EXP / BOUNDED / UNIT_ROWS / LOG_SOFTMAX forward 0.22 / 0.30 / 0.30 / 0.37 and
adjoint 0.10 / 0.50 / 0.18 / 0.09 of theirs (BOUNDED's 0.50 is the saturated 1 x 1 case, equal to float32 torch to the bit); the optimizer's norm
0.13, m 0.49, v 0.48 and theta 0.48 of their bounds -- the numpy mirror's own figures to the digit -- with float32 torch at 102, 143, 171 and 404 of
them once its float32 norm is 3e-5 off (n = 600 001); losses 0.012 and input gradients 0.043 of their bounds (float32 torch 0.070 / 0.047), no
edge row dropped; recorder cells 0.013 of theirs.  Every measured (error, yardstick) pair goes through `record()`
(tests/test_scale_gpu.py); profiles/step_kernels_parity.jsonl is one run's lines, DESIGN section 2 quotes the largest.  The file runs in
four seconds (145 tests; the first call of the process 1.2 s, every other test at most 0.13 s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from permutect_amd.data.datum import Data
from permutect_amd.engine import lib as L
from tests import step_kernel_cases as K
from tests.test_scale_gpu import record  # (appends a line to the suite's file of measured errors)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.5
PAD = 7                 # guard words on both sides of every buffer the kernels write
JUNK = 777.0
f32, f64 = np.float32, np.float64


def lib():
    return L.load()


def sync():
    torch.cuda.synchronize()


def dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


class Guarded:
    """`n` elements on the device between PAD guard words on each side; `init`: the elements' first content (default: the sentinel)"""

    def __init__(self, n, init=None, dtype=torch.float32):
        self.n = int(n)
        self.whole = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.whole[PAD:PAD + self.n]
        if init is not None:
            self.view.copy_(dev(init, dtype).reshape(-1))
        self.before = self.whole.clone()

    @property
    def ptr(self):
        return self.whole.data_ptr() + PAD * self.whole.element_size()  # (an empty view's own data_ptr() is NULL)

    def guards_stand(self):
        assert bool((self.whole[:PAD] == SENTINEL).all()) and bool((self.whole[PAD + self.n:] == SENTINEL).all()), "a guard word was overwritten"

    def untouched(self):
        assert torch.equal(self.whole.view(torch.int32), self.before.view(torch.int32)), "a refused / empty call wrote to a buffer"

    def numpy(self):
        self.guards_stand()
        return self.view.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


# =====================================================================================================================================
# phi
# =====================================================================================================================================
class PhiRun:
    """a program over `segs`, its segments apart from each other: gaps of 3 floats in theta / grad_theta and of 5 in phi / grad_phi"""

    def __init__(self, segs):
        self.segs = segs
        self.prog = L.PmtPhiProgram()
        self.prog.n_segs = len(segs)
        self.keep = []
        t_off, p_off, self.t_offs, self.p_offs = 2, 4, [], []
        for i, s in enumerate(segs):
            sg = self.prog.seg[i]
            sg.kind, sg.theta_off, sg.phi_off, sg.rows, sg.cols, sg.p0, sg.p1 = s.kind, t_off, p_off, s.rows, s.cols, s.p0, s.p1
            if s.base_array is not None:
                b = dev(s.base_array)
                self.keep.append(b)
                sg.base, sg.base_rs, sg.base_cs = b.data_ptr(), s.base_rs, s.base_cs
            self.t_offs.append(t_off)
            self.p_offs.append(p_off)
            t_off, p_off = t_off + s.x.size + 3, p_off + s.x.size + 5
        self.t_size, self.p_size = t_off, p_off
        theta, gphi = np.full(self.t_size, JUNK, f32), np.full(self.p_size, JUNK, f32)
        for s, a, b in zip(segs, self.t_offs, self.p_offs):
            theta[a:a + s.x.size], gphi[b:b + s.x.size] = s.x.ravel(), s.gy.ravel()
        self.theta, self.gphi = dev(theta), dev(gphi)

    def mask(self, offs, size):
        m = np.zeros(size, bool)
        for s, a in zip(self.segs, offs):
            m[a:a + s.x.size] = True
        return m

    def split(self, flat, offs):
        return [flat[a:a + s.x.size].reshape(s.x.shape) for s, a in zip(self.segs, offs)]

    def forward(self):
        self.phi = Guarded(self.p_size)
        assert lib().pmt_phi_forward(C.byref(self.prog), self.theta.data_ptr(), self.phi.ptr, L.raw_stream()) == 0
        sync()
        out = self.phi.numpy()
        assert (out[~self.mask(self.p_offs, self.p_size)] == SENTINEL).all(), "phi written outside the segments"
        return self.split(out, self.p_offs)

    def backward(self, prefill=None, times=1):
        """grad_theta after `times` calls: the segments start from `prefill` (flat, theta-sized; default zeros), the gaps from the sentinel"""
        start = np.full(self.t_size, SENTINEL, f32)
        m = self.mask(self.t_offs, self.t_size)
        start[m] = 0.0 if prefill is None else prefill[m]
        gt = Guarded(self.t_size, start)
        for _ in range(times):
            assert lib().pmt_phi_backward(C.byref(self.prog), self.theta.data_ptr(), self.phi.ptr, self.gphi.data_ptr(), gt.ptr, L.raw_stream()) == 0
        sync()
        out = gt.numpy()
        assert (out[~m] == SENTINEL).all(), "grad_theta written outside the segments"
        grads, starts = self.split(out, self.t_offs), self.split(start, self.t_offs)
        for s, g, g0 in zip(self.segs, grads, starts):
            if s.kind == K.PHI_ORTHOGONAL:  # the diagonal and the upper triangle are never written
                up = np.triu(np.ones(s.x.shape, bool))
                assert np.array_equal(bits(g[up]), bits(g0[up])), s.id
        return grads


def check_phi(run: PhiRun, ys, gs, tag):
    worst = dict(fwd=0.0, bwd=0.0, orth=0.0, fwd_yard=0.0, bwd_yard=0.0)
    for seg, y, g in zip(run.segs, ys, gs):
        ref = K.phi_torch(seg, torch.float64)
        yard = K.phi_yardstick(seg, ref)
        fwd, fwd_bound, bwd, bwd_bound = K.phi_errors(seg, y, g, ref, yard)
        print(f"{seg.id}: forward {fwd:.3e} (float32 torch {yard[0]:.3e}, bound {fwd_bound:.3e}) adjoint {bwd:.3e} ({yard[1]:.3e}, {bwd_bound:.3e})")
        record(test="step_kernels/phi", case=seg.id, tag=tag, forward_err=fwd, forward_yardstick=yard[0], forward_bound=fwd_bound,
               adjoint_err=bwd, adjoint_yardstick=yard[1], adjoint_bound=bwd_bound)
        assert np.isfinite(y).all() and np.isfinite(g).all(), seg.id
        assert fwd <= fwd_bound, (seg.id, fwd, fwd_bound)
        assert bwd <= bwd_bound, (seg.id, bwd, bwd_bound)
        worst["fwd"], worst["bwd"] = max(worst["fwd"], fwd / fwd_bound), max(worst["bwd"], bwd / bwd_bound if bwd_bound else 0.0)
        if seg.kind == K.PHI_ORTHOGONAL:
            q = y.astype(f64) if seg.base is None else seg.base.astype(f64).T @ y.astype(f64)
            orth = np.abs(q @ q.T - np.eye(seg.rows)).max()
            assert orth <= K.PHI_ORTH_TOL * seg.rows, (seg.id, orth)
            worst["orth"] = max(worst["orth"], orth / (K.PHI_ORTH_TOL * seg.rows))
            if seg.id.split("-")[2] == "zero":  # X = 0: exactly the identity, or exactly `base`
                assert np.array_equal(y, np.eye(seg.rows, dtype=f32) if seg.base is None else seg.base), seg.id
    return worst


@pytest.mark.parametrize("n", K.ORTHO_NS)
def test_phi_orthogonal(n):
    for layout in K.ORTHO_BASES:
        run = PhiRun(K.ortho_segs(n, layout))
        ys = run.forward()
        worst = check_phi(run, ys, run.backward(), "orthogonal")
        record(test="step_kernels/phi_orthogonal_worst", n=n, base=layout, **{k: v for k, v in worst.items() if "yard" not in k})


def test_phi_elementwise_kinds():
    run = PhiRun(K.elementwise_segs())
    ys = run.forward()
    check_phi(run, ys, run.backward(), "elementwise")


def test_phi_program_of_48_segments_and_the_adjoint_accumulates():
    segs = K.mixed_program_segs()
    assert len(segs) == L.MAX_PHI_SEGS == K.MAX_PHI_SEGS and {s.kind for s in segs} == set(range(5))
    run = PhiRun(segs)
    ys = run.forward()
    inc = run.backward()
    check_phi(run, ys, inc, "mixed-48")
    # each segment alone gives the same bits as in the program of 48
    for i in (0, 6, 13, 20, 47):
        one = PhiRun([segs[i]])
        assert np.array_equal(bits(one.forward()[0]), bits(ys[i])) and np.array_equal(bits(one.backward()[0]), bits(inc[i])), segs[i].id
    # into a prefilled grad_theta: prefill + increment, to one ulp of the larger of the sum and its terms
    prefill = K.rng_of("prefill").standard_normal(run.t_size).astype(f32)
    got = run.backward(prefill=prefill)
    twice = run.backward(times=2)
    for seg, g, g2, i0, p in zip(segs, got, twice, inc, run.split(prefill, run.t_offs)):
        low = np.tril(np.ones(seg.x.shape, bool), -1) if seg.kind == K.PHI_ORTHOGONAL else np.ones(seg.x.shape, bool)
        want = p.astype(f64) + i0.astype(f64)
        tol = K.ulp32(np.maximum(np.abs(want), np.maximum(np.abs(p), np.abs(i0))))
        assert (np.abs(g.astype(f64) - want)[low] <= tol[low]).all(), seg.id
        assert (np.abs(g2.astype(f64) - 2.0 * i0.astype(f64))[low] <= K.ulp32(2.0 * i0)[low]).all(), seg.id


def _phi_buffers(size=4096):
    return [Guarded(size) for _ in range(4)]


def test_phi_refusals_leave_the_buffers_untouched():
    theta, phi, gphi, gtheta = bufs = _phi_buffers()
    st = L.raw_stream()

    def both(prog):
        rcs = (lib().pmt_phi_forward(C.byref(prog), theta.ptr, phi.ptr, st),
               lib().pmt_phi_backward(C.byref(prog), theta.ptr, phi.ptr, gphi.ptr, gtheta.ptr, st))
        sync()
        for b in bufs:
            b.untouched()
        return rcs

    def ortho(n):
        prog = L.PmtPhiProgram()
        prog.n_segs = 1
        sg = prog.seg[0]
        sg.kind, sg.rows, sg.cols = L.PHI_ORTHOGONAL, n, n
        return prog

    assert both(ortho(L.MAX_ORTHO_DIM + 1)) == (L.E_UNSUPPORTED, L.E_UNSUPPORTED)  # N = 33
    prog = ortho(4)
    prog.seg[0].kind = 5
    assert both(prog) == (L.E_INVALID, L.E_INVALID)
    prog = ortho(4)
    prog.n_segs = L.MAX_PHI_SEGS + 1  # 49 segments (refused before any is read)
    assert both(prog) == (L.E_INVALID, L.E_INVALID)
    prog = ortho(4)
    prog.n_segs = 0  # launches nothing
    assert both(prog) == (0, 0)
    prog = ortho(4)
    assert lib().pmt_phi_forward(C.byref(prog), None, phi.ptr, st) == L.E_INVALID and lib().pmt_phi_forward(C.byref(prog), theta.ptr, None, st) == L.E_INVALID
    assert lib().pmt_phi_backward(C.byref(prog), theta.ptr, phi.ptr, gphi.ptr, None, st) == L.E_INVALID
    sync()
    for b in bufs:
        b.untouched()


# =====================================================================================================================================
# clip + AdamW
# =====================================================================================================================================
def adamw_hyper(hyper, step):
    return L.PmtAdamW(lr=hyper["lr"], beta1=hyper["beta1"], beta2=hyper["beta2"], eps=hyper["eps"], weight_decay=hyper["weight_decay"],
                      max_grad_norm=hyper["max_grad_norm"], step=step)


class AdamWRun:
    def __init__(self, theta, g, m, v):
        self.n = len(theta)
        self.theta, self.g, self.m, self.v = Guarded(self.n, theta), Guarded(self.n, g), Guarded(self.n, m), Guarded(self.n, v)
        self.scratch = Guarded(K.SCRATCH_FLOATS)
        self.norm = Guarded(1)

    def set_step_slot(self, value):
        self.scratch.view.view(torch.int32)[K.STEP_SLOT] = value

    def step_slot(self):
        return int(self.scratch.view.view(torch.int32)[K.STEP_SLOT].item())

    def call(self, hyper, step, norm_out=True, on_device=False):
        hp = adamw_hyper(hyper, K.STEP_ON_DEVICE if on_device else step)
        rc = lib().pmt_clip_adamw(self.theta.ptr, self.g.ptr, self.m.ptr, self.v.ptr, self.n, C.byref(hp), self.scratch.ptr,
                                  self.norm.ptr if norm_out else None, L.raw_stream())
        sync()
        assert rc == 0
        # the gradient is read only; of scratch only the launched workgroups' slots (and the step slot, on the device) change
        self.g.untouched()
        scratch, blocks = self.scratch.numpy(), K.opt_launched_blocks(self.n)
        rest = np.ones(K.SCRATCH_FLOATS, bool)
        rest[:blocks] = False
        rest[K.STEP_SLOT] = False
        assert (scratch[rest] == SENTINEL).all(), "scratch written beyond the launched workgroups' slots"
        assert (scratch[:blocks] >= 0).all()
        if not on_device:
            assert scratch[K.STEP_SLOT] == SENTINEL
        if not norm_out:
            self.norm.untouched()
        return self.theta.numpy(), self.m.numpy(), self.v.numpy(), float(self.norm.numpy()[0]), scratch[:blocks].copy()


@pytest.mark.parametrize("case", K.opt_cases(), ids=lambda c: c.id)
def test_clip_adamw(case):
    theta, g, m, v, hyper, step = K.opt_inputs(case)
    run = AdamWRun(theta, g, m, v)
    if case.n == 0:
        hp = adamw_hyper(hyper, step)
        assert lib().pmt_clip_adamw(run.theta.ptr, run.g.ptr, run.m.ptr, run.v.ptr, 0, C.byref(hp), run.scratch.ptr, run.norm.ptr, L.raw_stream()) == 0
        sync()
        for b in (run.theta, run.g, run.m, run.v, run.scratch, run.norm):
            b.untouched()
        return
    th, m2, v2, norm, partial = run.call(hyper, step, norm_out=case.norm != "null")
    ref = K.adamw_reference(theta, g, m, v, hyper, step)
    if case.norm == "null":
        norm = float(np.sqrt(partial.astype(f64).sum()))  # (the partial sums are there all the same)
    errs = K.opt_errors(ref, theta, th, m2, v2, norm)
    y = K.adamw_torch(theta, g, m, v, hyper, step, torch.float32)
    yard = K.opt_errors(ref, theta, *y)
    print(f"{case.id}: error / bound {errs}; float32 torch {yard}")
    record(test="step_kernels/clip_adamw", case=case.id, blocks=len(partial), **{f"{k}_err_over_bound": e for k, e in errs.items()},
           **{f"{k}_yardstick_over_bound": e for k, e in yard.items()})
    assert np.isfinite(th).all() and np.isfinite(m2).all() and np.isfinite(v2).all()
    assert abs(float(np.sqrt(partial.astype(f64).sum())) - ref["norm"]) <= K.OPT_NORM_TOL * ref["norm"]
    for k, e in errs.items():
        assert e <= 1.0, (case.id, k, e)
    coef = min(hyper["max_grad_norm"] / (ref["norm"] + 1e-6), 1.0) if hyper["max_grad_norm"] > 0 else 1.0
    assert (coef == 1.0) == (case.norm in ("below", "off") or case.state == "zero_grad")
    if case.state == "zero_grad":  # m and v stay zero, theta only decays
        assert norm == 0.0 and not m2.any() and not v2.any()
        assert np.abs(th.astype(f64) - theta.astype(f64) * (1 - hyper["lr"] * hyper["weight_decay"])).max() <= K.ulp32(theta).max()


@pytest.mark.parametrize("n", [257, 262145])
def test_clip_adamw_step_on_device_is_the_explicit_steps_bit_for_bit(n):
    theta, g, m, v, hyper, _ = K.opt_inputs(K.OptCase(n))
    explicit, device = AdamWRun(theta, g, m, v), AdamWRun(theta, g, m, v)
    device.set_step_slot(0)
    for step in (1, 2, 3):
        a = explicit.call(hyper, step)
        b = device.call(hyper, 0, on_device=True)
        assert device.step_slot() == step
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(bits(x), bits(y)), step
        assert a[3] == b[3]
    # n = 0 launches nothing: the step slot is left alone (include/permutect_amd.h: an empty update is not a step)
    hp = adamw_hyper(hyper, K.STEP_ON_DEVICE)
    before = device.scratch.whole.clone()
    assert lib().pmt_clip_adamw(device.theta.ptr, device.g.ptr, device.m.ptr, device.v.ptr, 0, C.byref(hp), device.scratch.ptr, None, L.raw_stream()) == 0
    sync()
    assert device.step_slot() == 3 and torch.equal(before.view(torch.int32), device.scratch.whole.view(torch.int32))


def test_clip_adamw_refusals_leave_the_buffers_untouched():
    theta, g, m, v, hyper, _ = K.opt_inputs(K.OptCase(257))
    run = AdamWRun(theta, g, m, v)
    hp, st = adamw_hyper(hyper, 1), L.raw_stream()
    good = [run.theta.ptr, run.g.ptr, run.m.ptr, run.v.ptr, run.n, C.byref(hp), run.scratch.ptr, run.norm.ptr, st]
    calls = []
    for i in (0, 1, 2, 3, 5, 6):  # theta, grad, exp_avg, exp_avg_sq, hyper, scratch
        calls.append(good[:i] + [None] + good[i + 1:])
    calls.append(good[:4] + [-1] + good[5:])
    calls.append(good[:5] + [C.byref(adamw_hyper(hyper, 0))] + good[6:])
    calls.append(good[:5] + [C.byref(adamw_hyper(hyper, -2))] + good[6:])
    for args in calls:
        assert lib().pmt_clip_adamw(*args) == L.E_INVALID
    sync()
    for b in (run.theta, run.g, run.m, run.v, run.scratch, run.norm):
        b.untouched()


# =====================================================================================================================================
# losses
# =====================================================================================================================================
class LossRun:
    def __init__(self, li: K.LossInputs, columns="strided", with_sources=True):
        self.li, n = li, li.n
        self.keep = [dev(a) for a in (li.logits_b, li.logits_bk, li.alt_count_raw, li.source_logits, li.weights, li.source_weights)]
        a = self.args = L.PmtLossArgs()
        a.num_variants, a.num_clusters, a.num_sources = n, li.k, li.s
        a.max_outlier_logit, a.max_alt_count = K.MAX_OUTLIER_LOGIT, K.MAX_ALT_COUNT
        a.logits_b, a.logits_bk, a.alt_count_raw, src, a.weights, a.source_weights = [t.data_ptr() if t.numel() else SENTINEL_PTR.ptr for t in self.keep]
        a.source_logits = src if with_sources else None
        if columns == "strided":  # columns of the [n, 19] array, junk everywhere else
            ints = dev(li.ints)
            self.keep.append(ints)
            cols = [ints[:, c] for c in (K.LABEL_COL, K.ALT_COUNT_COL, K.SOURCE_COL)]
            a.label_stride = a.alt_count_stride = a.source_stride = K.INT_COLS
        else:
            cols = [dev(li.ints[:, c]) for c in (K.LABEL_COL, K.ALT_COUNT_COL, K.SOURCE_COL)]
            self.keep.extend(cols)
            a.label_stride = a.alt_count_stride = a.source_stride = 1
        a.labels, a.alt_counts, a.sources = [c.data_ptr() if c.numel() else SENTINEL_PTR.ptr for c in cols]

    def forward(self):
        n = self.li.n
        outs = [Guarded(n) for _ in K.LOSS_VECS]
        o = L.PmtLossOutputs(*[b.ptr for b in outs])
        assert lib().pmt_losses_forward(C.byref(self.args), C.byref(o), L.raw_stream()) == 0
        sync()
        return [b.numpy() for b in outs]

    def backward(self, upstream, d_source_logits=True):
        li, n = self.li, self.li.n
        ups = [None if u is None else dev(u) for u in upstream]
        g = L.PmtLossOutputs(*[None if u is None else (u.data_ptr() if n else SENTINEL_PTR.ptr) for u in ups])
        grads = [Guarded(n), Guarded(n * (li.k + 2)), Guarded(n), Guarded(n * li.s)]
        d = L.PmtLossInputGrads(grads[0].ptr, grads[1].ptr, grads[2].ptr, grads[3].ptr if d_source_logits else None)
        assert lib().pmt_losses_backward(C.byref(self.args), C.byref(g), C.byref(d), L.raw_stream()) == 0
        sync()
        if not d_source_logits or li.s == 1 or not self.args.source_logits:
            grads[3].untouched()  # no source gradient is written
        return [grads[0].numpy(), grads[1].numpy().reshape(n, li.k + 2), grads[2].numpy(), grads[3].numpy().reshape(n, li.s)]


class _Ptr:
    """a valid device address for the pointers of an n = 0 call (an empty tensor's is NULL)"""

    @property
    def ptr(self):
        if not hasattr(self, "t"):
            self.t = torch.zeros(64, device=DEV)
        return self.t.data_ptr()


SENTINEL_PTR = _Ptr()


def check_losses(li, vecs, grads, upstream, tag, with_sources=True, d_source_logits=True):
    """bounds against float64 (the rows on which the float32 yardstick itself breaks one leave the tolerance check only) and the rows
    that must be exactly zero"""
    ups = li.upstream if upstream == "all" else upstream
    ref = K.losses_torch(li, torch.float64, ups, with_sources)
    yard = K.losses_torch(li, torch.float32, ups, with_sources)
    source_grad = li.s > 1 and with_sources and d_source_logits
    pick = lambda gs: list(gs[:3]) + [gs[3] if source_grad else None]  # noqa: E731
    dropped, y_loss, y_grad = K.loss_violations(li, yard[0], pick(yard[1]), ref, ups, with_sources)
    assert not dropped[li.edge_rows:].any() and dropped.sum() <= K.LOSS_MAX_DROPPED * max(li.edge_rows, 1)
    bad, w_loss, w_grad = K.loss_violations(li, vecs, pick(grads), ref, ups, with_sources)
    print(f"losses n={li.n} K={li.k} S={li.s} {tag}: error / bound {w_loss:.3f} (losses) {w_grad:.3f} (gradients); float32 torch {y_loss:.3f} {y_grad:.3f}; "
          f"{int(dropped.sum())} rows dropped")
    record(test="step_kernels/losses", n=li.n, clusters=li.k, sources=li.s, tag=tag, loss_err_over_bound=w_loss, grad_err_over_bound=w_grad,
           loss_yardstick_over_bound=y_loss, grad_yardstick_over_bound=y_grad, rows_dropped=int(dropped.sum()))
    for a in list(vecs) + [g for g in pick(grads) if g is not None]:
        assert np.isfinite(a).all()
    assert not (bad & ~dropped).any(), np.flatnonzero(bad & ~dropped)[:10]
    # ---- exactly zero -------------------------------------------------------------------------------------------------------------
    unlabeled = li.labels == K.LABEL_UNLABELED
    sup, unsup, _, src, _ = vecs
    assert not sup[unlabeled].any() and not grads[0][unlabeled].any()        # unlabeled: no supervised loss, no d_logits_b
    assert not unsup[~unlabeled].any() and not grads[1][~unlabeled].any()    # labeled: no unsupervised loss, no d_logits_bk row
    assert not grads[1][li.clip_kind == 2].any()                             # outlier logit above the clip: no d_logits_bk row
    g_unsup = (0 if ups[1] is None else ups[1].astype(f64)) + (0 if ups[4] is None else ups[4].astype(f64) * li.weights)
    at_clip = (li.clip_kind == 1) & unlabeled & (np.abs(g_unsup) > 0)
    assert (grads[1][at_clip, 1] != 0).all()                                 # exactly at the clip: torch's clamp passes the gradient
    if li.edge_rows and ups[1] is not None:
        assert at_clip.any() and ((li.clip_kind == 2) & unlabeled).any()
    if li.s == 1 or not with_sources:
        assert not src.any()                                                  # S = 1 / no source logits: the source loss is exactly 0


LOSS_CASES = [(shape, "strided") for shape in K.loss_shapes()] + [(shape, "dense") for shape in K.loss_shapes() if shape[1:] == (3, 3)]


@pytest.mark.parametrize("shape,columns", LOSS_CASES, ids=lambda v: v if isinstance(v, str) else "n%d-K%d-S%d" % v)
def test_losses(shape, columns):
    li = K.loss_inputs(*shape)
    run = LossRun(li, columns)
    vecs = run.forward()
    grads = run.backward(li.upstream)
    if li.n:
        check_losses(li, vecs, grads, "all", columns)


@pytest.mark.parametrize("shape", [(257, 3, 3), (1000, 16, 7), (257, 0, 1)], ids=lambda s: "n%d-K%d-S%d" % s)
def test_losses_optional_pointers(shape):
    li = K.loss_inputs(*shape)
    run = LossRun(li)
    vecs = run.forward()
    variants = [[None if j == i else u for j, u in enumerate(li.upstream)] for i in range(5)]   # each upstream pointer NULL in turn
    variants.append([None] * 4 + [li.upstream[4]])                                                # all but total_b
    for i, ups in enumerate(variants):
        check_losses(li, vecs, run.backward(ups), ups, f"upstream-variant-{i}")
    # d_source_logits = NULL: everything else as before
    check_losses(li, vecs, run.backward(li.upstream, d_source_logits=False), "all", "no-d_source_logits", d_source_logits=False)
    # source_logits = NULL: the source loss is exactly 0 and no source gradient is written
    run = LossRun(li, with_sources=False)
    check_losses(li, run.forward(), run.backward(li.upstream), "all", "no-source_logits", with_sources=False)


def test_losses_refusals_leave_the_buffers_untouched():
    li = K.loss_inputs(257, 3, 3)
    run = LossRun(li)
    outs = [Guarded(li.n) for _ in K.LOSS_VECS]
    grads = [Guarded(li.n), Guarded(li.n * 5), Guarded(li.n), Guarded(li.n * 3)]
    o, d = L.PmtLossOutputs(*[b.ptr for b in outs]), L.PmtLossInputGrads(*[b.ptr for b in grads])
    ups = [dev(u) for u in li.upstream]
    g = L.PmtLossOutputs(*[u.data_ptr() for u in ups])
    st = L.raw_stream()

    def refused(**changes):
        a = L.PmtLossArgs.from_buffer_copy(run.args)
        for k, val in changes.items():
            setattr(a, k, val)
        assert lib().pmt_losses_forward(C.byref(a), C.byref(o), st) == L.E_INVALID, changes
        assert lib().pmt_losses_backward(C.byref(a), C.byref(g), C.byref(d), st) == L.E_INVALID, changes

    refused(num_clusters=17)  # PMT_MAX_CLUSTERS + 1
    refused(num_clusters=-1)
    refused(num_variants=-1)
    refused(num_sources=0)
    for name in ("logits_b", "logits_bk", "alt_count_raw", "labels", "alt_counts", "weights", "source_weights", "sources"):
        refused(**{name: None})
    o_bad = L.PmtLossOutputs(outs[0].ptr, outs[1].ptr, outs[2].ptr, outs[3].ptr, None)
    assert lib().pmt_losses_forward(C.byref(run.args), C.byref(o_bad), st) == L.E_INVALID
    d_bad = L.PmtLossInputGrads(grads[0].ptr, None, grads[2].ptr, grads[3].ptr)
    assert lib().pmt_losses_backward(C.byref(run.args), C.byref(g), C.byref(d_bad), st) == L.E_INVALID
    sync()
    for b in outs + grads:
        b.untouched()


# =====================================================================================================================================
# recorder
# =====================================================================================================================================
REC_FIELDS = (("labels", Data.LABEL), ("variant_types", Data.VARIANT_TYPE), ("sources", Data.SOURCE), ("ref_counts", Data.REF_COUNT),
              ("alt_counts", Data.ALT_COUNT))


def record_args(cols, vecs, s, form, keep, null_sources=False):
    n = len(cols[Data.LABEL])
    a = L.PmtRecordArgs()
    a.num_variants, a.num_bins = n, s * K.REC_BINS_PER_SOURCE
    a.num_variant_types, a.num_ref_bins, a.num_alt_bins = len(K.DS.Variation), K.DS.NUM_REF_COUNT_BINS, K.DS.NUM_ALT_COUNT_BINS
    a.count_bin_skip, a.max_ref_count, a.max_alt_count = K.DS.COUNT_BIN_SKIP, K.DS.MAX_REF_COUNT, K.DS.MAX_ALT_COUNT
    if form == "int64-strided":  # columns of an [n, 19] int64 array, junk everywhere else
        ints = K.rng_of("record junk", n).integers(-99, 99, (n, K.INT_COLS))
        for f in cols:
            ints[:, f.idx] = cols[f]
        ints = dev(ints.astype(np.int64))
        keep.append(ints)
        tensors = {f: ints[:, f.idx] for f in cols}
    else:
        tensors = {f: dev(c.astype(np.int32)) for f, c in cols.items()}
        keep.extend(tensors.values())
    for name, f in REC_FIELDS:
        setattr(a, name, L.int_column(None if (name == "sources" and null_sources) else tensors[f]))
    for name in K.REC_VECS:
        t = dev(vecs[name])
        keep.append(t)
        setattr(a, name, t.data_ptr())
    return a


@pytest.mark.parametrize("form", ["int32-dense", "int64-strided"])
@pytest.mark.parametrize("s", K.REC_SS)
@pytest.mark.parametrize("n", K.REC_NS)
def test_record_losses(n, s, form):
    bins, keep = s * K.REC_BINS_PER_SOURCE, []
    hist = Guarded(6 * bins, np.zeros(6 * bins, f32))
    ref, yard = None, np.zeros((6, bins), f32)
    for launch in (0, 1):  # two launches into the same table accumulate
        cols, vecs = K.record_inputs(n, s, launch)
        assert Data.LABEL.idx == 2 and all(c.min() >= 0 for c in cols.values()) and cols[Data.ALT_COUNT].min() >= 1
        a = record_args(cols, vecs, s, form, keep, null_sources=(s == 1 and launch == 1))  # sources.ptr = NULL: source 0
        assert lib().pmt_record_losses(C.byref(a), hist.ptr, L.raw_stream()) == 0
        ref = K.record_reference(cols, vecs, s, ref)
        y = K.record_reference(cols, {k: v for k, v in vecs.items()}, s).astype(f32)
        yard = yard + y  # (float32 sums of the float64 per-launch tables: the table's own precision)
    sync()
    got = hist.numpy().reshape(6, bins).astype(f64)
    peak = np.abs(ref).max(axis=1, keepdims=True)
    bound = K.REC_RTOL * np.abs(ref) + K.REC_ATOL * peak
    err, yerr = np.abs(got - ref), np.abs(yard.astype(f64) - ref)
    print(f"recorder n={n} S={s} {form}: worst cell error / bound {(err / bound).max():.3e} (a float32 table {(yerr / bound).max():.3e})")
    record(test="step_kernels/record_losses", n=n, sources=s, form=form, workgroups=(n + 255) // 256, cell_err_over_bound=float((err / bound).max()),
           cell_yardstick_over_bound=float((yerr / bound).max()))
    assert (err <= bound).all()
    for h in (1, 3, 5):
        assert abs(got[h].sum() - ref[h].sum()) <= K.REC_TOTAL_RTOL * ref[h].sum()
    assert ((got == 0) == (ref == 0)).all()  # a cell nothing fell into is never written


def test_record_losses_refusals_leave_the_table_untouched():
    cols, vecs = K.record_inputs(257, 6)
    keep, st = [], L.raw_stream()
    hist = Guarded(6 * 2100, np.zeros(6 * 2100, f32))

    def rc(form="int32-dense", **changes):
        a = record_args(cols, vecs, 6, form, keep)
        for k, val in changes.items():
            setattr(a, k, val)
        return lib().pmt_record_losses(C.byref(a), hist.ptr, st), a

    assert rc(num_bins=7 * K.REC_BINS_PER_SOURCE)[0] == L.E_INVALID   # 2100 bins: seven sources do not fit
    assert rc(count_bin_skip=0)[0] == L.E_INVALID
    assert rc(num_bins=0)[0] == L.E_INVALID and rc(num_variants=-1)[0] == L.E_INVALID
    _, a = rc(num_variants=-1)
    a.num_variants = 257
    a.labels.elem_bytes = 2
    assert lib().pmt_record_losses(C.byref(a), hist.ptr, st) == L.E_INVALID
    a.labels.elem_bytes = 4
    a.weights = None
    assert lib().pmt_record_losses(C.byref(a), hist.ptr, st) == L.E_INVALID
    assert lib().pmt_record_losses(C.byref(a), None, st) == L.E_INVALID
    sync()
    hist.untouched()
