"""The stepped form of the haplotype CNN's batch-statistics kernels (csrc/pmt_cnn_bn.hip: pmt_cnn_bn_forward_moments / _backward_moments,
pmt_cnn_bn_merge, pmt_cnn_bn_forward_full / _backward_full), alone, through the C ABI in ONE process.  Ranks are simulated: the shards of one
batch share one statistics buffer and one gradient buffer.  Every shard's moments go into its slot of a [R, 3, C] float64 buffer (what the
all-reduce of zero-padded slots gathers), the merge is called once per simulated rank -- the forward's writes the same statistics every
time, the backward's adds that rank's own BatchNorm gradients -- and the backward ADDS into the gradient buffer, so running every shard's
backward into it is the SUM all-reduce of the ranks' gradients.

Stacks, sizes, references and tolerances are those of tests/cnn_bn_cases.py; the sharded batch is held to torch's fp64 train-mode
Sequential on the WHOLE batch."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from permutect_amd.engine import lib as L
from permutect_amd.engine.runtime import _stream
from tests import cnn_bn_cases as K

pytestmark = pytest.mark.gpu


class Stepped:
    """the stepped entry points on a cnn_bn_cases.Library, over the shards (sizes, in order) of one batch"""

    def __init__(self, lib: K.Library, shards):
        self.lib, self.shards = lib, list(shards)
        self.starts = np.concatenate([[0], np.cumsum(self.shards)]).tolist()
        self.moments = {}  # (layer index, backward) -> the [R, 3, C] buffer of the last run

    def _slices(self, *tensors):
        for r, size in enumerate(self.shards):
            yield (r, *[t[self.starts[r]:self.starts[r] + size] for t in tensors])

    def _bn_indices(self):
        c = self.lib.cnn
        return [i for i in range(c.n_layers) if c.layers[i].kind == L.CNN_BATCHNORM]

    def _merge(self, i, mom, backward, stats, gtheta):
        eng, ranks = self.lib.eng, len(self.shards)
        for r, size in enumerate(self.shards):
            L.check(eng.lib.pmt_cnn_bn_merge(C.byref(eng.plan.desc), C.byref(self.lib.cnn), i, size, mom.data_ptr(), ranks, r, backward,
                                             stats.data_ptr(), gtheta, _stream()), "pmt_cnn_bn_merge")

    def forward(self, hap):
        lib, elib, n = self.lib, self.lib.eng.lib, hap.shape[0]
        assert sum(self.shards) == n
        out = torch.empty(n, lib.cnn.out_dim, dtype=torch.float32, device="cuda")
        stats = torch.zeros(max(lib.cnn.reserved[0], 4), dtype=torch.float32, device="cuda")
        for i in self._bn_indices():
            mom = torch.zeros(len(self.shards), 3, lib.cnn.layers[i].in_ch, dtype=torch.float64, device="cuda")
            for r, h in self._slices(hap):
                ws = lib.workspace(h.shape[0])
                L.check(elib.pmt_cnn_bn_forward_moments(*lib._common(h), i, stats.data_ptr(), mom[r].data_ptr(), ws.data_ptr(), ws.numel(),
                                                        _stream()), "pmt_cnn_bn_forward_moments")
            self._merge(i, mom, 0, stats, None)
            self.moments[(i, 0)] = mom
        for r, h, o in self._slices(hap, out):
            L.check(elib.pmt_cnn_bn_forward_full(*lib._common(h), o.data_ptr(), out.stride(0), stats.data_ptr(), _stream()),
                    "pmt_cnn_bn_forward_full")
        return out, stats

    def backward(self, hap, d_out, stats):
        lib, eng, elib = self.lib, self.lib.eng, self.lib.eng.lib
        eng.space.gtheta.zero_()
        gtheta = eng.space.gtheta.data_ptr()
        for i in reversed(self._bn_indices()):
            mom = torch.zeros(len(self.shards), 3, lib.cnn.layers[i].in_ch, dtype=torch.float64, device="cuda")
            for r, h, g in self._slices(hap, d_out):
                ws = lib.workspace(h.shape[0])
                L.check(elib.pmt_cnn_bn_backward_moments(*lib._common(h), i, g.data_ptr(), d_out.stride(0), stats.data_ptr(), mom[r].data_ptr(),
                                                         ws.data_ptr(), ws.numel(), _stream()), "pmt_cnn_bn_backward_moments")
            self._merge(i, mom, 1, stats, gtheta)
            self.moments[(i, 1)] = mom
        for r, h, g in self._slices(hap, d_out):
            ws = lib.workspace(h.shape[0])
            L.check(elib.pmt_cnn_bn_backward_full(*lib._common(h), g.data_ptr(), d_out.stride(0), stats.data_ptr(), gtheta, ws.data_ptr(), ws.numel(),
                                                  _stream()),
                    "pmt_cnn_bn_backward_full")
        torch.cuda.synchronize()
        return {n: p.grad.detach().double().cpu().numpy() for n, p in lib.model.haplotypes_cnn._model.named_parameters()}


ONE_RANK = [(s, n) for s in ("a", "b", "c") for n in (17, 1000)]  # 17: two workgroups, the second ragged; 1000: many partials


@lru_cache(maxsize=None)
def _one_rank(stack, n):
    """Computed once per case: (one-call out / forward statistics / completed statistics / gradients, a second one-call backward's
    gradients on the same inputs, the same four of the stepped form with one rank)"""
    lib = K.library(stack)
    hap, d_out = (t.cuda() for t in K.references(stack, n)[:2])
    out1, stats1 = lib.forward(hap)
    fwd1 = stats1.clone()
    grads1 = lib.backward(hap, d_out, stats1)
    again = lib.backward(hap, d_out, fwd1.clone())
    st = Stepped(lib, [n])
    out2, stats2 = st.forward(hap)
    fwd2 = stats2.clone()
    grads2 = st.backward(hap, d_out, stats2)
    return (out1, fwd1, stats1, grads1), again, (out2, fwd2, stats2, grads2)


def _distance(a, b):
    """{tensor: largest difference in units of the tensor's largest element} of the tensors that differ in a bit"""
    return {k: float(np.abs(a[k] - b[k]).max() / np.abs(a[k]).max()) for k in a if not np.array_equal(a[k], b[k])}


@pytest.mark.parametrize("stack,n", ONE_RANK, ids=[f"{s}-n{n}" for s, n in ONE_RANK])
def test_one_rank_gives_the_bits_of_the_one_call_form(stack, n):
    """R = 1: sum / N is the one-call fold's own expression and the merge's cross term is exactly 0, so the statistics buffer after the
    forward and after the backward (c1 / c2), the outputs and EVERY gradient of the CNN are the bits of pmt_cnn_bn_forward /
    pmt_cnn_bn_backward.  That needs the one-call backward to give the same bits twice, which is asserted first: its full pass sums the
    convolutions' and the linear's gradients in a private row per workgroup, folded in workgroup order (float atomics between workgroups,
    as the plain CNN backward uses without its workspace, differ from call to call by 4e-8 .. 1.5e-6 of a tensor's largest element)."""
    (out1, fwd1, stats1, grads1), again, (out2, fwd2, stats2, grads2) = _one_rank(stack, n)
    twice = _distance(grads1, again)
    print("one-call backward against a second one-call backward:", twice)
    assert not twice, twice
    assert torch.equal(fwd2, fwd1) and torch.equal(out2, out1)
    assert torch.equal(stats2, stats1)  # ... completed by the backward: c1, c2
    differ = _distance(grads1, grads2)
    print("stepped against one-call:", differ)
    assert not differ, differ
    assert bool(torch.isfinite(stats2).all()) and float(stats2.abs().max()) > 0


SHARDED = [("a", 8, (1, 7)),          # the flattened BatchNorm (len 1) sees ONE value per channel on rank 0: not refused, its M2 is 0
           ("a", 37, (16, 16, 5)),    # shards on workgroup boundaries
           ("b", 2, (1, 1)),
           ("b", 17, (16, 1)),
           ("c", 17, (1, 16)),
           ("c", 1000, (7, 500, 493))]


@pytest.mark.parametrize("stack,n,shards", SHARDED, ids=[f"{s}-n{n}-" + "+".join(map(str, sh)) for s, n, sh in SHARDED])
def test_sharded_batch_matches_fp64_on_the_whole_batch(stack, n, shards):
    lib = K.library(stack)
    hap, d_out, (out64, g64, var64), (out32, g32, _) = K.references(stack, n)
    out_scale = max(1.0, float(np.abs(out64).max()))
    # the yardstick: torch fp32 on the CPU (tests/test_cnn_bn_kernels_gpu.py)
    y_out = float(np.abs(out32 - out64).max()) / out_scale
    y_l2, y_worst, y_name = K.grad_errors(lib.model, g32, g64)
    print(f"torch fp32: out {y_out:.2e}, gradient L2 {y_l2:.2e}, worst tensor {y_worst:.2e} ({y_name})")
    assert y_out <= K.OUT_TOL / 3 and y_l2 <= K.GRAD_L2_TOL / 3 and y_worst <= K.GRAD_TENSOR_TOL / 3
    st = Stepped(lib, shards)
    hap_d, d_out_d = hap.cuda(), d_out.cuda()
    out, stats = st.forward(hap_d)
    grads = st.backward(hap_d, d_out_d, stats)
    e_out = float(np.abs(out.double().cpu().numpy() - out64).max()) / out_scale
    e_l2, e_worst, e_name = K.grad_errors(lib.model, grads, g64)
    e_var = max(float(np.abs(v / r - 1).max()) for v, r in zip(lib.batch_variances(stats), var64))
    print(f"sharded   : out {e_out:.2e}, gradient L2 {e_l2:.2e}, worst tensor {e_worst:.2e} ({e_name}), unbiased variance {e_var:.2e}")
    assert all(np.all(np.isfinite(g)) for g in grads.values())
    assert e_out <= K.OUT_TOL, e_out
    assert e_l2 <= K.GRAD_L2_TOL, e_l2
    assert e_worst <= K.GRAD_TENSOR_TOL, (e_name, e_worst)
    if shards[0] == 1:  # a rank with one variant: count = len values per channel; a length-1 BatchNorm's single value has M2 = 0
        for i in st._bn_indices():
            mom = st.moments[(i, 0)].cpu().numpy()
            assert np.all(mom[0, 0] == lib.cnn.layers[i].in_len)
            if lib.cnn.layers[i].in_len == 1:
                assert np.all(mom[0, 2] == 0.0)
    if stack == "a":
        assert any(lib.cnn.layers[i].in_len == 1 for i in st._bn_indices())  # (the flattened BatchNorm is what (a, 8) as 1 + 7 is about)


def test_sharded_variance_of_a_channel_far_from_zero():
    """The model of tests/test_cnn_bn_kernels_gpu.py's variance test (stack b, the first convolution's bias at 100: |mean| / std ~ 1e3,
    n = 1000) in three shards.  Ranks that exchanged (sum x, sum x^2) would lose the variance in E[x^2] - mean^2; (count, sum, M2 about the
    rank's own mean) merged in fp64 does not.  The same bound: no farther from fp64 than max(1e-5 relative, 2 x torch-fp32-CPU's own)."""
    model = K.build_model("b", seed=12)
    conv = model.haplotypes_cnn._model[0]
    with torch.no_grad():
        probe = K.one_hot(K._draw(np.random.default_rng(1), 1000), torch.float64)
        std = torch.nn.functional.conv1d(probe, conv.weight.double().cpu(), None).std(dim=(0, 2)).mean()
        conv.weight.mul_(float(0.1 / std))
        conv.bias.fill_(100.0)
    lib = K.Library(model)
    hap, d_out = K.inputs(1000, model)
    _, _, var64 = K.run_torch(model, hap, d_out, torch.float64)
    _, _, var32 = K.run_torch(model, hap, d_out, torch.float32)
    _, stats = Stepped(lib, (7, 500, 493)).forward(hap.cuda())
    ours = lib.batch_variances(stats)[0]
    mean = stats[lib.bn_layers[0].reserved[0]:][:32].double().cpu().numpy()
    ratio = float(np.abs(mean / np.sqrt(var64[0])).min())
    err_ours = float(np.abs(ours / var64[0] - 1).max())
    err_torch = float(np.abs(var32[0] / var64[0] - 1).max())
    print(f"|mean| / std >= {ratio:.0f}; merged batch variance against fp64: kernels {err_ours:.3e}, torch fp32 on the CPU {err_torch:.3e}")
    assert 300 < ratio < 3000
    assert err_ours <= max(1e-5, 2 * err_torch), (err_ours, err_torch)


def test_two_sharded_forwards_give_the_same_bits():
    lib = K.library("c")
    hap = K.references("c", 1000)[0].cuda()
    st = Stepped(lib, (7, 500, 493))
    out1, stats1 = st.forward(hap)
    out2, stats2 = st.forward(hap)
    torch.cuda.synchronize()
    assert torch.equal(stats1, stats2) and torch.equal(out1, out2)
    assert bool(torch.isfinite(stats1).all()) and float(stats1.abs().max()) > 0


def test_refusals_of_the_stepped_form():
    """All decided on the host, before any launch: a single value per channel with ONE rank (as the one-call form), a layer index outside
    the descriptor, a layer that is no BatchNorm."""
    lib = K.library("a")
    eng, elib, c = lib.eng, lib.eng.lib, lib.cnn
    hap = K.references("a", 8)[0].cuda()
    one = hap[:1]
    stats = torch.zeros(max(c.reserved[0], 4), dtype=torch.float32, device="cuda")
    out = torch.zeros(8, c.out_dim, dtype=torch.float32, device="cuda")
    flat = [i for i in range(c.n_layers) if c.layers[i].kind == L.CNN_BATCHNORM and c.layers[i].in_len == 1][0]
    mom = torch.zeros(2, 3, c.layers[flat].in_ch, dtype=torch.float64, device="cuda")
    ws = lib.workspace(8)

    def merge(layer, n, ranks, rank, backward=0):
        return elib.pmt_cnn_bn_merge(C.byref(eng.plan.desc), C.byref(c), layer, n, mom.data_ptr(), ranks, rank, backward, stats.data_ptr(),
                                     eng.space.gtheta.data_ptr(), _stream())

    def moments(layer, h=hap):
        return elib.pmt_cnn_bn_forward_moments(*lib._common(h), layer, stats.data_ptr(), mom.data_ptr(), ws.data_ptr(), ws.numel(), _stream())

    assert merge(flat, 1, 1, 0) == L.E_INVALID  # R = 1, n * len = 1
    assert elib.pmt_cnn_bn_forward(*lib._common(one), out.data_ptr(), out.stride(0), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _stream()) == L.E_INVALID  # (as the one-call form says)
    conv = [i for i in range(c.n_layers) if c.layers[i].kind == L.CNN_CONV][0]
    d_out = torch.zeros(8, c.out_dim, dtype=torch.float32, device="cuda")
    for layer in (-1, c.n_layers, L.MAX_CNN_LAYERS + 5, conv):
        assert moments(layer) == L.E_INVALID, layer
        assert merge(layer, 8, 2, 0) == L.E_INVALID, layer
        assert elib.pmt_cnn_bn_backward_moments(*lib._common(hap), layer, d_out.data_ptr(), d_out.stride(0), stats.data_ptr(), mom.data_ptr(),
                                                ws.data_ptr(), ws.numel(), _stream()) == L.E_INVALID, layer
    assert merge(flat, 8, 2, 2) == L.E_INVALID and merge(flat, 8, 0, 0) == L.E_INVALID  # a rank outside the group, no ranks at all
    assert moments(flat, hap[:0]) == L.E_INVALID  # the stepped form takes a rank's own n >= 1
    torch.cuda.synchronize()
    assert float(stats.abs().max()) == 0.0 and float(mom.abs().max()) == 0.0  # nothing was launched
