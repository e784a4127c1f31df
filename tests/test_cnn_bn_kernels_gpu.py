"""The kernels that train the haplotype CNN's `batch_norm` tokens on batch statistics (csrc/pmt_cnn_bn.hip), alone, through the C ABI
(pmt_cnn_bn_forward / pmt_cnn_bn_backward), against torch's own nn.Sequential in fp64 on the CPU: tests/cnn_bn_cases.py holds the
stacks, the sizes and why they are what they are.

Every case first asserts that torch's fp32 on the CPU is within a third of each tolerance (the case is well-conditioned: what the
kernels are held to is not below what fp32 arithmetic gives), then holds the kernels to: outputs |err| <= 2e-5 x max(1, max|ref|), the
concatenated gradient 1e-4 relative L2, every gradient tensor 5e-4 of its scale (the bias of a convolution directly in front of a
BatchNorm has a true gradient of exactly zero: it is measured on the scale of the same layer's weight gradient)."""
import numpy as np
import pytest
import torch

from tests import cnn_bn_cases as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stack,n", K.CASES, ids=[f"{s}-n{n}" for s, n in K.CASES])
def test_forward_and_every_gradient_match_fp64(stack, n):
    lib = K.library(stack)
    hap, d_out, (out64, g64, _), (out32, g32, _) = K.references(stack, n)
    out_scale = max(1.0, float(np.abs(out64).max()))
    # the yardstick: torch fp32 on the CPU
    y_out = float(np.abs(out32 - out64).max()) / out_scale
    y_l2, y_worst, y_name = K.grad_errors(lib.model, g32, g64)
    print(f"torch fp32: out {y_out:.2e}, gradient L2 {y_l2:.2e}, worst tensor {y_worst:.2e} ({y_name})")
    assert y_out <= K.OUT_TOL / 3 and y_l2 <= K.GRAD_L2_TOL / 3 and y_worst <= K.GRAD_TENSOR_TOL / 3
    # the kernels
    hap_d, d_out_d = hap.cuda(), d_out.cuda()
    out, stats = lib.forward(hap_d)
    grads = lib.backward(hap_d, d_out_d, stats)
    e_out = float(np.abs(out.double().cpu().numpy() - out64).max()) / out_scale
    e_l2, e_worst, e_name = K.grad_errors(lib.model, grads, g64)
    print(f"kernels   : out {e_out:.2e}, gradient L2 {e_l2:.2e}, worst tensor {e_worst:.2e} ({e_name})")
    assert all(np.all(np.isfinite(g)) for g in grads.values())
    assert e_out <= K.OUT_TOL, e_out
    assert e_l2 <= K.GRAD_L2_TOL, e_l2
    assert e_worst <= K.GRAD_TENSOR_TOL, (e_name, e_worst)


def test_batch_variance_of_a_channel_far_from_zero_is_not_a_difference_of_large_sums():
    """Stack (b) with the first convolution's bias at 100 and its weights scaled down so that |mean| / std ~ 1e3 in the BatchNorm's
    input, n = 1000.  A naive fp32 sum x, sum x^2 loses the variance there by orders of magnitude (E[x^2] - mean^2 cancels six digits);
    per-workgroup (mean, M2) pairs merged in fp64 do not.  Bound: no farther from fp64 than the larger of 1e-5 relative and twice
    torch-fp32-CPU's own distance.  The factor is the one that gives the ratio, worked out on the fp64 convolution: with a flat 1e-3
    the ratio of this model is 3e5, where an fp32 activation of 100 +- 3e-4 (one ulp: 7.6e-6) no longer holds its own variance --
    torch's fp32 is 1.4e-3 from fp64 there, the kernels, which add the bias before the products, 1.2e-2 -- and nothing about the
    statistics can be read off."""
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
    _, stats = lib.forward(hap.cuda())
    ours = lib.batch_variances(stats)[0]
    mean = stats[lib.bn_layers[0].reserved[0]:][:32].double().cpu().numpy()
    ratio = float(np.abs(mean / np.sqrt(var64[0])).min())
    err_ours = float(np.abs(ours / var64[0] - 1).max())
    err_torch = float(np.abs(var32[0] / var64[0] - 1).max())
    print(f"|mean| / std >= {ratio:.0f}; batch variance against fp64: kernels {err_ours:.3e}, torch fp32 on the CPU {err_torch:.3e}")
    assert 300 < ratio < 3000
    assert err_ours <= max(1e-5, 2 * err_torch), (err_ours, err_torch)


@pytest.mark.parametrize("stack", ["a", "c"])
def test_two_forwards_give_the_same_bits(stack):
    """no float atomics in the statistics, partials merged in a fixed order: the statistics (and with them the outputs) repeat bit for bit"""
    lib = K.library(stack)
    hap = K.references(stack, 1000)[0].cuda()
    out1, stats1 = lib.forward(hap)
    out2, stats2 = lib.forward(hap)
    torch.cuda.synchronize()
    assert torch.equal(stats1, stats2) and torch.equal(out1, out2)
    assert bool(torch.isfinite(stats1).all()) and float(stats1.abs().max()) > 0
