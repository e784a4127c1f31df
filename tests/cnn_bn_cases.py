"""Shared cases of the haplotype CNN trained on batch statistics (csrc/pmt_cnn_bn.hip), the CNN ALONE through the C ABI:
pmt_cnn_bn_forward / pmt_cnn_bn_backward on a model's engine against torch's own nn.Sequential on the CPU, in fp64 (the reference) and in
fp32 (the yardstick: how far fp32 arithmetic itself is from exact -- never the target).

Three stacks on S = 21 positions: (a) the production stack with a batch_norm token in each foldable place, (b) one BatchNorm directly
behind the first convolution, (c) the options stack (dilation, stride, selu, 64 channels) with two BatchNorms in front of convolutions.
Sizes: the chunk of a workgroup is at most 16 variants, so 17 always gives two workgroups with a ragged second one and 1000 exercises
the merge over many partials; (a) leaves out n = 2 and 5 because a flattened BatchNorm over a handful of samples is ill-conditioned in
fp32 for torch as well (gradient relative L2 of torch fp32 against fp64: 9.8e-5 and 5.6e-5 there, <= 1.9e-6 from n = 8 on)."""
import copy
import ctypes as C
from functools import lru_cache

import numpy as np
import torch
from torch import nn

from permutect_amd.architecture.artifact_model import ArtifactModel
from permutect_amd.engine import lib as L
from permutect_amd.engine.runtime import _stream
from permutect_amd.parameters import P0_CNN_BATCHNORM, p0_params

H = 42  # haplotypes_length: S = 21
OUT_TOL, GRAD_L2_TOL, GRAD_TENSOR_TOL = 2e-5, 1e-4, 5e-4

STACKS = {
    "a": list(P0_CNN_BATCHNORM),
    "b": ["convolution/kernel_size=3/out_channels=32", "batch_norm", "pool/kernel_size=2", "leaky_relu", "flatten", "linear/out_features=10"],
    "c": ["convolution/kernel_size=3/out_channels=64", "pool/kernel_size=2", "leaky_relu", "batch_norm",
          "convolution/kernel_size=3/dilation=2/out_channels=5", "selu", "batch_norm",
          "convolution/kernel_size=3/stride=2/out_channels=8", "leaky_relu", "flatten", "linear/out_features=10"],
}
SIZES = {"a": [8, 17, 37, 1000], "b": [2, 5, 17, 1000], "c": [2, 5, 17, 1000]}
CASES = [(s, n) for s in ("a", "b", "c") for n in SIZES[s]]


def build_model(stack: str, device="cuda", seed=11):
    """an ArtifactModel whose haplotype CNN is `stack`, its CNN parameters away from their initial values (BatchNorm weights in [0.5, 1.5])"""
    params = p0_params()
    params.ref_seq_layer_strings = list(STACKS[stack])
    torch.manual_seed(seed)
    model = ArtifactModel(params, device=torch.device(device), num_read_features=61, num_info_features=71, haplotypes_length=H)
    with torch.no_grad():
        for mod in model.haplotypes_cnn._model.children():
            for name, p in mod.named_parameters():
                if isinstance(mod, nn.BatchNorm1d) and name == "weight":
                    p.uniform_(0.5, 1.5)
                else:
                    p.add_(0.05 * torch.randn_like(p))
    return model


def _draw(rng, n):
    return torch.from_numpy(rng.integers(0, 5, (n, H), dtype=np.int64))


def knife_edge_variants(model, hap) -> torch.Tensor:
    """[n] bool: the variants that put a value on a DISCONTINUITY of the backward, judged on the fp64 forward.  The derivative of
    leaky_relu / selu jumps where the pre-activation changes sign, and max-pooling sends its gradient to another position when the two
    largest values of a window change order.  An implementation that meets the forward tolerance -- 2e-5 of a layer's largest value --
    may legitimately sit on the other side of such a point than fp64 does whenever fp64 is closer to it than that, and its gradient then
    differs by a whole term (measured: one of 224 000 pre-activations at 6.6e-6 from zero, the CNN gradient 6.2e-3 off in relative L2).
    Such variants say nothing about the kernels; exact ties of a pooling window (identical sequence windows) are no edge: first wins."""
    seq = copy.deepcopy(model.haplotypes_cnn._model).cpu().double().train(True)
    bad = torch.zeros(hap.shape[0], dtype=torch.bool)
    x = one_hot(hap, torch.float64)
    with torch.no_grad():
        for m in seq.children():
            t = OUT_TOL * float(x.abs().max())
            if isinstance(m, (nn.LeakyReLU, nn.SELU)):
                bad |= (x.abs() < t).flatten(1).any(1)
            elif isinstance(m, nn.MaxPool1d):
                stride = m.stride if m.stride is not None else m.kernel_size
                top = x.unfold(2, m.kernel_size, stride).topk(2, dim=-1).values
                gap = top[..., 0] - top[..., 1]
                bad |= ((gap > 0) & (gap < t)).flatten(1).any(1)
            x = m(x)
    return bad


DISTINCT = 32  # distinct haplotype rows of a batch (see inputs)


def inputs(n: int, model, seed=5):
    """(haplotypes [n, H], upstream gradient [n, 10]), seeded.  The n variants are drawn from at most DISTINCT distinct haplotype rows
    (every variant has its own upstream gradient): a batch of 1000 independent rows holds half a million pre-activations, a handful of
    them always within fp32 reach of zero, and which side of zero an fp32 implementation lands on there is luck, not correctness.  With
    few distinct rows the values are few, and rows on a knife edge of `model`'s backward (above) are drawn again until none is left (the
    batch statistics couple the rows, so all of them are looked at again each time).  The batch statistics, the partials of every
    workgroup and their merge are those of n variants all the same."""
    rng = np.random.default_rng(seed + n)
    pool = _draw(rng, min(n, DISTINCT))
    pick = torch.from_numpy(np.concatenate([np.arange(len(pool)), rng.integers(0, len(pool), n - len(pool))]))
    pick = pick[torch.from_numpy(rng.permutation(n))]
    d_out = torch.from_numpy(rng.standard_normal((n, 10)).astype(np.float32))
    for _ in range(400):
        hap = pool[pick]
        bad = knife_edge_variants(model, hap)
        if not bool(bad.any()):
            return hap.contiguous(), d_out
        rows = torch.unique(pick[bad])
        pool[rows] = _draw(rng, len(rows))
    raise AssertionError("no well-conditioned batch found")


def one_hot(hap: torch.Tensor, dtype) -> torch.Tensor:
    """[n, H] codes -> [n, 10, S]: channel 2 * base + (0 ref | 1 alt) (reference data/batch.py:115-130)"""
    n, s = hap.shape[0], hap.shape[1] // 2
    oh = torch.zeros(n, 10, s, dtype=dtype)
    for half in (0, 1):
        codes = hap[:, half * s:(half + 1) * s]
        for base in range(5):
            oh[:, 2 * base + half, :] = (codes == base).to(dtype)
    return oh


def run_torch(model, hap, d_out, dtype):
    """torch's own train-mode forward and backward of the CNN on the CPU in `dtype`: (out, {parameter name: gradient}, [unbiased batch
    variance per BatchNorm]) as float64 arrays.  The variances are read from the running statistics of a copy with momentum 1."""
    seq = copy.deepcopy(model.haplotypes_cnn._model).cpu().to(dtype).train(True)
    bns = [m for m in seq.children() if isinstance(m, nn.BatchNorm1d)]
    for bn in bns:
        bn.momentum = 1.0
    out = seq(one_hot(hap, dtype))
    out.backward(d_out.to(dtype))
    grads = {n: p.grad.detach().double().numpy() for n, p in seq.named_parameters()}
    return out.detach().double().numpy(), grads, [bn.running_var.detach().double().numpy() for bn in bns]


def tensor_scales(model, grads):
    """the scale a gradient tensor's error is measured on: its own largest reference element -- except for the bias of a convolution /
    linear directly in front of a BatchNorm, whose true gradient is exactly zero (the BatchNorm subtracts the mean) and whose fp32
    value is rounding noise: the same layer's weight gradient"""
    mods = list(model.haplotypes_cnn._model.children())
    scale = {}
    for i, mod in enumerate(mods):
        for leaf, _ in mod.named_parameters():
            zero = leaf == "bias" and not isinstance(mod, nn.BatchNorm1d) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm1d)
            scale[f"{i}.{leaf}"] = float(np.abs(grads[f"{i}.weight" if zero else f"{i}.{leaf}"]).max())
    return scale


def grad_errors(model, grads, ref):
    """(relative L2 of the concatenated gradient, the worst tensor's largest error in units of its scale, that tensor's name)"""
    names = sorted(ref)
    v, r = np.concatenate([grads[n].ravel() for n in names]), np.concatenate([ref[n].ravel() for n in names])
    scale = tensor_scales(model, ref)
    per = {n: float(np.abs(grads[n] - ref[n]).max()) / scale[n] for n in names}
    worst = max(per, key=per.get)
    return float(np.linalg.norm(v - r) / np.linalg.norm(r)), per[worst], worst


class Library:
    """pmt_cnn_bn_forward / pmt_cnn_bn_backward on a model's engine, called as the C ABI declares them (include/permutect_amd.h)"""

    def __init__(self, model):
        self.model, self.eng = model, model.engine()
        eng = self.eng
        eng.draw_dropout_seed(False)
        eng.pack(eng.plan.materialize_phi(model).detach().contiguous())  # the packed weight fragments of the (unfolded) parameters
        self.cnn = eng.plan.cnn_train_desc(model)
        self.bn_layers = [self.cnn.layers[i] for i in range(self.cnn.n_layers) if self.cnn.layers[i].kind == L.CNN_BATCHNORM]

    def _common(self, hap):
        eng, plan = self.eng, self.eng.plan
        return (C.byref(plan.desc), plan.desc_dev.data_ptr(), C.byref(self.cnn), plan.cnn_train_dev.data_ptr(), eng.space.theta.data_ptr(),
                plan.packed.data_ptr(), hap.data_ptr(), hap.stride(0), hap.shape[0])

    def workspace(self, n):
        return torch.empty(max(int(self.eng.lib.pmt_cnn_bn_workspace_floats(C.byref(self.cnn), n)), 4), dtype=torch.float32, device="cuda")

    def forward(self, hap):
        """(out [n, 10], the statistics buffer) on the device"""
        n = hap.shape[0]
        out = torch.empty(n, self.cnn.out_dim, dtype=torch.float32, device="cuda")
        stats = torch.zeros(max(self.cnn.reserved[0], 4), dtype=torch.float32, device="cuda")
        ws = self.workspace(n)
        L.check(self.eng.lib.pmt_cnn_bn_forward(*self._common(hap), out.data_ptr(), out.stride(0), stats.data_ptr(), ws.data_ptr(), ws.numel(),
                                                _stream()), "pmt_cnn_bn_forward")
        return out, stats

    def backward(self, hap, d_out, stats):
        """{parameter name as in the Sequential: gradient} of the CNN's parameters (float64 arrays)"""
        eng = self.eng
        ws = self.workspace(hap.shape[0])
        eng.space.gtheta.zero_()
        L.check(eng.lib.pmt_cnn_bn_backward(*self._common(hap), d_out.data_ptr(), d_out.stride(0), stats.data_ptr(), eng.space.gtheta.data_ptr(),
                                            ws.data_ptr(), ws.numel(), _stream()), "pmt_cnn_bn_backward")
        torch.cuda.synchronize()
        return {n: p.grad.detach().double().cpu().numpy() for n, p in self.model.haplotypes_cnn._model.named_parameters()}

    def batch_variances(self, stats):
        """the unbiased batch variance of every BatchNorm as the forward stored it (float64 arrays)"""
        s = stats.double().cpu().numpy()
        return [s[b.reserved[0] + 2 * b.in_ch:b.reserved[0] + 3 * b.in_ch] for b in self.bn_layers]


@lru_cache(maxsize=None)
def library(stack: str) -> Library:
    return Library(build_model(stack))


@lru_cache(maxsize=None)
def references(stack: str, n: int):
    """(hap, d_out, fp64 (out, grads, variances), fp32 (out, grads, variances)) of a case, computed once"""
    model = library(stack).model
    hap, d_out = inputs(n, model)
    return hap, d_out, run_torch(model, hap, d_out, torch.float64), run_torch(model, hap, d_out, torch.float32)
