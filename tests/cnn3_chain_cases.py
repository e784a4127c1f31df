"""Cases, references and the numpy mirror for the batched haplotype-CNN backward's input-gradient chain on the bf16 matrix pipe
(csrc/pmt_cnn3.hip, phases 1 and 4; tests/test_cnn3_backward_chain_cpu.py and _gpu.py).

The stack is the production one of instance <8, 4, 3, 3, 7>: Conv1d(10 -> 32, 3) -> MaxPool1d(2) -> leaky ReLU -> Conv1d(32 -> 32, 3) ->
leaky ReLU -> Flatten -> Linear(224 -> 10) on 21 positions.

`reference(params, hap, d_out, dtype)` is torch autograd in float64 (the yardstick) or float32 (the float32 reference whose own
distance from fp64 the bound is a multiple of).  `mirror(...)` restates the kernel's arithmetic: every operand of the chain and of the
convolutions' weight gradients is hi + mid, two bf16 values rounded to nearest even; a product is mid.hi + hi.mid + hi.hi; the linear's
transpose contracts over its 10 outputs inside a 32-deep block whose other 22 k are zeros in BOTH operands.  Sums are taken in float64
here (the matrix core's are fp32), values between the phases are float32 as in LDS.

BOUND, per gradient tensor and case: the kernel stays within 4 x the float32 reference's relative L2 error from fp64, never above 2e-4.
Two bf16 pieces carry 16 significant bits, float32 24: where the MIRROR itself is beyond half of 4 x the reference's error the bound
is twice the mirror's value instead (still never above 2e-4).  That is the case for most tensors -- the float32 reference sits at
1 - 6e-7, the mirror at 1 - 6e-6 -- and bound() returns which of the two forms applied."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.test_cnn3_backward_pieces_cpu import split2

S, K1, K2, C1, C2, O = 21, 3, 3, 32, 32, 10
L1, P1, L2, ST2 = 19, 9, 7, 8
V, NW = 8, 4                      # variants per wave and batch, waves per workgroup of the backward
CAP = 2e-4                        # tests/test_cnn_gpu.py: the CNN gradient's bound
TENSORS = ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "linear.weight", "linear.bias"]
D_OUT_KINDS = ["normal", "zero", "scaled"]


def sizes(grid):
    """variant counts: around one batch of a wave, then around one full round of the grid the host picks (8 x NW x grid): a wave
    sees zero, one and two batches and a ragged last one"""
    full = V * NW * grid
    return [1, 7, 8, 9, full - 1, full, full + 1]


def make_params(seed=5):
    rng = np.random.default_rng(seed)
    u = lambda shape, fan: ((rng.random(shape) * 2 - 1) / np.sqrt(fan)).astype(np.float32)  # noqa: E731  (torch's default ranges)
    return {"conv1.weight": u((C1, 10, K1), 10 * K1), "conv1.bias": u((C1,), 10 * K1), "conv2.weight": u((C2, C1, K2), C1 * K2),
            "conv2.bias": u((C2,), C1 * K2), "linear.weight": u((O, C2 * L2), C2 * L2), "linear.bias": u((O,), C2 * L2)}


def make_haplotypes(n, seed=9):
    """U{0..4} codes [n, 2 S]; of every four rows one is an edge: one base throughout (every pool pair ties: the first position must
    win), two runs of one base each in both haplotypes (ties inside the runs, none across the border), ref == alt"""
    rng = np.random.default_rng(seed)
    hap = rng.integers(0, 5, (n, 2 * S), dtype=np.int64)
    for i in range(1, n, 4):
        kind = (i // 4) % 3
        if kind == 0:
            hap[i] = (i // 12) % 4
        elif kind == 1:
            hap[i, :] = (i // 12) % 4
            hap[i, S // 2:S] = hap[i, S + S // 2:] = (i // 12 + 1) % 4
        else:
            hap[i, S:] = hap[i, :S]
    return hap


def make_d_out(n, kind, seed=13):
    """N(0, 1); all zero; N(0, 1) with the first row scaled by 2^20 and the last by 2^-20 (one row: the first scale only)"""
    d = np.random.default_rng(seed).standard_normal((n, O)).astype(np.float32)
    if kind == "zero":
        d[:] = 0.0
    elif kind == "scaled":
        d[0] *= 2.0 ** 20
        if n > 1:
            d[n - 1] *= 2.0 ** -20
    return d


def one_hot(hap):
    """[n, 2 S] -> [n, 10, S]: channel 2 base + (0 ref | 1 alt) (oracle.artifact_oracle.one_hot_haplotypes)"""
    n = hap.shape[0]
    oh = (hap[:, :, None] == np.arange(5)[None, None, :])
    return np.ascontiguousarray(oh.transpose(0, 2, 1).reshape(n, 10, S))


def reference(params, hap, d_out, dtype):
    """the six gradient tensors by torch autograd in `dtype`, as float64 numpy arrays"""
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in params.items()}
    grads = {k: np.zeros(v.shape, np.float64) for k, v in params.items()}
    x_all, d_all = torch.from_numpy(one_hot(hap)).to(dtype), torch.from_numpy(d_out).to(dtype)
    for a in range(0, hap.shape[0], 4096):
        x, d = x_all[a:a + 4096], d_all[a:a + 4096]
        y = F.leaky_relu(F.max_pool1d(F.conv1d(x, p["conv1.weight"], p["conv1.bias"]), 2), 0.01)
        y = F.leaky_relu(F.conv1d(y, p["conv2.weight"], p["conv2.bias"]), 0.01)
        out = F.linear(y.flatten(1), p["linear.weight"], p["linear.bias"])
        for k, g in zip(TENSORS, torch.autograd.grad((out * d).sum(), [p[k] for k in TENSORS])):
            grads[k] += g.double().numpy()
    return grads


def forward32(params, hap):
    """what the training forward leaves in the stash, in float32: a1 [n, C1, P1] (pooled, activated), a2 [n, C2, L2], and the pool's
    argmax [n, C1, P1] (1: the second position of the pair won; the first wins a tie, like ATen's max_pool1d)"""
    x = one_hot(hap).astype(np.float32)
    w1, w2 = params["conv1.weight"], params["conv2.weight"]
    y1 = sum(np.einsum("oc,ncp->nop", w1[:, :, k], x[:, :, k:k + L1], optimize=True) for k in range(K1)) + params["conv1.bias"][None, :, None]
    first, second = y1[:, :, 0:2 * P1:2], y1[:, :, 1:2 * P1:2]
    arg = second > first
    pooled = np.where(arg, second, first)
    a1 = np.where(pooled > 0, pooled, np.float32(0.01) * pooled).astype(np.float32)
    y2 = sum(np.einsum("oc,ncp->nop", w2[:, :, k], a1[:, :, k:k + L2], optimize=True) for k in range(K2)) + params["conv2.bias"][None, :, None]
    a2 = np.where(y2 > 0, y2, np.float32(0.01) * y2).astype(np.float32)
    return a1, a2, arg


def _pieces(x):
    hi, mid = split2(np.asarray(x, dtype=np.float32))
    return hi.astype(np.float64), mid.astype(np.float64)


def product(a, b, spec, mutant=None, drop="drop_mid_hi"):
    """einsum `spec` of a and b from two bf16 pieces per operand: mid.hi + hi.mid + hi.hi (float64 sums)"""
    (ah, am), (bh, bm) = _pieces(a), _pieces(b)
    out = np.einsum(spec, ah, bm, optimize=True) + np.einsum(spec, ah, bh, optimize=True)
    if mutant != drop:
        out = out + np.einsum(spec, am, bh, optimize=True)
    return out


def mirror(params, hap, d_out, a1, a2, arg, mutant=None):
    """the kernel's backward on the stash (a1, a2, arg).  Mutants: "drop_mid_hi" leaves the mid.hi product out of phase 4;
    "one_piece" runs phase 4 on the hi pieces alone; "unpadded" reads the k >= 10 half of phase 1's block as whatever lies behind the
    operands (the next variant's d(out), the next output's weights) instead of zeros"""
    n = hap.shape[0]
    f32 = lambda v: np.asarray(v, dtype=np.float32)  # noqa: E731
    wl = params["linear.weight"].reshape(O, C2, L2)
    w2 = params["conv2.weight"]
    slope = lambda y: np.where(y > 0, np.float32(1), np.float32(0.01))  # noqa: E731
    # 1. d(a2)[n, ch, p] = sum_o Wl[o, ch, p] d(out)[n, o]: one 32-deep block, k >= O zero in both operands
    wl_k, d_k = np.zeros((32, C2, L2), np.float32), np.zeros((n, 32), np.float32)
    wl_k[:O], d_k[:, :O] = wl, d_out
    if mutant == "unpadded":
        d_k[:, O:2 * O] = np.roll(d_out, -1, axis=0)
        wl_k[O:2 * O] = np.roll(wl, -1, axis=0)
    d_a2 = f32(product(wl_k, d_k, "kcp,nk->ncp"))
    # 2. through the second activation; the linear's gradients (fp32 products)
    dy2 = f32(d_a2 * slope(a2))
    g = {"linear.weight": np.einsum("no,ncp->ocp", d_out.astype(np.float64), a2.astype(np.float64), optimize=True).reshape(O, C2 * L2),
         "linear.bias": d_out.astype(np.float64).sum(0), "conv2.bias": dy2.astype(np.float64).sum((0, 2))}
    # 3. conv2's weight gradient: k = (position, variant)
    g["conv2.weight"] = np.stack([product(dy2, a1[:, :, k:k + L2], "nop,ncp->oc") for k in range(K2)], axis=2)
    # 4. conv2's input gradient, a block of k = conv2's 32 output channels per tap; through the first activation
    dp = np.zeros((n, C1, P1), np.float64)
    for k in range(K2):
        if mutant == "one_piece":
            t = np.einsum("oc,nop->ncp", _pieces(w2[:, :, k])[0], _pieces(dy2)[0], optimize=True)
        else:
            t = product(w2[:, :, k], dy2, "oc,nop->ncp", mutant)
        dp[:, :, k:k + L2] += t
    dp = f32(f32(dp) * slope(a1))
    g["conv1.bias"] = dp.astype(np.float64).sum((0, 2))
    # 5. conv1's weight gradient: the pooled gradient (two pieces) against the one-hot (exact) at the pool's winning position
    dph, dpm = _pieces(dp)
    d2 = dph + dpm
    x = one_hot(hap).astype(np.float64)
    dy1 = np.zeros((n, C1, 2 * P1), np.float64)
    dy1[:, :, 0::2] = np.where(arg, 0.0, d2)
    dy1[:, :, 1::2] = np.where(arg, d2, 0.0)
    g["conv1.weight"] = np.stack([np.einsum("nop,ncp->oc", dy1, x[:, :, k:k + 2 * P1], optimize=True) for k in range(K1)], axis=2)
    return {k: np.asarray(g[k], dtype=np.float64).reshape(params[k].shape) for k in TENSORS}


def rel_l2(x, ref):
    """relative L2 distance; against an all-zero reference: 0 if x is all zero too, else inf"""
    den = float(np.linalg.norm(ref))
    if den == 0.0:
        return 0.0 if not np.any(x) else float("inf")
    return float(np.linalg.norm(np.asarray(x, np.float64) - ref) / den)


def bound(err32, err_mirror):
    """(the bound, whether it is the widened form): 4 x the float32 reference's error; twice the mirror's where the mirror is beyond
    half of that; 2e-4 at most"""
    widened = err_mirror > 0.5 * 4.0 * err32
    return min(CAP, 2.0 * err_mirror if widened else 4.0 * err32), widened


def decode_stash(stash, n):
    """the forward's records [n, 556] floats -> a1 [n, C1, P1], a2 [n, C2, L2], arg [n, C1, P1].  A record: [a1: P1 x 32][a2: ST2 x 32]
    [argmax: P1 words]; element e of a 32-block is channel 16 (e >> 4) + 4 (e & 3) + ((e & 15) >> 2); argmax word q: bit
    8 g + 4 mt + j is channel 16 mt + 4 j + g"""
    per = (P1 * 32 + ST2 * 32 + P1 + 3) & ~3
    rec = np.asarray(stash, dtype=np.float32).reshape(n, per)
    e = np.arange(32)
    chan = 16 * (e >> 4) + 4 * (e & 3) + ((e & 15) >> 2)
    a1, a2 = np.zeros((n, C1, P1), np.float32), np.zeros((n, C2, L2), np.float32)
    a1[:, chan, :] = rec[:, :P1 * 32].reshape(n, P1, 32).transpose(0, 2, 1)
    a2[:, chan, :] = rec[:, P1 * 32:P1 * 32 + ST2 * 32].reshape(n, ST2, 32).transpose(0, 2, 1)[:, :, :L2]
    words = np.ascontiguousarray(rec[:, P1 * 32 + ST2 * 32:P1 * 32 + ST2 * 32 + P1]).view(np.uint32)
    arg = np.zeros((n, C1, P1), bool)
    for gq in range(4):
        for mt in range(2):
            for j in range(4):
                arg[:, 16 * mt + 4 * j + gq, :] = (words >> (8 * gq + 4 * mt + j)) & 1
    return a1, a2, arg
