"""pmt_cnn3_backward_kernel<8, 4, 3, 3, 7> with its input-gradient chain (the linear's and conv2's transposes) as 32-deep bf16 products on
two-piece operands, called through the C entries (pmt_cnn_forward for the stash, pmt_cnn_backward) on buffers this file owns.

Per case: every one of the six gradient tensors against float64 autograd under the bound of tests/cnn3_chain_cases.py (4 x the float32
reference's own relative L2 error; twice the numpy mirror's where the mirror -- fed with the very stash the kernel read -- is beyond half
of that; 2e-4 at most), the guard words around the gradient buffer and the workspace, and the gradient buffer outside the CNN's six
tensors bit for bit.  Variant counts: 1, 7, 8, 9, then one below / at / one above 8 x 4 x the grid the host picks, so that a wave sees
zero, one and two batches and a ragged last one.  d(out): N(0, 1); all zero; one row scaled by 2^20 and one by 2^-20.  Of every four
haplotype rows one is an edge: one base throughout (every pool pair ties), two runs (ties inside them), ref == alt."""
import ctypes as C

import numpy as np
import pytest
import torch

from permutect_amd.engine import lib as L
from tests import cnn3_chain_cases as K
from tests.test_cnn_instances_gpu import B_BF21, B_BWD, B_FOLD, Row, build_model, compute_units
from tests.test_scale_gpu import record

pytestmark = pytest.mark.gpu

GUARD = 256                      # floats on either side
GUARD_WORD = 0x7FC0BEEF          # a NaN no kernel computes
FILL = 0x7FA11ED5                # the gradient buffer outside the CNN's tensors (another one)


@pytest.fixture(scope="module")
def rig():
    with pytest.MonkeyPatch.context() as mp:
        model, eng, sd = build_model(Row("p0", 42, "batched", B_BF21 + (B_BWD, B_FOLD)), mp)
        cnn = [(k, p) for k, p in model.named_parameters() if k.startswith("haplotypes_cnn.")]
        assert len(cnn) == 6
        params = {t: p.detach().cpu().numpy().astype(np.float32) for t, (_, p) in zip(K.TENSORS, cnn)}
        assert params["conv1.weight"].shape == (K.C1, 10, K.K1) and params["conv2.weight"].shape == (K.C2, K.C1, K.K2)
        assert params["linear.weight"].shape == (K.O, K.C2 * K.L2)
        where = {t: (eng.space.offset_of(p), p.numel()) for t, (_, p) in zip(K.TENSORS, cnn)}
        yield dict(eng=eng, params=params, where=where, model=model)


@pytest.fixture(scope="module")
def references(rig):
    """(n, kind) -> (hap, d_out, fp64 gradients, float32 reference's gradients): each computed once"""
    memo = {}

    def get(n, kind):
        if (n, kind) not in memo:
            hap, d = K.make_haplotypes(n), K.make_d_out(n, kind)
            memo[n, kind] = (hap, d, K.reference(rig["params"], hap, d, torch.float64), K.reference(rig["params"], hap, d, torch.float32))
        return memo[n, kind]
    return get


def guarded(n_floats, inner_word, dev):
    buf = torch.full((n_floats + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device=dev)
    buf[GUARD:GUARD + n_floats] = inner_word
    return buf


def guards_intact(buf, n_floats):
    return bool((buf[:GUARD] == GUARD_WORD).all()) and bool((buf[GUARD + n_floats:] == GUARD_WORD).all())


def run_kernel(rig, hap_np, d_np):
    """-> (gradient buffer as float32 numpy, its raw words, the stash, guards intact?)"""
    eng, dev = rig["eng"], torch.device("cuda")
    d, n = eng.plan.desc, hap_np.shape[0]
    hap, d_out = torch.from_numpy(hap_np).to(dev), torch.from_numpy(d_np).to(dev)
    out = torch.empty(n, K.O, dtype=torch.float32, device=dev)
    per = eng.lib.pmt_cnn_stash_floats(C.byref(d))
    assert per == (K.P1 * 32 + K.ST2 * 32 + K.P1 + 3) // 4 * 4
    stash = torch.empty(n * per, dtype=torch.float32, device=dev)
    theta, packed = eng.cnn_params()
    L.check(eng.lib.pmt_cnn_forward(C.byref(d), eng.plan.desc_dev.data_ptr(), theta.data_ptr(), packed.data_ptr(), hap.data_ptr(), hap.stride(0), n,
                                    out.data_ptr(), out.stride(0), stash.data_ptr(), L.raw_stream()), "pmt_cnn_forward")
    torch.cuda.synchronize()
    stash_np = stash.cpu().numpy()  # (before the backward: a development build of the kernel may write cycle stamps over dead records)
    ng, nws = eng.space.gtheta.numel(), eng.lib.pmt_cnn_workspace_floats(C.byref(d))
    assert nws > 0
    g, ws = guarded(ng, FILL, dev), guarded(nws, FILL, dev)
    for off, numel in rig["where"].values():
        g[GUARD + off:GUARD + off + numel] = 0
    L.check(eng.lib.pmt_cnn_backward(C.byref(d), eng.plan.desc_dev.data_ptr(), eng.space.theta.data_ptr(), eng.plan.packed.data_ptr(), hap.data_ptr(),
                                     hap.stride(0), n, d_out.data_ptr(), d_out.stride(0), stash.data_ptr(), g.data_ptr() + 4 * GUARD,
                                     ws.data_ptr() + 4 * GUARD, nws, L.raw_stream()), "pmt_cnn_backward")
    torch.cuda.synchronize()
    words = g[GUARD:GUARD + ng].cpu().numpy()
    return words.view(np.float32), words, stash_np, guards_intact(g, ng) and guards_intact(ws, nws)


def n_ids():
    return ["1", "7", "8", "9", "round-1", "round", "round+1"]


@pytest.mark.parametrize("kind", K.D_OUT_KINDS)
@pytest.mark.parametrize("which", range(7), ids=n_ids())
def test_every_gradient_tensor_against_fp64(which, kind, rig, references):
    n = K.sizes(compute_units())[which]
    hap, d, g64, g32 = references(n, kind)
    got, words, stash, intact = run_kernel(rig, hap, d)
    assert intact, "guard words around the gradient buffer / the workspace"
    outside = np.ones(words.size, bool)
    for off, numel in rig["where"].values():
        outside[off:off + numel] = False
    assert np.all(words[outside] == np.int32(FILL)), "the gradient buffer outside the CNN's tensors"
    gm = K.mirror(rig["params"], hap, d, *K.decode_stash(stash, n))
    failures = []
    for t in K.TENSORS:
        off, numel = rig["where"][t]
        mine = got[off:off + numel].astype(np.float64).reshape(g64[t].shape)
        assert np.all(np.isfinite(mine)), (n, kind, t)
        err, e32, em = K.rel_l2(mine, g64[t]), K.rel_l2(g32[t], g64[t]), K.rel_l2(gm[t], g64[t])
        b, widened = K.bound(e32, em)
        record(test="cnn3_backward_chain", n=n, d_out=kind, tensor=t, kernel_rel_l2=err, float32_reference=e32, mirror=em, bound=b, widened=bool(widened))
        print(f"n = {n} d(out) {kind} {t}: kernel {err:.2e}, float32 reference {e32:.2e}, mirror {em:.2e}, bound {b:.2e}{' (widened)' if widened else ''}")
        if not err <= b:
            failures.append((t, err, b))
    assert not failures, (n, kind, failures)


def test_a_pool_tie_routes_the_gradient_to_the_first_position(rig):
    """one base throughout: conv1's output is the same at every position, every pool pair ties, and the stash says the first won"""
    hap = K.make_haplotypes(9)
    _, _, stash, _ = run_kernel(rig, hap, K.make_d_out(9, "normal"))
    _, _, arg = K.decode_stash(stash, 9)
    assert len(set(hap[1])) == 1 and not arg[1].any()
    assert arg[0].any() and not arg[0].all()
    assert not arg[5][:, :3].any()  # two runs of one base: ties inside the first run
