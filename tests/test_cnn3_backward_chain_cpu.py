"""The numpy mirror of the batched haplotype-CNN backward with its input-gradient chain on two bf16 pieces (tests/cnn3_chain_cases.py)
against float64 autograd, on the cases of the device test that fit a CPU run: n = 1, 7, 8, 9 and 257 variants, every kind of d(out).

Asserted: the mirror within half of every bound (per gradient tensor and case; bound() says where the bound is the widened form,
twice the mirror's own value, and the test prints it); an all-zero d(out) gives all-zero gradients; the pool's ties go to the first
position; and three mutants -- the mid.hi product dropped from phase 4, phase 4 on one piece, phase 1's half-filled block read
unpadded -- each break the bound of the tensor their error travels into."""
import numpy as np
import pytest
import torch

from tests import cnn3_chain_cases as K

NS = [1, 7, 8, 9, 257]


@pytest.fixture(scope="module")
def params():
    return K.make_params()


@pytest.fixture(scope="module")
def cases(params):
    """(n, kind) -> (hap, d_out, stash, fp64 gradients, float32 reference's errors, mirror's gradients and errors), computed once"""
    out = {}
    for n in NS:
        hap = K.make_haplotypes(n)
        stash = K.forward32(params, hap)
        for kind in K.D_OUT_KINDS:
            d = K.make_d_out(n, kind)
            g64, g32 = K.reference(params, hap, d, torch.float64), K.reference(params, hap, d, torch.float32)
            gm = K.mirror(params, hap, d, *stash)
            out[n, kind] = dict(hap=hap, d=d, stash=stash, g64=g64, gm=gm,
                                e32={t: K.rel_l2(g32[t], g64[t]) for t in K.TENSORS}, em={t: K.rel_l2(gm[t], g64[t]) for t in K.TENSORS})
    return out


@pytest.mark.parametrize("kind", K.D_OUT_KINDS)
@pytest.mark.parametrize("n", NS)
def test_the_mirror_sits_within_half_of_every_bound(n, kind, cases):
    c = cases[n, kind]
    for t in K.TENSORS:
        b, widened = K.bound(c["e32"][t], c["em"][t])
        print(f"n = {n} d(out) {kind} {t}: float32 reference {c['e32'][t]:.2e}, mirror {c['em'][t]:.2e}, bound {b:.2e}"
              + (" (widened: the mirror is beyond half of 4 x the reference's error)" if widened else ""))
        assert np.all(np.isfinite(c["gm"][t]))
        assert c["em"][t] <= 0.5 * b or (b == 0.0 and c["em"][t] == 0.0), (n, kind, t, c["em"][t], b)
        assert c["em"][t] <= 0.5 * K.CAP, (n, kind, t, c["em"][t])


@pytest.mark.parametrize("n", NS)
def test_zero_upstream_gradients_give_zero_gradients(n, cases):
    c = cases[n, "zero"]
    for t in K.TENSORS:
        assert not np.any(c["gm"][t]) and not np.any(c["g64"][t]), (n, t)


def test_a_pool_tie_goes_to_the_first_position(params):
    hap = K.make_haplotypes(9)
    assert len(set(hap[1])) == 1  # one base throughout: conv1's output is the same at every position
    _, _, arg = K.forward32(params, hap)
    assert not arg[1].any()
    assert arg[0].any() and not arg[0].all()  # (a random row has both)
    half = hap[5]
    assert len(set(half[:K.S // 2])) == 1 and half[0] != half[K.S // 2]  # two runs: ties inside them
    assert not arg[5][:, :3].any()


@pytest.mark.parametrize("mutant,tensor", [("drop_mid_hi", "conv1.weight"), ("one_piece", "conv1.weight"), ("unpadded", "conv2.weight")])
@pytest.mark.parametrize("n", [9, 257])
def test_a_mutant_breaks_the_bound(n, mutant, tensor, params, cases):
    c = cases[n, "normal"]
    gm = K.mirror(params, c["hap"], c["d"], *c["stash"], mutant=mutant)
    err = K.rel_l2(gm[tensor], c["g64"][tensor])
    b, _ = K.bound(c["e32"][tensor], c["em"][tensor])
    print(f"n = {n} {mutant}: {tensor} {err:.2e} against the bound {b:.2e}")
    assert err > b, (n, mutant, tensor, err, b)
    if mutant != "unpadded":  # what lies before phase 4 is untouched
        assert np.array_equal(gm["conv2.weight"], c["gm"]["conv2.weight"]) and np.array_equal(gm["linear.weight"], c["gm"]["linear.weight"])
