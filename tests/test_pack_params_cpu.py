"""The reference side of tests/test_pack_params_gpu.py, without a GPU (tests/pack_cases.py holds the table of models, the decoder and the
mirror).

Held here, on every model of the table under both shape choices: (1) the DECODER (natural (row, column) -> place, from the documented
layout) and the MIRROR (pmt_pack_kernel's own walk, fragment index -> (row, column)) give the same `packed` image bit for bit, so the
two derivations check each other before a device is asked; (2) the regions the plan hands to the kernel's jobs do not overlap, keep their
padding to 256 floats, the fragment of slack behind each 16-bit table and the 512 floats of tail slack, from the descriptor alone; (3) the
mirror's image passes every assertion the GPU test makes on the device's -- sentinels outside the regions, exact zeros / -1 in the padding,
every emit destination once, the read-back products; (4) teeth: each mutant of the mirror -- k block and row tile of the 16-bit tables
exchanged, the low f16 piece unscaled, split_row without its second half, the bias destination in the column and the tail -- breaks an
assertion on the table; (5) coverage: every `kind` of PMT_PACK_KINDS, every vector job and every branch of the kernel is reached by a
model of the table; (6) the build that runs a model has the PMT_SPLIT0 its plan was laid out with.

The linears without a bias destination (item 4 of the issue) are printed by test_linears_without_a_bias_destination: the rotation (no
bias at all) in every model, and every read-set linear of the eval-mode batch_norm model, whose weights and biases are folded into phi --
that model is refused by the training path (tests/test_host_cpu.py), so no gradient is ever emitted through such a table."""
import numpy as np
import pytest

from tests import pack_cases as K

CASES = [(m, s) for m in K.MODELS for s in K.SHAPES]


@pytest.mark.parametrize("name,shape", CASES)
def test_decoder_and_mirror_agree_and_the_image_passes_every_check(name, shape):
    low = K.lowered(name, shape)
    mask = K.owned_mask(low)  # (asserts the regions apart from each other and their slack)
    want, got = K.decode(low), K.pack_mirror(low)
    assert K.first_difference(low, got, want) is None, K.first_difference(low, got, want)
    counts = K.check_image(low, got)
    assert counts["words"] == mask.sum() and counts["sentinel_words"] >= K.TAIL_SLACK + 256 * 3 * low.desc.n_linear
    assert K.build_split0(low) == low.split0 or not any(lin.out_split for lin in low.linears()), "the build's PMT_SPLIT0 is not the plan's"
    # the planted values are where the tables can go wrong: each is present in every distinct weight
    for lin in low.linears():
        w = K.weight_of(low, lin)
        if w.size >= len(K.PLANTED):
            assert all((w == v).any() for v in K.PLANTED) and np.signbit(w[w == 0]).any() and not np.signbit(w[w == 0]).all()
    print(low.id, "bias_cols", low.bias_cols, counts)


def test_the_table_reaches_every_branch_of_the_kernel():
    """the coverage row: every kind of PMT_PACK_KINDS and every vector job is claimed by a model, and every branch inside them"""
    reached = {}
    for name, shape in CASES:
        for b in K.branches_of(K.lowered(name, shape)):
            reached.setdefault(b, []).append(f"{name}-{shape}")
    assert set(reached) == K.ALL_BRANCHES, (K.ALL_BRANCHES - set(reached), set(reached) - K.ALL_BRANCHES)
    assert {K.lowered(n, s).bias_cols for n, s in CASES} == {0, 1}
    assert all(K.lowered(n, "any").bias_cols == 0 for n in K.MODELS) and K.lowered("p0_b16", "auto").bias_cols == 1
    assert reached["third_row_mlp"] == ["t0_two_sources-auto", "t0_two_sources-any"]
    assert {r.split("-")[0] for r in reached["split0_32"]} == {"wide64_d98"} and {r.split("-")[0] for r in reached["b_in_phi"]} == {"p0_batchnorm_eval"}
    import re
    src = open(K.os.path.join(K.os.path.dirname(K.os.path.dirname(K.os.path.abspath(__file__))), "permutect_amd", "csrc", "pmt_pack.hip")).read()
    assert int(re.search(r"#define PMT_PACK_KINDS (\d+)", src).group(1)) == K.PACK_KINDS == len(K.KIND_NAMES)


def test_linears_without_a_bias_destination():
    listing = {}
    for name, shape in CASES:
        low = K.lowered(name, shape)
        none = K.check_image(low, K.pack_mirror(low))["no_bias_destination"]
        listing[low.id] = none
        if name == "p0_batchnorm_eval":  # every read-set linear reads phi: no table has a bias destination
            assert len(none) > 1 and all(low.desc.lin[i].w_src < 0 for i in none)
        else:                            # the rotation alone, which has no bias
            assert none == [low.desc.rotation_lin] and low.desc.lin[none[0]].b_src == -1
    print("linears whose emit table has no bias destination:", listing)


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_mutants_of_the_mirror_break_the_table(mutant):
    broken = []
    for name, shape in CASES:
        low = K.lowered(name, shape)
        try:
            K.check_image(low, K.pack_mirror(low, mutant=mutant))
        except AssertionError:
            broken.append(low.id)
    print(mutant, "breaks", broken)
    assert broken


def test_a_second_set_of_parameters_moves_the_image_and_the_same_set_does_not():
    low = K.lowered("p0_b16", "auto")
    theta2, phi2 = K.fill_buffers(low, key=1)
    a, b = K.pack_mirror(low), K.pack_mirror(low, theta2, phi2)
    assert (a != b).sum() > 1000 and np.array_equal(a, K.pack_mirror(low))
    K.check_image(low, b, theta2, phi2)
