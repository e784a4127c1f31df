"""pmt_pack_params alone (csrc/pmt_pack.hip), through the C ABI, bit for bit against a decoder written from the documented layout in the
inverse direction (tests/pack_cases.py; tests/test_pack_params_cpu.py holds the decoder against a mirror of the kernel's own walk, the
region arithmetic, the mutants and the coverage of the kernel's branches).

The re-pack runs after every optimizer step and writes every operand the read-set kernels, the row MLPs and the CNN linears read; until
now it was held only through the 1e-4 parity of its consumers, which hides a wrong low piece (2^-11 of a weight), a destination emitted
twice or dropped in a padding column, and a write into the slack behind a region.  Here `packed` is the test's: every word starts as a
sentinel bit pattern, with guard words behind packed_size, and after ONE launch per model
  1. every word of every region (w_frag, wt_frag, b_pvec, wb_frag, wtb_frag, wh_frag, emit_tab, the block vectors, translation_pvec)
     equals the decoder's, bit for bit;
  2. padding rows, padding columns and absent k tiles hold exactly 0.0 in value tables and -1 in emit tables;
  3. every word the plan hands to no job still holds the sentinel: the padding of a region to 256 floats, the fragment of slack
     behind each 16-bit table, the 512 floats of tail slack, the guards;
  4. the destinations >= 0 of a read-set linear's emit table are the index set of W and b, each once -- in column in_dim with an empty
     tail under bias_cols where in_dim leaves padding, in the tail otherwise; the rotation's table indexes phi; a linear whose bias
     does not live in theta beside a theta weight has no bias destination (the eval-mode batch_norm model, which trains nowhere);
  5. read back and un-permuted, w_frag, hi + mid + lo of wb_frag and hi + lo / 4096 of wh_frag multiply a random float64 matrix to
     W x (exactly for the first two, to 2^-22 |W| |x| for the f16 pieces of the weights clamped to +-65504);
  6. a second call into the same buffer after theta and phi changed in place follows them, and after no change is bit-identical;
  7. a NULL model, theta or `packed` is PMT_E_INVALID and the sentinel stands.
Models: p0_b16, t0_b8, t0_two_sources (the third row MLP), p0_skip34, p0_deep, the eval-mode batch_norm model (linears that read phi),
wide_d98 and wide64_d98 (the wide builds; PMT_SPLIT0 = 32 for the latter), each under the library's own choice of instances and under
PMT_SHAPE=any (bias_cols 1 and 0), random parameters with 0.0, -0.0, 2^-15, 65504, 7e4 and two bf16 ties planted in every linear.

Exact: nothing is measured but the case list and the word counts (`record()`, profiles/bookkeeping_kernels_parity.jsonl)."""
import ctypes as C

import numpy as np
import pytest
import torch

from permutect_amd.engine import lib as L
from tests import pack_cases as K
from tests.test_scale_gpu import record

pytestmark = pytest.mark.gpu
DEV = "cuda"


class PackRun:
    def __init__(self, low: K.Lowered):
        self.low = low
        self.desc_dev = torch.frombuffer(bytearray(bytes(low.desc)), dtype=torch.uint8).to(DEV)
        self.theta, self.phi = torch.from_numpy(low.theta.copy()).to(DEV), torch.from_numpy(low.phi.copy()).to(DEV)
        words = np.full(low.desc.packed_size + K.GUARD, K.SENTINEL, np.uint32)
        self.packed = torch.from_numpy(words.view(np.int32).copy()).to(DEV)

    def call(self, model_host=True, model_dev=True, theta=True, packed=True):
        rc = self.low.lib.pmt_pack_params(C.byref(self.low.desc) if model_host else None, self.desc_dev.data_ptr() if model_dev else None,
                                          self.theta.data_ptr() if theta else None, self.phi.data_ptr(), self.packed.data_ptr() if packed else None, L.raw_stream())
        torch.cuda.synchronize()
        return rc

    def image(self):
        return self.packed.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("shape", K.SHAPES)
@pytest.mark.parametrize("name", K.MODELS)
def test_pack_params(name, shape):
    low = K.lowered(name, shape)
    assert K.build_split0(low) == low.split0 or not any(lin.out_split for lin in low.linears())
    run = PackRun(low)
    # 7. refused calls first: the sentinel stands
    for null in ("model_host", "model_dev", "theta", "packed"):
        assert run.call(**{null: False}) == L.E_INVALID, null
    assert (run.image() == K.SENTINEL).all()
    assert run.call() == 0
    first = run.image().copy()
    counts = K.check_image(low, first)  # 1. - 5.
    # 6. the same parameters again: bit-identical; other parameters, changed in place: the image follows
    assert run.call() == 0 and np.array_equal(run.image(), first)
    theta2, phi2 = K.fill_buffers(low, key=1)
    run.theta.copy_(torch.from_numpy(theta2))
    run.phi.copy_(torch.from_numpy(phi2))
    assert run.call() == 0
    second = run.image().copy()
    K.check_image(low, second, theta2, phi2)
    assert (second != first).sum() > 1000
    record(test="bookkeeping/pack_params", case=low.id, bias_cols=low.bias_cols, split0=low.split0, packed_size=low.desc.packed_size,
           **{k: (len(v) if isinstance(v, list) else v) for k, v in counts.items()})
