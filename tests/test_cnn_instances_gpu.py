"""Every compiled instance of the haplotype-CNN kernels (csrc/pmt_cnn.hip "general", pmt_cnn2.hip "wave", pmt_cnn3.hip "batched"), alone,
at every edge of the rule that schedules it.

The harness drives `HaplotypeCnnFunction.apply(engine, hap, trigger)` directly with `loss = (out * W).sum()` for a chosen upstream
gradient W and reads the `haplotypes_cnn.*` gradients: no read sets, no losses.  The reference is `oracle.artifact_oracle.cnn` in
float64 with autograd on the same W; the same call in float32 is the YARDSTICK (how far fp32 arithmetic itself is from exact), never
the target.

ROWS is the instance table: (stack, haplotypes_length, forced family, switches, the kernel symbols the row must reach).
tests/test_host_cpu.py::test_every_cnn_kernel_instance_is_claimed_by_a_test_row compares its union with the `pmt_cnn*_kernel` symbols of
the gfx950 code objects the build made; profiles/cnn_instances_kernel_names.txt is the kernel trace of one run of this file.

What the table found while it was written:
  * an EMPTY batch (n = 0) was refused with PMT_E_INVALID by pmt_cnn_forward / pmt_cnn_backward: the entry points looked at the pointers
    before at n, and an empty tensor has no pointer.  They now return PMT_OK for n = 0 first (csrc/pmt_cnn.hip).
  * PMT_CNN=batched with PMT_CNN_STASH=0 does not "fall to the wave kernels" in the backward: a family asked for by name never falls back
    (pmt_cnn_backward: force_cnn == 3 -> PMT_E_UNSUPPORTED).  The row that reaches `cnn2_backward<2, 2, 6>` behind a batched forward is the
    UNFORCED dispatch with PMT_CNN_STASH=0; the forced one asserts the refusal.

Variant counts come from the launch arithmetic of each family, restated below beside the lines it restates (general_vpb, wave_waves,
batched: V x NW); nothing is sized for one stack.  Per instance: n = 0 and 1; one below / at / one above a workgroup's capacity and (batched)
a wave's batch; one below / at / one above one full grid round and two rounds + 1 (a workgroup loops and its last round is a tail of one
variant); 224 / 225 for the batched backward's switch between atomics and workspace rows; 66 001 once per family.

Asserted: every element of the forward against fp64 at the project's bound |err| <= 2e-5 x max(1, max|ref|); the concatenated CNN gradient
for a dense seeded N(0, 1) W at relative L2 <= 2e-4 + GRAD_YARDSTICKS x yardstick; the same for W that is zero except on ONE variant (the
first, the last, the first of the last batch / workgroup / grid round, one in a workgroup's second round) against that variant's own fp64
gradient -- a variant that the backward drops, reads from a neighbour's stash slot or counts twice is a 100 % error there; two backwards
without zeroing give twice the gradient.  GRAD_YARDSTICKS = 2 holds with room: measured on an MI355X, the worst case is the legacy stack on
the general kernels at 66 001 variants, 7.71e-4 against a yardstick of 7.72e-4 (0.44 of its bound: four leaky-ReLU layers, slopes that fp32
rounding flips, in the kernel as in the float32 oracle); every other case stays below 0.005 of its bound (dense 2 - 9e-7 against yardsticks
of 3e-7 - 1.4e-6; one-hot <= 3.0e-7).  Every measured pair (HIP error, yardstick) is recorded with the suite's `record()`
(tests/test_scale_gpu.py; profiles/cnn_instances_parity.jsonl is one run's lines)."""
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from oracle import artifact_oracle as O
from permutect_amd.architecture.artifact_model import ArtifactModel
from permutect_amd.engine.lib import PmtError
from permutect_amd.engine.runtime import HaplotypeCnnFunction, VariantEmbedFunction
from permutect_amd.parameters import P0_CNN, P0_CNN_LEGACY, T0_CNN, T0_CNN_OPTIONS, ModelParameters, p0_params
from tests.helpers import load_case
from tests.test_scale_gpu import record  # (appends a line to the suite's file of measured errors)

pytestmark = pytest.mark.gpu

N_BIG = 66001         # the scale test's size (tests/test_scale_gpu.py)
FWD_TOL = 2e-5        # tests/test_cnn_gpu.py: |err| <= 2e-5 x max(1, max|ref|)
GRAD_TOL = 2e-4       # tests/test_cnn_gpu.py: the CNN gradient's relative L2
GRAD_YARDSTICKS = 2   # + this many times the float32 oracle's own relative L2 from fp64 on the same inputs
OUT_DIM = 10

# ---- the stacks ------------------------------------------------------------------------------------------------------------------
_selu = lambda slots: [("selu" if i in slots else s) for i, s in enumerate(P0_CNN)]  # noqa: E731  (activation slots: 2 and 4)
STACKS = {
    "p0": list(P0_CNN), "t0": list(T0_CNN), "legacy": list(P0_CNN_LEGACY), "options": list(T0_CNN_OPTIONS),
    "p0_selu1": _selu({2}), "p0_selu2": _selu({4}), "p0_selu12": _selu({2, 4}),
    # a FIRST convolution of 10 x 5 = 50 im2col columns (four k-tiles): the wave backward that keeps six k-tiles of both convolutions' dW
    "wide_first": ["convolution/kernel_size=5/out_channels=32", "leaky_relu", "pool/kernel_size=2",
                   "convolution/kernel_size=3/out_channels=16", "selu", "flatten", "linear/out_features=10"],
    # grammar corners the fixture stacks leave out: a selu behind a STRIDED convolution, pool kernel 3 (21 -> 9 -> 3 -> 2 positions)
    "corners": ["convolution/kernel_size=4/stride=2/out_channels=16", "selu", "pool/kernel_size=3",
                "convolution/kernel_size=2/out_channels=12", "leaky_relu", "flatten", "linear/out_features=10"],
}
FIXTURE_OF = {"p0": "p0_b16", "t0": "t0_b8", "legacy": "p0_cnn_legacy", "options": "t0_cnn_options"}  # (their linears fit H = 40 as well: 9 pooled positions either way)

# ---- the kernel symbols (demangled, up to the argument list) ---------------------------------------------------------------------
GEN_F, GEN_B = "pmt_cnn_forward_kernel", "pmt_cnn_backward_kernel"
W_F2, W_F4 = "pmt_cnn2_forward_kernel<2>", "pmt_cnn2_forward_kernel<4>"
W_B22, W_B66, W_B4 = "pmt_cnn2_backward_kernel<2, 2, 6>", "pmt_cnn2_backward_kernel<2, 6, 6>", "pmt_cnn2_backward_kernel<4, 2, 1>"
B_F21, B_F0 = "pmt_cnn3_forward_kernel<4, 8, 3, 3, 7, 21>", "pmt_cnn3_forward_kernel<4, 8, 3, 3, 7, 0>"
B_BF21 = ("pmt_cnn3_forward_bf_kernel<4, 8, 3, 3, 7, 21, 2, 2, true>", "pmt_cnn3_forward_bf_kernel<4, 8, 3, 3, 7, 21, 2, 2, false>")
B_BF0 = ("pmt_cnn3_forward_bf_kernel<4, 8, 3, 3, 7, 0, 0, 0, true>", "pmt_cnn3_forward_bf_kernel<4, 8, 3, 3, 7, 0, 0, 0, false>")
B_BWD, B_FOLD = "pmt_cnn3_backward_kernel<8, 4, 3, 3, 7>", "pmt_cnn3_fold_kernel"


def kernel_name(symbol: str) -> str:
    """a demangled symbol or a kernel-trace name -> the form of the table: no return type, no argument list, no `.kd`"""
    s = symbol.strip().strip('"')
    s = s[5:] if s.startswith("void ") else s
    s = s.split("(")[0].strip()
    return s[:-3] if s.endswith(".kd") else s


@dataclass(frozen=True)
class Row:
    stack: str
    H: int
    family: str          # PMT_CNN: general | wave | batched | auto (unforced)
    kernels: tuple = ()  # what the row must reach; () with refuses: the family does not take the stack
    env: tuple = ()      # further switches
    big: bool = False    # also at N_BIG
    refuses: str = ""    # "forward": the training forward raises "not supported"; "backward": the backward does

    @property
    def id(self):
        return "-".join([self.stack, f"H{self.H}", self.family] + [f"{k[4:].lower()}{v}" for k, v in self.env])


ROWS = [
    # batched (pmt_cnn3.hip).  A forward under no_grad keeps no stash: the `false` instances
    Row("p0", 42, "batched", B_BF21 + (B_BWD, B_FOLD), big=True),
    Row("p0", 42, "batched", (B_F21, B_BWD, B_FOLD), env=(("PMT_CNN_DBG", "256"),)),
    Row("p0", 40, "batched", B_BF0 + (B_BWD, B_FOLD)),
    Row("p0", 40, "batched", (B_F0, B_BWD, B_FOLD), env=(("PMT_CNN_DBG", "256"),)),
    Row("p0_selu1", 42, "batched", B_BF0 + (B_BWD, B_FOLD)),
    Row("p0_selu2", 42, "batched", B_BF0 + (B_BWD, B_FOLD)),
    Row("p0_selu12", 42, "batched", B_BF0 + (B_BWD, B_FOLD)),
    Row("p0", 42, "batched", B_BF21 + (B_BWD,), env=(("PMT_CNN_WORKSPACE", "0"),)),  # every workgroup adds with atomics: no fold
    # no stash: the batched forward, then the wave backward recomputing it -- unforced; a forced family refuses instead of falling back
    Row("p0", 42, "auto", (B_BF21[1], W_B22), env=(("PMT_CNN_STASH", "0"),)),
    Row("p0", 40, "auto", (B_BF0[1], W_B22), env=(("PMT_CNN_STASH", "0"),)),
    Row("p0", 42, "batched", (B_BF21[1],), env=(("PMT_CNN_STASH", "0"),), refuses="backward"),
    # wave (pmt_cnn2.hip)
    Row("p0", 42, "wave", (W_F2, W_B22), big=True),
    Row("p0", 42, "wave", (W_F2, W_B22), env=(("PMT_CNN_STASH", "0"),)),
    Row("wide_first", 42, "wave", (W_F2, W_B66)),
    Row("t0", 42, "wave", (W_F4, W_B4), big=True),
    Row("t0", 40, "wave", (W_F4, W_B4)),
    # general (pmt_cnn.hip)
    Row("legacy", 42, "general", (GEN_F, GEN_B), big=True),
    Row("options", 42, "general", (GEN_F, GEN_B)),
    Row("p0", 42, "general", (GEN_F, GEN_B)),
    Row("t0", 42, "general", (GEN_F, GEN_B)),
    Row("corners", 42, "general", (GEN_F, GEN_B)),
    # refusals: a family asked for by name that does not take the stack fails loudly
    Row("legacy", 42, "wave", refuses="forward"), Row("legacy", 42, "batched", refuses="forward"),
    Row("options", 42, "wave", refuses="forward"), Row("options", 42, "batched", refuses="forward"),
    Row("t0", 42, "batched", refuses="forward"), Row("wide_first", 42, "batched", refuses="forward"),
]


def claimed_kernels():
    return {k for row in ROWS for k in row.kernels}


# ---- the launch arithmetic, restated ---------------------------------------------------------------------------------------------
def compute_units() -> int:
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def general_vpb(cnn):
    """variants per workgroup of the general kernels (forward, backward): csrc/pmt_cnn.hip pick_vpb and its two callers -- half of 156 KiB
    less the kernel's static LDS, divided by the floats a variant takes, 16 at most.  Static LDS: CnnFwdShared = int[192]; CnnBwdShared
    = int[192] + float[4][256] + int[256] + float4[32 * 64]."""
    def pick(per, static):
        lds = 156 * 1024 // 2
        return min(16, ((lds - static) // 4) // per) if lds > static else 0
    return pick(2 * cnn.max_act, 192 * 4), pick(cnn.sum_act + 2 * cnn.max_act, 192 * 4 + 4 * 256 * 4 + 256 * 4 + 32 * 64 * 16)


def wave_waves(cnn, backward):
    """(variants per workgroup = waves, workgroups per CU) of the wave kernels: csrc/pmt_cnn2.hip cnn2_waves / cnn2_stage_floats as
    pmt_cnn2_try_forward / _backward call them (weights staged in LDS when four waves still fit beside them)."""
    convs = [L for L in list(cnn.layers)[:cnn.n_layers] if L.kind == 0]
    stage = 4
    for L in list(cnn.layers)[:cnn.n_layers]:
        if L.kind == 0:  # PMT_CNN_CONV: fragments of W (in_dim = in_ch x kernel), a bias tile per out tile, and W^T behind the first convolution
            ot, it = (L.out_ch + 15) // 16, (L.in_ch * L.kernel + 15) // 16
            stage += ot * it * 256 + 256 + 16 * ot + ((ot * it * 256 + 256) if (backward and L.in_off != 0) else 0)
        elif L.kind == 5:  # PMT_CNN_LINEAR
            stage += (L.out_ch * L.in_ch * L.in_len + 3) & ~3
    assert convs
    per = cnn.sum_act + (2 * cnn.max_act if backward else 0)
    static = 4 * 2 * 128 + (4 * 8 * 16 if backward else 0)

    def waves(static_bytes):
        half = min(8, (78 * 1024 - static_bytes) // (4 * per)) if 78 * 1024 > static_bytes else 0
        if half >= 4:
            return half, 2
        return (min(8, (156 * 1024 - static_bytes) // (4 * per)) if 156 * 1024 > static_bytes else 0), 1
    nw, per_cu = waves(static + 4 * stage)
    if nw < 4:
        nw, per_cu = waves(static)
    return nw, per_cu


BATCHED_WG, BATCHED_FWD_V, BATCHED_BWD_V = 32, 4, 8  # csrc/pmt_cnn3.hip: C3_FWD_V x C3_FWD_NW = C3_BWD_V x C3_BWD_NW = 32; cnn3_grid: min(ceil(n / 32), CUs)


@dataclass
class Schedule:
    ns: list      # the variant counts
    batch: int    # variants a wave of the BACKWARD takes at a time
    wg: int       # ... a workgroup takes per round
    round: int    # ... the whole grid takes per round (0: the grid never loops)


def schedule(row: Row, cnn) -> Schedule:
    cus = compute_units()
    edges = lambda x: [x - 1, x, x + 1]  # noqa: E731
    rounds = lambda r: edges(r) + [2 * r + 1]  # noqa: E731
    ns = [0, 1]
    batched_fwd = row.family in ("batched", "auto")
    wave_bwd = row.family == "wave" or (row.family == "auto" and dict(row.env).get("PMT_CNN_STASH") == "0")
    if batched_fwd:
        ns += edges(BATCHED_FWD_V) + edges(BATCHED_BWD_V) + edges(BATCHED_WG) + [224, 225] + rounds(BATCHED_WG * cus)
        s = Schedule(ns, BATCHED_BWD_V, BATCHED_WG, BATCHED_WG * cus)
    if row.family == "wave":
        nw, per_cu = wave_waves(cnn, False)
        assert nw >= 2, "the wave forward does not take this stack"
        ns += edges(nw) + rounds(nw * cus * per_cu)
    if wave_bwd:
        nw, per_cu = wave_waves(cnn, True)
        assert nw >= 2, "the wave backward does not take this stack"
        ns += edges(nw) + rounds(nw * cus * per_cu)
        s = Schedule(ns, 1, nw, nw * cus * per_cu)
    if row.family == "general":
        vf, vb = general_vpb(cnn)
        assert vf >= 1 and vb >= 1
        ns += edges(vf) + [2 * vf + 1] + edges(vb) + [2 * vb + 1, 2049]  # (2049: a thousand and more workgroups adding into the gradient)
        s = Schedule(ns, vb, vb, 0)
    if row.big:
        ns.append(N_BIG)
    s.ns = sorted({n for n in ns if n >= 0})
    return s


def probes(n: int, s: Schedule) -> list:
    """the variants a one-hot W singles out at n: the first, the last, the first of the last batch / workgroup / grid round, and one
    that a workgroup meets in its second round"""
    if n < 2:
        return []
    last = n - 1
    vs = {0, last, last // s.batch * s.batch, last // s.wg * s.wg}
    if s.round:
        vs.add(last // s.round * s.round)
        if n > s.round + 1:
            vs.add(s.round + 1)
    return sorted(vs)


# ---- inputs and the oracle -------------------------------------------------------------------------------------------------------
def make_haplotypes(n, H, seed):
    """U{0..4} codes; every seventh row is an edge of the encoding: one base throughout (A, C, G, T), ref == alt, code 4 (no base) only"""
    rng = np.random.default_rng(seed)
    hap = rng.integers(0, 5, (n, H), dtype=np.int64)
    for i in range(3, n, 7):
        kind = (i // 7) % 6
        if kind < 4:
            hap[i] = kind
        elif kind == 4:
            hap[i, H // 2:] = hap[i, :H // 2]
        else:
            hap[i] = 4
    return torch.from_numpy(hap)


class Oracle:
    """fp64 reference and fp32 yardstick of one (stack, H, weights) over a fixed seeded (hap, W) of N_BIG variants.  The gradient for the
    first n variants is kept as a running sum over the chunks between the sizes asked for, so every variant passes through autograd once
    per precision however many sizes the rows ask for."""

    def __init__(self, layers, H, sd):
        self.layers, self.sd, self.keys = layers, sd, list(sd.keys())
        self.hap = make_haplotypes(N_BIG, H, seed=1000 + H)
        self.W = torch.randn(N_BIG, OUT_DIM, generator=torch.Generator().manual_seed(77), dtype=torch.float32)
        self.fwd = torch.zeros(N_BIG, OUT_DIM, dtype=torch.float64)
        self.sums = {0: (0.0, 0.0)}
        self.single = {}

    def _run(self, hap, W, dtype):
        old = O.COMPUTE_DTYPE
        O.COMPUTE_DTYPE = dtype
        try:
            sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in self.sd.items()}
            out = O.cnn(sd, "haplotypes_cnn", self.layers, O.one_hot_haplotypes(hap))
            grads = torch.autograd.grad((out * W.to(dtype)).sum(), [sd[k] for k in self.keys])
        finally:
            O.COMPUTE_DTYPE = old
        return out.detach(), torch.cat([g.reshape(-1) for g in grads])

    def upto(self, n):
        """(forward [n, OUT_DIM] fp64, gradient fp64, gradient of the float32 oracle) of the first n variants with W[:n]"""
        if n not in self.sums:
            m = max(k for k in self.sums if k < n)
            g64, g32 = self.sums[m]
            for a in range(m, n, 8192):
                b = min(n, a + 8192)
                out, g = self._run(self.hap[a:b], self.W[a:b], torch.float64)
                self.fwd[a:b] = out
                g64 = g64 + g
                g32 = g32 + self._run(self.hap[a:b], self.W[a:b], torch.float32)[1]
            self.sums[n] = (g64, g32)
        g64, g32 = self.sums[n]
        return self.fwd[:n].numpy(), np.asarray(g64, dtype=np.float64), np.asarray(g32, dtype=np.float64)

    def one(self, v):
        if v not in self.single:
            g64 = self._run(self.hap[v:v + 1], self.W[v:v + 1], torch.float64)[1].numpy()
            g32 = self._run(self.hap[v:v + 1], self.W[v:v + 1], torch.float32)[1].numpy().astype(np.float64)
            self.single[v] = (g64, g32)
        return self.single[v]


_ORACLES = {}


def oracle_for(stack, H, sd):
    key = (stack, H)
    got = _ORACLES.get(key)
    if got is None or any(not torch.equal(got.sd[k], sd[k]) for k in sd):
        got = _ORACLES[key] = Oracle(STACKS[stack], H, sd)
    return got


def rel_l2(a, ref):
    return float(np.linalg.norm(a - ref) / max(float(np.linalg.norm(ref)), 1e-300))


# ---- the model under test --------------------------------------------------------------------------------------------------------
def build_model(row: Row, monkeypatch, params=None):
    for var in ("PMT_CNN", "PMT_CNN_DBG", "PMT_CNN_STASH", "PMT_CNN_WORKSPACE"):
        monkeypatch.delenv(var, raising=False)
    if row.family != "auto":
        monkeypatch.setenv("PMT_CNN", row.family)
    for k, v in row.env:
        monkeypatch.setenv(k, v)
    if params is None:
        params = p0_params()
    params.ref_seq_layer_strings = list(STACKS[row.stack])
    torch.manual_seed(11)
    model = ArtifactModel(params, device=torch.device("cuda"), num_read_features=61, num_info_features=71, haplotypes_length=row.H)
    cnn_params = [(k, p) for k, p in model.named_parameters() if k.startswith("haplotypes_cnn.")]
    with torch.no_grad():
        for _, p in cnn_params:
            p.add_(0.05 * torch.randn_like(p))  # (away from the initialisation: zero-initialised biases hide their paths)
        if row.stack in FIXTURE_OF:
            _, fsd, _ = load_case(FIXTURE_OF[row.stack])
            for k, p in cnn_params:
                p.copy_(fsd[k].to(p.device))
    model.train(True)
    eng = model.engine()
    eng.draw_dropout_seed(False)
    eng.pack(eng.plan.materialize_phi(model).detach().contiguous())  # the packed weight fragments the kernels read (artifact_model._encode)
    sd = {k: p.detach().cpu().clone() for k, p in cnn_params}
    assert list(sd) == [k for k in model.state_dict() if k.startswith("haplotypes_cnn.")]
    return model, eng, sd


def zero_grads(model, eng):
    model.zero_grad()
    eng.space.gtheta.zero_()  # (the flat gradient buffer the .grad views alias)


def cnn_grad(model):
    torch.cuda.synchronize()
    return np.concatenate([(p.grad.detach().cpu().numpy().ravel() if p.grad is not None else np.zeros(p.numel(), np.float32))
                           for k, p in model.named_parameters() if k.startswith("haplotypes_cnn.")]).astype(np.float64)


def backward_once(eng, hap, W):
    out = HaplotypeCnnFunction.apply(eng, hap, eng.trigger)
    (out * W).sum().backward()
    return out


def check_forward(out, ref, what):
    assert tuple(out.shape) == ref.shape, what
    got = out.detach().cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)), what
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    tol = FWD_TOL * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    assert err <= tol, (what, err, tol)
    return err


def grad_bound(yardstick):
    return GRAD_TOL + GRAD_YARDSTICKS * yardstick


# ---- the table, row by row -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_every_instance_at_every_scheduling_edge(row, monkeypatch):
    model, eng, sd = build_model(row, monkeypatch)
    dev = torch.device("cuda")
    orc = oracle_for(row.stack, row.H, sd)
    if row.refuses:
        hap, W = orc.hap[:33].to(dev), orc.W[:33].to(dev)
        zero_grads(model, eng)
        if row.refuses == "forward":
            with pytest.raises(PmtError, match="not supported"):
                HaplotypeCnnFunction.apply(eng, hap, eng.trigger)
        else:
            out = HaplotypeCnnFunction.apply(eng, hap, eng.trigger)
            check_forward(out, orc.upto(33)[0], row.id)
            with pytest.raises(PmtError, match="not supported"):
                (out * W).sum().backward()
        return
    sch = schedule(row, eng.plan.desc.cnn)
    worst = {"forward": 0.0, "dense": 0.0, "one_hot": 0.0}
    for n in sch.ns:
        hap, W = orc.hap[:n].to(dev), orc.W[:n].to(dev)
        fwd, g64, g32 = orc.upto(n)
        what = f"{row.id} n={n}"
        # forward: without a stash (no_grad) and the training forward
        with torch.no_grad():
            e0 = check_forward(HaplotypeCnnFunction.apply(eng, hap, eng.trigger), fwd, what + " eval")
        zero_grads(model, eng)
        e1 = check_forward(backward_once(eng, hap, W), fwd, what + " train")
        g1 = cnn_grad(model)
        if n == 0:  # an empty batch: an empty result, no launch, the gradients untouched
            assert not g1.any(), what
            record(test="cnn_instances", row=row.id, family=row.family, instance=list(row.kernels), n=0, forward_max_err=0.0)
            continue
        yard = rel_l2(g32, g64)
        dense = rel_l2(g1, g64)
        backward_once(eng, hap, W)  # no zeroing in between: the gradients add up
        twice = rel_l2(cnn_grad(model), 2 * g64)
        # one variant at a time
        one_hot, one_hot_yard, one_hot_v = 0.0, 0.0, -1
        for v in probes(n, sch):
            W1 = torch.zeros_like(W)
            W1[v] = W[v]
            zero_grads(model, eng)
            backward_once(eng, hap, W1)
            r64, r32 = orc.one(v)
            e, y = rel_l2(cnn_grad(model), r64), rel_l2(r32, r64)
            if e / grad_bound(y) >= one_hot / grad_bound(one_hot_yard):
                one_hot, one_hot_yard, one_hot_v = e, y, v
        record(test="cnn_instances", row=row.id, family=row.family, instance=list(row.kernels), n=n, forward_max_err=max(e0, e1),
               grad_rel_l2_dense=dense, grad_rel_l2_twice=twice, yardstick=yard, bound=grad_bound(yard),
               grad_rel_l2_worst_one_hot=one_hot, one_hot_variant=one_hot_v, one_hot_yardstick=one_hot_yard, one_hot_bound=grad_bound(one_hot_yard))
        print(f"{what}: forward {max(e0, e1):.2e}; dense {dense:.2e} twice {twice:.2e} (yardstick {yard:.2e}); "
              f"one-hot {one_hot:.2e} at variant {one_hot_v} (yardstick {one_hot_yard:.2e})")
        assert dense <= grad_bound(yard), (what, "dense W", dense, yard)
        assert twice <= grad_bound(yard), (what, "two backwards", twice, yard)
        assert one_hot <= grad_bound(one_hot_yard), (what, "one-hot W at variant", one_hot_v, one_hot, one_hot_yard)
        worst = {"forward": max(worst["forward"], e0, e1), "dense": max(worst["dense"], dense / grad_bound(yard)),
                 "one_hot": max(worst["one_hot"], one_hot / grad_bound(one_hot_yard))}
    record(test="cnn_instances_worst", row=row.id, forward_max_err=worst["forward"], dense_over_bound=worst["dense"], one_hot_over_bound=worst["one_hot"])


# ---- strides, integer types -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["batched", "wave", "general"])
def test_haplotypes_as_a_column_slice_and_as_narrow_integers(family, monkeypatch):
    """`hap` as the loader hands it over -- the haplotype columns of an int64 [n, 16 + H] array (row stride 58) -- and as int32 / int16 (the
    `.long()` path): the same results as the contiguous int64 tensor's reference."""
    row = Row("p0", 42, family)
    model, eng, sd = build_model(row, monkeypatch)
    dev = torch.device("cuda")
    orc = oracle_for("p0", 42, sd)
    for n in (1, 33, 301):
        fwd, g64, g32 = orc.upto(n)
        W = orc.W[:n].to(dev)
        ints = torch.full((n, 16 + 42), 3, dtype=torch.int64)  # (a kernel that ignored the stride would read these 3s)
        ints[:, 16:] = orc.hap[:n]
        views = {"int64 stride 58": ints.to(dev)[:, 16:], "int32": orc.hap[:n].to(torch.int32).to(dev), "int16": orc.hap[:n].to(torch.int16).to(dev)}
        assert views["int64 stride 58"].stride(0) == 58
        for name, hap in views.items():
            zero_grads(model, eng)
            check_forward(backward_once(eng, hap, W), fwd, f"{family} {name} n={n}")
            err, yard = rel_l2(cnn_grad(model), g64), rel_l2(g32, g64)
            record(test="cnn_instances_strides", family=family, input=name, n=n, grad_rel_l2_dense=err, yardstick=yard)
            assert err <= grad_bound(yard), (family, name, n, err, yard)


# ---- through VariantEmbedFunction: the CNN's column block at 4-, 4- and 8-byte aligned bases ---------------------------------------
EMBED_MODELS = {  # info-MLP output width: (read layers, d_ffn, blocks, info layers, aggregation layers) -- shapes of tests/test_shapes_gpu.py with the info width changed
    7: ([16], 40, 2, [7], [12]),
    9: ([16], 40, 2, [9], [12]),
    50: ([30, -2], 20, 4, [50, -1], [-2, 10]),
}


@pytest.mark.parametrize("family", ["batched", "wave", "general"])
@pytest.mark.parametrize("e_info", [7, 9, 50])
def test_cnn_columns_of_the_variant_embedding_at_odd_info_widths(e_info, family, monkeypatch):
    """VariantEmbedFunction hands the CNN `ve + 4 * e_info` bytes with row stride e_info + 10: with an odd e_info the CNN's output and its
    upstream gradient start 4-byte aligned.  Haplotype columns and all CNN gradients against fp64, the info columns against the oracle's
    info MLP (so the column just left of the CNN block is what the row kernel wrote, untouched by the CNN launch)."""
    rl, dffn, nb, il, al = EMBED_MODELS[e_info]
    row = Row("p0", 42, family)
    model, eng, sd = build_model(row, monkeypatch, ModelParameters(rl, dffn, nb, il, al, 4, [10, 10], list(P0_CNN), 0.0, 0.3))
    dev = torch.device("cuda")
    orc = oracle_for("p0", 42, sd)
    full = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for n in (33, 301):
        fwd, g64, g32 = orc.upto(n)
        info = torch.randn(n, 71, generator=torch.Generator().manual_seed(5), dtype=torch.float32)
        Wv = torch.randn(n, e_info + OUT_DIM, generator=torch.Generator().manual_seed(6), dtype=torch.float32)
        Wv[:, e_info:] = orc.W[:n]
        zero_grads(model, eng)
        ve = VariantEmbedFunction.apply(eng, info.to(dev), orc.hap[:n].to(dev), eng.trigger)
        assert tuple(ve.shape) == (n, e_info + OUT_DIM) and ve.data_ptr() % 16 == 0  # the CNN's base: 12, 4, 8 bytes past a 16-byte boundary
        (ve * Wv.to(dev)).sum().backward()
        check_forward(ve[:, e_info:], fwd, f"{family} e_info={e_info} n={n}")
        with torch.no_grad():
            info_ref = O.mlp(full, "info_embedding", [71] + il, info).numpy().astype(np.float64)
        check_forward(ve[:, :e_info], info_ref, f"{family} e_info={e_info} n={n} info columns")
        err, yard = rel_l2(cnn_grad(model), g64), rel_l2(g32, g64)
        record(test="cnn_instances_embed", family=family, e_info=e_info, n=n, grad_rel_l2_dense=err, yardstick=yard)
        assert err <= grad_bound(yard), (family, e_info, n, err, yard)


# ---- the new length, end to end ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2])
def test_haplotypes_of_length_40_through_the_whole_model(seed):
    """haplotypes_length = 40 (20 bases of context) through Batch, the loader's column layout and VariantEmbedFunction: losses and every
    gradient of a P0 model against the oracle's autograd, with the tolerances of test_random_mixed_batches_match_oracle."""
    from permutect_amd.data.batch import Batch
    from permutect_amd.training.optimizer import FusedClipAdamW
    from tests.test_train_gpu import _compare_gradients
    H = 40
    rng = np.random.default_rng(300 + seed)
    nb = 28
    kinds = rng.integers(0, 4, nb)
    nref = np.where(kinds == 0, 0, np.where(kinds == 1, 1, np.where(kinds == 2, rng.integers(0, 11, nb), rng.integers(0, 60, nb))))
    nalt = np.where(kinds == 0, 1, np.where(kinds == 1, 1, np.where(kinds == 2, rng.integers(1, 16, nb), rng.integers(1, 60, nb))))
    ints = np.zeros((nb, 16 + H), dtype=np.int16)
    ints[:, 0], ints[:, 1], ints[:, 2] = nref, nalt, rng.integers(0, 3, nb)
    ints[:, 16:] = rng.integers(0, 5, (nb, H))
    floats = np.zeros((nb, 6 + 71), dtype=np.float16)
    floats[:, 6:] = rng.standard_normal((nb, 71)).astype(np.float16)
    packed = rng.integers(0, 256, (int(nref.sum() + nalt.sum()), 12), dtype=np.uint8)
    _, sd, _ = load_case("p0_b16")  # (the linear behind the flatten has 32 x 7 inputs at 20 positions as at 21)
    cfg = O.Config([30, -2, -2, -2], [20, -2, -2, -2], [-2, -2, 10], 20, 6, 4, list(P0_CNN), 61, 71, H)
    dev = torch.device("cuda")
    model = ArtifactModel(p0_params(), device=dev, num_read_features=61, num_info_features=71, haplotypes_length=H)
    model.load_state_dict(sd)
    model.train(True)
    batch = Batch.from_arrays(ints, floats, packed).copy_to(dev)
    out = model.compute_batch_output(batch)
    losses = model.compute_batch_losses(out, batch)
    opt = FusedClipAdamW(model, lr=1e-3, weight_decay=0.01)
    opt.zero_grad()
    losses.total_loss.backward()
    torch.cuda.synchronize()
    i64 = torch.from_numpy(ints.astype(np.int64))
    ob = dict(reads_re=torch.from_numpy(O.decode_packed_reads(packed).astype(np.float32)), nref=i64[:, O.REF_COUNT],
              nalt=i64[:, O.ALT_COUNT], labels=i64[:, O.LABEL], sources=i64[:, O.SOURCE],
              info_be=torch.from_numpy(floats[:, O.INFO_START:].astype(np.float32)), haplotypes_bh=i64[:, O.HAPLOTYPES_START:])
    assert ob["haplotypes_bh"].shape[1] == H
    _, ref_losses, ref_grads = O.train_step_grads(sd, cfg, ob)
    ref_total = ref_losses["total_losses_b"].detach().numpy()
    np.testing.assert_allclose(losses.total_losses_b.detach().cpu().numpy(), ref_total, rtol=1e-4, atol=1e-4 + 1e-5 * np.abs(ref_total).max())
    _compare_gradients(model, {k: v.numpy() for k, v in ref_grads.items()})
