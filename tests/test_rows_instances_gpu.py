"""Every compiled instance of the row-MLP kernels (csrc/pmt_rows.hip: pmt_rows_forward_kernel<TRAIN, WLDS, NT>, pmt_rows_backward_kernel<NT>,
pmt_rows_fold_kernel), alone, at every edge of the host arithmetic that picks and schedules it.

The harness calls the C ABI itself (pmt_rows_forward / pmt_rows_backward through ctypes) and owns every buffer the kernels touch: the input
with three junk columns behind each row (a kernel that ignored the stride would read them), outputs and d_in one row and three columns
larger than asked for and filled with a sentinel, a stash filled with NaN, a fresh zero `grad_theta` of theta_size, a zero workspace.  After
every call: the sentinels still stand, nothing of `grad_theta` outside the MLP's own parameters is touched, the workspace is zero again.
The reference is `oracle.artifact_oracle.mlp` in float64 with autograd on `loss = (out * W).sum()` (x requires a gradient too); the same call
in float32 is the YARDSTICK, never the target.  Dropout rows are given the masks `pmt_dropout_mask` exports.

ROWS is the instance table: (which MLP, input width, layer list) and the instance the row expects -- NT, WLDS, the wide first linear, gradient
replicas.  `assert_instance` restates rows_nt / rows_packed_span / ROWS_LDS_MAX_FLOATS / the wide-first rule / rows_param_span on the lowered
descriptor and holds each row to its expectation; tests/test_host_cpu.py::test_every_rows_kernel_instance_is_claimed_by_a_test_row compares
the table's union with the `pmt_rows_*_kernel` symbols of the libraries the build made (profiles/rows_instances_kernel_names.txt is the
kernel trace of one run of this file).

Row counts come from the launch arithmetic (256 rows per workgroup, a wave takes two tiles of 16): 0, 1, 15 .. 17, 31 .. 33, 255 .. 257; 1792 /
1793 (grid 7 -> 8: the gradient replicas start); 3072 / 3073 (grid 12 -> 13: fold slice 0 enters its four-in-flight loop); 4096 / 4097 (grid 16,
17); for the two production MLPs 65 536 / 65 537 (grid 256, 257: workgroup 256 shares replica 0).

Asserted per (row, n): both forwards (with and without a stash) element-wise at |err| <= 2e-5 x max(1, max|ref|) and bit-identical to each
other; the MLP's concatenated parameter gradient for a dense N(0, 1) W at relative L2 <= 1e-4 + 2 x yardstick; d_in element-wise at the
forward's bound + 2 x the float32 oracle's own max error; a second backward into the same grad_theta gives twice the gradient; W zero except
on ONE row (the first, the last, the first of the last tile / wave / workgroup, row 65 536) against that row's own float64 gradient, d_in
nonzero in that row only; d_in_scale 1.0, -0.01 and 0.0, d_in = None, the refusal of d_in behind a wide first linear; with the workspace,
without one and with one a float too small the same gradient up to summation order (relative L2 <= 5e-6); invalid arguments refused with
every buffer untouched; n = 0 launches nothing.

What the table found while it was written: no defect of the kernels or the entry points -- all twenty rows pass at every size on their
first run on an MI355X.  Two instances of the wide build had no candidate among the issue's layer lists (NT = 8 with the weights in LDS:
71 -> [100, -1, 20] is 43 520 packed floats); the row 71 -> [72, 20] (18 432) was added for them.

Measured on an MI355X (the bounds are not tightened to these): forward at most 3.3e-6 (eight ops, n = 1792) and at most 0.036 of its bound
(the production info MLP at 4096 rows: 2.5e-6 against 6.9e-5), the float32 oracle itself up to 1.7e-6; dense gradient at most 5.8e-7
against yardsticks of up to 1.9e-6, at most 0.006 of its bound (the source adversary at 4097 rows), the second backward the same;
one-hot gradient at most 4.3e-7 (0.004 of its bound; the 72 472-parameter MLP at 1793 rows); d_in at most 9.1e-7 against a float32 oracle
at 8.0e-7 (the wide build at 3072 rows, 0.024 of its bound), one-hot d_in at most 4.1e-7; without a workspace or with a short one at most
4.0e-7 from the replica path (65 536 rows); the parameter gradient with d_in_scale -0.01 / 0 / no d_in at
most 8.3e-8 from the one at scale 1.  Every measured (error, yardstick) pair is recorded with the suite's `record()`
(tests/test_scale_gpu.py; profiles/rows_instances_parity.jsonl is one run's lines).  The file runs in five seconds (the production info
MLP with its two 65 5xx sizes: 1.6 s; every other row at most 0.4 s)."""
import ctypes as C
import zlib
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from oracle import artifact_oracle as O
from permutect_amd.architecture.artifact_model import ArtifactModel
from permutect_amd.engine import lib as L
from permutect_amd.engine.lib import PmtError
from permutect_amd.parameters import p0_params
from tests.test_scale_gpu import record  # (appends a line to the suite's file of measured errors)

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5          # tests/test_cnn_instances_gpu.py FWD_TOL: |err| <= 2e-5 x max(1, max|ref|)
GRAD_TOL = 1e-4         # the gradient contract, relative L2
GRAD_YARDSTICKS = 2     # + this many times the float32 oracle's own relative L2 from fp64 (the CNN file's convention)
ORDER_TOL = 5e-6        # tests/test_scale_gpu.py: workspace against atomics, the same sum in another order
SENTINEL = -12345.5
JUNK = 777.0            # the three columns behind every input / d_out row
PAD = 3
SEED = 0x5EED0001CAFE   # the dropout seed every call passes (only an MLP lowered with dropout looks at it)
DROPOUT_P = 0.25        # (P of tests/test_dropout_gpu.py, whose mask_provider the dropout rows use)
ROWS_PER_BLOCK, TILE, WAVE_ROWS = 256, 16, 32  # csrc/pmt_rows.hip:14 ROWS_PER_BLOCK = PMT_WAVES x PMT_RT x 16 = 8 x 2 x 16
ROWS_REPLICAS = 256     # csrc/pmt_rows.hip:235
N_BIG = (65536, 65537)
PREFIX = {L.ROWS_INFO: "info_embedding", L.ROWS_ALT_COUNT: "alt_count_predictor.wrapped_module", L.ROWS_SOURCE: "source_predictor.wrapped_module"}


# ---- the table -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Row:
    id: str
    which: int
    in_dim: int            # the info vector's width (info rows); the reducer's output width, 10, for the adversaries
    layers: tuple          # behind the input, as ModelParameters writes them
    nt: int                # the register layout the row must reach: 2, 4 (PMT_NT of the default library), 8 (the wide library's)
    wlds: bool             # weights staged in LDS
    wide_first: bool       # the first linear reads more than PMT_MAX_WIDTH inputs: no d_in
    replicas: bool = True  # the parameter span fits 65 536 floats: replicas + fold from grid 8 on
    big: bool = False      # also at 65 536 / 65 537 rows
    dropout: float = 0.0
    sources: int = 1
    wide_lib: bool = False

    @property
    def kernels(self):
        b = lambda v: "true" if v else "false"  # noqa: E731
        return ((f"pmt_rows_forward_kernel<true, {b(self.wlds)}, {self.nt}>", f"pmt_rows_forward_kernel<false, {b(self.wlds)}, {self.nt}>",
                 f"pmt_rows_backward_kernel<{self.nt}>") + (("pmt_rows_fold_kernel",) if self.replicas else ()))


INFO, ALT, SRC = L.ROWS_INFO, L.ROWS_ALT_COUNT, L.ROWS_SOURCE
ROWS = [
    Row("A-info-production", INFO, 71, (20, -2, -2, -2), 2, True, True, big=True),            # 19 200 of 19 456 floats: 75 KiB of LDS, above 64 KiB
    Row("B-alt-count-production", ALT, 10, (30, -1, -1, -1, 1), 2, True, False, big=True),    # d_in
    Row("C-source-3", SRC, 10, (-1, -1, 3), 2, True, False, sources=3),                       # op 0 is a skip block, out_dim 3
    Row("D-info-just-over-lds", INFO, 71, (20, -2, -2, -2, 9), 2, False, True),               # 20 480 floats
    Row("E-info-nt4-lds", INFO, 71, (48, -1, 20), 4, True, True),
    Row("F-info-nt4-global", INFO, 71, (64, -2, 20), 4, False, True),
    Row("G-info-one-op", INFO, 40, (20,), 4, True, False),                                    # zero stash slots
    Row("H-info-deep-nt4", INFO, 71, (40, -3, -4, 20), 4, False, True),                       # skip_block_backward_deep
    Row("H-info-deep-nt2", INFO, 71, (24, -3, -4), 2, False, True),
    Row("I-info-span-beyond-65536", INFO, 71, (64, -4, -4, -4, -4, 20), 4, False, True, replicas=False),
    Row("J-info-eight-ops", INFO, 71, (20, -1, -1, -1, -1, -1, -1, -1), 2, False, True),
    Row("K-info-wide-global", INFO, 71, (100, -1, 20), 8, False, False, wide_lib=True),       # (PMT_MAX_WIDTH = 128 there: 71 inputs are not "wide")
    Row("K-info-wide-lds", INFO, 71, (72, 20), 8, True, False, wide_lib=True),
    Row("L-info-dropout", INFO, 71, (20, -2, -2, -2), 2, True, True, dropout=DROPOUT_P),
    Row("L-source-dropout", SRC, 10, (-1, -1, 3), 2, True, False, sources=3, dropout=DROPOUT_P),
    Row("M-info-32", INFO, 32, (20, -2), 2, True, False),                                     # the NT switch: 32 / 33
    Row("M-info-33", INFO, 33, (20, -2), 4, True, False),
    Row("M-info-64", INFO, 64, (20, -2), 4, True, False),                                     # the wide-first switch: 64 / 65
    Row("M-info-65", INFO, 65, (20, -2), 2, True, True),
    Row("M-info-128", INFO, 128, (20, -2), 2, True, True),                                    # the maximum
]
REFUSED = [  # lowering raises PmtError
    ("nine-ops", 71, (20, -1, -1, -1, -1, -1, -1, -1, -1), "exceeds the kernel limit"),
    ("129-inputs", 129, (20, -2), "exceeds"),
]


def claimed_kernels(wide_lib=None):
    """the union of the table's kernels: of the rows that run the default library (False), the wide one (True), all (None)"""
    return {k for row in ROWS if wide_lib is None or row.wide_lib == wide_lib for k in row.kernels}


def row_counts(row: Row):
    ns = [0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1792, 1793, 3072, 3073, 4096, 4097]
    return ns + (list(N_BIG) if row.big else [])


def probes(n: int):
    """the rows a one-hot W singles out at n: the first, the last, the first of the last tile / wave / workgroup, row 65 536"""
    last = n - 1
    vs = {0, last, last // TILE * TILE, last // WAVE_ROWS * WAVE_ROWS, last // ROWS_PER_BLOCK * ROWS_PER_BLOCK}
    if n > 65536:
        vs.add(65536)
    return sorted(vs)


# ---- the host arithmetic, restated on the lowered descriptor ------------------------------------------------------------------------
def linears_of(desc, which):
    """(op index, layer index in the op, PmtLinear) of every linear of a row MLP, in program order"""
    mlp = desc.row_mlp[which]
    for op in range(mlp.n_ops):
        o = mlp.ops[op]
        for k in range(o.n_layers if o.kind == L.OP_SKIP else 1):
            yield op, k, desc.lin[o.lin[k]]


def rows_nt(desc, which, max_width):
    """csrc/pmt_rows.hip:344-357 rows_nt: 2 when every activation behind the input fits two tiles, else PMT_NT = PMT_MAX_WIDTH / 16"""
    mlp = desc.row_mlp[which]
    if mlp.out_dim > 32 or (32 < mlp.in_dim <= max_width):
        return max_width // 16
    for op, k, lin in linears_of(desc, which):
        wide_first = op == 0 and k == 0 and mlp.in_dim > max_width
        if lin.out_dim > 32 or (lin.in_dim > 32 and not wide_first):
            return max_width // 16
    return 2


def rows_packed_span(desc, which):
    """csrc/pmt_rows.hip:323-341 rows_packed_span: the floats of `packed` from the first linear's fragments to the end of the last one's
    transposed fragments; :342, :369: staged in LDS when that is at most ROWS_LDS_MAX_FLOATS = 19 * 1024"""
    a, b = 2 ** 31 - 1, -1
    for _, _, lin in linears_of(desc, which):
        frag = ((lin.out_dim + 15) // 16) * ((lin.in_dim + 15) // 16) * 256
        assert lin.w_frag >= 0 and lin.wt_frag >= 0 and (lin.b_pvec < 0 or lin.w_frag <= lin.b_pvec < lin.wt_frag)
        a, b = min(a, lin.w_frag), max(b, lin.wt_frag + frag)
    assert b > a and a % 4 == 0 and (b - a) % 4 == 0
    return b - a


def rows_wlds(desc, which):
    return rows_packed_span(desc, which) <= 19 * 1024


def rows_wide_first(desc, which, max_width):
    """csrc/pmt_rows.hip:83, :193 (and :391, the refusal of d_in): in_dim > PMT_MAX_WIDTH"""
    return desc.row_mlp[which].in_dim > max_width


def rows_param_span(desc, which):
    """csrc/pmt_rows.hip:259-284 rows_param_span: [lo, hi) of theta over every weight, bias and alpha of the MLP; None beyond 65 536 floats"""
    mlp = desc.row_mlp[which]
    a, b = 2 ** 31 - 1, -1
    for op in range(mlp.n_ops):
        o = mlp.ops[op]
        if o.kind == L.OP_SKIP:
            a, b = min(a, o.alpha_src), max(b, o.alpha_src + 1)
    for _, _, lin in linears_of(desc, which):
        a, b = min(a, lin.w_src), max(b, lin.w_src + lin.in_dim * lin.out_dim)
        if lin.b_src >= 0:
            a, b = min(a, lin.b_src), max(b, lin.b_src + lin.out_dim)
    return None if (b <= a or b - a > (1 << 16)) else (a, b)


def assert_instance(row: Row, desc, lib, space, mlp_params):
    """the row reaches the instance it claims, by the restated arithmetic; the library is the one the row names"""
    limits = L.limits_of(lib)
    if row.wide_lib:
        assert limits["max_width"] == 128 and limits["max_half_ffn"] == 16, limits  # the wide build, which the build already makes
    else:
        assert lib is L.load() and limits["max_width"] == 64, limits
    mw = limits["max_width"]
    mlp = desc.row_mlp[row.which]
    assert (mlp.in_dim, mlp.out_dim) == (row.in_dim, O.mlp_output_dim([row.in_dim] + list(row.layers))), row.id
    assert mlp.n_ops == len(row.layers) and mlp.dropout == int(row.dropout > 0), row.id
    got = (rows_nt(desc, row.which, mw), rows_wlds(desc, row.which), rows_wide_first(desc, row.which, mw), rows_param_span(desc, row.which) is not None)
    assert got == (row.nt, row.wlds, row.wide_first, row.replicas), (row.id, got, rows_packed_span(desc, row.which))
    if row.id.startswith("A-"):
        assert rows_packed_span(desc, row.which) == 19200 and 4 * 19200 > 64 * 1024  # under the limit by 256 floats; LDS above 64 KiB
    # the workspace: 256 replicas of the parameter span, restated from the flat buffer's offsets
    lo = min(space.offset_of(p) for p in mlp_params)
    hi = max(space.offset_of(p) + p.numel() for p in mlp_params)
    want = ROWS_REPLICAS * (hi - lo) if hi - lo <= (1 << 16) else 0
    assert (want > 0) == row.replicas and int(lib.pmt_rows_workspace_floats(C.byref(desc), row.which)) == want, (row.id, lo, hi)
    if row.replicas:
        assert rows_param_span(desc, row.which) == (lo, hi)


# ---- the model under test --------------------------------------------------------------------------------------------------------
def make_model(which, in_dim, layers, device, dropout=0.0, sources=1):
    params = p0_params()
    params.dropout_p = dropout
    if which == INFO:
        params.info_layers = list(layers)
    torch.manual_seed(11)
    model = ArtifactModel(params, device=device, num_read_features=61, num_info_features=in_dim if which == INFO else 71, haplotypes_length=42)
    if sources > 1:
        model.reset_source_predictor(sources)
    named = [(k, p) for k, p in model.named_parameters() if k.startswith(PREFIX[which] + ".")]
    with torch.no_grad():
        for k, p in named:
            p.add_(0.05 * torch.randn_like(p))  # (away from the initialisation: zero-initialised biases hide their paths)
            if k.endswith(".alpha"):
                p.fill_(0.5)
    model.train(True)
    return model, named


def set_env(monkeypatch):
    for var in ("PMT_CNN", "PMT_CNN_DBG", "PMT_ROWS_WORKSPACE"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("PMT_SHAPE", "any")  # the generic read-set instances: whatever the info width makes of d_model, no library is built


def build_model(row: Row, monkeypatch, device):
    set_env(monkeypatch)
    model, named = make_model(row.which, row.in_dim, row.layers, device, row.dropout, row.sources)
    sd = {k: p.detach().cpu().clone() for k, p in named}
    return model, named, sd


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def stand_in_masks(p):
    """a seeded stand-in for pmt_dropout_mask (the CPU test of the table's reference side): a function of (linear, row, feature) as well"""
    def provide(key, y, row0=0):
        rows = []
        for r in range(row0, row0 + y.shape[0]):
            rng = np.random.default_rng([zlib.crc32(key.encode()), r])
            rows.append(np.where(rng.random(y.shape[1]) >= p, 1.0 / (1.0 - p), 0.0))
        return torch.from_numpy(np.asarray(rows, dtype=np.float32).reshape(tuple(y.shape)))
    return provide


class Oracle:
    """fp64 reference and fp32 yardstick of one table row over a fixed seeded (x, W).  The parameter gradient for the first n rows is a
    running sum over the chunks between the sizes asked for, so every row passes through autograd once per precision."""

    def __init__(self, row: Row, sd, masks=None):
        self.prefix, self.sizes, self.sd, self.keys, self.masks = PREFIX[row.which], [row.in_dim] + list(row.layers), sd, list(sd), masks
        self.n_max = max(row_counts(row))
        self.out_dim = O.mlp_output_dim(self.sizes)
        g = torch.Generator().manual_seed(1000 + zlib.crc32(row.id.encode()) % 1000)
        self.x = torch.randn(self.n_max, row.in_dim, generator=g, dtype=torch.float32)
        self.W = torch.randn(self.n_max, self.out_dim, generator=g, dtype=torch.float32)
        self.fwd = {d: torch.zeros(self.n_max, self.out_dim, dtype=torch.float64) for d in (torch.float64, torch.float32)}
        self.din = {d: torch.zeros(self.n_max, row.in_dim, dtype=torch.float64) for d in (torch.float64, torch.float32)}
        self.sums = {0: (0.0, 0.0)}
        self.single = {}

    def _run(self, a, b, dtype):
        sd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in self.sd.items()}
        x = self.x[a:b].to(dtype).requires_grad_(True)
        drop = None if self.masks is None else (lambda key, y: self.masks(key, y, a).to(dtype))
        out = O.mlp(sd, self.prefix, self.sizes, x, dropout=drop)
        grads = torch.autograd.grad((out * self.W[a:b].to(dtype)).sum(), [sd[k] for k in self.keys] + [x])
        return out.detach().double(), torch.cat([g.reshape(-1) for g in grads[:-1]]).double(), grads[-1].double()

    def upto(self, n):
        """of the first n rows with W[:n]: forward and d_in in both precisions [n, .], the parameter gradient in both"""
        if n not in self.sums:
            m = max(k for k in self.sums if k < n)
            g = list(self.sums[m])
            for a in range(m, n, 8192):
                b = min(n, a + 8192)
                for i, dtype in enumerate((torch.float64, torch.float32)):
                    out, gp, din = self._run(a, b, dtype)
                    self.fwd[dtype][a:b], self.din[dtype][a:b] = out, din
                    g[i] = g[i] + gp
            self.sums[n] = tuple(g)
        g64, g32 = self.sums[n]
        f = lambda t: t[:n].numpy()  # noqa: E731
        return dict(fwd=f(self.fwd[torch.float64]), fwd32=f(self.fwd[torch.float32]), din=f(self.din[torch.float64]), din32=f(self.din[torch.float32]),
                    g=np.asarray(g64, dtype=np.float64), g32=np.asarray(g32, dtype=np.float64))

    def one(self, v):
        """row v alone: (parameter gradient fp64, of the float32 oracle, d_in fp64 [in_dim], of the float32 oracle)"""
        if v not in self.single:
            r64, r32 = self._run(v, v + 1, torch.float64), self._run(v, v + 1, torch.float32)
            self.single[v] = (r64[1].numpy(), r32[1].numpy(), r64[2][0].numpy(), r32[2][0].numpy())
        return self.single[v]


def rel_l2(a, ref):
    return float(np.linalg.norm(a - ref) / max(float(np.linalg.norm(ref)), 1e-300))


def grad_bound(yardstick):
    return GRAD_TOL + GRAD_YARDSTICKS * yardstick


def elementwise_tol(ref, ref32):
    """the forward's bound on the scale of `ref`, plus twice the float32 oracle's own max error"""
    scale = float(np.abs(ref).max()) if ref.size else 0.0
    own = float(np.abs(ref32 - ref).max()) if ref.size else 0.0
    return FWD_TOL * max(1.0, scale) + 2 * own


# ---- the harness -----------------------------------------------------------------------------------------------------------------
F_WHICH, F_THETA, F_PACKED, F_IN, F_N, F_OUT = 2, 3, 4, 5, 7, 8             # positions in pmt_rows_forward's argument list
B_WHICH, B_THETA, B_PACKED, B_IN, B_N, B_DOUT, B_STASH, B_GTHETA = 2, 3, 4, 5, 7, 8, 10, 11  # ... in pmt_rows_backward's


class Harness:
    def __init__(self, row: Row, model, named, orc: Oracle):
        self.dev = torch.device("cuda")
        eng = model.engine()
        eng.pack(eng.plan.materialize_phi(model).detach().contiguous())  # the packed weight fragments the kernels read
        self.row, self.lib, self.desc, self.desc_dev, self.space = row, eng.lib, eng.plan.desc, eng.plan.desc_dev, eng.space
        self.theta, self.packed, self.eng = eng.space.theta, eng.plan.packed, eng
        self.params = [p for _, p in named]
        self.own = [(eng.space.offset_of(p), p.numel()) for p in self.params]
        self.theta_size = int(self.desc.theta_size)
        assert self.theta_size == self.theta.numel()
        self.outside = torch.ones(self.theta_size, dtype=torch.bool, device=self.dev)
        for o, k in self.own:
            self.outside[o:o + k] = False
        self.in_dim, self.out_dim = row.in_dim, orc.out_dim
        self.wide_first = row.wide_first
        # inputs: three junk columns behind every row, one junk row behind the last
        self.x = torch.full((orc.n_max + 1, self.in_dim + PAD), JUNK, dtype=torch.float32, device=self.dev)
        self.x[:orc.n_max, :self.in_dim] = orc.x.to(self.dev)
        self.W = torch.full((orc.n_max + 1, self.out_dim + PAD), JUNK, dtype=torch.float32, device=self.dev)
        self.W[:orc.n_max, :self.out_dim] = orc.W.to(self.dev)
        self.W1 = torch.full_like(self.W, JUNK)  # the one-hot upstream gradient: zero but for one row
        self.W1[:, :self.out_dim] = 0.0
        self.ws_floats = int(self.lib.pmt_rows_workspace_floats(C.byref(self.desc), row.which))
        self.ws = torch.zeros(self.ws_floats, dtype=torch.float32, device=self.dev) if self.ws_floats else None
        self.stream = L.raw_stream(self.dev)

    # -- argument lists (positional, so that the invalid-argument checks can replace one at a time)
    def forward_args(self, n, out, stash):
        return [C.byref(self.desc), self.desc_dev.data_ptr(), self.row.which, self.theta.data_ptr(), self.packed.data_ptr(), self.x.data_ptr(),
                self.x.stride(0), n, out.data_ptr(), out.stride(0), None if stash is None else stash.data_ptr(), SEED, self.stream]

    def backward_args(self, n, d_out, stash, gtheta, d_in, scale, ws, ws_floats):
        return [C.byref(self.desc), self.desc_dev.data_ptr(), self.row.which, self.theta.data_ptr(), self.packed.data_ptr(), self.x.data_ptr(),
                self.x.stride(0), n, d_out.data_ptr(), d_out.stride(0), stash.data_ptr(), gtheta.data_ptr(),
                None if d_in is None else d_in.data_ptr(), 0 if d_in is None else d_in.stride(0), scale,
                None if ws is None else ws.data_ptr(), ws_floats, SEED, self.stream]

    def new_out(self, n):
        return torch.full((max(n, 0) + 1, self.out_dim + PAD), SENTINEL, dtype=torch.float32, device=self.dev)

    def new_d_in(self, n):
        return torch.full((max(n, 0) + 1, self.in_dim + PAD), SENTINEL, dtype=torch.float32, device=self.dev)

    def new_stash(self, n):
        floats = int(self.lib.pmt_rows_stash_bytes(C.byref(self.desc), self.row.which, n)) // 4
        tiles = (n + ROWS_PER_BLOCK - 1) // ROWS_PER_BLOCK * (ROWS_PER_BLOCK // TILE)
        slots = max(self.desc.row_mlp[self.row.which].n_ops - 1, 1)  # (an MLP of one op keeps nothing; the size still is one slot per tile)
        assert floats == tiles * slots * L.limits_of(self.lib)["slot_floats"], (n, floats)
        return torch.full((max(floats, 4),), float("nan"), dtype=torch.float32, device=self.dev)

    @staticmethod
    def inner(buf, n, width, what):
        """a padded, sentinel-filled result -> its [n, width] part; row n and the columns behind `width` still hold the sentinel"""
        torch.cuda.synchronize()
        a = buf.cpu().numpy()
        assert np.all(a[n:] == SENTINEL) and np.all(a[:, width:] == SENTINEL), what
        return a[:n, :width].astype(np.float64)

    def forward(self, n, stash, what):
        out = self.new_out(n)
        rc = self.lib.pmt_rows_forward(*self.forward_args(n, out, stash))
        assert rc == 0, (what, rc)
        got = self.inner(out, n, self.out_dim, what)
        assert np.all(np.isfinite(got)), what
        return got

    def backward(self, n, d_out, stash, what, gtheta=None, d_in="auto", scale=1.0, ws="own", want_rc=0):
        """one pmt_rows_backward -> (the MLP's gradient [concatenated, fp64], d_in [n, in_dim] or None, grad_theta).  `ws`: "own" (the
        workspace of pmt_rows_workspace_floats), None, "short" (the same, declared one float too small)"""
        gtheta = torch.zeros(self.theta_size, dtype=torch.float32, device=self.dev) if gtheta is None else gtheta
        want_d_in = (not self.wide_first) if d_in == "auto" else bool(d_in)
        d_in_buf = self.new_d_in(n) if want_d_in else None
        ws_t = None if ws is None else self.ws
        ws_floats = 0 if ws_t is None else self.ws_floats - (1 if ws == "short" else 0)
        rc = self.lib.pmt_rows_backward(*self.backward_args(n, d_out, stash, gtheta, d_in_buf, scale, ws_t, ws_floats))
        assert rc == want_rc, (what, rc)
        d_in_got = None if d_in_buf is None else self.inner(d_in_buf, n if rc == 0 else 0, self.in_dim, what)
        torch.cuda.synchronize()
        assert float(gtheta[self.outside].abs().max()) == 0.0, (what, "grad_theta outside the MLP's own parameters")
        if self.ws is not None:
            assert float(self.ws.abs().max()) == 0.0, (what, "the workspace is not left zero")
        g = gtheta.cpu().numpy()
        return np.concatenate([g[o:o + k] for o, k in self.own]).astype(np.float64), d_in_got, gtheta


# ---- checks of one (row, n) ---------------------------------------------------------------------------------------------------------
def check_empty(h: Harness, what):
    """n = 0: PMT_OK, nothing launched, every buffer as it was"""
    stash = h.new_stash(0)
    for st in (None, stash):
        out = h.new_out(0)
        assert h.lib.pmt_rows_forward(*h.forward_args(0, out, st)) == 0, what
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), what
    g, d_in, gtheta = h.backward(0, h.W, stash, what)
    assert not g.any() and float(gtheta.abs().max()) == 0.0 and (d_in is None or d_in.shape[0] == 0), what
    assert bool(torch.isnan(stash).all()), what


def check_invalid(h: Harness, n, stash, what):
    """null pointers, `which` outside 0 .. 2, n < 0, an MLP that is not lowered: PMT_E_INVALID, nothing launched"""
    out, d_in = h.new_out(n), h.new_d_in(n)
    gtheta = torch.zeros(h.theta_size, dtype=torch.float32, device=h.dev)
    fa = lambda: h.forward_args(n, out, stash)  # noqa: E731
    ba = lambda: h.backward_args(n, h.W, stash, gtheta, None if h.wide_first else d_in, 1.0, h.ws, h.ws_floats)  # noqa: E731
    edits_f = [(0, None), (1, None), (F_THETA, None), (F_PACKED, None), (F_IN, None), (F_OUT, None), (F_WHICH, -1), (F_WHICH, 3), (F_N, -1)]
    edits_b = [(0, None), (1, None), (B_THETA, None), (B_PACKED, None), (B_IN, None), (B_DOUT, None), (B_STASH, None), (B_GTHETA, None),
               (B_WHICH, -1), (B_WHICH, 3), (B_N, -1)]
    if h.desc.row_mlp[SRC].n_ops == 0:  # (a model of one source lowers no source adversary)
        edits_f.append((F_WHICH, SRC))
        edits_b.append((B_WHICH, SRC))
    for pos, value in edits_f:
        args = fa()
        args[pos] = value
        assert h.lib.pmt_rows_forward(*args) == L.E_INVALID, (what, "forward", pos, value)
    for pos, value in edits_b:
        args = ba()
        args[pos] = value
        assert h.lib.pmt_rows_backward(*args) == L.E_INVALID, (what, "backward", pos, value)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((d_in == SENTINEL).all()) and float(gtheta.abs().max()) == 0.0, what
    assert h.ws is None or float(h.ws.abs().max()) == 0.0, what


def check_size(row: Row, h: Harness, orc: Oracle, n: int):
    what = f"{row.id} n={n}"
    if n == 0:
        check_empty(h, what)
        record(test="rows_instances", row=row.id, instance=list(row.kernels), n=0, forward_max_err=0.0)
        return None
    ref = orc.upto(n)
    # ---- forward: without a stash, with one
    out0 = h.forward(n, None, what + " forward")
    stash = h.new_stash(n)
    out1 = h.forward(n, stash, what + " training forward")
    assert np.array_equal(out0, out1), (what, "the two forwards differ")
    fwd_err, fwd_yard = float(np.abs(out0 - ref["fwd"]).max()), float(np.abs(ref["fwd32"] - ref["fwd"]).max())
    fwd_tol = FWD_TOL * max(1.0, float(np.abs(ref["fwd"]).max()))
    check_invalid(h, n, stash, what)
    # ---- backward, dense W ~ N(0, 1)
    yard = rel_l2(ref["g32"], ref["g"])
    g1, d_in1, gtheta = h.backward(n, h.W, stash, what + " dense")
    dense = rel_l2(g1, ref["g"])
    g2, _, _ = h.backward(n, h.W, stash, what + " second backward", gtheta=gtheta)  # no zeroing in between: the gradients add up
    twice = rel_l2(g2, 2 * ref["g"])
    d_in_err = d_in_tol = d_in_yard = 0.0
    if not row.wide_first:
        d_in_err, d_in_tol = float(np.abs(d_in1 - ref["din"]).max()), elementwise_tol(ref["din"], ref["din32"])
        d_in_yard = float(np.abs(ref["din32"] - ref["din"]).max())
    # ---- reversal: d_in_scale -0.01 and 0.0, no d_in at all; behind a wide first linear d_in is refused
    rev = {}
    if row.wide_first:
        g_ref, d_in_ref, gt = h.backward(n, h.W, stash, what + " d_in refused", d_in=True, want_rc=L.E_UNSUPPORTED)
        assert not g_ref.any() and float(gt.abs().max()) == 0.0 and d_in_ref.shape[0] == 0, (what, "a refused call launched something")
    else:
        g_m, d_in_m, _ = h.backward(n, h.W, stash, what + " scale -0.01", scale=-0.01)
        g_0, d_in_0, _ = h.backward(n, h.W, stash, what + " scale 0", scale=0.0)
        g_n, _, _ = h.backward(n, h.W, stash, what + " no d_in", d_in=False)
        rev = {"scale_-0.01": rel_l2(g_m, g1), "scale_0": rel_l2(g_0, g1), "no_d_in": rel_l2(g_n, g1)}
        rev_err = float(np.abs(d_in_m - (-0.01) * ref["din"]).max())
        rev_tol = elementwise_tol(0.01 * ref["din"], 0.01 * ref["din32"])
        product = (np.float32(-0.01) * d_in1.astype(np.float32)).astype(np.float64)  # (one float32 multiplication of what scale 1.0 stores)
    # ---- workspace: none, one float too small
    g_none, _, _ = h.backward(n, h.W, stash, what + " no workspace", ws=None)
    g_short, _, _ = h.backward(n, h.W, stash, what + " short workspace", ws="short" if h.ws is not None else None)
    ws_none, ws_short = rel_l2(g_none, g1), rel_l2(g_short, g1)
    # ---- one row at a time
    one_hot, one_hot_yard, one_hot_v, one_hot_din = 0.0, 0.0, -1, 0.0
    failures = []
    for v in probes(n):
        h.W1[v, :h.out_dim] = h.W[v, :h.out_dim]
        g, d_in, _ = h.backward(n, h.W1, stash, what + f" one-hot row {v}")
        h.W1[v, :h.out_dim] = 0.0
        r64, r32, din64, din32 = orc.one(v)
        e, y = rel_l2(g, r64), rel_l2(r32, r64)
        if e / grad_bound(y) >= one_hot / grad_bound(one_hot_yard):
            one_hot, one_hot_yard, one_hot_v = e, y, v
        if e > grad_bound(y):
            failures.append((what, "one-hot W at row", v, e, y))
        if d_in is not None:
            others = np.delete(d_in, v, axis=0)
            e_din = float(np.abs(d_in[v] - din64).max())
            one_hot_din = max(one_hot_din, e_din)
            if others.any() or e_din > elementwise_tol(din64, din32):
                failures.append((what, "d_in of one-hot W at row", v, e_din, int(np.count_nonzero(others))))
    record(test="rows_instances", row=row.id, instance=list(row.kernels), n=n, forward_max_err=fwd_err, forward_yardstick=fwd_yard,
           forward_bound=fwd_tol, grad_rel_l2_dense=dense, grad_rel_l2_twice=twice, yardstick=yard, bound=grad_bound(yard),
           d_in_max_err=d_in_err, d_in_yardstick=d_in_yard, d_in_bound=d_in_tol, grad_rel_l2_worst_one_hot=one_hot, one_hot_row=one_hot_v,
           one_hot_yardstick=one_hot_yard, one_hot_bound=grad_bound(one_hot_yard), one_hot_d_in_max_err=one_hot_din,
           no_workspace_rel_l2=ws_none, short_workspace_rel_l2=ws_short, **rev)
    print(f"{what}: forward {fwd_err:.2e} (yardstick {fwd_yard:.2e}, bound {fwd_tol:.2e}); dense {dense:.2e} twice {twice:.2e} (yardstick {yard:.2e}); "
          f"d_in {d_in_err:.2e} (yardstick {d_in_yard:.2e}, bound {d_in_tol:.2e}); one-hot {one_hot:.2e} at row {one_hot_v} (yardstick {one_hot_yard:.2e}); "
          f"no workspace {ws_none:.2e} short {ws_short:.2e} {rev}")
    assert fwd_err <= fwd_tol, (what, "forward", fwd_err, fwd_tol)
    assert dense <= grad_bound(yard), (what, "dense W", dense, yard)
    assert twice <= grad_bound(yard), (what, "two backwards into one grad_theta", twice, yard)
    assert not failures, failures
    if not row.wide_first:
        assert d_in_err <= d_in_tol, (what, "d_in", d_in_err, d_in_tol)
        assert rev_err <= rev_tol, (what, "d_in at scale -0.01", rev_err, rev_tol)
        assert np.all(np.abs(d_in_m - product) <= 2.0 ** -22 * np.abs(product) + 1e-37), (what, "d_in at scale -0.01 is not -0.01 x d_in at scale 1")
        assert not d_in_0.any(), (what, "d_in at scale 0")
        assert max(rev.values()) <= ORDER_TOL, (what, "the parameter gradient depends on d_in", rev)
    assert ws_none <= ORDER_TOL and ws_short <= ORDER_TOL, (what, "workspace against atomics", ws_none, ws_short)
    return dict(forward=fwd_err / fwd_tol, dense=max(dense, twice) / grad_bound(yard), one_hot=one_hot / grad_bound(one_hot_yard),
                d_in=d_in_err / d_in_tol if d_in_tol else 0.0)


# ---- the table, row by row -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_every_rows_instance_at_every_scheduling_edge(row, monkeypatch):
    from tests.test_dropout_gpu import mask_provider
    model, named, sd = build_model(row, monkeypatch, torch.device("cuda"))
    eng = model.engine()
    assert_instance(row, eng.plan.desc, eng.lib, eng.space, [p for _, p in named])
    assert abs(eng.plan.desc.dropout_p - row.dropout) < 1e-7
    orc = Oracle(row, sd, mask_provider(model, SEED) if row.dropout else None)
    h = Harness(row, model, named, orc)
    worst = {}
    for n in row_counts(row):
        ratios = check_size(row, h, orc, n)
        for k, v in (ratios or {}).items():
            worst[k] = max(worst.get(k, 0.0), v)
    record(test="rows_instances_worst", row=row.id, **{k + "_over_bound": v for k, v in worst.items()})


@pytest.mark.parametrize("name,in_dim,layers,message", REFUSED, ids=[r[0] for r in REFUSED])
def test_row_mlps_beyond_the_kernel_limits_are_refused_at_lowering(name, in_dim, layers, message, monkeypatch):
    set_env(monkeypatch)
    model, _ = make_model(INFO, in_dim, layers, torch.device("cuda"))
    with pytest.raises(PmtError, match=message):
        model.engine()
