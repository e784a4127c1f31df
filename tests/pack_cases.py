"""What tests/test_pack_params_cpu.py and tests/test_pack_params_gpu.py share: the table of lowered models, a DECODER of `packed` written
from the documented layout in the inverse direction, and a numpy MIRROR of pmt_pack_kernel's own forward map (with the mutants of the CPU
test as switches).  Nothing here needs a GPU: a model is lowered on the CPU (`EnginePlan(model, ParamSpace(model, cpu), cpu)`), and the
kernel reads nothing of it but the descriptor and two flat float buffers, which the tests fill themselves.

The kernel (csrc/pmt_pack.hip) walks every table by fragment index and asks which (row, column) belongs there.  The decoder walks the
natural matrix and asks where (row, column) goes, from what include/permutect_amd.h (PmtLinear) and csrc/pmt_device.hpp say:
  * position p of a 16-feature tile holds feature 4 (p & 3) + (p >> 2), so feature f sits at position 4 (f % 4) + f / 4;
  * an fp32 A fragment is [k tile][row tile][lane = 16 g + row position][register j] with k = 16 kt + 4 j + g (kt-major: the order
    linear_acc walks them);
  * the bf16 pieces are [k block of 32][row tile][piece][lane = 16 kg + row position][8] with element e = 4 (k tile & 1) + (k % 16) / 4 and
    kg = k % 4 -- the feature order of two fp32 activation tiles --, three pieces hi, mid, lo with hi + mid + lo = w;
  * the f16 pieces are [row tile][k block][piece][lane][8] (row tile FIRST, as the header says), the same element order, two pieces
    f16(w) and f16(2^12 (w - f16(w))) of w clamped to +-65504;
  * a gated block's first projection (out_split = h) has virtual output rows: row o < h at o, row h + r at split0 + r, split0 =
    16 ceil(h / 16) (PMT_SPLIT0 of the build that runs the model);
  * the emit table is [(out tile, in tile)][lane = 16 g + column position][register j] with row feature 4 j + g (the matrix core's C
    layout), holding w_off + o in_dim + c, then per out tile sixteen bias destinations in position order; in a model of the exact-width
    instances (bias_cols) a linear whose in_dim leaves padding in its last tile has its bias destinations in column in_dim and an empty
    tail; a bias that does not live in theta beside a theta weight has no destination;
  * vectors (bias, LayerNorm, translation) are in tile-position order, padded with zeros to whole tiles.
Rounding is restated on the CPU: np.float16 and torch.bfloat16 casts are round-to-nearest-even and the residuals are exact in float32, so
every comparison is bit for bit.

Every linear of every model gets, at distinct places of its weight: 0.0, -0.0, 2^-15 (a denormal high f16 piece), 65504 and 7e4 (the
saturation), 1 + 2^-8 (a tie of the high bf16 piece) and 1 + 2^-9 + 2^-17 (a tie of the middle one)."""
import ctypes as C
import os
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from permutect_amd.engine import lib as L
from tests.helpers import params_for

f32, f64 = np.float32, np.float64
CPU = torch.device("cpu")
MODELS = ("p0_b16", "t0_b8", "t0_two_sources", "p0_skip34", "p0_deep", "p0_batchnorm_eval", "wide_d98", "wide64_d98")
SHAPES = ("auto", "any")   # the instance the library picks (bias_cols = 1 for the exact-width ones) and PMT_SHAPE=any (bias_cols = 0)
SENTINEL = 0xC0FEBEEF      # a bit pattern no table holds: as a float -7.96, as two halves neither a planted value nor -1
GUARD = 64
TAIL_SLACK = 512           # engine/plan.py: packed_size = the last table's end + 512 (the kernels prefetch two fragments ahead)
PACK_KINDS = 7             # csrc/pmt_pack.hip: PMT_PACK_KINDS
KIND_NAMES = ("w_frag", "wt_frag", "b_pvec", "wb_frag", "wtb_frag", "emit_tab", "wh_frag")
VECTOR_JOBS = ("norm_w", "norm_b", "sgu_norm_w", "sgu_norm_b", "ref_reg", "translation")
PLANTED = np.asarray([0.0, -0.0, 2.0 ** -15, 65504.0, 7e4, 1 + 2.0 ** -8, 1 + 2.0 ** -9 + 2.0 ** -17], f32)
MUTANTS = ("swap_block_order", "unscaled_low", "split_first_half_only", "bias_twice")


def ceil16(n):
    return (n + 15) // 16 * 16


@dataclass
class Lowered:
    name: str
    shape: str
    desc: L.PmtModel
    lib: object
    bias_cols: int
    split0: int
    theta: np.ndarray
    phi: np.ndarray

    @property
    def id(self):
        return f"{self.name}-{self.shape}"

    def linears(self):
        return [self.desc.lin[i] for i in range(self.desc.n_linear)]


def source(buf_theta, buf_phi, src):
    """(the buffer a *_src names, the offset in it): theta at src >= 0, phi at -(src + 2)"""
    return (buf_theta, src) if src >= 0 else (buf_phi, -(src + 2))


def weight_of(low: Lowered, lin, theta=None, phi=None):
    buf, off = source(low.theta if theta is None else theta, low.phi if phi is None else phi, lin.w_src)
    return buf[off:off + lin.out_dim * lin.in_dim].reshape(lin.out_dim, lin.in_dim)


def bias_of(low: Lowered, lin, theta=None, phi=None):
    buf, off = source(low.theta if theta is None else theta, low.phi if phi is None else phi, lin.b_src)
    return buf[off:off + lin.out_dim]


def fill_buffers(low: Lowered, key=0):
    """random theta and phi (the kernel reads them as flat floats), the planted values in every linear's weight"""
    rng = np.random.default_rng([key, len(low.name), low.desc.theta_size])
    theta = (0.3 * rng.standard_normal(low.desc.theta_size)).astype(f32)
    phi = (0.3 * rng.standard_normal(low.desc.phi_size)).astype(f32)
    done = set()
    for lin in low.linears():
        if (lin.w_src, lin.out_dim * lin.in_dim) in done:
            continue
        done.add((lin.w_src, lin.out_dim * lin.in_dim))
        buf, off = source(theta, phi, lin.w_src)
        n = lin.out_dim * lin.in_dim
        where = off + rng.permutation(n)[:min(n, len(PLANTED))]
        buf[where] = PLANTED[:len(where)]
    return theta, phi


@lru_cache(maxsize=None)
def lowered(name: str, shape: str) -> Lowered:
    from permutect_amd.architecture.artifact_model import ArtifactModel
    from permutect_amd.engine.plan import EnginePlan, ParamSpace, _split0
    from permutect_amd.parameters import P0_DIMS, p0_params
    params = p0_params() if name == "p0_batchnorm_eval" else params_for(name)
    if name == "p0_batchnorm_eval":
        params.batch_normalize = True
    old = {k: os.environ.get(k) for k in ("PMT_SHAPE", "PMT_LIB", "PMT_JIT")}
    os.environ.pop("PMT_LIB", None)
    os.environ["PMT_JIT"] = "0"  # (a test never starts a build: every model of the table has its library among the built variants)
    if shape == "any":
        os.environ["PMT_SHAPE"] = "any"
    else:
        os.environ.pop("PMT_SHAPE", None)
    try:
        torch.manual_seed(11)
        model = ArtifactModel(params, device=CPU, **P0_DIMS)
        if name == "t0_two_sources":
            model.reset_source_predictor(2)
        model.eval()
        plan = EnginePlan(model, ParamSpace(model, CPU), CPU)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    desc = plan.desc
    sid = plan.lib.pmt_shape_id(C.byref(desc))
    h = desc.d_ffn // 2
    low = Lowered(name, shape, desc, plan.lib, int(sid in (L.SHAPE_EXACT, L.SHAPE_EXACT_BF16)), _split0(h), None, None)
    low.theta, low.phi = fill_buffers(low)
    assert 16 * ((L.limits_of(plan.lib)["max_half_ffn"] + 15) // 16) >= low.split0  # the build that runs the model has room for its halves
    return low


def build_split0(low: Lowered) -> int:
    """PMT_SPLIT0 of the build that runs the model (csrc/pmt_device.hpp: 16 tiles' worth of PMT_MAX_HALF_FFN)"""
    return 16 * ((L.limits_of(low.lib)["max_half_ffn"] + 15) // 16)


# =====================================================================================================================================
# the regions the plan hands to the kernel's jobs, from the descriptor alone
# =====================================================================================================================================
def geometry(low: Lowered, lin):
    out_v = low.split0 + lin.out_split if lin.out_split > 0 else lin.out_dim
    nmt, nkt = (out_v + 15) // 16, (lin.in_dim + 15) // 16
    return out_v, nmt, nkt


def regions(low: Lowered):
    """[(name, first word, words)]: every word of `packed` a job of the kernel writes"""
    d, out = low.desc, []
    for i, lin in enumerate(low.linears()):
        _, nmt, nkt = geometry(low, lin)
        out += [(f"lin{i}.w_frag", lin.w_frag, nmt * nkt * 256), (f"lin{i}.wt_frag", lin.wt_frag, nmt * nkt * 256)]
        if lin.b_pvec >= 0:
            out.append((f"lin{i}.b_pvec", lin.b_pvec, nmt * 16))
        out += [(f"lin{i}.wb_frag", lin.wb_frag, nmt * ((nkt + 1) // 2) * 768), (f"lin{i}.wtb_frag", lin.wtb_frag, nkt * ((nmt + 1) // 2) * 768),
                (f"lin{i}.wh_frag", lin.wh_frag, nmt * ((nkt + 1) // 2) * 512)]
        if lin.emit_tab >= 0:
            out.append((f"lin{i}.emit_tab", lin.emit_tab, nmt * nkt * 256 + nmt * 16))
    h = d.d_ffn // 2
    for b in range(d.num_blocks):
        blk = d.blocks[b]
        out += [(f"block{b}.norm_w", blk.norm_w_pvec, ceil16(d.d_model)), (f"block{b}.norm_b", blk.norm_b_pvec, ceil16(d.d_model)),
                (f"block{b}.sgu_norm_w", blk.sgu_norm_w_pvec, ceil16(h)), (f"block{b}.sgu_norm_b", blk.sgu_norm_b_pvec, ceil16(h)),
                (f"block{b}.ref_reg", blk.ref_reg_pvec, ceil16(h))]
    out.append(("translation", d.translation_pvec, ceil16(d.feature_dim)))
    return out


def owned_mask(low: Lowered):
    """bool [packed_size]: the words the plan hands to a job.  Asserts that no two regions overlap, that every one lies inside the buffer
    short of its tail slack, that each 16-bit table has its fragment of slack behind it and each region its padding to 256 floats."""
    size = low.desc.packed_size
    mask = np.zeros(size, bool)
    for name, start, n in regions(low):
        assert 0 <= start and start + n <= size - TAIL_SLACK and start % 4 == 0, (name, start, n, size)
        assert not mask[start:start + n].any(), f"{name} overlaps another region"
        mask[start:start + n] = True
    for i, lin in enumerate(low.linears()):
        _, nmt, nkt = geometry(low, lin)
        for start, n in ((lin.wb_frag, nmt * ((nkt + 1) // 2) * 768), (lin.wtb_frag, nkt * ((nmt + 1) // 2) * 768), (lin.wh_frag, nmt * ((nkt + 1) // 2) * 512)):
            assert not mask[start + n:start + n + 256].any(), f"lin{i}: no fragment of slack behind a 16-bit table"
        assert lin.w_frag % 256 == 0 and lin.wt_frag % 256 == 0, f"lin{i}: a region does not start on 256 floats"
    assert not mask[size - TAIL_SLACK:].any()
    return mask


# =====================================================================================================================================
# rounding, restated
# =====================================================================================================================================
def f16_pieces(w, scaled=True):
    """(hi, lo) bit patterns (uint16) of float32 values: the clamp to +-65504, f16(w), f16(2^12 (w - hi))"""
    w = np.clip(np.asarray(w, f32), f32(-65504), f32(65504))
    hi = w.astype(np.float16)
    resid = w - hi.astype(f32)  # exact in float32
    lo = (resid * f32(4096) if scaled else resid).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def bf16_pieces(w):
    """(hi, mid, lo) bit patterns (uint16) of float32 values: csrc/pmt_device.hpp: split_bf16x3"""
    t = torch.from_numpy(np.ascontiguousarray(w, f32))
    hi = t.to(torch.bfloat16)
    r1 = t - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return tuple(p.view(torch.int16).numpy().view(np.uint16) for p in (hi, mid, lo))


def as_halves(words, start, n_words):
    """the uint16 view of words [start, start + n_words) of a uint32 image"""
    return words[start:start + n_words].view(np.uint16)


# =====================================================================================================================================
# the decoder: natural (row, column) -> place
# =====================================================================================================================================
def position_of(f):
    """the position inside its tile of feature f % 16"""
    f = np.asarray(f) % 16
    return 4 * (f % 4) + f // 4


def virtual_row(o, h, split0):
    o = np.asarray(o)
    return o if h <= 0 else np.where(o < h, o, split0 + (o - h))


def frag_index(rows, ks, n_row_tiles):
    """fp32 A fragment: the word of element (row, k)"""
    r, k = rows[:, None], ks[None, :]
    return (((k // 16) * n_row_tiles + r // 16) * 64 + (k % 4) * 16 + position_of(r)) * 4 + (k % 16) // 4


def piece_index(rows, ks, n_row_tiles, n_k_blocks, pieces, row_tile_major):
    """16-bit pieces: the half-word of piece 0 of element (row, k); piece q lies 512 q further"""
    r, k = rows[:, None], ks[None, :]
    mt, kb = r // 16, k // 32
    blk = mt * n_k_blocks + kb if row_tile_major else kb * n_row_tiles + mt
    return blk * (pieces * 512) + ((k % 4) * 16 + position_of(r)) * 8 + 4 * ((k // 16) % 2) + (k % 16) // 4


def emit_index(vrows, cols, nkt):
    """emit table: the entry of dW element (virtual row, column)"""
    r, c = vrows[:, None], cols[None, :]
    return ((r // 16) * nkt + c // 16) * 256 + ((r % 4) * 16 + position_of(c)) * 4 + (r % 16) // 4


def vector_index(f):
    f = np.asarray(f)
    return 16 * (f // 16) + position_of(f)


def linear_places(low: Lowered, lin):
    """the index arrays of one linear, each [out_dim, in_dim] (or [out_dim]): where W[o, c] lies in each table"""
    _, nmt, nkt = geometry(low, lin)
    v, c = virtual_row(np.arange(lin.out_dim), lin.out_split, low.split0), np.arange(lin.in_dim)
    return dict(w=frag_index(v, c, nmt), wt=frag_index(c, v, nkt).T, wb=piece_index(v, c, nmt, (nkt + 1) // 2, 3, False),
                wtb=piece_index(c, v, nkt, (nmt + 1) // 2, 3, False).T, wh=piece_index(v, c, nmt, (nkt + 1) // 2, 2, True),
                emit=emit_index(v, c, nkt), emit_bias_col=emit_index(v, np.asarray([lin.in_dim]), nkt)[:, 0], vec=vector_index(v), v=v)


def decode(low: Lowered, theta=None, phi=None):
    """the whole `packed` image (uint32 [packed_size + GUARD]) the documented layout asks for: the sentinel everywhere, zeros (-1 in the
    emit tables) over every region a job owns, then every element of every natural matrix and vector at its place"""
    theta = low.theta if theta is None else theta
    phi = low.phi if phi is None else phi
    d = low.desc
    img = np.full(d.packed_size + GUARD, SENTINEL, np.uint32)
    fl = img.view(f32)
    for name, start, n in regions(low):
        img[start:start + n] = 0xFFFFFFFF if name.endswith("emit_tab") else 0
    for lin in low.linears():
        _, nmt, nkt = geometry(low, lin)
        w = weight_of(low, lin, theta, phi)
        at = linear_places(low, lin)
        fl[lin.w_frag + at["w"]] = w
        fl[lin.wt_frag + at["wt"]] = w
        if lin.b_pvec >= 0:
            fl[lin.b_pvec + at["vec"]] = bias_of(low, lin, theta, phi)
        for off, key, n_words in ((lin.wb_frag, "wb", nmt * ((nkt + 1) // 2) * 768), (lin.wtb_frag, "wtb", nkt * ((nmt + 1) // 2) * 768)):
            halves = as_halves(img, off, n_words)
            for q, piece in enumerate(bf16_pieces(w)):
                halves[at[key] + 512 * q] = piece
        halves = as_halves(img, lin.wh_frag, nmt * ((nkt + 1) // 2) * 512)
        for q, piece in enumerate(f16_pieces(w)):
            halves[at["wh"] + 512 * q] = piece
        if lin.emit_tab >= 0:
            tab = img[lin.emit_tab:lin.emit_tab + nmt * nkt * 256 + nmt * 16].view(np.int32)
            w_off = lin.w_src if lin.w_src >= 0 else -(lin.w_src + 2)
            tab[at["emit"]] = w_off + np.arange(lin.out_dim)[:, None] * lin.in_dim + np.arange(lin.in_dim)[None, :]
            in_column = low.bias_cols != 0 and lin.in_dim % 16 != 0
            if in_column:
                if lin.w_src >= 0 and lin.b_src >= 0:
                    tab[at["emit_bias_col"]] = lin.b_src + np.arange(lin.out_dim)
            elif lin.b_src >= 0:
                tab[nmt * nkt * 256 + at["vec"]] = lin.b_src + np.arange(lin.out_dim)
    h = d.d_ffn // 2
    vectors = [(d.translation_src, d.translation_pvec, d.feature_dim)]
    for b in range(d.num_blocks):
        blk = d.blocks[b]
        vectors += [(blk.norm_w_src, blk.norm_w_pvec, d.d_model), (blk.norm_b_src, blk.norm_b_pvec, d.d_model), (blk.sgu_norm_w_src, blk.sgu_norm_w_pvec, h),
                    (blk.sgu_norm_b_src, blk.sgu_norm_b_pvec, h), (blk.ref_reg_src, blk.ref_reg_pvec, h)]
    for src, dst, n in vectors:
        buf, off = source(theta, phi, src)
        fl[dst + vector_index(np.arange(n))] = buf[off:off + n]
    return img


# =====================================================================================================================================
# the mirror: fragment index -> (row, column), as the kernel walks
# =====================================================================================================================================
def split_row(v, h, split0, first_half_only=False):
    if h <= 0:
        return v
    second = np.where((v - split0) < h, h + (v - split0), -1)
    if first_half_only:
        second = np.full_like(v, -1)
    return np.where(v < split0, np.where(v < h, v, -1), second)


def _gather(w, orow, icol, ok):
    ok = ok & (orow >= 0) & (orow < w.shape[0]) & (icol < w.shape[1])
    return np.where(ok, w[np.where(ok, orow, 0), np.where(ok, icol, 0)], f32(0)).astype(f32)


def pack_mirror(low: Lowered, theta=None, phi=None, split0=None, mutant=None):
    """csrc/pmt_pack.hip: pmt_pack_kernel job by job in numpy, into a sentinel image.  `split0`: PMT_SPLIT0 of the build (default: the
    plan's).  Mutants: swap_block_order (k block and row tile of the 16-bit tables exchanged), unscaled_low (the low f16 piece without its
    2^12), split_first_half_only (split_row without the second half), bias_twice (the bias destination in the column AND the tail)."""
    assert mutant is None or mutant in MUTANTS
    theta = low.theta if theta is None else theta
    phi = low.phi if phi is None else phi
    s0 = low.split0 if split0 is None else split0
    d = low.desc
    img = np.full(d.packed_size + GUARD, SENTINEL, np.uint32)
    fl = img.view(f32)
    srow = lambda v, h: split_row(v, h, s0, mutant == "split_first_half_only")  # noqa: E731
    swap = mutant == "swap_block_order"
    for lin in low.linears():
        h = lin.out_split
        out_v = s0 + h if h > 0 else lin.out_dim
        w = weight_of(low, lin, theta, phi)
        for kind in (0, 1):
            Mv, Kv = (out_v, lin.in_dim) if kind == 0 else (lin.in_dim, out_v)
            nmt, nkt = (Mv + 15) >> 4, (Kv + 15) >> 4
            i = np.arange(nmt * nkt * 256)
            j, lane, tile = i & 3, (i >> 2) & 63, i >> 8
            mt, kt, m, g = tile % nmt, tile // nmt, lane & 15, lane >> 4
            mv, kv = 16 * mt + 4 * (m & 3) + (m >> 2), 16 * kt + 4 * j + g
            orow, icol = (srow(mv, h), kv) if kind == 0 else (srow(kv, h), mv)
            fl[(lin.w_frag if kind == 0 else lin.wt_frag) + i] = _gather(w, orow, icol, (mv < Mv) & (kv < Kv))
        if lin.b_pvec >= 0:
            b = bias_of(low, lin, theta, phi)
            i = np.arange(((out_v + 15) >> 4) * 16)
            v = 16 * (i >> 4) + 4 * (i & 3) + ((i >> 2) & 3)
            r = np.where(v < out_v, srow(v, h), -1)
            ok = (r >= 0) & (r < lin.out_dim)
            fl[lin.b_pvec + i] = np.where(ok, b[np.where(ok, r, 0)], f32(0))
        for kind in (3, 4, 6):
            Mv, Kv = (lin.in_dim, out_v) if kind == 4 else (out_v, lin.in_dim)
            nmt, nkt = (Mv + 15) >> 4, (Kv + 15) >> 4
            nkb = (nkt + 1) >> 1
            i = np.arange(nkb * nmt * 512)
            e, lane, blk = i & 7, (i >> 3) & 63, i >> 9
            row_tile_major = (kind == 6) != swap
            mt, kb = (blk // nkb, blk % nkb) if row_tile_major else (blk % nmt, blk // nmt)
            m, kg = lane & 15, lane >> 4
            mv, kv = 16 * mt + 4 * (m & 3) + (m >> 2), 16 * (2 * kb + (e >> 2)) + 4 * (e & 3) + kg
            orow, icol = (srow(kv, h), mv) if kind == 4 else (srow(mv, h), kv)
            val = _gather(w, orow, icol, (mv < Mv) & (kv < Kv) & ((2 * kb + (e >> 2)) < nkt))
            if kind == 6:
                pieces, start = f16_pieces(val, scaled=mutant != "unscaled_low"), lin.wh_frag
            else:
                pieces, start = bf16_pieces(val), (lin.wb_frag if kind == 3 else lin.wtb_frag)
            halves = as_halves(img, start, nkb * nmt * 256 * len(pieces))
            for q, piece in enumerate(pieces):
                halves[blk * len(pieces) * 512 + lane * 8 + e + 512 * q] = piece
        if lin.emit_tab >= 0:
            nmt, nkt = (out_v + 15) >> 4, (lin.in_dim + 15) >> 4
            tab = img[lin.emit_tab:lin.emit_tab + nmt * nkt * 256 + nmt * 16].view(np.int32)
            w_off = lin.w_src if lin.w_src >= 0 else -(lin.w_src + 2)
            bias_col = low.bias_cols != 0 and (lin.in_dim & 15) != 0
            bias_same = lin.w_src >= 0 and lin.b_src >= 0
            i = np.arange(nmt * nkt * 256)
            j, lane, blk = i & 3, (i >> 2) & 63, i >> 8
            ot = blk // nkt
            it = blk - ot * nkt
            pf = 16 * ot + 4 * j + (lane >> 4)
            o = np.where(pf < out_v, srow(pf, h), -1)
            cp = lane & 15
            col = 16 * it + 4 * (cp & 3) + (cp >> 2)
            row_ok = (o >= 0) & (o < lin.out_dim)
            tab[i] = np.where(row_ok & (col < lin.in_dim), w_off + o * lin.in_dim + col,
                              np.where(bias_col & bias_same & row_ok & (col == lin.in_dim), lin.b_src + o, -1))
            i = np.arange(nmt * 16)
            p = i & 15
            pf = 16 * (i >> 4) + 4 * (p & 3) + (p >> 2)
            o = np.where(pf < out_v, srow(pf, h), -1)
            in_tail = (not bias_col) or mutant == "bias_twice"
            tab[nmt * nkt * 256 + i] = np.where(in_tail & (lin.b_src >= 0) & (o >= 0) & (o < lin.out_dim), lin.b_src + o, -1)
    hh = d.d_ffn // 2
    jobs = []
    for b in range(d.num_blocks):
        blk = d.blocks[b]
        jobs += [(blk.norm_w_src, blk.norm_w_pvec, d.d_model), (blk.norm_b_src, blk.norm_b_pvec, d.d_model), (blk.sgu_norm_w_src, blk.sgu_norm_w_pvec, hh),
                 (blk.sgu_norm_b_src, blk.sgu_norm_b_pvec, hh), (blk.ref_reg_src, blk.ref_reg_pvec, hh)]
    jobs.append((d.translation_src, d.translation_pvec, d.feature_dim))
    for src, dst, n in jobs:
        buf, off = source(theta, phi, src)
        i = np.arange(ceil16(n))
        f = 16 * (i >> 4) + 4 * (i & 3) + ((i >> 2) & 3)
        fl[dst + i] = np.where(f < n, buf[off + np.where(f < n, f, 0)], f32(0))
    return img


# =====================================================================================================================================
# the assertions both tests make on a `packed` image
# =====================================================================================================================================
def first_difference(low: Lowered, got, want):
    """None, or (region name, word in it, got, want) of the first word that differs"""
    bad = np.flatnonzero(np.asarray(got, np.uint32) != np.asarray(want, np.uint32))
    if not len(bad):
        return None
    w = int(bad[0])
    for name, start, n in regions(low):
        if start <= w < start + n:
            return name, w - start, hex(int(got[w])), hex(int(want[w])), len(bad)
    return "outside every region", w, hex(int(got[w])), hex(int(want[w])), len(bad)


def check_image(low: Lowered, img, theta=None, phi=None):
    """items 1 to 5 of the issue on a uint32 image of packed_size + GUARD words.  Returns the word counts of the case."""
    theta = low.theta if theta is None else theta
    phi = low.phi if phi is None else phi
    img = np.asarray(img, np.uint32)
    want = decode(low, theta, phi)
    mask = np.concatenate([owned_mask(low), np.zeros(GUARD, bool)])
    # 3. every word no job owns still holds the sentinel: the padding of the regions, the slack behind the 16-bit tables, the tail, the guards
    assert (img[~mask] == SENTINEL).all(), ("a word outside every region was written", first_difference(low, np.where(mask, want, img), want))
    # 1. and 2. every word of every region is the decoder's, bit for bit (the padding 0.0 / -1 with it)
    assert first_difference(low, img, want) is None, first_difference(low, img, want)
    fl = img.view(f32)
    counts = dict(words=int(mask.sum()), sentinel_words=int((~mask).sum()), linears=low.desc.n_linear, emit_tables=0, no_bias_destination=[])
    rng = np.random.default_rng(5)
    for n, lin in enumerate(low.linears()):
        _, nmt, nkt = geometry(low, lin)
        at = linear_places(low, lin)
        w = weight_of(low, lin, theta, phi)
        # 2. the padding: every value word no natural element lands on is exactly +0.0
        pad = np.ones(nmt * nkt * 256, bool)
        pad[at["w"].ravel()] = False
        assert not img[lin.w_frag:lin.w_frag + nmt * nkt * 256][pad].any() and pad.sum() == nmt * nkt * 256 - w.size
        # 5. read back and multiply: un-permuted, each table gives W x in float64 (exactly: the pieces sum to the float32 value)
        x = rng.standard_normal((lin.in_dim, 3))
        ref = w.astype(f64) @ x
        bound = 2.0 ** -22 * (np.abs(w.astype(f64)) @ np.abs(x))
        # (the gathers made contiguous: the same matrix product in the same order is the same bits)
        back = [np.ascontiguousarray(fl[lin.w_frag + at["w"]], f64), np.ascontiguousarray(fl[lin.wt_frag + at["wt"]], f64)]
        assert np.array_equal(back[0] @ x, ref) and np.array_equal(back[1] @ x, ref), f"lin{n}: w_frag / wt_frag un-permuted is not W"
        halves = as_halves(img, lin.wb_frag, nmt * ((nkt + 1) // 2) * 768)
        pieces = [torch.from_numpy(halves[at["wb"] + 512 * q].astype(np.int16)).view(torch.bfloat16).double().numpy() for q in range(3)]
        assert np.array_equal(np.ascontiguousarray(pieces[0] + pieces[1] + pieces[2]) @ x, ref), f"lin{n}: hi + mid + lo of the bf16 pieces is not W"
        halves = as_halves(img, lin.wh_frag, nmt * ((nkt + 1) // 2) * 512)
        hi, lo = (halves[at["wh"] + 512 * q].view(np.float16).astype(f64) for q in range(2))
        clamped = np.clip(w.astype(f64), -65504.0, 65504.0)
        assert (np.abs((hi + lo / 4096.0) @ x - clamped @ x) <= 2.0 ** -22 * (np.abs(clamped) @ np.abs(x))).all(), f"lin{n}: hi + lo / 4096 of the f16 pieces is not W"
        assert (np.abs((hi + lo / 4096.0) @ x - ref) <= bound).all() or (np.abs(w) > 65504).any()
        # 4. the emit table: every destination once
        if lin.emit_tab < 0:
            continue
        counts["emit_tables"] += 1
        tab = img[lin.emit_tab:lin.emit_tab + nmt * nkt * 256 + nmt * 16].view(np.int32)
        block, tail = tab[:nmt * nkt * 256], tab[nmt * nkt * 256:]
        dest = np.sort(np.concatenate([block[block >= 0], tail[tail >= 0]]))
        w_off = lin.w_src if lin.w_src >= 0 else -(lin.w_src + 2)
        w_set = w_off + np.arange(w.size)
        in_column = low.bias_cols != 0 and lin.in_dim % 16 != 0
        if lin.w_src >= 0 and lin.b_src >= 0:
            assert np.array_equal(dest, np.sort(np.concatenate([w_set, lin.b_src + np.arange(lin.out_dim)]))), f"lin{n}: the destinations are not W and b, each once"
            if in_column:
                assert (tail == -1).all() and np.array_equal(np.sort(block[at["emit_bias_col"]]), lin.b_src + np.arange(lin.out_dim))
            else:
                assert np.array_equal(np.sort(tail[tail >= 0]), lin.b_src + np.arange(lin.out_dim)) and np.array_equal(np.sort(block[block >= 0]), w_set)
        else:  # the weight in phi (the rotation, a folded BatchNorm): the table indexes phi, and a bias not in theta beside a theta weight has no destination
            assert np.array_equal(dest, w_set) and (tail == -1).all() and lin.w_src < 0 and lin.b_src < 0, f"lin{n}"
            counts["no_bias_destination"].append(n)
    return counts


def branches_of(low: Lowered):
    """which branches of the kernel a lowered model reaches: the coverage row of the CPU test"""
    d, got = low.desc, set()
    for lin in low.linears():
        _, nmt, nkt = geometry(low, lin)
        got |= {"kind0", "kind1", "kind3", "kind4", "kind6"}
        got.add("kind2" if lin.b_pvec >= 0 else "no_bias")
        got.add("kind5" if lin.emit_tab >= 0 else "no_emit_table")
        got.add("out_split" if lin.out_split > 0 else "plain_rows")
        got.add("w_in_phi" if lin.w_src < 0 else "w_in_theta")
        if lin.b_src < -1:
            got.add("b_in_phi")
        if nkt % 2:
            got.add("absent_k_tile")
        if lin.in_dim % 16:
            got.add("padding_columns")
        if lin.out_dim % 16 or lin.out_split % 16:
            got.add("padding_rows")
        if lin.emit_tab >= 0 and lin.in_dim % 16:
            got.add("bias_in_column" if low.bias_cols else "bias_in_tail_beside_padding")
        if lin.emit_tab >= 0 and lin.in_dim % 16 == 0 and lin.b_src >= 0:
            got.add("bias_in_tail_full_tiles")
    got |= {"vector_" + v for v in (VECTOR_JOBS if d.num_blocks else VECTOR_JOBS[-1:])}
    if low.split0 == 32:
        got.add("split0_32")
    if d.row_mlp[L.ROWS_SOURCE].n_ops > 0:
        got.add("third_row_mlp")
    return got


ALL_BRANCHES = ({f"kind{k}" for k in range(PACK_KINDS)} | {"vector_" + v for v in VECTOR_JOBS}
                | {"no_bias", "no_emit_table", "out_split", "plain_rows", "w_in_phi", "w_in_theta", "b_in_phi", "absent_k_tile", "padding_columns",
                   "padding_rows", "bias_in_column", "bias_in_tail_beside_padding", "bias_in_tail_full_tiles", "split0_32", "third_row_mlp"})
