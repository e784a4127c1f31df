"""The filtered VCF of `filter_variants` (reference tools/filter_variants.py:369-617 `apply_filtering_to_vcf`): every record of the input
VCF finds its candidate, gets its FILTER text and -- when it has a candidate -- five INFO fields, and the file is written with every
other byte as it stood.

The reference builds a Datum and a PosteriorResult per candidate, keeps a dict keyed by the string `contig:pos:alt` and, per cyvcf2
record, does a lookup, 21 `"{:.3f}".format` calls, one `torch.topk` and a Python set of filter names.  Here the record table of
data/vcf_text.py and the text go to the device and four library calls do the work (csrc/pmt_vcf.hip; the rule is stated in
include/permutect_amd.h: PmtVcfArgs): pmt_site_keys, a sort, pmt_vcf_match, pmt_vcf_plan, a cumsum, pmt_vcf_write slab by slab.
Integer arithmetic only, so the bytes do not depend on the grid, the slab size or the run.  The numpy mirror in this module (the CPU
path, and PMT_FILTERED_VCF=torch on a device) leaves the same bytes.

Two deliberate differences from the reference: the decision is the `filtered_b` that is passed in (float32 error probability against
the threshold of the CANDIDATE's variant type; the reference recomputes 1 - p in double and takes the type from the record's own
alleles -- records whose own type differs are counted as `type_mismatch`), and untouched fields are the input's bytes (the reference
rewrites every record through htslib).  Output is plain text, or gzip when the path ends in `.gz`; no bgzip, no index."""
from __future__ import annotations

import ctypes as C
import gzip
import os
import re
from typing import Dict, List

import numpy as np
import torch

from permutect_amd.data import site_annotation as S
from permutect_amd.data import vcf_text as V
from permutect_amd.data.datum import Data
from permutect_amd.enums import Call

CALL_NAMES = [call.name.lower() for call in Call]               # reference tools/filter_variants.py: FILTER_NAMES
FILTER_ORDER = ["contamination", "slippage"] + CALL_NAMES       # the ONE order a record's filters are written in; bit k of the mask
INFO_KEYS = ("POST", "PRIOR", "SPECLL", "ARTLOD", "NORMLL")     # in the order the reference sets them on a record
NUM_VALUES = 21
LITERALS = [b";POST="] + [b","] * 4 + [b";PRIOR="] + [b","] * 4 + [b";SPECLL="] + [b","] * 4 + [b";ARTLOD=", b";NORMLL="] + [b","] * 4
COUNT_NAMES = ("matched", "unmatched", "zero_alt_depth", "passed") + tuple("filtered_" + name for name in CALL_NAMES) + (
    "trusted_kept", "type_mismatch", "unformattable")
NUMBER_WIDTH = 21                                               # a sign, 19 digits (q < 1000 * 2^53 < 10^19) and a point
DEFAULT_SLAB_BYTES = 256 << 20
_FILTER_TEXT = [b";".join(name.encode() for k, name in enumerate(FILTER_ORDER) if mask >> k & 1) or b"PASS" for mask in range(128)]
_FILTER_LENGTH = np.array([len(t) for t in _FILTER_TEXT], np.int64)


def on_device(device) -> bool:
    """the library calls (True) or the numpy mirror"""
    return torch.device(device).type == "cuda" and os.environ.get("PMT_FILTERED_VCF", "") != "torch"


# ---- the header ----------------------------------------------------------------------------------------------------------------------------
def header_additions(passing_call: int) -> List[tuple]:
    """(kind, dict) in the reference's order (tools/filter_variants.py:463-508)"""
    all_types = ", ".join(call.name for call in Call)
    out = [("FORMAT", {"ID": "DP", "Number": "1", "Type": "Integer", "Description": "depth"})]
    for key, description in (("POST", "Mutect3 posterior probability of {" + all_types + "}"), ("PRIOR", "Log priors of {" + all_types + "}"),
                             ("SPECLL", "Log spectra likelihoods of {" + all_types + "}"),
                             ("NORMLL", "Log normal likelihoods of {" + all_types + "}"), ("ARTLOD", "Mutect3 artifact log odds")):
        out.append(("INFO", {"ID": key, "Number": "A", "Type": "Float", "Description": description}))
    out += [("FILTER", {"ID": name, "Description": name}) for n, name in enumerate(CALL_NAMES) if n != int(passing_call)]
    return out


def amended_header(header: List[bytes], passing_call: int) -> List[bytes]:
    """the header with the new lines in front of the #CHROM line, each only when the header has no line of that kind and ID.  A header
    that already declares one of the five INFO IDs is a ValueError: the file was annotated before."""
    have = set()
    for line in header:
        found = re.match(rb"##(INFO|FORMAT|FILTER)=<ID=([^,>]+)", line)
        if found:
            have.add((found.group(1).decode(), found.group(2).decode("latin-1")))
    again = [key for key in INFO_KEYS if ("INFO", key) in have]
    if again:
        raise ValueError(f"the VCF's header already declares INFO {', '.join(again)}: it was filtered before")
    chrom = max((i for i, line in enumerate(header) if line.startswith(b"#CHROM")), default=len(header))
    end = b"\r\n" if chrom < len(header) and header[chrom].endswith(b"\r\n") else b"\n"
    new = []
    for kind, entry in header_additions(passing_call):
        if (kind, entry["ID"]) in have:
            continue
        fields = ",".join(f"{k}={entry[k]}" for k in ("ID", "Number", "Type") if k in entry) + f",Description=\"{entry['Description']}\""
        new.append(f"##{kind}=<{fields}>".encode() + end)
    before = list(header[:chrom])
    if before and not before[-1].endswith(b"\n"):
        before[-1] = before[-1] + end
    return before + new + list(header[chrom:])


# ---- "{:.3f}" in integers ------------------------------------------------------------------------------------------------------------------
def format_float32(values):
    """`"{:.3f}".format(float(x))` of every float32 of `values` (include/permutect_amd.h: A NUMBER): chars uint8 [n, 21], each text
    right-aligned; lengths int64 [n]; unformattable bool [n] (finite, |x| >= 2^53: length 0).  Vectorised integer numpy."""
    u = np.uint64
    bits = np.ascontiguousarray(values, np.float32).view(np.uint32).ravel().astype(u)
    negative = (bits >> u(31)) != 0
    exponent = ((bits >> u(23)) & u(255)).astype(np.int64)
    fraction = bits & u(0x7FFFFF)
    special = exponent == 255
    unformattable = (exponent >= 127 + 53) & ~special
    m = np.where(exponent != 0, fraction | u(0x800000), fraction) * u(1000)
    e = np.where(exponent != 0, exponent - 150, -149)
    q_up = m << np.clip(e, 0, 29).astype(u)
    s = np.clip(-e, 1, 63).astype(u)
    q_down = m >> s
    remainder, half = m & ((u(1) << s) - u(1)), u(1) << (s - u(1))
    q_down = q_down + ((remainder > half) | ((remainder == half) & ((q_down & u(1)) == 1))).astype(u)
    q = np.where(e >= 0, q_up, np.where(e > -64, q_down, u(0)))
    q = np.where(special | unformattable, u(0), q)
    n = len(q)
    chars = np.full((n, NUMBER_WIDTH), ord(" "), np.uint8)
    digits = np.full(n, 4, np.int64)
    rest = q.copy()
    for k in range(19):
        column = NUMBER_WIDTH - 1 - (k if k < 3 else k + 1)
        if k >= 4:
            digits += rest != 0
        live = (k < 4) | (rest != 0)
        chars[:, column] = np.where(live, (rest % u(10)).astype(np.uint8) + ord("0"), chars[:, column])
        rest //= u(10)
    chars[:, NUMBER_WIDTH - 4] = ord(".")
    rows = np.arange(n)
    sign_column = NUMBER_WIDTH - 2 - digits
    chars[rows, sign_column] = np.where(negative, ord("-"), chars[rows, sign_column])
    lengths = negative + digits + 1
    is_nan, is_inf = special & (fraction != 0), special & (fraction == 0)
    for text, which in ((b" nan", is_nan), (b" inf", is_inf & ~negative), (b"-inf", is_inf & negative)):
        chars[which, NUMBER_WIDTH - 4:] = np.frombuffer(text, np.uint8)
    lengths = np.where(is_nan | (is_inf & ~negative), 3, np.where(is_inf, 4, lengths))
    lengths = np.where(unformattable, 0, lengths).astype(np.int64)
    return chars, lengths, unformattable


def format_strings(values) -> List[str]:
    chars, lengths, _ = format_float32(values)
    return [chars[i, NUMBER_WIDTH - int(n):].tobytes().decode() for i, n in enumerate(lengths)]


def appended_text(values_r21: np.ndarray):
    """[r, 21] float32 -> the bytes of every row's `;POST=...;NORMLL=...` concatenated, the rows' starts int64 [r + 1], unformattable
    values per row"""
    r = len(values_r21)
    chars, lengths, unformattable = format_float32(values_r21)
    literal_length = np.tile(np.array([len(t) for t in LITERALS], np.int64), r)
    widths = literal_length + lengths
    ends = np.cumsum(widths)
    begins = ends - widths
    out = np.zeros(int(ends[-1]) if r else 0, np.uint8)
    literal_bytes = np.zeros((NUM_VALUES, 8), np.uint8)
    for j, text in enumerate(LITERALS):
        literal_bytes[j, :len(text)] = np.frombuffer(text, np.uint8)
    which = np.tile(np.arange(NUM_VALUES), r)
    for t in range(8):
        sel = np.flatnonzero(literal_length > t)
        out[begins[sel] + t] = literal_bytes[which[sel], t]
    for k in range(NUMBER_WIDTH):
        sel = np.flatnonzero(lengths > k)
        out[ends[sel] - 1 - k] = chars[sel, NUMBER_WIDTH - 1 - k]
    row_start = np.concatenate([[0], ends.reshape(r, NUM_VALUES)[:, -1]]).astype(np.int64) if r else np.zeros(1, np.int64)
    return out, row_start, unformattable.reshape(r, NUM_VALUES).sum(axis=1)


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------------
def candidate_arrays(posterior_int_rows, outputs: Dict[str, np.ndarray]):
    """values float32 [n, 21] in the order they are written (POST, PRIOR, SPECLL, ARTLOD, NORMLL), filtered uint8 [n], variant types
    uint8 [n].  `outputs`: the arrays of --calls_output and `artifact_logits_b`."""
    def f32(name, shape):
        array = np.ascontiguousarray(np.asarray(outputs[name]), np.float32)
        if array.shape != shape:
            raise ValueError(f"filtered VCF: {name} of shape {array.shape}, expected {shape}")
        return array

    rows = np.asarray(posterior_int_rows)
    n = len(rows)
    values = np.concatenate([f32("posterior_probabilities_bc", (n, 5)), f32("log_priors_bc", (n, 5)), f32("spectra_log_lks_bc", (n, 5)),
                             f32("artifact_logits_b", (n,))[:, None], f32("normal_log_lks_bc", (n, 5))], axis=1)
    filtered = np.ascontiguousarray(np.asarray(outputs["filtered_b"]).astype(np.uint8))
    if filtered.shape != (n,):
        raise ValueError(f"filtered VCF: filtered_b of shape {filtered.shape}, expected {(n,)}")
    variant_types = np.ascontiguousarray(rows[:, Data.VARIANT_TYPE.idx].astype(np.uint8)) if n else np.zeros(0, np.uint8)
    return np.ascontiguousarray(values), filtered, variant_types


def first_error_call(probabilities_r5: np.ndarray, passing_call: int) -> np.ndarray:
    """the call with the largest float32 probability among the four that are not the passing one, the lowest index among equal maxima
    (architecture/posterior_evaluation.py: first_argmax)"""
    best_call = np.full(len(probabilities_r5), -1, np.int64)
    best = np.zeros(len(probabilities_r5), np.float32)
    for c in range(len(Call)):
        if c == int(passing_call):
            continue
        better = (best_call < 0) | (probabilities_r5[:, c] > best)
        best_call, best = np.where(better, c, best_call), np.where(better, probabilities_r5[:, c], best)
    return best_call


class Plan:
    """what the match and the plan leave per record: the candidate's row or -1, the filter mask, the error call or -1, the output
    line's length and start; the counters"""

    def __init__(self, matched, mask, error_call, out_length, counts):
        self.matched, self.mask, self.error_call, self.out_length = matched, mask, error_call, out_length
        self.out_start = np.concatenate([[0], np.cumsum(out_length)]).astype(np.int64)
        self.counts = np.asarray(counts, np.int64)

    def counts_dict(self) -> Dict[str, int]:
        return dict(zip(COUNT_NAMES, (int(c) for c in self.counts)))


def _check_formattable(plan: Plan, values: np.ndarray):
    if plan.counts[COUNT_NAMES.index("unformattable")]:
        rows = np.unique(plan.matched[plan.matched >= 0])
        bits = values[rows].view(np.uint32)
        exponent = (bits >> 23) & 255
        bad = rows[((exponent >= 127 + 53) & (exponent != 255)).any(axis=1)]
        raise ValueError(f"filtered VCF: {int(plan.counts[-1])} values of magnitude 2^53 or more cannot be written; the first in candidate row "
                         f"{int(bad[0])}: the posterior stage's numbers are broken")


# ---- the numpy mirror ----------------------------------------------------------------------------------------------------------------------
def match_mirror(records: V.VcfRecords, posterior_int_rows) -> np.ndarray:
    """int32 [records]: the LAST candidate in dataset order with the record's key, or -1"""
    rows = np.asarray(posterior_int_rows)
    matched = np.full(len(records), -1, np.int32)
    if len(rows) == 0 or len(records) == 0:
        return matched
    first_column = S._identity_layout(rows)
    locus, _, _, ref_code, alt_code = S.decode_identity(rows[:, first_column: first_column + 7])
    key = S.candidate_allele_keys(ref_code, alt_code)
    order = np.lexsort((key, locus))  # stable: candidates of one key stay in dataset order
    distinct, rank_of_candidate = np.unique(locus, return_inverse=True)
    table = ((rank_of_candidate.astype(np.uint64) << np.uint64(32)) | key.astype(np.uint64))[order]
    rank = np.minimum(np.searchsorted(distinct, records.locus), len(distinct) - 1)
    wanted = (rank.astype(np.uint64) << np.uint64(32)) | records.allele_key.astype(np.uint64)
    after = np.searchsorted(table, wanted, side="right")
    at = np.maximum(after - 1, 0)
    has_key = ((records.flags & V.HAS_KEY) != 0) & ((records.flags & V.VERBATIM) == 0)
    found = has_key & (after > 0) & (distinct[rank] == records.locus) & (table[at] == wanted)
    matched[found] = order[at[found]].astype(np.int32)
    return matched


def plan_mirror(records: V.VcfRecords, matched, flags, values, filtered, variant_types, passing_call: int) -> Plan:
    """pmt_vcf_plan by vectorised numpy; `flags`: the records' with ZERO_ALT_DEPTH set where it holds"""
    n = len(records)
    verbatim = (flags & V.VERBATIM) != 0
    is_matched = (matched >= 0) & ~verbatim
    row = np.maximum(matched, 0).astype(np.int64)
    mask = (flags & (V.CONTAMINATION | V.SLIPPAGE)).astype(np.int64)
    error_call = np.full(n, -1, np.int64)
    append_length = np.zeros(n, np.int64)
    unformattable = np.zeros(n, np.int64)
    type_mismatch = np.zeros(n, bool)
    if is_matched.any():
        rows = row[is_matched]
        _, lengths, bad = format_float32(values[rows])
        append_length[is_matched] = lengths.reshape(-1, NUM_VALUES).sum(axis=1) + sum(len(t) for t in LITERALS)
        unformattable[is_matched] = bad.reshape(-1, NUM_VALUES).sum(axis=1)
        calls = np.where(filtered[rows] != 0, first_error_call(values[rows, :5], passing_call), -1)
        error_call[is_matched] = calls
        type_mismatch[is_matched] = records.variation[is_matched] != variant_types[rows]
    mask = np.where(error_call >= 0, mask | (4 << np.maximum(error_call, 0)), mask)
    zero = ~is_matched & ~verbatim & ((flags & V.ZERO_ALT_DEPTH) != 0)
    mask = np.where(zero, mask | (4 << int(Call.SEQ_ERROR)), mask)
    mask = np.where(verbatim, 0, mask)
    line_length = np.diff(records.line_start)
    dot = (flags & V.INFO_DOT) != 0
    out_length = np.where(verbatim, line_length, line_length - (records.filter_end - records.filter_begin) + _FILTER_LENGTH[mask]
                          + np.where(is_matched, append_length - 2 * dot, 0))
    data = ~verbatim
    counts = [is_matched.sum(), (data & ~is_matched).sum(), zero.sum(), (data & (mask == 0)).sum()]
    counts += [(data & ((mask >> (2 + c)) & 1 != 0)).sum() for c in range(len(Call))]
    counts += [(data & ((mask & 3) != 0)).sum(), type_mismatch.sum(), unformattable.sum()]
    return Plan(matched, mask.astype(np.uint8), error_call.astype(np.int8), out_length.astype(np.int64), counts)


def write_mirror(records: V.VcfRecords, plan: Plan, flags, values) -> bytes:
    """pmt_vcf_write on the host: the appended texts by vectorised numpy, one Python loop for the final splice"""
    is_matched = (plan.matched >= 0) & ((flags & V.VERBATIM) == 0)
    appended, row_start, _ = appended_text(values[plan.matched[is_matched].astype(np.int64)])
    appended = appended.tobytes()
    text = records.text.tobytes()
    pieces = []
    m = 0
    starts, fb, fe, ie = records.line_start.tolist(), records.filter_begin.tolist(), records.filter_end.tolist(), records.info_end.tolist()
    for i in range(len(records)):
        a, b = starts[i], starts[i + 1]
        if flags[i] & V.VERBATIM:
            pieces.append(text[a:b])
            continue
        pieces.append(text[a: a + fb[i]])
        pieces.append(_FILTER_TEXT[plan.mask[i]])
        if is_matched[i]:
            dot = bool(flags[i] & V.INFO_DOT)
            pieces.append(text[a + fe[i]: a + (fe[i] + 1 if dot else ie[i])])
            pieces.append(appended[int(row_start[m]) + (1 if dot else 0): int(row_start[m + 1])])
            m += 1
        else:
            pieces.append(text[a + fe[i]: a + ie[i]])
        pieces.append(text[a + ie[i]: b])
    out = b"".join(pieces)
    assert len(out) == int(plan.out_start[-1]), (len(out), int(plan.out_start[-1]))
    return out


def flags_with_alt_depth(records: V.VcfRecords, matched: np.ndarray) -> np.ndarray:
    """the records' flags with ZERO_ALT_DEPTH set on the unmatched records whose tumor sample has no alt depth: looked up lazily, on
    the host, for those records only"""
    flags = records.flags.copy()
    unmatched = np.flatnonzero((matched < 0) & ((flags & V.VERBATIM) == 0))
    if len(unmatched):
        flags[unmatched[records.zero_alt_depth(unmatched)]] |= V.ZERO_ALT_DEPTH
    return flags


# ---- the device stage ------------------------------------------------------------------------------------------------------------------------
class DeviceVcf:
    """The record table and the candidates' arrays on the device with the outputs of the four library calls.  `match()`, `plan()`,
    `write(first, stop)`: one library call each (match: pmt_site_keys, two stable torch sorts, pmt_vcf_match)."""

    def __init__(self, records: V.VcfRecords, posterior_int_rows, values, filtered, variant_types, passing_call: int, device, threads: int = 0):
        from permutect_amd.engine import lib as L
        self.L, self.records, self.device, self.threads = L, records, torch.device(device), int(threads)
        self.table = records.to(device)
        n, c = len(records), len(values)
        rows = torch.as_tensor(np.ascontiguousarray(posterior_int_rows) if isinstance(posterior_int_rows, np.ndarray) else posterior_int_rows).to(device)
        assert rows.dim() == 2, rows.shape
        if rows.numel() and rows.stride(1) != 1:
            rows = rows.contiguous()
        assert rows.element_size() in (2, 4, 8) and not rows.is_floating_point(), rows.dtype
        self.rows, self.first_column = rows, (S._identity_layout(rows) if c else 0)
        self.values = torch.from_numpy(values).to(device)
        self.filtered, self.variant_types = torch.from_numpy(filtered).to(device), torch.from_numpy(variant_types).to(device)
        self.flags = self.table[6].clone()
        self.matched = torch.empty(n, dtype=torch.int32, device=device)
        self.mask = torch.empty(n, dtype=torch.uint8, device=device)
        self.error_call = torch.empty(n, dtype=torch.int8, device=device)
        self.out_length = torch.empty(n, dtype=torch.int64, device=device)
        self.counters = torch.zeros(L.VCF_COUNTERS, dtype=torch.int64, device=device)
        self.out_start = None
        self.sorted = None
        a = self.args = L.PmtVcfArgs()
        a.num_records, a.num_candidates, a.threads_hint, a.passing_call = n, c, self.threads, int(passing_call)
        a.line_start, a.filter_begin, a.filter_end, a.info_end, a.rec_locus, a.rec_key = (t.data_ptr() for t in self.table[:6])
        a.rec_flags, a.rec_variation = self.flags.data_ptr(), self.table[7].data_ptr()
        a.values, a.filtered, a.variant_types = self.values.data_ptr(), self.filtered.data_ptr(), self.variant_types.data_ptr()
        a.matched, a.mask, a.error_call = self.matched.data_ptr(), self.mask.data_ptr(), self.error_call.data_ptr()
        a.out_length, a.counters = self.out_length.data_ptr(), self.counters.data_ptr()

    def _call(self, name):
        self.L.check(getattr(self.L.load(), name)(C.byref(self.args), self.L.raw_stream(self.device)), name)

    def match(self):
        L, c = self.L, len(self.values)
        locus = torch.empty(c, dtype=torch.int64, device=self.device)
        key = torch.empty(c, dtype=torch.int32, device=self.device)
        k = L.PmtSiteKeysArgs()
        k.num_candidates, k.int_rows, k.int_row_stride = c, self.rows.data_ptr(), self.rows.stride(0) if c else 7
        k.int_elem_bytes, k.first_column, k.threads_hint = self.rows.element_size(), self.first_column, self.threads
        k.locus, k.allele_key = locus.data_ptr(), key.data_ptr()
        L.check(L.load().pmt_site_keys(C.byref(k), L.raw_stream(self.device)), "pmt_site_keys")
        # ascending by (locus as unsigned, key, row): two stable sorts; flipping the top bit makes the signed order the unsigned one
        by_key = torch.sort(key, stable=True).indices
        by_locus = torch.sort((locus ^ torch.iinfo(torch.int64).min)[by_key], stable=True).indices
        order = by_key[by_locus]
        self.sorted = (locus[order].contiguous(), key[order].contiguous(), order.contiguous())
        self.args.cand_locus, self.args.cand_key, self.args.cand_row = (t.data_ptr() for t in self.sorted)
        self._call("pmt_vcf_match")
        return self.matched

    def set_zero_alt_depth(self, flags: np.ndarray):
        self.flags.copy_(torch.from_numpy(np.ascontiguousarray(flags)).to(self.device))

    def plan(self):
        self.counters.zero_()
        self._call("pmt_vcf_plan")
        self.out_start = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), torch.cumsum(self.out_length, 0)])
        self.args.out_start = self.out_start.data_ptr()
        return self.out_length

    def write(self, first: int, stop: int, text: torch.Tensor, text_base: int, out: torch.Tensor, out_base: int):
        """records [first, stop): `text` holds the input's bytes from `text_base` on, `out` takes the output's from `out_base` on"""
        assert text.dtype == torch.uint8 and out.dtype == torch.uint8 and text.is_contiguous() and out.is_contiguous()
        a = self.args
        a.first_record, a.count = int(first), int(stop) - int(first)
        a.text, a.text_base, a.text_bytes = text.data_ptr(), int(text_base), text.numel()
        a.out, a.out_base, a.out_bytes = out.data_ptr(), int(out_base), out.numel()
        self._call("pmt_vcf_write")
        return out

    def host_plan(self) -> Plan:
        return Plan(self.matched.cpu().numpy(), self.mask.cpu().numpy(), self.error_call.cpu().numpy(), self.out_length.cpu().numpy(),
                    self.counters.cpu().numpy())


def slabs(line_start: np.ndarray, slab_bytes: int):
    """[first, stop) runs of whole lines of at most `slab_bytes` input bytes each (one line at least)"""
    n, first = len(line_start) - 1, 0
    while first < n:
        stop = int(np.searchsorted(line_start, line_start[first] + max(int(slab_bytes), 1), side="right")) - 1
        stop = min(max(stop, first + 1), n)
        yield first, stop
        first = stop


# ---- the whole stage ---------------------------------------------------------------------------------------------------------------------------
def filtered_vcf_bytes(records: V.VcfRecords, posterior_int_rows, outputs, passing_call: int, device, slab_bytes: int = DEFAULT_SLAB_BYTES,
                       threads: int = 0):
    """-> (a generator of the output's data bytes slab by slab, the Plan).  Everything that can refuse the run -- a record without AD,
    an unformattable value -- has happened when this returns: nothing is written before."""
    values, filtered, variant_types = candidate_arrays(posterior_int_rows, outputs)
    if not on_device(device):
        matched = match_mirror(records, posterior_int_rows)
        flags = flags_with_alt_depth(records, matched)
        plan = plan_mirror(records, matched, flags, values, filtered, variant_types, passing_call)
        _check_formattable(plan, values)
        return iter([write_mirror(records, plan, flags, values)]), plan
    stage = DeviceVcf(records, posterior_int_rows, values, filtered, variant_types, passing_call, device, threads)
    matched = stage.match().cpu().numpy()
    stage.set_zero_alt_depth(flags_with_alt_depth(records, matched))
    stage.plan()
    plan = stage.host_plan()
    _check_formattable(plan, values)

    def generate():
        for first, stop in slabs(records.line_start, slab_bytes):
            text_base, out_base = int(records.line_start[first]), int(plan.out_start[first])
            text = torch.from_numpy(records.text[text_base: int(records.line_start[stop])]).to(device)
            out = torch.empty(int(plan.out_start[stop]) - out_base, dtype=torch.uint8, device=device)
            yield stage.write(first, stop, text, text_base, out, out_base).cpu().numpy().tobytes()

    return generate(), plan


def write_filtered_vcf(records: V.VcfRecords, header: List[bytes], posterior_int_rows, outputs: Dict[str, np.ndarray], passing_call: int,
                       device, path, slab_bytes: int = DEFAULT_SLAB_BYTES, threads: int = 0) -> Dict[str, int]:
    """Writes the filtered VCF to `path` (gzip when it ends in `.gz`) and returns the counters by name.  `outputs`: the arrays of
    --calls_output (`posterior_outputs`) and `artifact_logits_b`; `filtered_b` is taken as given.  On a ROCm device the library, else
    (and under PMT_FILTERED_VCF=torch) the numpy mirror: the same bytes."""
    new_header = amended_header(header, passing_call)
    chunks, plan = filtered_vcf_bytes(records, posterior_int_rows, outputs, passing_call, device, slab_bytes, threads)
    with (gzip.open(path, "wb") if str(path).endswith(".gz") else open(path, "wb")) as file:
        for line in new_header:
            file.write(line)
        for chunk in chunks:
            file.write(chunk)
    return plan.counts_dict()
