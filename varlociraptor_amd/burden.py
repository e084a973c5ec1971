"""Mutational burden: `estimate mutational-burden` (reference src/estimation/mutational_burden.rs).

The expected number of coding variants per megabase as a function of the (minimum) allele frequency: every coding record of an
annotated calls file gives one entry per sample and ALT allele, (FORMAT/AF, probability of the chosen events, signature), and each
output value is the ln_sum_exp of the probabilities of one signature within one VAF range, scaled to the coding genome size.  The
reduction over (range, group) cells has a HIP kernel behind the C ABI (`vlr_range_group_lse`, csrc/vlr_callstats.hip) and the
record pass runs in the engine (`vlr_calls_mutational_burden`, csrc/vlr_callsfile.cpp); next to them is the host restatement
(`device="cpu"`: the htslib-free reader of bcfio.py and numpy) that the CPU suite and the comparisons use.

Row order is this project's: the reference iterates a HashMap, so its order is unspecified.  Rows come by range index, then by
signature in declaration order (DEL METH INS INV DUP BND MNV Complex C>A C>G C>T T>A T>C T>G), then by sample name; empty cells
give no row.  `table` mode prints floats in shortest round-trip form (Python's repr); the reference's exact spelling of exponents
(Rust's Display through the csv crate) cannot be checked here, as there is no Rust toolchain to run it.  The plots are vega-lite
documents written for this project with the reference's data field names (`min_vaf` / `vaf`, `mb`, `vartype`, `sample`) and its
y-scale domains (print_plot, :192-212).
"""
from __future__ import annotations

import json
import math
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .fdr import LN10, _relative_eq

SIGNATURES = ("DEL", "METH", "INS", "INV", "DUP", "BND", "MNV", "Complex", "C>A", "C>G", "C>T", "T>A", "T>C", "T>G")  # :439-480
N_SIG = len(SIGNATURES)
_SNV_CLASS = {"C>A": 8, "G>T": 8, "C>G": 9, "G>C": 9, "C>T": 10, "G>A": 10, "T>A": 11, "A>T": 11, "T>C": 12, "A>G": 12, "T>G": 13, "A>C": 13}
MODES = ("hist", "curve", "multibar", "table")
NO_RECORDS = "unable to estimate TMB because no valid records were found in the given BCF/VCF"  # errors.rs:32
MAX_RANGES, MAX_GROUPS = 128, 14 * 16


def signature(ref: str, alt: str) -> int:
    """signatures() (:482-515) as an index into SIGNATURES; an SNV that is no substitution between A, C, G and T raises (the
    reference panics there)."""
    sym = {"<DEL>": 0, "<INV>": 3, "<DUP>": 4, "<BND>": 5, "<METH>": 1}
    if alt in sym:
        return sym[alt]
    if len(ref) == 1 and len(alt) == 1:
        try:
            return _SNV_CLASS[ref + ">" + alt]
        except KeyError:
            raise ValueError("%s>%s is not a substitution between A, C, G and T" % (ref, alt)) from None
    if len(ref) > 1 and len(alt) == 1:
        return 0
    if len(ref) == 1 and len(alt) > 1:
        return 2
    if len(ref) == len(alt) and len(ref) > 1:
        return 6
    return 7


def is_coding(ann: Optional[str]) -> bool:
    """is_valid_variant (:18-43): some ANN entry has |-field 7 == protein_coding and a non-empty field 13; no ANN: not coding."""
    if not isinstance(ann, str):
        return False
    for entry in ann.split(","):
        coding = False
        for i, field in enumerate(entry.split("|")):
            if i == 7:
                coding = field == "protein_coding"
            if i == 13:
                coding = coding and field != ""
        if coding:
            return True
    return False


def linspace(a: float, b: float, n: int) -> List[float]:
    """itertools_num::linspace: a + step * i."""
    step = (b - a) / (n - 1)
    return [a + step * i for i in range(n)]


def ranges(mode: str, cutoff: float = 0.2) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) of the half-open VAF ranges of a mode: curve / table [t_j, inf), hist [c_i - 0.05, c_i + 0.05), multibar
    [cutoff, 1.0) (a VAF of 1.0 is outside, as in the reference)."""
    if mode in ("curve", "table"):
        lo = linspace(0.0, 1.0, 100)
        hi = [math.inf] * 100
    elif mode == "hist":
        c = linspace(0.05, 0.95, 19)
        lo, hi = [x - 0.05 for x in c], [x + 0.05 for x in c]
    elif mode == "multibar":
        lo, hi = [float(cutoff)], [1.0]
    else:
        raise ValueError("unknown mode %r" % mode)
    return np.array(lo, np.float64), np.array(hi, np.float64)


def _ln_add_exp(a: float, b: float) -> float:
    if a != a or b != b:
        return math.nan
    if b > a:
        a, b = b, a
    if a == -math.inf:
        return a
    return a + math.log1p(math.exp(b - a))


def collect_entries(records, file_samples: Sequence[str], events: Sequence[str], samples: Sequence[str], by_sample: bool):
    """The record pass (:103-181): (vaf f64, ln_prob f64, group int32) per (sample, allele) of the coding records that carry every
    event tag, in the reference's push order: record order, within a record by sample name, then allele.  group = index of the
    sample in `samples` * 14 + signature (by_sample) or the signature."""
    cols = []
    for s in samples:
        if s not in file_samples:
            raise ValueError("Sample %s not found" % s)
        cols.append(list(file_samples).index(s))
    by_name = sorted(enumerate(cols), key=lambda sc: samples[sc[0]].encode())  # the reference iterates a BTreeMap keyed by sample name (:160)
    tags = ["PROB_" + e.upper() for e in events]
    vaf, lnp, grp = [], [], []
    for rec in records:
        afs = rec["format"].get("AF")
        if afs is None:
            raise ValueError("record %s:%d has no FORMAT/AF" % (rec["chrom"], rec["pos"]))
        if not is_coding(rec["info"].get("ANN")):
            continue
        alts = rec["alt"].split(",") if rec["alt"] != "." else []
        probs = [-math.inf] * len(alts)
        skip = False
        for t in tags:
            vals = rec["info"].get(t)
            if not isinstance(vals, list) or not vals:
                skip = True
                break
            if len(vals) < len(alts):
                raise ValueError("record %s:%d: %s has %d values for %d ALT alleles" % (rec["chrom"], rec["pos"], t, len(vals), len(alts)))
            for a in range(len(alts)):
                p = vals[a]
                probs[a] = _ln_add_exp(probs[a], math.nan if (p is None or p != p) else -float(p) * LN10 / 10.0)
        if skip:
            continue
        try:
            sig = [signature(rec["ref"], a) for a in alts]
        except ValueError as e:
            raise ValueError("record %s:%d: %s" % (rec["chrom"], rec["pos"], e)) from None
        for si, col in by_name:
            af = afs[col]
            for a in range(min(len(alts), len(af))):
                v = af[a]
                if v is None or v != v:
                    continue
                vaf.append(float(v))
                lnp.append(probs[a])
                grp.append((si * N_SIG if by_sample else 0) + sig[a])
    return np.array(vaf, np.float64), np.array(lnp, np.float64), np.array(grp, np.int32)


def _device_index(device) -> int:
    s = str(device)
    if s.startswith("cuda"):
        return int(s.split(":")[1]) if ":" in s else 0
    return int(s)


def range_group_lse(vaf, ln_prob, group, lo, hi, n_groups: int, device="cpu") -> np.ndarray:
    """out[r, g] = ln_sum_exp (bio semantics: the maximum apart, ln1p of the others) of the ln_prob of group g with
    lo[r] <= vaf < hi[r]; -inf for an empty cell; a NaN ln_prob makes its cells NaN.  device="cpu": the restatement, which adds a
    cell's terms in the reference's order (by VAF, equal VAFs in input order); an int or "cuda[:k]": vlr_range_group_lse (its own
    fixed order, include/vlr.h)."""
    vaf = np.ascontiguousarray(vaf, np.float64)
    lp = np.ascontiguousarray(ln_prob, np.float64)
    grp = np.ascontiguousarray(group, np.int32)
    lo = np.ascontiguousarray(lo, np.float64)
    hi = np.ascontiguousarray(hi, np.float64)
    R, G = len(lo), int(n_groups)
    if not (len(vaf) == len(lp) == len(grp)) or len(hi) != R:
        raise ValueError("array lengths differ")
    if not (1 <= R <= MAX_RANGES and 1 <= G <= MAX_GROUPS):
        raise ValueError("n_ranges outside [1, %d] or n_groups outside [1, %d]" % (MAX_RANGES, MAX_GROUPS))
    if len(grp) and (grp.min() < 0 or grp.max() >= G):
        raise ValueError("group outside [0, %d)" % G)
    out = np.full((R, G), -np.inf)
    if device != "cpu":
        import ctypes as C
        from . import engine
        L = engine.lib()
        engine.check(L.vlr_range_group_lse(_device_index(device), len(vaf), vaf.ctypes.data, lp.ctypes.data, grp.ctypes.data, R, lo.ctypes.data, hi.ctypes.data, G, out.ctypes.data))
        return out
    # The reference's order of a cell's terms: its map is keyed by VAF and a key's entries keep their push order, so a range query
    # walks the entries by (VAF, push order); into_group_map keeps that order within a group.  Sort once by (group, VAF), stable.
    order = np.lexsort((vaf, grp))
    gs, vs, ps = grp[order], vaf[order], lp[order]
    starts = np.searchsorted(gs, np.arange(G + 1))
    for g in range(G):
        v, p = vs[starts[g]:starts[g + 1]], ps[starts[g]:starts[g + 1]]
        if not len(v):
            continue
        for r in range(R):
            a, b = np.searchsorted(v, lo[r], "left"), np.searchsorted(v, hi[r], "left")  # v ascending: lo <= v < hi is one slice
            if b > a:
                out[r, g] = _ln_sum_exp(p[a:b])
    return out


_SEQUENTIAL_MAX = 4096


def _ln_sum_exp(q: np.ndarray) -> float:
    """bio ln_sum_exp over the terms in the given order: first maximum apart, the others added sequentially
    from 0.0, ln1p.  Up to _SEQUENTIAL_MAX terms this is the reference's arithmetic operation for operation, with libm's exp;
    longer cells use numpy's exp (which may differ from libm's in the last bit) and a sequential accumulate."""
    if np.isnan(q).any():
        return math.nan
    im = int(np.argmax(q))  # first occurrence, as the reference's strict > keeps it
    m = float(q[im])
    if m == -math.inf:
        return m
    if len(q) <= _SEQUENTIAL_MAX:
        s = 0.0
        for i, x in enumerate(q.tolist()):
            if i != im and x != -math.inf:
                s += math.exp(x - m)
        return m + math.log1p(s)
    t = np.exp(q - m)
    t[im] = 0.0
    return m + math.log1p(float(np.add.accumulate(t)[-1]))


def last_kernel_ms() -> Tuple[float, float]:
    """vlr_callstats_last_kernel_ms: device milliseconds of the kernels of the last vlr_range_group_lse and vlr_posterior_odds_keep."""
    import ctypes as C
    from . import engine
    L = engine.lib()
    a, b = C.c_double(), C.c_double()
    L.vlr_callstats_last_kernel_ms(C.byref(a), C.byref(b))
    return float(a.value), float(b.value)


def cells_native(path: str, events: Sequence[str], samples: Sequence[str], by_sample: bool, lo, hi, device: int = 0, threads: int = 0) -> Tuple[np.ndarray, int]:
    """vlr_calls_mutational_burden (include/vlr.h): record pass and reduction in the engine.  Returns (cells [R, G], n_entries)."""
    import ctypes as C
    from . import engine
    L = engine.lib()
    lo = np.ascontiguousarray(lo, np.float64)
    hi = np.ascontiguousarray(hi, np.float64)
    G = (len(samples) if by_sample else 1) * N_SIG
    out = np.full((len(lo), G), -np.inf)
    ev = (C.c_char_p * len(events))(*[e.encode() for e in events])
    sm = (C.c_char_p * len(samples))(*[s.encode() for s in samples])
    n = C.c_int64()
    engine.check(L.vlr_calls_mutational_burden(path.encode(), len(events), ev, len(samples), sm, int(bool(by_sample)), len(lo), lo.ctypes.data, hi.ctypes.data,
                                               int(device), int(threads), out.ctypes.data, C.byref(n)))
    return out, int(n.value)


def cells_host(path: str, events: Sequence[str], samples: Sequence[str], by_sample: bool, lo, hi) -> Tuple[np.ndarray, int]:
    """The restatement of cells_native: bcfio reader, collect_entries, numpy reduction."""
    from .bcfio import BcfReader
    r = BcfReader(path)
    vaf, lnp, grp = collect_entries(r, r.samples, events, samples, by_sample)
    if not len(vaf):
        raise ValueError(NO_RECORDS)
    return range_group_lse(vaf, lnp, grp, lo, hi, (len(samples) if by_sample else 1) * N_SIG), len(vaf)


def rows(mode: str, cells: np.ndarray, samples: Sequence[str], coding_genome_size: float, cutoff: float = 0.2) -> List[dict]:
    """The output rows of a mode from its cells ([R, 14], multibar [1, n_samples * 14]): mb = e^cell / coding_genome_size * 1e6
    (calc_mb, :186-190); by range index, then signature in declaration order, then sample name; `_range` is the range index."""
    lo, _ = ranges(mode, cutoff)
    centers = linspace(0.05, 0.95, 19)
    out = []
    for r in range(cells.shape[0]):
        for s in range(N_SIG):
            if mode == "multibar":
                for name, si in sorted((name, si) for si, name in enumerate(samples)):
                    c = cells[r, si * N_SIG + s]
                    if c != -math.inf:
                        out.append({"_range": r, "vaf": float(cutoff), "mb": math.exp(c) / coding_genome_size * 1000000.0, "vartype": SIGNATURES[s], "sample": name})
                continue
            c = cells[r, s]
            if c == -math.inf:
                continue
            mb = math.exp(c) / coding_genome_size * 1000000.0
            if mode == "hist":
                out.append({"_range": r, "vaf": centers[r], "mb": mb, "vartype": SIGNATURES[s]})
            else:
                out.append({"_range": r, "min_vaf": float(lo[r]), "mb": mb, "vartype": SIGNATURES[s]})
    return out


def table_text(rws: Sequence[dict]) -> str:
    """`table` mode: TSV, floats in shortest round-trip form."""
    return "min_vaf\tmb\tvartype\n" + "".join("%r\t%r\t%s\n" % (r["min_vaf"], r["mb"], r["vartype"]) for r in rws)


def plot_document(mode: str, rws: Sequence[dict]) -> dict:
    """A vega-lite document of a mode's rows.  y-scale domains as print_plot (:192-212): curve takes the maximum at range 0 and the
    cut point at range 10, hist the maximum at range 0 and the cut point at range 2 (each the sum over the signatures), multibar
    the largest bar for both; equal cut point and maximum: one panel from 0."""
    x = "min_vaf" if mode == "curve" else "vaf"
    values = [{k: v for k, v in r.items() if k != "_range"} for r in rws]
    if mode == "multibar":
        max_mb = cut_mb = max([r["mb"] for r in rws if r["mb"] > 0.0], default=0.0)
    else:
        cut_at = 10 if mode == "curve" else 2
        max_mb = sum(r["mb"] for r in rws if r["_range"] == 0)
        cut_mb = sum(r["mb"] for r in rws if r["_range"] == cut_at)

    def panel(domain, height, with_x):
        enc = {"x": {"field": x, "type": "quantitative" if mode == "curve" else "ordinal", "title": "minimum VAF" if mode == "curve" else "VAF",
                     "axis": None if not with_x else {}},
               "y": {"field": "mb", "type": "quantitative", "aggregate": "sum", "title": "variants per megabase", "scale": {"domain": domain, "clamp": True}},
               "color": {"field": "vartype", "type": "nominal", "title": "signature"}}
        if mode == "multibar":
            enc["x"] = {"field": "sample", "type": "nominal", "title": "sample"}
        return {"height": height, "width": 480, "mark": {"type": "area" if mode == "curve" else "bar", "clip": True}, "encoding": enc}

    doc = {"$schema": "https://vega.github.io/schema/vega-lite/v5.json", "description": "mutational burden (%s)" % mode, "data": {"values": values},
           "spacing": 4, "vconcat": [panel([0.0, max_mb], 240, True)]}
    if mode != "multibar" and not _relative_eq(cut_mb, max_mb):
        doc["vconcat"] = [panel([cut_mb, max_mb], 60, False), panel([0.0, cut_mb], 240, True)]
    return doc


def estimate(path: str, events: Sequence[str], samples: Sequence[str], coding_genome_size: float, mode: str, cutoff: float = 0.2, device="0", out=None) -> List[dict]:
    """The command: rows of `mode` from the annotated calls BCF `path`, written to `out` (default stdout) as TSV (table) or as a
    vega-lite document.  device: HIP device index, or "cpu" for the restatement."""
    if mode not in MODES:
        raise ValueError("unknown mode %r" % mode)
    lo, hi = ranges(mode, cutoff)
    by_sample = mode == "multibar"
    if device == "cpu":
        cells, _ = cells_host(path, events, samples, by_sample, lo, hi)
    else:
        cells, _ = cells_native(path, events, samples, by_sample, lo, hi, device=_device_index(device))
    rws = rows(mode, cells, samples, float(coding_genome_size), cutoff)
    fh = out if out is not None else sys.stdout
    if mode == "table":
        fh.write(table_text(rws))
    else:
        fh.write(json.dumps(plot_document(mode, rws), indent=2) + "\n")
    return rws
