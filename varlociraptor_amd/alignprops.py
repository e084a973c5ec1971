"""`estimate alignment-properties` (reference src/estimation/alignment_properties.rs, src/cli.rs:423-448, 1321-1334).

Gap and homopolymer-run parameters, the wildtype homopolymer error model, the insert size and the CIGAR maxima of a sample, from
the first N mapped records of its BAM files.  The per-record work — the CIGAR walk against the reference, 16 x 16 transition
counts, homopolymer-run counters, maxima and insert sizes — runs as HIP (`vlr_bamstats_*`, csrc/vlr_bamstats.hip; `device=k`).
`device="cpu"` is the pure-Python restatement of `AlignmentProperties::estimate` (:148-463) and `cigar_stats` (:693-861) that the
CPU suite uses and the GPU suite compares against.  Both hand their integer counts to the same finishing math (`finish`: insert-size
percentiles, mean / sd, `estimate_gap_params`, `estimate_hop_params`, `wildtype_homopolymer_error_model`, :864-1012) and the same
serde-style JSON writer (`to_json`).  `load` reads the JSON back into `realign.GapParams` / `realign.HopParams`.

Also here: a small BAM / BGZF writer and a pseudo-bin BAI writer for synthetic test inputs (the project's BAM reader is
`readwindows.read_bam`), and the mapped counts of BAI / CSI indices the default record count needs (:466-531).
"""
from __future__ import annotations

import gzip
import json
import math
import os
import struct
import sys
import zlib
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import realign

# ------------------------------------------------------------------------------------------------ states (:537-606)
MATCH = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
GAP_X, GAP_Y, OTHER = 4, 5, 14
N_STATES = 14          # STATES: every state but Other (:556-571)
MIN_HOMOPOLYMER_LEN = 2
I16_MAX = 32767
SEQ_CODE = b"=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
# records per the reference's skip rule (:286-292): mapq 0, duplicate (0x400), QC fail (0x200), unmapped (0x4), empty SEQ
FLAG_PAIRED, FLAG_UNMAPPED, FLAG_MATE_UNMAPPED, FLAG_FIRST, FLAG_QCFAIL, FLAG_DUP = 0x1, 0x4, 0x8, 0x40, 0x200, 0x400


def _upper(c: int) -> int:
    return c - 32 if 97 <= c <= 122 else c


def state_match(c: int) -> int:
    return MATCH.get(_upper(c), OTHER)


def state_hop_x(c: int) -> int:
    m = MATCH.get(_upper(c))
    return OTHER if m is None else 6 + 2 * m


def state_hop_y(c: int) -> int:
    m = MATCH.get(_upper(c))
    return OTHER if m is None else 7 + 2 * m


class AlignPropsError(ValueError):
    """A malformed input: a record, a CIGAR running past its contig or read, a missing contig or index."""


# ------------------------------------------------------------------------------------------------ counts
@dataclass
class Counts:
    """What the per-record pass leaves: integer counts only (the device path returns exactly these)."""
    transitions: np.ndarray = field(default_factory=lambda: np.zeros((16, 16), dtype=np.int64))
    hops: Dict[Tuple[int, int, int], int] = field(default_factory=dict)   # (raw base byte, k0, k1) -> count (CigarStats::hop_counts)
    insert_sizes: List[int] = field(default_factory=list)                 # one per record that gives one, in record order
    max_del: Optional[int] = None
    max_ins: Optional[int] = None
    frac_max_softclip: Optional[float] = None
    max_read_len: int = 0
    max_mapq: int = 0
    n_taken: int = 0               # n_records_analysed
    n_skipped: int = 0             # n_records_skipped (records read before the cap that the skip rule drops)
    n_not_usable: int = 0          # is_not_regular
    n_softclips: int = 0
    n_not_paired: int = 0          # RecordFlagStats over the taken records (:196-207)
    n_not_first: int = 0
    n_mate_unmapped: int = 0
    n_tid_mismatch: int = 0
    seconds: Optional[List[float]] = None   # the device path's stage times (vlr_bamstats_counts.seconds)

    def hop(self, base: int, k0: int, k1: int):
        key = (base, k0, k1)
        self.hops[key] = self.hops.get(key, 0) + 1


# ------------------------------------------------------------------------------------------------ BAM reading
@dataclass
class Record:
    tid: int
    pos: int
    mapq: int
    flag: int
    cigar: List[Tuple[int, int]]   # (op code 0..8, length)
    seq: bytes                     # decoded letters of "=ACMGRSVTWYHKDBN"
    mtid: int
    tlen: int
    aux: bytes
    index: int                     # record number in its file (0-based, header excluded)


def inflate_bgzf(path: str) -> bytes:
    with open(path, "rb") as f:
        raw = f.read()
    try:
        return gzip.decompress(raw)
    except (OSError, EOFError, zlib.error) as e:
        raise AlignPropsError(f"{path}: corrupt or truncated BGZF stream ({e})")


def bam_header(d: bytes, path: str = "BAM") -> Tuple[List[Tuple[str, int]], int]:
    """(contigs, offset of the first record) of an inflated BAM stream (SAM spec 4.2)."""
    if len(d) < 12 or d[:4] != b"BAM\x01":
        raise AlignPropsError(f"{path}: not a BAM file")
    l_text, = struct.unpack_from("<i", d, 4)
    o = 8 + l_text
    if l_text < 0 or o + 4 > len(d):
        raise AlignPropsError(f"{path}: truncated BAM header")
    n_ref, = struct.unpack_from("<i", d, o)
    o += 4
    contigs = []
    for _ in range(n_ref):
        if o + 4 > len(d):
            raise AlignPropsError(f"{path}: truncated BAM header")
        l_name, = struct.unpack_from("<i", d, o)
        if l_name < 1 or o + 8 + l_name > len(d):
            raise AlignPropsError(f"{path}: truncated BAM header")
        name = d[o + 4:o + 4 + l_name - 1].decode()
        l_ref, = struct.unpack_from("<i", d, o + 4 + l_name)
        contigs.append((name, l_ref))
        o += 8 + l_name
    return contigs, o


def iter_records(d: bytes, o: int, path: str = "BAM") -> Iterable[Record]:
    """The records of an inflated BAM stream from offset o, each checked against its block_size (a malformed one is an error)."""
    k = 0
    while o < len(d):
        if o + 4 > len(d):
            raise AlignPropsError(f"{path}: record {k}: truncated")
        bs, = struct.unpack_from("<I", d, o)
        end = o + 4 + bs
        if bs < 32 or end > len(d):
            raise AlignPropsError(f"{path}: record {k}: truncated or malformed (block_size {bs})")
        tid, pos, l_rn, mapq, _bin, n_cig, flag, l_seq, mtid, _mpos, tlen = struct.unpack_from("<iiBBHHHiiii", d, o + 4)
        p = o + 36
        fixed = l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        if l_seq < 0 or l_rn < 1 or p + fixed > end:
            raise AlignPropsError(f"{path}: record {k}: malformed (fields overrun block_size)")
        p += l_rn
        cig = []
        for j in range(n_cig):
            v, = struct.unpack_from("<I", d, p + 4 * j)
            if (v & 15) > 8:
                raise AlignPropsError(f"{path}: record {k}: unknown CIGAR operation {v & 15}")
            cig.append((v & 15, v >> 4))
        p += 4 * n_cig
        packed = d[p:p + (l_seq + 1) // 2]
        seq = bytearray(l_seq)
        for i in range(l_seq):
            b = packed[i >> 1]
            seq[i] = SEQ_CODE[(b >> 4) if (i & 1) == 0 else (b & 15)]
        p += (l_seq + 1) // 2 + l_seq
        yield Record(tid, pos, mapq, flag, cig, bytes(seq), mtid, tlen, d[p:end], k)
        o = end
        k += 1


def aux_ef_is_one(aux: bytes) -> bool:
    """utils/mod.rs:61-71 aux_tag_is_entire_fragment: the first EF tag, of an integer type (c C s S i I), equals 1."""
    sizes = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}
    ints = {ord("c"): "<b", ord("C"): "<B", ord("s"): "<h", ord("S"): "<H", ord("i"): "<i", ord("I"): "<I"}
    p = 0
    while p + 3 <= len(aux):
        tag, t = aux[p:p + 2], aux[p + 2]
        q = p + 3
        if t in sizes:
            n = sizes[t]
        elif t in (ord("Z"), ord("H")):
            z = aux.find(b"\0", q)
            if z < 0:
                return False
            n = z + 1 - q
        elif t == ord("B"):
            if q + 5 > len(aux):
                return False
            sub, cnt = aux[q], struct.unpack_from("<I", aux, q + 1)[0]
            if sub not in sizes or sub == ord("A"):
                return False
            n = 5 + cnt * sizes[sub]
        else:
            return False
        if q + n > len(aux):
            return False
        if tag == b"EF":
            return t in ints and struct.unpack_from(ints[t], aux, q)[0] == 1
        p = q + n
    return False


# ------------------------------------------------------------------------------------------------ FASTA through its .fai
def read_fai(fasta: str) -> Dict[str, Tuple[int, int, int, int]]:
    """name -> (length, offset, line bases, line width) of FASTA.fai (the reference reads through bio's IndexedReader)."""
    fai = fasta + ".fai"
    if not os.path.exists(fai):
        raise AlignPropsError(f"{fasta}: no .fai index (index the reference with samtools faidx)")
    out = {}
    with open(fai) as f:
        for line in f:
            t = line.rstrip("\n").split("\t")
            if len(t) >= 5:
                out[t[0]] = (int(t[1]), int(t[2]), int(t[3]), int(t[4]))
    return out


def read_contig(fasta: str, entry: Tuple[int, int, int, int]) -> bytes:
    """One contig's bases, case preserved."""
    length, off, lb, lw = entry
    if length == 0:
        return b""
    nlines = (length - 1) // lb + 1
    with open(fasta, "rb") as f:
        f.seek(off)
        raw = f.read((nlines - 1) * lw + (length - (nlines - 1) * lb))
    seq = b"".join(raw[i * lw:i * lw + lb] for i in range(nlines))[:length]
    if len(seq) != length:
        raise AlignPropsError(f"{fasta}: contig shorter than its .fai entry")
    return seq


# ------------------------------------------------------------------------------------------------ the per-record pass
def _taken(r: Record) -> bool:
    """:286-292: not skipped (secondary and supplementary records are kept)."""
    return not (r.mapq == 0 or r.flag & (FLAG_DUP | FLAG_QCFAIL | FLAG_UNMAPPED) or len(r.seq) == 0)


def _extend(base: int, ref: bytes, start: int, step: int, stop: int) -> int:
    """utils/homopolymers.rs:162-165 extend_homopolymer_stretch over ref[start], ref[start + step], ... (stop exclusive)."""
    b = _upper(base)
    n, i = 0, start
    while i != stop and _upper(ref[i]) == b:
        n += 1
        i += step
    return n


def cigar_stats(r: Record, ref: bytes, c: Counts, where: str) -> Tuple[bool, Optional[int]]:
    """:693-861 for one record (allow_hardclips = false: the CLI estimates the insert size).  Adds to c; returns (is_not_regular,
    ref end position).  Accesses the reference would make out of bounds (it panics there) raise AlignPropsError."""
    T = c.transitions
    qseq, L = r.seq, len(ref)
    qpos, rpos = 0, r.pos
    irregular = soft = False
    fmax = None

    def oob(what):
        raise AlignPropsError(f"{where}: {what} (CIGAR runs past the contig or the read)")

    if rpos < 0:
        oob("negative position")
    for op, l in r.cigar:
        if op == 2:                                           # D
            c.max_del = l if c.max_del is None else max(c.max_del, l)
            irregular = True
            if l < I16_MAX:
                if l == 0 or rpos + l > L:
                    oob(f"deletion of {l} at {rpos}")
                base = ref[rpos]
                bu = _upper(base)
                hom = all(_upper(x) == bu for x in ref[rpos + 1:rpos + l])
                if hom:
                    ln = l
                    if rpos + l < L:
                        ln += _extend(base, ref, rpos + l, 1, L)
                    if rpos > 1:                              # reads ref[..rpos - 1] in reverse: base rpos - 1 is skipped
                        ln += _extend(base, ref, rpos - 2, -1, -1)
                    if ln >= MIN_HOMOPOLYMER_LEN:
                        ms, hs = state_match(base), state_hop_x(base)
                        T[ms, ms] += l
                        T[ms, hs] += 1
                        T[hs, hs] += max(ln - max(l - 2, 0), 0)
                        if rpos + ln + 1 < L:
                            T[hs, state_match(ref[rpos + ln + 1])] += 1
                        c.hop(base, ln, ln - l)
                if not hom or l == 1:
                    T[state_match(base), GAP_X] += 1
                    T[GAP_X, GAP_X] += max(l - 2, 0)
                    if rpos + l + 1 < L:
                        T[GAP_X, state_match(ref[rpos + l + 1])] += 1
            rpos += l
        elif op == 1:                                         # I
            c.max_ins = l if c.max_ins is None else max(c.max_ins, l)
            irregular = True
            if l < I16_MAX:
                if rpos >= L or qpos + max(l, 1) > len(qseq):
                    oob(f"insertion of {l} at {rpos}")
                base = ref[rpos] if _upper(ref[rpos]) == qseq[qpos] else qseq[qpos]
                q0 = _upper(qseq[qpos])
                hom = all(_upper(x) == q0 for x in qseq[qpos:qpos + l])
                if hom:
                    ln = l + _extend(qseq[qpos], ref, rpos, 1, L)
                    if rpos > 0:
                        ln += _extend(qseq[qpos], ref, rpos - 1, -1, -1)
                    if ln >= MIN_HOMOPOLYMER_LEN:
                        ms, hs = state_match(base), state_hop_y(base)
                        T[ms, ms] += l
                        T[ms, hs] += 1
                        T[hs, hs] += max(ln - max(l - 2, 0), 0)
                        if rpos + 1 < L:
                            T[hs, state_match(ref[rpos + 1])] += 1
                        c.hop(base, ln - l, l)
                if not hom or l == 1:
                    T[state_match(base), GAP_Y] += 1
                    T[GAP_Y, GAP_Y] += max(l - 2, 0)
                    if rpos + l + 1 < L:
                        T[GAP_Y, state_match(ref[rpos + l + 1])] += 1
            qpos += l
        elif op in (0, 7, 8):                                 # M = X
            if rpos + l > L or qpos + l > len(qseq):
                oob(f"match of {l} at {rpos}")
            k = 0
            while k < l:                                      # group_by the raw (rbase, qbase) pair
                rb, qb = ref[rpos + k], qseq[qpos + k]
                e = k + 1
                while e < l and ref[rpos + e] == rb and qseq[qpos + e] == qb:
                    e += 1
                if _upper(rb) == qb and e - k >= MIN_HOMOPOLYMER_LEN:
                    c.hop(rb, e - k, e - k)
                k = e
            for k in range(l - 1):                            # tuple_windows: within one operation
                T[state_match(ref[rpos + k]), state_match(ref[rpos + k + 1])] += 1
            qpos += l
            rpos += l
        elif op == 4:                                         # S
            s = l / len(qseq)
            fmax = s if fmax is None else max(fmax, s)
            irregular = soft = True
            qpos += l
        elif op == 3:                                         # N
            rpos += l
        elif op == 5:                                         # H (hard clips make a record irregular: omit_insert_size = false)
            irregular = True
    if fmax is not None:
        c.frac_max_softclip = fmax if c.frac_max_softclip is None else max(c.frac_max_softclip, fmax)
    c.n_not_usable += irregular
    c.n_softclips += soft
    return irregular, rpos


def count_bams(fasta: str, bams: Sequence[str], num_records: int) -> Counts:
    """The loop of :277-369 over the files in the order given (the same file may come twice): the first num_records taken records."""
    fai = read_fai(fasta)
    refs: Dict[str, bytes] = {}
    c = Counts()
    for path in bams:
        if c.n_taken >= num_records:
            break
        d = inflate_bgzf(path)
        contigs, o = bam_header(d, path)
        for r in iter_records(d, o, path):
            if not _taken(r):
                c.n_skipped += 1
                continue
            c.n_taken += 1
            c.n_not_paired += not (r.flag & FLAG_PAIRED)
            c.n_not_first += not (r.flag & FLAG_FIRST)
            c.n_mate_unmapped += bool(r.flag & FLAG_MATE_UNMAPPED)
            c.n_tid_mismatch += r.tid != r.mtid
            if not 0 <= r.tid < len(contigs):
                raise AlignPropsError(f"{path}: record {r.index}: reference id {r.tid} out of range")
            name = contigs[r.tid][0]
            if name not in refs:
                if name not in fai:
                    raise AlignPropsError(f"{fasta}: contig {name} (of {path}) is missing from the reference")
                refs[name] = read_contig(fasta, fai[name])
            irregular, end = cigar_stats(r, refs[name], c, f"{path}: record {r.index}")
            if not irregular:
                if r.flag & FLAG_PAIRED:
                    if r.flag & FLAG_FIRST and r.tid == r.mtid and not r.flag & FLAG_MATE_UNMAPPED:
                        c.insert_sizes.append(abs(r.tlen))
                elif aux_ef_is_one(r.aux):
                    c.insert_sizes.append(end - r.pos)
            c.max_mapq = max(c.max_mapq, r.mapq)
            c.max_read_len = max(c.max_read_len, len(r.seq))
            if c.n_taken >= num_records:
                break
    return c


# ------------------------------------------------------------------------------------------------ finishing math
def percentile_r8(values: Sequence[float], p: int) -> float:
    """statrs 0.18 Data::percentile(p) = quantile(p / 100), R-8: h = (n + 1/3) tau + 1/3."""
    x = sorted(values)
    n = len(x)
    tau = p / 100.0
    if n == 0 or tau < 0.0 or tau > 1.0:
        return math.nan
    h = (n + 1.0 / 3.0) * tau + 1.0 / 3.0
    hf = int(h)
    if hf <= 0 or tau == 0.0:
        return x[0]
    if hf >= n or tau == 1.0:
        return x[-1]
    a, b = x[hf - 1], x[hf]
    return a + (h - hf) * (b - a)


def sample_std_dev(values: Sequence[float]) -> float:
    """statrs Statistics::variance (running sum form), square-rooted: NaN below two values."""
    it = iter(values)
    try:
        s = float(next(it))
    except StopIteration:
        return math.nan
    i, var = 1.0, 0.0
    for x in it:
        x = float(x)
        i += 1.0
        s += x
        diff = i * x - s
        var += diff * diff / (i * (i - 1.0))
    return math.sqrt(var / (i - 1.0)) if i > 1.0 else math.nan


def insert_size(tlens: Sequence[int]) -> Optional[Tuple[float, float]]:
    """:413-431: values within [percentile 5, percentile 95]; mean over them, sample sd (NaN with fewer than two)."""
    if not tlens:
        return None
    v = [float(t) for t in tlens]
    upper, lower = percentile_r8(v, 95), percentile_r8(v, 5)
    valid = [t for t in v if lower <= t <= upper]
    mean = sum(valid, 0.0) / len(valid) if valid else math.nan
    return mean, sample_std_dev(valid)


def _ln_checked(p: float) -> float:
    """LogProb::from(Prob::checked(p).unwrap_or(Prob::zero())): ln p for p in [0, 1], ln 0 otherwise (NaN included)."""
    if not (0.0 <= p <= 1.0):
        return -math.inf
    return math.log(p) if p > 0.0 else -math.inf


def _div(a: int, b: int) -> float:
    if b == 0:
        return math.nan if a == 0 else math.inf
    return a / b


def gap_params(T: np.ndarray) -> Optional[realign.GapParams]:
    """:864-931; None: the fallback to GapParams::default() (a start or extension count below 100)."""
    out, insufficient = [], False
    from_match = int(T[0:4, 0:N_STATES].sum())
    for gap in (GAP_X, GAP_Y):
        start = int(T[0:4, gap].sum())
        extend = int(T[gap, gap])
        insufficient |= start < 100 or extend < 100
        from_gap = int(T[gap, 0:N_STATES].sum())
        out.append((_ln_checked(_div(start, from_match)), _ln_checked(_div(extend, from_gap))))
    if insufficient:
        return None
    # [GapX, GapY] destructured as [[insertion...], [deletion...]]: deletions (GapX) feed prob_insertion_*
    (ins, ins_ext), (dele, del_ext) = out
    return realign.GapParams(ins, dele, ins_ext, del_ext)


def hop_params(T: np.ndarray) -> Optional[realign.HopParams]:
    """:933-983; None: the fallback to HopParams::default() (start + extend below 100 for a base and direction)."""
    seq, ref, insufficient = [], [], False
    for m in range(4):
        from_prev = int(T[m, 0:N_STATES].sum())
        probs = []
        for hop in (6 + 2 * m, 7 + 2 * m):
            n = int(T[m, hop]) + int(T[hop, hop])
            insufficient |= n < 100
            probs.append(_ln_checked(_div(n, from_prev)))
        seq.append(probs[0])
        ref.append(probs[1])
    if insufficient:
        return None
    return realign.HopParams(tuple(seq), tuple(ref), tuple(seq), tuple(ref))


def wildtype_model(hops: Dict[Tuple[int, int, int], int]) -> Dict[int, float]:
    """:985-1012: key k0 - k1 clamped to i16; denominator = sum of the counters >= 10; numerators sum every count."""
    n = float(sum(v for v in hops.values() if v >= 10))
    grouped: Dict[int, int] = {}
    for (_b, k0, k1), v in hops.items():
        k = max(-32768, min(32767, k0 - k1))
        grouped[k] = grouped.get(k, 0) + v
    out = {}
    for k in sorted(grouped):
        v = grouped[k]
        out[k] = (v / n) if n != 0.0 else (math.nan if v == 0 else math.inf)
    return out


@dataclass
class AlignmentProperties:
    insert_size: Optional[Tuple[float, float]]   # (mean, sd)
    max_del_cigar_len: Optional[int]
    max_ins_cigar_len: Optional[int]
    frac_max_softclip: Optional[float]
    max_read_len: int
    max_mapq: int
    gap_params: realign.GapParams
    hop_params: realign.HopParams
    wildtype_homopolymer_error_model: Dict[int, float]
    gap_fallback: bool = False
    hop_fallback: bool = False


def finish(c: Counts) -> AlignmentProperties:
    g, h = gap_params(c.transitions), hop_params(c.transitions)
    return AlignmentProperties(insert_size(c.insert_sizes), c.max_del, c.max_ins, c.frac_max_softclip, c.max_read_len, c.max_mapq,
                               g or realign.GapParams(), h or realign.HopParams(), wildtype_model(c.hops), g is None, h is None)


# ------------------------------------------------------------------------------------------------ serde_json::to_string_pretty
def ryu(x: float) -> str:
    """A finite f64 as serde_json writes it (ryu's shortest digits and layout); NaN and +-inf as null."""
    if x != x or x in (math.inf, -math.inf):
        return "null"
    if x == 0.0:
        return "-0.0" if math.copysign(1.0, x) < 0 else "0.0"
    sign = "-" if x < 0 else ""
    mant, _, ex = repr(abs(x)).partition("e")
    ip, _, fp = mant.partition(".")
    digits = (ip + fp).lstrip("0")
    k = (int(ex) if ex else 0) - len(fp)
    stripped = digits.rstrip("0")
    k += len(digits) - len(stripped)
    digits = stripped
    n = len(digits)
    kk = n + k                                   # 10^(kk - 1) <= x < 10^kk
    if 0 <= k and kk <= 16:
        s = digits + "0" * k + ".0"
    elif 0 < kk <= 16:
        s = digits[:kk] + "." + digits[kk:]
    elif -5 < kk <= 0:
        s = "0." + "0" * (-kk) + digits
    elif n == 1:
        s = digits + "e" + str(kk - 1)
    else:
        s = digits[0] + "." + digits[1:] + "e" + str(kk - 1)
    return sign + s


def _opt_int(v):
    return "null" if v is None else str(int(v))


def to_json(p: AlignmentProperties) -> str:
    """serde_json::to_string_pretty(&AlignmentProperties): struct order, two-space indent; the model map in ascending key order."""
    def arr(vals, ind):
        return "[\n" + ",\n".join(ind + "  " + ryu(v) for v in vals) + "\n" + ind + "]"

    L = ["{"]
    if p.insert_size is None:
        L.append('  "insert_size": null,')
    else:
        L += ['  "insert_size": {', f'    "mean": {ryu(p.insert_size[0])},', f'    "sd": {ryu(p.insert_size[1])}', "  },"]
    L.append(f'  "max_del_cigar_len": {_opt_int(p.max_del_cigar_len)},')
    L.append(f'  "max_ins_cigar_len": {_opt_int(p.max_ins_cigar_len)},')
    L.append(f'  "frac_max_softclip": {"null" if p.frac_max_softclip is None else ryu(p.frac_max_softclip)},')
    L.append(f'  "max_read_len": {int(p.max_read_len)},')
    L.append(f'  "max_mapq": {int(p.max_mapq)},')
    g = p.gap_params
    L += ['  "gap_params": {', f'    "prob_insertion_artifact": {ryu(g.prob_insertion_artifact)},',
          f'    "prob_deletion_artifact": {ryu(g.prob_deletion_artifact)},',
          f'    "prob_insertion_extend_artifact": {ryu(g.prob_insertion_extend_artifact)},',
          f'    "prob_deletion_extend_artifact": {ryu(g.prob_deletion_extend_artifact)}', "  },"]
    h = p.hop_params
    L.append('  "hop_params": {')
    names = ("prob_seq_homopolymer", "prob_ref_homopolymer", "prob_seq_extend_homopolymer", "prob_ref_extend_homopolymer")
    for i, nm in enumerate(names):
        L.append(f'    "{nm}": {arr(getattr(h, nm), "    ")}' + ("," if i < 3 else ""))
    L.append("  },")
    m = p.wildtype_homopolymer_error_model
    if not m:
        L.append('  "wildtype_homopolymer_error_model": {},')
    else:
        L.append('  "wildtype_homopolymer_error_model": {')
        ks = sorted(m)
        L += [f'    "{k}": {ryu(m[k])}' + ("," if i < len(ks) - 1 else "") for i, k in enumerate(ks)]
        L.append("  },")
    L.append('  "initial": false')
    L.append("}")
    return "\n".join(L)


# BackwardsCompatibility::default_homopolymer_error_model (:39-50)
DEFAULT_WILDTYPE_MODEL = {0: 0.9975414130829068, 1: 0.0010076175889726332, -1: 0.0010076175889726332, -2: 0.00020152351779452663,
                          2: 0.00010076175889726332, 3: 5.038087944863166e-5, -3: 9.068558300753699e-5}


def load(path_or_text: str) -> AlignmentProperties:
    """An alignment-properties JSON (a path or the text) with serde's defaults (:59-83); null gap / hop values are ln 0
    (parse_float_or_null, pairhmm.rs:136-142); unknown fields (the `cigar_counts` of older reference versions) are ignored."""
    text = path_or_text
    if not path_or_text.lstrip().startswith("{"):
        with open(path_or_text) as f:
            text = f.read()
    d = json.loads(text)

    def ln(v):
        return -math.inf if v is None else float(v)

    def num(v):
        return math.nan if v is None else float(v)

    g = realign.GapParams()
    if d.get("gap_params") is not None:
        gp = d["gap_params"]
        g = realign.GapParams(ln(gp["prob_insertion_artifact"]), ln(gp["prob_deletion_artifact"]),
                              ln(gp["prob_insertion_extend_artifact"]), ln(gp["prob_deletion_extend_artifact"]))
    h = realign.HopParams()
    if d.get("hop_params") is not None:
        hp = d["hop_params"]
        h = realign.HopParams(*(tuple(ln(v) for v in hp[k]) for k in
                                ("prob_seq_homopolymer", "prob_ref_homopolymer", "prob_seq_extend_homopolymer", "prob_ref_extend_homopolymer")))
    isz = d.get("insert_size")
    model = d.get("wildtype_homopolymer_error_model")
    return AlignmentProperties(
        None if isz is None else (num(isz["mean"]), num(isz["sd"])), d.get("max_del_cigar_len"), d.get("max_ins_cigar_len"),
        None if d.get("frac_max_softclip") is None else float(d["frac_max_softclip"]), int(d["max_read_len"]), int(d.get("max_mapq", 60)),
        g, h, dict(DEFAULT_WILDTYPE_MODEL) if model is None else {int(k): num(v) for k, v in model.items()})


# ------------------------------------------------------------------------------------------------ the default record count
def chi2_1_inverse_cdf(q: float) -> float:
    """ChiSquared(1).inverse_cdf(q): x with erf(sqrt(x / 2)) = q, by bisection on the upper tail erfc (full f64 precision)."""
    tail = 1.0 - q
    lo, hi = 0.0, 1.0
    while math.erfc(math.sqrt(hi / 2.0)) > tail:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid in (lo, hi):
            break
        if math.erfc(math.sqrt(mid / 2.0)) > tail:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def default_num_records(num_alignments: Optional[int]) -> int:
    """:466-531 estimate_number_of_alignments_for_hphmm_mle_param_estimation (precision 1e-5 relative, confidence 0.1)."""
    per, precision, conf, n_valid = 100, 1e-5, 0.1, 82
    b = chi2_1_inverse_cdf(1.0 - conf / float(n_valid))
    out = []
    for p in (0.25, 1e-1, 1e-2, 1e-3, 1e-4, 1e-5):
        p_ = precision * p
        if num_alignments:
            t = float(num_alignments) * float(per)
            v = (b * t * p * (1.0 - p) / (p_ ** 2 * (t - 1.0) + b * p * (1.0 - p))) / float(per)
        else:
            v = ((b * p * (1.0 - p)) / (p_ ** 2)) / float(per)
        out.append(math.ceil(v))
    return max(out)


def _index_path(bam: str) -> Optional[str]:
    for suf in (".csi", ".bai"):          # htslib looks for a CSI first
        if os.path.exists(bam + suf):
            return bam + suf
    if bam.endswith(".bam") and os.path.exists(bam[:-4] + ".bai"):
        return bam[:-4] + ".bai"
    return None


def index_mapped(path: str) -> int:
    """Sum over the references of the mapped count in the pseudo-bin of a BAI (bin 37450) or CSI (bin (8^(depth+1) - 1) / 7 + 1)."""
    with open(path, "rb") as f:
        d = f.read()
    if d[:2] == b"\x1f\x8b":
        d = gzip.decompress(d)
    if d[:4] == b"BAI\x01":
        csi, o, meta = False, 4, 37450
    elif d[:4] == b"CSI\x01":
        _min_shift, depth, l_aux = struct.unpack_from("<iii", d, 4)
        csi, o, meta = True, 16 + l_aux, ((1 << (3 * depth + 3)) - 1) // 7 + 1
    else:
        raise AlignPropsError(f"{path}: not a BAI or CSI index")
    n_ref, = struct.unpack_from("<i", d, o)
    o += 4
    total = 0
    for _ in range(n_ref):
        n_bin, = struct.unpack_from("<i", d, o)
        o += 4
        for _ in range(n_bin):
            b, = struct.unpack_from("<I", d, o)
            o += 12 if csi else 4
            n_chunk, = struct.unpack_from("<i", d, o)
            o += 4
            if b == meta and n_chunk == 2:
                total += struct.unpack_from("<Q", d, o + 16)[0]
            o += 16 * n_chunk
        if not csi:
            n_intv, = struct.unpack_from("<i", d, o)
            o += 4 + 8 * n_intv
    return total


def num_alignments(bams: Sequence[str], required: bool) -> Optional[int]:
    """:217-231 (index_stats): the mapped counts of the files' indices; None when an index is missing and not required."""
    total = 0
    for b in bams:
        ix = _index_path(b)
        if ix is None:
            if required:
                raise AlignPropsError(f"{b}: no BAM index (.bai / .csi); it is needed without --num-records")
            return None
        total += index_mapped(ix)
    return total


# ------------------------------------------------------------------------------------------------ the command
def warnings(c: Counts, n_alignments: Optional[int], p: AlignmentProperties) -> List[str]:
    """The reference's warn! messages (:393-446)."""
    s = f"in {c.n_taken} alignments (out of {n_alignments if n_alignments is not None else 0})"
    out = []
    if p.gap_fallback or p.hop_fallback:
        out += ["Insufficient observations for hop parameter estimation, falling back to default hop parameters"] * (p.gap_fallback + p.hop_fallback)
    if p.max_del_cigar_len is None:
        out.append(f"No deletion CIGAR operations found {s}. Varlociraptor will be unable to estimate the sampling bias for deletions.")
    if p.max_ins_cigar_len is None:
        out.append(f"No insertion CIGAR operations found {s}. Varlociraptor will be unable to estimate the sampling bias for insertions.")
    if p.frac_max_softclip is None:
        out.append(f"No softclip CIGAR operations found {s}. Varlociraptor will be unable to estimate the sampling bias for larger indels.")
    if p.insert_size is None:
        out.append(
            "\nFound no records to use for estimating the insert size. Will assume\nsingle end sequencing data and calculate deletion "
            "probabilities without\nconsidering the insert size.\n\nIf your data should be paired end, please consider manually "
            "providing\n--alignment-properties, e.g. computed with `samtools stats`. Also,\nthe following counts of unusable records "
            "might indicate a source of\nthis problem:\n\n"
            f"- I, D, S or H CIGAR operation: {c.n_not_usable}\n- S CIGAR (soft clip, e.g. due to UMIs or adapters): {c.n_softclips}\n\n"
            f"In addition, {c.n_skipped} records were skipped in the estimation for one\nof the following reasons:\n"
            f"- not paired: {c.n_not_paired}\n- not the first segment with regard to the template sequence: {c.n_not_first}\n"
            "- mapping quality of 0: 0\n- marked as a duplicate: 0\n"
            f"- mate mapped to different template (e.g. different chromosome): {c.n_tid_mismatch}\n"
            "- failed some quality check according to the 512 SAM flag: 0\n"
            f"- mate unmapped: {c.n_mate_unmapped}\n- record unmapped: 0\n")
    return out


def counts(fasta: str, bams: Sequence[str], num_records: int, device="cpu") -> Counts:
    if device == "cpu":
        return count_bams(fasta, bams, num_records)
    return count_bams_device(fasta, bams, num_records, int(device))


def estimate(fasta: str, bams: Sequence[str], num_records: Optional[int] = None, device="cpu", warn=None):
    """(properties, counts) of the command.  Without num_records the indices are required (the default count needs them); with it
    they are optional (a deviation: the reference opens every BAM through its index)."""
    n_al = num_alignments(bams, required=num_records is None)
    need = default_num_records(n_al)
    if num_records is None:
        num_records = need
    elif warn is not None:
        if num_records < need:
            warn(f"Number of records ({num_records}) is smaller than the number of records needed to estimate the HPHMM's transition "
                 f"probabilities to a certain precision ({need}). This may lead to inaccurate results.")
        else:
            warn(f"Number of records ({num_records}) is larger than the number of records needed to estimate the HPHMM's transition "
                 f"probabilities to a certain precision ({need}). This may lead to unnecessarily long runtime.")
    c = counts(fasta, bams, num_records, device)
    p = finish(c)
    if warn is not None:
        for w in warnings(c, n_al, p):
            warn(w)
    return p, c


def run_cli(fasta: str, bams: Sequence[str], num_records: Optional[int], device) -> int:
    def warn(msg):
        print(f"[WARN] {msg}", file=sys.stderr)
    try:
        p, _ = estimate(fasta, bams, num_records, device=device, warn=warn)
    except AlignPropsError as e:
        print(f"error: {e}", file=sys.stderr)
        return 1
    print(to_json(p))
    return 0


# ------------------------------------------------------------------------------------------------ the device path
def count_bams_device(fasta: str, bams: Sequence[str], num_records: int, device: int, window_bytes: int = 0) -> Counts:
    """The same counts from the HIP path (vlr_bamstats_*: inflate, record split and statistics kernels on `device`)."""
    import ctypes as C
    from . import abi, engine
    L = engine.lib()
    h = C.c_void_p()
    rc = L.vlr_bamstats_open(device, fasta.encode(), C.c_int64(num_records), C.c_int64(window_bytes), C.byref(h))
    if rc != 0:
        raise AlignPropsError((L.vlr_last_error() or b"").decode())
    try:
        for b in bams:
            rc = L.vlr_bamstats_add_bam(h, b.encode())
            if rc != 0:
                raise AlignPropsError((L.vlr_last_error() or b"").decode())
        res = abi.BamStatsResult()
        rc = L.vlr_bamstats_result(h, C.byref(res))
        if rc != 0:
            raise AlignPropsError((L.vlr_last_error() or b"").decode())
        c = Counts()
        c.transitions = np.ctypeslib.as_array(res.transitions).reshape(16, 16).astype(np.int64)
        c.max_del = None if res.max_del < 0 else int(res.max_del)
        c.max_ins = None if res.max_ins < 0 else int(res.max_ins)
        c.frac_max_softclip = float(res.frac_max_softclip) if res.has_softclip else None
        c.max_read_len, c.max_mapq = int(res.max_read_len), int(res.max_mapq)
        c.n_taken, c.n_skipped, c.n_not_usable, c.n_softclips = int(res.n_taken), int(res.n_skipped), int(res.n_not_usable), int(res.n_softclips)
        c.n_not_paired, c.n_not_first, c.n_mate_unmapped, c.n_tid_mismatch = (int(res.n_not_paired), int(res.n_not_first),
                                                                               int(res.n_mate_unmapped), int(res.n_tid_mismatch))
        nk = int(res.n_hop_keys)
        keys = (C.c_uint64 * max(nk, 1))()
        vals = (C.c_uint64 * max(nk, 1))()
        ni = int(res.n_insert_sizes)
        isz = (C.c_int64 * max(ni, 1))()
        rc = L.vlr_bamstats_read(h, keys, vals, C.c_int64(nk), isz, C.c_int64(ni))
        if rc != 0:
            raise AlignPropsError((L.vlr_last_error() or b"").decode())
        for i in range(nk):
            k = int(keys[i])
            c.hops[(k >> 56, (k >> 28) & 0xFFFFFFF, k & 0xFFFFFFF)] = int(vals[i])
        c.insert_sizes = [int(isz[i]) for i in range(ni)]
        c.seconds = list(res.seconds)
        return c
    finally:
        L.vlr_bamstats_close(h)


# ------------------------------------------------------------------------------------------------ synthetic BAM writing
def bgzf_compress(data: bytes, member_bytes: int = 0xff00) -> bytes:
    """BGZF members of at most member_bytes inflated bytes each, then the EOF member (SAM spec 4.1)."""
    out = bytearray()
    for i in range(0, len(data), member_bytes):
        out += _bgzf_member(data[i:i + member_bytes])
    out += _bgzf_member(b"")
    return bytes(out)


def _bgzf_member(chunk: bytes) -> bytes:
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    cdata = co.compress(chunk) + co.flush()
    bsize = 18 + len(cdata) + 8 - 1
    assert bsize < 65536
    head = struct.pack("<BBBBIBBHBBHH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6, ord("B"), ord("C"), 2, bsize)
    return head + cdata + struct.pack("<II", zlib.crc32(chunk) & 0xffffffff, len(chunk))


def reg2bin(beg: int, end: int) -> int:
    """SAM spec 5.3 (bam_reg2bin)."""
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def aux_field(tag: str, typ: str, value) -> bytes:
    """One aux field: A c C s S i I f Z H, or B with (subtype, values)."""
    t = tag.encode() + typ.encode()
    if typ == "A":
        return t + value.encode()
    if typ in "cCsSiIf":
        return t + struct.pack("<" + {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[typ], value)
    if typ in "ZH":
        return t + value.encode() + b"\0"
    if typ == "B":
        sub, vals = value
        return t + sub.encode() + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]), *vals)
    raise ValueError(typ)


def encode_record(tid: int, pos: int, mapq: int, flag: int, cigar: Sequence[Tuple[str, int]], seq: str, mtid: int = -1, mpos: int = -1,
                  tlen: int = 0, aux: bytes = b"", name: str = "r", qual: Optional[bytes] = None) -> bytes:
    """One BAM record (block_size included); cigar as (op letter, length); qual: one byte per base (default: 0x1e throughout)."""
    rn = name.encode() + b"\0"
    cig = b"".join(struct.pack("<I", (l << 4) | CIGAR_OPS.index(op)) for op, l in cigar)
    rlen = sum(l for op, l in cigar if op in "MDN=X")
    codes = [SEQ_CODE.index(ch.upper().encode()) if ch.upper().encode() in SEQ_CODE else 15 for ch in seq]
    packed = bytearray((len(codes) + 1) // 2)
    for i, v in enumerate(codes):
        packed[i >> 1] |= v << (4 if (i & 1) == 0 else 0)
    qual = b"\x1e" * len(seq) if qual is None else bytes(qual)
    assert len(qual) == len(seq)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(rn), mapq, reg2bin(pos, pos + max(rlen, 1)), len(cigar), flag, len(seq),
                       mtid, mpos, tlen) + rn + cig + bytes(packed) + qual + aux
    return struct.pack("<I", len(body)) + body


def encode_bam(contigs: Sequence[Tuple[str, int]], records: Sequence[bytes], text: str = "") -> bytes:
    h = bytearray(b"BAM\x01") + struct.pack("<i", len(text)) + text.encode() + struct.pack("<i", len(contigs))
    for name, ln in contigs:
        nb = name.encode() + b"\0"
        h += struct.pack("<i", len(nb)) + nb + struct.pack("<i", ln)
    return bytes(h) + b"".join(records)


def write_bam(path: str, contigs: Sequence[Tuple[str, int]], records: Sequence[bytes], member_bytes: int = 0xff00) -> None:
    with open(path, "wb") as f:
        f.write(bgzf_compress(encode_bam(contigs, records), member_bytes))


def write_bai_counts(path: str, mapped: Sequence[int], unmapped: Sequence[int]) -> None:
    """A BAI holding only the pseudo-bin of each reference (mapped / unmapped counts): enough for index_stats, not for region
    queries."""
    out = bytearray(b"BAI\x01") + struct.pack("<i", len(mapped))
    for m, u in zip(mapped, unmapped):
        out += struct.pack("<iIi", 1, 37450, 2) + struct.pack("<QQQQ", 0, 0, m, u) + struct.pack("<i", 0)
    with open(path, "wb") as f:
        f.write(bytes(out))


def write_fasta(path: str, contigs: Dict[str, bytes], width: int = 60) -> None:
    """FASTA plus its .fai."""
    fai = []
    with open(path, "wb") as f:
        for name, seq in contigs.items():
            f.write(b">" + name.encode() + b"\n")
            off = f.tell()
            for i in range(0, len(seq), width):
                f.write(seq[i:i + width] + b"\n")
            fai.append(f"{name}\t{len(seq)}\t{off}\t{width}\t{width + 1}\n")
    with open(path + ".fai", "w") as f:
        f.write("".join(fai))
