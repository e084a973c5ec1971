"""SNV and MNV allele supports from BAM records: the observations of the most common variant type, scored base by base
from the read's own alignment, without realignment.  A CPU restatement of the reference's path and the front end of its HIP kernel
(csrc/vlr_basepileup.hip, vlr_basepileup_* of include/vlr.h).  Mirrors

  Snv::allele_support_per_read                variants/types/snv.rs:66-150 (the branch without realignment)
  Mnv::allele_support_per_read                variants/types/mnv.rs:73-205 (the same branch; third-allele override :163-181)
  prob_read_base and its tables               variants/evidence/bases.rs
  AlleleSupport::merge / prob_missed_allele   variants/types/mod.rs:100-160
  SingleLocus::overlap                        variants/types/mod.rs:440-473 (evidence = Enclosing, clips not considered)
  aux_tag_strand_info / contains_indel_op     utils/mod.rs:53-59, :110-120
  is_explainable_by_error_rates               variants/evidence/realignment/edit_distance.rs:31-47
  ReadEmission::error_rate                    variants/evidence/realignment/pairhmm.rs:436-451
  is_valid_record                             variants/sample.rs:281-286 (unmapped, secondary, duplicate, QC-fail dropped; supplementary kept)
  Strand::from_record_and_pos / |=            variants/evidence/observations/read_observation.rs:60-122
  candidate typing                            utils/collect_variants.rs (equal lengths: 1 = SNV, more = MNV)
  CigarStringView::read_pos                   rust-htslib, restated in readwindows.read_pos

NOT mirrored (callers must know): realignment of reads that carry an I or D operation against the SNV / MNV emission parameters —
with realign_indel_reads=True such records are not scored but handed back flagged NEEDS_REALIGN (the reference's default is to
realign them; the default here is False: every read is scored from its alignment) —, alternative variants at the locus (with them the
reference realigns every read of an MNV), `max_depth` subsampling of the pileup, the artifact-hypothesis features of fragments
(`pileup` builds locus_flags 0), and a `preprocess variants` command that writes an observation BCF.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from .readwindows import BamRecord, prob_mapping, read_bam, read_fasta, read_pos

MAX_LEN = abi.BASEPILEUP_MAX_LEN   # MNV bases the kernel scores (VLR_BASEPILEUP_MAX_LEN); longer ones go through the restatement
NEEDS_REALIGN = abi.BASEPILEUP_HIT_NEEDS_REALIGN


class ReadPosOutOfBounds(ValueError):
    """Error::ReadPosOutOfBounds: the SI tag is shorter than the read position"""


class InvalidStrandInfo(ValueError):
    """Error::InvalidStrandInfo: an SI character outside + - * ."""


def ln_one_minus_exp(p: float) -> float:
    """bio LogProb::ln_one_minus_exp"""
    if p < -0.693:
        return math.log1p(-math.exp(p))
    x = -math.expm1(p)
    return math.log(x) if x > 0.0 else -math.inf


def ln_sum_exp(ps: Sequence[float]) -> float:
    """bio LogProb::ln_sum_exp"""
    if not ps:
        return -math.inf
    imax = 0
    for i in range(1, len(ps)):
        if ps[i] > ps[imax]:
            imax = i
    pmax = ps[imax]
    if pmax == -math.inf:
        return -math.inf
    if pmax == math.inf:
        return math.inf
    s = 0.0
    for i, p in enumerate(ps):
        if i != imax:
            s += math.exp(p - pmax)
    return pmax + math.log1p(s)


@dataclass
class Tables:
    """BASEQUAL_TO_PROB_CALL / _MISCALL (bases.rs:38-53) for q = 0..255"""
    call: List[float]
    miscall: List[float]
    confusion: float = math.log(0.3333)   # PROB_CONFUSION
    any: float = math.log(0.25)           # PROB_ANY


def python_tables() -> Tables:
    miscall = [-q * math.log(10.0) / 10.0 for q in range(256)]
    return Tables([ln_one_minus_exp(m) for m in miscall], miscall)


def library_tables() -> Tables:
    """the tables the kernel scores with (vlr_basepileup_tables): a restatement run on them agrees with it bit for bit"""
    import ctypes as C
    from . import engine
    L = engine.lib()
    call, mis = (C.c_double * 256)(), (C.c_double * 256)()
    engine._check(L.vlr_basepileup_tables(call, mis))
    return Tables(list(call), list(mis))


TABLES = python_tables()
STRAND_OF_ITEM = {ord("+"): abi.STRAND_FORWARD, ord("-"): abi.STRAND_REVERSE, ord("*"): abi.STRAND_BOTH, ord("."): abi.STRAND_NONE}


def prob_read_base(read_base: int, allele_base: int, q: int, t: Tables = TABLES) -> float:
    """bases.rs:14-26 (bases as upper-case byte values)"""
    if read_base == allele_base:
        return t.call[q]
    if read_base == ord("N"):
        return t.any
    return t.miscall[q] + t.confusion


def strand_or(a: int, b: int) -> int:
    """Strand |= (read_observation.rs:112-122)"""
    if a == abi.STRAND_NONE:
        return b
    if b == abi.STRAND_NONE:
        return a
    return abi.STRAND_BOTH if a != b else a


def strand_of_item(ch: int) -> int:
    if ch not in STRAND_OF_ITEM:
        raise InvalidStrandInfo("invalid strand information %r in the SI tag" % chr(ch))
    return STRAND_OF_ITEM[ch]


def is_valid_record(flag: int) -> bool:
    """sample.rs:281-286"""
    return not flag & (0x100 | 0x400 | 0x4 | 0x200)


def contains_indel_op(rec: BamRecord) -> bool:
    return any(op in "ID" for op, _ in rec.cigar)


_AUX_FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def aux_fields(aux: bytes):
    """(tag, type, value bytes) of every aux field (SAM spec 4.2.4); ValueError when the bytes are malformed"""
    o, n = 0, len(aux)
    while o < n:
        if o + 3 > n:
            raise ValueError("malformed aux field")
        tag, ty = aux[o:o + 2], chr(aux[o + 2])
        o += 3
        if ty in _AUX_FIXED:
            nb = _AUX_FIXED[ty]
        elif ty in "ZH":
            e = aux.find(b"\0", o)
            if e < 0:
                raise ValueError("malformed aux field")
            nb = e - o + 1
        elif ty == "B":
            if o + 5 > n or chr(aux[o]) not in _AUX_FIXED or chr(aux[o]) == "A":
                raise ValueError("malformed aux field")
            nb = 5 + _AUX_FIXED[chr(aux[o])] * struct.unpack_from("<I", aux, o + 1)[0]
        else:
            raise ValueError("malformed aux field")
        if o + nb > n:
            raise ValueError("malformed aux field")
        yield tag, ty, aux[o:o + nb]
        o += nb


def aux_tag_strand_info(rec: BamRecord) -> Optional[bytes]:
    """utils/mod.rs:53-59: the SI tag when it is a string"""
    for tag, ty, val in aux_fields(rec.aux):
        if tag == b"SI":
            return val[:-1] if ty == "Z" else None
    return None


def leading_hardclips(rec: BamRecord) -> int:
    return rec.cigar[0][1] if rec.cigar and rec.cigar[0][0] == "H" else 0


@dataclass
class Locus:
    kind: int            # abi.BASEPILEUP_SNV / _MNV
    ref_id: int          # index of the contig in the BAM header
    start: int           # 0-based
    ref: bytes
    alt: bytes

    @property
    def end(self) -> int:
        return self.start + len(self.ref)


def locus(ref_seq: bytes, ref_id: int, pos: int, ref: bytes, alt: bytes) -> Locus:
    """The SNV / MNV candidate `ref` > `alt` at 0-based `pos` of the contig sequence `ref_seq` (utils/collect_variants.rs)."""
    ref, alt = bytes(ref).upper(), bytes(alt).upper()
    if alt.startswith(b"<") or b"[" in alt or b"]" in alt or alt in (b"*", b"."):
        raise ValueError("symbolic ALT allele %r is neither an SNV nor an MNV" % alt)
    if len(ref) != len(alt) or not ref:
        raise ValueError("REF and ALT of different lengths are not an SNV or MNV (readwindows.indel_locus handles them)")
    if ref_seq[pos:pos + len(ref)].upper() != ref:
        raise ValueError("REF allele does not match the reference sequence at position %d" % (pos + 1))
    return Locus(abi.BASEPILEUP_SNV if len(ref) == 1 else abi.BASEPILEUP_MNV, ref_id, pos, ref, alt)


@dataclass
class Hit:
    """one (record, locus) allele support; after merge_mates one fragment"""
    locus: int
    record: int                      # ordinal of the record in the file (the first one of a merged fragment)
    prob_ref: float
    prob_alt: float
    strand: int                      # abi.STRAND_*
    read_position: Optional[int]
    third_allele: int                # evidence (edit distance), 0 = none
    mapq: int
    flag: int                        # FLAG & (0x1 | 0x10 | 0x40)
    status: int = 0                  # NEEDS_REALIGN
    records: Tuple[int, ...] = ()

    def key(self):
        return (self.locus, self.record, self.prob_ref, self.prob_alt, self.strand, self.read_position, self.third_allele, self.mapq, self.flag, self.status)


def enclosing(rec: BamRecord, loc: Locus) -> bool:
    """SingleLocus::overlap(read, false, 0, 0) == Enclosing"""
    return rec.pos >= 0 and rec.pos <= loc.start and rec.end_pos() >= loc.end


def allele_support(rec: BamRecord, loc: Locus, li: int = 0, ordinal: int = 0, t: Tables = TABLES, realign_indel_reads: bool = False) -> Optional[Hit]:
    """Snv / Mnv::allele_support_per_read of a valid record; None = no observation."""
    if not enclosing(rec, loc):
        return None
    hit = Hit(li, ordinal, 0.0, 0.0, abi.STRAND_NONE, None, 0, rec.mapq, rec.flag & (0x1 | 0x10 | 0x40), 0, (ordinal,))
    if realign_indel_reads and contains_indel_op(rec):
        hit.status = NEEDS_REALIGN
        return hit
    rec_strand = abi.STRAND_REVERSE if rec.flag & 0x10 else abi.STRAND_FORWARD
    si = aux_tag_strand_info(rec)
    if loc.kind == abi.BASEPILEUP_SNV:
        qpos = read_pos(rec, loc.start, False, False)
        if qpos is None:
            return None
        rb, q, alt, ref = rec.seq[qpos], rec.qual[qpos], loc.alt[0], loc.ref[0]
        pa = prob_read_base(rb, alt, q, t)
        non_alt, third = ref, False
        if rb != ord("N") and rb != alt:
            third = rb != ref
            non_alt = rb
        pr = prob_read_base(rb, non_alt, q, t)
        hit.prob_ref, hit.prob_alt = pr, pa
        hit.read_position = qpos + leading_hardclips(rec)
        hit.third_allele = 1 if third else 0
        if pr != pa:
            if si is not None:
                if qpos >= len(si):
                    raise ReadPosOutOfBounds("read position %d outside the SI tag of %s" % (qpos, rec.qname))
                hit.strand = strand_of_item(si[qpos])
            else:
                hit.strand = rec_strand
        return hit
    pr = pa = pt = 0.0
    strand, dist = abi.STRAND_NONE, 0
    for b in range(len(loc.ref)):
        qpos = read_pos(rec, loc.start + b, False, False)
        if qpos is None:
            return None
        if b == 0:
            hit.read_position = qpos + leading_hardclips(rec)
        rb, q, alt, ref = rec.seq[qpos], rec.qual[qpos], loc.alt[b], loc.ref[b]
        if rb != ord("N") and rb != alt:
            dist += 1
        ba, br, bt = prob_read_base(rb, alt, q, t), prob_read_base(rb, ref, q, t), prob_read_base(rb, rb, q, t)
        if ba != br and si is not None:
            if qpos >= len(si):
                raise ReadPosOutOfBounds("read position %d outside the SI tag of %s" % (qpos, rec.qname))
            strand = strand_or(strand, strand_of_item(si[qpos]))
        pr += br
        pa += ba
        pt += bt
    if pa > pr and dist > 0 and not explainable(dist, len(loc.ref), rec.qual, t):
        pr = pt
        hit.third_allele = dist
    if si is None and pr != pa:
        strand = rec_strand
    hit.prob_ref, hit.prob_alt, hit.strand = pr, pa, strand
    return hit


def error_rate(qual: bytes, t: Tables = TABLES) -> float:
    """ReadEmission::error_rate (pairhmm.rs:436-451): ln of the mean miscall probability over the whole read"""
    return ln_sum_exp([t.miscall[q] for q in qual]) - math.log(len(qual))


def expected_substitutions(length: int, qual: bytes, t: Tables = TABLES) -> float:
    return length * math.exp(error_rate(qual, t))


def explainable(dist: int, length: int, qual: bytes, t: Tables = TABLES) -> bool:
    """is_explainable_by_error_rates (edit_distance.rs:31-47) with no insertions or deletions (their terms are 0 <= x)"""
    return dist <= expected_substitutions(length, qual, t)


@dataclass
class Scored:
    hits: List[Hit]                  # locus-major, record order within a locus
    needs_realign: List[Hit]         # the same order; status NEEDS_REALIGN
    n_records: int = 0
    n_rejected: int = 0
    bad_records: List[int] = field(default_factory=list)


def record_is_bad(rec: BamRecord) -> bool:
    """what the kernel refuses beyond a record that does not parse: a CIGAR that consumes more bases than SEQ has, malformed aux fields"""
    if sum(l for op, l in rec.cigar if op in "MIS=X") > len(rec.seq):
        return True
    try:
        for _ in aux_fields(rec.aux):
            pass
    except ValueError:
        return True
    return False


def score_records(records: Sequence[BamRecord], loci: Sequence[Locus], t: Tables = TABLES, realign_indel_reads: bool = False, first_ordinal: int = 0) -> Scored:
    """Every (record, locus) support of `records` (in file order) for `loci` (sorted by (ref_id, start))."""
    import bisect
    keys = [(l.ref_id, l.start) for l in loci]
    assert keys == sorted(keys), "loci must be sorted by (ref_id, start)"
    per_locus: List[List[Hit]] = [[] for _ in loci]
    out = Scored([], [], len(records))
    for k, rec in enumerate(records):
        if not is_valid_record(rec.flag):
            out.n_rejected += 1
            continue
        if record_is_bad(rec):
            out.bad_records.append(first_ordinal + k)
            continue
        if rec.ref_id < 0 or rec.pos < 0:
            continue
        end = rec.end_pos()
        li = bisect.bisect_left(keys, (rec.ref_id, rec.pos))
        while li < len(loci) and loci[li].ref_id == rec.ref_id and loci[li].start < end:
            h = allele_support(rec, loci[li], li, first_ordinal + k, t, realign_indel_reads)
            if h is not None:
                per_locus[li].append(h)
            li += 1
    for hs in per_locus:
        for h in hs:
            (out.needs_realign if h.status & NEEDS_REALIGN else out.hits).append(h)
    return out


def _is_alt_support(h: Hit) -> bool:
    return h.prob_alt > h.prob_ref


def merge(a: Hit, b: Hit) -> Hit:
    """AlleleSupport::merge (types/mod.rs:104-160): `b` merged into `a`"""
    pos = a.read_position
    if _is_alt_support(a):
        if _is_alt_support(b) and a.read_position != b.read_position:
            pos = None
    elif _is_alt_support(b):
        pos = b.read_position
    if a.strand == abi.STRAND_NONE:
        strand = b.strand
    elif b.strand != abi.STRAND_NONE and a.strand != b.strand:
        strand = abi.STRAND_BOTH
    else:
        strand = a.strand
    # EditDistance::update adds the two distances
    return Hit(a.locus, a.record, a.prob_ref + b.prob_ref, a.prob_alt + b.prob_alt, strand, pos, a.third_allele + b.third_allele, a.mapq, a.flag,
               a.status | b.status, a.records + b.records)


def merge_mates(hits: Sequence[Hit], qnames: Sequence[str]) -> List[Hit]:
    """Fragments from the supports of one locus: records that share a QNAME are merged left then right, in record order; the
    fragments come in the order of their first record."""
    order: List[str] = []
    by_name: Dict[str, Hit] = {}
    for h, q in zip(hits, qnames):
        if q in by_name:
            by_name[q] = merge(by_name[q], h)
        else:
            by_name[q] = Hit(h.locus, h.record, h.prob_ref, h.prob_alt, h.strand, h.read_position, h.third_allele, h.mapq, h.flag, h.status, h.records or (h.record,))
            order.append(q)
    return [by_name[q] for q in order]


_merge_mates = merge_mates   # (allele_supports has a parameter of the same name)


@dataclass
class Supports:
    """the observations of one candidate, one per fragment"""
    prob_alt: np.ndarray
    prob_ref: np.ndarray
    strand: np.ndarray           # abi.STRAND_*
    read_position: np.ndarray    # int64, -1 = none
    third_allele: np.ndarray     # evidence, 0 = none
    mapq: np.ndarray
    paired: np.ndarray           # bool
    read_len: np.ndarray         # bases of the (first) record
    records: List[Tuple[int, ...]]
    needs_realign: List[int]     # ordinals of the records left to a realigner (realign_indel_reads=True)

    def __len__(self):
        return len(self.prob_alt)


def _supports(hits: Sequence[Hit], read_len: Dict[int, int], needs: Sequence[Hit]) -> Supports:
    return Supports(np.array([h.prob_alt for h in hits], float), np.array([h.prob_ref for h in hits], float), np.array([h.strand for h in hits], np.uint8),
                    np.array([-1 if h.read_position is None else h.read_position for h in hits], np.int64),
                    np.array([h.third_allele for h in hits], np.uint32), np.array([h.mapq for h in hits], np.uint8),
                    np.array([bool(h.flag & 0x1) for h in hits], bool), np.array([read_len[h.record] for h in hits], np.int64),
                    [h.records or (h.record,) for h in hits], [h.record for h in needs])


def record_heads(bam: str, ordinals: Sequence[int]) -> Dict[int, Tuple[str, int]]:
    """{ordinal: (QNAME, l_seq)} of the given records, read from the inflated file by walking the block sizes"""
    from . import alignprops
    want = set(int(o) for o in ordinals)
    out: Dict[int, Tuple[str, int]] = {}
    if not want:
        return out
    d = alignprops.inflate_bgzf(bam)
    _, o = alignprops.bam_header(d, bam)
    k, last = 0, max(want)
    while o + 36 <= len(d) and k <= last:
        bs, = struct.unpack_from("<I", d, o)
        if k in want:
            l_rn = d[o + 12]
            l_seq, = struct.unpack_from("<i", d, o + 20)
            out[k] = (bytes(d[o + 36:o + 36 + l_rn - 1]).decode(), l_seq)
        o += 4 + bs
        k += 1
    return out


class BasePileupError(ValueError):
    pass


def locus_arrays(loci: Sequence[Locus]):
    """(ref_id, start, length, kind, ref bases, alt bases) of `loci` as the open calls of the SNV / MNV sessions take them"""
    def bases(attr):
        return np.frombuffer(b"".join(getattr(l, attr) for l in loci) or b"\0", np.uint8).copy()
    return (np.array([l.ref_id for l in loci], np.int32), np.array([l.start for l in loci], np.int64), np.array([len(l.ref) for l in loci], np.int32),
            np.array([l.kind for l in loci], np.uint8), bases("ref"), bases("alt"))


def device_hits(bam: str, loci: Sequence[Locus], device: int = 0, realign_indel_reads: bool = False, hit_capacity: Optional[int] = None,
                window_bytes: int = 0, retry: bool = True):
    """(hits as a numpy array of abi.BASEPILEUP_HIT_DTYPE, locus-major; abi.BasePileupCounts) from the kernel.  `loci` sorted by
    (ref_id, start), MNVs of at most MAX_LEN bases.  An overflow of `hit_capacity` is retried once with the needed capacity unless
    retry=False (then the counts carry BASEPILEUP_OVERFLOW and the array is empty)."""
    import ctypes as C
    from . import engine
    L = engine.lib()
    n = len(loci)
    ref_id, start, length, kind, refb, altb = locus_arrays(loci)
    cap = int(hit_capacity) if hit_capacity is not None else max(1 << 16, 64 * n)
    while True:
        h = C.c_void_p()
        engine._check(L.vlr_basepileup_open(int(device), n, ref_id.ctypes.data, start.ctypes.data, length.ctypes.data, kind.ctypes.data, refb.ctypes.data,
                                            altb.ctypes.data, int(bool(realign_indel_reads)), cap, int(window_bytes), C.byref(h)))
        try:
            engine._check(L.vlr_basepileup_add_bam(h, bam.encode()))
            res = abi.BasePileupCounts()
            engine._check(L.vlr_basepileup_result(h, C.byref(res)))
            if res.status & abi.BASEPILEUP_GUARD_DAMAGED:
                raise BasePileupError("the guard words behind the hit buffer changed")
            if res.status & abi.BASEPILEUP_OVERFLOW and retry:
                cap = int(res.needed_capacity)
                retry = False
                continue
            hits = np.zeros(int(res.n_hits), abi.BASEPILEUP_HIT_DTYPE)
            engine._check(L.vlr_basepileup_read(h, hits.ctypes.data, int(res.n_hits)))
            return hits, res
        finally:
            L.vlr_basepileup_close(h)


def hits_from_array(a: np.ndarray) -> List[Hit]:
    """device hits as Hit objects; raises what the reference raises for a hit that carries an error status"""
    out = []
    for r in a:
        st = int(r["status"])
        if st & abi.BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS:
            raise ReadPosOutOfBounds("read position outside the SI tag of record %d" % int(r["record"]))
        if st & abi.BASEPILEUP_HIT_INVALID_STRAND_INFO:
            raise InvalidStrandInfo("invalid strand information in the SI tag of record %d" % int(r["record"]))
        if st & abi.BASEPILEUP_HIT_LEADING_REFSKIP:
            raise ValueError("leading reference skip")
        rp = int(r["read_position"])
        out.append(Hit(int(r["locus"]), int(r["record"]), float(r["prob_ref"]), float(r["prob_alt"]), int(r["strand"]),
                       None if rp == abi.BASEPILEUP_NO_READ_POSITION else rp, int(r["third_allele"]), int(r["mapq"]), int(r["flag"]), st, (int(r["record"]),)))
    return out


def allele_supports(bam: str, fasta: str, candidates: Sequence[Tuple[str, int, bytes, bytes]], device=0, realign_indel_reads: bool = False,
                    merge_mates: bool = True, window_bytes: int = 0) -> List[Supports]:
    """Per candidate (contig, 0-based position, REF, ALT), in the order given, one observation per fragment.  device="cpu": the
    restatement; a device number: the kernel (mates merged on the host; MNVs longer than MAX_LEN through the restatement on the
    library's tables)."""
    from . import alignprops
    seqs = read_fasta(fasta)
    contigs, _ = alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)
    tid = {name: k for k, (name, _) in enumerate(contigs)}
    loci = []
    for c, pos, ref, alt in candidates:
        if c not in tid or c not in seqs:
            raise ValueError("contig %s is not in the BAM header and the reference" % c)
        loci.append(locus(seqs[c], tid[c], int(pos), ref, alt))
    order = sorted(range(len(loci)), key=lambda k: (loci[k].ref_id, loci[k].start))
    per: List[Tuple[List[Hit], List[Hit]]] = [([], []) for _ in loci]
    recs = None
    if device == "cpu":
        _, recs = read_bam(bam)
        sc = score_records(recs, [loci[k] for k in order], TABLES, realign_indel_reads)
        if sc.bad_records:
            raise BasePileupError("%s: record %d is malformed" % (bam, sc.bad_records[0]))
        for h in sc.hits:
            per[order[h.locus]][0].append(h)
        for h in sc.needs_realign:
            per[order[h.locus]][1].append(h)
    else:
        short = [k for k in order if len(loci[k].ref) <= MAX_LEN]
        long_ = [k for k in order if len(loci[k].ref) > MAX_LEN]
        arr, res = device_hits(bam, [loci[k] for k in short], int(device), realign_indel_reads, window_bytes=window_bytes)
        if res.status & abi.BASEPILEUP_BAD_RECORD:
            raise BasePileupError("%s: record %d is malformed" % (bam, int(res.first_bad_record)))
        for h in hits_from_array(arr):
            per[short[h.locus]][1 if h.status & NEEDS_REALIGN else 0].append(h)
        if long_:
            _, recs = read_bam(bam)
            sc = score_records(recs, [loci[k] for k in long_], library_tables(), realign_indel_reads)
            for h in sc.hits:
                per[long_[h.locus]][0].append(h)
            for h in sc.needs_realign:
                per[long_[h.locus]][1].append(h)
    if recs is not None:
        heads = {k: (r.qname, len(r.seq)) for k, r in enumerate(recs)}
    else:
        heads = record_heads(bam, [h.record for hs, _ in per for h in hs])
    out = []
    for hs, needs in per:
        if merge_mates:
            hs = _merge_mates(hs, [heads[h.record][0] for h in hs])
        out.append(_supports(hs, {h.record: heads[h.record][1] for h in hs}, needs))
    return out


PROB_05 = math.log(0.5)


def pileup(supports: Sequence[Supports], candidates: Sequence[Tuple[str, int, bytes, bytes]]):
    """The supports of `candidates` as a single-sample PileupBatch for the engine: prob_mapping from MAPQ, prob_missed_allele per
    types/mod.rs:100-102, certain sampling (prob_sample_alt = ln 1: snv.rs:244, mnv.rs:300), no double-overlap term, uniform hit
    probability over the read, and no artifact hypotheses (locus_flags 0: the features of a fragment they need are not built here)."""
    from .batch import PileupBatch
    off = np.zeros(len(supports) + 1, np.int64)
    cols = {k: [] for k in ("prob_mapping", "prob_alt", "prob_ref", "prob_missed_allele", "prob_sample_alt", "prob_double_overlap", "prob_hit_base", "flags")}
    for k, s in enumerate(supports):
        n = len(s)
        off[k + 1] = off[k] + n
        pa, pr = s.prob_alt.copy(), s.prob_ref.copy()
        both = np.isneginf(pa) & np.isneginf(pr)      # AlleleSupport::both_alleles_impossible
        pa[both] = PROB_05
        pr[both] = PROB_05
        cols["prob_mapping"].append(np.array([prob_mapping(int(m)) for m in s.mapq], float))
        cols["prob_alt"].append(pa)
        cols["prob_ref"].append(pr)
        cols["prob_missed_allele"].append(np.logaddexp(pa, pr) - math.log(2.0))
        cols["prob_sample_alt"].append(np.zeros(n))
        cols["prob_double_overlap"].append(np.full(n, -np.inf))
        cols["prob_hit_base"].append(-np.log(np.maximum(s.read_len, 1).astype(float)))
        top = int(s.mapq.max()) if n else 0
        cols["flags"].append(abi.pack_flags(s.strand, np.full(n, abi.ORIENT_NONE), np.zeros(n, bool), np.zeros(n, bool), s.paired, s.mapq == top,
                                            np.full(n, abi.ALTLOCUS_NONE)))
    cat = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}
    loc = {"locus_flags": np.zeros(len(supports), np.uint8),
           "variant_type": np.array([abi.VT_SNV if len(c[2]) == 1 else abi.VT_MNV for c in candidates], np.uint8),
           "ref_base": np.array([bytes(c[2]).upper()[0] for c in candidates], np.uint8),
           "alt_base": np.array([bytes(c[3]).upper()[0] for c in candidates], np.uint8)}
    return PileupBatch(1, off.astype(np.uint32), {k: (np.asarray(v, np.float32) if k != "flags" else np.asarray(v, np.uint32)) for k, v in cat.items()}, loc)
