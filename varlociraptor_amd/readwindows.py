"""Read windows and allele windows from BAM records (the "next" row: the pair-HMM kernels fed with BAM-derived pairs).

Host side of `varlociraptor preprocess variants` for indel-like candidates, as far as the realignment needs it: which records are
evidence for a candidate, which window of a read is realigned, against which windows of the reference and of the alt allele, and the
per-read supports that come out of the edit-distance and pair-HMM kernels (`realign.best_hits`, `realign.prob_related`,
`realign.prob_related_homopolymer` — there is no CPU path).  Mirrors

  rust-htslib `CigarStringView::read_pos(ref_pos, include_softclips, include_dels)`   (third-party; semantics as documented there:
        leading soft clips shift the alignment start when they are included, a position inside a deletion projects to the read
        position at which the deletion starts, hard clips and pads consume nothing)
  Realigner::candidate_region                 realignment/mod.rs:58-153
  Realigner::ref_window / max_window          realignment/mod.rs:149-158 (ref window = 1.5 x realignment window)
  SingleLocus::overlap (enclosing / some)     variants/types/mod.rs (used by {Deletion,Insertion,Replacement}::is_valid_evidence)
  candidate classification                    utils/collect_variants.rs:274-300 (deletion / insertion with a one-base anchor, anything
                                              else of unequal lengths a replacement)
  alt allele windows                          types/deletion.rs:117-137, types/insertion.rs:92-113, types/replacement.rs:73-103
  Realigner::allele_support (single locus)    realignment/mod.rs:161-424: edit-distance hit -> banded pair HMM -> normalisation

NOT mirrored (callers must know): fragments — a read pair is two single-end observations here, without mate merging and the
insert-size support of deletion.rs:232-258 —, alternative variants at the locus (`alt_variants`), the read-inferred third allele
(mod.rs:311-349), merged multi-locus regions (mod.rs:201-240), `homopolymer_indel_len`, SI:Z strand information over an interval,
`prob_sample_alt`.  `evidence` / `device_supports` (the device path: csrc/vlr_indelpileup.hip, vlr_indelpileup_* of include/vlr.h) take
the reference's record filter and keep no-overlap reads; `evidence_windows` keeps its older filter.
SNVs / MNVs are scored base by base in the reference, without realignment: that path is varlociraptor_amd/basecalls.py.  A minimal
BAM / FASTA reader is included (BGZF members are gzip members): the reference reads through htslib.
"""
from __future__ import annotations

import gzip
import math
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

MAX_PATTERN_LEN = 128   # edit_distance.rs:145-147
SEQ_CODE = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"


@dataclass
class BamRecord:
    qname: str
    flag: int
    ref_id: int
    pos: int          # 0-based leftmost
    mapq: int
    cigar: List[Tuple[str, int]]
    seq: bytes
    qual: bytes
    mate_ref_id: int
    mate_pos: int
    tlen: int
    aux: bytes = b""  # the raw aux fields behind the qualities
    raw_name: Optional[bytes] = None  # the QNAME's bytes as the record holds them (read_bam)

    @property
    def reverse(self) -> bool:
        return bool(self.flag & 0x10)

    @property
    def unmapped(self) -> bool:
        return bool(self.flag & 0x4)

    def end_pos(self) -> int:
        """exclusive reference end of the alignment (CigarStringView::end_pos)"""
        return self.pos + sum(l for op, l in self.cigar if op in "MDN=X")


def read_bam(path: str) -> Tuple[List[Tuple[str, int]], List[BamRecord]]:
    """(contigs, records) of a BAM file (SAM spec §4.2)."""
    d = gzip.open(path).read()
    assert d[:4] == b"BAM\x01"
    l_text, = struct.unpack_from("<i", d, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", d, o)
    o += 4
    contigs = []
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", d, o)
        name = d[o + 4:o + 4 + l_name - 1].decode()
        l_ref, = struct.unpack_from("<i", d, o + 4 + l_name)
        contigs.append((name, l_ref))
        o += 8 + l_name
    recs = []
    while o < len(d):
        block_size, = struct.unpack_from("<i", d, o)
        ref_id, pos, l_read_name, mapq, _bin, n_cigar, flag, l_seq, mate_ref, mate_pos, tlen = struct.unpack_from("<iiBBHHHiiii", d, o + 4)
        p = o + 36
        raw_name = bytes(d[p:p + l_read_name - 1])
        qname = raw_name.decode("utf-8", "replace")
        p += l_read_name
        cigar = []
        for k in range(n_cigar):
            v, = struct.unpack_from("<I", d, p + 4 * k)
            cigar.append((CIGAR_OPS[v & 0xf], v >> 4))
        p += 4 * n_cigar
        packed = d[p:p + (l_seq + 1) // 2]
        seq = bytearray(l_seq)
        for i in range(l_seq):
            b = packed[i >> 1]
            seq[i] = ord(SEQ_CODE[(b >> 4) if (i & 1) == 0 else (b & 0xf)])
        p += (l_seq + 1) // 2
        qual = d[p:p + l_seq]
        recs.append(BamRecord(qname, flag, ref_id, pos, mapq, cigar, bytes(seq), bytes(qual), mate_ref, mate_pos, tlen, bytes(d[p + l_seq:o + 4 + block_size]), raw_name))
        o += 4 + block_size
    return contigs, recs


def read_fasta(path: str) -> Dict[str, bytes]:
    out: Dict[str, bytearray] = {}
    name = None
    for line in open(path):
        line = line.strip()
        if line.startswith(">"):
            name = line[1:].split()[0]
            out[name] = bytearray()
        elif name is not None:
            out[name] += line.encode()
    return {k: bytes(v) for k, v in out.items()}


def read_pos(rec: BamRecord, ref_pos: int, include_softclips: bool, include_dels: bool) -> Optional[int]:
    """rust-htslib CigarStringView::read_pos."""
    cig = rec.cigar
    rpos, qpos, j = rec.pos, 0, 0
    for i, (op, l) in enumerate(cig):
        if op in "M=XI":
            j = i
            break
        if op == "S":
            j = i
            if include_softclips:
                rpos = max(0, rpos - l)
            break
        if op == "D":
            rpos += l
        elif op == "N":
            raise ValueError("leading reference skip")
        elif op in "HP":
            if i == len(cig) - 1:
                return None
    while rpos <= ref_pos and j < len(cig):
        op, l = cig[j]
        inside = rpos <= ref_pos < rpos + l
        if op in "M=X" and inside:
            return qpos + (ref_pos - rpos)
        if op == "S" and include_softclips and inside:
            return qpos + (ref_pos - rpos)
        if op == "D" and include_dels and inside:
            return qpos
        if op in "M=X":
            rpos += l; qpos += l
        elif op == "S":
            qpos += l
            if include_softclips:
                rpos += l
        elif op == "I":
            qpos += l
        elif op in "DN":
            rpos += l
        elif op == "H" and j == len(cig) - 1:
            return None
        j += 1
    return None


def overlaps(rec: BamRecord, start: int, end: int) -> bool:
    """the alignment (with soft clips) shares at least one position with [start, end): SingleLocus::overlap(read, true, ..) != None"""
    lead = rec.cigar[0][1] if rec.cigar and rec.cigar[0][0] == "S" else 0
    trail = rec.cigar[-1][1] if len(rec.cigar) > 1 and rec.cigar[-1][0] == "S" else 0
    return rec.pos - lead < end and rec.end_pos() + trail > start


@dataclass
class CandidateRegion:
    overlap: bool
    read_interval: Tuple[int, int]
    ref_interval: Tuple[int, int]


def candidate_region(rec: BamRecord, locus_start: int, locus_end: int, ref_len: int, window: int = 64) -> CandidateRegion:
    """Realigner::candidate_region (realignment/mod.rs:58-153); `window` = --realignment-window (max_window), ref window = 1.5 x."""
    ref_window = int(window * 1.5)
    seq_len = len(rec.seq)

    def ref_interval(bp: int) -> Tuple[int, int]:
        return max(0, bp - ref_window), min(bp + ref_window, ref_len)

    qs, qe = read_pos(rec, locus_start, True, True), read_pos(rec, locus_end, True, True)
    if qs is not None and qe is not None:
        max_window = max(0, window - (qe - qs) // 2)
        ro, re_ = max(0, qs - max_window), min(qe + max_window, seq_len)
        exceed = max(0, (re_ - ro) - MAX_PATTERN_LEN)
        if exceed > 0:
            ro += exceed // 2
            re_ -= int(math.ceil(exceed / 2.0))
        return CandidateRegion(True, (ro, re_), ref_interval(locus_start))
    if qs is not None:
        return CandidateRegion(True, (max(0, qs - window), min(qs + window, seq_len)), ref_interval(locus_start))
    if qe is not None:
        return CandidateRegion(True, (max(0, qe - window), min(qe + window, seq_len)), ref_interval(locus_end))
    m = seq_len // 2
    enclosed = rec.pos >= locus_start and rec.end_pos() <= locus_end
    return CandidateRegion(enclosed, (max(0, m - window), min(m + window - 1, seq_len)), ref_interval(rec.pos + m))


def prob_mapping(mapq: int) -> float:
    """ln(1 - 10^(-MAPQ/10)) (read_observation.rs:620-640; MAPQ 0 -> ln 0)"""
    p = 1.0 - 10.0 ** (-mapq / 10.0)
    return math.log(p) if p > 0.0 else -math.inf


@dataclass
class IndelLocus:
    kind: str                 # "deletion" | "insertion" | "replacement"
    start: int                # locus start (0-based; the anchor base of a deletion / insertion)
    end: int                  # locus end (exclusive)
    len_diff: int             # alt length - ref length
    alt_allele: bytes         # the alt allele window (independent of the read)


def indel_locus(ref_seq: bytes, pos: int, ref: bytes, alt: bytes, window: int = 64) -> IndelLocus:
    """Locus and alt allele window of the candidate `ref` > `alt` at 0-based `pos` of the contig sequence `ref_seq`."""
    from . import realign
    ref, alt = bytes(ref).upper(), bytes(alt).upper()
    if ref_seq[pos:pos + len(ref)].upper() != ref:
        raise ValueError("REF allele does not match the reference sequence at position %d" % (pos + 1))
    if len(ref) == len(alt):
        raise ValueError("SNVs and MNVs are not realigned (types/snv.rs, types/mnv.rs)")
    ref_window = int(window * 1.5)
    n = len(ref_seq)
    if len(alt) == 1 and ref[:1] == alt:
        # Deletion::new: locus = start..end, deleted bases start+1..end (deletion.rs:41-49); alt window deletion.rs:117-137
        dl = len(ref) - 1
        return IndelLocus("deletion", pos, pos + dl, -dl, realign.deletion_allele(ref_seq, max(0, pos - ref_window), min(pos + ref_window, n - dl), pos, dl))
    if len(ref) == 1 and alt[:1] == ref:
        # Insertion::new: locus = start..start+1; alt window insertion.rs:92-113
        ins = alt[1:]
        return IndelLocus("insertion", pos, pos + 1, len(ins), realign.insertion_allele(ref_seq, max(0, pos - ref_window), min(pos + len(ins) + ref_window, n), pos, ins))
    # Replacement::new: locus = the REF allele's interval; alt window replacement.rs:73-103
    return IndelLocus("replacement", pos, pos + len(ref), len(alt) - len(ref),
                      realign.replacement_allele(ref_seq, max(0, pos - ref_window), min(pos + len(ref) + ref_window, n), pos, len(ref), alt))


def substitution_locus(ref_seq: bytes, pos: int, ref: bytes, alt: bytes, window: int = 64) -> IndelLocus:
    """Locus and alt allele window of the SNV / MNV candidate `ref` > `alt` (equal lengths) at 0-based `pos`, for the realignment of
    indel-bearing reads (snv.rs:157-178, mnv.rs:224-233: Snv / MnvEmissionParams): the contig over [max(0, pos - rw), min(pos + len + rw,
    n)), rw = int(window * 1.5), with the locus bytes replaced — realign.replacement_allele with len(alt) == len(ref)."""
    from . import realign
    ref, alt = bytes(ref).upper(), bytes(alt).upper()
    if len(ref) != len(alt) or not ref:
        raise ValueError("REF and ALT of different lengths are not an SNV or MNV (indel_locus handles them)")
    if ref_seq[pos:pos + len(ref)].upper() != ref:
        raise ValueError("REF allele does not match the reference sequence at position %d" % (pos + 1))
    rw_, n = int(window * 1.5), len(ref_seq)
    return IndelLocus("substitution", pos, pos + len(ref), 0,
                      realign.replacement_allele(ref_seq, max(0, pos - rw_), min(pos + len(ref) + rw_, n), pos, len(ref), alt))


def evidence_windows(records: List[BamRecord], ref_seq: bytes, locus: IndelLocus, window: int = 64) -> list:
    """(record, read window, qualities, ref allele window) of every record that is valid evidence for the locus (mapped, primary,
    overlapping it with its soft clips, with a candidate region)."""
    from . import realign
    out = []
    n = len(ref_seq)
    for r in records:
        if r.unmapped or r.flag & 0x900 or not overlaps(r, locus.start, locus.end):   # (secondary / supplementary records carry no evidence)
            continue
        reg = candidate_region(r, locus.start, locus.end, n, window)
        if not reg.overlap:
            continue
        ro, re_ = reg.read_interval
        if re_ - ro < 1:
            continue
        out.append((r, r.seq[ro:re_].upper(), list(r.qual[ro:re_]), realign.ref_allele(ref_seq, *reg.ref_interval)))
    return out


def pair_batch(reads: list, alt_allele: bytes):
    """(ref allele, read), (alt allele, read) per read as a realign.PairBatch, bands unset"""
    from .realign import PairBatch
    pb = PairBatch()
    for r, seq, qual, ref_allele in reads:
        pb.add(ref_allele, seq, qual, -1)
        pb.add(alt_allele, seq, qual, -1)
    return pb


def allele_supports(reads: list, alt_allele: bytes, gap=None, hop=None, device: int = 0):
    """(ln P(read | alt), ln P(read | ref)) per read, normalised (Realigner::allele_support, mod.rs:161-424, one locus, no
    alternative variants): the edit-distance kernel bands every pair (best hit + EDIT_BAND, pairhmm.rs:20), the pair-HMM kernel scores
    it — `hop` (realign.HopParams) selects the homopolymer mode —, mod.rs:359-385 normalises.  Returns (prob_alt, prob_ref, PairBatch)."""
    import numpy as np
    from . import realign
    pb = pair_batch(reads, alt_allele)
    dist, _, _ = realign.best_hits(pb, device)
    pb.band = [int(x) + realign.EDIT_BAND if x >= 0 else -1 for x in dist]
    lnp = realign.prob_related_homopolymer(pb, gap, hop, device) if hop is not None else realign.prob_related(pb, gap, device)
    n = len(reads)
    pa, pr = np.empty(n), np.empty(n)
    for k in range(n):
        pr[k], pa[k] = realign.normalize_support(float(lnp[2 * k]), float(lnp[2 * k + 1]))
    return pa, pr, pb


# ---------------------------------------------------------------------------------------------- the device path (vlr_indelpileup_*)
NO_OVERLAP, LEADING_REFSKIP = 1, 2     # Evidence.status / the status byte of a vlr_indelpileup_hit (abi.INDELPILEUP_HIT_*)
MODES = {"exact": 0, "fast": 1, "homopolymer": 2}


@dataclass
class Evidence:
    """One (record, locus) pair the realignment sees.  status 0: the windows to realign; NO_OVERLAP: the candidate region does not
    overlap (supports ln 0.5 / ln 0.5, mod.rs:186-199); LEADING_REFSKIP: read_pos fails on a CIGAR that begins with N.  A status other
    than 0 comes with empty windows and intervals."""
    record: int                        # ordinal of the record
    status: int
    read_interval: Tuple[int, int]
    ref_interval: Tuple[int, int]
    read_window: bytes
    quals: bytes
    ref_allele: bytes                  # the ref allele window, upper case
    flag: int                          # FLAG & (0x1 | 0x10 | 0x40)
    mapq: int

    def key(self):
        return (self.record, self.status, self.read_interval, self.ref_interval, self.flag, self.mapq)


def evidence(records: List[BamRecord], ref_seq: bytes, locus: IndelLocus, window: int = 64, first_ordinal: int = 0,
             ref_id: Optional[int] = None) -> List[Evidence]:
    """What csrc/vlr_indelpileup.h computes per record, restated: every valid record (basecalls.is_valid_record, sample.rs:281-286:
    unmapped, secondary, duplicate and QC-fail records dropped, supplementary ones kept) on the locus's contig (`ref_id`, the index
    in the BAM header; None = every record lies on it) whose alignment with its soft clips overlaps [start, end), with the windows
    of its candidate region.  Differs from evidence_windows in the filter and in keeping no-overlap reads."""
    from . import realign
    from .basecalls import is_valid_record
    out = []
    n = len(ref_seq)
    for k, r in enumerate(records):
        if not is_valid_record(r.flag) or r.ref_id < 0 or r.pos < 0 or (ref_id is not None and r.ref_id != ref_id):
            continue
        if not overlaps(r, locus.start, locus.end):
            continue
        flag = r.flag & (0x1 | 0x10 | 0x40)
        try:
            reg = candidate_region(r, locus.start, locus.end, n, window)
        except ValueError:
            out.append(Evidence(first_ordinal + k, LEADING_REFSKIP, (0, 0), (0, 0), b"", b"", b"", flag, r.mapq))
            continue
        if not reg.overlap:
            out.append(Evidence(first_ordinal + k, NO_OVERLAP, (0, 0), (0, 0), b"", b"", b"", flag, r.mapq))
            continue
        ro, re_ = reg.read_interval
        if re_ - ro < 1:
            continue
        rb, re2 = reg.ref_interval
        rb = min(rb, re2)          # (a breakpoint behind the contig's end: an empty window)
        out.append(Evidence(first_ordinal + k, 0, (ro, re_), (rb, re2), r.seq[ro:re_].upper(), bytes(r.qual[ro:re_]),
                            realign.ref_allele(ref_seq, rb, re2).upper(), flag, r.mapq))
    return out


class IndelPileupError(ValueError):
    pass


@dataclass
class PairArrays:
    """the pair arrays of a session opened with keep_pairs, in hit order: the layout of realign.PairBatch.arrays()"""
    x_offset: "object"
    x_bases: "object"
    y_offset: "object"
    y_bases: "object"
    y_quals: "object"
    band: "object"

    def arrays(self):
        return self.x_offset, self.x_bases, self.y_offset, self.y_bases, self.y_quals, self.band


def locus_arrays(ref_id, loci: List[IndelLocus]):
    """(ref_id, start, end, kind, alt_off, alt bases) of `loci` on the contigs `ref_id` as the open calls of the indel sessions take them:
    the alt allele window of locus k lies at alt bases[alt_off[k] .. alt_off[k + 1])"""
    import numpy as np
    from . import abi
    kinds = {"deletion": abi.INDELPILEUP_DELETION, "insertion": abi.INDELPILEUP_INSERTION, "replacement": abi.INDELPILEUP_REPLACEMENT}
    alt_off = np.zeros(len(loci) + 1, np.uint64)
    alt_off[1:] = np.cumsum([len(l.alt_allele) for l in loci])
    return (np.array(list(ref_id), np.int32), np.array([l.start for l in loci], np.int64), np.array([l.end for l in loci], np.int64),
            np.array([kinds[l.kind] for l in loci], np.uint8), alt_off, np.frombuffer(b"".join(bytes(l.alt_allele) for l in loci) or b"\0", np.uint8).copy())


def device_hits(bams, fasta: str, ref_id, loci: List[IndelLocus], mode: str = "exact", gap=None, hop=None, window: int = 64, device: int = 0,
                hit_capacity: Optional[int] = None, window_bytes: int = 0, keep_pairs: bool = False, retry: bool = True):
    """(hits as a numpy array of abi.INDELPILEUP_HIT_DTYPE, locus-major; abi.IndelPileupCounts; PairArrays or None) from the kernels.
    `bams`: one path or a list of them (one session, records counted through).  `loci` with their `ref_id` (index of the contig in the
    BAM header), sorted by (ref_id, start).  An overflow of `hit_capacity` is retried once with the needed capacity unless retry=False
    (then the counts carry INDELPILEUP_OVERFLOW and the array is empty)."""
    import ctypes as C
    import numpy as np
    from . import abi, engine, realign
    L = engine.lib()
    if mode not in MODES:
        raise ValueError("mode must be one of %s" % ", ".join(MODES))
    n = len(loci)
    rid, start, end, kind, alt_off, altb = locus_arrays(ref_id, loci)
    g = (gap or realign.GapParams()).as_array()
    if mode == "homopolymer":
        h_ = (hop or realign.HopParams()).as_array()
    else:
        h_ = None
    cap = int(hit_capacity) if hit_capacity is not None else max(1 << 16, 64 * n)
    paths = [bams] if isinstance(bams, str) else list(bams)
    while True:
        h = C.c_void_p()
        engine._check(L.vlr_indelpileup_open(int(device), fasta.encode(), n, rid.ctypes.data, start.ctypes.data, end.ctypes.data, kind.ctypes.data,
                                             alt_off.ctypes.data, altb.ctypes.data, int(window), MODES[mode], g, h_, int(bool(keep_pairs)), cap,
                                             int(window_bytes), C.byref(h)))
        try:
            for p in paths:
                engine._check(L.vlr_indelpileup_add_bam(h, p.encode()))
            res = abi.IndelPileupCounts()
            engine._check(L.vlr_indelpileup_result(h, C.byref(res)))
            if res.status & abi.INDELPILEUP_GUARD_DAMAGED:
                raise IndelPileupError("the guard words behind the hit buffer changed")
            if res.status & abi.INDELPILEUP_OVERFLOW and retry:
                cap = int(res.needed_capacity)
                retry = False
                continue
            hits = np.zeros(int(res.n_hits), abi.INDELPILEUP_HIT_DTYPE)
            engine._check(L.vlr_indelpileup_read(h, hits.ctypes.data, int(res.n_hits)))
            pairs = None
            if keep_pairs and not res.status & abi.INDELPILEUP_OVERFLOW:
                npairs, nx, ny = int(res.n_pairs), int(res.x_bytes), int(res.y_bytes)
                xo, yo = np.zeros(npairs + 1, np.uint32), np.zeros(npairs + 1, np.uint32)
                xb, yb, qb = np.zeros(max(nx, 1), np.uint8), np.zeros(max(ny, 1), np.uint8), np.zeros(max(ny, 1), np.uint8)
                band = np.zeros(npairs, np.int32)
                engine._check(L.vlr_indelpileup_read_pairs(h, xo.ctypes.data, xb.ctypes.data, nx, yo.ctypes.data, yb.ctypes.data, qb.ctypes.data, ny,
                                                           band.ctypes.data, npairs))
                pairs = PairArrays(xo, xb, yo, yb, qb, band)
            return hits, res, pairs
        finally:
            L.vlr_indelpileup_close(h)


@dataclass
class LocusSupports:
    """the evidences of one candidate: its locus, its hits (abi.INDELPILEUP_HIT_DTYPE, record order) and the normalised supports"""
    locus: IndelLocus
    hits: "object"
    prob_alt: "object"
    prob_ref: "object"


def device_supports(bam: str, fasta: str, candidates, mode: str = "exact", gap=None, hop=None, window: int = 64, device: int = 0,
                    hit_capacity: Optional[int] = None, window_bytes: int = 0, keep_pairs: bool = False):
    """Per candidate (contig, 0-based position, REF, ALT), in the order given, the supports of every evidence from BAM records on the
    device (vlr_indelpileup_*): (ln P(read | alt), ln P(read | ref)) normalised as mod.rs:359-385, (ln 0.5, ln 0.5) for a read without
    overlap.  An overflow of the hit buffer is retried once with the needed capacity.  A record whose CIGAR begins with a reference
    skip raises the ValueError read_pos raises.  Returns a list of LocusSupports (with keep_pairs: (list, PairArrays in the
    session's locus order))."""
    import numpy as np
    from . import abi, alignprops, realign
    seqs = read_fasta(fasta)
    contigs, _ = alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)
    tid = {name: k for k, (name, _) in enumerate(contigs)}
    loci, rid = [], []
    for c, pos, ref, alt in candidates:
        if c not in tid or c not in seqs:
            raise ValueError("contig %s is not in the BAM header and the reference" % c)
        loci.append(indel_locus(seqs[c].upper(), int(pos), ref, alt, window))
        rid.append(tid[c])
    order = sorted(range(len(loci)), key=lambda k: (rid[k], loci[k].start))
    arr, res, pairs = device_hits(bam, fasta, [rid[k] for k in order], [loci[k] for k in order], mode, gap, hop, window, device, hit_capacity, window_bytes,
                                  keep_pairs)
    if res.status & abi.INDELPILEUP_BAD_RECORD:
        raise IndelPileupError("%s: record %d is malformed" % (bam, int(res.first_bad_record)))
    if res.status & abi.INDELPILEUP_OVERFLOW:
        raise IndelPileupError("%s: %d hits do not fit the hit buffer" % (bam, int(res.needed_capacity)))
    if (arr["status"] & LEADING_REFSKIP).any():
        raise ValueError("leading reference skip")
    out: List[Optional[LocusSupports]] = [None] * len(loci)
    first = np.searchsorted(arr["locus"], np.arange(len(loci) + 1))
    for j, k in enumerate(order):
        hs = arr[first[j]:first[j + 1]]
        pa, pr = np.empty(len(hs)), np.empty(len(hs))
        for i, h in enumerate(hs):
            pr[i], pa[i] = realign.normalize_support(float(h["ln_ref"]), float(h["ln_alt"]))
        out[k] = LocusSupports(loci[k], hs, pa, pr)
    return (out, pairs) if keep_pairs else out
