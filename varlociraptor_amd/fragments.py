"""Fragment observations of SNV / MNV candidates from BAM records: one observation per fragment, with the features the artifact
hypotheses need, as `varlociraptor preprocess variants` forms them for a single-locus SNV or MNV.  A CPU restatement of the reference's
path and the front end of its HIP kernels (csrc/vlr_fragpileup.hip, vlr_fragpileup_* of include/vlr.h).  Mirrors

  RecordBuffer window (read-pair mode)           variants/sample.rs:96-108, 259-268: W = (insert_size.mean + 6 sd) as u64, without an
                                                 insert size max_read_len + max_del_cigar_len + 10; a record is a member of a locus when
                                                 its START lies in [start - W, end).  The test is on the start alone: that is how
                                                 rust-htslib's RecordBuffer::fetch keeps records (a crate the reference does not vendor)
  Variant::extract_observations                  variants/types/mod.rs:283-407: pairing by QNAME in file order (the first member is
                                                 `left`, every later one replaces `right` unless both are first AND last in template),
                                                 pairs with a MAPQ of 0 dropped, candidates in the byte order of their names
  Snv / Mnv::is_valid_evidence, allele_support   snv.rs:186-242, mnv.rs:242-300 (per-read supports: basecalls.allele_support)
  Variant::evidence_to_observation               read_observation.rs:630-670 (an observation only for a merged strand other than None)
  prob_mapping / min_mapq                        mod.rs:255-281 (the lower MAPQ of a pair)
  read_orientation, Evidence::read_orientation   read_observation.rs:131-159, 743-765 (RO:Z, else rust-htslib's read_pair_orientation)
  Evidence::softclipped / len / is_paired / alt_loci, ExactAltLoci   read_observation.rs:161-210, 766-815
  major_read_position, major_alt_locus, locus_to_bucket, calc_major_feature, process   read_observation.rs:294-351, 498-605
  adjust_prob_mapping                            read_observation.rs:456-496

What runs where: the kernels form members, fragments, observations, the major read position and — from the XA:Z entries of the
records, as keys (64-bit FNV-1a of the contig bytes, bucket position; two contig names that collide in 64 bits would be merged) — the
major alt locus and every observation's alt-locus class.  The front end adds what needs libm: prob_hit_base = -ln(len_sum) and the
MAPQ adjustment (a sequential ln_sum_exp in observation order).  A locus with more than abi.FRAGPILEUP_MAX_MEMBERS members, or whose
observations carry more alt loci than that, comes back flagged and is finished with the restatement on the library's tables, as are
MNVs longer than basecalls.MAX_LEN.

Realignment of indel-bearing reads (snv.rs:72-86, mnv.rs:83, Realigner::allele_support, realignment/mod.rs:161-424): with a
RealignSpec a record that encloses the locus and carries an I or D operation is realigned against the ref and the alt allele window
(`realign_evidence`, `realigned_hit`): candidate region (mod.rs:58-153) on [start, start + len), ref allele window = its ref interval,
alt allele window = readwindows.substitution_locus, edit distance / band / pair HMM of the spec's mode, realign.normalize_support;
strand = the record's when the supports differ, else none; no read position, no third-allele evidence.  device="cpu" scores the windows
with the CPU restatement of the pair HMMs under oracle/, a device number with the kernels (vlr_fragpileup_open_realign in one pass over
the BAM; loci finished on the host through realign.best_hits / prob_related*).  NOT mirrored there: the read-inferred third allele
(mod.rs:317-348: needs the Myers traceback of the `bio` crate, which the reference does not vendor), `alt_variants`
(--atomic-candidate-variants stays required, so an MNV is realigned only for an indel operation), `homopolymer_indel_len`.  Refused,
with the record's ordinal: a CIGAR that begins with N (read_pos fails) and a record that needs realignment and carries an SI:Z tag
(strand information over an interval, mod.rs:381-387).

NOT mirrored (callers must know): `alt_variants`; without a RealignSpec the realignment (with realign_indel_reads=True such
observations come back flagged NEEDS_REALIGN and `observations` raises), `max_depth` subsampling (the `rand` crate's StdRng),
`report_fragment_ids` (None), indel / SV / breakend candidates with their insert-size terms, haplotype blocks, methylation.
`preprocess_variants` is the command `python -m varlociraptor_amd preprocess variants`; it says what it does not do as errors.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi, basecalls
from .basecalls import Hit, Locus, Tables
from .engine import EngineError   # (a reference without its .fai index, a window the kernels refuse: what the command reports)
from .readwindows import BamRecord, read_bam, read_fasta

NEEDS_REALIGN = basecalls.NEEDS_REALIGN
INVALID_RO = abi.FRAGPILEUP_OBS_INVALID_RO
REALIGN_STRAND_INFO = abi.FRAGPILEUP_OBS_REALIGN_STRAND_INFO
MAX_INDEL_WINDOW = abi.INDELPILEUP_MAX_WINDOW   # cli.rs:877
ORIENT_INVALID = 255
RO_VALUES = {b"F1R2": abi.FRAG_F1R2, b"F2R1": abi.FRAG_F2R1, b"F1F2": abi.FRAG_F1F2, b"F2F1": abi.FRAG_F2F1, b"R1R2": abi.FRAG_R1R2,
             b"R2R1": abi.FRAG_R2R1, b"R1F2": abi.FRAG_R1F2, b"R2F1": abi.FRAG_R2F1, b"None": abi.FRAG_ORIENT_NONE}
PROB_05 = math.log(0.5)


class InvalidReadOrientationInfo(ValueError):
    """Error::InvalidReadOrientationInfo: an RO:Z value that names no orientation"""


class FragPileupError(ValueError):
    pass


class NeedsRealign(FragPileupError):
    """a read the reference would realign (realign_indel_reads=True) and no RealignSpec to realign it with"""


class LeadingRefSkip(FragPileupError):
    """rust-htslib's read_pos fails on a CIGAR that begins with a reference skip"""


class RealignStrandInfo(FragPileupError):
    """a record that needs realignment carries an SI:Z tag: strand information over an interval (mod.rs:381-387) is not built"""


@dataclass
class RealignSpec:
    """how indel-bearing reads are realigned: --indel-window, --pairhmm-mode, gap and homopolymer parameters (realign.GapParams /
    HopParams; None = the defaults, as for an alignment-properties JSON without them)"""
    window: int = 64
    mode: str = "exact"
    gap: Optional[object] = None
    hop: Optional[object] = None

    def __post_init__(self):
        from .readwindows import MODES
        if not 1 <= int(self.window) <= MAX_INDEL_WINDOW:
            raise ValueError("indel window %d outside 1 .. %d" % (self.window, MAX_INDEL_WINDOW))
        if self.mode not in MODES:
            raise ValueError("mode must be one of %s" % ", ".join(MODES))


@dataclass
class Props:
    """what the path needs of the alignment properties"""
    window: int
    max_mapq: int
    max_read_len: int


def window_of(insert_size: Optional[Tuple[float, float]], max_read_len: int, max_del_cigar_len: Optional[int]) -> int:
    """sample.rs:259-268 (read-pair mode)"""
    if insert_size is not None:
        return max(int(insert_size[0] + insert_size[1] * 6.0), 0)
    return int(max_read_len) + int(max_del_cigar_len or 0) + 10


def props_of(p) -> Props:
    """from alignprops.AlignmentProperties or the dict of an alignment-properties JSON"""
    if isinstance(p, Props):
        return p
    if isinstance(p, dict):
        ins = p.get("insert_size")
        ins = (float(ins["mean"]), float(ins["sd"])) if ins else None
        # max_mapq: serde default 60 (estimation/alignment_properties.rs BackwardsCompatibility::default_max_mapq)
        return Props(window_of(ins, int(p["max_read_len"]), p.get("max_del_cigar_len")), int(p.get("max_mapq", 60)), int(p["max_read_len"]))
    return Props(window_of(p.insert_size, p.max_read_len, p.max_del_cigar_len), int(p.max_mapq), int(p.max_read_len))


# ---------------------------------------------------------------------------------------------- per-record features
def _first_aux(rec: BamRecord, tag: bytes):
    for t, ty, val in basecalls.aux_fields(rec.aux):
        if t == tag:
            return ty, val
    return None


def orientation_of_flags(rec: BamRecord) -> int:
    """rust-htslib read_pair_orientation: paired, both mates mapped, one contig, different positions; the mate that lies left first"""
    f = rec.flag
    if not f & 0x1 or f & 0x4 or f & 0x8 or rec.ref_id != rec.mate_ref_id or rec.pos == rec.mate_pos:
        return abi.FRAG_ORIENT_NONE
    fwd, mfwd, first = not f & 0x10, not f & 0x20, bool(f & 0x40)
    p1, p2 = (rec.pos, rec.mate_pos) if first else (rec.mate_pos, rec.pos)
    f1, f2 = (fwd, mfwd) if first else (mfwd, fwd)
    if p1 < p2:
        return RO_VALUES[("%s1%s2" % ("F" if f1 else "R", "F" if f2 else "R")).encode()]
    return RO_VALUES[("%s2%s1" % ("F" if f2 else "R", "F" if f1 else "R")).encode()]


def record_orientation(rec: BamRecord) -> int:
    """read_orientation (read_observation.rs:131-159); ORIENT_INVALID where the reference fails"""
    ro = _first_aux(rec, b"RO")
    if ro is not None and ro[0] == "Z":
        vals = ro[1][:-1].split(b",")
        if len(vals) != 1:
            return abi.FRAG_ORIENT_NONE
        return RO_VALUES.get(vals[0], ORIENT_INVALID)
    return orientation_of_flags(rec)


def softclipped(rec: BamRecord) -> bool:
    """leading_softclips() > 0 || trailing_softclips() > 0 (rust-htslib: one hard clip at either end is skipped)"""
    c = rec.cigar
    if not c:
        return False
    lead = c[1] if c[0][0] == "H" and len(c) > 1 else c[0]
    trail = c[-2] if c[-1][0] == "H" and len(c) > 1 else c[-1]
    return (lead[0] == "S" and lead[1] > 0) or (trail[0] == "S" and trail[1] > 0)


def _parse_u64(s: bytes) -> Optional[int]:
    """str::parse::<u64>: an optional '+', then decimal digits only, no overflow"""
    if s[:1] == b"+":
        s = s[1:]
    if not s or any(c < 0x30 or c > 0x39 for c in s):
        return None
    v = int(s)
    return v if v < 1 << 64 else None


def alt_loci(rec: BamRecord) -> List[Tuple[bytes, int]]:
    """ExactAltLoci::from (read_observation.rs:167-210): (contig, position) of the XA:Z entries with exactly four items"""
    xa = _first_aux(rec, b"XA")
    if xa is None or xa[0] != "Z":
        return []
    out = []
    for entry in xa[1][:-1].split(b";"):
        if not entry:
            continue
        items = entry.split(b",")
        if len(items) != 4:
            continue
        pos = items[1][1:] if items[1][:1] == b"-" else items[1]
        v = _parse_u64(pos)
        if v is not None:
            out.append((items[0], v))
    return out


def has_xa(rec: BamRecord) -> bool:
    xa = _first_aux(rec, b"XA")
    return xa is not None and xa[0] == "Z"


def fnv1a64(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def bucket(loc: Tuple[bytes, int], max_read_len: int) -> Tuple[bytes, int]:
    """locus_to_bucket"""
    coeff = max_read_len * 10
    return loc[0], loc[1] // coeff * coeff


def hashed(loc: Tuple[bytes, int]) -> Tuple[int, int]:
    """the alt-locus key in integers: (64-bit FNV-1a of the contig bytes, position).  Two contig names that collide in 64 bits would be
    merged."""
    return fnv1a64(loc[0]), loc[1]


def calc_major_feature(values):
    """read_observation.rs:498-527: the most common value when it occurs more than once and more often than any other"""
    counts: Dict = {}
    for v in values:
        counts[v] = counts.get(v, 0) + 1
    if not counts:
        return None
    top = sorted(counts.values(), reverse=True)
    if top[0] == 1 or (len(top) > 1 and top[1] == top[0]):
        return None
    return next(v for v, n in counts.items() if n == top[0])


# ---------------------------------------------------------------------------------------------- fragments of one locus
@dataclass
class FragObs:
    prob_ref: float
    prob_alt: float
    left: int                        # record ordinals; right = None for a single read
    right: Optional[int]
    read_position: Optional[int]
    third_allele: int
    len_sum: int
    min_mapq: int
    orientation: int                 # abi.FRAG_*
    strand: int
    softclipped: bool
    paired: bool
    is_max_mapq: bool
    has_xa: bool
    status: int = 0
    alt_loci: List[Tuple[bytes, int]] = field(default_factory=list)
    alt_locus: Optional[int] = None   # abi.ALTLOCUS_*, where the kernels gave it

    def key(self):
        return (self.prob_ref, self.prob_alt, self.left, self.right, self.read_position, self.third_allele, self.len_sum, self.min_mapq, self.orientation,
                self.strand, self.softclipped, self.paired, self.is_max_mapq, self.has_xa, self.status)


def is_member(rec: BamRecord, loc: Locus, window: int) -> bool:
    return basecalls.is_valid_record(rec.flag) and rec.ref_id == loc.ref_id and rec.pos >= 0 and max(loc.start - window, 0) <= rec.pos < loc.end


def _support(rec: BamRecord, loc: Locus, li: int, ordinal: int, t: Tables, realign_indel_reads: bool, realigned: Optional[Dict] = None) -> Optional[Hit]:
    """allele_support_per_read; what the reference raises comes back as the hit's status.  `realigned`: {(ordinal, locus): Hit} of the
    records that were realigned"""
    try:
        h = basecalls.allele_support(rec, loc, li, ordinal, t, realign_indel_reads)
        if h is not None and h.status & NEEDS_REALIGN and realigned is not None:
            return realigned[(ordinal, li)]
        return h
    except basecalls.ReadPosOutOfBounds:
        st = abi.BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS
    except basecalls.InvalidStrandInfo:
        st = abi.BASEPILEUP_HIT_INVALID_STRAND_INFO
    except ValueError:
        st = abi.BASEPILEUP_HIT_LEADING_REFSKIP
    return Hit(li, ordinal, 0.0, 0.0, abi.STRAND_NONE, None, 0, rec.mapq, 0, st, (ordinal,))


def fragment_observation(left: Tuple[int, BamRecord], right: Optional[Tuple[int, BamRecord]], loc: Locus, li: int, max_mapq: int, t: Tables,
                         realign_indel_reads: bool = False, realigned: Optional[Dict] = None) -> Optional[FragObs]:
    """mod.rs:352-384 and evidence_to_observation for one candidate"""
    lo, lr = left
    if right is not None:
        if lr.mapq == 0 or right[1].mapq == 0:
            return None
        if not basecalls.enclosing(lr, loc) and not basecalls.enclosing(right[1], loc):
            return None
    elif not basecalls.enclosing(lr, loc):
        return None
    hl = _support(lr, loc, li, lo, t, realign_indel_reads, realigned)
    hr = _support(right[1], loc, li, right[0], t, realign_indel_reads, realigned) if right is not None else None
    if hl is None and hr is None:
        return None
    h = basecalls.merge(hl, hr) if hl is not None and hr is not None else (hl if hl is not None else hr)
    status = h.status
    if status:
        h = Hit(li, lo, 0.0, 0.0, abi.STRAND_NONE, None, 0, 0, 0, status)
    elif h.strand == abi.STRAND_NONE:
        return None
    orient = record_orientation(lr)
    if right is not None:
        o2 = record_orientation(right[1])
        if ORIENT_INVALID in (orient, o2):
            orient = ORIENT_INVALID
        elif orient != o2:
            orient = abi.FRAG_ORIENT_NONE
    if orient == ORIENT_INVALID:
        status |= INVALID_RO
        orient = abi.FRAG_ORIENT_NONE
    recs = [lr] + ([right[1]] if right is not None else [])
    min_mapq = min(r.mapq for r in recs)
    return FragObs(h.prob_ref, h.prob_alt, lo, right[0] if right is not None else None, h.read_position, h.third_allele, sum(len(r.seq) for r in recs), min_mapq,
                   orient, h.strand, any(softclipped(r) for r in recs), bool(lr.flag & 0x1), min_mapq == max_mapq, any(has_xa(r) for r in recs), status,
                   [a for r in recs for a in alt_loci(r)])


def locus_observations(members: Sequence[Tuple[int, BamRecord]], loc: Locus, li: int, max_mapq: int, t: Tables = basecalls.TABLES,
                       realign_indel_reads: bool = False, realigned: Optional[Dict] = None) -> List[FragObs]:
    """the observations of one locus from its members (ordinal, record) in file order, in the byte order of the names"""
    cand: Dict[bytes, List] = {}
    for o, rec in members:
        name = rec.raw_name if rec.raw_name is not None else rec.qname.encode()   # the record's bytes: the order and the pairing are on them
        c = cand.get(name)
        if c is None:
            cand[name] = [(o, rec), None]
            continue
        lf, f = c[0][1].flag, rec.flag
        if (lf & 0x40 and f & 0x40) and (lf & 0x80 and f & 0x80):
            continue
        c[1] = (o, rec)
    out = []
    for name in sorted(cand):
        ob = fragment_observation(cand[name][0], cand[name][1], loc, li, max_mapq, t, realign_indel_reads, realigned)
        if ob is not None:
            out.append(ob)
    return out


def major_read_position(obs: Sequence[FragObs]) -> Optional[int]:
    return calc_major_feature(o.read_position for o in obs if o.status == 0 and o.prob_alt > o.prob_ref and o.read_position is not None)


@dataclass
class Restated:
    per_locus: List[List[FragObs]]           # in the order of the loci given
    n_members: List[int]
    n_records: int = 0
    max_read_len: int = 0
    n_rejected: int = 0
    bad_records: List[int] = field(default_factory=list)
    evidences: List["RealignEvidence"] = field(default_factory=list)   # with a RealignSpec: the realigned evidences, record-major


# ---------------------------------------------------------------------------------------------- realignment of indel-bearing reads
@dataclass
class RealignEvidence:
    """one (record, locus) pair that is realigned: what csrc/vlr_fragpileup.h `realign_evidence` computes, and its scores"""
    locus: int
    ev: "object"                     # readwindows.Evidence: status 0 / NO_OVERLAP / LEADING_REFSKIP / abi.INDELPILEUP_HIT_STRAND_INFO
    alt_allele: bytes                # the alt allele window (empty with a status)
    ln_ref: float = -math.inf        # raw scores and edit distances, as in a vlr_indelpileup_hit
    ln_alt: float = -math.inf
    dist_ref: int = -1
    dist_alt: int = -1

    def key(self):
        return (self.locus,) + self.ev.key()


def realign_evidence(rec: BamRecord, loc: Locus, li: int, ordinal: int, ref_seq: bytes, window: int) -> RealignEvidence:
    """The windows of a record that encloses `loc` and carries an I or D operation (`ref_seq`: its contig, upper case)."""
    from . import readwindows as rw
    from . import realign
    flag = rec.flag & (0x1 | 0x10 | 0x40)

    def refused(status):
        return RealignEvidence(li, rw.Evidence(ordinal, status, (0, 0), (0, 0), b"", b"", b"", flag, rec.mapq), b"")
    try:
        reg = rw.candidate_region(rec, loc.start, loc.end, len(ref_seq), window)
    except ValueError:
        return refused(rw.LEADING_REFSKIP)
    if basecalls.aux_tag_strand_info(rec) is not None:
        return refused(abi.INDELPILEUP_HIT_STRAND_INFO)
    ro, re_ = reg.read_interval
    if not reg.overlap or re_ - ro < 1:
        return refused(rw.NO_OVERLAP)
    rb, re2 = reg.ref_interval
    rb = min(rb, re2)
    alt = rw.substitution_locus(ref_seq, loc.start, loc.ref, loc.alt, window).alt_allele
    return RealignEvidence(li, rw.Evidence(ordinal, 0, (ro, re_), (rb, re2), rec.seq[ro:re_].upper(), bytes(rec.qual[ro:re_]),
                                           realign.ref_allele(ref_seq, rb, re2).upper(), flag, rec.mapq), alt)


def evidence_pair_batch(evs: Sequence[RealignEvidence]):
    """pair 2e = (ref allele window, read window), pair 2e + 1 = (alt allele window, read window), bands unset"""
    from .realign import PairBatch
    pb = PairBatch()
    for e in evs:
        pb.add(e.ev.ref_allele, e.ev.read_window, e.ev.quals, -1)
        pb.add(e.alt_allele, e.ev.read_window, e.ev.quals, -1)
    return pb


def score_pairs(pb, spec: RealignSpec, device="cpu"):
    """(edit distances, ln P) of every pair of a realign.PairBatch in the spec's mode; sets the bands as the reference does (distance + 4,
    -1 without a hit, none in fast mode).  device="cpu": oracle/'s restatement of the pair HMMs; a device number: the kernels."""
    from . import realign
    gap = spec.gap or realign.GapParams()
    n = len(pb)
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0)
    if device != "cpu":
        dist, _, _ = realign.best_hits(pb, int(device))
        if spec.mode == "fast":
            return dist, realign.prob_best_path(pb, gap, int(device))
        pb.band = [int(x) + realign.EDIT_BAND if x >= 0 else -1 for x in dist]
        if spec.mode == "homopolymer":
            return dist, realign.prob_related_homopolymer(pb, gap, spec.hop or realign.HopParams(), int(device))
        return dist, realign.prob_related(pb, gap, int(device))
    from oracle import oracle      # (the repository's CPU restatement of the pair HMMs; built on first use)
    oracle.build()
    g = [gap.prob_insertion_artifact, gap.prob_deletion_artifact, gap.prob_insertion_extend_artifact, gap.prob_deletion_extend_artifact]
    dist, lnp = np.full(n, -1, np.int32), np.full(n, -math.inf)
    for k in range(n):
        x, y, q = pb.x[k], pb.y[k], pb.q[k]
        if not x or not y:
            continue
        dist[k] = oracle.edit_distance(x, y)[0]
        if spec.mode == "fast":
            lnp[k] = oracle.pathhmm_best(x, y, q, g)
            continue
        pb.band[k] = int(dist[k]) + realign.EDIT_BAND if dist[k] >= 0 else -1
        if spec.mode == "homopolymer":
            lnp[k] = oracle.homopoly_prob_related(x, y, q, g, (spec.hop or realign.HopParams()).as_list(), pb.band[k])
        else:
            lnp[k] = oracle.pairhmm_prob_related(x, y, q, g, pb.band[k])
    return dist, lnp


def realigned_hit(e: RealignEvidence, rec: BamRecord) -> Hit:
    """the member support of a realigned evidence (csrc/vlr_fragpileup.h `apply_realigned`)"""
    from . import readwindows as rw
    from . import realign
    o = e.ev.record
    if e.ev.status & rw.LEADING_REFSKIP:
        return Hit(e.locus, o, 0.0, 0.0, abi.STRAND_NONE, None, 0, rec.mapq, e.ev.flag, abi.BASEPILEUP_HIT_LEADING_REFSKIP, (o,))
    if e.ev.status & abi.INDELPILEUP_HIT_STRAND_INFO:
        return Hit(e.locus, o, 0.0, 0.0, abi.STRAND_NONE, None, 0, rec.mapq, e.ev.flag, REALIGN_STRAND_INFO, (o,))
    pr, pa = realign.normalize_support(e.ln_ref, e.ln_alt)     # (no overlap: ln 0 twice -> ln 0.5 twice, mod.rs:186-199)
    strand = abi.STRAND_NONE if pr == pa else (abi.STRAND_REVERSE if rec.flag & 0x10 else abi.STRAND_FORWARD)
    return Hit(e.locus, o, pr, pa, strand, None, 0, rec.mapq, e.ev.flag, 0, (o,))


def realign_members(good: Sequence[Tuple[int, BamRecord]], loci: Sequence[Locus], which: Sequence[int], props: Props, spec: RealignSpec, ref_seqs: Dict[int, bytes],
                    device="cpu"):
    """(evidences record-major, loci ascending within a record; {(ordinal, locus): Hit}) of the members of the loci `which` (ascending)
    that need realignment"""
    evs: List[RealignEvidence] = []
    recs: List[BamRecord] = []
    for o, rec in good:
        if not basecalls.contains_indel_op(rec):
            continue
        for li in which:
            loc = loci[li]
            if is_member(rec, loc, props.window) and basecalls.enclosing(rec, loc):
                evs.append(realign_evidence(rec, loc, li, o, ref_seqs[loc.ref_id], spec.window))
                recs.append(rec)
    dist, lnp = score_pairs(evidence_pair_batch(evs), spec, device)
    hits = {}
    for k, (e, rec) in enumerate(zip(evs, recs)):
        e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt = float(lnp[2 * k]), float(lnp[2 * k + 1]), int(dist[2 * k]), int(dist[2 * k + 1])
        hits[(e.ev.record, e.locus)] = realigned_hit(e, rec)
    return evs, hits


def restate(records: Sequence[BamRecord], loci: Sequence[Locus], props: Props, t: Tables = basecalls.TABLES, realign_indel_reads: bool = False,
            first_ordinal: int = 0, only: Optional[Sequence[int]] = None, realign: Optional[RealignSpec] = None, ref_seqs: Optional[Dict[int, bytes]] = None,
            device="cpu") -> Restated:
    """The observations of every locus (`only`: of these loci) from `records` in file order.  `realign`: indel-bearing reads are
    realigned (realign_indel_reads is implied) against `ref_seqs` {ref_id: contig, upper case}, scored on `device`."""
    out = Restated([[] for _ in loci], [0] * len(loci), len(records), props.max_read_len)
    good = []
    for k, rec in enumerate(records):
        if not basecalls.is_valid_record(rec.flag):
            out.n_rejected += 1
        elif basecalls.record_is_bad(rec):
            out.bad_records.append(first_ordinal + k)
        elif rec.ref_id >= 0 and rec.pos >= 0:
            good.append((first_ordinal + k, rec))
    which = list(range(len(loci)) if only is None else only)
    realigned = None
    if realign is not None:
        if ref_seqs is None:
            raise ValueError("realignment needs the contigs of the loci (ref_seqs)")
        realign_indel_reads = True
        out.evidences, realigned = realign_members(good, loci, sorted(which), props, realign, ref_seqs, device)
    for li in which:
        loc = loci[li]
        members = [(o, r) for o, r in good if is_member(r, loc, props.window)]
        out.n_members[li] = len(members)
        out.per_locus[li] = locus_observations(members, loc, li, props.max_mapq, t, realign_indel_reads, realigned)
    return out


# ---------------------------------------------------------------------------------------------- the device
def _bases(loci, attr):
    return np.frombuffer(b"".join(getattr(l, attr) for l in loci) or b"\0", np.uint8).copy()


def device_observations(bams, loci: Sequence[Locus], props: Props, device: int = 0, realign_indel_reads: bool = False, member_capacity: Optional[int] = None,
                        name_capacity: Optional[int] = None, window_bytes: int = 0, retry: bool = True, key_capacity: Optional[int] = None,
                        realign: Optional[RealignSpec] = None, fasta: Optional[str] = None, evidence_capacity: Optional[int] = None, pair_byte_limit: int = 0,
                        evidences: bool = False):
    """(observations as abi.FRAGPILEUP_OBS_DTYPE, locus records as abi.FRAGPILEUP_LOCUS_DTYPE, abi.FragPileupCounts) from the kernels.
    `bams`: a path or several (one record stream: a pair may straddle two files); `loci` sorted by (ref_id, start), MNVs of at most
    basecalls.MAX_LEN bases.  An overflow of a capacity is retried once with the needed ones unless retry=False.
    `realign` (with `fasta`): indel-bearing reads are realigned in the same pass (vlr_fragpileup_open_realign; realign_indel_reads is
    implied); evidences=True adds (the realigned evidences as abi.INDELPILEUP_HIT_DTYPE, record-major; abi.FragPileupRealignCounts) to
    the result."""
    import ctypes as C
    from . import engine
    L = engine.lib()
    if isinstance(bams, str):
        bams = [bams]
    n = len(loci)
    ref_id = np.array([l.ref_id for l in loci], np.int32)
    start = np.array([l.start for l in loci], np.int64)
    length = np.array([len(l.ref) for l in loci], np.int32)
    kind = np.array([l.kind for l in loci], np.uint8)
    refb, altb = _bases(loci, "ref"), _bases(loci, "alt")
    mcap = int(member_capacity) if member_capacity is not None else max(1 << 16, 256 * n)
    ncap = int(name_capacity) if name_capacity is not None else max(1 << 20, 4096 * n)
    kcap = int(key_capacity) if key_capacity is not None else max(1 << 16, 256 * n)
    ecap = int(evidence_capacity) if evidence_capacity is not None else 1 << 14
    if realign is not None:
        from . import realign as rl
        from .readwindows import MODES
        if fasta is None:
            raise ValueError("realignment needs the reference (fasta)")
        gap = (realign.gap or rl.GapParams()).as_array()
        hop = (realign.hop or rl.HopParams()).as_array() if realign.mode == "homopolymer" else None
    while True:
        h = C.c_void_p()
        head = (int(device), n, ref_id.ctypes.data, start.ctypes.data, length.ctypes.data, kind.ctypes.data, refb.ctypes.data, altb.ctypes.data)
        caps = (int(props.window), int(props.max_mapq), int(props.max_read_len), mcap, ncap, kcap, int(window_bytes))
        if realign is None:
            engine._check(L.vlr_fragpileup_open(*head, int(bool(realign_indel_reads)), *caps, C.byref(h)))
        else:
            engine._check(L.vlr_fragpileup_open_realign(*head, 1, *caps, fasta.encode(), int(realign.window), MODES[realign.mode], gap, hop, ecap, int(pair_byte_limit),
                                                        C.byref(h)))
        try:
            for b in bams:
                engine._check(L.vlr_fragpileup_add_bam(h, b.encode()))
            res = abi.FragPileupCounts()
            engine._check(L.vlr_fragpileup_result(h, C.byref(res)))
            if res.status & abi.FRAGPILEUP_GUARD_DAMAGED:
                raise FragPileupError("the guard words behind a buffer of the fragment session changed")
            rres = abi.FragPileupRealignCounts()
            if realign is not None:
                engine._check(L.vlr_fragpileup_realign_result(h, C.byref(rres)))
            over = abi.FRAGPILEUP_ANY_OVERFLOW | abi.FRAGPILEUP_EVIDENCE_OVERFLOW
            if res.status & over and retry:
                mcap, ncap, kcap = max(mcap, int(res.needed_members)), max(ncap, int(res.needed_name_bytes)), max(kcap, int(res.needed_keys))
                ecap = max(ecap, int(rres.needed_evidences))
                retry = False
                continue
            obs = np.zeros(int(res.n_obs), abi.FRAGPILEUP_OBS_DTYPE)
            loc = np.zeros(n, abi.FRAGPILEUP_LOCUS_DTYPE)
            if not res.status & over:
                engine._check(L.vlr_fragpileup_read(h, obs.ctypes.data, len(obs), loc.ctypes.data, n))
            if not evidences:
                return obs, loc, res
            ev = np.zeros(int(rres.n_evidences), abi.INDELPILEUP_HIT_DTYPE)
            if realign is not None and len(ev):
                engine._check(L.vlr_fragpileup_read_realigned(h, ev.ctypes.data, len(ev)))
            return obs, loc, res, ev, rres
        finally:
            L.vlr_fragpileup_close(h)


def obs_from_array(a: np.ndarray) -> List[FragObs]:
    out = []
    for r in a:
        rp, right, bits = int(r["read_position"]), int(r["right"]), int(r["bits"])
        out.append(FragObs(float(r["prob_ref"]), float(r["prob_alt"]), int(r["left"]), None if right == abi.FRAGPILEUP_NO_RECORD else right,
                           None if rp == abi.BASEPILEUP_NO_READ_POSITION else rp, int(r["third_allele"]), int(r["len_sum"]), int(r["min_mapq"]),
                           int(r["orientation"]), int(r["strand"]), bool(bits & abi.FRAGPILEUP_SOFTCLIPPED), bool(bits & abi.FRAGPILEUP_PAIRED),
                           bool(bits & abi.FRAGPILEUP_MAX_MAPQ), bool(bits & abi.FRAGPILEUP_HAS_XA), int(r["status"]), alt_locus=int(r["alt_locus"])))
    return out


def raise_for_status(o: FragObs):
    """what the reference raises for this observation (and what this path does not do)"""
    if o.status & abi.BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS:
        raise basecalls.ReadPosOutOfBounds("read position outside the SI tag of record %d" % o.left)
    if o.status & abi.BASEPILEUP_HIT_INVALID_STRAND_INFO:
        raise basecalls.InvalidStrandInfo("invalid strand information in the SI tag of record %d" % o.left)
    if o.status & abi.BASEPILEUP_HIT_LEADING_REFSKIP:
        raise LeadingRefSkip("leading reference skip in record %d%s" % (o.left, "" if o.right is None else " or its mate, record %d" % o.right))
    if o.status & REALIGN_STRAND_INFO:
        raise RealignStrandInfo("record %d%s carries an insertion or deletion and an SI:Z tag: REALIGN_STRAND_INFO (strand information over the realigned "
                                "interval is not built)" % (o.left, "" if o.right is None else " or its mate, record %d," % o.right))
    if o.status & INVALID_RO:
        raise InvalidReadOrientationInfo("invalid read orientation in the RO tag of record %d or its mate" % o.left)
    if o.status & NEEDS_REALIGN:
        raise NeedsRealign("record %d (or its mate) carries an insertion or deletion and would be realigned by the reference: NEEDS_REALIGN "
                              "(give a RealignSpec / --realign-indel-reads to realign it)" % o.left)


# ---------------------------------------------------------------------------------------------- pileups
@dataclass
class ObsTable:
    """the processed pileup of one candidate (read_observation.rs: ProcessedReadObservation), one row per fragment in name order"""
    prob_alt: np.ndarray
    prob_ref: np.ndarray
    prob_mapping: np.ndarray         # adjusted unless omit_mapq_adjustment
    prob_hit_base: np.ndarray
    strand: np.ndarray
    orientation: np.ndarray          # abi.FRAG_*
    read_position_major: np.ndarray
    softclipped: np.ndarray
    paired: np.ndarray
    is_max_mapq: np.ndarray
    alt_locus: np.ndarray            # abi.ALTLOCUS_*
    third_allele: np.ndarray
    records: List[Tuple[int, ...]]
    major_read_position: Optional[int] = None
    major_alt_locus: Optional[Tuple[bytes, int]] = None

    def __len__(self):
        return len(self.prob_alt)


def relative_eq(a: float, b: float) -> bool:
    """approx::relative_eq! with its defaults (epsilon = max_relative = f64::EPSILON)"""
    if a == b:
        return True
    if math.isinf(a) or math.isinf(b):
        return False
    d = abs(a - b)
    eps = 2.220446049250313e-16
    return d <= eps or d <= max(abs(a), abs(b)) * eps


def adjusted_prob_mapping(pm: Sequence[float], max_mapq: int, t: Tables) -> List[float]:
    """adjust_prob_mapping (read_observation.rs:456-496)"""
    if not pm:
        return []
    top = t.call[max_mapq]
    probs = [p if relative_eq(p, top) else PROB_05 for p in pm]
    s = basecalls.ln_sum_exp(probs)
    n = len(pm)
    if n < 20:
        s = basecalls.ln_sum_exp([s, PROB_05])   # ln_add_exp
        n += 1
    return [s - math.log(n)] * len(pm)


def alt_locus_classes(obs: Sequence[FragObs], max_read_len: int, key=lambda b: b):
    """(major alt locus, class per observation): major_alt_locus and the alt_locus rule of `process`; `key` = hashed for the integer key"""
    buckets = [[key(bucket(a, max_read_len)) for a in o.alt_loci] for o in obs]
    major = calc_major_feature(b for bs in buckets for b in bs)
    if major is None:
        return None, [abi.ALTLOCUS_NONE] * len(obs)
    return major, [abi.ALTLOCUS_MAJOR if major in bs else (abi.ALTLOCUS_NONE if not bs else abi.ALTLOCUS_SOME) for bs in buckets]


def table_of(obs: Sequence[FragObs], props: Props, t: Tables, omit_mapq_adjustment: bool = False, major: object = "compute") -> ObsTable:
    """`process` and adjust_prob_mapping over the observations of one locus; `major`: the major read position where the device gave it"""
    for o in obs:
        raise_for_status(o)
    if major == "compute":
        major = major_read_position(obs)
    pm = [t.call[o.min_mapq] for o in obs]
    if not omit_mapq_adjustment:
        pm = adjusted_prob_mapping(pm, props.max_mapq, t)
    if obs and all(o.alt_locus is not None for o in obs):   # from the kernels (the major key itself stays on the device)
        major_alt, classes = None, [o.alt_locus for o in obs]
    else:
        major_alt, classes = alt_locus_classes(obs, props.max_read_len)
    return ObsTable(np.array([o.prob_alt for o in obs], float), np.array([o.prob_ref for o in obs], float), np.array(pm, float),
                    np.array([-math.log(o.len_sum) if o.len_sum else math.inf for o in obs], float), np.array([o.strand for o in obs], np.uint8),
                    np.array([o.orientation for o in obs], np.uint8),
                    np.array([major is not None and o.read_position == major for o in obs], bool), np.array([o.softclipped for o in obs], bool),
                    np.array([o.paired for o in obs], bool), np.array([o.is_max_mapq for o in obs], bool), np.array(classes, np.uint8),
                    np.array([o.third_allele for o in obs], np.uint32), [(o.left,) if o.right is None else (o.left, o.right) for o in obs], major, major_alt)


def observations(bam, fasta: str, candidates: Sequence[Tuple[str, int, bytes, bytes]], props, device=0, omit_mapq_adjustment: bool = False,
                 realign_indel_reads: bool = False, window_bytes: int = 0, realign: Optional[RealignSpec] = None) -> List[ObsTable]:
    """Per candidate (contig, 0-based position, REF, ALT), in the order given, its processed pileup.  device="cpu": the restatement; a
    device number: the kernels, finished as the module header says.  `realign`: indel-bearing reads are realigned (module header);
    realign_indel_reads=True without it raises NeedsRealign for such a read."""
    from . import alignprops
    props = props_of(props)
    bams = [bam] if isinstance(bam, str) else list(bam)
    seqs = read_fasta(fasta)
    contigs, _ = alignprops.bam_header(alignprops.inflate_bgzf(bams[0]), bams[0])
    tid = {name: k for k, (name, _) in enumerate(contigs)}
    loci = []
    for c, pos, ref, alt in candidates:
        if c not in tid or c not in seqs:
            raise ValueError("contig %s is not in the BAM header and the reference" % c)
        loci.append(basecalls.locus(seqs[c], tid[c], int(pos), ref, alt))
    ref_seqs = {tid[c]: seqs[c].upper() for c in set(c for c, _, _, _ in candidates)} if realign is not None else None
    order = sorted(range(len(loci)), key=lambda k: (loci[k].ref_id, loci[k].start))
    recs: Optional[List[BamRecord]] = None

    def records():
        nonlocal recs
        if recs is None:
            recs = [r for b in bams for r in read_bam(b)[1]]
        return recs
    out: List[Optional[ObsTable]] = [None] * len(loci)
    if device == "cpu":
        t = basecalls.TABLES
        rs = restate(records(), [loci[k] for k in order], props, t, realign_indel_reads, realign=realign, ref_seqs=ref_seqs)
        if rs.bad_records:
            raise FragPileupError("%s: record %d is malformed" % (bams[0], rs.bad_records[0]))
        for j, k in enumerate(order):
            out[k] = table_of(rs.per_locus[j], props, t, omit_mapq_adjustment)
        return out
    t = basecalls.library_tables()
    short = [k for k in order if len(loci[k].ref) <= basecalls.MAX_LEN]
    arr, lrec, res = device_observations(bams, [loci[k] for k in short], props, int(device), realign_indel_reads, window_bytes=window_bytes, realign=realign, fasta=fasta)
    if res.status & abi.FRAGPILEUP_BAD_RECORD:
        raise FragPileupError("%s: record %d is malformed" % (bams[0], int(res.first_bad_record)))
    deep = abi.FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS | abi.FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI
    host = [k for k in order if len(loci[k].ref) > basecalls.MAX_LEN] + [k for j, k in enumerate(short) if lrec[j]["status"] & deep]
    for j, k in enumerate(short):
        if lrec[j]["status"] & deep:
            continue
        o0 = int(lrec[j]["obs_offset"])
        obs = obs_from_array(arr[o0:o0 + int(lrec[j]["n_obs"])])
        mj = int(lrec[j]["major_read_position"])
        out[k] = table_of(obs, props, t, omit_mapq_adjustment, None if mj == abi.BASEPILEUP_NO_READ_POSITION else mj)
    if host:
        rs = restate(records(), [loci[k] for k in host], props, t, realign_indel_reads, realign=realign, ref_seqs=ref_seqs, device=int(device))
        for j, k in enumerate(host):
            out[k] = table_of(rs.per_locus[j], props, t, omit_mapq_adjustment)
    return out


def pack_orientation(orientation: np.ndarray) -> np.ndarray:
    """abi.FRAG_* -> the two-bit VLR_ORIENT_* class of the packed flags"""
    o = np.full(len(orientation), abi.ORIENT_OTHER, np.uint32)
    o[orientation == abi.FRAG_F1R2] = abi.ORIENT_F1R2
    o[orientation == abi.FRAG_F2R1] = abi.ORIENT_F2R1
    o[orientation == abi.FRAG_ORIENT_NONE] = abi.ORIENT_NONE
    return o


def pileup(tables: Sequence[ObsTable], candidates: Sequence[Tuple[str, int, bytes, bytes]], omit_bias_mask: int = 0):
    """(PileupBatch, third-allele column) of one sample: every feature flag filled, locus_flags as obsfmt.read_observation_vcf sets them
    for precise SNVs / MNVs; the column goes to ingest.write_observations(third_allele_evidence=...)."""
    from .batch import PileupBatch
    off = np.zeros(len(tables) + 1, np.int64)
    names = ("prob_mapping", "prob_alt", "prob_ref", "prob_missed_allele", "prob_sample_alt", "prob_double_overlap", "prob_hit_base", "flags")
    cols: Dict[str, List[np.ndarray]] = {k: [] for k in names}
    third = []
    for k, s in enumerate(tables):
        n = len(s)
        off[k + 1] = off[k] + n
        pa, pr = s.prob_alt.copy(), s.prob_ref.copy()
        both = np.isneginf(pa) & np.isneginf(pr)      # AlleleSupport::both_alleles_impossible
        pa[both] = PROB_05
        pr[both] = PROB_05
        cols["prob_mapping"].append(s.prob_mapping)
        cols["prob_alt"].append(pa)
        cols["prob_ref"].append(pr)
        cols["prob_missed_allele"].append(np.logaddexp(pa, pr) - math.log(2.0))
        cols["prob_sample_alt"].append(np.zeros(n))
        cols["prob_double_overlap"].append(np.where(s.strand == abi.STRAND_BOTH, 0.0, -np.inf))
        cols["prob_hit_base"].append(s.prob_hit_base)
        cols["flags"].append(abi.pack_flags(s.strand, pack_orientation(s.orientation), s.read_position_major, s.softclipped, s.paired, s.is_max_mapq, s.alt_locus))
        third.append(s.third_allele.astype(np.int32))
    cat = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}
    snv = np.array([len(c[2]) == 1 for c in candidates], bool)
    lf = 0
    for bit in (abi.BIAS_ORIENTATION, abi.BIAS_STRAND, abi.BIAS_POSITION, abi.BIAS_SOFTCLIP, abi.BIAS_ALTLOCUS):
        if not omit_bias_mask & bit:
            lf |= bit
    if not omit_bias_mask & abi.BIAS_ORIENTATION:
        lf |= abi.LOCUS_REMOVE_NONSTANDARD
    loc = {"locus_flags": (np.full(len(tables), lf, np.uint8) | np.where(snv, abi.LOCUS_HAS_SNV, 0).astype(np.uint8)),
           "variant_type": np.where(snv, abi.VT_SNV, abi.VT_MNV).astype(np.uint8),
           "ref_base": np.array([bytes(c[2]).upper()[0] if len(c[2]) == 1 else 0 for c in candidates], np.uint8),
           "alt_base": np.array([bytes(c[3]).upper()[0] if len(c[3]) == 1 else 0 for c in candidates], np.uint8)}
    batch = PileupBatch(1, off.astype(np.uint32), {k: (np.asarray(v, np.float32) if k != "flags" else np.asarray(v, np.uint32)) for k, v in cat.items()}, loc)
    return batch, (np.concatenate(third) if third else np.zeros(0, np.int32))


# ---------------------------------------------------------------------------------------------- preprocess variants
class PreprocessError(ValueError):
    """something `preprocess variants` does not do, or an input it cannot use; the message names the record or the flag"""


def gap_hop_of(p):
    """(realign.GapParams, realign.HopParams) of alignment properties (the dict of a JSON or alignprops.AlignmentProperties): the
    defaults where the JSON has none"""
    if isinstance(p, dict):
        import json
        from . import alignprops
        p = alignprops.load(json.dumps(p))
    return p.gap_params, p.hop_params


def read_candidates(path: str) -> List[Tuple[str, int, str, str, str]]:
    """(CHROM, 1-based POS, ID, REF, ALT) per ALT allele of a candidate VCF (text) or BCF, in file order"""
    out = []
    if path.endswith(".bcf"):
        from .bcfio import BcfReader
        rows = [(r["chrom"], int(r["pos"]), r["id"], r["ref"], r["alt"]) for r in BcfReader(path)]
    else:
        import gzip
        rows = []
        with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as fh:
            for line in fh:
                if line.startswith("#") or not line.strip():
                    continue
                f = line.rstrip("\n").split("\t")
                rows.append((f[0], int(f[1]), f[2], f[3], f[4]))
    for chrom, pos, rid, ref, alt in rows:
        for a in (alt if isinstance(alt, (list, tuple)) else str(alt).split(",")):
            out.append((chrom, pos, rid if rid else ".", ref, a))
    return out


def preprocess_variants(reference: str, candidates: str, bam: str, output: str, alignment_properties: Optional[str] = None, device=0,
                        atomic_candidate_variants: bool = False, omit_mapq_adjustment: bool = False, max_depth: int = 200,
                        score_indel_reads_from_alignment: bool = False, warn=None, realign: Optional[RealignSpec] = None) -> int:
    """`preprocess variants` for SNV / MNV candidates of one sample: the observation BCF `output` (format v15) that `call variants`
    reads.  Returns the number of records written.  `realign` (--realign-indel-reads): indel-bearing reads over a candidate are
    realigned as the reference does by default; its gap / hop parameters default to those of the alignment properties."""
    import json
    from . import ingest
    if not atomic_candidate_variants:
        raise PreprocessError("--atomic-candidate-variants is required: candidates are scored one by one from the read's own alignment; "
                              "realignment against the other candidates at a locus (alt_variants) is not built")
    sites = read_candidates(candidates)
    cands = []
    for chrom, pos, rid, ref, alt in sites:
        sym = alt.startswith("<") or "[" in alt or "]" in alt or alt in ("*", ".")
        if sym or len(ref) != len(alt) or not ref:
            raise PreprocessError("candidate %s:%d %s>%s is not an SNV or MNV: indel, structural and breakend candidates are not built" % (chrom, pos, ref, alt))
        cands.append((chrom, pos - 1, ref.encode(), alt.encode()))
    if realign is not None and score_indel_reads_from_alignment:
        raise PreprocessError("--realign-indel-reads and --score-indel-reads-from-alignment exclude each other")
    if alignment_properties is not None:
        pj = json.load(open(alignment_properties))
    else:
        from . import alignprops
        pj = alignprops.estimate(reference, [bam], None, device)[0]
    props = props_of(pj)
    if realign is not None and realign.gap is None and realign.hop is None:
        realign = RealignSpec(realign.window, realign.mode, *gap_hop_of(pj))
    try:
        tabs = observations(bam, reference, cands, props, device=device, omit_mapq_adjustment=omit_mapq_adjustment,
                            realign_indel_reads=not score_indel_reads_from_alignment, realign=realign)
    except NeedsRealign as e:
        raise PreprocessError(str(e) + "; --score-indel-reads-from-alignment scores such reads as they are aligned, --realign-indel-reads realigns them") from e
    deep = sum(1 for t in tabs if len(t) > max_depth)
    if deep and warn is not None:
        warn("%d of %d loci have more than --max-depth %d observations; they are processed whole (the reference's subsampling is not built)" % (deep, len(tabs), max_depth))
    batch, third = pileup(tabs, cands)
    ingest.write_observations(output, batch, 0, third_allele_evidence=third, sites=sites)
    return len(sites)
