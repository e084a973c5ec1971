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
(mod.rs:317-348: needs the Myers traceback of the `bio` crate, which the reference does not vendor), `homopolymer_indel_len`.  The
other alleles of a locus (`alt_variants`) are scored against on request (`alt_variants=True`, --alt-variants: the section "the other
alleles of a locus" below); --atomic-candidate-variants has nothing to do with them: in the reference that flag only switches off the
realignment of SNV / MNV candidates (preprocessing/mod.rs:511, 535), the other alleles are collected either way (587-613).  Refused,
with the record's ordinal: a CIGAR that begins with N (read_pos fails) and a record that needs realignment and carries an SI:Z tag
(strand information over an interval, mod.rs:381-387).

NOT mirrored (callers must know): without a RealignSpec the realignment (with realign_indel_reads=True such
observations come back flagged NEEDS_REALIGN and `observations` raises), `max_depth` subsampling (the `rand` crate's StdRng),
`report_fragment_ids` (None), replacement / SV / breakend candidates, haplotype blocks.  Deletion and insertion candidates
are built on request (`indel_candidates`, --indel-candidates): the section "deletion and insertion candidates" below has their rule
and what of it is not mirrored.  Methylation candidates (ALT <METH>) are built on request too (`methylation_readtype`,
--methylation-read-type): methylation.py has their rule and what of it is not mirrored (max_depth subsampling, report_fragment_ids).
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
    if realigned is not None and (ordinal, li) in realigned and not basecalls.contains_indel_op(rec):
        return realigned[(ordinal, li)]        # mnv.rs:83: an MNV with other alleles at its locus realigns every enclosing record
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
                         realign_indel_reads: bool = False, realigned: Optional[Dict] = None, rule=None) -> Optional[FragObs]:
    """mod.rs:352-384 and evidence_to_observation for one candidate.  `rule`: the enclosing test and the per-read support of another
    candidate kind (methylation.Rule); None = an SNV / MNV"""
    lo, lr = left
    enc = basecalls.enclosing if rule is None else rule.enclosing
    if right is not None:
        if lr.mapq == 0 or right[1].mapq == 0:
            return None
        if not enc(lr, loc) and not enc(right[1], loc):
            return None
    elif not enc(lr, loc):
        return None
    if rule is None:
        hl = _support(lr, loc, li, lo, t, realign_indel_reads, realigned)
        hr = _support(right[1], loc, li, right[0], t, realign_indel_reads, realigned) if right is not None else None
    else:
        hl = rule.support(lr, loc, li, lo, t)
        hr = rule.support(right[1], loc, li, right[0], t) if right is not None else None
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
                       realign_indel_reads: bool = False, realigned: Optional[Dict] = None, rule=None) -> List[FragObs]:
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
        ob = fragment_observation(cand[name][0], cand[name][1], loc, li, max_mapq, t, realign_indel_reads, realigned, rule)
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
    winner: int = 0                  # with competitors (alt_variants): the reference-side allele that gave ln_ref, 0 = the reference
    n_tied: int = 0                  # reference-side alleles at the minimum edit distance
    n_ref_side_hits: int = 0         # reference-side alleles with a hit

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


# ---------------------------------------------------------------------------------------------- the other alleles of a locus
# `alt_variants` of the reference (csrc/vlr_altvariants.h states the rule for the kernels; this is the same in Python):
#   the competitors of a candidate      utils/variant_buffer.rs:203-222: the other variants at its (CHROM, POS), the ones before it in
#                                       the file, then the ones after it (`alt_variant_groups`); they are collected with or without
#                                       --atomic-candidate-variants (preprocessing/mod.rs:587-613)
#   a competitor's allele window        its own alt allele window (`competitor_window`): alt_emission_params of snv.rs:158-178,
#                                       mnv.rs:213-234, deletion.rs:121-141 and insertion.rs:74-98 all ignore the region interval they
#                                       are handed, so the window does not depend on the evidence
#   the reference side of an evidence   realignment/mod.rs:250-292 with prob_allele (426-479): edit distances of the reference (i = 0)
#                                       and the competitors (i = 1 .. K); alleles without a hit are out; the ones at the minimum are
#                                       the tied set; only they are scored by the pair HMM; the largest score wins, the lowest i on
#                                       equal scores (`p > prob`) (`score_alt_evidences`)
#   which reads are realigned           every member of an indel candidate; under a RealignSpec the reads of an SNV with an I / D
#                                       operation (snv.rs:76) and the reads of an MNV with one OR any enclosing read when the MNV
#                                       has a competitor (mnv.rs:83)
MAX_ALT_VARIANTS = abi.FRAGPILEUP_MAX_ALT_VARIANTS


def alt_variant_groups(rows) -> List[List[int]]:
    """Per row of `rows` ((CHROM, POS, ...) tuples in file order, as read_candidates gives them) the indices of its competitors: the
    other rows of its run of consecutive rows with equal (CHROM, POS), the ones before it, then the ones after it.  More than
    MAX_ALT_VARIANTS competitors are refused, the locus named."""
    out: List[List[int]] = []
    k, n = 0, len(rows)
    while k < n:
        j = k
        while j < n and (rows[j][0], rows[j][1]) == (rows[k][0], rows[k][1]):
            j += 1
        if j - k - 1 > MAX_ALT_VARIANTS:
            raise PreprocessError("locus %s:%s has %d candidate alleles: at most %d other alleles of a locus are scored against (alt_variants)"
                                  % (rows[k][0], rows[k][1], j - k, MAX_ALT_VARIANTS))
        for i in range(k, j):
            out.append(list(range(k, i)) + list(range(i + 1, j)))
        k = j
    return out


def competitor_window(seq: bytes, pos: int, ref: bytes, alt: bytes, window: int) -> bytes:
    """the alt allele window of the candidate `ref` > `alt` at 0-based `pos` of the contig `seq` as a session builds it for that
    candidate itself: readwindows.substitution_locus (SNV / MNV) or readwindows.indel_locus (deletion / insertion)"""
    from . import readwindows as rw
    loc = rw.substitution_locus(seq.upper(), pos, ref, alt, window) if len(ref) == len(alt) else rw.indel_locus(seq.upper(), pos, ref, alt, window)
    if loc.kind == "replacement":
        raise PreprocessError("a replacement allele (%s>%s at position %d) cannot compete: replacements are not built" % (bytes(ref).decode(), bytes(alt).decode(), pos + 1))
    return bytes(loc.alt_allele)


def select_alleles(dist: Sequence[int]):
    """prob_allele's first loop over the reference side: dist[i] of the reference (i = 0) and the competitors, -1 = no hit.
    (minimum distance or -1, the tied alleles ascending, the number of alleles with a hit)"""
    hits = [d for d in dist if d >= 0]
    if not hits:
        return -1, [], 0
    m = min(hits)
    return m, [i for i, d in enumerate(dist) if d == m], len(hits)


def pair_edit_distances(pb, device="cpu") -> np.ndarray:
    """the edit distance of every pair of a realign.PairBatch (-1: an empty window, no hit)"""
    from . import realign
    if len(pb) == 0:
        return np.zeros(0, np.int32)
    if device != "cpu":
        return np.asarray(realign.best_hits(pb, int(device))[0], np.int32)
    from oracle import oracle
    oracle.build()
    return np.array([oracle.edit_distance(x, y)[0] if x and y else -1 for x, y in zip(pb.x, pb.y)], np.int32)


def pair_hmm(pb, dist: Sequence[int], spec: RealignSpec, device="cpu") -> np.ndarray:
    """ln P of every pair of a realign.PairBatch whose edit distances are `dist`, in the spec's mode, with the bands score_pairs sets"""
    from . import realign
    gap = spec.gap or realign.GapParams()
    n = len(pb)
    if n == 0:
        return np.zeros(0)
    if spec.mode != "fast":
        pb.band = [int(x) + realign.EDIT_BAND if x >= 0 else -1 for x in dist]
    if device != "cpu":
        if spec.mode == "fast":
            return realign.prob_best_path(pb, gap, int(device))
        if spec.mode == "homopolymer":
            return realign.prob_related_homopolymer(pb, gap, spec.hop or realign.HopParams(), int(device))
        return realign.prob_related(pb, gap, int(device))
    from oracle import oracle
    oracle.build()
    g = [gap.prob_insertion_artifact, gap.prob_deletion_artifact, gap.prob_insertion_extend_artifact, gap.prob_deletion_extend_artifact]
    lnp = np.full(n, -math.inf)
    for k in range(n):
        x, y, q = pb.x[k], pb.y[k], pb.q[k]
        if not x or not y:
            continue
        if spec.mode == "fast":
            lnp[k] = oracle.pathhmm_best(x, y, q, g)
        elif spec.mode == "homopolymer":
            lnp[k] = oracle.homopoly_prob_related(x, y, q, g, (spec.hop or realign.HopParams()).as_list(), pb.band[k])
        else:
            lnp[k] = oracle.pairhmm_prob_related(x, y, q, g, pb.band[k])
    return lnp


def score_alt_evidences(evs: Sequence[RealignEvidence], competitors: Sequence[Sequence[bytes]], spec: RealignSpec, device="cpu") -> Tuple[int, int]:
    """Scores `evs` in place against the reference, their alt allele and the competitor windows of their loci (competitors[locus]):
    ln_ref / dist_ref from the winner of the tied set, ln_alt / dist_alt as ever, winner, n_tied, n_ref_side_hits.  Returns (pairs
    through the edit distance, pairs through the pair HMM): only the tied set and the alt pair are scored by the pair HMM."""
    from .realign import PairBatch
    pb, first = PairBatch(), []
    for e in evs:            # pair 0 = ref, pair 1 = alt, pair 1 + i = competitor i (an evidence with a status: empty windows)
        first.append(len(pb))
        pb.add(e.ev.ref_allele, e.ev.read_window, e.ev.quals, -1)
        pb.add(e.alt_allele, e.ev.read_window, e.ev.quals, -1)
        for w in competitors[e.locus]:
            pb.add(w if not e.ev.status else b"", e.ev.read_window, e.ev.quals, -1)
    dist = pair_edit_distances(pb, device)
    kept, kb, sel = [], PairBatch(), []
    for e, p0 in zip(evs, first):
        k = len(competitors[e.locus])
        m, tied, n_hits = select_alleles([int(dist[p0])] + [int(dist[p0 + 1 + i]) for i in range(1, k + 1)])
        pairs = [p0 if i == 0 else p0 + 1 + i for i in (tied or [0])]           # (no hit at all: the reference's pair, as without competitors)
        sel.append((m, tied, n_hits, len(kept), pairs))
        for p in sorted(pairs + [p0 + 1]):
            kept.append(p)
            kb.add(pb.x[p], pb.y[p], pb.q[p], -1)
    lnp = pair_hmm(kb, [int(dist[p]) for p in kept], spec, device)
    at = {}
    for c, p in enumerate(kept):
        at[p] = c
    for e, p0, (m, tied, n_hits, _, pairs) in zip(evs, first, sel):
        best, winner = None, 0
        for i, p in zip(tied or [0], pairs):
            v = float(lnp[at[p]])
            if best is None or v > best:
                best, winner = v, i
        e.ln_ref, e.dist_ref, e.ln_alt, e.dist_alt = best, m, float(lnp[at[p0 + 1]]), int(dist[p0 + 1])
        e.winner, e.n_tied, e.n_ref_side_hits = winner, len(tied), n_hits
    return len(pb), len(kept)


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
                    device="cpu", competitors: Optional[Sequence[Sequence[bytes]]] = None):
    """(evidences record-major, loci ascending within a record; {(ordinal, locus): Hit}) of the members of the loci `which` (ascending)
    that need realignment.  `competitors`: per locus the allele windows of the other candidates at its position (alt_variants)."""
    evs: List[RealignEvidence] = []
    recs: List[BamRecord] = []
    for o, rec in good:
        indel = basecalls.contains_indel_op(rec)
        for li in which:
            loc = loci[li]
            if not indel and not (competitors is not None and len(loc.ref) > 1 and competitors[li]):      # snv.rs:76, mnv.rs:83
                continue
            if is_member(rec, loc, props.window) and basecalls.enclosing(rec, loc):
                evs.append(realign_evidence(rec, loc, li, o, ref_seqs[loc.ref_id], spec.window))
                recs.append(rec)
    if competitors is not None:
        score_alt_evidences(evs, competitors, spec, device)
        return evs, {(e.ev.record, e.locus): realigned_hit(e, rec) for e, rec in zip(evs, recs)}
    dist, lnp = score_pairs(evidence_pair_batch(evs), spec, device)
    hits = {}
    for k, (e, rec) in enumerate(zip(evs, recs)):
        e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt = float(lnp[2 * k]), float(lnp[2 * k + 1]), int(dist[2 * k]), int(dist[2 * k + 1])
        hits[(e.ev.record, e.locus)] = realigned_hit(e, rec)
    return evs, hits


def restate(records: Sequence[BamRecord], loci: Sequence[Locus], props: Props, t: Tables = basecalls.TABLES, realign_indel_reads: bool = False,
            first_ordinal: int = 0, only: Optional[Sequence[int]] = None, realign: Optional[RealignSpec] = None, ref_seqs: Optional[Dict[int, bytes]] = None,
            device="cpu", rule=None, competitors: Optional[Sequence[Sequence[bytes]]] = None) -> Restated:
    """The observations of every locus (`only`: of these loci) from `records` in file order.  `realign`: indel-bearing reads are
    realigned (realign_indel_reads is implied) against `ref_seqs` {ref_id: contig, upper case}, scored on `device`.  `rule`: the loci
    are of another candidate kind (methylation.Rule with methylation.MethLocus).  `competitors` (with `realign`): per locus the allele
    windows of the other candidates at its position (alt_variants)."""
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
        out.evidences, realigned = realign_members(good, loci, sorted(which), props, realign, ref_seqs, device, competitors)
    for li in which:
        loc = loci[li]
        members = [(o, r) for o, r in good if is_member(r, loc, props.window)]
        out.n_members[li] = len(members)
        out.per_locus[li] = locus_observations(members, loc, li, props.max_mapq, t, realign_indel_reads, realigned, rule)
    return out


# ---------------------------------------------------------------------------------------------- the device
def _capacities(n: int, member_capacity, name_capacity, key_capacity):
    return (int(member_capacity) if member_capacity is not None else max(1 << 16, 256 * n), int(name_capacity) if name_capacity is not None else max(1 << 20, 4096 * n),
            int(key_capacity) if key_capacity is not None else max(1 << 16, 256 * n))


def competitor_arrays(competitors: Sequence[Sequence[bytes]]):
    """(comp_offset u64[n_loci + 1], comp_base_offset u64[n_comp + 1], the window bytes) of per-locus competitor windows, as
    vlr_fragpileup_set_alt_variants takes them"""
    off = np.zeros(len(competitors) + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in competitors])
    flat = [bytes(w) for c in competitors for w in c]
    boff = np.zeros(len(flat) + 1, np.uint64)
    boff[1:] = np.cumsum([len(w) for w in flat])
    return off, boff, np.frombuffer(b"".join(flat) or b"\0", np.uint8).copy()


def _set_alt_variants(L, competitors):
    """the after_open of a session with competitors"""
    from . import engine
    arrays = competitor_arrays(competitors)

    def after_open(h):
        engine._check(L.vlr_fragpileup_set_alt_variants(h, *(a.ctypes.data for a in arrays)))
    return after_open


def _read_alt(L, h, n_evidences: int):
    """(abi.FRAGPILEUP_ALT_HIT_DTYPE per evidence, abi.FragPileupAltCounts) of a collected session with competitors"""
    import ctypes as C
    from . import engine
    ah = np.zeros(n_evidences, abi.FRAGPILEUP_ALT_HIT_DTYPE)
    ac = abi.FragPileupAltCounts()
    engine._check(L.vlr_fragpileup_alt_result(h, C.byref(ac)))
    if n_evidences:
        engine._check(L.vlr_fragpileup_read_alt_variants(h, ah.ctypes.data, n_evidences))
    return ah, ac


def _session(L, open_call, args_of, caps, bams, retry: bool, realigning: bool, read, after_open=None):
    """One fragment session run to its result: open_call(*args_of(member, name, key, evidence capacity), the handle), every BAM added,
    abi.FragPileupCounts (and abi.FragPileupRealignCounts of a `realigning` session) read, FragPileupError for damaged guards; an
    overflow of a capacity is retried once with the needed ones while `retry`; then what read(handle, counts, realign counts, fits)
    returns — fits: no capacity overflowed.  `after_open(handle)` runs before the first BAM is added.  The session is closed whatever
    happens."""
    import ctypes as C
    from . import engine
    mcap, ncap, kcap, ecap = caps
    while True:
        h = C.c_void_p()
        engine._check(open_call(*args_of(mcap, ncap, kcap, ecap), C.byref(h)))
        try:
            if after_open is not None:
                after_open(h)
            for b in [bams] if isinstance(bams, str) else bams:
                engine._check(L.vlr_fragpileup_add_bam(h, b.encode()))
            res = abi.FragPileupCounts()
            engine._check(L.vlr_fragpileup_result(h, C.byref(res)))
            if res.status & abi.FRAGPILEUP_GUARD_DAMAGED:
                raise FragPileupError("the guard words behind a buffer of the fragment session changed")
            rres = abi.FragPileupRealignCounts()
            if realigning:
                engine._check(L.vlr_fragpileup_realign_result(h, C.byref(rres)))
            over = abi.FRAGPILEUP_ANY_OVERFLOW | abi.FRAGPILEUP_EVIDENCE_OVERFLOW
            if res.status & over and retry:
                mcap, ncap, kcap = max(mcap, int(res.needed_members)), max(ncap, int(res.needed_name_bytes)), max(kcap, int(res.needed_keys))
                ecap = max(ecap, int(rres.needed_evidences))
                retry = False
                continue
            return read(h, res, rres, not res.status & over)
        finally:
            L.vlr_fragpileup_close(h)


def device_observations(bams, loci: Sequence[Locus], props: Props, device: int = 0, realign_indel_reads: bool = False, member_capacity: Optional[int] = None,
                        name_capacity: Optional[int] = None, window_bytes: int = 0, retry: bool = True, key_capacity: Optional[int] = None,
                        realign: Optional[RealignSpec] = None, fasta: Optional[str] = None, evidence_capacity: Optional[int] = None, pair_byte_limit: int = 0,
                        evidences: bool = False, competitors: Optional[Sequence[Sequence[bytes]]] = None):
    """(observations as abi.FRAGPILEUP_OBS_DTYPE, locus records as abi.FRAGPILEUP_LOCUS_DTYPE, abi.FragPileupCounts) from the kernels.
    `bams`: a path or several (one record stream: a pair may straddle two files); `loci` sorted by (ref_id, start), MNVs of at most
    basecalls.MAX_LEN bases.  An overflow of a capacity is retried once with the needed ones unless retry=False.
    `realign` (with `fasta`): indel-bearing reads are realigned in the same pass (vlr_fragpileup_open_realign; realign_indel_reads is
    implied); evidences=True adds (the realigned evidences as abi.INDELPILEUP_HIT_DTYPE, record-major; abi.FragPileupRealignCounts) to
    the result.  `competitors` (with `realign`): per locus the allele windows of the other candidates at its position
    (vlr_fragpileup_set_alt_variants); with evidences=True the result then also has (abi.FRAGPILEUP_ALT_HIT_DTYPE per evidence,
    abi.FragPileupAltCounts)."""
    from . import engine
    L = engine.lib()
    n = len(loci)
    if competitors is not None and realign is None:
        raise ValueError("competitors need a RealignSpec: without realignment the other alleles of a locus have no effect")
    arrays = basecalls.locus_arrays(loci)
    head = (int(device), n) + tuple(a.ctypes.data for a in arrays) + (int(bool(realign_indel_reads or realign is not None)), int(props.window), int(props.max_mapq),
                                                                     int(props.max_read_len))
    caps = _capacities(n, member_capacity, name_capacity, key_capacity) + (int(evidence_capacity) if evidence_capacity is not None else 1 << 14,)
    if realign is not None:
        from . import realign as rl
        from .readwindows import MODES
        if fasta is None:
            raise ValueError("realignment needs the reference (fasta)")
        gap = (realign.gap or rl.GapParams()).as_array()
        hop = (realign.hop or rl.HopParams()).as_array() if realign.mode == "homopolymer" else None
        score = (fasta.encode(), int(realign.window), MODES[realign.mode], gap, hop)

    def args_of(mcap, ncap, kcap, ecap):
        args = head + (mcap, ncap, kcap, int(window_bytes))
        return args if realign is None else args + score + (ecap, int(pair_byte_limit))

    def read(h, res, rres, fits):
        obs = np.zeros(int(res.n_obs), abi.FRAGPILEUP_OBS_DTYPE)
        loc = np.zeros(n, abi.FRAGPILEUP_LOCUS_DTYPE)
        if fits:
            engine._check(L.vlr_fragpileup_read(h, obs.ctypes.data, len(obs), loc.ctypes.data, n))
        if not evidences:
            return obs, loc, res
        ev = np.zeros(int(rres.n_evidences), abi.INDELPILEUP_HIT_DTYPE)
        if realign is not None and len(ev):    # (not under `fits`, unlike the indel session's: after an overflow a session reports no evidences)
            engine._check(L.vlr_fragpileup_read_realigned(h, ev.ctypes.data, len(ev)))
        if competitors is not None:
            return (obs, loc, res, ev, rres) + _read_alt(L, h, len(ev))
        return obs, loc, res, ev, rres
    return _session(L, L.vlr_fragpileup_open if realign is None else L.vlr_fragpileup_open_realign, args_of, caps, bams, retry, realign is not None, read,
                    _set_alt_variants(L, competitors) if competitors is not None else None)


def _locus_slices(bam: str, res, lrec):
    """What the locus records of a session say: FragPileupError for a malformed record of `bam`; then (the loci that go to the restatement,
    flagged with too many members or alt loci; per other locus, (its index, the slice of its observations))."""
    if res.status & abi.FRAGPILEUP_BAD_RECORD:
        raise FragPileupError("%s: record %d is malformed" % (bam, int(res.first_bad_record)))
    deep = abi.FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS | abi.FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI
    flagged = [j for j in range(len(lrec)) if lrec[j]["status"] & deep]
    return flagged, [(j, slice(int(lrec[j]["obs_offset"]), int(lrec[j]["obs_offset"]) + int(lrec[j]["n_obs"]))) for j in range(len(lrec)) if not lrec[j]["status"] & deep]


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
    prob_sample_alt: Optional[np.ndarray] = None   # an indel candidate (None: ln 1, an SNV / MNV)

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


class _Inputs:
    """what one call of `observations` reads of its files, once: the reference, the contigs of the first BAM's header, and — only when
    a restatement needs them — the records of the BAMs"""
    def __init__(self, bams, fasta):
        from . import alignprops
        self.bams = list(bams)
        self.seqs = read_fasta(fasta)
        contigs, _ = alignprops.bam_header(alignprops.inflate_bgzf(self.bams[0]), self.bams[0])
        self.tid = {name: k for k, (name, _) in enumerate(contigs)}
        self._records: Optional[List[BamRecord]] = None

    def records(self) -> List[BamRecord]:
        if self._records is None:
            self._records = [r for b in self.bams for r in read_bam(b)[1]]
        return self._records


def observations(bam, fasta: str, candidates: Sequence[Tuple[str, int, bytes, bytes]], props, device=0, omit_mapq_adjustment: bool = False,
                 realign_indel_reads: bool = False, window_bytes: int = 0, realign: Optional[RealignSpec] = None,
                 indel_candidates: Optional[RealignSpec] = None, indel_props: Optional[IndelProps] = None, _inputs: Optional["_Inputs"] = None,
                 methylation_readtype: Optional[str] = None, alt_variants: bool = False, _competitors=None) -> List[ObsTable]:
    """Per candidate (contig, 0-based position, REF, ALT), in the order given, its processed pileup.  device="cpu": the restatement; a
    device number: the kernels, finished as the module header says.  `realign`: indel-bearing reads are realigned (module header);
    realign_indel_reads=True without it raises NeedsRealign for such a read.  `indel_candidates`: deletion / insertion candidates
    (REF and ALT of different lengths) are built, every member realigned with this spec, through the indel session (`indel_tables`;
    `indel_props`: what they need of the alignment properties, default: read from `props`); the SNV / MNV candidates of the same call
    go the way they always went.  `methylation_readtype` ("converted" / "annotated"): candidates with ALT <METH> are built through the
    methylation session (methylation.tables); the other candidates of the same call go the way they always went.  `alt_variants`: every
    realigned read is scored against the other candidates at its candidate's position too (the section "the other alleles of a locus"
    above): consecutive candidates with equal (contig, position) form a group."""
    bams = [bam] if isinstance(bam, str) else list(bam)
    inp = _inputs if _inputs is not None else _Inputs(bams, fasta)      # (read once, shared by the SNV / MNV and the indel part of a mixed call)
    seqs, tid = inp.seqs, inp.tid
    comp = _competitors             # per candidate the (contig, position, REF, ALT) of its competitors; None: no alt_variants
    if alt_variants and comp is None:
        comp = [[candidates[j] for j in g] for g in alt_variant_groups(candidates)]
        for c, g in zip(candidates, comp):
            if g and any(bytes(x[3]).startswith(b"<") for x in [c] + g):
                raise PreprocessError("locus %s:%d has a symbolic allele beside other candidates: symbolic alleles do not compete (alt_variants)" % (c[0], c[1] + 1))

    def windows(ks, window):
        """the competitor windows of the candidates `ks`, for a session that realigns with `window`"""
        if comp is None:
            return None
        return [[competitor_window(seqs[c], int(pos), ref, alt, window) for c, pos, ref, alt in comp[k]] for k in ks]
    meth = [k for k, c in enumerate(candidates) if bytes(c[3]) == b"<METH>"]
    if meth:
        from . import methylation
        if methylation_readtype is None:
            raise ValueError("candidate %s:%d is a methylation candidate (methylation_readtype builds them)" % (candidates[meth[0]][0], candidates[meth[0]][1] + 1))
        meth_set = set(meth)
        rest = [k for k in range(len(candidates)) if k not in meth_set]
        out: List[Optional[ObsTable]] = [None] * len(candidates)
        if rest:
            for k, tab in zip(rest, observations(bam, fasta, [candidates[k] for k in rest], props, device, omit_mapq_adjustment, realign_indel_reads, window_bytes, realign,
                                                 indel_candidates, indel_props, _inputs=inp, _competitors=[comp[k] for k in rest] if comp is not None else None)):
                out[k] = tab
        loci = []
        for k in meth:
            c, pos = candidates[k][0], int(candidates[k][1])
            if c not in tid or c not in seqs:
                raise ValueError("contig %s is not in the BAM header and the reference" % c)
            loci.append(methylation.MethLocus(tid[c], pos))
        for k, tab in zip(meth, methylation.tables(bams, loci, props_of(props), methylation_readtype, device, omit_mapq_adjustment, window_bytes, records=inp.records)):
            out[k] = tab
        return out
    ind = [k for k, c in enumerate(candidates) if len(c[2]) != len(c[3])]
    if ind:
        if indel_candidates is None:
            raise ValueError("candidate %s:%d is not an SNV or MNV (indel_candidates builds deletions and insertions)" % (candidates[ind[0]][0], candidates[ind[0]][1] + 1))
        ip = indel_props if indel_props is not None else indel_props_of(props)
        ind_set = set(ind)
        rest = [k for k in range(len(candidates)) if k not in ind_set]
        out: List[Optional[ObsTable]] = [None] * len(candidates)
        if rest:
            for k, tab in zip(rest, observations(bam, fasta, [candidates[k] for k in rest], props, device, omit_mapq_adjustment, realign_indel_reads, window_bytes, realign,
                                                 _inputs=inp, _competitors=[comp[k] for k in rest] if comp is not None else None)):
                out[k] = tab
        sites, what = [], []
        for k in ind:
            c, pos, ref, alt = candidates[k]
            if c not in tid or c not in seqs:
                raise ValueError("contig %s is not in the BAM header and the reference" % c)
            what.append("%s:%d %s>%s" % (c, pos + 1, bytes(ref).decode(), bytes(alt).decode()))
            sites.append(indel_site(seqs[c], tid[c], int(pos), ref, alt, indel_candidates.window, what[-1]))
        ref_seqs = {tid[c]: seqs[c].upper() for c in set(candidates[k][0] for k in ind)}
        for k, tab in zip(ind, indel_tables(bams, fasta, sites, what, props_of(props), ip, indel_candidates, device, omit_mapq_adjustment, window_bytes, ref_seqs,
                                           records=inp.records, competitors=windows(ind, indel_candidates.window))):
            out[k] = tab
        return out
    props = props_of(props)
    loci = []
    for c, pos, ref, alt in candidates:
        if c not in tid or c not in seqs:
            raise ValueError("contig %s is not in the BAM header and the reference" % c)
        loci.append(basecalls.locus(seqs[c], tid[c], int(pos), ref, alt))
    ref_seqs = {tid[c]: seqs[c].upper() for c in set(c for c, _, _, _ in candidates)} if realign is not None else None
    order = sorted(range(len(loci)), key=lambda k: (loci[k].ref_id, loci[k].start))
    records = inp.records
    out: List[Optional[ObsTable]] = [None] * len(loci)
    # (without a RealignSpec the other alleles of an SNV / MNV locus have no effect: snv.rs:87-143 never looks at them)
    cw = windows(range(len(loci)), realign.window) if realign is not None else None
    if device == "cpu":
        t = basecalls.TABLES
        rs = restate(records(), [loci[k] for k in order], props, t, realign_indel_reads, realign=realign, ref_seqs=ref_seqs,
                     competitors=[cw[k] for k in order] if cw is not None else None)
        if rs.bad_records:
            raise FragPileupError("%s: record %d is malformed" % (bams[0], rs.bad_records[0]))
        for j, k in enumerate(order):
            out[k] = table_of(rs.per_locus[j], props, t, omit_mapq_adjustment)
        return out
    t = basecalls.library_tables()
    short = [k for k in order if len(loci[k].ref) <= basecalls.MAX_LEN]
    arr, lrec, res = device_observations(bams, [loci[k] for k in short], props, int(device), realign_indel_reads, window_bytes=window_bytes, realign=realign, fasta=fasta,
                                         competitors=[cw[k] for k in short] if cw is not None else None)[:3]
    flagged, slices = _locus_slices(bams[0], res, lrec)
    host = [k for k in order if len(loci[k].ref) > basecalls.MAX_LEN] + [short[j] for j in flagged]
    for j, sl in slices:
        mj = int(lrec[j]["major_read_position"])
        out[short[j]] = table_of(obs_from_array(arr[sl]), props, t, omit_mapq_adjustment, None if mj == abi.BASEPILEUP_NO_READ_POSITION else mj)
    if host:
        rs = restate(records(), [loci[k] for k in host], props, t, realign_indel_reads, realign=realign, ref_seqs=ref_seqs, device=int(device),
                     competitors=[cw[k] for k in host] if cw is not None else None)
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
        cols["prob_sample_alt"].append(np.zeros(n) if s.prob_sample_alt is None else s.prob_sample_alt)
        cols["prob_double_overlap"].append(np.where(s.strand == abi.STRAND_BOTH, 0.0, -np.inf))
        cols["prob_hit_base"].append(s.prob_hit_base)
        cols["flags"].append(abi.pack_flags(s.strand, pack_orientation(s.orientation), s.read_position_major, s.softclipped, s.paired, s.is_max_mapq, s.alt_locus))
        third.append(s.third_allele.astype(np.int32))
    cat = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}
    indel = np.array([len(c[2]) != len(c[3]) for c in candidates], bool)      # (a <METH> candidate too: the locus flags of a precise candidate that is no SNV / MNV)
    meth = np.array([bytes(c[3]) == b"<METH>" for c in candidates], bool)
    snv = np.array([len(c[2]) == 1 for c in candidates], bool) & ~indel
    lf = lf_indel = 0
    for bit in (abi.BIAS_ORIENTATION, abi.BIAS_STRAND, abi.BIAS_POSITION, abi.BIAS_SOFTCLIP, abi.BIAS_ALTLOCUS):
        if not omit_bias_mask & bit:
            lf |= bit
            if bit in (abi.BIAS_STRAND, abi.BIAS_ALTLOCUS):   # what obsfmt.read_observation_vcf sets for a precise indel without a homopolymer length
                lf_indel |= bit
    if not omit_bias_mask & abi.BIAS_ORIENTATION:
        lf |= abi.LOCUS_REMOVE_NONSTANDARD
    loc = {"locus_flags": (np.where(indel, lf_indel, lf).astype(np.uint8) | np.where(snv, abi.LOCUS_HAS_SNV, 0).astype(np.uint8)),
           "variant_type": np.where(meth, abi.VT_OTHER, np.where(indel, abi.VT_INDEL, np.where(snv, abi.VT_SNV, abi.VT_MNV))).astype(np.uint8),
           "ref_base": np.array([bytes(c[2]).upper()[0] if len(c[2]) == 1 and len(c[3]) == 1 else 0 for c in candidates], np.uint8),
           "alt_base": np.array([bytes(c[3]).upper()[0] if len(c[2]) == 1 and len(c[3]) == 1 else 0 for c in candidates], np.uint8)}
    batch = PileupBatch(1, off.astype(np.uint32), {k: (np.asarray(v, np.float32) if k != "flags" else np.asarray(v, np.uint32)) for k, v in cat.items()}, loc)
    return batch, (np.concatenate(third) if third else np.zeros(0, np.int32))


# ---------------------------------------------------------------------------------------------- deletion and insertion candidates
# What the reference runs for a deletion / insertion candidate between the per-read supports (readwindows.py) and the pileup:
#   Deletion::new / centerpoint, fetch loci          deletion.rs:41-85 (start, start + round(len / 2) with f64::round, end - 1)
#   Fetches::push                                    sample.rs:163-178 (merged when locus.start - W <= last.end + W)
#   is_valid_evidence                                deletion.rs:158-197, insertion.rs:139-157
#   allele_support (every member is realigned)       deletion.rs:204-262, insertion.rs:165-204, Realigner::allele_support (mod.rs:161-424)
#   estimate_insert_size                             insert_size.rs:17-45
#   allele_support_isize, isize_pmf, is_within_sd    types/mod.rs:197-240, sampling_bias/fragments.rs:32-44, 147-166
#   prob_sample_alt                                  deletion.rs:264-293, insertion.rs:206-227, sampling_bias/reads.rs, fragments.rs:17-145
#   update_max_cigar_ops_len while reading           types/mod.rs:310, alignment_properties.rs:94-144 (only what is already Some)
# Only deletions whose three fetch loci merge into one fetch are built (`fetches_merge`): membership is then is_member on [start, end).
# The kernels (vlr_fragpileup_open_indel) give members, evidences, fragments with the validity rule, insert sizes, read lengths and
# the per-locus CIGAR maxima; `isize_support`, `prob_sample_alt` and the running maxima need libm and are these functions on both
# paths, so the two agree with ==.  Phi is 0.5 erfc(-x / sqrt 2) from libm where the reference calls GSL's ugaussian_P: unpinned.
# The other alleles of a locus (alt_variants): on request, the section "the other alleles of a locus" above.
# NOT mirrored: the read-inferred third allele, homopolymer_indel_len and the two prob_observable_at_homopolymer_*
# fields (none: the Myers traceback of the `bio` crate), max_depth subsampling, report_fragment_ids, replacements, SVs, breakends,
# deletions with more than one fetch, and — in a file that mixes candidates — what records that are members of SNV / MNV candidates
# only would add to the running maxima.
MAX_INDEL_LEN = abi.FRAGPILEUP_MAX_INDEL_LEN


class UnrealisticIsizeSd(FragPileupError):
    """Error::UnrealisticIsizeSd: an insert-size standard deviation of 0"""


class NonPositiveInsertSize(FragPileupError):
    """the assertion of insert_size.rs:38-42"""


@dataclass
class IndelProps:
    """what an indel candidate needs of the alignment properties beyond Props; the three maxima rise while records are read"""
    insert_size: Optional[Tuple[float, float]]     # (mean, sd)
    max_del_cigar_len: Optional[int]
    max_ins_cigar_len: Optional[int]
    frac_max_softclip: Optional[float]

    def key(self):
        return (self.insert_size, self.max_del_cigar_len, self.max_ins_cigar_len, self.frac_max_softclip)


def indel_props_of(p) -> IndelProps:
    if isinstance(p, IndelProps):
        return p
    g = p.get if isinstance(p, dict) else (lambda k: getattr(p, k, None))
    ins = g("insert_size")
    if ins is not None and not isinstance(ins, tuple):
        ins = (float(ins["mean"]), float(ins["sd"])) if isinstance(ins, dict) else (float(ins.mean), float(ins.sd))
    return IndelProps(ins, g("max_del_cigar_len"), g("max_ins_cigar_len"), g("frac_max_softclip"))


@dataclass
class IndelSite:
    """a deletion / insertion candidate: readwindows.IndelLocus on its contig"""
    ref_id: int
    locus: "object"

    @property
    def kind(self):
        return self.locus.kind

    @property
    def start(self):
        return self.locus.start

    @property
    def end(self):
        return self.locus.end

    @property
    def length(self) -> int:
        """enclosable_len: the deleted / the inserted bases"""
        return abs(self.locus.len_diff)


def centerpoint(start: int, length: int) -> int:
    """deletion.rs:45: start + (len as f64 / 2.0).round() — f64::round rounds half away from zero, unlike Python's round()"""
    return start + (length + 1) // 2


def fetches_merge(start: int, end: int, window: int) -> bool:
    """do the three fetch loci of the deletion [start, end) merge into one fetch (Fetches::push)?"""
    c = centerpoint(start, end - start)
    last_end = start + 1
    for s, e in ((c, c + 1), (end - 1, end)):
        if max(s - window, 0) > last_end + window:
            return False
        last_end = e
    return True


def clips(rec: BamRecord) -> Tuple[int, int, int, int]:
    """(leading soft, leading hard, trailing soft, trailing hard) as rust-htslib counts them: a soft clip behind one hard clip counts"""
    c = rec.cigar
    if not c:
        return 0, 0, 0, 0
    lh = c[0][1] if c[0][0] == "H" else 0
    first = (c[1] if len(c) > 1 else None) if lh or c[0][0] == "H" else c[0]
    th = c[-1][1] if c[-1][0] == "H" else 0
    last = (c[-2] if len(c) > 1 else None) if th or c[-1][0] == "H" else c[-1]
    return (first[1] if first and first[0] == "S" else 0), lh, (last[1] if last and last[0] == "S" else 0), th


def estimate_insert_size(left: BamRecord, right: BamRecord) -> int:
    """insert_size.rs:17-45 as written; the caller raises for a value <= 0"""
    def aln(r):
        ls, lh, ts, th = clips(r)
        return max(r.pos - (ls + lh), 0), r.end_pos() + ts + th
    (l0, l1), (r0, r1) = aln(left), aln(right)
    return (r0 - l1) + (l1 - l0) + (r1 - r0)


def ugaussian_p(x: float) -> float:
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def isize_pmf(value: float, mean: float, sd: float) -> float:
    """sampling_bias/fragments.rs:164-166: the difference of two Phi values, as written (its underflow to ln 0 is what isize_support keys on)"""
    d = ugaussian_p((value + 0.5 - mean) / sd) - ugaussian_p((value - 0.5 - mean) / sd)
    return math.log(d) if d > 0.0 else -math.inf


def isize_support(insert_size: int, length: int, ip: IndelProps) -> Tuple[float, float]:
    """(ln P(insert size | ref), ln P(insert size | alt)) of allele_support_isize (types/mod.rs:197-240)"""
    mean, sd = ip.insert_size
    if sd == 0.0:
        raise UnrealisticIsizeSd("the insert size standard deviation of the alignment properties is 0")
    p_ref = isize_pmf(float(insert_size), mean, sd)
    p_alt = isize_pmf(float(insert_size), mean + float(length), sd)

    def within_sd(shift):
        return abs(float(insert_size) - (mean + shift)) <= sd
    if (p_ref == -math.inf and not within_sd(float(length))) or (p_alt == -math.inf and not within_sd(0.0)):
        return 0.0, 0.0
    return p_ref, p_alt


def feasible_bases(site: IndelSite, read_len: int, ip: IndelProps) -> Optional[int]:
    """deletion.rs:95-110, insertion.rs:102-117"""
    maxlen = ip.max_del_cigar_len if site.kind == "deletion" else ip.max_ins_cigar_len
    if maxlen is not None and site.length <= maxlen:
        return read_len
    return None if ip.frac_max_softclip is None else int(read_len * ip.frac_max_softclip)


def prob_sample_alt_read(site: IndelSite, read_len: int, ip: IndelProps) -> float:
    """sampling_bias/reads.rs:20-40"""
    feasible = feasible_bases(site, read_len, ip)
    if feasible is None:
        return 0.0
    n_alt = min(site.length, read_len)
    n_alt_valid = min(n_alt, feasible)
    return (math.log(n_alt_valid) if n_alt_valid else -math.inf) - (math.log(n_alt) if n_alt else -math.inf)


def isize_pmf_range(ip: IndelProps) -> range:
    """fragments.rs:20-29 (f64::round: half away from zero)"""
    mean, sd = ip.insert_size
    m = int(math.floor(abs(mean) + 0.5)) if mean >= 0 else 0
    s = int(math.ceil(sd)) * 6
    return range(max(m - s, 0), m + s)


def expected_prob_sample_alt(left_len: int, right_len: int, left_feasible: int, right_feasible: int, delta_ref: int, delta_alt: int, enclose_only: bool,
                             ip: IndelProps) -> float:
    """fragments.rs:47-116"""
    inf_l, inf_r = max(left_len - left_feasible, 0), max(right_len - right_feasible, 0)
    if not enclose_only:
        inf_l, inf_r = max(inf_l - left_feasible, 0), max(inf_r - right_feasible, 0)
    infeasible_read_pos = inf_l + inf_r
    mean, sd = ip.insert_size
    ps = []
    for x in isize_pmf_range(ip):
        internal = max(max(x - left_len, 0) - right_len, 0)
        infeasible_alt = infeasible_read_pos + max(internal + 1 - delta_alt, 0)
        infeasible_ref = max(internal + 1 - delta_ref, 0)
        valid_alt = max(max(x - delta_alt, 0) - infeasible_alt, 0)
        valid_ref = max(x - infeasible_ref, 0)
        if x <= delta_alt or x <= delta_alt + infeasible_alt or x <= infeasible_ref:
            continue
        ps.append(isize_pmf(float(x), mean, sd) + (math.log(valid_alt) - math.log(valid_ref)))
    p = basecalls.ln_sum_exp(ps)
    if p > 0.0:                         # cap_numerical_overshoot(NUMERICAL_EPSILON = 1e-3)
        if p > 1e-3:
            raise FragPileupError("expected_prob_sample_alt: ln probability %g above 0" % p)
        p = 0.0
    return p


def prob_sample_alt(site: IndelSite, len_left: int, len_right: Optional[int], ip: IndelProps, memo: Optional[Dict] = None) -> float:
    """deletion.rs:264-293, insertion.rs:206-227; len_right = None for a single read.  `memo`: {(len_left, len_right): value} of one
    candidate under one state of the properties"""
    key = (len_left, len_right)
    if memo is not None and key in memo:
        return memo[key]
    if len_right is None:
        p = prob_sample_alt_read(site, len_left, ip)
    elif site.kind == "deletion" and ip.insert_size is not None:
        lf, rf = feasible_bases(site, len_left, ip), feasible_bases(site, len_right, ip)
        p = expected_prob_sample_alt(len_left, len_right, lf, rf, site.length, 0, True, ip) if lf is not None and rf is not None else -math.inf
    else:
        one = basecalls.ln_one_minus_exp
        p = one(one(prob_sample_alt_read(site, len_left, ip)) + one(prob_sample_alt_read(site, len_right, ip)))
    if memo is not None:
        memo[key] = p
    return p


def cigar_maxima(rec: BamRecord) -> Tuple[int, int, int]:
    """(longest D, longest I, largest S) of a record: what update_max_cigar_ops_len looks at"""
    m = {"D": 0, "I": 0, "S": 0}
    for op, l in rec.cigar:
        if op in m and l > m[op]:
            m[op] = l
    return m["D"], m["I"], m["S"]


def clip_frac_greater(a: Tuple[int, int], b: Tuple[int, int]) -> bool:
    """the order of the soft-clip fractions (clip, l_seq): by the fraction, then by the clip; l_seq == 0 is the least"""
    if a[1] == 0:
        return False
    if b[1] == 0:
        return True
    x, y = a[0] * b[1], b[0] * a[1]
    return x > y if x != y else a[0] > b[0]


def raised(ip: IndelProps, max_del: int, max_ins: int, clip: Tuple[int, int]) -> IndelProps:
    """the properties after the members of a locus were read: each maximum rises only where it is already Some (`initial` is false)"""
    frac = ip.frac_max_softclip
    if frac is not None and clip[1] > 0:
        frac = max(frac, clip[0] / clip[1])
    return IndelProps(ip.insert_size, None if ip.max_del_cigar_len is None else max(ip.max_del_cigar_len, max_del),
                      None if ip.max_ins_cigar_len is None else max(ip.max_ins_cigar_len, max_ins), frac)


@dataclass
class IndelObs:
    """a fragment observation of an indel locus before the host-side terms: FragObs and what the side record carries"""
    obs: FragObs
    insert_size: int                 # 0 = none
    len_left: int
    len_right: int                   # 0 for a single read
    flags: int = 0

    def key(self):
        return self.obs.key() + (self.insert_size, self.len_left, self.len_right, self.flags)


def indel_evidence(rec: BamRecord, site: IndelSite, li: int, ordinal: int, ref_seq: bytes, window: int) -> RealignEvidence:
    """the windows of a member of an indel locus: realign_evidence with the locus's own alt allele window"""
    from . import readwindows as rw
    from . import realign
    flag = rec.flag & (0x1 | 0x10 | 0x40)

    def refused(status):
        return RealignEvidence(li, rw.Evidence(ordinal, status, (0, 0), (0, 0), b"", b"", b"", flag, rec.mapq), b"")
    try:
        reg = rw.candidate_region(rec, site.start, site.end, len(ref_seq), window)
    except ValueError:
        return refused(rw.LEADING_REFSKIP)
    if basecalls.aux_tag_strand_info(rec) is not None:
        return refused(abi.INDELPILEUP_HIT_STRAND_INFO)
    ro, re_ = reg.read_interval
    if not reg.overlap or re_ - ro < 1:
        return refused(rw.NO_OVERLAP)
    rb, re2 = reg.ref_interval
    rb = min(rb, re2)
    return RealignEvidence(li, rw.Evidence(ordinal, 0, (ro, re_), (rb, re2), rec.seq[ro:re_].upper(), bytes(rec.qual[ro:re_]),
                                           realign.ref_allele(ref_seq, rb, re2).upper(), flag, rec.mapq), bytes(site.locus.alt_allele))


def indel_fragment_observation(left: Tuple[int, BamRecord], right: Optional[Tuple[int, BamRecord]], site: IndelSite, li: int, max_mapq: int,
                               has_insert_size: bool, hits: Dict) -> Optional[IndelObs]:
    """is_valid_evidence and evidence_to_observation of a deletion / insertion for one candidate fragment; `hits`: {(ordinal, locus):
    Hit} of the realigned members (realigned_hit).  The insert-size term is not in it: isize_support adds it."""
    from .readwindows import overlaps
    lo, lr = left
    with_isize = right is not None and site.kind == "deletion" and has_insert_size
    if right is not None:
        if lr.mapq == 0 or right[1].mapq == 0:
            return None
        if not overlaps(lr, site.start, site.end) and not overlaps(right[1], site.start, site.end):
            return None
        if with_isize:
            c = centerpoint(site.start, site.end - site.start)
            if not (lr.pos < c and right[1].end_pos() > c):
                return None
    elif not overlaps(lr, site.start, site.end):
        return None
    h = hits[(lo, li)]
    if right is not None:
        h = basecalls.merge(h, hits[(right[0], li)])
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
    ob = FragObs(h.prob_ref, h.prob_alt, lo, right[0] if right is not None else None, None, 0, sum(len(r.seq) for r in recs), min_mapq, orient, h.strand,
                 any(softclipped(r) for r in recs), bool(lr.flag & 0x1), min_mapq == max_mapq, any(has_xa(r) for r in recs), status,
                 [a for r in recs for a in alt_loci(r)])
    isz = estimate_insert_size(lr, right[1]) if with_isize else 0
    return IndelObs(ob, isz, len(lr.seq), len(right[1].seq) if right is not None else 0, abi.FRAGPILEUP_INDEL_NONPOSITIVE_ISIZE if with_isize and isz <= 0 else 0)


@dataclass
class IndelRestated:
    per_locus: List[List[IndelObs]]
    n_members: List[int]
    maxima: List[Tuple[int, int, Tuple[int, int]]]          # per locus (max D, max I, (clip, l_seq))
    evidences: List[RealignEvidence]                        # record-major, loci ascending within a record
    n_records: int = 0
    n_rejected: int = 0
    bad_records: List[int] = field(default_factory=list)


def restate_indel(records: Sequence[BamRecord], sites: Sequence[IndelSite], props: Props, has_insert_size: bool, spec: RealignSpec, ref_seqs: Dict[int, bytes],
                  device="cpu", first_ordinal: int = 0, competitors: Optional[Sequence[Sequence[bytes]]] = None) -> IndelRestated:
    """The fragment observations of deletion / insertion loci (sorted by (ref_id, start)) from `records` in file order, before the
    host-side terms: what the indel session of the kernels computes, restated.  `competitors`: per site the allele windows of the
    other candidates at its position (alt_variants)."""
    out = IndelRestated([[] for _ in sites], [0] * len(sites), [(0, 0, (0, 0))] * len(sites), [], len(records))
    good = []
    for k, rec in enumerate(records):
        if not basecalls.is_valid_record(rec.flag):
            out.n_rejected += 1
        elif basecalls.record_is_bad(rec):
            out.bad_records.append(first_ordinal + k)
        elif rec.ref_id >= 0 and rec.pos >= 0:
            good.append((first_ordinal + k, rec))
    recs_of = []
    for o, rec in good:
        for li, site in enumerate(sites):
            if is_member(rec, site, props.window):
                out.evidences.append(indel_evidence(rec, site, li, o, ref_seqs[site.ref_id], spec.window))
                recs_of.append(rec)
    hits = {}
    if competitors is not None:
        score_alt_evidences(out.evidences, competitors, spec, device)
        hits = {(e.ev.record, e.locus): realigned_hit(e, rec) for e, rec in zip(out.evidences, recs_of)}
    else:
        dist, lnp = score_pairs(evidence_pair_batch(out.evidences), spec, device)
        for k, (e, rec) in enumerate(zip(out.evidences, recs_of)):
            e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt = float(lnp[2 * k]), float(lnp[2 * k + 1]), int(dist[2 * k]), int(dist[2 * k + 1])
            hits[(e.ev.record, e.locus)] = realigned_hit(e, rec)
    for li, site in enumerate(sites):
        members = [(o, r) for o, r in good if is_member(r, site, props.window)]
        out.n_members[li] = len(members)
        md, mi, mc = 0, 0, (0, 0)
        cand: Dict[bytes, List] = {}
        for o, rec in members:
            d, i, s = cigar_maxima(rec)
            md, mi = max(md, d), max(mi, i)
            if s and len(rec.seq) and clip_frac_greater((s, len(rec.seq)), mc):
                mc = (s, len(rec.seq))
            name = rec.raw_name if rec.raw_name is not None else rec.qname.encode()
            c = cand.get(name)
            if c is None:
                cand[name] = [(o, rec), None]
                continue
            lf, f = c[0][1].flag, rec.flag
            if (lf & 0x40 and f & 0x40) and (lf & 0x80 and f & 0x80):
                continue
            c[1] = (o, rec)
        out.maxima[li] = (md, mi, mc)
        for name in sorted(cand):
            ob = indel_fragment_observation(cand[name][0], cand[name][1], site, li, props.max_mapq, has_insert_size, hits)
            if ob is not None:
                out.per_locus[li].append(ob)
    return out


def device_indel_observations(bams, sites: Sequence[IndelSite], props: Props, has_insert_size: bool, spec: RealignSpec, fasta: str, device: int = 0,
                              member_capacity: Optional[int] = None, name_capacity: Optional[int] = None, key_capacity: Optional[int] = None,
                              evidence_capacity: Optional[int] = None, window_bytes: int = 0, pair_byte_limit: int = 0, retry: bool = True,
                              competitors: Optional[Sequence[Sequence[bytes]]] = None):
    """(observations abi.FRAGPILEUP_OBS_DTYPE, their side records abi.FRAGPILEUP_INDEL_OBS_DTYPE, locus records abi.FRAGPILEUP_LOCUS_DTYPE,
    per-locus maxima abi.FRAGPILEUP_INDEL_LOCUS_DTYPE, abi.FragPileupCounts, evidences abi.INDELPILEUP_HIT_DTYPE record-major,
    abi.FragPileupRealignCounts) from the kernels (vlr_fragpileup_open_indel).  `sites` sorted by (ref_id, start).  An overflow of a
    capacity is retried once with the needed ones unless retry=False.  `competitors`: per site the allele windows of the other
    candidates at its position (vlr_fragpileup_set_alt_variants); the result then also has (abi.FRAGPILEUP_ALT_HIT_DTYPE per evidence,
    abi.FragPileupAltCounts)."""
    from . import engine
    from . import realign as rl
    from .readwindows import MODES, locus_arrays
    L = engine.lib()
    n = len(sites)
    arrays = locus_arrays([s.ref_id for s in sites], [s.locus for s in sites])
    caps = _capacities(n, member_capacity, name_capacity, key_capacity)
    caps += (int(evidence_capacity) if evidence_capacity is not None else caps[0],)
    gap = (spec.gap or rl.GapParams()).as_array()
    hop = (spec.hop or rl.HopParams()).as_array() if spec.mode == "homopolymer" else None
    head = (int(device), n) + tuple(a.ctypes.data for a in arrays) + (int(props.window), int(props.max_mapq), int(props.max_read_len))
    score = (fasta.encode(), int(spec.window), MODES[spec.mode], gap, hop)

    def args_of(mcap, ncap, kcap, ecap):
        return head + (mcap, ncap, kcap, int(window_bytes)) + score + (ecap, int(pair_byte_limit), int(bool(has_insert_size)))

    def read(h, res, rres, fits):
        obs = np.zeros(int(res.n_obs), abi.FRAGPILEUP_OBS_DTYPE)
        obx = np.zeros(int(res.n_obs), abi.FRAGPILEUP_INDEL_OBS_DTYPE)
        loc = np.zeros(n, abi.FRAGPILEUP_LOCUS_DTYPE)
        lox = np.zeros(n, abi.FRAGPILEUP_INDEL_LOCUS_DTYPE)
        ev = np.zeros(int(rres.n_evidences), abi.INDELPILEUP_HIT_DTYPE)
        if fits:
            engine._check(L.vlr_fragpileup_read(h, obs.ctypes.data, len(obs), loc.ctypes.data, n))
            engine._check(L.vlr_fragpileup_read_indel(h, obx.ctypes.data, len(obx), lox.ctypes.data, n))
            if len(ev):
                engine._check(L.vlr_fragpileup_read_realigned(h, ev.ctypes.data, len(ev)))
        if competitors is not None:
            return (obs, obx, loc, lox, res, ev, rres) + _read_alt(L, h, len(ev) if fits else 0)
        return obs, obx, loc, lox, res, ev, rres
    return _session(L, L.vlr_fragpileup_open_indel, args_of, caps, bams, retry, True, read, _set_alt_variants(L, competitors) if competitors is not None else None)


def indel_obs_from_arrays(a: np.ndarray, x: np.ndarray) -> List[IndelObs]:
    return [IndelObs(o, int(r["insert_size"]), int(r["len_left"]), int(r["len_right"]), int(r["flags"])) for o, r in zip(obs_from_array(a), x)]


def indel_table_of(obs: Sequence[IndelObs], site: IndelSite, props: Props, ip: IndelProps, t: Tables, omit_mapq_adjustment: bool = False) -> ObsTable:
    """The processed pileup of an indel candidate from its fragment observations: the insert-size term merged into the supports
    (deletion.rs:253-257: strand none, so nothing else changes), prob_sample_alt, then `process` as for every candidate.  `ip`: the
    properties after this candidate's members were read."""
    memo: Dict = {}
    finished, psa = [], []
    for io in obs:
        o = io.obs
        if o.status & REALIGN_STRAND_INFO:     # (every member of an indel candidate is realigned, with or without an indel operation of its own)
            raise RealignStrandInfo("record %d%s carries an SI:Z tag: REALIGN_STRAND_INFO (every record at an indel candidate is realigned, and strand "
                                    "information over the realigned interval is not built)" % (o.left, "" if o.right is None else " or its mate, record %d," % o.right))
        raise_for_status(o)
        if io.flags & abi.FRAGPILEUP_INDEL_NONPOSITIVE_ISIZE:
            raise NonPositiveInsertSize("bug: insert size %d is smaller than zero (records %d and %d)" % (io.insert_size, o.left, o.right))
        if io.insert_size:
            p_ref, p_alt = isize_support(io.insert_size, site.length, ip)
            o = FragObs(o.prob_ref + p_ref, o.prob_alt + p_alt, *o.key()[2:], alt_loci=o.alt_loci, alt_locus=o.alt_locus)
        finished.append(o)
        psa.append(prob_sample_alt(site, io.len_left, io.len_right if o.right is not None else None, ip, memo))
    tab = table_of(finished, props, t, omit_mapq_adjustment, None)
    tab.prob_sample_alt = np.array(psa, float)
    return tab


def indel_site(seq: bytes, ref_id: int, pos: int, ref: bytes, alt: bytes, window: int, what: str) -> IndelSite:
    """the deletion / insertion candidate `what` (for messages), or the refusal that names it"""
    from .readwindows import indel_locus
    loc = indel_locus(seq.upper(), pos, ref, alt, window)
    if loc.kind == "replacement":
        raise PreprocessError("candidate %s is a replacement: only deletions (ALT = the first base of REF) and insertions (REF = the first base of ALT) are built" % what)
    if loc.end - loc.start > MAX_INDEL_LEN or abs(loc.len_diff) > MAX_INDEL_LEN:
        raise PreprocessError("candidate %s: an indel of %d bases is longer than the %d a fragment session takes" % (what, abs(loc.len_diff), MAX_INDEL_LEN))
    return IndelSite(ref_id, loc)


def indel_tables(bams, fasta: str, sites: Sequence[IndelSite], what: Sequence[str], props: Props, ip: IndelProps, spec: RealignSpec, device=0,
                 omit_mapq_adjustment: bool = False, window_bytes: int = 0, ref_seqs: Optional[Dict[int, bytes]] = None, records=None,
                 competitors: Optional[Sequence[Sequence[bytes]]] = None) -> List[ObsTable]:
    """Per deletion / insertion candidate, in the order given (the order of the candidate file: the running maxima follow it), its
    processed pileup.  device="cpu": the restatement with the CPU pair HMMs; a device number: the kernels.  `competitors`: per site, in
    the order given, the allele windows of the other candidates at its position (alt_variants)."""
    for s, w in zip(sites, what):
        if s.kind == "deletion" and not fetches_merge(s.start, s.end, props.window):
            raise PreprocessError("candidate %s: the three fetch loci of the deletion (start, centerpoint, end - 1) do not merge into one fetch with a window of %d; "
                                  "deletions with more than one fetch are not built" % (w, props.window))
    order = sorted(range(len(sites)), key=lambda k: (sites[k].ref_id, sites[k].start))
    sorted_sites = [sites[k] for k in order]
    sorted_comp = [competitors[k] for k in order] if competitors is not None else None
    has_isize = ip.insert_size is not None
    per: List[Optional[List[IndelObs]]] = [None] * len(sites)
    maxima: List = [None] * len(sites)
    t = basecalls.TABLES if device == "cpu" else basecalls.library_tables()
    host = list(range(len(order)))
    if device != "cpu":
        obs, obx, loc, lox, res = device_indel_observations(bams, sorted_sites, props, has_isize, spec, fasta, int(device), window_bytes=window_bytes,
                                                            competitors=sorted_comp)[:5]
        blist = [bams] if isinstance(bams, str) else list(bams)
        host, slices = _locus_slices(blist[0], res, loc)
        if res.status & (abi.FRAGPILEUP_ANY_OVERFLOW | abi.FRAGPILEUP_EVIDENCE_OVERFLOW):
            raise FragPileupError("%s: the members or evidences do not fit the buffers of the fragment session" % blist[0])
        for j, k in enumerate(order):
            maxima[k] = (int(lox[j]["max_del"]), int(lox[j]["max_ins"]), (int(lox[j]["max_clip"]), int(lox[j]["max_clip_l_seq"])))
        for j, sl in slices:
            per[order[j]] = indel_obs_from_arrays(obs[sl], obx[sl])
    if host:   # the restatement: everything on the CPU path, the flagged loci of the device path (scored on the device)
        blist = [bams] if isinstance(bams, str) else list(bams)
        recs = records() if records is not None else [r for b in blist for r in read_bam(b)[1]]      # (`records`: the caller's, read once)
        if ref_seqs is None:
            raise ValueError("the restatement needs the contigs of the loci (ref_seqs)")
        rs = restate_indel(recs, [sorted_sites[j] for j in host], props, has_isize, spec, ref_seqs, device,
                           competitors=[sorted_comp[j] for j in host] if sorted_comp is not None else None)
        if rs.bad_records:
            raise FragPileupError("%s: record %d is malformed" % (blist[0], rs.bad_records[0]))
        for i, j in enumerate(host):
            per[order[j]], maxima[order[j]] = rs.per_locus[i], rs.maxima[i]
    out = []
    for k, site in enumerate(sites):    # candidate order: the properties rise as the reference reads
        ip = raised(ip, *maxima[k])
        out.append(indel_table_of(per[k], site, props, ip, t, omit_mapq_adjustment))
    return out


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
                        score_indel_reads_from_alignment: bool = False, warn=None, realign: Optional[RealignSpec] = None,
                        indel_candidates: Optional[RealignSpec] = None, methylation_readtype: Optional[str] = None, alt_variants: bool = False) -> int:
    """`preprocess variants` for SNV / MNV candidates of one sample: the observation BCF `output` (format v15) that `call variants`
    reads.  Returns the number of records written.  `realign` (--realign-indel-reads): indel-bearing reads over a candidate are
    realigned as the reference does by default; its gap / hop parameters default to those of the alignment properties.
    `indel_candidates` (--indel-candidates): deletion and insertion candidates are built too, one observation per fragment (the
    section "deletion and insertion candidates" above); the file may mix them with SNVs / MNVs, records keep the candidate order.
    `methylation_readtype` (--methylation-read-type converted|annotated): candidates with ALT <METH> are built too (methylation.py);
    without it such a candidate is refused as every symbolic allele is.
    `alt_variants` (--alt-variants): a realigned read is scored against the other ALT alleles at its candidate's (CHROM, POS) as well
    (the section "the other alleles of a locus" above); without it every candidate is scored as if it were alone at its position."""
    import json
    from . import ingest
    if not atomic_candidate_variants:
        raise PreprocessError("--atomic-candidate-variants is required: SNV / MNV candidates are scored from the read's own alignment, as that flag of the "
                              "reference makes it (preprocessing/mod.rs:511, 535); scoring against the other candidates at a locus does not depend on it: --alt-variants")
    sites = read_candidates(candidates)
    if alt_variants:
        alt_variant_groups(sites)         # (a locus with too many alleles is refused before anything is read)
    cands = []
    if methylation_readtype is not None:
        from . import methylation
        if methylation_readtype not in methylation.READTYPES:
            raise PreprocessError("--methylation-read-type must be one of %s" % ", ".join(methylation.READTYPES))
    for chrom, pos, rid, ref, alt in sites:
        if methylation_readtype is not None and alt == "<METH>" and ref:
            cands.append((chrom, pos - 1, ref.encode(), alt.encode()))
            continue
        sym = alt.startswith("<") or "[" in alt or "]" in alt or alt in ("*", ".")
        if indel_candidates is not None and (sym or not ref or not alt):
            raise PreprocessError("candidate %s:%d %s>%s is a symbolic or breakend allele: only SNVs, MNVs, deletions and insertions are built" % (chrom, pos, ref, alt))
        if indel_candidates is None and (sym or len(ref) != len(alt) or not ref):
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
    if indel_candidates is not None and indel_candidates.gap is None and indel_candidates.hop is None:
        indel_candidates = RealignSpec(indel_candidates.window, indel_candidates.mode, *gap_hop_of(pj))
    try:
        tabs = observations(bam, reference, cands, props, device=device, omit_mapq_adjustment=omit_mapq_adjustment,
                            realign_indel_reads=not score_indel_reads_from_alignment, realign=realign, indel_candidates=indel_candidates,
                            indel_props=indel_props_of(pj) if indel_candidates is not None else None, methylation_readtype=methylation_readtype,
                            alt_variants=alt_variants)
    except NeedsRealign as e:
        raise PreprocessError(str(e) + "; --score-indel-reads-from-alignment scores such reads as they are aligned, --realign-indel-reads realigns them") from e
    deep = sum(1 for t in tabs if len(t) > max_depth)
    if deep and warn is not None:
        warn("%d of %d loci have more than --max-depth %d observations; they are processed whole (the reference's subsampling is not built)" % (deep, len(tabs), max_depth))
    batch, third = pileup(tabs, cands)
    ingest.write_observations(output, batch, 0, third_allele_evidence=third, sites=sites)
    return len(sites)
