"""Fragment observations of methylation candidates (ALT <METH>) from BAM records: a CPU restatement of the reference's
variants/types/methylation.rs and the front end of the methylation session of the fragment kernels (vlr_fragpileup_open_methylation;
csrc/vlr_methylation.h states the same rule for the kernels).  Mirrors

  the locus                  [pos, pos + 1) at the candidate's POS, the C of a CpG (:31-39); prob_sample_alt = ln 1 (:464-466); no homopolymer
                             model, no third allele
  read_reverse_orientation   :486-495: unpaired, the reverse flag; paired, (reverse && first) || (!reverse && !first).  A record of reverse
                             orientation is read at pos + 1 (the G), the others at pos (:47-50)
  is_valid_evidence          :393-435: SingleLocus::overlap(read, false, start_offset, 0) == Enclosing with start_offset = 1 for reverse
                             orientation: rec.pos <= start + off and rec.end_pos >= start + 1 (a reverse-orientation record that ends at
                             start + 1 is enclosing and has no base there: enclosing, without support); in an annotated session either
                             record must carry an Mm / MM tag of any type (mm_exists) — implied by a support, see csrc/vlr_methylation.h
  allele_support_per_read    :41-86, process_read :250-275: read_pos(position, false, false); no support for a FLAG outside
                             {0, 16, 83, 99, 147, 163} (read_invalid), for a mutation at the read position (:334-367), for an annotated
                             record without a usable map
  converted reads            :306-324 with basecalls.prob_read_base (the tables of the SNV arm)
  annotated reads            :283-298: ln((ml + 0.5) / 256) and ln(1 - exp of it) from the record's 5mC map, ln 0 / ln 1 outside it
  extract_mm_ml_5mc          :130-221, as written (`mm_map`)
  strand                     Strand::from_record_and_pos when prob_ref != prob_alt, else none
  read position              Some(qpos) (:72): the position in SEQ, without the leading hard clip the SNV arm adds

The fragment rules (pairing, MAPQ-0 pairs, merge, the strand-none drop, major read position, alt loci) are those of fragments.py, run
with this module's `Rule` in place of the SNV / MNV one.
NOT mirrored: `max_depth` subsampling, `report_fragment_ids`, an MM value that is not UTF-8, and — in an annotated session — the
reference's silence about a CIGAR that begins with N in a fragment without any Mm / MM tag (here it is refused like every such CIGAR).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import abi, basecalls, fragments
from .basecalls import Hit, Tables
from .readwindows import BamRecord, read_pos

CONVERTED, ANNOTATED = "converted", "annotated"
READTYPES = {CONVERTED: abi.METH_CONVERTED, ANNOTATED: abi.METH_ANNOTATED}
VALID_FLAGS = (0, 16, 83, 99, 147, 163)     # read_invalid (:374-376)


@dataclass
class MethTables:
    ln_meth: List[float]       # ln((ml + 0.5) / 256)
    ln_unmeth: List[float]     # ln(1 - exp(ln_meth))


def python_meth_tables() -> MethTables:
    meth = [math.log((ml + 0.5) / 256.0) for ml in range(256)]
    return MethTables(meth, [math.log(1.0 - math.exp(p)) for p in meth])


def library_meth_tables() -> MethTables:
    """the tables an annotated session scores with (vlr_methylation_tables)"""
    import ctypes as C
    from . import engine
    L = engine.lib()
    a, b = (C.c_double * 256)(), (C.c_double * 256)()
    engine._check(L.vlr_methylation_tables(a, b))
    return MethTables(list(a), list(b))


METH_TABLES = python_meth_tables()


@dataclass
class MethLocus:
    ref_id: int
    start: int

    @property
    def end(self) -> int:
        return self.start + 1


def reverse_orientation(flag: int) -> bool:
    paired, reverse, first = bool(flag & 0x1), bool(flag & 0x10), bool(flag & 0x40)
    return (reverse and first) or (not reverse and not first) if paired else reverse


def enclosing(rec: BamRecord, loc: MethLocus) -> bool:
    off = 1 if reverse_orientation(rec.flag) else 0
    return rec.pos >= 0 and rec.pos <= loc.start + off and rec.end_pos() >= loc.start + 1


def mutation_occurred(rev: bool, annotated: bool, base: int) -> bool:
    if rev:
        return base in (b"CAT" if annotated else b"CT")
    return base in (b"GAT" if annotated else b"AG")


def mm_map(rec: BamRecord) -> Optional[Dict[int, int]]:
    """extract_mm_ml_5mc: {read position: ML value} of the record's 5mC calls, None without a usable map"""
    first: Dict[bytes, Tuple[str, bytes]] = {}
    for tag, ty, val in basecalls.aux_fields(rec.aux):
        if tag in (b"Mm", b"MM", b"Ml", b"ML") and tag not in first:
            first[tag] = (ty, val)
    mm = first.get(b"Mm", first.get(b"MM"))
    ml = first.get(b"Ml", first.get(b"ML"))
    if mm is None or ml is None or mm[0] != "Z" or ml[0] != "B" or ml[1][:1] != b"C":
        return None
    text, values = mm[1][:-1], ml[1][5:]
    rev = reverse_orientation(rec.flag)
    out: Dict[int, int] = {}
    ml_index = 0
    for block in text.split(b";"):
        if not block or b"," not in block:
            continue
        header, positions = block.split(b",", 1)
        deltas = [d for d in (fragments._parse_u64(s) for s in positions.split(b",")) if d is not None]
        if header.startswith(b"C+m") or header.startswith(b"C-m"):
            target = ord("G") if rev else ord("C")
            where = [i for i, c in enumerate(rec.seq) if c == target]
            if rev:
                where.reverse()
            meth_pos = 0
            for d in deltas:
                meth_pos += d
                if meth_pos >= len(where):
                    return None
                out[where[meth_pos]] = values[ml_index] if ml_index < len(values) else 0
                ml_index += 1
                meth_pos += 1
        else:
            ml_index += len(deltas)
    return out


@dataclass
class Rule:
    """what fragments.fragment_observation asks of a candidate kind: the enclosing test and the per-read support"""
    readtype: str = CONVERTED
    mt: MethTables = None
    accept_any_flag: bool = False       # switches read_invalid off: only for recordings that predate that rule

    def __post_init__(self):
        if self.readtype not in READTYPES:
            raise ValueError("methylation read type must be one of %s" % ", ".join(READTYPES))
        if self.mt is None:
            self.mt = METH_TABLES
        self._maps: Dict[int, Optional[Dict[int, int]]] = {}

    def enclosing(self, rec: BamRecord, loc: MethLocus) -> bool:
        return enclosing(rec, loc)

    def _map(self, rec: BamRecord, ordinal: int):
        if ordinal not in self._maps:       # (once per record, as the reference caches prob_methylation)
            self._maps[ordinal] = mm_map(rec)
        return self._maps[ordinal]

    def support(self, rec: BamRecord, loc: MethLocus, li: int, ordinal: int, t: Tables) -> Optional[Hit]:
        """allele_support_per_read; what the reference raises comes back as the hit's status"""
        if not enclosing(rec, loc):
            return None
        rev = reverse_orientation(rec.flag)
        flag = rec.flag & (0x1 | 0x10 | 0x40)

        def refused(status):
            return Hit(li, ordinal, 0.0, 0.0, abi.STRAND_NONE, None, 0, rec.mapq, flag, status, (ordinal,))
        try:
            qpos = read_pos(rec, loc.start + (1 if rev else 0), False, False)
        except ValueError:
            return refused(abi.BASEPILEUP_HIT_LEADING_REFSKIP)
        if qpos is None:
            return None
        annotated = self.readtype == ANNOTATED
        base = rec.seq[qpos]
        if annotated:
            m = self._map(rec, ordinal)
            if m is None:
                return None
        if mutation_occurred(rev, annotated, base) or (not self.accept_any_flag and rec.flag not in VALID_FLAGS):
            return None
        if annotated:
            if qpos in m:
                pa, pr = self.mt.ln_meth[m[qpos]], self.mt.ln_unmeth[m[qpos]]
            else:
                pa, pr = -math.inf, 0.0
        else:
            q = rec.qual[qpos]
            pa = basecalls.prob_read_base(base, ord("G") if rev else ord("C"), q, t)
            pr = basecalls.prob_read_base(base, ord("A") if rev else ord("T"), q, t)
        strand = abi.STRAND_NONE
        if pr != pa:
            si = basecalls.aux_tag_strand_info(rec)
            if si is not None:
                if qpos >= len(si):
                    return refused(abi.BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS)
                if si[qpos] not in basecalls.STRAND_OF_ITEM:
                    return refused(abi.BASEPILEUP_HIT_INVALID_STRAND_INFO)
                strand = basecalls.STRAND_OF_ITEM[si[qpos]]
            else:
                strand = abi.STRAND_REVERSE if rec.flag & 0x10 else abi.STRAND_FORWARD
        return Hit(li, ordinal, pr, pa, strand, qpos, 0, rec.mapq, flag, 0, (ordinal,))


def restate(records: Sequence[BamRecord], loci: Sequence[MethLocus], props, readtype: str, t: Tables = basecalls.TABLES, mt: Optional[MethTables] = None,
            accept_any_flag: bool = False, first_ordinal: int = 0, only: Optional[Sequence[int]] = None) -> fragments.Restated:
    """The observations of every methylation locus (`only`: of these) from `records` in file order: fragments.restate under the
    methylation rule.  accept_any_flag=True switches the flag rule `read_invalid` off (recordings made before the reference had it)."""
    return fragments.restate(records, loci, fragments.props_of(props), t, first_ordinal=first_ordinal, only=only, rule=Rule(readtype, mt, accept_any_flag))


def device_observations(bams, loci: Sequence[MethLocus], props, readtype: str, device: int = 0, member_capacity: Optional[int] = None, name_capacity: Optional[int] = None,
                        window_bytes: int = 0, retry: bool = True, key_capacity: Optional[int] = None):
    """(observations as abi.FRAGPILEUP_OBS_DTYPE, locus records as abi.FRAGPILEUP_LOCUS_DTYPE, abi.FragPileupCounts) of a methylation
    session of the kernels.  `loci` sorted by (ref_id, start).  An overflow of a capacity is retried once with the needed ones unless
    retry=False."""
    from . import engine
    if readtype not in READTYPES:
        raise ValueError("methylation read type must be one of %s" % ", ".join(READTYPES))
    props = fragments.props_of(props)
    L = engine.lib()
    n = len(loci)
    ref_id = np.array([l.ref_id for l in loci], np.int32)
    start = np.array([l.start for l in loci], np.int64)
    head = (int(device), n, ref_id.ctypes.data, start.ctypes.data, READTYPES[readtype], int(props.window), int(props.max_mapq), int(props.max_read_len))
    caps = fragments._capacities(n, member_capacity, name_capacity, key_capacity) + (0,)

    def args_of(mcap, ncap, kcap, ecap):
        return head + (mcap, ncap, kcap, int(window_bytes))

    def read(h, res, rres, fits):
        obs = np.zeros(int(res.n_obs), abi.FRAGPILEUP_OBS_DTYPE)
        loc = np.zeros(n, abi.FRAGPILEUP_LOCUS_DTYPE)
        if fits:
            engine._check(L.vlr_fragpileup_read(h, obs.ctypes.data, len(obs), loc.ctypes.data, n))
        return obs, loc, res
    return fragments._session(L, L.vlr_fragpileup_open_methylation, args_of, caps, bams, retry, False, read)


def tables(bams, loci: Sequence[MethLocus], props, readtype: str, device=0, omit_mapq_adjustment: bool = False, window_bytes: int = 0, records=None,
           accept_any_flag: bool = False) -> List[fragments.ObsTable]:
    """Per methylation locus, in the order given, its processed pileup.  device="cpu": the restatement; a device number: the kernels,
    with the loci they flag (too many members or alt loci) finished by the restatement on the library's tables.  `records`: a callable
    that gives the records of the BAMs (read once by the caller)."""
    from .readwindows import read_bam
    bams = [bams] if isinstance(bams, str) else list(bams)
    props = fragments.props_of(props)
    order = sorted(range(len(loci)), key=lambda k: (loci[k].ref_id, loci[k].start))
    sorted_loci = [loci[k] for k in order]
    out: List[Optional[fragments.ObsTable]] = [None] * len(loci)
    if records is None:
        def records():
            return [r for b in bams for r in read_bam(b)[1]]
    if device == "cpu":
        t, host = basecalls.TABLES, list(range(len(order)))
        mt = METH_TABLES
    else:
        if accept_any_flag:
            raise ValueError("accept_any_flag is a switch of the restatement alone")
        t, mt = basecalls.library_tables(), library_meth_tables()
        arr, lrec, res = device_observations(bams, sorted_loci, props, readtype, int(device), window_bytes=window_bytes)
        if res.status & abi.FRAGPILEUP_ANY_OVERFLOW:
            raise fragments.FragPileupError("%s: the members do not fit the buffers of the fragment session" % bams[0])
        host, slices = fragments._locus_slices(bams[0], res, lrec)
        for j, sl in slices:
            mj = int(lrec[j]["major_read_position"])
            out[order[j]] = fragments.table_of(fragments.obs_from_array(arr[sl]), props, t, omit_mapq_adjustment, None if mj == abi.BASEPILEUP_NO_READ_POSITION else mj)
    if host:
        rs = restate(records(), [sorted_loci[j] for j in host], props, readtype, t, mt, accept_any_flag)
        if rs.bad_records:
            raise fragments.FragPileupError("%s: record %d is malformed" % (bams[0], rs.bad_records[0]))
        for i, j in enumerate(host):
            out[order[j]] = fragments.table_of(rs.per_locus[i], props, t, omit_mapq_adjustment)
    return out
