"""The restatement of the realignment of indel-bearing reads over SNV / MNV candidates (varlociraptor_amd/fragments.py with a RealignSpec,
device="cpu": the windows scored by oracle/'s CPU pair HMMs), no GPU.  Every expectation below follows from the sequences of
tests/fragrealign_cases.py alone: which allele a read spells, not what the code returns."""
import math

import pytest

import fragrealign_cases as rc
from varlociraptor_amd import abi, basecalls, fragments
from varlociraptor_amd import readwindows as rw

SPEC = fragments.RealignSpec()
NONE, FWD, REV, BOTH = abi.STRAND_NONE, abi.STRAND_FORWARD, abi.STRAND_REVERSE, abi.STRAND_BOTH


def run(records, cands, props=rc.P30, spec=SPEC, contigs=None, realign=True):
    """(Restated, loci, parsed records) of encoded records over candidates on the hand contig"""
    import tempfile
    contigs = contigs or {"c1": rc.REF}
    with tempfile.TemporaryDirectory() as tmp:
        bam, _ = rc.bc.write_case(tmp, "case", contigs, records)
        recs = rw.read_bam(bam)[1]
    loci = rc.bc.loci_of(cands, contigs)
    if not realign:
        return fragments.restate(recs, loci, props), loci, recs
    return fragments.restate(recs, loci, props, realign=spec, ref_seqs=rc.ref_seqs_of(contigs)), loci, recs


@pytest.fixture(scope="module")
def hand(oracle):
    recs = rc.hand_records()
    rs, loci, parsed = run(list(recs.values()), [rc.SNV20, rc.MNV40])
    return list(recs), rs, loci, parsed


def obs_of(hand, label, locus=0):
    labels, rs, _, _ = hand
    k = labels.index(label)
    return [o for o in rs.per_locus[locus] if o.left == k]


def test_a_read_that_spells_an_allele_supports_it_whatever_its_alignment_says(hand):
    labels, rs, loci, parsed = hand
    # scored from the alignment the two reads support the wrong allele ...
    plain, _, _ = run([rc.hand_records()["alt_misplaced"], rc.hand_records()["ref_misplaced"]], [rc.SNV20], realign=False)
    a, r = plain.per_locus[0]
    assert a.prob_alt < a.prob_ref and r.prob_alt > r.prob_ref
    # ... realigned, the right one; the strand is the record's, there is no read position and no third-allele evidence
    a, = obs_of(hand, "alt_misplaced")
    r, = obs_of(hand, "ref_misplaced")
    assert a.prob_alt > a.prob_ref and r.prob_ref > r.prob_alt
    assert (a.strand, r.strand) == (FWD, REV) and a.read_position is None and r.read_position is None and a.third_allele == r.third_allele == 0
    assert a.status == r.status == 0


def test_an_uninformative_read_is_dropped_unless_its_mate_carries_a_strand(hand):
    labels, rs, _, _ = hand
    assert obs_of(hand, "uninformative") == []
    e, = [e for e in rs.evidences if e.ev.record == labels.index("uninformative")]
    h = fragments.realigned_hit(e, hand[3][e.ev.record])
    assert h.prob_ref == h.prob_alt and h.strand == NONE
    o, = obs_of(hand, "unin_pair_1")
    assert o.right == labels.index("unin_pair_2") and o.strand == REV and o.prob_alt > o.prob_ref and o.read_position == 5


def test_every_realigned_support_is_normalised(hand):
    labels, rs, _, parsed = hand
    assert len(rs.evidences) == 10
    for e in rs.evidences:
        h = fragments.realigned_hit(e, parsed[e.ev.record])
        assert abs(math.exp(h.prob_ref) + math.exp(h.prob_alt) - 1.0) <= 1e-12, e


def test_mates_merge_as_allele_supports_do(hand):
    labels, rs, _, parsed = hand
    both, = obs_of(hand, "both_1")
    e1, e2 = [e for e in rs.evidences if e.ev.record in (labels.index("both_1"), labels.index("both_2"))]
    h1, h2 = fragments.realigned_hit(e1, parsed[e1.ev.record]), fragments.realigned_hit(e2, parsed[e2.ev.record])
    assert both.right == labels.index("both_2") and both.strand == BOTH and both.read_position is None
    assert (both.prob_ref, both.prob_alt) == (h1.prob_ref + h2.prob_ref, h1.prob_alt + h2.prob_alt) and both.prob_alt > both.prob_ref
    # one mate realigned (ref), one scored base by base (alt): read position from the alt-supporting mate, strand both
    mixed, = obs_of(hand, "mixed_1")
    assert mixed.right == labels.index("mixed_2") and mixed.strand == BOTH and mixed.read_position == 5 and mixed.third_allele == 0


def test_mapq0_single_read_is_kept(hand):
    o, = obs_of(hand, "mapq0")
    assert o.min_mapq == 0 and not o.is_max_mapq and o.prob_alt > o.prob_ref


def test_mnv_with_an_indel_inside_is_realigned(hand):
    labels, rs, loci, parsed = hand
    k = labels.index("mnv_across_D")
    assert basecalls.enclosing(parsed[k], loci[1]) and basecalls.allele_support(parsed[k], loci[1], 1, k, realign_indel_reads=True).status == fragments.NEEDS_REALIGN
    d, = obs_of(hand, "mnv_across_D", 1)
    i, = obs_of(hand, "mnv_alt_with_I", 1)
    assert d.prob_ref > d.prob_alt and d.strand == FWD and i.prob_alt > i.prob_ref and i.strand == REV


def test_refusals_carry_a_status_of_their_own_and_name_the_record(oracle):
    recs = rc.refused_records()
    rs, loci, _ = run(list(recs.values()), [rc.SNV20])
    assert [(e.ev.record, e.ev.status) for e in rs.evidences] == [(1, abi.INDELPILEUP_HIT_LEADING_REFSKIP), (2, abi.INDELPILEUP_HIT_STRAND_INFO)]
    by_left = {o.left: o for o in rs.per_locus[0]}
    assert (by_left[0].status, by_left[1].status, by_left[2].status) == (0, abi.BASEPILEUP_HIT_LEADING_REFSKIP, abi.FRAGPILEUP_OBS_REALIGN_STRAND_INFO)
    props = rc.P30
    with pytest.raises(fragments.LeadingRefSkip, match="record 1"):
        fragments.table_of([by_left[1]], props, basecalls.TABLES)
    with pytest.raises(fragments.RealignStrandInfo, match="record 2"):
        fragments.table_of([by_left[2]], props, basecalls.TABLES)
    # without a spec the read is still only flagged
    flagged, _, _ = run(list(recs.values())[2:], [rc.SNV20], realign=False)
    rs2 = fragments.restate(rw_records(list(recs.values())[2:]), loci, props, realign_indel_reads=True)
    with pytest.raises(fragments.NeedsRealign):
        fragments.table_of(rs2.per_locus[0], props, basecalls.TABLES)


def rw_records(records):
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        bam, _ = rc.bc.write_case(tmp, "case", {"c1": rc.REF}, records)
        return rw.read_bam(bam)[1]


def test_window_edges(oracle):
    n = len(rc.REF)
    edge = rc.edge_records()
    # the read ends at the locus end: read_pos(locus end) is None -> the window is [qs - w, qs + w) around read_pos(20) = 20
    rec, cand = edge["ends_at_locus_end"]
    rs, loci, parsed = run([rec], [cand])
    e, = rs.evidences
    assert rw.read_pos(parsed[0], 21, True, True) is None and rw.read_pos(parsed[0], 20, True, True) == 20
    assert e.ev.status == 0 and e.ev.read_interval == (0, 21) and e.ev.ref_interval == (0, n) and len(e.alt_allele) == n
    # first bases: the ref window [max(0, 2 - 96), 2 + 96), the alt window [0, 2 + 1 + 96) one longer
    rec, cand = edge["first_bases"]
    rs, _, _ = run([rec], [cand], spec=fragments.RealignSpec(64))
    e, = rs.evidences
    assert e.ev.ref_interval == (0, 98) and len(e.alt_allele) == 99 and e.alt_allele[2:3] == b"A" and e.alt_allele[:2] + e.alt_allele[3:] == rc.REF[:2] + rc.REF[3:99]
    o, = rs.per_locus[0]
    assert o.prob_alt > o.prob_ref
    # last bases: ref window [98 - 96, min(98 + 96, n)), alt window to min(99 + 96, n) -- both clamped to the contig, separately
    rec, cand = edge["last_bases"]
    rs, _, _ = run([rec], [cand])
    e, = rs.evidences
    assert e.ev.ref_interval == (2, n) and len(e.alt_allele) == n - 2 and e.alt_allele[96:97] == b"C"
    o, = rs.per_locus[0]
    assert o.prob_alt > o.prob_ref
    # with a window of 20 the two windows of the first case differ in both ends: [0, 32) and [0, 33); of the last: [68, n) both
    rs, _, _ = run([edge["first_bases"][0]], [edge["first_bases"][1]], spec=fragments.RealignSpec(20))
    assert rs.evidences[0].ev.ref_interval == (0, 32) and len(rs.evidences[0].alt_allele) == 33


def test_a_long_read_is_trimmed_to_the_pattern_length(oracle):
    contigs, cand, rec = rc.long_read_case()
    rs, loci, parsed = run([rec], [cand], props=fragments.Props(200, 60, 151), contigs=contigs)
    e, = rs.evidences
    # read_pos(200) = 71, read_pos(201) = 72: [71 - 64, 72 + 64) = [7, 136), 129 bases, exceed 1: floor(1 / 2) = 0 in front, ceil = 1 behind
    assert e.ev.read_interval == (7, 135) and len(e.ev.read_window) == rw.MAX_PATTERN_LEN
    assert e.ev.ref_interval == (200 - 96, 200 + 96) and len(e.alt_allele) == 193


@pytest.mark.parametrize("window", [1, 64])
def test_smallest_and_largest_window(oracle, window):
    rs, _, parsed = run([rc.hand_records()["alt_misplaced"]], [rc.SNV20], spec=fragments.RealignSpec(window))
    e, = rs.evidences
    rw_ = int(window * 1.5)
    # read_pos(20) = 13, read_pos(21) = 14
    assert e.ev.read_interval == (max(0, 13 - window), min(14 + window, 25))
    assert e.ev.ref_interval == (max(0, 20 - rw_), min(20 + rw_, len(rc.REF))) and len(e.alt_allele) == min(21 + rw_, len(rc.REF)) - max(0, 20 - rw_)
    h = fragments.realigned_hit(e, parsed[0])
    assert abs(math.exp(h.prob_ref) + math.exp(h.prob_alt) - 1.0) <= 1e-12
    if window == 64:
        assert h.prob_alt > h.prob_ref
    with pytest.raises(ValueError):
        fragments.RealignSpec(65)
    with pytest.raises(ValueError):
        fragments.RealignSpec(0)


def test_candidate_regions_equal_the_indel_restatement(hand):
    labels, rs, loci, parsed = hand
    for e in rs.evidences:
        loc = loci[e.locus]
        reg = rw.candidate_region(parsed[e.ev.record], loc.start, loc.end, len(rc.REF), SPEC.window)
        assert reg.overlap and reg.read_interval == e.ev.read_interval and reg.ref_interval == e.ev.ref_interval
        # and the indel session's own evidence of the same record over the same interval
        ind = rw.evidence([parsed[e.ev.record]], rc.REF, rw.IndelLocus("replacement", loc.start, loc.end, 0, b""), SPEC.window, first_ordinal=e.ev.record)
        assert ind[0].key() == e.ev.key()


def test_substitution_locus_is_separate_from_indel_locus():
    with pytest.raises(ValueError):
        rw.indel_locus(rc.REF, 20, b"C", b"T")
    with pytest.raises(ValueError):
        rw.substitution_locus(rc.REF, 20, b"CG", b"T")
    loc = rw.substitution_locus(rc.REF, 40, b"TGA", b"CCA", 4)
    assert (loc.start, loc.end, loc.len_diff) == (40, 43, 0) and loc.alt_allele == rc.REF[34:40] + b"CCA" + rc.REF[43:49]


def test_fast_and_homopolymer_modes_run_on_the_cpu(oracle):
    from varlociraptor_amd import realign
    for spec in (fragments.RealignSpec(64, "fast"), fragments.RealignSpec(64, "homopolymer", realign.GapParams(-9.0, -8.0, -1.5, -1.2),
                                                                            realign.HopParams((-6.0,) * 4, (-6.5,) * 4, (-1.0,) * 4, (-1.1,) * 4))):
        rs, _, _ = run([rc.hand_records()["alt_misplaced"], rc.hand_records()["ref_misplaced"]], [rc.SNV20], spec=spec)
        a, r = rs.per_locus[0]
        assert a.prob_alt > a.prob_ref and r.prob_ref > r.prob_alt, spec.mode
        assert (rs.evidences[0].dist_alt, rs.evidences[1].dist_ref) == (0, 0)
