"""varlociraptor_amd/basecalls.py, the CPU restatement of the reference's SNV / MNV allele supports (no GPU): the records and truth
values of the reference's own unit test (variants/types/snv.rs:316-416), one hand-made record per rule (tests/basecall_cases.py), the
mate merge, and the reference testcases under tests/golden/bam/ end to end: restatement -> pileup -> oracle against each testcase's
own `expected:` block."""
import math

import numpy as np
import pytest

import bam_pairs as bp
import basecall_cases as bc
from varlociraptor_amd import abi, basecalls, cli
from varlociraptor_amd.readwindows import read_bam

T = basecalls.TABLES
LN_ANY, LN_CONF = math.log(0.25), math.log(0.3333)


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    """{label: Hit or None per candidate} of the hand records, plus the parsed records"""
    tmp = tmp_path_factory.mktemp("hand")
    recs = bc.hand_records()
    bam, _ = bc.write_case(tmp, "hand", {"c1": bc.HAND_REF}, recs.values())
    loci = bc.loci_of(bc.HAND_CANDIDATES, {"c1": bc.HAND_REF})
    _, parsed = read_bam(bam)
    by = dict(zip(recs, parsed))
    return by, loci


def sup(hand, label, li, **kw):
    by, loci = hand
    return basecalls.allele_support(by[label], loci[li], li, 0, T, **kw)


def test_tables_follow_bases_rs():
    assert T.miscall[0] == 0.0 and T.call[0] == -math.inf
    for q in (1, 3, 4, 10, 30, 93, 255):
        assert T.miscall[q] == -q * math.log(10.0) / 10.0
        assert math.isclose(T.call[q], math.log1p(-10.0 ** (-q / 10.0)), rel_tol=1e-12)
    assert basecalls.prob_read_base(ord("N"), ord("A"), 30) == LN_ANY
    assert basecalls.prob_read_base(ord("C"), ord("A"), 30) == T.miscall[30] + LN_CONF
    assert basecalls.prob_read_base(ord("A"), ord("A"), 30) == T.call[30]


def test_the_records_of_the_references_own_snv_test(tmp_path):
    bam, _ = bc.write_case(tmp_path, "snvrs", {"ref": bc.SNV_RS_REF}, bc.snv_rs_records())
    loc, = bc.loci_of([bc.SNV_RS_CANDIDATE], {"ref": bc.SNV_RS_REF})
    _, recs = read_bam(bam)
    hits = [basecalls.allele_support(r, loc) for r in recs]
    probs_ref, probs_alt, eps = [0.9999, 0.00033, 0.99999], [0.000033, 0.999, 0.0000033], [0.000001, 0.00001, 0.0000001]
    for h, pr, pa, e in zip(hits, probs_ref, probs_alt, eps):
        assert abs(math.exp(h.prob_ref) - pr) <= e and abs(math.exp(h.prob_alt) - pa) <= e
    assert hits[3] is None and hits[4] is None                     # M_Del_M, M_RefSkip_M
    assert hits[0].read_position == 10                             # 5 + 5 hard-clipped bases
    assert hits[1].read_position == 5 + 2 and hits[2].read_position == 3
    assert [h.third_allele for h in hits[:3]] == [0, 0, 0]


def test_enclosing_at_the_exact_boundaries(hand):
    assert sup(hand, "snv_starts_at_locus", 0) is not None and sup(hand, "snv_ends_at_locus", 0) is not None
    assert sup(hand, "snv_starts_behind", 0) is None and sup(hand, "snv_ends_before", 0) is None
    assert sup(hand, "mnv_starts_at_locus", 1) is not None and sup(hand, "mnv_ends_at_locus", 1) is not None
    assert sup(hand, "mnv_starts_behind", 1) is None and sup(hand, "mnv_ends_before", 1) is None
    assert sup(hand, "snv_ends_at_locus", 0).read_position == 9 and sup(hand, "mnv_ends_at_locus", 1).read_position == 7


def test_snv_bases(hand):
    h = sup(hand, "snv_alt", 0)
    assert (h.prob_alt, h.prob_ref, h.strand, h.third_allele, h.read_position) == (T.call[30], T.miscall[30] + LN_CONF, abi.STRAND_FORWARD, 0, 5)
    h = sup(hand, "snv_N", 0)
    assert (h.prob_alt, h.prob_ref, h.strand, h.third_allele) == (LN_ANY, LN_ANY, abi.STRAND_NONE, 0)
    h = sup(hand, "snv_third", 0)   # the read's own base stands in for REF
    assert (h.prob_alt, h.prob_ref, h.strand, h.third_allele) == (T.miscall[30] + LN_CONF, T.call[30], abi.STRAND_REVERSE, 1)
    h = sup(hand, "snv_hardclip_softclip", 0)
    assert h.read_position == 5 + 4 and h.prob_alt == T.call[30]


def test_snv_qualities_0_93_255(hand):
    h = sup(hand, "snv_q0", 0)
    assert h.prob_alt == -math.inf and h.prob_ref == LN_CONF
    h = sup(hand, "snv_q93", 0)
    assert h.prob_ref == T.call[93] and h.prob_alt == T.miscall[93] + LN_CONF and h.prob_ref < 0.0
    h = sup(hand, "snv_q255", 0)
    assert h.prob_alt == T.call[255] and h.prob_ref == T.miscall[255] + LN_CONF


def test_mnv_sums_and_missing_positions(hand):
    m, c = T.miscall[30] + LN_CONF, T.call[30]
    h = sup(hand, "mnv_ref", 1)
    assert (h.prob_ref, h.prob_alt, h.strand, h.third_allele, h.read_position) == (c + c + c, m + m + c, abi.STRAND_FORWARD, 0, 5)
    h = sup(hand, "mnv_alt", 1)
    assert (h.prob_ref, h.prob_alt, h.strand, h.third_allele) == (m + m + c, c + c + c, abi.STRAND_REVERSE, 0)
    assert sup(hand, "mnv_across_D", 1) is None and sup(hand, "mnv_across_N", 1) is None
    h = sup(hand, "mnv_N_inside", 1)   # N is no edit: alt still explains the read without a third allele
    assert (h.prob_ref, h.prob_alt, h.third_allele) == (m + LN_ANY + c, c + LN_ANY + c, 0)


def test_mnv_third_allele_override(hand):
    by, loci = hand
    m, c = T.miscall[30] + LN_CONF, T.call[30]
    for label, fires in (("mnv_override_fires", True), ("mnv_override_explainable", False)):
        expect = basecalls.expected_substitutions(3, by[label].qual)
        assert abs(1 - expect) >= 0.5, expect          # the decision is half a substitution away from the knife edge
        h = sup(hand, label, 1)
        assert h.prob_alt == c + c + m
        if fires:
            assert h.prob_ref == c + c + c and h.third_allele == 1    # the read's own sequence as the third allele
        else:
            assert h.prob_ref == m + m + m and h.third_allele == 0
    assert not basecalls.explainable(1, 3, by["mnv_override_fires"].qual) and basecalls.explainable(1, 3, by["mnv_override_explainable"].qual)


def test_si_tag_gives_the_strand_per_position(hand, tmp_path):
    assert sup(hand, "snv_si_minus", 0).strand == abi.STRAND_REVERSE
    assert sup(hand, "snv_si_dot", 0).strand == abi.STRAND_NONE
    assert sup(hand, "mnv_si_both", 1).strand == abi.STRAND_BOTH
    assert sup(hand, "mnv_si_same", 1).strand == abi.STRAND_FORWARD
    assert sup(hand, "snv_si_not_a_string", 0).strand == abi.STRAND_REVERSE     # not a string: the record's strand
    bad = bc.hand_error_records()
    bam, _ = bc.write_case(tmp_path, "err", {"c1": bc.HAND_REF}, bad.values())
    _, recs = read_bam(bam)
    loci = bc.loci_of(bc.HAND_CANDIDATES, {"c1": bc.HAND_REF})
    with pytest.raises(basecalls.ReadPosOutOfBounds):
        basecalls.allele_support(recs[0], loci[0])
    with pytest.raises(basecalls.InvalidStrandInfo):
        basecalls.allele_support(recs[1], loci[0])


def test_flag_rule_and_realign_indel_reads(hand):
    by, loci = hand
    recs = list(by.values())
    sc = basecalls.score_records(recs, loci)
    assert sc.n_rejected == 4 and sc.n_records == len(recs) and not sc.bad_records
    labels = list(by)
    seen = {labels[h.record] for h in sc.hits}
    assert not seen & {"flag_secondary", "flag_qcfail", "flag_duplicate", "flag_unmapped"} and "flag_supplementary" in seen
    assert [h.locus for h in sc.hits] == sorted(h.locus for h in sc.hits)                         # locus-major
    assert all(a.record < b.record for a, b in zip(sc.hits, sc.hits[1:]) if a.locus == b.locus)   # record order within a locus
    sr = basecalls.score_records(recs, loci, realign_indel_reads=True)
    flagged = {labels[h.record] for h in sr.needs_realign}
    assert flagged == {"snv_behind_insertion", "mnv_across_D"} and all(h.status == basecalls.NEEDS_REALIGN for h in sr.needs_realign)
    assert bc.hit_keys(sr.hits) == [k for k, h in zip(bc.hit_keys(sc.hits), sc.hits) if labels[h.record] not in flagged]
    assert sup(hand, "mnv_across_D", 0, realign_indel_reads=True) is None                         # Enclosing comes first


def test_merge_mates(hand):
    by, loci = hand
    labels = list(by)
    sc = basecalls.score_records(list(by.values()), loci)
    snv = [h for h in sc.hits if h.locus == 0]
    names = [by[labels[h.record]].qname for h in snv]
    merged = {names[[x.record for x in snv].index(f.record)]: f for f in basecalls.merge_mates(snv, names)}
    a, r = T.call[30], T.miscall[30] + LN_CONF
    f = merged["pair_aa"]     # both support alt at different read positions: no read position; strands differ
    assert (f.prob_alt, f.prob_ref, f.read_position, f.strand, len(f.records)) == (a + a, r + r, None, abi.STRAND_BOTH, 2)
    f = merged["pair_ar"]     # the read position of the mate that supports alt
    assert (f.prob_alt, f.prob_ref, f.read_position, f.strand) == (a + r, r + a, 8, abi.STRAND_BOTH)
    f = merged["pair_ra"]
    assert (f.prob_alt, f.prob_ref, f.read_position) == (r + a, a + r, 3)
    f = merged["pair_rr"]     # equal positions stay
    assert (f.prob_alt, f.prob_ref, f.read_position, f.strand) == (r + r, a + a, 8, abi.STRAND_BOTH)
    assert merged["snv_alt"].records == (labels.index("snv_alt"),)          # a single record stays as it is
    assert len(merged) == len(set(names))
    # equal read positions and strands of two alt supports stay; strand none takes the other; third-allele evidence adds up
    H = basecalls.Hit
    x = basecalls.merge(H(0, 0, -5.0, -1.0, abi.STRAND_FORWARD, 4, 1, 60, 0), H(0, 1, -6.0, -2.0, abi.STRAND_FORWARD, 4, 2, 60, 0))
    assert (x.read_position, x.strand, x.third_allele, x.prob_ref, x.prob_alt) == (4, abi.STRAND_FORWARD, 3, -11.0, -3.0)
    x = basecalls.merge(H(0, 0, -5.0, -5.0, abi.STRAND_NONE, 4, 0, 60, 0), H(0, 1, -6.0, -2.0, abi.STRAND_REVERSE, None, 2, 60, 0))
    assert (x.read_position, x.strand, x.third_allele) == (None, abi.STRAND_REVERSE, 2)


def test_candidate_typing():
    ref = bc.HAND_REF
    assert basecalls.locus(ref, 0, 20, b"c", b"t").kind == abi.BASEPILEUP_SNV and basecalls.locus(ref, 0, 40, b"TGA", b"cca").kind == abi.BASEPILEUP_MNV
    for r, a in ((b"C", b"<DEL>"), (b"CG", b"C"), (b"C", b"CT"), (b"A", b"T")):
        with pytest.raises(ValueError):
            basecalls.locus(ref, 0, 20, r, a)


@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_fixture_meets_its_expected_block(oracle, golden_dir, name):
    bam, fasta, scenario, cand = bc.fixture_case(golden_dir, name)
    sup_ = basecalls.allele_supports(bam, fasta, cand, device="cpu")
    batch = basecalls.pileup(sup_, cand)
    assert batch.n_loci == 1 and batch.n_obs == len(sup_[0]) > 0 and batch.locus["variant_type"][0] == (abi.VT_SNV if len(cand[0][2]) == 1 else abi.VT_MNV)
    sc = cli.scenario_from_yaml(scenario, contig=cand[0][0])
    res = oracle.call(sc, batch)
    assert bc.FIXTURES[name](float(res.map_vaf[0, 0]), bp.phred_by_event(sc, res.ln_posterior[0])), float(res.map_vaf[0, 0])
