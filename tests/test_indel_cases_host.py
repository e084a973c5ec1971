"""The restatement varlociraptor_amd/readwindows.py `evidence` (what csrc/vlr_indelpileup.h computes per record) on the inputs of
tests/indel_cases.py, without a library: the hand records and the synthetic set reach every branch of candidate_region, both status
bits and every filtered flag — asserted by name, so that the host-program and GPU tests, which compare with `evidence`, cannot pass on
inputs that look nowhere — and on the BAM fixtures of bam_pairs.BAM_CASES `evidence` and the older `evidence_windows` give the same
windows for the records both keep, the difference between the two sets being exactly the records with 0x200 / 0x400 / 0x800 and the
no-overlap ones."""
import os

import pytest

import bam_pairs as bp
import indel_cases as ic
from varlociraptor_amd import readwindows as rw


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("hand")
    recs = ic.hand_records()
    bam, _ = ic.write_case(tmp, "hand", ic.HAND_CONTIGS, recs.values())
    loci, rid, order = ic.loci_of(ic.HAND_CANDIDATES.values(), ic.HAND_CONTIGS)
    cl = list(ic.HAND_CANDIDATES)
    labels = list(recs)
    exp = ic.expected(bam, ic.HAND_CONTIGS, loci, rid)
    by = {(cl[order[j]], labels[e.record]): e for j, e in exp}
    _, parsed = rw.read_bam(bam)
    return dict(by=by, recs=dict(zip(labels, parsed)), loci=dict(zip([cl[k] for k in order], loci)), exp=exp)


def branch(rec, loc):
    """which arm of candidate_region a record takes for a locus: 1 encloses, 2 start only, 3 end only, 4 neither"""
    qs, qe = rw.read_pos(rec, loc.start, True, True), rw.read_pos(rec, loc.end, True, True)
    return 1 if qs is not None and qe is not None else 2 if qs is not None else 3 if qe is not None else 4


def test_hand_records_reach_every_branch_by_name(hand):
    by, recs, loci = hand["by"], hand["recs"], hand["loci"]

    def at(locus, record):
        e = by[(locus, record)]
        return branch(recs[record], loci[locus]), e.status, e.read_interval, e.ref_interval
    # branch 1: the read encloses the locus; read window clamped at the read's ends, ref window 96 on either side
    assert at("del", "plain_over_del") == (1, 0, (0, 60), (24, 216))
    # read_pos inside a deletion projects to where the deletion starts: qs = 20, qe = 21 / qs = qe = 15
    assert rw.read_pos(recs["carries_del"], 123, True, True) == 21 and rw.read_pos(recs["carries_del"], 123, True, False) is None
    assert rw.read_pos(recs["D_covers_locus_start"], 120, True, True) == 15 and at("del", "D_covers_locus_start")[0] == 1
    # leading deletion, hard clips, a hard clip in front of a soft clip, a leading soft clip with and without include_softclips
    assert rw.read_pos(recs["leading_D"], 120, True, True) == 17 and at("del", "leading_D")[:2] == (1, 0)
    assert rw.read_pos(recs["hard_clips"], 120, True, True) == 20
    assert rw.read_pos(recs["hard_then_soft_clip"], 120, True, True) == 13
    assert rw.read_pos(recs["lead_softclip"], 110, True, True) == 3 and rw.read_pos(recs["lead_softclip"], 110, False, True) is None
    # a leading clip longer than pos: the alignment start stays at 0; the ref window clamps at 0
    assert rw.read_pos(recs["lead_clip_longer_than_pos"], 0, True, True) == 0 and rw.read_pos(recs["lead_clip_longer_than_pos"], 20, True, True) == 20
    assert at("del_clamps_at_0", "lead_clip_longer_than_pos") == (1, 0, (0, 50), (0, 116))
    # ... and at the contig's end
    assert at("ins_clamps_at_end", "near_end")[3] == (489, 600) and at("del_near_end", "near_end")[3] == (494, 600)
    # an insertion at the locus; a read that reaches the locus by its trailing clip alone
    assert at("ins", "carries_ins")[:3] == (1, 0, (0, 54))
    assert at("ins", "trail_softclip")[:3] == (1, 0, (0, 38)) and recs["trail_softclip"].end_pos() == 195
    # the MAX_PATTERN_LEN trim: 129 bases -> 0 off the front, 1 off the back; 153 bases with max_window clamped at 0 -> 12 and 13
    assert at("ins", "window_128_odd_trim") == (1, 0, (36, 164), (104, 296))
    assert at("long_del", "window_trim_odd_25") == (1, 0, (32, 160), (204, 396))
    # branch 2 and 3: only the locus start, only its end (the ref window sits at the end)
    assert at("repl", "covers_repl_start_only") == (2, 0, (0, 40), (164, 356))
    assert at("repl", "covers_repl_end_only") == (3, 0, (0, 40), (167, 359))
    assert at("long_del", "clip_reaches_long_del")[:3] == (2, 0, (0, 50))      # (through its soft clip: read_pos counts it as aligned)
    # read windows of 1, 63, 64, 65 (branch 2, clamped by the read), 127 (branch 4) and 128
    assert [at("long_del", r)[2] for r in ("window_1", "window_63", "window_64", "window_65")] == [(0, 1), (0, 63), (0, 64), (0, 65)]
    # branch 4: inside the long deletion (enclosed), and spanning it with a reference skip (NO_OVERLAP)
    assert at("long_del", "inside_long_del") == (4, 0, (0, 50), (340 + 25 - 96, 340 + 25 + 96))
    assert at("long_del", "inside_long_del_130") == (4, 0, (1, 128), (310 + 65 - 96, 310 + 65 + 96))
    assert at("long_del", "N_spans_long_del") == (4, rw.NO_OVERLAP, (0, 0), (0, 0))
    # a CIGAR that begins with N
    assert by[("del", "begins_with_N")].status == rw.LEADING_REFSKIP and by[("del", "begins_with_N")].read_window == b""
    with pytest.raises(ValueError):
        rw.read_pos(recs["begins_with_N"], 120, True, True)
    # the flag rule: 0x100, 0x200, 0x400 and 0x4 are no evidence, 0x800 is; FLAG bits and MAPQ travel with the evidence
    for r in ("flag_secondary", "flag_qcfail", "flag_duplicate", "flag_unmapped"):
        assert rw.overlaps(recs[r], loci["del"].start, loci["del"].end) and ("del", r) not in by
    assert ("del", "flag_supplementary") in by
    assert (by[("ins", "mapq_0")].mapq, by[("ins", "mapq_0")].flag, by[("ins", "paired_first")].flag) == (0, 0x10, 0x41)
    # the other contig: its record is evidence for its own locus alone; a read without bases gives none
    assert ("ins_c2", "on_c2") in by and not any(r in ("on_c2", "on_c2_behind") for l, r in by if l != "ins_c2") and ("ins_c2", "on_c2_behind") not in by
    assert branch(recs["empty_seq"], loci["del"]) == 4 and rw.overlaps(recs["empty_seq"], 120, 123) and ("del", "empty_seq") not in by
    # lower-case reference bases come out upper case; the windows are the record's own bytes
    e = by[("del", "quals")]
    assert ic.C1[100:140].islower() and e.ref_allele == ic.U1[24:216] and e.read_window[25:26] == b"N" and e.quals == bytes((7 * k) % 94 for k in range(50))
    assert {len(e.read_window) for e in by.values()} >= {0, 1, 63, 64, 65, 127, 128}


def test_synthetic_set_reaches_every_branch_too(tmp_path):
    contigs, cands, recs = ic.synthetic()
    bam, _ = ic.write_case(tmp_path, "syn", contigs, recs)
    loci, rid, _ = ic.loci_of(cands, contigs)
    exp = ic.expected(bam, contigs, loci, rid)
    _, parsed = rw.read_bam(bam)
    seen = {(branch(parsed[e.record], loci[j]), e.status) for j, e in exp if e.status != rw.LEADING_REFSKIP}
    assert seen >= {(1, 0), (2, 0), (3, 0), (4, 0), (4, rw.NO_OVERLAP)} and any(e.status == rw.LEADING_REFSKIP for _, e in exp)
    assert len(exp) > 200 and {r for r in rid} == {0, 1} and any(len(e.read_window) == 128 for _, e in exp)
    assert any(e.ref_interval[0] == 0 for _, e in exp if e.status == 0) and any(e.ref_interval[1] == len(contigs["s1"]) for _, e in exp)
    kept = {e.record for _, e in exp}
    assert not any(parsed[k].flag & 0x704 for k in kept) and any(parsed[k].flag & 0x800 for k in kept)


@pytest.mark.parametrize("name", sorted(bp.BAM_CASES))
def test_fixture_windows_equal_evidence_windows_where_both_keep_the_record(golden_dir, name):
    d = os.path.join(golden_dir, "bam", name)
    case = bp.indel_pairs(d, ic.WINDOW)
    bam, _, contigs, names, cand = ic.fixture_case(golden_dir, name)
    loci, rid, _ = ic.loci_of(cand, contigs, names=names)
    exp = ic.expected(bam, contigs, loci, rid, names=names)
    _, recs = rw.read_bam(bam)
    assert loci[0].alt_allele == case.alt_allele and len(case.reads) == bp.BAM_CASES[name]["n_reads"]
    # evidence_windows hands out the record objects of its own read_bam: match them by their place in the file through equal content
    place = {}
    for k, r in enumerate(recs):
        place.setdefault((r.qname, r.flag, r.pos, tuple(r.cigar), r.seq), []).append(k)
    old_at = {}
    for r, seq, q, ra in case.reads:
        old_at[place[(r.qname, r.flag, r.pos, tuple(r.cigar), r.seq)].pop(0)] = (seq, bytes(bytearray(q)), ra)
    assert len(old_at) == len(case.reads)
    new_at = {e.record: e for _, e in exp}
    both = sorted(set(old_at) & set(new_at))
    assert len(both) > 0
    for k in both:
        assert new_at[k].status == 0 and (new_at[k].read_window, new_at[k].quals, new_at[k].ref_allele) == old_at[k]
    # only the old filter keeps: duplicates and QC-fail reads; only the new one: supplementary and no-overlap reads
    assert all(recs[k].flag & 0x600 for k in set(old_at) - set(new_at))
    assert all(recs[k].flag & 0x800 or new_at[k].status == rw.NO_OVERLAP for k in set(new_at) - set(old_at))
    assert all(new_at[k].status in (0, rw.NO_OVERLAP) for k in new_at)
    print(name, "old filter %d reads, new filter %d (%d no-overlap)" % (len(old_at), len(new_at), sum(e.status == rw.NO_OVERLAP for e in new_at.values())))
