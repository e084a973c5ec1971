"""The other alleles of a locus (`alt_variants`) in the restatement of varlociraptor_amd/fragments.py, on the CPU: the grouping, the
reference side of an evidence with competitors, which reads are realigned, and that nothing changes without the flag.  The
expectations are stated from the sequences of tests/altvariant_cases.py (which allele a read carries, how many edits it is from
which window), not from the code under test; scores come from the CPU oracle's pair HMMs."""
import os

import numpy as np
import pytest

import altvariant_cases as ac
import basecall_cases as bc
from varlociraptor_amd import fragments, readwindows, realign
from varlociraptor_amd.readwindows import read_bam

F = fragments
PJ = {"insert_size": {"mean": 130.0, "sd": 12.0}, "max_del_cigar_len": 4, "max_ins_cigar_len": 4, "frac_max_softclip": 0.1, "max_read_len": ac.READ, "max_mapq": 60}


# ------------------------------------------------------------------------------------------------ grouping
def test_groups_follow_consecutive_rows_with_equal_chrom_and_pos(tmp_path):
    vcf = tmp_path / "c.vcf"
    vcf.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n"
                   "a1\t151\t.\tTGA\tT,TA\n"          # one record with two ALTs ...
                   "a1\t151\t.\tTG\tT\n"              # ... and the next record at the same POS: one group of three
                   "a1\t160\t.\tC\tG\n"               # another POS breaks the group
                   "a1\t151\t.\tT\tC\n")              # the same POS again, but not consecutive: a group of its own
    rows = F.read_candidates(str(vcf))
    assert [(r[1], r[3], r[4]) for r in rows] == [(151, "TGA", "T"), (151, "TGA", "TA"), (151, "TG", "T"), (160, "C", "G"), (151, "T", "C")]
    # the ones before it, then the ones after it
    assert F.alt_variant_groups(rows) == [[1, 2], [0, 2], [0, 1], [], []]
    assert F.alt_variant_groups([]) == []


def test_sixteen_competitors_are_refused_and_the_locus_is_named():
    rows = [("chr7", 1234, ".", "T", "T" + "A" * (k + 1)) for k in range(16)]
    assert all(len(g) == 15 for g in F.alt_variant_groups(rows))
    rows.append(("chr7", 1234, ".", "T", "TC"))
    with pytest.raises(F.PreprocessError) as e:
        F.alt_variant_groups(rows)
    assert "chr7:1234" in str(e.value) and "17" in str(e.value)


def test_competitor_windows_are_the_candidates_own_alt_windows():
    ref = ac.contig()
    for window in (10, 64):
        for c, pos, r, a in ac.two_deletions(ref) + ac.insertions(ref, 3):
            assert F.competitor_window(ref, pos, r, a, window) == bytes(readwindows.indel_locus(ref, pos, r, a, window).alt_allele)
        for c, pos, r, a in ac.mnv_site(ref):
            w = F.competitor_window(ref, pos, r, a, window)
            rw_ = int(window * 1.5)
            assert w == ref[max(0, pos - rw_):pos] + a + ref[pos + len(r):pos + len(r) + rw_]
    with pytest.raises(F.PreprocessError):
        F.competitor_window(ref, ac.DEL_AT, b"TGA", b"CC", 64)


# ------------------------------------------------------------------------------------------------ a two-deletion site
@pytest.fixture(scope="module")
def two_del(oracle, tmp_path_factory):
    """reads with the G deleted (the TG>T allele) and reads with the A deleted (the tie) over the site, restated with and without the
    competitors"""
    tmp = tmp_path_factory.mktemp("twodel")
    ref = ac.contig()
    cands = ac.two_deletions(ref)
    sites, comp = ac.sites_and_windows(ref, cands)
    n_g, n_a = 6, 3
    recs = ac.by_start(ac.del_reads(ref, "G", n_g) + ac.del_reads(ref, "A", n_a, prefix="t"))
    bam, fa = bc.write_case(tmp, "twodel", {"a1": ref}, recs)
    records = read_bam(bam)[1]
    alone = F.restate_indel(records, sites, ac.PROPS, True, F.RealignSpec(), {0: ref.upper()}, "cpu")
    with_c = F.restate_indel(records, sites, ac.PROPS, True, F.RealignSpec(), {0: ref.upper()}, "cpu", competitors=comp)
    names = [r.qname for r in records]
    return ref, cands, sites, comp, records, names, alone, with_c, bam, fa


def _of(rs, names, locus, kind):
    """the evidences of `locus` whose record's name says it carries `kind` ("dG": the G deleted, "tA": the A deleted)"""
    return [e for e in rs.evidences if e.locus == locus and names[e.ev.record].startswith(kind)]


def test_one_base_deletion_reads_count_against_the_two_base_deletion(two_del):
    ref, cands, sites, comp, records, names, alone, with_c, _, _ = two_del
    assert [len(c) for c in comp] == [1, 1] and comp[0][0] == bytes(sites[1].locus.alt_allele) and comp[1][0] == bytes(sites[0].locus.alt_allele)
    # scored alone, a read with the G deleted is one edit from the reference (T G A C) and one from TGA>T (T C): it fits neither
    for e in _of(alone, names, 0, "dG"):
        assert (e.dist_ref, e.dist_alt) == (1, 1)
    assert len(_of(alone, names, 0, "dG")) == 6
    # with TG>T as a competitor the reference side wins through it, at distance 0
    for e in _of(with_c, names, 0, "dG"):
        assert (e.winner, e.dist_ref, e.dist_alt, e.n_tied, e.n_ref_side_hits) == (1, 0, 1, 1, 2)
        pr, pa = realign.normalize_support(e.ln_ref, e.ln_alt)
        assert pr > pa + 10.0                       # a wide margin: ln odds above 10
    # the same reads stay alt support of TG>T, whose competitor (TGA>T) is further away than the reference
    for e in _of(with_c, names, 1, "dG"):
        assert (e.winner, e.dist_ref, e.dist_alt) == (0, 1, 0) and e.ln_alt > e.ln_ref + 10.0
    # the observations: every fragment of these reads is reference support of TGA>T and alt support of TG>T
    g = {k for k, n in enumerate(names) if n.startswith("dG")}
    o0 = [o.obs for o in with_c.per_locus[0] if o.obs.left in g]
    o1 = [o.obs for o in with_c.per_locus[1] if o.obs.left in g]
    assert len(o0) == len(o1) == 6 and all(o.prob_ref > o.prob_alt + 10.0 for o in o0) and all(o.prob_alt > o.prob_ref + 10.0 for o in o1)
    # alone they were near 0.5 / 0.5 for TGA>T in comparison: the margin was below the one the competitor gives
    a0 = [o.obs for o in alone.per_locus[0] if o.obs.left in g]
    assert all(abs(o.prob_ref - o.prob_alt) < 10.0 for o in a0)


def test_a_tie_is_decided_by_the_pair_hmm(two_del, oracle):
    ref, cands, sites, comp, records, names, alone, with_c, _, _ = two_del
    gap = realign.GapParams()
    g = [gap.prob_insertion_artifact, gap.prob_deletion_artifact, gap.prob_insertion_extend_artifact, gap.prob_deletion_extend_artifact]
    evs = _of(with_c, names, 1, "tA")
    assert len(evs) == 3
    for e in evs:
        # a read with the A deleted (T G C) is one edit from the reference, one from TGA>T (T C) and one from TG>T (T A C)
        assert (e.n_tied, e.n_ref_side_hits, e.dist_ref, e.dist_alt) == (2, 2, 1, 1)
        s_ref = oracle.pairhmm_prob_related(e.ev.ref_allele, e.ev.read_window, e.ev.quals, g, 1 + realign.EDIT_BAND)
        s_comp = oracle.pairhmm_prob_related(comp[1][0], e.ev.read_window, e.ev.quals, g, 1 + realign.EDIT_BAND)
        assert s_ref != s_comp
        assert e.winner == (1 if s_comp > s_ref else 0) and e.ln_ref == max(s_ref, s_comp)


def test_equal_scores_keep_the_lowest_index(oracle):
    ref = ac.contig()
    window = ref[100:160]
    read = ref[110:150]
    ev = readwindows.Evidence(0, 0, (0, 40), (100, 160), read, bytes([30] * 40), window, 0, 60)
    # competitor 1 and competitor 2 are the reference window itself: equal distances, equal scores
    e = F.RealignEvidence(0, ev, ref[90:150])
    n_edit, n_hmm = F.score_alt_evidences([e], [[window, window]], F.RealignSpec(), "cpu")
    assert (e.winner, e.n_tied, e.n_ref_side_hits, e.dist_ref) == (0, 3, 3, 0) and (n_edit, n_hmm) == (4, 4)
    # a reference that is further away than two identical competitors: the first of them wins
    far = bytearray(window)
    far[25] = ord("A") if window[25:26] != b"A" else ord("C")
    e2 = F.RealignEvidence(0, readwindows.Evidence(0, 0, (0, 40), (100, 160), read, bytes([30] * 40), bytes(far), 0, 60), ref[90:150])
    n_edit, n_hmm = F.score_alt_evidences([e2], [[window, window]], F.RealignSpec(), "cpu")
    assert (e2.winner, e2.n_tied, e2.n_ref_side_hits, e2.dist_ref) == (1, 2, 3, 0) and (n_edit, n_hmm) == (4, 3)
    # no competitor: what score_pairs gives
    e3 = F.RealignEvidence(0, ev, ref[90:150])
    assert F.score_alt_evidences([e3], [[]], F.RealignSpec(), "cpu") == (2, 2)
    dist, lnp = F.score_pairs(F.evidence_pair_batch([e3]), F.RealignSpec(), "cpu")
    assert (e3.ln_ref, e3.ln_alt, e3.dist_ref, e3.dist_alt, e3.winner, e3.n_tied) == (float(lnp[0]), float(lnp[1]), int(dist[0]), int(dist[1]), 0, 1)


def test_select_alleles_states_the_tied_set():
    assert F.select_alleles([3, 1, 1, 2]) == (1, [1, 2], 4)
    assert F.select_alleles([-1, 5]) == (5, [1], 1)
    assert F.select_alleles([-1, -1]) == (-1, [], 0)
    assert F.select_alleles([2] * 16) == (2, list(range(16)), 16)


# ------------------------------------------------------------------------------------------------ an MNV with a competitor
def test_an_mnv_with_a_competitor_realigns_every_enclosing_read(oracle, tmp_path):
    ref = ac.contig()
    mnv, snv, mnv2 = ac.mnv_site(ref)
    recs = ac.plain_reads(ref, ac.MNV_AT, 4, "p")          # no I / D operation
    bam, fa = bc.write_case(tmp_path, "mnv", {"a1": ref}, recs)
    records = read_bam(bam)[1]
    loci = bc.loci_of([mnv, snv], {"a1": ref})             # sorted by start; equal starts keep the order given
    is_mnv = [len(l.ref) > 1 for l in loci]
    assert sorted(is_mnv) == [False, True]
    spec = F.RealignSpec()
    win = lambda c: F.competitor_window(ref, c[1], c[2], c[3], spec.window)
    comp = [[win(snv)] if m else [win(mnv)] for m in is_mnv]
    rs = F.restate(records, loci, ac.PROPS, realign=spec, ref_seqs={0: ref.upper()}, competitors=comp)
    # the MNV: all four enclosing reads are realigned; the SNV with a competitor and the same reads: none
    assert sorted(e.locus for e in rs.evidences) == [is_mnv.index(True)] * 4
    assert all(e.n_ref_side_hits == 2 and e.winner == 0 and e.dist_ref == 0 for e in rs.evidences)      # the reads carry the reference
    # without competitors (or without the spec) nothing is realigned
    assert F.restate(records, loci, ac.PROPS, realign=spec, ref_seqs={0: ref.upper()}).evidences == []
    assert F.restate(records, loci, ac.PROPS).evidences == []
    # and the observations of the SNV are the ones scored from the alignment either way
    plain = F.restate(records, loci, ac.PROPS, realign=spec, ref_seqs={0: ref.upper()})
    j = is_mnv.index(False)
    assert [o.key() for o in rs.per_locus[j]] == [o.key() for o in plain.per_locus[j]] and len(plain.per_locus[j]) == 4


# ------------------------------------------------------------------------------------------------ the flag
def _tables_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x) == len(y) and x.records == y.records
        for f in ("prob_ref", "prob_alt", "prob_mapping", "prob_mismapping", "prob_sample_alt", "prob_hit_base", "strand", "read_position", "third_allele"):
            if hasattr(x, f):
                assert (np.asarray(getattr(x, f)) == np.asarray(getattr(y, f))).all(), f


def test_without_the_flag_the_tables_are_todays(two_del):
    ref, cands, sites, comp, records, names, alone, with_c, bam, fa = two_del
    today = F.observations(bam, fa, cands, PJ, device="cpu", indel_candidates=F.RealignSpec())
    off = F.observations(bam, fa, cands, PJ, device="cpu", indel_candidates=F.RealignSpec(), alt_variants=False)
    on = F.observations(bam, fa, cands, PJ, device="cpu", indel_candidates=F.RealignSpec(), alt_variants=True)
    _tables_equal(today, off)
    # the restatement without competitors is the one of the fixture too, evidence for evidence
    again = F.restate_indel(records, sites, ac.PROPS, True, F.RealignSpec(), {0: ref.upper()}, "cpu")
    assert [(e.key(), e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt) for e in again.evidences] == [(e.key(), e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt) for e in alone.evidences]
    # with the flag the TGA>T table changes: the one-deletion reads become reference support
    assert not (np.asarray(on[0].prob_ref) == np.asarray(today[0].prob_ref)).all()
    assert (np.asarray(on[0].prob_ref) > np.asarray(on[0].prob_alt)).sum() > (np.asarray(today[0].prob_ref) > np.asarray(today[0].prob_alt) + 10.0).sum()


def test_preprocess_variants_takes_the_flag_and_still_names_the_atomic_flag(two_del, tmp_path):
    ref, cands, sites, comp, records, names, alone, with_c, bam, fa = two_del
    vcf = tmp_path / "c.vcf"
    vcf.write_text("##fileformat=VCFv4.2\n##contig=<ID=a1,length=%d>\n#CHROM\tPOS\tID\tREF\tALT\na1\t%d\t.\tTGA\tT\na1\t%d\t.\tTG\tT\n" % (len(ref), ac.DEL_AT + 1, ac.DEL_AT + 1))
    pj = tmp_path / "p.json"
    import json
    pj.write_text(json.dumps(PJ))
    with pytest.raises(F.PreprocessError) as e:
        F.preprocess_variants(fa, str(vcf), bam, str(tmp_path / "o.bcf"), str(pj), "cpu", alt_variants=True)
    assert "--atomic-candidate-variants" in str(e.value)
    many = tmp_path / "many.vcf"
    many.write_text("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n" + "".join("a1\t%d\t.\tT\tT%s\n" % (ac.DEL_AT + 1, "C" * (k + 1)) for k in range(17)))
    with pytest.raises(F.PreprocessError) as e:
        F.preprocess_variants(fa, str(many), bam, str(tmp_path / "o.bcf"), str(pj), "cpu", atomic_candidate_variants=True, indel_candidates=F.RealignSpec(), alt_variants=True)
    assert "a1:%d" % (ac.DEL_AT + 1) in str(e.value)


# ------------------------------------------------------------------------------------------------ a multi-allelic reference testcase
def test_the_three_mnvs_of_test_giab_30_meet_their_block(oracle, golden_dir):
    """tests/golden/bam/ALTVARIANTS.md: the three MNV alleles at 1:301 of test_giab_30 (alt_variants.tsv, all records of the testcase's
    candidates.vcf) through the restatement with realignment and `alt_variants` -> pileup -> oracle: every allele meets the testcase's
    `expected:` block (`NA12878 == 0.0`), and the figures are the recorded ones"""
    import sys
    import fragment_cases as fc
    sys.path.insert(0, os.path.join(os.path.dirname(golden_dir), "..", "tools"))
    import make_altvariant_fixtures as tool
    d = os.path.join(golden_dir, "bam", "test_giab_30")
    cand = tool.candidates_of(d)
    assert len(cand) == 3 and len({c[:2] for c in cand}) == 1 and F.alt_variant_groups(cand) == [[1, 2], [0, 2], [0, 1]]
    # the first allele is the one the fixture always held
    assert cand[0] == bc.fixture_case(golden_dir, "test_giab_30")[3][0]
    alone, with_c = tool.call_site(d, False), tool.call_site(d, True)
    for n, n_alt, vaf, phred in with_c:
        assert fc.FIXTURES["test_giab_30"][0](vaf, phred)
    row = [l for l in open(os.path.join(golden_dir, "bam", "ALTVARIANTS.md")) if l.startswith("| test_giab_30 ")][0].split("|")
    assert row[5].strip() == "; ".join("%d, %d, %.4g" % g[:3] for g in alone) and row[6].strip() == "; ".join("%d, %d, %.4g" % g[:3] for g in with_c)
    assert row[7].strip() == "yes"
    # the rule shows on real data: with competitors more reads support the second and third allele (reads without an I / D operation
    # are realigned at an MNV that has other alleles), none fewer
    assert [g[1] for g in with_c] != [g[1] for g in alone] and all(w[1] >= a[1] for w, a in zip(with_c, alone))
