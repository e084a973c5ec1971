"""The restatement of fragment observations (varlociraptor_amd/fragments.py) without a GPU: the hand cases of tests/fragment_cases.py
against the expectations stated there, the hashed alt-locus key against the string key, the per-record features against the
reference's recorded observations of two testcases, and the testcases of tests/golden/bam/FRAGMENTS.md through restatement -> pileup ->
oracle against their own `expected:` blocks."""
import collections
import os

import numpy as np
import pytest

import bam_pairs as bp
import fragment_cases as fc
from varlociraptor_amd import abi, basecalls, cli, fragments, obsfmt
from varlociraptor_amd.readwindows import read_bam, read_fasta


def restated(tmp, case):
    bam, fa = fc.write_case(tmp, case)
    loci, order = fc.loci_of(case)
    rs = fragments.restate(read_bam(bam)[1], loci, case.props)
    obs = [None] * len(order)
    for j, k in enumerate(order):
        obs[k] = rs.per_locus[j]
    return bam, fa, obs


@pytest.mark.parametrize("case", fc.hand_cases(), ids=lambda c: c.name)
def test_hand_case(case, tmp_path):
    bam, fa, obs = restated(tmp_path, case)
    if any(o.status for os_ in obs for o in os_):
        with pytest.raises(fragments.InvalidReadOrientationInfo):
            fragments.observations(bam, fa, case.candidates, case.props, device="cpu")
        fc.check_case(case, [[None] * len(o) for o in obs], obs)
        return
    fc.check_case(case, fragments.observations(bam, fa, case.candidates, case.props, device="cpu"), obs)


def all_observation_lists(tmp, golden_dir):
    for case in fc.hand_cases():
        for obs in restated(tmp, case)[2]:
            yield case.name, obs, case.props
    for name in fc.FIXTURES:
        bam, fasta, _, cand, props = fc.fixture_case(golden_dir, name)
        contigs, recs = read_bam(bam)
        loc = basecalls.locus(read_fasta(fasta)[cand[0][0]], [c for c, _ in contigs].index(cand[0][0]), *cand[0][1:])
        yield name, fragments.restate(recs, [loc], props).per_locus[0], props


def test_hashed_alt_loci_equal_string_alt_loci(tmp_path, golden_dir):
    n_with = 0
    for name, obs, props in all_observation_lists(tmp_path, golden_dir):
        ms, cs = fragments.alt_locus_classes(obs, props.max_read_len)
        mh, ch = fragments.alt_locus_classes(obs, props.max_read_len, key=fragments.hashed)
        assert cs == ch and (ms is None) == (mh is None) and (ms is None or fragments.hashed(ms) == mh), name
        n_with += sum(1 for o in obs if o.alt_loci)
    assert n_with > 5


def test_major_feature_rules():
    assert fragments.calc_major_feature([]) is None and fragments.calc_major_feature([1, 2, 3]) is None
    assert fragments.calc_major_feature([4, 4]) == 4 and fragments.calc_major_feature([4, 4, 5, 5]) is None and fragments.calc_major_feature([5, 4, 4, 5, 4]) == 4


def test_mapq_adjustment_by_hand():
    t = basecalls.TABLES
    # one observation at the maximal MAPQ: mean of itself and the pseudo observation ln 0.5
    got = fragments.adjusted_prob_mapping([t.call[60]], 60, t)
    assert got == [basecalls.ln_sum_exp([t.call[60], fragments.PROB_05]) - np.log(2)]
    # 20 observations: no pseudo observation; the ones below the maximum count as ln 0.5
    pm = [t.call[60]] * 15 + [t.call[20]] * 5
    assert fragments.adjusted_prob_mapping(pm, 60, t) == [basecalls.ln_sum_exp([t.call[60]] * 15 + [fragments.PROB_05] * 5) - float(np.log(20))] * 20
    assert abs(np.exp(fragments.adjusted_prob_mapping(pm, 60, t)[0]) - (15 * (1 - 1e-6) + 5 * 0.5) / 20) < 1e-12


@pytest.mark.parametrize("name,count", [("test_uzuner_clonal_1", 102), ("test_uzuner_clonal_3", 110)])
def test_per_record_features_equal_the_recorded_observations(golden_dir, name, count):
    """the reference's recorded v15 observations are one per READ: they pin strand, orientation class, softclipped and paired of every
    record that encloses the locus (not fragments, order or the probabilities of pairs)"""
    batch, _ = obsfmt.read_observation_vcf([os.path.join(golden_dir, "testcases", name, "observations.vcf")])
    recorded = collections.Counter((int(x) & 3, (int(x) >> abi.F_ORIENT_SHIFT) & 3, bool(int(x) & abi.F_SOFTCLIPPED), bool(int(x) & abi.F_PAIRED))
                                   for x in batch.columns["flags"])
    bam, fasta, _, cand, _ = fc.fixture_case(golden_dir, name)
    contigs, recs = read_bam(bam)
    loc = basecalls.locus(read_fasta(fasta)[cand[0][0]], [c for c, _ in contigs].index(cand[0][0]), *cand[0][1:])
    mine = collections.Counter()
    for k, r in enumerate(recs):
        h = basecalls.allele_support(r, loc, 0, k) if basecalls.is_valid_record(r.flag) and r.ref_id == loc.ref_id else None
        if h is not None:
            mine[(h.strand, int(fragments.pack_orientation(np.array([fragments.record_orientation(r)]))[0]), fragments.softclipped(r), bool(r.flag & 1))] += 1
    assert sum(recorded.values()) == count and mine == recorded


def call_fixture(oracle, golden_dir, name, device="cpu"):
    bam, fasta, scenario, cand, props = fc.fixture_case(golden_dir, name)
    tabs = fragments.observations(bam, fasta, cand, props, device=device)
    batch, _ = fragments.pileup(tabs, cand)
    sc = cli.scenario_from_yaml(scenario, contig=cand[0][0])
    res = oracle.call(sc, batch)
    return float(res.map_vaf[0, 0]), bp.phred_by_event(sc, res.ln_posterior[0]), batch


def test_fixtures_meet_their_expected_blocks(oracle, golden_dir):
    """restatement -> pileup -> oracle; which cases meet their block is what FRAGMENTS.md lists, at least MIN_MET of the thirteen do, and
    the two that missed before fragments and artifact hypotheses were built are among them"""
    met = {}
    for name, (pred, listed) in fc.FIXTURES.items():
        vaf, ph, batch = call_fixture(oracle, golden_dir, name)
        met[name] = bool(pred(vaf, ph))
        print(name, batch.n_obs, vaf, "met" if met[name] else "missed")
        assert met[name] == listed, (name, vaf)
    assert sum(met.values()) >= fc.MIN_MET and all(met[n] for n in fc.MUST_MEET)
    doc = open(os.path.join(golden_dir, "bam", "FRAGMENTS.md")).read()
    for name, ok in met.items():
        row, = [l for l in doc.split("\n") if l.startswith("| %s |" % name)]
        assert ("| yes |" in row) == ok


def test_pileup_fills_the_feature_flags(oracle, golden_dir):
    _, _, batch = call_fixture(oracle, golden_dir, "test_giab_10")
    f = batch.columns["flags"]
    assert (batch.locus["locus_flags"][0] & abi.BIAS_ALL) == (abi.BIAS_ALL & ~abi.BIAS_HOMOPOLYMER) and batch.locus["locus_flags"][0] & abi.LOCUS_HAS_SNV
    assert (f & abi.F_PAIRED).any() and (f & abi.F_MAX_MAPQ).any() and len(set((f >> abi.F_ORIENT_SHIFT) & 3)) > 1 and len(set(f & 3)) > 1
    assert len(set(batch.columns["prob_mapping"])) == 1 and len(set(batch.columns["prob_hit_base"])) > 1
