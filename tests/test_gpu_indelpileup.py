"""Indel allele supports from BAM records on the GPU (vlr_indelpileup_*, csrc/vlr_indelpileup.hip).  The kernels' hits must equal the
restatement (readwindows.evidence) field for field; their scores must equal, with == on f64, what today's Python path returns for a
PairBatch built from the same Evidence windows — realign.best_hits, then prob_related / prob_related_homopolymer / prob_best_path: the
same kernels fed the same bytes —, in all three modes on the hand records and the synthetic set of tests/indel_cases.py and in the
testcase's own mode on every fixture of bam_pairs.BAM_CASES; the kept pair arrays must be that PairBatch's arrays byte for byte; the
hit bytes must not depend on how the file is cut into feeds, files or record sub-ranges; an overflow of the hit buffer and a file cut
inside a record are reported, not faults; and device_supports -> pileup -> engine meets each testcase's own `expected:` block."""
import math
import os
import struct

import numpy as np
import pytest

import bam_pairs as bp
import indel_cases as ic
from varlociraptor_amd import abi, alignprops, cli, engine, realign
from varlociraptor_amd import readwindows as rw

pytestmark = pytest.mark.gpu

NANOPORE = bp.BAM_CASES["test_nanopore_05"]
MODES = {"exact": (None, None), "fast": (None, None), "homopolymer": (realign.GapParams(*NANOPORE["gap"]), realign.HopParams(*NANOPORE["hop"]))}


def python_path(pb, mode, gap, hop):
    """(dist, ln P) of every pair through the entry points the Python path uses; sets the bands of `pb` as it does"""
    if len(pb) == 0:
        return np.zeros(0, np.int32), np.zeros(0)
    dist, _, _ = realign.best_hits(pb)
    if mode == "fast":
        return dist, realign.prob_best_path(pb, gap)
    pb.band = [int(x) + realign.EDIT_BAND if x >= 0 else -1 for x in dist]
    return dist, realign.prob_related_homopolymer(pb, gap, hop) if mode == "homopolymer" else realign.prob_related(pb, gap)


class Case:
    """a BAM with its loci and, per mode, the expectation computed once"""

    def __init__(self, tmp, name, contigs, names, cands, records=None, bam=None, fasta=None):
        self.contigs, self.names = contigs, names
        self.loci, self.rid, self.order = ic.loci_of(cands, contigs, names=names)
        if bam is None:
            bam, fasta = ic.write_case(tmp, name, contigs, records)
        self.bam, self.fasta, self.records = bam, fasta, records
        self.exp = ic.expected(bam, contigs, self.loci, self.rid, names=names)
        self.n_records = len(rw.read_bam(bam)[1])
        self.scores = {}

    def want(self, mode, gap=None, hop=None):
        if mode not in self.scores:
            pb = ic.pair_batch(self.exp, self.loci)
            dist, lnp = python_path(pb, mode, gap, hop)
            self.scores[mode] = (pb, dist, lnp)
        return self.scores[mode]

    def hits(self, mode="exact", gap=None, hop=None, bams=None, **kw):
        return rw.device_hits(bams or self.bam, self.fasta, self.rid, self.loci, mode, gap, hop, **kw)

    def check(self, mode="exact", gap=None, hop=None, **kw):
        arr, res, pairs = self.hits(mode, gap, hop, keep_pairs=True, **kw)
        pb, dist, lnp = self.want(mode, gap, hop)
        # field equality
        assert ic.hit_keys(arr) == ic.evidence_keys(self.exp)
        assert not arr["pad"].any()
        # bitwise scores
        for got, want in ((arr["ln_ref"], lnp[0::2]), (arr["ln_alt"], lnp[1::2]), (arr["dist_ref"], dist[0::2]), (arr["dist_alt"], dist[1::2])):
            assert got.tobytes() == np.ascontiguousarray(want).tobytes()
        # pair arrays
        for got, want in zip(pairs.arrays(), pb.arrays()):
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
        n = len(self.exp)
        assert (res.n_hits, res.n_records, res.n_pairs, res.status, res.needed_capacity, res.first_bad_record) == (n, self.n_records, 2 * n, 0, n, -1)
        assert (res.x_bytes, res.y_bytes) == (sum(len(x) for x in pb.x), sum(len(y) for y in pb.y))
        return arr, res


@pytest.fixture(scope="module")
def hand(tmp_path_factory):
    recs = ic.hand_records()
    return Case(tmp_path_factory.mktemp("hand"), "hand", ic.HAND_CONTIGS, list(ic.HAND_CONTIGS), ic.HAND_CANDIDATES.values(), list(recs.values()))


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("synth")
    contigs, cands, recs = ic.synthetic()
    c = Case(tmp, "synth", contigs, list(contigs), cands, recs)
    c.tmp = tmp
    c.small, _ = ic.write_case(tmp, "synth_small_members", contigs, recs, member_bytes=300)   # records straddle BGZF members
    return c


@pytest.mark.parametrize("mode", sorted(MODES))
def test_hand_records_fields_scores_and_pairs(hand, mode):
    arr, res = hand.check(mode, *MODES[mode])
    assert res.n_rejected == 4 and set(arr["status"]) == {0, abi.INDELPILEUP_HIT_NO_OVERLAP, abi.INDELPILEUP_HIT_LEADING_REFSKIP}
    assert {1, 63, 64, 65, 127, 128} <= set(int(x) for x in arr["read_len"])
    empty = arr[arr["status"] != 0]
    assert np.isneginf(empty["ln_ref"]).all() and np.isneginf(empty["ln_alt"]).all() and (empty["dist_ref"] == -1).all()
    scored = arr[arr["status"] == 0]
    assert (scored["dist_ref"] >= 0).all() and (scored["dist_alt"] >= 0).all() and not np.isnan(scored["ln_ref"]).any()
    assert mode != "exact" or np.isfinite(scored["ln_ref"]).all()   # (the best path of the fast mode may run through a quality 0 base)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_synthetic_set_fields_scores_and_pairs(synth, mode):
    arr, res = synth.check(mode, *MODES[mode])
    assert res.n_hits > 200 and list(arr["locus"]) == sorted(arr["locus"]) and {synth.rid[k] for k in set(arr["locus"])} == {0, 1}


def test_one_chunk_wider_than_the_scan_fields_scores_and_pairs(tmp_path):
    """The prefix sums over a chunk's three u64 count arrays (vlr_bam::scan_kernel of csrc/vlr_bamsession.h, 1024 threads, one workgroup
    per array) where a thread's slice holds two records and the threads of the upper half have none: 1100 records in one chunk (the
    default window_bytes holds the whole file).  The module's 260-record input never gives a thread two records.  Exact mode; the
    comparison of test_synthetic_set_fields_scores_and_pairs: every hit's place, score and pair bytes."""
    contigs, cands, recs = ic.synthetic(n_records=1100)
    c = Case(tmp_path, "scan1100", contigs, list(contigs), cands, recs)
    arr, res = c.check("exact")
    assert res.n_records == 1100 and res.n_hits > 800 and list(arr["locus"]) == sorted(arr["locus"])


def test_hits_do_not_depend_on_feeds_files_or_sub_ranges(synth, monkeypatch):
    base, _, _ = synth.hits()
    assert len(base) == len(synth.exp)
    # window_bytes = 1, the smallest legal value: every feed is one 300-byte BGZF member, records straddle feeds, chunks hold a few records
    for wb in (1, 4096, 0):
        got, res, _ = synth.hits(bams=synth.small, window_bytes=wb)
        assert got.tobytes() == base.tobytes() and res.status == 0, wb
    # two files into one session: the records are counted through
    half = len(synth.records) // 2
    a, _ = ic.write_case(synth.tmp, "first_half", synth.contigs, synth.records[:half])
    b, _ = ic.write_case(synth.tmp, "second_half", synth.contigs, synth.records[half:])
    got, res, pairs = synth.hits(bams=[a, b], keep_pairs=True)
    assert got.tobytes() == base.tobytes() and res.n_records == len(synth.records)
    for x, y in zip(pairs.arrays(), synth.want("exact")[0].arrays()):
        assert x.tobytes() == y.tobytes()
    # record sub-ranges, as for a chunk whose pair bytes pass 2^31: cut every 3000 bytes
    monkeypatch.setenv("VLR_INDELPILEUP_PAIR_BYTES", "3000")
    got, res, pairs = synth.hits(keep_pairs=True)
    assert got.tobytes() == base.tobytes() and res.status == 0 and res.x_bytes > 30000
    for x, y in zip(pairs.arrays(), synth.want("exact")[0].arrays()):
        assert x.tobytes() == y.tobytes()


def test_hit_capacity_overflow_is_reported_and_the_retry_succeeds(synth, golden_dir, tmp_path):
    need = len(synth.exp)
    arr, res, _ = synth.hits(hit_capacity=need - 1, retry=False)
    assert res.status == abi.INDELPILEUP_OVERFLOW and res.needed_capacity == need and res.n_hits == 0 and len(arr) == 0   # (no GUARD_DAMAGED)
    arr, res, _ = synth.hits(bams=synth.small, hit_capacity=7, retry=False, window_bytes=1)      # overflow in the first of many chunks
    assert res.status == abi.INDELPILEUP_OVERFLOW and res.needed_capacity == need
    arr, res, _ = synth.hits(hit_capacity=0, retry=False)
    assert res.status == abi.INDELPILEUP_OVERFLOW and res.needed_capacity == need
    arr, res, _ = synth.hits(hit_capacity=need, retry=False)
    assert res.status == 0 and res.n_hits == need
    arr, res, _ = synth.hits(hit_capacity=need - 1)                                             # the retry with the needed capacity
    assert res.status == 0 and ic.hit_keys(arr) == ic.evidence_keys(synth.exp)
    # device_supports retries too
    bam, fasta, contigs, names, cand = ic.fixture_case(golden_dir, "test_giab_04", tmp_path)
    sup = rw.device_supports(bam, fasta, cand, hit_capacity=3)
    full = rw.device_supports(bam, fasta, cand)
    assert len(sup[0].hits) > 3 and sup[0].hits.tobytes() == full[0].hits.tobytes()


def test_a_file_cut_inside_a_record_is_malformed_input_not_a_fault(synth):
    contigs, recs = synth.contigs, synth.records
    last = recs[-1]
    cut = 36 + last[12] + 5            # inside the second CIGAR word
    assert struct.unpack_from("<H", last, 16)[0] >= 2
    head = alignprops.encode_bam([(c, len(s)) for c, s in contigs.items()], recs[:-1])
    front_bam, _ = ic.write_case(synth.tmp, "front", contigs, recs[:-1])
    want, _, _ = synth.hits(bams=front_bam)
    for name, tail in (("ends_inside", last[:cut]), ("block_size_of_the_cut", struct.pack("<I", cut - 4) + last[4:cut])):
        path = str(synth.tmp / (name + ".bam"))
        with open(path, "wb") as f:
            f.write(alignprops.bgzf_compress(head + tail))
        arr, res, _ = synth.hits(bams=path)
        assert res.status == abi.INDELPILEUP_BAD_RECORD and res.first_bad_record == len(recs) - 1
        assert arr.tobytes() == want.tobytes() and len(arr) > 200
        with pytest.raises(rw.IndelPileupError):
            rw.device_supports(path, synth.fasta, [c for c in ic.synthetic()[1][:3]])
    # and the device is fine afterwards
    synth.check()


def test_open_refuses_bad_arguments(hand, tmp_path):
    for window in (65, 0):
        with pytest.raises(engine.EngineError):
            hand.hits(window=window)
    with pytest.raises(engine.EngineError):
        rw.device_hits(hand.bam, hand.fasta, hand.rid[::-1], hand.loci[::-1])                      # not sorted
    with pytest.raises(engine.EngineError):
        rw.device_hits(hand.bam, hand.fasta, [7] * len(hand.loci), hand.loci)                      # a reference id the header does not have
    with pytest.raises(engine.EngineError):
        hand.hits(gap=realign.GapParams(0.1, -1.0, -math.inf, -math.inf))                          # not a ln probability
    fa = str(tmp_path / "only_c2.fa")
    alignprops.write_fasta(fa, {"c2": ic.C2})
    with pytest.raises(engine.EngineError):
        rw.device_hits(hand.bam, fa, hand.rid, hand.loci)                                          # a contig missing from the FASTA
    hand.check()


def test_device_supports_raises_on_a_leading_reference_skip(hand):
    with pytest.raises(ValueError, match="leading reference skip"):
        rw.device_supports(hand.bam, hand.fasta, [ic.HAND_CANDIDATES["del"]])
    sup = rw.device_supports(hand.bam, hand.fasta, [ic.HAND_CANDIDATES["long_del"], ic.HAND_CANDIDATES["ins"]])
    assert [s.locus.kind for s in sup] == ["deletion", "insertion"]
    k = list(sup[0].hits["status"]).index(abi.INDELPILEUP_HIT_NO_OVERLAP)
    assert (sup[0].prob_alt[k], sup[0].prob_ref[k]) == (math.log(0.5), math.log(0.5))
    for s in sup:
        for i, h in enumerate(s.hits):
            assert (s.prob_ref[i], s.prob_alt[i]) == realign.normalize_support(float(h["ln_ref"]), float(h["ln_alt"]))


@pytest.mark.parametrize("name", sorted(bp.BAM_CASES))
def test_fixture_hits_scores_and_call(oracle, golden_dir, tmp_path, name):
    spec = bp.BAM_CASES[name]
    bam, fasta, contigs, names, cand = ic.fixture_case(golden_dir, name, tmp_path)
    gap = realign.GapParams(*spec["gap"]) if spec["gap"] else realign.GapParams()
    hop = realign.HopParams(*spec["hop"]) if spec.get("hop") else None
    mode = "homopolymer" if hop is not None else "exact"
    case = Case(tmp_path, name, contigs, names, cand, bam=bam, fasta=fasta)
    arr, res = case.check(mode, gap, hop)
    assert case.loci[0].kind == spec["kind"] and res.n_hits > 20
    # end to end: device_supports -> one observation per evidence -> the engine
    sup, = rw.device_supports(bam, fasta, cand, mode, gap, hop)
    assert sup.hits.tobytes() == arr.tobytes()
    _, recs = rw.read_bam(bam)
    loc = sup.locus
    pile = bp.IndelCase(loc.kind, loc.start, loc.end, loc.len_diff, loc.alt_allele, [(recs[int(h["record"])], None, None, None) for h in sup.hits])
    batch = bp.single_end_pileup(pile, sup.prob_alt, sup.prob_ref)
    sc = cli.scenario_from_yaml(os.path.join(golden_dir, *spec["scenario"]), **({"contig": spec["contig"]} if spec["contig"] else {}))
    plan = engine.Plan(sc)
    got = plan.call_host(batch)
    plan.close()
    ref = oracle.call(sc, batch)
    assert np.allclose(np.exp(got.ln_posterior), np.exp(ref.ln_posterior), atol=1e-6, rtol=0) and abs(got.map_vaf[0, 0] - ref.map_vaf[0, 0]) <= 1e-6
    vaf = float(got.map_vaf[0, 0])
    phred = bp.phred_by_event(sc, got.ln_posterior[0])
    print(name, "reads under the old filter %d, evidences under the new one %d (%d without overlap); MAP VAF %g" % (
        spec["n_reads"], len(sup.hits), int((sup.hits["status"] == abi.INDELPILEUP_HIT_NO_OVERLAP).sum()), vaf), phred)
    # the testcase's own expectation (testcase.yaml `expected:`)
    assert spec["expected"](vaf, phred), (vaf, phred)
