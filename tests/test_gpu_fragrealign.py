"""Realignment of indel-bearing reads inside the fragment session on the GPU (vlr_fragpileup_open_realign, csrc/vlr_fragpileup.hip with
csrc/vlr_pairscore.h).  The realigned evidences (vlr_fragpileup_read_realigned) must equal the restatement (fragments.realign_evidence)
in every integer field and window coordinate; their raw scores and distances must equal, with == on f64, what the Python path returns
through the same kernels for the windows rebuilt from those coordinates, in all three modes; the observations must equal the CPU
restatement's (oracle/'s pair HMMs) in every integer field and within the kernel-vs-restatement bound of 1e-9 in
prob_ref / prob_alt; the bytes must not depend on window_bytes, the split into files or the ranges the evidences are scored in; the
counts around wave, block and scan edges; an overflow of the evidence capacity is reported with the exact need; and the command
`preprocess variants --realign-indel-reads` writes the records of write_observations(pileup(observations(..., realign=spec)))."""
import struct

import numpy as np
import pytest

import basecall_cases as bc
import fragment_cases as fc
import fragrealign_cases as rc
from varlociraptor_amd import abi, alignprops, basecalls, cli, engine, fragments, realign
from varlociraptor_amd.readwindows import read_bam, read_fasta

pytestmark = pytest.mark.gpu
NANOPORE_LIKE = (realign.GapParams(-9.0, -8.0, -1.5, -1.2), realign.HopParams((-6.0,) * 4, (-6.5,) * 4, (-1.0,) * 4, (-1.1,) * 4))
SPECS = {"exact": fragments.RealignSpec(64, "exact"), "fast": fragments.RealignSpec(64, "fast"),
         "homopolymer": fragments.RealignSpec(64, "homopolymer", *NANOPORE_LIKE)}
K_THREADS = 256   # vlr_ip::kThreads


def test_the_entry_point_is_exported():
    assert engine.lib().vlr_fragpileup_open_realign is not None and engine.lib().vlr_abi_version() == 14


class Case:
    """a BAM with its loci; the CPU restatement computed once per mode"""

    def __init__(self, tmp, name, contigs, cands, recs, props):
        self.contigs, self.cands, self.props, self.raw = contigs, cands, props, recs
        self.loci = bc.loci_of(cands, contigs)
        self.bam, self.fasta = bc.write_case(tmp, name, contigs, recs)
        self.records = read_bam(self.bam)[1]
        self.tmp = tmp
        self.cpu = {}

    def want(self, mode="exact"):
        if mode not in self.cpu:
            self.cpu[mode] = fragments.restate(self.records, self.loci, self.props, basecalls.library_tables(), realign=SPECS[mode], ref_seqs=rc.ref_seqs_of(self.contigs))
        return self.cpu[mode]

    def run(self, mode="exact", bams=None, **kw):
        return fragments.device_observations(bams or self.bam, self.loci, self.props, 0, realign=SPECS[mode], fasta=self.fasta, evidences=True, **kw)

    def check(self, mode="exact", **kw):
        obs, lrec, res, ev, rres = self.run(mode, **kw)
        rs = self.want(mode)
        assert res.status == 0 and (rres.n_evidences, rres.needed_evidences) == (len(rs.evidences), len(rs.evidences))
        # integer fields and window coordinates
        assert rc.hit_keys(ev) == rc.evidence_keys(rs.evidences)
        assert not ev["pad"].any()
        # raw scores and distances: the same kernels on the windows rebuilt from the coordinates
        pb = rc.windows_of(ev, self.contigs, self.loci, self.records, SPECS[mode].window)
        dist, lnp = fragments.score_pairs(pb, SPECS[mode], device=0)
        for got, exp in ((ev["ln_ref"], lnp[0::2]), (ev["ln_alt"], lnp[1::2]), (ev["dist_ref"], dist[0::2]), (ev["dist_alt"], dist[1::2])):
            assert got.tobytes() == np.ascontiguousarray(exp).tobytes()
        assert (rres.x_bytes, rres.y_bytes) == (sum(len(x) for x in pb.x), sum(len(y) for y in pb.y))
        # observations against the CPU restatement
        rc.assert_observations_close(obs, lrec, rs)
        assert not (obs["status"] & abi.BASEPILEUP_HIT_NEEDS_REALIGN).any()
        return obs, lrec, res, ev, rres


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    contigs, cands, recs, props = fc.synthetic(n_pairs=600)
    return Case(tmp_path_factory.mktemp("fragrealign"), "synth", contigs, cands, recs, props)


@pytest.mark.parametrize("mode", sorted(SPECS))
def test_evidences_scores_and_observations(synth, mode):
    obs, lrec, res, ev, rres = synth.check(mode)
    assert len(ev) > 30 and len(obs) > 300 and len({int(l) for l in ev["locus"]}) > 5
    scored = ev[ev["status"] == 0]
    assert (scored["dist_ref"] >= 0).all() and not np.isnan(scored["ln_ref"]).any()


def test_hand_records_on_the_device(tmp_path):
    recs = rc.hand_records()
    c = Case(tmp_path, "hand", {"c1": rc.REF}, [rc.SNV20, rc.MNV40], list(recs.values()), rc.P30)
    obs, lrec, res, ev, _ = c.check()
    assert len(ev) == 10 and set(ev["status"]) == {0}
    edge = rc.edge_records()
    for k, (label, (rec, cand)) in enumerate(edge.items()):
        c = Case(tmp_path, label, {"c1": rc.REF}, [cand], [rec], rc.P30)
        _, _, _, ev, _ = c.check()
        assert len(ev) == 1 and ev["status"][0] == 0, label
    contigs, cand, rec = rc.long_read_case()
    _, _, _, ev, _ = Case(tmp_path, "long", contigs, [cand], [rec], fragments.Props(200, 60, 151)).check()
    assert int(ev["read_len"][0]) == 128
    c = Case(tmp_path, "refused", {"c1": rc.REF}, [rc.SNV20], list(rc.refused_records().values()), rc.P30)
    obs, _, _, ev, _ = c.check()
    assert list(ev["status"]) == [abi.INDELPILEUP_HIT_LEADING_REFSKIP, abi.INDELPILEUP_HIT_STRAND_INFO]
    assert sorted(int(s) for s in obs["status"]) == [0, abi.BASEPILEUP_HIT_LEADING_REFSKIP, abi.FRAGPILEUP_OBS_REALIGN_STRAND_INFO]


def test_bytes_do_not_depend_on_feeds_files_or_ranges(synth):
    base = synth.run()
    assert base[4].n_ranges == 1
    small, _ = bc.write_case(synth.tmp, "small_members", synth.contigs, synth.raw, member_bytes=300)
    # window_bytes = 1: the smallest legal value, every feed one 300-byte BGZF member, a chunk holds a record or a few
    for wb in (1, 0):
        got = synth.run(bams=small, window_bytes=wb)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[3].tobytes() == base[3].tobytes(), wb
    half = len(synth.raw) // 2
    a, _ = bc.write_case(synth.tmp, "first_half", synth.contigs, synth.raw[:half])
    b, _ = bc.write_case(synth.tmp, "second_half", synth.contigs, synth.raw[half:])
    got = synth.run(bams=[a, b])
    assert got[0].tobytes() == base[0].tobytes() and got[3].tobytes() == base[3].tobytes() and got[2].n_records == len(synth.raw)
    # ranges, as for evidences whose pair bytes pass 2^31: cut every 1000 bytes
    got = synth.run(pair_byte_limit=1000)
    assert got[4].n_ranges > 5 and got[4].x_bytes > 5000
    assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[3].tobytes() == base[3].tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, K_THREADS - 1, K_THREADS, K_THREADS + 1])
def test_evidence_counts_at_wave_and_block_edges(tmp_path, n):
    contigs, cands, recs, props = rc.counted(n)
    _, _, _, ev, rres = Case(tmp_path, "count%d" % n, contigs, cands, recs, props).check()
    assert len(ev) == n and rres.n_ranges == (1 if n else 0)


@pytest.mark.parametrize("n_records", [1024, 1025])
def test_a_chunk_at_the_scan_edge(tmp_path, n_records):
    contigs, cands, recs, props = rc.counted(n_records // 4, n_records - n_records // 4)
    obs, lrec, res, ev, _ = Case(tmp_path, "scan%d" % n_records, contigs, cands, recs, props).check()
    assert res.n_records == n_records and len(ev) == n_records // 4


def test_evidence_overflow_is_reported_and_the_retry_succeeds(synth):
    need = len(synth.want().evidences)
    for cap, kw in ((need - 1, {}), (0, {}), (3, dict(bams=bc.write_case(synth.tmp, "small_again", synth.contigs, synth.raw, member_bytes=300)[0], window_bytes=1))):
        obs, lrec, res, ev, rres = synth.run(evidence_capacity=cap, retry=False, **kw)
        assert res.status == abi.FRAGPILEUP_EVIDENCE_OVERFLOW and rres.needed_evidences == need and rres.n_evidences == 0 and len(obs) == 0, cap   # (no GUARD_DAMAGED)
    obs, lrec, res, ev, rres = synth.run(evidence_capacity=need, retry=False)
    assert res.status == 0 and rres.n_evidences == need
    base = synth.run()
    got = synth.run(evidence_capacity=need - 1)       # the retry with the need
    assert got[2].status == 0 and got[0].tobytes() == base[0].tobytes() and got[3].tobytes() == base[3].tobytes()


def test_open_refuses_bad_windows(synth):
    for w in (0, 65):
        spec = fragments.RealignSpec(64, "exact")
        spec.window = w
        with pytest.raises(engine.EngineError):
            fragments.device_observations(synth.bam, synth.loci, synth.props, 0, realign=spec, fasta=synth.fasta)
    # the old entry still only flags
    obs, _, _ = fragments.device_observations(synth.bam, synth.loci, synth.props, 0, True)
    assert (obs["status"] & abi.BASEPILEUP_HIT_NEEDS_REALIGN).any()


def _candidates_vcf(path, rows):
    with open(path, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for chrom, pos0, ref, alt in rows:
            f.write("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (chrom, pos0 + 1, ref.decode(), alt.decode()))
    return str(path)


def _bcf_records(path):
    """the bytes of the BCF records behind the header"""
    d = alignprops.inflate_bgzf(path)
    l_text, = struct.unpack_from("<I", d, 5)
    return bytes(d[9 + l_text:])


def test_preprocess_variants_realigns_an_indel_bearing_read(tmp_path, capsys):
    from varlociraptor_amd import ingest
    case = {c.name: c for c in fc.hand_cases()}["softclip_behind_hardclip"]       # its record 3 carries an insertion over the locus
    bam, fa = fc.write_case(tmp_path, case)
    vcf = _candidates_vcf(tmp_path / "cand.vcf", case.candidates)
    pj = tmp_path / "props.json"
    pj.write_text('{"insert_size":null,"max_del_cigar_len":null,"max_ins_cigar_len":null,"frac_max_softclip":null,"max_read_len":12,"max_mapq":60}')
    out = str(tmp_path / "o.bcf")
    args = ["preprocess", "variants", fa, "--candidates", vcf, "--bam", bam, "--alignment-properties", str(pj), "--atomic-candidate-variants", "--output", out]
    cli.main(args + ["--realign-indel-reads"])
    spec = fragments.RealignSpec(64, "exact", realign.GapParams(), realign.HopParams())
    tabs = fragments.observations(bam, fa, case.candidates, case.props, device=0, realign_indel_reads=True, realign=spec)
    assert len(tabs[0]) == 4 and tabs[0].records[3] == (3,)
    batch, third = fragments.pileup(tabs, case.candidates)
    direct = str(tmp_path / "direct.bcf")
    ingest.write_observations(direct, batch, 0, third_allele_evidence=third, sites=[(c, p + 1, ".", r.decode(), a.decode()) for c, p, r, a in case.candidates])
    assert _bcf_records(out) == _bcf_records(direct) and len(_bcf_records(out)) > 100
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--realign-indel-reads", "--score-indel-reads-from-alignment"])
    assert e.value.code != 0 and "exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--realign-indel-reads", "--indel-window", "65"])
    assert e.value.code != 0
    # the refusals name the record
    c = Case(tmp_path, "refused", {"c1": rc.REF, "c2": rc.REF[:50]}, [rc.SNV20], list(rc.refused_records().values())[:2], rc.P30)
    with pytest.raises(fragments.LeadingRefSkip, match="record 1"):
        fragments.observations(c.bam, c.fasta, c.cands, c.props, device=0, realign=spec)


# testcase -> its `expected:` block is met by the CPU restatement with realignment (tests/golden/bam/REALIGNED.md); all four are
REALIGNED_FIXTURES = ("test_giab_02", "test_giab_03", "test_giab_30", "test_uzuner_clonal_1")


@pytest.mark.parametrize("name", REALIGNED_FIXTURES)
def test_reference_testcases_through_the_command_with_realignment(oracle, golden_dir, tmp_path, name):
    """preprocess variants --realign-indel-reads -> call variants: the call the oracle gives on the same batch, within the tolerances of
    test_gpu_fragpileup.test_preprocess_variants_end_to_end, and the testcase's own `expected:` block (test_giab_02 and test_giab_03:
    `NA12878 == 0.5`, missed without the realignment)"""
    import json
    import os
    import bam_pairs as bp
    from varlociraptor_amd.bcfio import BcfReader
    bam, held, scenario, cand, props = fc.fixture_case(golden_dir, name)
    fasta = str(tmp_path / "ref.fa")          # the testcases hold their reference without an index: a copy with its .fai
    alignprops.write_fasta(fasta, read_fasta(held))
    pj = os.path.join(golden_dir, "bam", name, "properties.json")
    vcf = _candidates_vcf(tmp_path / "cand.vcf", cand)
    out = str(tmp_path / "obs.bcf")
    cli.main(["preprocess", "variants", fasta, "--candidates", vcf, "--bam", bam, "--alignment-properties", pj, "--atomic-candidate-variants", "--realign-indel-reads",
              "--output", out])
    spec = fragments.RealignSpec(64, "exact", *fragments.gap_hop_of(json.load(open(pj))))
    tabs = fragments.observations(bam, fasta, cand, props, device=0, realign=spec)
    batch, _ = fragments.pileup(tabs, cand)
    sc = cli.scenario_from_yaml(scenario, contig=cand[0][0])
    sample, = list(sc.samples)
    calls = str(tmp_path / "calls.bcf")
    cli.main(["call", "variants", "--output", calls, "generic", "--scenario", scenario, "--obs", "%s=%s" % (sample, out)])
    rec, = list(BcfReader(calls))
    ref = oracle.call(sc, batch)
    vaf = float(rec["format"]["AF"][0][0]) if isinstance(rec["format"]["AF"][0], (list, tuple)) else float(rec["format"]["AF"][0])
    print(name, "observations", len(tabs[0]), "MAP VAF", vaf, "oracle", float(ref.map_vaf[0, 0]))
    assert abs(vaf - float(ref.map_vaf[0, 0])) <= 1e-6
    for ev, want in bp.phred_by_event(sc, ref.ln_posterior[0]).items():
        got = rec["info"][ev][0]
        assert abs(got - want) <= 3e-6 * max(1.0, abs(want)) or (np.isinf(want) and got > 3000), (ev, got, want)
    assert fc.FIXTURES[name][0](vaf, bp.phred_by_event(sc, ref.ln_posterior[0]))
