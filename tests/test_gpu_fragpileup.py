"""Fragment observations of SNV / MNV candidates on the GPU (vlr_fragpileup_*, csrc/vlr_fragpileup.hip): the kernels' observations and
locus records must equal the restatement's (varlociraptor_amd/fragments.py run on the library's own tables) field for field, f64
compared with ==, on the hand cases, the fixtures and the synthetic BAMs of tests/fragment_cases.py; the sort of the fragment kernel is
run at member counts around every power of two up to VLR_FRAGPILEUP_MAX_MEMBERS and one above it; the output bytes must not depend on
how the input is cut into feeds or files; overflows and a file cut inside a record are reported, not faults; and `observations` ->
`pileup` -> engine meets the `expected:` block of every testcase that tests/golden/bam/FRAGMENTS.md lists as met."""
import os
import struct

import numpy as np
import pytest

import bam_pairs as bp
import basecall_cases as bc
import fragment_cases as fc
from varlociraptor_amd import abi, alignprops, basecalls, cli, engine, fragments
from varlociraptor_amd.readwindows import read_bam, read_fasta

pytestmark = pytest.mark.gpu
MAX = abi.FRAGPILEUP_MAX_MEMBERS


@pytest.fixture(scope="module")
def tables():
    return basecalls.library_tables()


def check(bams, loci, props, tables, realign=False, **kw):
    obs, lrec, res = fragments.device_observations(bams, loci, props, 0, realign, **kw)
    recs = [r for b in ([bams] if isinstance(bams, str) else bams) for r in read_bam(b)[1]]
    rs = fragments.restate(recs, loci, props, tables, realign)
    fc.assert_same(obs, lrec, rs)
    assert (res.n_obs, res.n_members, res.n_records, res.n_rejected, res.status) == (len(obs), sum(rs.n_members), rs.n_records, rs.n_rejected, 0)
    assert res.needed_members == sum(rs.n_members) and res.first_bad_record == -1
    return obs, lrec, res


def test_hand_cases_equal_the_restatement_and_their_stated_expectations(tables, tmp_path):
    for case in fc.hand_cases():
        bam, fa = fc.write_case(tmp_path, case)
        loci, order = fc.loci_of(case)
        obs, lrec, _ = check(bam, loci, case.props, tables)
        per = [None] * len(order)
        for j, k in enumerate(order):
            per[k] = fragments.obs_from_array(obs[int(lrec[j]["obs_offset"]):int(lrec[j]["obs_offset"]) + int(lrec[j]["n_obs"])])
        stated = [[{f: v for f, v in w.items() if f not in ("alt_loci", "alt_locus", "major")} for w in ws] for ws in case.expect]
        fc.check_case(fc.Case(case.name, case.records, case.candidates, case.props, stated), per, per)
        if any(o.status for p in per for o in p):
            with pytest.raises(fragments.InvalidReadOrientationInfo):
                fragments.observations(bam, fa, case.candidates, case.props, device=0)
            continue
        # the front end (alt loci from the XA tags, MAPQ adjustment, prob_hit_base) against the stated classes and the restatement's tables
        dev = fragments.observations(bam, fa, case.candidates, case.props, device=0)
        stated = [[{f: v for f, v in w.items() if f != "alt_loci"} for w in ws] for ws in case.expect]
        fc.check_case(fc.Case(case.name, case.records, case.candidates, case.props, stated), dev, per)
        cpu = fragments.observations(bam, fa, case.candidates, case.props, device="cpu")
        for d, c in zip(dev, cpu):
            assert_tables_equal(d, c)


def assert_tables_equal(d, c):
    """a device table against a CPU table: the integer columns equal.  The f64 columns come from different tables: the library's may differ
    from Python's by 2 ulp per entry (test_gpu_basepileup.py), a support sums at most 2 x VLR_BASEPILEUP_MAX_LEN = 64 entries of one sign,
    each sum adding half an ulp: below 64 x 2.5 ulp = 3.6e-14 relative, so 1e-13 (the device against the restatement on the library's own
    tables is compared with == in `check`)"""
    for f in ("strand", "orientation", "read_position_major", "softclipped", "paired", "is_max_mapq", "alt_locus", "third_allele"):
        assert np.array_equal(getattr(d, f), getattr(c, f)), f
    assert d.records == c.records and d.major_read_position == c.major_read_position
    for f in ("prob_alt", "prob_ref", "prob_mapping", "prob_hit_base"):
        assert np.allclose(getattr(d, f), getattr(c, f), rtol=1e-13, atol=0, equal_nan=True), f


@pytest.fixture(scope="module")
def synth(tmp_path_factory, tables):
    tmp = tmp_path_factory.mktemp("fragsynth")
    contigs, cands, recs, props = fc.synthetic()
    loci = bc.loci_of(cands, contigs)
    bam, fa = bc.write_case(tmp, "synth", contigs, recs)
    small, _ = bc.write_case(tmp, "synth_small_members", contigs, recs, member_bytes=300)   # records straddle BGZF members
    rs = fragments.restate(read_bam(bam)[1], loci, props, tables)
    return dict(tmp=tmp, contigs=contigs, cands=cands, loci=loci, recs=recs, props=props, bam=bam, fa=fa, small=small, rs=rs)


def test_synthetic_paired_bam_equals_the_restatement(synth, tables):
    obs, lrec, res = check(synth["bam"], synth["loci"], synth["props"], tables)
    assert len(synth["recs"]) > 3000 and res.n_obs > 1000 and res.n_rejected > 10
    assert set(obs["strand"]) == {0, 1, 2} and (obs["right"] == abi.FRAGPILEUP_NO_RECORD).any() and (obs["bits"] & abi.FRAGPILEUP_HAS_XA).any()
    assert (obs["bits"] & abi.FRAGPILEUP_READPOS_MAJOR).any() and (obs["bits"] & abi.FRAGPILEUP_SOFTCLIPPED).any() and len(set(obs["orientation"])) >= 4
    assert (obs["min_mapq"] == 20).any() and (obs["third_allele"] > 0).any()
    check(synth["bam"], synth["loci"], synth["props"], tables, realign=True)
    # the front end against the CPU path, every candidate
    dev = fragments.observations(synth["bam"], synth["fa"], synth["cands"], synth["props"], device=0)
    cpu = fragments.observations(synth["bam"], synth["fa"], synth["cands"], synth["props"], device="cpu")
    assert any((d.alt_locus != abi.ALTLOCUS_NONE).any() for d in dev)
    for d, c in zip(dev, cpu):
        assert_tables_equal(d, c)


SORT_COUNTS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, MAX - 1, MAX, MAX + 1]


def test_sort_edges_and_a_locus_above_the_limit(tables, tmp_path):
    contigs, cands, recs, props = fc.deep_loci(SORT_COUNTS)
    loci = bc.loci_of(cands, contigs)
    bam, fa = bc.write_case(tmp_path, "deep", contigs, recs)
    obs, lrec, res = check(bam, loci, props, tables)
    assert [int(x) for x in lrec["n_members"]] == SORT_COUNTS and res.n_loci_too_deep == 1
    assert [int(s) for s in lrec["status"]] == [0] * (len(SORT_COUNTS) - 1) + [abi.FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS]
    assert int(lrec[-2]["n_obs"]) > MAX // 2
    # the front end finishes the flagged locus with the restatement: the last two candidates through both paths
    dev = fragments.observations(bam, fa, cands[-2:], props, device=0)
    cpu = fragments.observations(bam, fa, cands[-2:], props, device="cpu")
    assert len(dev[1]) == len(cpu[1]) > MAX // 2
    for d, c in zip(dev, cpu):
        assert_tables_equal(d, c)


def test_alt_loci_at_the_limit_of_the_key_sort_and_above_it(tables, tmp_path):
    """256 x 16 = VLR_FRAGPILEUP_MAX_MEMBERS keys are sorted on the device; 300 x 14 come back flagged and the front end finishes the locus"""
    for case, flagged in ((fc.xa_heavy(256, 16), False), (fc.xa_heavy(300, 14), True)):
        bam, fa = fc.write_case(tmp_path, case)
        loci, _ = fc.loci_of(case)
        obs, lrec, res = check(bam, loci, case.props, tables)
        assert bool(lrec[0]["status"] & abi.FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI) == flagged and res.n_loci_too_deep == int(flagged)
        dev = fragments.observations(bam, fa, case.candidates, case.props, device=0)
        cpu = fragments.observations(bam, fa, case.candidates, case.props, device="cpu")
        assert_tables_equal(dev[0], cpu[0])
        assert list(dev[0].alt_locus) == [abi.ALTLOCUS_SOME] + [abi.ALTLOCUS_MAJOR] * (len(case.records) - 1)


def test_bytes_do_not_depend_on_the_feeds_the_files_or_the_run(synth):
    loci, props = synth["loci"], synth["props"]
    base = fragments.device_observations(synth["bam"], loci, props)
    again = fragments.device_observations(synth["bam"], loci, props)
    assert base[0].tobytes() == again[0].tobytes() and base[1].tobytes() == again[1].tobytes() and len(base[0]) > 1000
    # window_bytes = 1, the smallest legal value: every feed is one 300-byte BGZF member; then one member record's worth; then a few KiB
    for wb in (1, 64, 4096):
        got = fragments.device_observations(synth["small"], loci, props, window_bytes=wb)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[2].status == 0, wb
    # the input split into two files between the mates of a pair that forms an observation
    recs = synth["recs"]
    pair = next(o for o in base[0] if o["right"] != abi.FRAGPILEUP_NO_RECORD and o["right"] > o["left"] + 3)
    cut = int(pair["left"]) + 1
    assert cut <= int(pair["right"])
    a, _ = bc.write_case(synth["tmp"], "part_a", synth["contigs"], recs[:cut])
    b, _ = bc.write_case(synth["tmp"], "part_b", synth["contigs"], recs[cut:])
    got = fragments.device_observations([a, b], loci, props)
    assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[2].n_records == len(recs)


def test_overflow_of_each_capacity_is_reported_and_the_retry_succeeds(synth):
    loci, props, rs = synth["loci"], synth["props"], synth["rs"]
    base = fragments.device_observations(synth["bam"], loci, props)
    need_m, need_n, need_k = int(base[2].needed_members), int(base[2].needed_name_bytes), int(base[2].needed_keys)
    assert need_m == sum(rs.n_members) and need_n > need_m and need_k > 10
    obs, lrec, res = fragments.device_observations(synth["bam"], loci, props, key_capacity=need_k - 1, retry=False)
    assert res.status == abi.FRAGPILEUP_KEY_OVERFLOW and res.needed_keys == need_k and res.needed_members == need_m and len(obs) == 0
    obs, lrec, res = fragments.device_observations(synth["bam"], loci, props, member_capacity=need_m - 1, retry=False)
    assert res.status == abi.FRAGPILEUP_MEMBER_OVERFLOW and res.needed_members == need_m and res.needed_name_bytes == need_n and len(obs) == 0   # (no GUARD_DAMAGED)
    obs, lrec, res = fragments.device_observations(synth["bam"], loci, props, name_capacity=need_n - 1, retry=False)
    assert res.status == abi.FRAGPILEUP_NAME_OVERFLOW and res.needed_name_bytes == need_n and len(obs) == 0
    obs, lrec, res = fragments.device_observations(synth["small"], loci, props, member_capacity=7, name_capacity=5, key_capacity=1, retry=False, window_bytes=1)   # in the first of many chunks
    assert res.status == abi.FRAGPILEUP_ANY_OVERFLOW and (res.needed_members, res.needed_name_bytes, res.needed_keys) == (need_m, need_n, need_k)
    obs, lrec, res = fragments.device_observations(synth["bam"], loci, props, member_capacity=0, name_capacity=0, key_capacity=0, retry=False)
    assert res.status == abi.FRAGPILEUP_ANY_OVERFLOW
    got = fragments.device_observations(synth["bam"], loci, props, member_capacity=3, name_capacity=3, key_capacity=0)    # the retry with the needed capacities
    assert got[2].status == 0 and got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()
    got = fragments.device_observations(synth["bam"], loci, props, member_capacity=need_m, name_capacity=need_n, key_capacity=need_k, retry=False)   # exactly enough
    assert got[2].status == 0 and got[0].tobytes() == base[0].tobytes()


def test_a_file_cut_inside_a_record_is_malformed_input_not_a_fault(synth, tables):
    contigs, recs, loci, props = synth["contigs"], synth["recs"], synth["loci"], synth["props"]
    last = recs[-1]
    head = alignprops.encode_bam([(c, len(s)) for c, s in contigs.items()], recs[:-1])
    front, _ = bc.write_case(synth["tmp"], "front", contigs, recs[:-1])
    want = fragments.device_observations(front, loci, props)
    for name, tail in (("ends_in_the_name", last[:36 + 2]), ("block_size_of_the_cut", struct.pack("<I", len(last) - 6) + last[4:len(last) - 2])):
        path = str(synth["tmp"] / (name + ".bam"))
        with open(path, "wb") as f:
            f.write(alignprops.bgzf_compress(head + tail))
        obs, lrec, res = fragments.device_observations(path, loci, props)
        assert res.status == abi.FRAGPILEUP_BAD_RECORD and res.first_bad_record == len(recs) - 1
        assert obs.tobytes() == want[0].tobytes() and lrec.tobytes() == want[1].tobytes()
        with pytest.raises(fragments.FragPileupError):
            fragments.observations(path, synth["fa"], synth["cands"][:2], props, device=0)
    check(synth["bam"], loci, props, tables)     # and the device is fine afterwards


def test_open_refuses_bad_arguments():
    L = [basecalls.Locus(abi.BASEPILEUP_SNV, 0, 10, b"A", b"C")]
    with pytest.raises(engine.EngineError):
        fragments.device_observations("/nonexistent.bam", L, fragments.Props(100, 60, 0))          # max_read_len <= 0
    with pytest.raises(engine.EngineError):
        fragments.device_observations("/nonexistent.bam", L, fragments.Props(-1, 60, 100))         # a negative window
    with pytest.raises(engine.EngineError):
        fragments.device_observations("/nonexistent.bam", L + [basecalls.Locus(abi.BASEPILEUP_SNV, 0, 5, b"A", b"C")], fragments.Props(100, 60, 100))   # not sorted


@pytest.mark.parametrize("name", sorted(fc.FIXTURES))
def test_fixture_observations_and_call(oracle, golden_dir, tables, name):
    bam, fasta, scenario, cand, props = fc.fixture_case(golden_dir, name)
    contigs, _ = alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)
    seqs = read_fasta(fasta)
    loci = [basecalls.locus(seqs[c], [n for n, _ in contigs].index(c), p, r, a) for c, p, r, a in cand]
    obs, lrec, res = check(bam, loci, props, tables)
    assert res.n_obs > 0
    dev = fragments.observations(bam, fasta, cand, props, device=0)
    cpu = fragments.observations(bam, fasta, cand, props, device="cpu")
    assert_tables_equal(dev[0], cpu[0])
    # end to end: the kernels' observations as a pileup through the engine, against the oracle and the testcase's own expectation
    batch, _ = fragments.pileup(dev, cand)
    sc = cli.scenario_from_yaml(scenario, contig=cand[0][0])
    plan = engine.Plan(sc)
    got = plan.call_host(batch)
    plan.close()
    ref = oracle.call(sc, batch)
    assert np.allclose(np.exp(got.ln_posterior), np.exp(ref.ln_posterior), atol=1e-6, rtol=0) and abs(got.map_vaf[0, 0] - ref.map_vaf[0, 0]) <= 1e-6
    pred, listed = fc.FIXTURES[name]
    assert bool(pred(float(got.map_vaf[0, 0]), bp.phred_by_event(sc, got.ln_posterior[0]))) == listed, float(got.map_vaf[0, 0])


# ---------------------------------------------------------------------------------------------- preprocess variants
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


@pytest.mark.parametrize("name", ["test_giab_30", "test_uzuner_clonal_1"])
def test_preprocess_variants_end_to_end(oracle, golden_dir, tmp_path, name):
    from varlociraptor_amd import ingest
    from varlociraptor_amd.bcfio import BcfReader
    bam, fasta, scenario, cand, props = fc.fixture_case(golden_dir, name)
    vcf = _candidates_vcf(tmp_path / "cand.vcf", cand)
    out = str(tmp_path / "obs.bcf")
    cli.main(["preprocess", "variants", fasta, "--candidates", vcf, "--bam", bam, "--alignment-properties", os.path.join(golden_dir, "bam", name, "properties.json"),
              "--atomic-candidate-variants", "--score-indel-reads-from-alignment", "--output", out])
    # byte for byte the records of write_observations(fragments.pileup(...))
    tabs = fragments.observations(bam, fasta, cand, props, device=0)
    batch, third = fragments.pileup(tabs, cand)
    direct = str(tmp_path / "direct.bcf")
    ingest.write_observations(direct, batch, 0, third_allele_evidence=third, sites=[(c, p + 1, ".", r.decode(), a.decode()) for c, p, r, a in cand])
    assert _bcf_records(out) == _bcf_records(direct) and len(_bcf_records(out)) > 100
    # `call variants` on the file: the call the oracle gives on the same batch, and the testcase's own expectation
    sc = cli.scenario_from_yaml(scenario, contig=cand[0][0])
    sample, = list(sc.samples)
    calls = str(tmp_path / "calls.bcf")
    cli.main(["call", "variants", "--output", calls, "generic", "--scenario", scenario, "--obs", "%s=%s" % (sample, out)])
    rec, = list(BcfReader(calls))
    ref = oracle.call(sc, batch)
    assert (rec["chrom"], rec["pos"], rec["ref"], rec["alt"]) == (cand[0][0], cand[0][1] + 1, cand[0][2].decode(), cand[0][3].decode())
    vaf = float(rec["format"]["AF"][0][0]) if isinstance(rec["format"]["AF"][0], (list, tuple)) else float(rec["format"]["AF"][0])
    assert abs(vaf - float(ref.map_vaf[0, 0])) <= 1e-6
    for ev, want in bp.phred_by_event(sc, ref.ln_posterior[0]).items():
        got = rec["info"][ev][0]
        assert abs(got - want) <= 3e-6 * max(1.0, abs(want)) or (np.isinf(want) and got > 3000), (ev, got, want)
    assert fc.FIXTURES[name][0](vaf, bp.phred_by_event(sc, ref.ln_posterior[0]))


def test_preprocess_variants_refusals(golden_dir, tmp_path, capsys):
    bam, fasta, _, cand, _ = fc.fixture_case(golden_dir, "test_giab_30")
    pj = os.path.join(golden_dir, "bam", "test_giab_30", "properties.json")
    vcf = _candidates_vcf(tmp_path / "cand.vcf", cand)
    out = str(tmp_path / "obs.bcf")
    base = ["preprocess", "variants", fasta, "--bam", bam, "--alignment-properties", pj, "--output", out]
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--candidates", vcf])
    assert e.value.code != 0 and "--atomic-candidate-variants" in capsys.readouterr().err
    indel = _candidates_vcf(tmp_path / "indel.vcf", [(cand[0][0], 300, b"TG", b"T")])
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--candidates", indel, "--atomic-candidate-variants"])
    err = capsys.readouterr().err
    assert e.value.code != 0 and "%s:301 TG>T" % cand[0][0] in err and "not an SNV or MNV" in err
    assert not os.path.exists(out)


def test_preprocess_variants_names_a_read_that_needs_realignment(tmp_path, capsys):
    case = {c.name: c for c in fc.hand_cases()}["softclip_behind_hardclip"]       # its record 3 carries an insertion over the locus
    bam, fa = fc.write_case(tmp_path, case)
    vcf = _candidates_vcf(tmp_path / "cand.vcf", case.candidates)
    pj = tmp_path / "props.json"
    pj.write_text('{"insert_size":null,"max_del_cigar_len":null,"max_ins_cigar_len":null,"frac_max_softclip":null,"max_read_len":12,"max_mapq":60}')
    args = ["preprocess", "variants", fa, "--candidates", vcf, "--bam", bam, "--alignment-properties", str(pj), "--atomic-candidate-variants", "--output", str(tmp_path / "o.bcf")]
    with pytest.raises(SystemExit) as e:
        cli.main(args)
    err = capsys.readouterr().err
    assert e.value.code != 0 and "record 3" in err and "NEEDS_REALIGN" in err
    cli.main(args + ["--score-indel-reads-from-alignment", "--max-depth", "2"])
    assert "1 of 1 loci have more than --max-depth 2" in capsys.readouterr().err and os.path.getsize(tmp_path / "o.bcf") > 0
