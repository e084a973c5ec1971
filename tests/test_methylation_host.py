"""Methylation candidates of `preprocess variants` on the CPU (no GPU): the restatement of varlociraptor_amd/methylation.py against
expectations stated from the records (tests/methylation_cases.py) and against the recordings of the reference's five methylation
testcases, and csrc/vlr_fragpileup_host.cpp — the text of csrc/vlr_methylation.h compiled with -fsanitize=address,undefined into a
stand-alone program (nothing is preloaded into any process; every record, the members, the name and key pools lie in heap blocks of
exactly their size) — against that restatement, f64 compared with ==."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import host_program
import methylation_cases as mc
from varlociraptor_amd import abi, basecalls, fragments, methylation
from varlociraptor_amd.readwindows import read_bam

sys.path.insert(0, os.path.join(host_program.ROOT, "tools"))

T, MT = basecalls.TABLES, methylation.METH_TABLES


def restated(tmp, cases, name="case"):
    bam, _ = mc.write_bam(tmp, name, cases.records)
    return methylation.restate(read_bam(bam)[1], mc.LOCI, mc.PROPS, cases.readtype)


@pytest.mark.parametrize("cases", mc.all_cases(), ids=lambda c: c.readtype)
def test_restatement_gives_the_stated_observations(cases, tmp_path):
    rs = restated(tmp_path, cases)
    assert rs.n_members == [len(cases.records)] and not rs.bad_records and rs.n_rejected == 0
    mc.check_expectations(cases, rs.per_locus[0], T, MT)
    assert sum(e is not None for e in cases.expect.values()) == len(rs.per_locus[0]) > 10


def test_orientation_and_flag_rule_tables():
    # read_reverse_orientation over the accepted flags, and what the flag rule refuses
    assert [methylation.reverse_orientation(f) for f in (0, 16, 83, 99, 147, 163)] == [False, True, True, False, False, True]
    assert methylation.VALID_FLAGS == (0, 16, 83, 99, 147, 163)
    # the two tables of annotated reads: ln((ml + 0.5) / 256) and the complement; ml = 255 is not certainty
    assert MT.ln_meth[0] == np.log(0.5 / 256) and MT.ln_meth[255] == np.log(255.5 / 256) < 0
    assert all(abs(np.exp(a) + np.exp(b) - 1.0) < 1e-15 for a, b in zip(MT.ln_meth, MT.ln_unmeth))


def test_accept_any_flag_switches_only_the_flag_rule(tmp_path):
    cases = mc.converted_cases()
    bam, _ = mc.write_bam(tmp_path, "anyflag", cases.records)
    recs = read_bam(bam)[1]
    strict = methylation.restate(recs, mc.LOCI, mc.PROPS, "converted").per_locus[0]
    loose = methylation.restate(recs, mc.LOCI, mc.PROPS, "converted", accept_any_flag=True).per_locus[0]
    extra = {o.left for o in loose} - {o.left for o in strict}
    assert extra == {cases.first["flag_%d" % f] for f in (65, 97, 2048, 2064)}
    assert [o.key() for o in loose if o.left not in extra] == [o.key() for o in strict]


@pytest.mark.parametrize("name", sorted(mc.error_cases()))
def test_what_the_reference_fails_on_is_a_status(name, tmp_path):
    readtype, records, status = mc.error_cases()[name]
    bam, _ = mc.write_bam(tmp_path, name, records)
    obs = methylation.restate(read_bam(bam)[1], mc.LOCI, mc.PROPS, readtype).per_locus[0]
    assert [(o.status, o.prob_ref, o.prob_alt, o.read_position) for o in obs] == [(status, 0.0, 0.0, None)]
    with pytest.raises((fragments.FragPileupError, ValueError)):
        fragments.table_of(obs, mc.PROPS, T)


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_long_annotated_record(rev):
    ref, rec, loci, called = mc.long_record(rev)
    from varlociraptor_amd import alignprops
    recs = read_bam_bytes(alignprops.encode_bam([("m1", len(ref))], [rec]))
    rs = methylation.restate(recs, loci, fragments.Props(len(ref), 60, 20000), "annotated")
    assert len(loci) > 250 and sum(v is not None for v in called.values()) >= len(loci) // 3
    for loc, obs in zip(loci, rs.per_locus):
        o, = obs
        ml = called[loc.start]
        want = (MT.ln_unmeth[ml], MT.ln_meth[ml]) if ml is not None else (0.0, -np.inf)
        assert (o.prob_ref, o.prob_alt, o.read_position) == want + (loc.start + (1 if rev else 0) - 100,)


def read_bam_bytes(data):
    import gzip
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".bam") as f:
        f.write(gzip.compress(data))
        f.flush()
        return read_bam(f.name)[1]


# ---------------------------------------------------------------------------------------------- the held testcases
@pytest.fixture(scope="module")
def tool():
    import make_methylation_fixtures
    return make_methylation_fixtures


@pytest.mark.parametrize("name", mc.FIXTURES)
def test_fixture_reproduces_the_recordings(oracle, tool, name):
    """Observation counts equal the recorded ones; prob_ref / prob_alt as sorted multisets after the writer's MiniLogProb coding: the
    f16-coded values bit-equal, the f32-coded ones within twice the largest deviation tools/make_methylation_fixtures.py measured
    (METHYLATION.md; one f32 rounding of values near 1: 2e-7).  The annotated case's recordings predate the flag rule: they are compared
    with accept_any_flag=True, and the rule as the source has it gives 22 of the 24.  Every case meets its `expected:` block."""
    _, _, _, _, case, recorded = tool.load_case(name)
    annotated = case["methylation_readtype"] == "annotated"
    cand, tab = tool.case_tables(name)
    cmp_tab = tool.case_tables(name, accept_any_flag=True)[1] if annotated else tab
    assert len(cmp_tab) == len(recorded["prob_ref"]) == mc.RECORDED_COUNTS[name]
    if annotated:
        assert len(tab) == mc.PACBIO_WITH_FLAG_RULE
    f16_equal, worst, where = tool.deviation(cmp_tab, recorded)
    print(name, "f16 equal:", f16_equal, "largest f32 deviation:", worst, where)
    assert f16_equal
    bound = 2.0 * mc.max_f32_deviation()
    assert 0.0 < bound < 1e-6 and worst <= bound, (worst, where)
    vafs, ph, ok = tool.call(name, cand, tab)
    print(name, vafs, case["expected"])
    assert ok, (vafs, ph)


# ---------------------------------------------------------------------------------------------- the host program
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "vlr_fragpileup_host")


def run_program(program, tmp, blob, tag="m"):
    paths = [os.path.join(str(tmp), tag + n) for n in ("in.bin", "out.bin")]
    with open(paths[0], "wb") as f:
        f.write(blob)
    if os.path.exists(paths[1]):
        os.remove(paths[1])
    r = subprocess.run([program] + paths, capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return r.returncode, (open(paths[1], "rb").read() if r.returncode == 0 else None)


def same_as_restatement(program, tmp, readtype, loci, records, props=mc.PROPS, contigs=None):
    rc, data = run_program(program, tmp, mc.pack_host_input(readtype, loci, records, props))
    assert rc == 0
    call, mis, ln_meth, ln_unmeth, obs, loc, cls = mc.parse_host_output(data, len(loci), len(records))
    bam, _ = mc.write_bam(tmp, "hp", records, contigs)
    t = basecalls.Tables(list(call), list(mis))
    mt = methylation.MethTables(list(ln_meth), list(ln_unmeth))
    rs = methylation.restate(read_bam(bam)[1], loci, props, readtype, t, mt)
    assert not cls.any() and not obs["pad"].any()
    for j in range(len(loci)):
        sl = slice(int(loc[j]["obs_offset"]), int(loc[j]["obs_offset"]) + int(loc[j]["n_obs"]))
        assert [o.key() for o in fragments.obs_from_array(obs[sl])] == [o.key() for o in rs.per_locus[j]], j
        assert int(loc[j]["n_members"]) == rs.n_members[j] and int(loc[j]["status"]) == 0
        mj = fragments.major_read_position(rs.per_locus[j])
        assert int(loc[j]["major_read_position"]) == (abi.BASEPILEUP_NO_READ_POSITION if mj is None else mj)
    return obs, t, mt


def test_host_tables_are_the_python_ones(program, tmp_path):
    rc, data = run_program(program, tmp_path, mc.pack_host_input("annotated", mc.LOCI, []))
    _, _, ln_meth, ln_unmeth, obs, _, _ = mc.parse_host_output(data, 1, 0)
    assert rc == 0 and len(obs) == 0 and list(ln_meth) == MT.ln_meth and list(ln_unmeth) == MT.ln_unmeth


@pytest.mark.parametrize("cases", mc.all_cases(), ids=lambda c: c.readtype)
def test_host_program_equals_restatement_on_the_hand_cases(cases, program, tmp_path):
    obs, t, mt = same_as_restatement(program, tmp_path, cases.readtype, mc.LOCI, cases.records)
    mc.check_expectations(cases, fragments.obs_from_array(obs), t, mt)


def test_host_program_on_errors_and_the_long_records(program, tmp_path):
    for name, (readtype, records, status) in mc.error_cases().items():
        obs, _, _ = same_as_restatement(program, tmp_path, readtype, mc.LOCI, records)
        assert list(obs["status"]) == [status], name
    for rev in (False, True):
        ref, rec, loci, _ = mc.long_record(rev, n=3000, n_loci=60)
        obs, _, _ = same_as_restatement(program, tmp_path, "annotated", loci, [rec], fragments.Props(len(ref), 60, 3000), {"m1": ref})
        assert len(obs) == len(loci)


def test_host_program_on_damaged_inputs(program, tmp_path):
    """truncated and overwritten copies of the annotated hand cases: every run ends with the program's output or its refusal (2: an
    input it cannot read, 3: count and fill differ), never a sanitizer report; a record that no longer decodes is classed bad"""
    cases = mc.annotated_cases()
    blob = mc.pack_host_input("annotated", mc.LOCI, cases.records)
    head = len(blob) - sum(len(r) for r in cases.records)
    rng = random.Random(5)
    for cut in [3, 4, 30, head - 1, head, head + 17, len(blob) - 40, len(blob) - 1]:
        rc, _ = run_program(program, tmp_path, blob[:cut], "cut")
        assert rc == 2, cut
    ran = 0
    for k in range(60):
        b = bytearray(blob)
        if k % 2:      # inside the aux fields of the records: tag names, types, the MM text, the ML counts
            at = rng.randrange(head, len(b))
            b[at] = rng.choice([0, 1, ord(","), ord(";"), ord("C"), ord("Z"), ord("B"), 0xff])
        else:
            for _ in range(4):
                b[rng.randrange(head, len(b))] = rng.randrange(256)
        rc, data = run_program(program, tmp_path, bytes(b), "ow")
        assert rc in (0, 2, 3), (k, rc)
        if rc == 0:
            ran += 1
            obs = mc.parse_host_output(data, 1, len(cases.records))[4]
            assert np.isin(obs["status"], [0, abi.BASEPILEUP_HIT_LEADING_REFSKIP, abi.BASEPILEUP_HIT_INVALID_STRAND_INFO, abi.BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS,
                                           abi.FRAGPILEUP_OBS_INVALID_RO]).all()
    assert ran > 30


# ---------------------------------------------------------------------------------------------- the command
def command_case(tmp_path, cases, extra=()):
    bam, fa = mc.write_bam(tmp_path, "cmd", cases.records)
    vcf, props = os.path.join(str(tmp_path), "c.vcf"), os.path.join(str(tmp_path), "p.json")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=m1>\n##ALT=<ID=METH,Description=\"methylation\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        f.write("m1\t%d\t.\tC\t<METH>\t.\t.\t.\n" % (mc.CPG + 1))
        for row in extra:
            f.write("m1\t%d\t.\t%s\t%s\t.\t.\t.\n" % row)
    json.dump({"insert_size": None, "max_del_cigar_len": None, "max_ins_cigar_len": None, "frac_max_softclip": None, "max_read_len": 190, "max_mapq": 60}, open(props, "w"))
    return fa, vcf, bam, props


def test_command_refuses_without_the_flag_with_todays_text(tmp_path):
    fa, vcf, bam, props = command_case(tmp_path, mc.converted_cases())
    out = os.path.join(str(tmp_path), "o.bcf")
    with pytest.raises(fragments.PreprocessError, match=r"candidate m1:101 C><METH> is not an SNV or MNV: indel, structural and breakend candidates are not built"):
        fragments.preprocess_variants(fa, vcf, bam, out, props, "cpu", True)
    with pytest.raises(fragments.PreprocessError, match=r"candidate m1:101 C><METH> is a symbolic or breakend allele: only SNVs, MNVs, deletions and insertions are built"):
        fragments.preprocess_variants(fa, vcf, bam, out, props, "cpu", True, indel_candidates=fragments.RealignSpec())
    with pytest.raises(fragments.PreprocessError, match="--methylation-read-type must be one of"):
        fragments.preprocess_variants(fa, vcf, bam, out, props, "cpu", True, methylation_readtype="bisulfite")
    assert not os.path.exists(out)


@pytest.mark.parametrize("cases", mc.all_cases(), ids=lambda c: c.readtype)
def test_command_writes_a_file_the_decoder_reads_back(cases, tmp_path):
    """`preprocess variants --methylation-read-type … --device cpu` on a file that mixes the <METH> candidate with an SNV: the observation
    BCF read back through ingest carries, in candidate order, the restatement's observations, the variant class of a symbolic allele
    that is no indel or SV, no ref / alt base, prob_sample_alt = ln 1"""
    from varlociraptor_amd import cli, ingest
    snv_at = mc.CPG - 6
    other = "A" if mc.REF[snv_at:snv_at + 1] != b"A" else "C"
    fa, vcf, bam, props = command_case(tmp_path, cases, extra=[(snv_at + 1, mc.REF[snv_at:snv_at + 1].decode(), other)])
    out = os.path.join(str(tmp_path), "o.bcf")
    cli.main(["preprocess", "variants", fa, "--candidates", vcf, "--bam", bam, "--alignment-properties", props, "--atomic-candidate-variants",
              "--score-indel-reads-from-alignment", "--methylation-read-type", cases.readtype, "--device", "cpu", "--output", out])
    batch, sites = ingest.read_observations([out])
    cands = [("m1", mc.CPG, b"C", b"<METH>"), ("m1", snv_at, mc.REF[snv_at:snv_at + 1], other.encode())]
    want = fragments.observations(bam, fa, cands, json.load(open(props)), device="cpu", methylation_readtype=cases.readtype)
    off = batch.obs_offset
    assert batch.n_loci == 2 and [int(off[k + 1] - off[k]) for k in range(2)] == [len(t) for t in want] and len(want[0]) > 10 and len(want[1]) > 10
    assert list(batch.locus["variant_type"]) == [abi.VT_OTHER, abi.VT_SNV] and batch.locus["ref_base"][0] == 0 and batch.locus["alt_base"][0] == 0
    assert [tuple(s[:4]) for s in sites][0][2:] == ("C", "<METH>")
    from varlociraptor_amd.synth import minilogprob_round
    sl = slice(int(off[0]), int(off[1]))
    for col, arr in (("prob_alt", want[0].prob_alt), ("prob_ref", want[0].prob_ref)):
        a, b = batch.columns[col][sl].astype(float), minilogprob_round(arr).astype(float)
        fin = np.isfinite(b)
        assert (a[fin] == b[fin]).all() and (a[~fin] < -1e30).all(), col
    assert (batch.columns["prob_sample_alt"][sl] == 0.0).all()
    # the SNV record of the mixed file is what the path writes for it alone
    alone = fragments.observations(bam, fa, cands[1:], json.load(open(props)), device="cpu")[0]
    assert (alone.prob_alt == want[1].prob_alt).all() and alone.records == want[1].records
