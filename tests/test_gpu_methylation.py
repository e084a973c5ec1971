"""Methylation candidates in the fragment session on the device (vlr_fragpileup_open_methylation, csrc/vlr_fragpileup.hip over
csrc/vlr_methylation.h) against the restatement of varlociraptor_amd/methylation.py run on the library's own tables: every field of
every observation and locus record with ==, f64 included, on the hand cases of tests/methylation_cases.py (which also state what each
fragment must give), on the reference's five methylation testcases, at wave edges, at the deepest locus, on a 20 000-base annotated
record that is a member of 300 loci; the output bytes do not depend on how the input is cut into feeds or files; overflows and a file
cut inside a record are reported, not faults; and `preprocess variants --methylation-read-type` -> `call variants generic` meets the
`expected:` block of every testcase.  Every test here needs the entry point or the flag, which the parent commit does not have."""
import io
import json
import os
import random
import struct
import sys

import numpy as np
import pytest

import basecall_cases as bc
import methylation_cases as mc
from varlociraptor_amd import abi, alignprops, basecalls, cli, engine, fragments, methylation
from varlociraptor_amd.readwindows import read_bam, read_fasta

pytestmark = pytest.mark.gpu
M = methylation


@pytest.fixture(scope="module")
def tables():
    return basecalls.library_tables(), M.library_meth_tables()


def device(bams, loci, readtype, props=mc.PROPS, **kw):
    return M.device_observations(bams, loci, props, readtype, 0, **kw)


def check(bams, loci, readtype, tables, props=mc.PROPS, **kw):
    """the device's observations and locus records equal the restatement's, field for field"""
    t, mt = tables
    obs, lrec, res = device(bams, loci, readtype, props, **kw)
    recs = [r for b in ([bams] if isinstance(bams, str) else bams) for r in read_bam(b)[1]]
    rs = M.restate(recs, loci, props, readtype, t, mt)
    assert res.status == 0 and res.n_records == len(recs) and res.n_rejected == rs.n_rejected and res.n_members == sum(rs.n_members) and not obs["pad"].any()
    assert res.n_obs == sum(len(x) for x in rs.per_locus)
    for j in range(len(loci)):
        sl = slice(int(lrec[j]["obs_offset"]), int(lrec[j]["obs_offset"]) + int(lrec[j]["n_obs"]))
        assert [o.key() for o in fragments.obs_from_array(obs[sl])] == [o.key() for o in rs.per_locus[j]], j
        mj = fragments.major_read_position(rs.per_locus[j])
        assert (int(lrec[j]["n_members"]), int(lrec[j]["status"]), int(lrec[j]["major_read_position"])) == \
            (rs.n_members[j], 0, abi.BASEPILEUP_NO_READ_POSITION if mj is None else mj), j
        major = [bool(b & abi.FRAGPILEUP_READPOS_MAJOR) for b in obs[sl]["bits"]]
        assert major == [mj is not None and o.status == 0 and o.read_position == mj for o in rs.per_locus[j]], j
    return obs, lrec, res, rs


def test_library_tables_are_the_python_ones(tables):
    assert tables[1].ln_meth == M.METH_TABLES.ln_meth and tables[1].ln_unmeth == M.METH_TABLES.ln_unmeth


@pytest.mark.parametrize("cases", mc.all_cases(), ids=lambda c: c.readtype)
def test_hand_cases(cases, tables, tmp_path):
    bam, _ = mc.write_bam(tmp_path, "hand", cases.records)
    obs, lrec, res, rs = check(bam, mc.LOCI, cases.readtype, tables)
    mc.check_expectations(cases, fragments.obs_from_array(obs), *tables)
    assert len(obs) > 10
    # many small BGZF members: records straddle them
    bam2, _ = mc.write_bam(tmp_path, "hand_small", cases.records, member_bytes=300)
    assert device(bam2, mc.LOCI, cases.readtype)[0].tobytes() == obs.tobytes()


@pytest.mark.parametrize("name", sorted(mc.error_cases()))
def test_what_the_reference_fails_on_is_a_status(name, tables, tmp_path):
    readtype, records, status = mc.error_cases()[name]
    bam, fa = mc.write_bam(tmp_path, name, records)
    obs, _, _, _ = check(bam, mc.LOCI, readtype, tables)
    assert [(int(o["status"]), float(o["prob_ref"]), float(o["prob_alt"]), int(o["read_position"])) for o in obs] == [(status, 0.0, 0.0, abi.BASEPILEUP_NO_READ_POSITION)]
    with pytest.raises((fragments.FragPileupError, ValueError)):
        fragments.observations(bam, fa, [("m1", mc.CPG, b"C", b"<METH>")], mc.PROPS, device=0, methylation_readtype=readtype)


def many(n, seed=0, annotated=False):
    """n records over the CpG, coordinate sorted: every accepted flag and 65, pairs and single reads, C / T / N / a mutation at the
    position; annotated: each with a 5mC call at its C / G of the CpG (at its first C / G where the position holds another base)"""
    rng = random.Random(seed * 7919 + n)
    recs = []
    for k in range(n):
        pos = 71 + rng.randrange(30)
        flag = rng.choice([0, 16, 99, 147, 83, 163, 65])
        rev = M.reverse_orientation(flag)
        edits = {mc.at(pos, rev): rng.choice("GGGA" if rev else "CCCT") if rng.random() < 0.9 else rng.choice("NACGT")}
        if mc.at(pos, rev) >= mc.READ:      # a reverse-orientation record that ends at the G: enclosing, no base there
            edits = {}
        name = "w%05d" % (k // 2 if k % 5 else 50000 + k)
        aux = b""
        if annotated and k % 11:
            seq = bytearray(mc.REF[pos:pos + mc.READ])
            for i, b in edits.items():
                seq[i] = ord(b)
            q = mc.at(pos, rev)
            hit = q < mc.READ and seq[q] == (ord("G") if rev else ord("C"))
            delta = (seq[q + 1:].count(b"G") if rev else seq[:q].count(b"C")) if hit else 0
            aux = mc.mm_aux("C+h,1;C+m,%d;" % delta, [rng.randrange(256), rng.randrange(256)])
        recs.append((pos, k, bc.make_read(mc.REF, pos, [("M", mc.READ)], edits, name=name, flag=flag, mapq=rng.choice([60, 60, 60, 30, 0]), q=rng.choice([2, 20, 30, 41]), aux=aux)))
    recs.sort(key=lambda x: x[:2])
    return [r for _, _, r in recs]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_record_counts_at_wave_and_workgroup_edges(n, tables, tmp_path):
    bam, _ = mc.write_bam(tmp_path, "n%d" % n, many(n))
    obs, lrec, res, _ = check(bam, mc.LOCI, "converted", tables)
    assert int(lrec["n_members"][0]) == n and (n < 60 or len(obs) > n // 4)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_deepest_locus_and_the_fallback(n, tables, tmp_path):
    """VLR_FRAGPILEUP_MAX_MEMBERS members at one locus are formed on the device; one more flags the locus TOO_MANY_MEMBERS, and the front
    end finishes it with the restatement: the tables equal those of the restatement either way"""
    bam, fa = mc.write_bam(tmp_path, "deep%d" % n, many(n, 1))
    deep = n > abi.FRAGPILEUP_MAX_MEMBERS
    if not deep:
        check(bam, mc.LOCI, "converted", tables)
    else:
        _, lrec, res = device(bam, mc.LOCI, "converted")
        assert res.status == 0 and res.n_loci_too_deep == 1 and res.n_obs == 0
        assert (int(lrec["n_members"][0]), int(lrec["status"][0]), int(lrec["n_obs"][0])) == (n, abi.FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS, 0)
    t, mt = tables
    dev, = M.tables(bam, mc.LOCI, mc.PROPS, "converted", 0)
    rs = M.restate(read_bam(bam)[1], mc.LOCI, mc.PROPS, "converted", t, mt)
    want = fragments.table_of(rs.per_locus[0], mc.PROPS, t)
    assert len(dev) == len(want) > 1000 and dev.records == want.records
    for col in ("prob_ref", "prob_alt", "prob_mapping", "prob_hit_base", "strand", "read_position_major"):
        assert (getattr(dev, col) == getattr(want, col)).all(), col


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "reverse"])
def test_a_20000_base_annotated_record_that_is_a_member_of_300_loci(rev, tables, tmp_path):
    ref, rec, loci, called = mc.long_record(rev)
    bam, _ = mc.write_bam(tmp_path, "long", [rec], {"m1": ref})
    props = fragments.Props(len(ref), 60, 20000)
    obs, lrec, res, rs = check(bam, loci, "annotated", tables, props)
    t, mt = tables
    assert len(loci) > 250 and len(obs) == len(loci) == res.n_members
    for loc, o in zip(loci, obs):
        ml = called[loc.start]
        want = (mt.ln_unmeth[ml], mt.ln_meth[ml]) if ml is not None else (0.0, -np.inf)
        assert (float(o["prob_ref"]), float(o["prob_alt"]), int(o["read_position"])) == want + (loc.start + (1 if rev else 0) - 100,)


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """both kinds of hand records in one annotated input (the converted ones carry no MM tag), plus 200 annotated records"""
    tmp = tmp_path_factory.mktemp("meth_mixed")
    recs = mc.annotated_cases().records + mc.converted_cases().records + many(200, 2, annotated=True)
    bam, fa = mc.write_bam(tmp, "mixed", recs)
    return {"tmp": tmp, "recs": recs, "bam": bam, "fa": fa}


def test_bytes_do_not_depend_on_feeds_files_or_runs(mixed, tables):
    base = check(mixed["bam"], mc.LOCI, "annotated", tables)
    recs = mixed["recs"]
    for wb in (4096, 65536, 1 << 22):
        got = device(mixed["bam"], mc.LOCI, "annotated", window_bytes=wb)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), wb
    again = device(mixed["bam"], mc.LOCI, "annotated")
    assert again[0].tobytes() == base[0].tobytes() and again[1].tobytes() == base[1].tobytes()
    pair = next(o for o in base[0] if o["right"] != abi.FRAGPILEUP_NO_RECORD)     # the file split between the mates of a pair
    cut = int(pair["left"]) + 1
    a, _ = mc.write_bam(mixed["tmp"], "part_a", recs[:cut])
    b, _ = mc.write_bam(mixed["tmp"], "part_b", recs[cut:])
    got = device([a, b], mc.LOCI, "annotated")
    assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes() and got[2].n_records == len(recs)


def test_overflow_of_each_capacity_is_reported_and_the_retry_succeeds(mixed, tmp_path):
    # (two records with XA tags in front, so that the session needs alt-locus keys)
    xa = [bc.make_read(mc.REF, 71, [("M", mc.READ)], name="xa%d" % k, aux=alignprops.aux_field("XA", "Z", "m2,+%d,30M,0;m3,-77,30M,1;" % (100 + k))) for k in range(2)]
    bam, _ = mc.write_bam(tmp_path, "caps", xa + mixed["recs"])
    base = device(bam, mc.LOCI, "annotated")
    need = {"member_capacity": int(base[2].needed_members), "name_capacity": int(base[2].needed_name_bytes), "key_capacity": int(base[2].needed_keys)}
    assert base[2].status == 0 and need["member_capacity"] == len(mixed["recs"]) + 2 and need["key_capacity"] == 4 and len(base[0]) > 50
    for cap, bit in (("member_capacity", abi.FRAGPILEUP_MEMBER_OVERFLOW), ("name_capacity", abi.FRAGPILEUP_NAME_OVERFLOW), ("key_capacity", abi.FRAGPILEUP_KEY_OVERFLOW)):
        obs, _, res = device(bam, mc.LOCI, "annotated", retry=False, **dict(need, **{cap: need[cap] - 1}))
        assert res.status == bit and not res.status & abi.FRAGPILEUP_GUARD_DAMAGED and len(obs) == 0, (cap, res.status)
        assert (int(res.needed_members), int(res.needed_name_bytes), int(res.needed_keys)) == tuple(need.values()), cap
    for got in (device(bam, mc.LOCI, "annotated", retry=False, **need), device(bam, mc.LOCI, "annotated", member_capacity=1, name_capacity=1, key_capacity=1)):
        assert got[2].status == 0 and got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes()


def test_a_file_cut_inside_a_record_is_malformed_input_not_a_fault(mixed, tables):
    recs = mixed["recs"]
    last = mc.annotated_cases().records[0]          # an annotated record: the cut lies inside its MM text
    head = alignprops.encode_bam([("m1", len(mc.REF))], recs)
    want = device(mixed["bam"], mc.LOCI, "annotated")
    for name, tail in (("ends_in_the_name", last[:36 + 2]), ("block_size_of_the_cut", struct.pack("<I", len(last) - 4 - 12) + last[4:len(last) - 12])):
        path = str(mixed["tmp"] / (name + ".bam"))
        with open(path, "wb") as f:
            f.write(alignprops.bgzf_compress(head + tail))
        obs, lrec, res = device(path, mc.LOCI, "annotated")
        assert res.status == abi.FRAGPILEUP_BAD_RECORD and res.first_bad_record == len(recs)
        assert obs.tobytes() == want[0].tobytes() and lrec.tobytes() == want[1].tobytes()
        with pytest.raises(fragments.FragPileupError, match="record %d is malformed" % len(recs)):
            fragments.observations(path, mixed["fa"], [("m1", mc.CPG, b"C", b"<METH>")], mc.PROPS, device=0, methylation_readtype="annotated")
    check(mixed["bam"], mc.LOCI, "annotated", tables)     # and the device is fine afterwards


def test_open_refuses_bad_arguments():
    import ctypes as C
    L = engine.lib()
    h = C.c_void_p()
    ref_id, start = np.zeros(2, np.int32), np.array([5, 3], np.int64)
    args = lambda rid, st, rt: (0, 2, rid.ctypes.data, st.ctypes.data, rt, 100, 60, 40, 16, 64, 16, 0, C.byref(h))
    assert L.vlr_fragpileup_open_methylation(*args(ref_id, start, abi.METH_CONVERTED)) == abi.ERR_INVALID_ARGUMENT      # not sorted
    assert b"not sorted" in L.vlr_last_error()
    assert L.vlr_fragpileup_open_methylation(*args(ref_id, np.array([3, 5], np.int64), 2)) == abi.ERR_INVALID_ARGUMENT      # no such read type
    assert b"readtype" in L.vlr_last_error()
    with pytest.raises(ValueError, match="read type"):
        device("x.bam", mc.LOCI, "bisulfite")


def command_files(tmp_path, d=None, cases=None):
    """(fasta with index, vcf, bam, properties path) of a held testcase, or of hand cases"""
    vcf = os.path.join(str(tmp_path), "c.vcf")
    if d is None:
        bam, fa = mc.write_bam(tmp_path, "cmd", cases.records)
        props = os.path.join(str(tmp_path), "p.json")
        json.dump({"insert_size": None, "max_del_cigar_len": None, "max_ins_cigar_len": None, "frac_max_softclip": None, "max_read_len": 190, "max_mapq": 60}, open(props, "w"))
        row = ("m1", mc.CPG + 1, "C", "<METH>")
    else:
        import glob
        bam, = glob.glob(os.path.join(d, "*.bam"))
        fa = os.path.join(str(tmp_path), "ref.fa")                       # (the fixtures hold their reference without an index)
        alignprops.write_fasta(fa, read_fasta(os.path.join(d, "ref.fa")))
        props = os.path.join(d, "properties.json")
        rec = open(os.path.join(d, "variant.tsv")).read().split("\n")[1].split("\t")
        row = (rec[0], int(rec[1]), rec[3], rec[4])
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##ALT=<ID=METH,Description=\"methylation\">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % row)
    return fa, vcf, bam, props


def test_meth_without_the_flag_is_refused_with_todays_text(tmp_path, capsys):
    fa, vcf, bam, props = command_files(tmp_path, cases=mc.converted_cases())
    out = os.path.join(str(tmp_path), "o.bcf")
    args = ["preprocess", "variants", fa, "--candidates", vcf, "--bam", bam, "--alignment-properties", props, "--atomic-candidate-variants", "--output", out]
    with pytest.raises(SystemExit):
        cli.main(args)
    assert "candidate m1:101 C><METH> is not an SNV or MNV: indel, structural and breakend candidates are not built" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(args + ["--indel-candidates"])
    assert "candidate m1:101 C><METH> is a symbolic or breakend allele: only SNVs, MNVs, deletions and insertions are built" in capsys.readouterr().err
    assert not os.path.exists(out)
    cli.main(args + ["--methylation-read-type", "converted"])
    assert os.path.exists(out)


@pytest.mark.parametrize("name", mc.FIXTURES)
def test_reference_testcases_on_the_device_and_end_to_end(oracle, golden_dir, tables, tmp_path, name):
    """the held testcase: the device's observations equal the restatement's field for field, and `preprocess variants
    --methylation-read-type …` -> `call variants generic` meets the testcase's `expected:` block"""
    from varlociraptor_amd import ingest
    sys.path.insert(0, os.path.join(os.path.dirname(golden_dir), "..", "tools"))
    import make_methylation_fixtures as tool
    from make_indel_fragment_fixtures import met
    d, bam, pj, rec, case, recorded = tool.load_case(name)
    names = [c for c, _ in alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)[0]]
    loci = [M.MethLocus(names.index(rec[0]), int(rec[1]) - 1)]
    obs, _, _, _ = check(bam, loci, case["methylation_readtype"], tables, fragments.props_of(pj))
    assert len(obs) == (mc.PACBIO_WITH_FLAG_RULE if case["methylation_readtype"] == "annotated" else mc.RECORDED_COUNTS[name])
    fa, vcf, bam, props = command_files(tmp_path, d)
    out = os.path.join(str(tmp_path), "o.bcf")
    cli.main(["preprocess", "variants", fa, "--candidates", vcf, "--bam", bam, "--alignment-properties", props, "--atomic-candidate-variants", "--output", out,
              "--methylation-read-type", case["methylation_readtype"]])
    batch, _ = ingest.read_observations([out])
    assert batch.n_obs == len(obs) and list(batch.locus["variant_type"]) == [abi.VT_OTHER]
    res = cli.call_variants(cli.scenario_from_yaml(os.path.join(d, "scenario.yaml")), {case["sample"]: out}, out=io.StringIO())
    vafs = {case["sample"]: float(res.map_vaf[0, 0])}
    print(name, vafs, case["expected"])
    assert (res.status[0] & 0xF) == 0 and not case["expected"]["posteriors"]
    assert met(case["expected"]["allelefreqs"], [], vafs, {}), vafs
