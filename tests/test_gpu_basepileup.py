"""SNV / MNV allele supports from BAM records on the GPU (vlr_basepileup_*, csrc/vlr_basepileup.hip): the kernel's hits must equal the
restatement's (varlociraptor_amd/basecalls.py run on the library's own tables, vlr_basepileup_tables) field for field, f64 compared
with ==, on the records of the reference's SNV unit test, the hand cases and the seeded synthetic BAM of tests/basecall_cases.py and
on every reference testcase under tests/golden/bam/; the hit array must not depend on how the file is cut into feeds; an overflow of
the hit buffer and a file cut inside a record are reported, not faults; and allele_supports -> pileup -> engine meets each testcase's
own `expected:` block."""
import struct

import numpy as np
import pytest

import bam_pairs as bp
import basecall_cases as bc
from varlociraptor_amd import abi, alignprops, basecalls, cli, engine
from varlociraptor_amd.readwindows import read_fasta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables():
    return basecalls.library_tables()


def expected(bam, loci, tables, realign=False):
    sc = bc.restatement(bam, loci, tables, realign)
    return sorted(sc.hits + sc.needs_realign, key=lambda h: (h.locus, h.record)), sc


def check(bam, loci, tables, realign=False, **kw):
    arr, res = basecalls.device_hits(bam, loci, 0, realign, **kw)
    want, sc = expected(bam, loci, tables, realign)
    assert bc.hit_keys(basecalls.hits_from_array(arr)) == bc.hit_keys(want)
    assert (res.n_hits, res.n_records, res.n_rejected, res.n_needs_realign, res.status) == (len(want), sc.n_records, sc.n_rejected, len(sc.needs_realign), 0)
    assert res.needed_capacity == len(want) and res.first_bad_record == -1
    return arr, res


def test_library_tables_equal_the_python_tables_within_2_ulp(tables):
    """one exp and one log1p (or expm1 and log) on correctly rounded or 1-ulp libm inputs"""
    worst = 0.0
    for mine, ref in ((tables.call, basecalls.TABLES.call), (tables.miscall, basecalls.TABLES.miscall)):
        a, b = np.array(mine), np.array(ref)
        assert np.array_equal(np.isneginf(a), np.isneginf(b))
        fin = np.isfinite(b) & (b != 0.0)
        worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / np.spacing(np.abs(b[fin])))))
    print("largest table difference: %.1f ulp" % worst)
    assert worst <= 2.0
    assert tables.miscall[0] == 0.0 and tables.call[0] == -np.inf


def test_snv_rs_and_hand_records(tables, tmp_path):
    bam, _ = bc.write_case(tmp_path, "snvrs", {"ref": bc.SNV_RS_REF}, bc.snv_rs_records())
    arr, _ = check(bam, bc.loci_of([bc.SNV_RS_CANDIDATE], {"ref": bc.SNV_RS_REF}), tables)
    assert list(arr["record"]) == [0, 1, 2] and list(arr["read_position"]) == [10, 7, 3]
    loci = bc.loci_of(bc.HAND_CANDIDATES, {"c1": bc.HAND_REF})
    recs = bc.hand_records()
    bam, _ = bc.write_case(tmp_path, "hand", {"c1": bc.HAND_REF}, recs.values())
    arr, res = check(bam, loci, tables)
    assert res.n_rejected == 4
    # with realign_indel_reads the records with an I or D come back flagged, the others are unchanged
    arr2, res2 = check(bam, loci, tables, realign=True)
    labels = list(recs)
    flagged = arr2[(arr2["status"] & abi.BASEPILEUP_HIT_NEEDS_REALIGN) != 0]
    assert {labels[int(r)] for r in flagged["record"]} == {"snv_behind_insertion", "mnv_across_D"} and res2.n_needs_realign == 2
    keep = ~np.isin(arr["record"], flagged["record"])
    assert arr[keep].tobytes() == arr2[(arr2["status"] & abi.BASEPILEUP_HIT_NEEDS_REALIGN) == 0].tobytes()


def test_error_statuses_surface_as_the_references_errors(tmp_path):
    loci = bc.loci_of(bc.HAND_CANDIDATES, {"c1": bc.HAND_REF})
    recs = list(bc.hand_error_records().values()) + [bc.make_read(bc.HAND_REF, 15, [("N", 2), ("M", 10)])]
    bam, _ = bc.write_case(tmp_path, "err", {"c1": bc.HAND_REF}, recs)
    arr, res = basecalls.device_hits(bam, loci)
    assert list(arr["status"]) == [abi.BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS, abi.BASEPILEUP_HIT_INVALID_STRAND_INFO, abi.BASEPILEUP_HIT_LEADING_REFSKIP]
    with pytest.raises(basecalls.ReadPosOutOfBounds):
        basecalls.hits_from_array(arr[:1])
    with pytest.raises(basecalls.InvalidStrandInfo):
        basecalls.hits_from_array(arr[1:2])
    with pytest.raises(basecalls.ReadPosOutOfBounds):
        basecalls.allele_supports(bam, str(tmp_path / "err.fa"), bc.HAND_CANDIDATES[:1], device=0)


@pytest.fixture(scope="module")
def synth(tmp_path_factory, tables):
    tmp = tmp_path_factory.mktemp("synth")
    contigs, cands, recs = bc.synthetic()
    loci = bc.loci_of(cands, contigs)
    bam, _ = bc.write_case(tmp, "synth", contigs, recs)
    small, _ = bc.write_case(tmp, "synth_small_members", contigs, recs, member_bytes=300)   # records straddle BGZF members
    want, sc = expected(bam, loci, tables)
    return dict(tmp=tmp, contigs=contigs, loci=loci, recs=recs, bam=bam, small=small, want=want, sc=sc)


def test_synthetic_bam_equals_the_restatement(synth, tables):
    arr, res = check(synth["bam"], synth["loci"], tables)
    assert res.n_hits > 1000 and (arr["third_allele"] > 1).any() and set(arr["strand"]) == {0, 1, 2, 3}
    assert list(arr["locus"]) == sorted(arr["locus"])
    with_reads = set(arr["locus"])
    assert any(l.ref_id == 1 for l in synth["loci"]) and not any(synth["loci"][k].ref_id == 1 for k in with_reads) and len(with_reads) < len(synth["loci"])
    check(synth["bam"], synth["loci"], tables, realign=True)


@pytest.mark.parametrize("n_records", [1023, 1024, 1025, 2049])
def test_one_chunk_around_the_scan_width_equals_the_restatement(tables, tmp_path, n_records):
    """The prefix sum over a chunk's per-record counts (vlr_bam::scan_kernel of csrc/vlr_bamsession.h, 1024 threads, u32 counts) where a
    thread's slice holds one record with trailing threads empty (1023), exactly one (1024), two with the threads of the upper half
    empty (1025: slices of 2, 513 of them used) and three (2049): one chunk of n_records records (the default window_bytes holds the
    whole file), every hit's place checked against the restatement.  The module's 300-record input never gives a thread two records.
    The same kernel scans the fragment session's three count arrays; tests/test_gpu_fragpileup.py's module input has more than 3000
    records in one chunk and 120 loci, so slices of three and four records and the per-locus scans are covered there."""
    contigs, cands, recs = bc.synthetic(n_records=n_records, n_loci=200)
    loci = bc.loci_of(cands, contigs)
    bam, _ = bc.write_case(tmp_path, "scan%d" % n_records, contigs, recs)
    arr, res = check(bam, loci, tables)
    assert res.n_records == n_records and res.n_hits > 1000 and res.n_rejected > 50


def test_hits_do_not_depend_on_the_feeds_or_the_run(synth):
    base, _ = basecalls.device_hits(synth["bam"], synth["loci"])
    again, _ = basecalls.device_hits(synth["bam"], synth["loci"])
    assert base.tobytes() == again.tobytes()
    # window_bytes = 1, the smallest legal value: every feed is one 300-byte BGZF member, records straddle feeds, chunks hold a few records
    tiny, res = basecalls.device_hits(synth["small"], synth["loci"], window_bytes=1)
    assert tiny.tobytes() == base.tobytes() and res.status == 0
    mid, _ = basecalls.device_hits(synth["small"], synth["loci"], window_bytes=4096)
    assert mid.tobytes() == base.tobytes()


def test_hit_capacity_overflow_is_reported_and_the_retry_succeeds(synth):
    need = len(synth["want"])
    arr, res = basecalls.device_hits(synth["bam"], synth["loci"], hit_capacity=need - 1, retry=False)
    assert res.status == abi.BASEPILEUP_OVERFLOW and res.needed_capacity == need and res.n_hits == 0 and len(arr) == 0   # (guard words intact: no GUARD_DAMAGED)
    arr, res = basecalls.device_hits(synth["small"], synth["loci"], hit_capacity=7, retry=False, window_bytes=1)      # overflow in the first of many chunks
    assert res.status == abi.BASEPILEUP_OVERFLOW and res.needed_capacity == need
    arr, res = basecalls.device_hits(synth["bam"], synth["loci"], hit_capacity=0, retry=False)
    assert res.status == abi.BASEPILEUP_OVERFLOW and res.needed_capacity == need
    arr, res = basecalls.device_hits(synth["bam"], synth["loci"], hit_capacity=need - 1)    # the retry with the needed capacity
    assert res.status == 0 and bc.hit_keys(basecalls.hits_from_array(arr)) == bc.hit_keys(synth["want"])
    arr, res = basecalls.device_hits(synth["bam"], synth["loci"], hit_capacity=need, retry=False)
    assert res.status == 0 and res.n_hits == need


def test_a_file_cut_inside_a_cigar_is_malformed_input_not_a_fault(synth, tables):
    contigs, recs, loci = synth["contigs"], synth["recs"], synth["loci"]
    last = recs[-1]
    cut = 36 + last[12] + 5            # inside the second CIGAR word
    assert struct.unpack_from("<H", last, 16)[0] >= 2
    head = alignprops.encode_bam([(c, len(s)) for c, s in contigs.items()], recs[:-1])
    front, _ = bc.write_case(synth["tmp"], "front", contigs, recs[:-1])
    want, _ = expected(front, loci, tables)
    for name, tail in (("ends_inside", last[:cut]), ("block_size_of_the_cut", struct.pack("<I", cut - 4) + last[4:cut])):
        path = str(synth["tmp"] / (name + ".bam"))
        with open(path, "wb") as f:
            f.write(alignprops.bgzf_compress(head + tail))
        arr, res = basecalls.device_hits(path, loci)
        assert res.status == abi.BASEPILEUP_BAD_RECORD and res.first_bad_record == len(recs) - 1
        assert bc.hit_keys(basecalls.hits_from_array(arr)) == bc.hit_keys(want)
        with pytest.raises(basecalls.BasePileupError):
            basecalls.allele_supports(path, str(synth["tmp"] / "synth.fa"), [("s1", l.start, l.ref, l.alt) for l in loci[:3] if l.ref_id == 0], device=0)
    # and the device is fine afterwards
    check(synth["bam"], loci, tables)


def test_open_refuses_bad_loci():
    L = [basecalls.Locus(abi.BASEPILEUP_SNV, 0, 10, b"A", b"C"), basecalls.Locus(abi.BASEPILEUP_SNV, 0, 5, b"A", b"C")]
    with pytest.raises(engine.EngineError):
        basecalls.device_hits("/nonexistent.bam", L)                                     # not sorted
    with pytest.raises(engine.EngineError):
        basecalls.device_hits("/nonexistent.bam", [basecalls.Locus(abi.BASEPILEUP_MNV, 0, 5, b"A" * 33, b"C" * 33)])   # longer than VLR_BASEPILEUP_MAX_LEN


@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_fixture_hits_and_call(oracle, golden_dir, tables, name):
    bam, fasta, scenario, cand = bc.fixture_case(golden_dir, name)
    contigs, _ = alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)
    names = [c for c, _ in contigs]
    seqs = read_fasta(fasta)
    loci = [basecalls.locus(seqs[c], names.index(c), p, r, a) for c, p, r, a in cand]
    arr, res = check(bam, loci, tables)
    assert res.n_hits > 0
    # end to end: the kernel's supports, mates merged, as a pileup through the engine
    sup = basecalls.allele_supports(bam, fasta, cand, device=0)
    cpu = basecalls.allele_supports(bam, fasta, cand, device="cpu")
    assert sup[0].records == cpu[0].records and np.allclose(sup[0].prob_alt, cpu[0].prob_alt, rtol=1e-14, atol=0, equal_nan=True)
    batch = basecalls.pileup(sup, cand)
    sc = cli.scenario_from_yaml(scenario, contig=cand[0][0])
    plan = engine.Plan(sc)
    got = plan.call_host(batch)
    plan.close()
    ref = oracle.call(sc, batch)
    assert np.allclose(np.exp(got.ln_posterior), np.exp(ref.ln_posterior), atol=1e-6, rtol=0) and abs(got.map_vaf[0, 0] - ref.map_vaf[0, 0]) <= 1e-6
    assert bc.FIXTURES[name](float(got.map_vaf[0, 0]), bp.phred_by_event(sc, got.ln_posterior[0])), float(got.map_vaf[0, 0])
