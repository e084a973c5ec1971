"""The kernel bodies of csrc/vlr_fragpileup.hip on the CPU, under the sanitizers (no GPU): csrc/vlr_fragpileup_host.cpp compiles the same
header (csrc/vlr_fragpileup.h) the kernels compile, with -fsanitize=address,undefined, into a stand-alone program under the build
directory; nothing is preloaded into any process.  Every record is handed to it in a heap block of exactly its size and the name pool
is a heap block of exactly the bytes counted, so a read or write behind either is a report.  The program runs over every hand case,
the synthetic inputs of tests/fragment_cases.py and the fixtures — its observations must equal the restatement's, f64 compared with ==
on the program's own tables — and over the hand records cut at every byte of their name and aux area and with their RO / XA values
overwritten: those must come back as bad records (or as records with other features) without a report."""
import os
import struct
import subprocess

import numpy as np
import pytest

import basecall_cases as bc
import fragment_cases as fc
import host_program
from varlociraptor_amd import abi, alignprops, basecalls, fragments
from varlociraptor_amd.readwindows import read_bam, read_fasta


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "vlr_fragpileup_host")


def run(program, tmp, loci, records, props, realign=False):
    """(observations, locus records, classes, Tables) of the host program over encoded records"""
    starts = np.concatenate(([0], np.cumsum([len(r) for r in records]))).astype(np.uint64)
    blob = b"VFPH" + struct.pack("<iqiiq", int(realign), props.window, props.max_mapq, props.max_read_len, len(loci))
    blob += np.array([l.ref_id for l in loci], np.int32).tobytes() + np.array([l.start for l in loci], np.int64).tobytes()
    blob += np.array([len(l.ref) for l in loci], np.int32).tobytes() + np.array([l.kind for l in loci], np.uint8).tobytes()
    blob += b"".join(l.ref for l in loci) + b"".join(l.alt for l in loci)
    blob += struct.pack("<q", len(records)) + starts.tobytes() + b"".join(records)
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    d = open(dst, "rb").read()
    tab = np.frombuffer(d, np.float64, 512)
    n, = struct.unpack_from("<q", d, 4096)
    obs = np.frombuffer(d, abi.FRAGPILEUP_OBS_DTYPE, n, 4104)
    lrec = np.frombuffer(d, abi.FRAGPILEUP_LOCUS_DTYPE, len(loci), 4104 + 56 * n)
    cls = np.frombuffer(d, np.uint8, len(records), 4104 + 56 * n + 24 * len(loci))
    return obs, lrec, cls, basecalls.Tables(list(tab[:256]), list(tab[256:]))


def same_as_restatement(program, tmp, contigs, loci, records, props, realign=False):
    obs, lrec, cls, tables = run(program, tmp, loci, records, props, realign)
    bam, _ = bc.write_case(tmp, "case", contigs, records)
    rs = fragments.restate(read_bam(bam)[1], loci, props, tables, realign)
    fc.assert_same(obs, lrec, rs)
    assert int((cls == 1).sum()) == rs.n_rejected and not (cls == 2).any()
    return obs, lrec


def test_hand_cases_equal_the_restatement(program, tmp_path):
    for case in fc.hand_cases():
        loci, _ = fc.loci_of(case)
        same_as_restatement(program, tmp_path, {"c1": fc.REF, "c2": fc.REF[:50]}, loci, case.records, case.props)


def test_synthetic_and_deep_loci_equal_the_restatement(program, tmp_path):
    contigs, cands, recs, props = fc.synthetic()
    obs, lrec = same_as_restatement(program, tmp_path, contigs, bc.loci_of(cands, contigs), recs, props)
    assert len(obs) > 1000 and set(obs["strand"]) == {0, 1, 2} and (obs["right"] == abi.FRAGPILEUP_NO_RECORD).any() and (obs["bits"] & abi.FRAGPILEUP_HAS_XA).any()
    assert (lrec["major_read_position"] != abi.BASEPILEUP_NO_READ_POSITION).any()
    same_as_restatement(program, tmp_path, contigs, bc.loci_of(cands, contigs), recs, props, realign=True)
    contigs, cands, recs, props = fc.deep_loci([1, 2, 3, 63, 64, 65, 255, 256, 257])
    obs, lrec = same_as_restatement(program, tmp_path, contigs, bc.loci_of(cands, contigs), recs, props)
    assert list(lrec["n_members"]) == [1, 2, 3, 63, 64, 65, 255, 256, 257]
    # alt loci at the limit of the key sort (256 x 16 = VLR_FRAGPILEUP_MAX_MEMBERS keys) and above it (flagged)
    for case, flagged in ((fc.xa_heavy(256, 16), False), (fc.xa_heavy(300, 14), True)):
        loci, _ = fc.loci_of(case)
        obs, lrec = same_as_restatement(program, tmp_path, {"c1": fc.REF, "c2": fc.REF[:50]}, loci, case.records, case.props)
        assert bool(lrec[0]["status"] & abi.FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI) == flagged
        assert flagged or (len(obs) == 256 and list(obs["alt_locus"]) == [abi.ALTLOCUS_SOME] + [abi.ALTLOCUS_MAJOR] * 255)


@pytest.mark.parametrize("name", sorted(fc.FIXTURES))
def test_fixture_equals_the_restatement(program, tmp_path, golden_dir, name):
    bam, fasta, _, cand, props = fc.fixture_case(golden_dir, name)
    d = alignprops.inflate_bgzf(bam)
    contigs, o = alignprops.bam_header(d, bam)
    records = []
    while o < len(d):
        bs, = struct.unpack_from("<I", d, o)
        records.append(bytes(d[o:o + 4 + bs]))
        o += 4 + bs
    seqs = read_fasta(fasta)
    names = [c for c, _ in contigs]
    loci = [basecalls.locus(seqs[c], names.index(c), p, r, a) for c, p, r, a in cand]
    obs, lrec, cls, tables = run(program, tmp_path, loci, records, props)
    rs = fragments.restate(read_bam(bam)[1], loci, props, tables)
    fc.assert_same(obs, lrec, rs)
    assert len(obs) > 0 and not (cls == 2).any()


def test_truncated_and_overwritten_records_are_bad_records_not_faults(program, tmp_path):
    case = {c.name: c for c in fc.hand_cases()}
    hand = [r for c in case.values() for r in c.records]
    loci, _ = fc.loci_of(case["xa_entries"])
    cut, patched = [], []
    for r in hand:
        l_rn, n_cig, l_seq = r[12], struct.unpack_from("<H", r, 16)[0], struct.unpack_from("<i", r, 20)[0]
        aux0 = 36 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        for k in list(range(36, 36 + l_rn)) + list(range(aux0 + 1, len(r))):      # every byte of the name and of the aux area
            cut.append(r[:k])
            patched.append(struct.pack("<I", k - 4) + r[4:k])
    obs, lrec, cls, _ = run(program, tmp_path, loci, cut + patched, fc.P30)
    # a record cut inside its name or inside an aux field is refused; one cut between two aux fields is a record with fewer fields
    assert (cls[:len(cut)] == 2).all() and len(cls) > 1000
    assert set(cls[len(cut):]) <= {0, 2} and (cls[len(cut):] == 2).sum() > len(patched) * 3 // 4
    # RO and XA values overwritten: no NUL (the string runs to the record's end), only commas, only semicolons, bytes above 127
    def rec(k):
        return fc.rd("v%02d" % k, 12, flag=0x61, mtid=0, mpos=30, aux=fc.A("RO", "Z", "F1R2") + fc.A("XA", "Z", "chr2,+130,12M,0;"))
    base = rec(0)
    n = len(base)
    ro, xa = n - 25, n - 17      # the first byte of the RO value and of the XA value

    def put(k, off, data):
        b = bytearray(rec(k))
        b[off:off + len(data)] = data
        assert len(b) == n
        return bytes(b)
    weird = [put(1, ro, b",,,,"), put(2, ro, b"\xff\xfe\x80\x81"), put(3, xa, b";" * 16), put(4, xa, b"," * 16), put(5, xa, b"\xff" * 16),
             put(6, xa, b"c,+99999999999,M")]
    no_nul = [put(7, n - 1, b";"), put(8, ro + 4, b"x")]     # XA runs to the record's end: refused; RO runs into the XA field: one long value
    obs, lrec, cls, _ = run(program, tmp_path, loci, weird + no_nul + [base], fc.P30)
    assert list(cls) == [0] * len(weird) + [2, 0, 0]
    # (v00 .. v08 in name order: v07 is the refused one) the classes follow the entries that still parse: chr2,+130 twice = the major locus
    assert [int(c) for c in obs["alt_locus"]] == [abi.ALTLOCUS_MAJOR] * 3 + [abi.ALTLOCUS_NONE] * 4 + [abi.ALTLOCUS_NONE]
    assert len(obs) == len(weird) + 2 and obs[0]["orientation"] == abi.FRAG_F1R2
