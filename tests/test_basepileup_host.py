"""The kernel body of csrc/vlr_basepileup.hip on the CPU, under the sanitizers (no GPU): csrc/vlr_basepileup_host.cpp compiles the
same header (csrc/vlr_basepileup.h) the kernel compiles, with -fsanitize=address,undefined, into a small program under the build
directory.  Every record is handed to the scoring in a heap block of exactly its size, so a read behind a record's end is a report.
The program runs over every fixture and every synthetic input of tests/basecall_cases.py — its hits must equal the restatement's,
f64 compared with == on the program's own tables — and over truncated and corrupted copies of the hand records: each one cut at every
byte offset of its fixed head, read name and CIGAR (once as the bytes are, once with block_size set to the cut), and with its length
fields and aux fields overwritten.  Those must come back as bad records without a sanitizer report."""
import os
import struct
import subprocess

import numpy as np
import pytest

import basecall_cases as bc
import host_program
from varlociraptor_amd import abi, alignprops, basecalls
from varlociraptor_amd.readwindows import read_bam


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "vlr_basepileup_host")


def run(program, tmp, loci, records, realign=False):
    """(hits as a structured array, classes, Tables) of the host program over encoded records"""
    starts = np.concatenate(([0], np.cumsum([len(r) for r in records]))).astype(np.uint64)
    blob = b"VBPH" + struct.pack("<iq", int(realign), len(loci))
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
    hits = np.frombuffer(d, abi.BASEPILEUP_HIT_DTYPE, n, 4104)
    cls = np.frombuffer(d, np.uint8, len(records), 4104 + 48 * n)
    return hits, cls, basecalls.Tables(list(tab[:256]), list(tab[256:]))


def same_as_restatement(program, tmp, contigs, candidates, records, realign=False):
    loci = bc.loci_of(candidates, contigs)
    hits, cls, tables = run(program, tmp, loci, records, realign)
    bam, _ = bc.write_case(tmp, "case", contigs, records)
    sc = bc.restatement(bam, loci, tables, realign)
    got = basecalls.hits_from_array(hits)
    want = sorted(sc.hits + sc.needs_realign, key=lambda h: (h.locus, h.record))
    assert bc.hit_keys(got) == bc.hit_keys(want)
    assert int((cls == 1).sum()) == sc.n_rejected and not (cls == 2).any()
    return got


def test_program_tables_are_the_python_tables(program, tmp_path):
    _, _, t = run(program, tmp_path, [], [])
    for mine, ref in ((t.call, basecalls.TABLES.call), (t.miscall, basecalls.TABLES.miscall)):
        a, b = np.array(mine), np.array(ref)
        assert np.array_equal(np.isneginf(a), np.isneginf(b))
        fin = np.isfinite(b)
        assert np.all(np.abs(a[fin] - b[fin]) <= 2 * np.spacing(np.abs(b[fin])))


def test_snv_rs_hand_and_synthetic_records_equal_the_restatement(program, tmp_path):
    assert len(same_as_restatement(program, tmp_path, {"ref": bc.SNV_RS_REF}, [bc.SNV_RS_CANDIDATE], bc.snv_rs_records())) == 3
    hand = list(bc.hand_records().values())
    n = len(same_as_restatement(program, tmp_path, {"c1": bc.HAND_REF}, bc.HAND_CANDIDATES, hand))
    m = same_as_restatement(program, tmp_path, {"c1": bc.HAND_REF}, bc.HAND_CANDIDATES, hand, realign=True)
    # (the read with a deletion inside the MNV gives no observation when it is scored, and a NEEDS_REALIGN entry when it is not)
    assert len(m) == n + 1 and sum(1 for h in m if h.status & basecalls.NEEDS_REALIGN) == 2
    contigs, cands, recs = bc.synthetic()
    got = same_as_restatement(program, tmp_path, contigs, cands, recs)
    assert len(got) > 1000 and any(h.third_allele > 1 for h in got) and {h.strand for h in got} == {0, 1, 2, 3}
    same_as_restatement(program, tmp_path, contigs, cands, recs, realign=True)


def test_error_statuses(program, tmp_path):
    loci = bc.loci_of(bc.HAND_CANDIDATES, {"c1": bc.HAND_REF})
    bad = bc.hand_error_records()
    hits, cls, _ = run(program, tmp_path, loci, list(bad.values()) + [bc.make_read(bc.HAND_REF, 15, [("N", 2), ("M", 10)])])
    assert [int(h["status"]) for h in hits] == [abi.BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS, abi.BASEPILEUP_HIT_INVALID_STRAND_INFO, abi.BASEPILEUP_HIT_LEADING_REFSKIP]
    with pytest.raises(basecalls.ReadPosOutOfBounds):
        basecalls.hits_from_array(hits[:1])


@pytest.mark.parametrize("name", sorted(bc.FIXTURES))
def test_fixture_equals_the_restatement(program, tmp_path, golden_dir, name):
    bam, fasta, _, cand = bc.fixture_case(golden_dir, name)
    d = alignprops.inflate_bgzf(bam)
    contigs, o = alignprops.bam_header(d, bam)
    records = []
    while o < len(d):
        bs, = struct.unpack_from("<I", d, o)
        records.append(bytes(d[o:o + 4 + bs]))
        o += 4 + bs
    from varlociraptor_amd.readwindows import read_fasta
    seqs = read_fasta(fasta)
    names = [c for c, _ in contigs]
    loci = [basecalls.locus(seqs[c], names.index(c), p, r, a) for c, p, r, a in cand]
    hits, cls, tables = run(program, tmp_path, loci, records)
    sc = bc.restatement(bam, loci, tables)
    assert bc.hit_keys(basecalls.hits_from_array(hits)) == bc.hit_keys(sc.hits) and len(sc.hits) > 0
    assert not (cls == 2).any() and int((cls == 1).sum()) == sc.n_rejected


def test_truncated_and_corrupted_records_are_bad_records_not_faults(program, tmp_path):
    loci = bc.loci_of(bc.HAND_CANDIDATES, {"c1": bc.HAND_REF})
    hand = list(bc.hand_records().values())
    cut, patched = [], []
    for r in hand:
        l_rn, n_cig = r[12], struct.unpack_from("<H", r, 16)[0]
        for k in range(0, 36 + l_rn + 4 * n_cig):          # every byte offset of the head, the read name and the CIGAR
            cut.append(r[:k])
            if k >= 4:
                patched.append(struct.pack("<I", k - 4) + r[4:k])
    hits, cls, _ = run(program, tmp_path, loci, cut + patched)
    assert len(hits) == 0 and (cls == 2).all() and len(cls) > 3000
    # length fields that overrun block_size, CIGAR codes, aux fields
    base = bc.make_read(bc.HAND_REF, 15, [("M", 12)], {5: "T"}, aux=alignprops.aux_field("SI", "Z", "++++++++++++") + alignprops.aux_field("XB", "B", ("i", [1, 2])))
    n = len(base)
    l_rn = base[12]

    def put(off, fmt, v, r=base):
        b = bytearray(r)
        struct.pack_into(fmt, b, off, v)
        return bytes(b)
    bad = [put(12, "<B", 255), put(12, "<B", 0), put(16, "<H", 65535), put(16, "<H", 9), put(20, "<i", 0x7fffffff), put(20, "<i", -1), put(20, "<i", 13),
           put(0, "<I", 0xffffffff), put(0, "<I", n), put(0, "<I", n - 5),
           put(36 + l_rn, "<I", (12 << 4) | 9), put(36 + l_rn, "<I", (12 << 4) | 15), put(36 + l_rn, "<I", (13 << 4) | 0), put(36 + l_rn, "<I", (0xfffffff << 4) | 4),
           base[:n - 9] + b"\x01" * 9,                                       # the B array's count and values overwritten
           put(n - 12, "<I", 0x7fffffff), put(n - 13, "<B", ord("q")),       # B count far past the end; unknown subtype
           put(n - 17, "<B", ord("+")),                                      # the NUL of SI overwritten: the string runs into the next field
           base + b"XYZ", base + b"XYi\x01", base + b"X"]
    bad = [struct.pack("<I", len(b) - 4) + b[4:] if len(b) != n else b for b in bad]   # appended bytes belong to the record
    hits, cls, _ = run(program, tmp_path, loci, bad + [base])
    assert list(cls[:-1]) == [2] * len(bad), list(cls)
    assert cls[-1] == 0 and len(hits) == 1 and hits[0]["record"] == len(bad) and hits[0]["locus"] == 0
