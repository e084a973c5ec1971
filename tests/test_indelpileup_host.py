"""The evidence text of csrc/vlr_indelpileup.hip on the CPU, under the sanitizers (no GPU): csrc/vlr_indelpileup_host.cpp compiles the
same header (csrc/vlr_indelpileup.h) the kernels compile, with -fsanitize=address,undefined, into a small program under the build
directory.  Every record is handed to it in a heap block of exactly its size and every contig in one of exactly its length, so a
read behind either end is a report.  The program runs over the hand records, the synthetic set (tests/indel_cases.py) and every
fixture of bam_pairs.BAM_CASES — its descriptors and window bytes must equal the restatement's (readwindows.evidence) — and over
truncated and corrupted copies of the hand records: each one cut at every byte offset of its fixed head, read name and CIGAR (once as
the bytes are, once with block_size set to the cut), with its length fields overwritten, and with CIGARs that consume more than
l_seq.  Those must come back as bad records without a sanitizer report."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_pairs as bp
import host_program
import indel_cases as ic
from varlociraptor_amd import abi


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "vlr_indelpileup_host")


def run(program, tmp, contigs, names, loci, rid, records, window=ic.WINDOW):
    """(hits, (x_offset, x_bases, y_offset, y_bases, y_quals), classes) of the host program over encoded records; `contigs` {name: bytes},
    `names` the contigs of the BAM header (one the reference lacks goes in with length -1)"""
    ref_id, start, end, alt_off, altb = ic.as_arrays(loci, rid)
    starts = np.concatenate(([0], np.cumsum([len(r) for r in records]))).astype(np.uint64)
    blob = b"VIPH" + struct.pack("<iq", window, len(loci)) + ref_id.tobytes() + start.tobytes() + end.tobytes() + alt_off.tobytes() + altb
    blob += struct.pack("<q", len(names)) + np.array([len(contigs[n]) if n in contigs else -1 for n in names], np.int64).tobytes()
    blob += b"".join(contigs[n] for n in names if n in contigs)
    blob += struct.pack("<q", len(records)) + starts.tobytes() + b"".join(records)
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([program, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    d = open(dst, "rb").read()
    n, = struct.unpack_from("<q", d, 0)
    o = 8
    hits = np.frombuffer(d, abi.INDELPILEUP_HIT_DTYPE, n, o)
    o += 64 * n
    xo = np.frombuffer(d, np.uint32, 2 * n + 1, o)
    o += 4 * (2 * n + 1)
    yo = np.frombuffer(d, np.uint32, 2 * n + 1, o)
    o += 4 * (2 * n + 1)
    nx, ny = int(xo[-1]), int(yo[-1])
    xb, yb, qb = d[o:o + nx], d[o + nx:o + nx + ny], d[o + nx + ny:o + nx + 2 * ny]
    o += nx + 2 * ny
    cls = np.frombuffer(d, np.uint8, len(records), o)
    assert o + len(records) == len(d)
    return hits, (xo, xb, yo, yb, qb), cls


def same_as_restatement(program, tmp, contigs, names, candidates, records, window=ic.WINDOW):
    loci, rid, _ = ic.loci_of(candidates, contigs, window, names=names)
    hits, (xo, xb, yo, yb, qb), cls = run(program, tmp, contigs, names, loci, rid, records, window)
    bam = os.path.join(str(tmp), "case.bam")
    from varlociraptor_amd import alignprops
    alignprops.write_bam(bam, [(n, len(contigs.get(n, b""))) for n in names], list(records))
    exp = ic.expected(bam, contigs, loci, rid, window, names=names)
    assert ic.hit_keys(hits) == ic.evidence_keys(exp)
    want = ic.pair_batch(exp, loci).arrays()
    assert np.array_equal(xo, want[0]) and np.array_equal(yo, want[2])
    assert (xb or b"\0") == want[1].tobytes() and (yb or b"\0") == want[3].tobytes() and (qb or b"\0") == want[4].tobytes()
    assert (hits["dist_ref"] == -1).all() and (hits["ln_ref"] == 0).all() and not hits["pad"].any()
    assert not (cls == 2).any()
    return hits, exp, cls


def test_hand_records_equal_the_restatement(program, tmp_path):
    recs = ic.hand_records()
    hits, exp, cls = same_as_restatement(program, tmp_path, ic.HAND_CONTIGS, list(ic.HAND_CONTIGS), ic.HAND_CANDIDATES.values(), list(recs.values()))
    assert int((cls == 1).sum()) == 4 and len(hits) == len(exp) > 30
    assert set(hits["status"]) == {0, abi.INDELPILEUP_HIT_NO_OVERLAP, abi.INDELPILEUP_HIT_LEADING_REFSKIP}
    assert {1, 63, 64, 65, 127, 128} <= set(int(x) for x in hits["read_len"])
    # other realignment windows: every clamp moves
    for window in (1, 7, 33):
        same_as_restatement(program, tmp_path, ic.HAND_CONTIGS, list(ic.HAND_CONTIGS), ic.HAND_CANDIDATES.values(), list(recs.values()), window)


def test_synthetic_set_equals_the_restatement(program, tmp_path):
    contigs, cands, recs = ic.synthetic()
    hits, exp, _ = same_as_restatement(program, tmp_path, contigs, list(contigs), cands, recs)
    assert len(hits) > 200 and len(set(hits["locus"])) > 20
    # loci the other way round in the file (the same contigs under other reference ids)
    flipped = {"s2": contigs["s2"], "s1": contigs["s1"]}
    recs2 = [r[:4] + struct.pack("<i", 1 - struct.unpack_from("<i", r, 4)[0]) + r[8:] for r in recs]
    same_as_restatement(program, tmp_path, flipped, list(flipped), cands, recs2)


@pytest.mark.parametrize("name", sorted(bp.BAM_CASES))
def test_fixture_equals_the_restatement(program, tmp_path, golden_dir, name):
    bam, _, contigs, names, cand = ic.fixture_case(golden_dir, name)
    _, records = ic.split_records(bam)
    hits, exp, _ = same_as_restatement(program, tmp_path, contigs, names, cand, records)
    assert len(hits) > 20


def test_truncated_and_corrupted_records_are_bad_records_not_faults(program, tmp_path):
    loci, rid, _ = ic.loci_of(ic.HAND_CANDIDATES.values(), ic.HAND_CONTIGS)
    names = list(ic.HAND_CONTIGS)
    hand = list(ic.hand_records().values())
    cut, patched = [], []
    for r in hand:
        l_rn, n_cig = r[12], struct.unpack_from("<H", r, 16)[0]
        for k in range(0, 36 + l_rn + 4 * n_cig):          # every byte offset of the head, the read name and the CIGAR
            cut.append(r[:k])
            if k >= 4:
                patched.append(struct.pack("<I", k - 4) + r[4:k])
    hits, _, cls = run(program, tmp_path, ic.HAND_CONTIGS, names, loci, rid, cut + patched)
    assert len(hits) == 0 and (cls == 2).all() and len(cls) > 3000
    # length fields that overrun block_size, CIGAR codes, CIGARs that consume more than l_seq
    base = ic.make_read(ic.C1, 100, [("M", 21), ("D", 3), ("M", 40)], name="base")
    n = len(base)
    l_rn = base[12]
    c0 = 36 + l_rn

    def put(off, fmt, v, r=base):
        b = bytearray(r)
        struct.pack_into(fmt, b, off, v)
        return bytes(b)
    bad = [put(12, "<B", 255), put(12, "<B", 0), put(16, "<H", 65535), put(16, "<H", 9), put(20, "<i", 0x7fffffff), put(20, "<i", -1), put(20, "<i", 62),
           put(0, "<I", 0xffffffff), put(0, "<I", n), put(0, "<I", n - 5),
           put(c0, "<I", (21 << 4) | 9), put(c0, "<I", (21 << 4) | 15),
           put(c0, "<I", (22 << 4) | 0), put(c0 + 8, "<I", (41 << 4) | 0),                  # one base more than l_seq, in either M
           put(c0 + 4, "<I", (3 << 4) | 1), put(c0 + 4, "<I", (0xfffffff << 4) | 4),         # the D turned into an I / an enormous soft clip
           put(c0, "<I", (0xfffffff << 4) | 0),
           base + b"XYZ", base + b"X"]
    bad = [struct.pack("<I", len(b) - 4) + b[4:] if len(b) != n else b for b in bad]   # appended bytes belong to the record
    hits, _, cls = run(program, tmp_path, ic.HAND_CONTIGS, names, loci, rid, bad + [base])
    assert list(cls[:-1]) == [2] * len(bad), list(cls)
    assert cls[-1] == 0 and len(hits) == 1 and hits[0]["record"] == len(bad) and (hits[0]["read_begin"], hits[0]["read_len"]) == (0, 61)
    # legal but extreme: enormous D / N / H / P operations and positions near 2^31 must not overflow anything
    far = [put(c0 + 4, "<I", (0xfffffff << 4) | 2), put(c0 + 4, "<I", (0xfffffff << 4) | 3), put(8, "<i", 0x7ffffff0),
           ic.make_read(ic.C1, 100, [("H", 0xfffffff), ("M", 30), ("P", 0xfffffff), ("M", 10), ("H", 0xfffffff)])]
    hits, _, cls = run(program, tmp_path, ic.HAND_CONTIGS, names, loci, rid, far)
    assert (cls == 0).all()
