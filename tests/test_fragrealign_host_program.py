"""The realigning fragment session without its pair-HMM kernels, on the CPU under the sanitizers (no GPU): csrc/vlr_fragpileup_host.cpp
with its two extra arguments compiles the text of csrc/vlr_fragpileup.h — the evidence of a flagged record (candidate region, windows),
the gather of the four windows byte by byte, normalize_support, apply_realigned — with -fsanitize=address,undefined into a stand-alone
program; nothing is preloaded into any process.  Every record, every contig and every gathered window lies in a heap block of exactly
its size, so a read or write behind one is a report.  The evidences and window bytes must equal the restatement's, and with the
restatement's raw scores handed in, the observations must equal the restatement's, f64 compared with ==."""
import os
import struct
import subprocess

import numpy as np
import pytest

import basecall_cases as bc
import fragment_cases as fc
import fragrealign_cases as rc
import host_program
from test_fragpileup_host import run as run_plain
from varlociraptor_amd import abi, basecalls, fragments
from varlociraptor_amd.readwindows import read_bam


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "vlr_fragpileup_host")


def run(program, tmp, contigs, loci, records, props, spec, evidences):
    """(observations, locus records, hits, window bytes, Tables) of the host program in its realigning mode; `evidences`: the
    restatement's, for their raw scores"""
    starts = np.concatenate(([0], np.cumsum([len(r) for r in records]))).astype(np.uint64)
    blob = b"VFPH" + struct.pack("<iqiiq", 1, props.window, props.max_mapq, props.max_read_len, len(loci))
    blob += np.array([l.ref_id for l in loci], np.int32).tobytes() + np.array([l.start for l in loci], np.int64).tobytes()
    blob += np.array([len(l.ref) for l in loci], np.int32).tobytes() + np.array([l.kind for l in loci], np.uint8).tobytes()
    blob += b"".join(l.ref for l in loci) + b"".join(l.alt for l in loci)
    blob += struct.pack("<q", len(records)) + starts.tobytes() + b"".join(records)
    rblob = b"VFRH" + struct.pack("<iq", spec.window, len(contigs))
    for seq in contigs.values():
        rblob += struct.pack("<q", len(seq)) + seq.upper()
    rblob += struct.pack("<q", len(evidences)) + np.array([[e.ln_ref, e.ln_alt] for e in evidences], np.float64).tobytes()
    paths = [os.path.join(str(tmp), n) for n in ("in.bin", "out.bin", "rin.bin", "rout.bin")]
    for p, b in ((paths[0], blob), (paths[2], rblob)):
        with open(p, "wb") as f:
            f.write(b)
    r = subprocess.run([program] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    d = open(paths[1], "rb").read()
    n, = struct.unpack_from("<q", d, 4096)
    obs = np.frombuffer(d, abi.FRAGPILEUP_OBS_DTYPE, n, 4104)
    lrec = np.frombuffer(d, abi.FRAGPILEUP_LOCUS_DTYPE, len(loci), 4104 + 56 * n)
    rd = open(paths[3], "rb").read()
    ne, = struct.unpack_from("<q", rd, 0)
    return obs, lrec, np.frombuffer(rd, abi.INDELPILEUP_HIT_DTYPE, ne, 8), rd[8 + 64 * ne:]


def same_as_restatement(program, tmp, contigs, cands, records, props, spec=fragments.RealignSpec()):
    loci = bc.loci_of(cands, contigs)
    bam, _ = bc.write_case(tmp, "case", contigs, records)
    _, _, _, tables = run_plain(program, tmp, loci, records, props)       # the program's own tables
    rs = fragments.restate(read_bam(bam)[1], loci, props, tables, realign=spec, ref_seqs=rc.ref_seqs_of(contigs))
    obs, lrec, hits, windows = run(program, tmp, contigs, loci, records, props, spec, rs.evidences)
    assert rc.hit_keys(hits) == rc.evidence_keys(rs.evidences) and not hits["pad"].any()
    assert windows == b"".join(e.ev.ref_allele + e.alt_allele + e.ev.read_window + e.ev.quals for e in rs.evidences)
    fc.assert_same(obs, lrec, rs)      # f64 with ==: normalize_support makes the libm calls realign.normalize_support makes
    return obs, hits, rs


def test_hand_records_edges_and_refusals(oracle, program, tmp_path):
    recs = rc.hand_records()
    obs, hits, rs = same_as_restatement(program, tmp_path, {"c1": rc.REF}, [rc.SNV20, rc.MNV40], list(recs.values()), rc.P30)
    assert len(hits) == 10 and len(obs) > 6
    for label, (rec, cand) in rc.edge_records().items():
        for window in (1, 20, 64):
            _, hits, _ = same_as_restatement(program, tmp_path, {"c1": rc.REF}, [cand], [rec], rc.P30, fragments.RealignSpec(window))
            assert len(hits) == 1 and hits["status"][0] == 0, label
    contigs, cand, rec = rc.long_read_case()
    _, hits, _ = same_as_restatement(program, tmp_path, contigs, [cand], [rec], fragments.Props(200, 60, 151))
    assert int(hits["read_len"][0]) == 128
    obs, hits, _ = same_as_restatement(program, tmp_path, {"c1": rc.REF}, [rc.SNV20], list(rc.refused_records().values()), rc.P30)
    assert list(hits["status"]) == [abi.INDELPILEUP_HIT_LEADING_REFSKIP, abi.INDELPILEUP_HIT_STRAND_INFO]
    assert sorted(int(s) for s in obs["status"]) == [0, abi.BASEPILEUP_HIT_LEADING_REFSKIP, abi.FRAGPILEUP_OBS_REALIGN_STRAND_INFO]


def test_synthetic_pairs(oracle, program, tmp_path):
    contigs, cands, recs, props = fc.synthetic(n_pairs=600)
    obs, hits, rs = same_as_restatement(program, tmp_path, contigs, cands, recs, props)
    assert len(hits) > 30 and len(obs) > 300 and not (obs["status"] & basecalls.NEEDS_REALIGN).any()
    # the existing output stays what it was: without the two arguments the flagged members come back flagged
    plain, _, _, _ = run_plain(program, tmp_path, bc.loci_of(cands, contigs), recs, props, realign=True)
    assert (plain["status"] & basecalls.NEEDS_REALIGN).any()


def test_counted_evidences(oracle, program, tmp_path):
    for n in (0, 1, 65):
        contigs, cands, recs, props = rc.counted(n)
        _, hits, _ = same_as_restatement(program, tmp_path, contigs, cands, recs, props)
        assert len(hits) == n
