"""The passes of a session with competitors (csrc/vlr_altvariants.h: layout, expand, select, compact, collect) on the CPU under the
sanitizers (no GPU): csrc/vlr_altvariants_host.cpp compiles the text the kernels of csrc/vlr_fragpileup.hip run, with
-fsanitize=address,undefined, into a stand-alone program; nothing is preloaded into any process.  Every window and every array lies
in a heap block of exactly its size, so a read or write behind one is a report.  The expanded and the compacted bytes, the kept pairs,
the winner, n_tied, the distances and the scores must equal what the restatement of fragments.py says of the same evidences."""
import os
import struct
import subprocess

import numpy as np
import pytest

import altvariant_cases as ac
import basecall_cases as bc
import host_program
from varlociraptor_amd import abi, fragments, readwindows, realign
from varlociraptor_amd.readwindows import read_bam

F = fragments


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "vlr_altvariants_host")


def pack_table(comp, limit, n_base_off=None):
    off, boff, bases = F.competitor_arrays(comp)
    boff = boff[:n_base_off] if n_base_off is not None else boff
    blob = b"VAVH" + struct.pack("<q", len(comp)) + off.tobytes() + struct.pack("<q", len(boff)) + boff.tobytes()
    return blob + (bases.tobytes()[:int(boff[-1])] if len(boff) else b"") + struct.pack("<Q", limit)


def all_pairs(evs, comp, spec):
    """(realign.PairBatch of every pair of the layout, its edit distances, its pair-HMM scores) through the CPU oracle"""
    pb = realign.PairBatch()
    for e in evs:
        for w in [e.ev.ref_allele, e.alt_allele] + [w if not e.ev.status else b"" for w in comp[e.locus]]:
            pb.add(w, e.ev.read_window, e.ev.quals, -1)
    dist = F.pair_edit_distances(pb, "cpu")
    return pb, dist, F.pair_hmm(pb, dist, spec, "cpu")


def run(program, tmp, evs, comp, spec=F.RealignSpec(), limit=1 << 20, dist=None, lnp=None):
    """the program on the evidences `evs` (scored or not) with the competitor windows comp[locus]; the parsed output"""
    pb, d0, l0 = all_pairs(evs, comp, spec)
    dist = d0 if dist is None else np.asarray(dist, np.int32)
    lnp = l0 if lnp is None else np.asarray(lnp, np.float64)
    blob = pack_table(comp, limit) + struct.pack("<iq", int(spec.mode == "fast"), len(evs))
    for e in evs:
        blob += struct.pack("<5I", e.locus, e.ev.status, len(e.ev.ref_allele), len(e.alt_allele), len(e.ev.read_window))
    for e in evs:
        blob += e.ev.ref_allele + e.alt_allele + e.ev.read_window + e.ev.quals
    blob += struct.pack("<q", len(pb)) + dist.astype(np.int32).tobytes() + lnp.astype(np.float64).tobytes()
    out = run_blob(program, tmp, blob)
    bad, where = struct.unpack_from("<iq", out, 0)
    assert bad == 0, (bad, where)
    n_pairs, n_kept = struct.unpack_from("<qq", out, 12)
    assert n_pairs == len(pb)
    o = 28
    xoff = np.frombuffer(out, "<u4", n_pairs + 1, o); o += 4 * (n_pairs + 1)
    yoff = np.frombuffer(out, "<u4", n_pairs + 1, o); o += 4 * (n_pairs + 1)
    x = out[o:o + int(xoff[-1])]; o += int(xoff[-1])
    y = out[o:o + int(yoff[-1])]; o += int(yoff[-1])
    q = out[o:o + int(yoff[-1])]; o += int(yoff[-1])
    cxoff = np.frombuffer(out, "<u4", n_kept + 1, o); o += 4 * (n_kept + 1)
    cyoff = np.frombuffer(out, "<u4", n_kept + 1, o); o += 4 * (n_kept + 1)
    cband = np.frombuffer(out, "<i4", n_kept, o); o += 4 * n_kept
    cx = out[o:o + int(cxoff[-1])]; o += int(cxoff[-1])
    cy = out[o:o + int(cyoff[-1])]; o += int(cyoff[-1])
    cq = out[o:o + int(cyoff[-1])]; o += int(cyoff[-1])
    res = np.frombuffer(out, np.dtype([("ln_ref", "<f8"), ("ln_alt", "<f8"), ("dist_ref", "<i4"), ("dist_alt", "<i4"), ("alt", abi.FRAGPILEUP_ALT_HIT_DTYPE)]), len(evs), o)
    assert o + 32 * len(evs) == len(out)
    # the expanded batch is the layout's, byte for byte
    assert x == b"".join(pb.x) and y == b"".join(pb.y) and q == b"".join(bytes(v) for v in pb.q)
    assert list(np.diff(xoff)) == [len(v) for v in pb.x] and list(np.diff(yoff)) == [len(v) for v in pb.y]
    return dict(n_pairs=n_pairs, n_kept=n_kept, cxoff=cxoff, cyoff=cyoff, cband=cband, cx=cx, cy=cy, cq=cq, res=res, pb=pb, dist=dist, lnp=lnp)


def run_blob(program, tmp, blob):
    pin, pout = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(pin, "wb") as f:
        f.write(blob)
    r = subprocess.run([program, pin, pout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return open(pout, "rb").read()


def same_as_restatement(program, tmp, evs, comp, spec=F.RealignSpec()):
    """the program against fragments.score_alt_evidences over the same evidences (scored in place)"""
    n_edit, n_hmm = F.score_alt_evidences(evs, comp, spec, "cpu")
    got = run(program, tmp, evs, comp, spec)
    assert (got["n_pairs"], got["n_kept"]) == (n_edit, n_hmm)
    r = got["res"]
    assert [(float(a["ln_ref"]), float(a["ln_alt"]), int(a["dist_ref"]), int(a["dist_alt"]), int(a["alt"]["winner"]), int(a["alt"]["n_tied"]), int(a["alt"]["n_ref_side_hits"]))
            for a in r] == [(e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt, e.winner, e.n_tied, e.n_ref_side_hits) for e in evs]
    assert not r["alt"]["pad"].any()
    # the compacted batch: per evidence the tied reference-side pairs and the alt pair, in pair order, with band = distance + 4
    pb, dist = got["pb"], got["dist"]
    kept, p0 = [], 0
    for e in evs:
        k = len(comp[e.locus])
        _, tied, _ = F.select_alleles([int(dist[p0])] + [int(dist[p0 + 1 + i]) for i in range(1, k + 1)])
        kept += sorted([p0 if i == 0 else p0 + 1 + i for i in (tied or [0])] + [p0 + 1])
        p0 += 2 + k
    assert got["cx"] == b"".join(pb.x[p] for p in kept) and got["cy"] == b"".join(pb.y[p] for p in kept) and got["cq"] == b"".join(bytes(pb.q[p]) for p in kept)
    assert list(np.diff(got["cxoff"])) == [len(pb.x[p]) for p in kept] and list(np.diff(got["cyoff"])) == [len(pb.y[p]) for p in kept]
    assert list(got["cband"]) == [(int(dist[p]) + realign.EDIT_BAND if dist[p] >= 0 and spec.mode != "fast" else -1) for p in kept]
    return got


def evidences_of(tmp, name, ref, cands, recs, window=64):
    sites, comp = ac.sites_and_windows(ref, cands, window)
    bam, _ = bc.write_case(tmp, name, {"a1": ref}, recs)
    order = sorted(range(len(sites)), key=lambda k: sites[k].start)
    rs = F.restate_indel(read_bam(bam)[1], [sites[k] for k in order], ac.PROPS, True, F.RealignSpec(window), {0: ref.upper()}, "cpu")
    return rs.evidences, [comp[k] for k in order]


def test_the_two_deletion_site_and_the_tie(oracle, program, tmp_path):
    ref = ac.contig()
    recs = ac.by_start(ac.del_reads(ref, "G", 6) + ac.del_reads(ref, "A", 3, prefix="t") + ac.del_reads(ref, "ref", 2, prefix="r"))
    evs, comp = evidences_of(tmp_path, "twodel", ref, ac.two_deletions(ref), recs)
    assert len(evs) == 22
    for mode in ("exact", "fast", "homopolymer"):
        got = same_as_restatement(program, tmp_path, evs, comp, F.RealignSpec(64, mode))
        # a kept pair beyond two per evidence is a tie: the three A-deleted reads at both candidates, and the six G-deleted reads at
        # TG>T, where T A C is one edit from the reference (T G A C) and one from the competitor TGA>T (T C)
        assert got["n_pairs"] == 3 * 22 and got["n_kept"] == 2 * 22 + 2 * 3 + 6
    winners = [(e.locus, e.winner) for e in evs if e.n_tied == 1 and e.dist_ref == 0 and e.dist_alt == 1]
    assert (0, 1) in winners                 # TGA>T: the one-deletion reads win through the competitor


def test_no_competitor_fifteen_competitors_and_loci_interleaved(oracle, program, tmp_path):
    ref = ac.contig()
    cands = ac.lone_deletion(ref) + ac.two_deletions(ref) + ac.insertions(ref, 16)
    recs = ac.by_start(ac.plain_reads(ref, ac.LONE_AT + 2, 3, "l") + ac.del_reads(ref, "G", 3) + ac.ins_reads(ref, 5) + ac.plain_reads(ref, ac.INS_AT, 2, "q"))
    evs, comp = evidences_of(tmp_path, "mixed", ref, cands, recs)
    assert sorted(set(len(c) for c in comp)) == [0, 1, 15]
    got = same_as_restatement(program, tmp_path, evs, comp)
    assert got["n_pairs"] == sum(2 + len(comp[e.locus]) for e in evs)
    # K = 0 evidences keep exactly their two pairs
    assert all(e.n_tied == 1 and e.winner == 0 for e in evs if not comp[e.locus])
    # the reads that carry insertion 3 are at distance 0 from that competitor for every other insertion candidate
    ins3 = [e for e in evs if len(comp[e.locus]) == 15 and e.dist_ref == 0 and e.winner > 0]
    assert len(ins3) >= 5 * 14
    # an evidence alone, and the last evidence's windows at the very end of every block
    same_as_restatement(program, tmp_path, evs[-1:], comp)
    same_as_restatement(program, tmp_path, evs[:1], comp)
    same_as_restatement(program, tmp_path, [], comp)


def test_evidences_with_a_status_and_without_any_hit(oracle, program, tmp_path):
    ref = ac.contig()
    window = ref[100:160]
    refused = F.RealignEvidence(0, readwindows.Evidence(7, readwindows.NO_OVERLAP, (0, 0), (0, 0), b"", b"", b"", 0, 60), b"")
    scored = F.RealignEvidence(0, readwindows.Evidence(8, 0, (0, 40), (100, 160), ref[110:150], bytes([30] * 40), window, 0, 60), ref[90:150])
    comp = [[ref[95:155], ref[105:165]]]
    got = same_as_restatement(program, tmp_path, [refused, scored, refused], comp)
    assert got["n_pairs"] == 12 and got["n_kept"] == 2 + 4 + 2          # a status keeps the (empty) reference and alt pairs
    assert (refused.winner, refused.n_tied, refused.n_ref_side_hits, refused.dist_ref, refused.ln_ref) == (0, 0, 0, -1, -np.inf)
    # no reference-side hit but the reference: the competitors' distances are -1
    pb, dist, lnp = all_pairs([scored], comp, F.RealignSpec())
    d = dist.copy(); d[2:] = -1
    r = run(program, tmp_path, [scored], comp, dist=d, lnp=lnp)["res"][0]
    assert (int(r["alt"]["winner"]), int(r["alt"]["n_tied"]), int(r["alt"]["n_ref_side_hits"]), int(r["dist_ref"]), float(r["ln_ref"])) == (0, 1, 1, int(dist[0]), float(lnp[0]))
    # all distances equal: every reference-side allele is tied; the largest score wins, the lowest index on equal scores
    d = np.full(4, 2, np.int32)
    l = np.array([-5.0, -1.0, -3.0, -3.0])
    got = run(program, tmp_path, [scored], comp, dist=d, lnp=l)
    r = got["res"][0]
    assert got["n_kept"] == 4 and (int(r["alt"]["winner"]), int(r["alt"]["n_tied"]), float(r["ln_ref"]), float(r["ln_alt"])) == (1, 3, -3.0, -1.0)
    l = np.array([-3.0, -1.0, -3.0, -3.0])
    assert int(run(program, tmp_path, [scored], comp, dist=d, lnp=l)["res"][0]["alt"]["winner"]) == 0
    l = np.array([-4.0, -1.0, -3.5, -3.0])
    assert int(run(program, tmp_path, [scored], comp, dist=d, lnp=l)["res"][0]["alt"]["winner"]) == 2


def test_tables_that_are_refused(program, tmp_path):
    w = b"ACGT" * 4
    tail = struct.pack("<iq", 0, 0) + struct.pack("<q", 0)

    def verdict(blob):
        return struct.unpack_from("<iq", run_blob(program, tmp_path, blob + tail), 0)
    assert verdict(pack_table([[w] * 15, []], 64))[0] == 0
    assert verdict(pack_table([[], [w] * 16], 64)) == (2, 1)                      # sixteen competitors at locus 1
    assert verdict(pack_table([[w], [w * 5]], 64)) == (3, 1)                      # a window longer than the limit: competitor 1
    assert verdict(pack_table([[w, w]], 64, n_base_off=2))[0] == 1                # offsets that do not cover the competitors
    off = np.array([0, 2, 1], np.uint64)                                         # descending competitor offsets
    blob = b"VAVH" + struct.pack("<q", 2) + off.tobytes() + struct.pack("<q", 2) + np.array([0, 16], np.uint64).tobytes() + w + struct.pack("<Q", 64)
    assert verdict(blob) == (1, 1)
    boff = np.array([0, 16, 8], np.uint64)                                       # descending window offsets
    blob = b"VAVH" + struct.pack("<q", 1) + np.array([0, 2], np.uint64).tobytes() + struct.pack("<q", 3) + boff.tobytes() + w[:8] + struct.pack("<Q", 64)
    assert verdict(blob) == (1, 1)
