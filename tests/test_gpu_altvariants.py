"""The other alleles of a locus (`alt_variants`) on the device (vlr_fragpileup_set_alt_variants, csrc/vlr_altvariants.h and the
frag_alt_* kernels of csrc/vlr_fragpileup.hip) against the restatement of varlociraptor_amd/fragments.py: winner, n_tied and the
distances with ==, the raw scores with == against the same windows sent through realign.best_hits / prob_related* (the restatement
scored on the device), observations field for field, finished supports within 1e-9 of the restatement scored on the CPU.  The
parent commit has neither the entry points nor the flag."""
import os

import numpy as np
import pytest

import altvariant_cases as ac
import basecall_cases as bc
import fragindel_cases as ic
from varlociraptor_amd import abi, engine, fragments
from varlociraptor_amd.readwindows import read_bam

pytestmark = pytest.mark.gpu
F = fragments
TOL = 1e-9
PJ = {"insert_size": {"mean": 130.0, "sd": 12.0}, "max_del_cigar_len": 4, "max_ins_cigar_len": 4, "frac_max_softclip": 0.1, "max_read_len": ac.READ, "max_mapq": 60}


def hit_keys(arr):
    return [(int(h["locus"]), int(h["record"]), int(h["status"]), (int(h["read_begin"]), int(h["read_begin"]) + int(h["read_len"])),
             (int(h["ref_begin"]), int(h["ref_begin"]) + int(h["ref_len"])), int(h["flag"]), int(h["mapq"])) for h in arr]


def sorted_sites(ref, cands, window=64):
    """(sites sorted by start as a session takes them, their competitor windows)"""
    sites, comp = ac.sites_and_windows(ref, cands, window)
    order = sorted(range(len(sites)), key=lambda k: sites[k].start)
    return [sites[k] for k in order], [comp[k] for k in order]


def same(tmp, name, ref, sites, comp, records, props=ac.PROPS, spec=F.RealignSpec(), cpu=True, **kw):
    """one indel session with competitors against the restatement; returns what the session gave"""
    bam, fa = bc.write_case(tmp, name, {"a1": ref}, records)
    got = F.device_indel_observations(bam, sites, props, True, spec, fa, 0, competitors=comp, **kw)
    obs, obx, loc, lox, res, ev, rres, ah, ac_ = got
    assert res.status == 0, res.status
    recs = read_bam(bam)[1]
    on_dev = F.restate_indel(recs, sites, props, True, spec, {0: ref.upper()}, 0, competitors=comp)
    want = on_dev.evidences
    assert hit_keys(ev) == [e.key() for e in want] and not ev["pad"].any() and not ah["pad"].any()
    assert [(int(a["winner"]), int(a["n_tied"]), int(a["n_ref_side_hits"])) for a in ah] == [(e.winner, e.n_tied, e.n_ref_side_hits) for e in want]
    assert [(float(h["ln_ref"]), float(h["ln_alt"]), int(h["dist_ref"]), int(h["dist_alt"])) for h in ev] == [(e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt) for e in want]
    ic.assert_same(obs, obx, loc, lox, on_dev)
    assert int(ac_.n_edit_pairs) == sum(2 + len(comp[e.locus]) for e in want)
    assert int(ac_.n_hmm_pairs) == sum(1 + max(1, e.n_tied) for e in want)
    assert int(ac_.n_competitors) == sum(len(c) for c in comp) and int(ac_.n_loci_with_competitors) == sum(1 for c in comp if c)
    if cpu:
        on_cpu = F.restate_indel(recs, sites, props, True, spec, {0: ref.upper()}, "cpu", competitors=comp)
        assert [(e.winner, e.n_tied, e.dist_ref, e.dist_alt) for e in on_cpu.evidences] == [(e.winner, e.n_tied, e.dist_ref, e.dist_alt) for e in want]
        ic.assert_same(obs, obx, loc, lox, on_cpu, TOL)
    return got, bam, fa, on_dev


# ------------------------------------------------------------------------------------------------ the two-deletion site
@pytest.mark.parametrize("mode", ["exact", "fast", "homopolymer"])
def test_two_deletions_at_one_position(oracle, tmp_path, mode):
    ref = ac.contig()
    sites, comp = sorted_sites(ref, ac.two_deletions(ref))
    recs = ac.by_start(ac.del_reads(ref, "G", 6) + ac.del_reads(ref, "A", 3, prefix="t") + ac.del_reads(ref, "ref", 2, prefix="r"))
    (obs, obx, loc, lox, res, ev, rres, ah, cnt), bam, _, rs = same(tmp_path, "two_" + mode, ref, sites, comp, recs, spec=F.RealignSpec(64, mode))
    names = [r.qname for r in read_bam(bam)[1]]
    g = [k for k, h in enumerate(ev) if names[int(h["record"])].startswith("dG")]
    # stated from the sequences: at TGA>T (locus 0) a read with the G deleted is 0 edits from the competitor TG>T and wins through it
    at0 = [k for k in g if int(ev[k]["locus"]) == 0]
    assert len(at0) == 6 and all((int(ah[k]["winner"]), int(ev[k]["dist_ref"]), int(ev[k]["dist_alt"])) == (1, 0, 1) for k in at0)
    # ... and stays alt support of TG>T (locus 1)
    at1 = [k for k in g if int(ev[k]["locus"]) == 1]
    assert all(int(ah[k]["winner"]) == 0 and int(ev[k]["dist_alt"]) == 0 and float(ev[k]["ln_alt"]) > float(ev[k]["ln_ref"]) for k in at1)
    o0 = obs[int(loc[0]["obs_offset"]):int(loc[0]["obs_offset"]) + int(loc[0]["n_obs"])]
    gl = {int(ev[k]["record"]) for k in at0}
    assert sum(1 for o in o0 if int(o["left"]) in gl and o["prob_ref"] > o["prob_alt"] + 10.0) == 6


def test_the_compaction_scores_only_the_tied_set_and_the_alt_pair(oracle, tmp_path):
    ref = ac.contig()
    sites, comp = sorted_sites(ref, ac.two_deletions(ref))
    # TGA>T alone in the session, TG>T its competitor
    (_, _, _, _, _, ev, _, ah, cnt), _, _, _ = same(tmp_path, "g", ref, sites[:1], comp[:1], ac.del_reads(ref, "G", 7), cpu=False)
    assert len(ev) == 7 and int(cnt.n_hmm_pairs) == 2 * 7 and int(cnt.n_edit_pairs) == 3 * 7 and set(ah["n_tied"]) == {1}
    # the tie: reads with the A deleted are one edit from the reference and from the competitor
    (_, _, _, _, _, ev, _, ah, cnt), _, _, _ = same(tmp_path, "a", ref, sites[:1], comp[:1], ac.del_reads(ref, "A", 5), cpu=False)
    assert len(ev) == 5 and int(cnt.n_hmm_pairs) == 3 * 5 and int(cnt.n_edit_pairs) == 3 * 5 and set(ah["n_tied"]) == {2}


# ------------------------------------------------------------------------------------------------ shapes
@pytest.fixture(scope="module")
def mixed():
    """loci with K = 0 (a lone deletion), 1 (the two deletions) and 15 (sixteen insertions) in one session: 3 + 2 * 3 + 16 * 17 = 281
    evidences, one above a whole block of the select kernel, with irregular pair offsets"""
    ref = ac.contig()
    cands = ac.lone_deletion(ref) + ac.two_deletions(ref) + ac.insertions(ref, 16)
    sites, comp = sorted_sites(ref, cands)
    recs = ac.by_start(ac.plain_reads(ref, ac.LONE_AT + 2, 3, "l") + ac.del_reads(ref, "G", 2) + ac.del_reads(ref, "A", 1, prefix="t") + ac.ins_reads(ref, 12) +
                       ac.plain_reads(ref, ac.INS_AT, 5, "q"))
    return ref, sites, comp, recs


def test_loci_with_0_1_and_15_competitors_interleaved(oracle, tmp_path, mixed):
    ref, sites, comp, recs = mixed
    assert [len(c) for c in comp] == [0, 1, 1] + [15] * 16
    (obs, _, loc, _, _, ev, rres, ah, cnt), _, _, rs = same(tmp_path, "mixed", ref, sites, comp, recs)
    assert len(ev) == 3 + 2 * 3 + 16 * 17 == 281 and int(rres.n_ranges) == 1
    # the twelve reads that carry insertion 3 are at distance 0 from it: it wins at every other insertion candidate
    k3 = 3 + 3                                     # the locus of insertion 3 in the sorted session
    w = [int(a["winner"]) for a, h in zip(ah, ev) if int(h["locus"]) not in (0, 1, 2, k3) and int(h["dist_ref"]) == 0 and int(a["winner"]) > 0]
    assert len(w) == 12 * 15
    assert all(int(a["winner"]) == 0 and int(a["n_tied"]) == 1 for a, h in zip(ah, ev) if int(h["locus"]) == 0)


@pytest.mark.parametrize("n", [3, 4, 5, 257])
def test_evidence_counts_at_the_block_edges(oracle, tmp_path, n):
    """the expand kernel takes four evidences per block, the select and collect kernels 256"""
    ref = ac.contig()
    sites, comp = sorted_sites(ref, ac.lone_deletion(ref) + ac.two_deletions(ref))
    recs = ac.by_start(ac.plain_reads(ref, ac.LONE_AT + 2, n % 2, "l") + ac.del_reads(ref, "G", n // 2))
    (_, _, _, _, _, ev, _, _, _), _, _, _ = same(tmp_path, "n%d" % n, ref, sites, comp, recs, cpu=False)
    assert len(ev) == n


def test_windows_at_the_lane_stride_and_a_128_base_read_window(oracle, tmp_path):
    ref = ac.contig()
    sites, comp = sorted_sites(ref, ac.two_deletions(ref))
    w = comp[0][0]
    lo = len(w) // 2 - 31
    cut = [w[lo:lo + 63], w[lo:lo + 64], w[lo:lo + 65], w]          # windows of 63, 64 and 65 bytes around the site, and the whole one
    props = F.Props(200, 60, 150)
    recs = [ac.del_read(ref, ac.DEL_AT - 75 + k, "G", "long%d" % k, length=150) for k in range(3)] + ac.del_reads(ref, "G", 2)
    (_, _, _, _, _, ev, _, ah, _), _, _, _ = same(tmp_path, "lanes", ref, sites[:1], [cut], ac.by_start(recs), props=props)
    assert [len(c) for c in cut[:3]] == [63, 64, 65] and sorted(int(h["read_len"]) for h in ev)[-3:] == [128, 128, 128]
    assert all(int(a["n_ref_side_hits"]) >= 2 for a in ah)


def test_ranges_do_not_change_a_byte(oracle, tmp_path, mixed):
    ref, sites, comp, recs = mixed
    (obs, obx, loc, lox, _, ev, rres, ah, cnt), bam, fa, _ = same(tmp_path, "whole", ref, sites, comp, recs, cpu=False)
    whole = [a.tobytes() for a in (obs, obx, loc, lox, ev, ah)]
    # an evidence of an insertion locus has 17 pairs of about 200 + 40 bytes: 6000 bytes hold one such evidence and not two, so every one
    # of them is a range of its own and the boundary falls between two evidences of the same locus
    for limit, least in ((6000, 16 * 17), (40000, 10), (0, 1)):
        got = F.device_indel_observations(bam, sites, ac.PROPS, True, F.RealignSpec(), fa, 0, competitors=comp, pair_byte_limit=limit)
        assert [a.tobytes() for a in got[:4] + (got[5], got[7])] == whole
        assert int(got[6].n_ranges) >= least and (int(got[8].n_edit_pairs), int(got[8].n_hmm_pairs)) == (int(cnt.n_edit_pairs), int(cnt.n_hmm_pairs))
    # determinism: the same bytes from a second run and from other feed chunkings
    for wb in (0, 4096, 70000):
        got = F.device_indel_observations(bam, sites, ac.PROPS, True, F.RealignSpec(), fa, 0, competitors=comp, window_bytes=wb)
        assert [a.tobytes() for a in got[:4] + (got[5], got[7])] == whole


def test_an_evidence_overflow_is_reported_and_the_retry_succeeds(oracle, tmp_path, mixed):
    ref, sites, comp, recs = mixed
    bam, fa = bc.write_case(tmp_path, "over", {"a1": ref}, recs)
    full = F.device_indel_observations(bam, sites, ac.PROPS, True, F.RealignSpec(), fa, 0, competitors=comp)
    short = F.device_indel_observations(bam, sites, ac.PROPS, True, F.RealignSpec(), fa, 0, competitors=comp, evidence_capacity=100, retry=False)
    assert short[4].status & abi.FRAGPILEUP_EVIDENCE_OVERFLOW and int(short[6].needed_evidences) == 281 and len(short[0]) == 0 and len(short[7]) == 0
    again = F.device_indel_observations(bam, sites, ac.PROPS, True, F.RealignSpec(), fa, 0, competitors=comp, evidence_capacity=100)
    assert again[4].status == 0 and [a.tobytes() for a in again[:4] + (again[5], again[7])] == [a.tobytes() for a in full[:4] + (full[5], full[7])]


# ------------------------------------------------------------------------------------------------ sessions without competitors
def test_a_session_without_the_call_is_the_parents(oracle, tmp_path):
    """a case of fragindel_cases.py: without vlr_fragpileup_set_alt_variants the session gives what the restatement without competitors
    gives (the parent's expectation), and a table without any competitor gives the same bytes through the other path"""
    ref = ic.contig()
    _, sites = ic.sites_of(ref)
    recs = ic.pairs(ref, 60)
    bam, fa = bc.write_case(tmp_path, "plain", {"i1": ref}, recs)
    obs, obx, loc, lox, res, ev, rres = F.device_indel_observations(bam, sites, ic.PROPS, True, F.RealignSpec(), fa, 0)
    want = F.restate_indel(read_bam(bam)[1], sites, ic.PROPS, True, F.RealignSpec(), {0: ref.upper()}, 0)
    assert [(float(h["ln_ref"]), float(h["ln_alt"]), int(h["dist_ref"]), int(h["dist_alt"])) for h in ev] == [(e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt) for e in want.evidences]
    ic.assert_same(obs, obx, loc, lox, want)
    empty = F.device_indel_observations(bam, sites, ic.PROPS, True, F.RealignSpec(), fa, 0, competitors=[[] for _ in sites])
    assert [a.tobytes() for a in empty[:4] + (empty[5],)] == [a.tobytes() for a in (obs, obx, loc, lox, ev)]
    assert int(empty[8].n_edit_pairs) == int(empty[8].n_hmm_pairs) == 2 * len(ev) and not empty[7]["winner"].any()


# ------------------------------------------------------------------------------------------------ refusals
def _refused(L, h, comp_off, base_off=None, bases=None):
    """the message of a vlr_fragpileup_set_alt_variants that must be refused with VLR_ERR_INVALID_ARGUMENT"""
    u64 = lambda v: None if v is None else np.array(v, np.uint64)
    arrays = (u64(comp_off), u64(base_off), bases)
    try:
        engine._check(L.vlr_fragpileup_set_alt_variants(h, *(a.ctypes.data if a is not None else None for a in arrays)))
    except engine.EngineError as e:
        assert e.code == abi.ERR_INVALID_ARGUMENT
        return str(e)
    raise AssertionError("vlr_fragpileup_set_alt_variants took %r" % (arrays,))


def _open_indel(L, sites, fa):
    """an indel session opened through the C ABI itself (the arrays must outlive the open call only)"""
    import ctypes as C
    from varlociraptor_amd import realign as rl
    from varlociraptor_amd.readwindows import MODES, locus_arrays
    arrays = locus_arrays([s.ref_id for s in sites], [s.locus for s in sites])
    h = C.c_void_p()
    engine._check(L.vlr_fragpileup_open_indel(0, len(sites), *(a.ctypes.data for a in arrays), ac.PROPS.window, ac.PROPS.max_mapq, ac.PROPS.max_read_len, 1 << 12, 1 << 16,
                                              1 << 12, 0, fa.encode(), 64, MODES["exact"], rl.GapParams().as_array(), None, 1 << 12, 0, 1, C.byref(h)))
    return h


def _finish(L, h, n_loci, bam=None):
    """add `bam` (if given), collect, and return the bytes of the observations; the session stays open"""
    import ctypes as C
    if bam is not None:
        engine._check(L.vlr_fragpileup_add_bam(h, bam.encode()))
    res = abi.FragPileupCounts()
    engine._check(L.vlr_fragpileup_result(h, C.byref(res)))
    assert res.status == 0
    obs, loc = np.zeros(int(res.n_obs), abi.FRAGPILEUP_OBS_DTYPE), np.zeros(n_loci, abi.FRAGPILEUP_LOCUS_DTYPE)
    engine._check(L.vlr_fragpileup_read(h, obs.ctypes.data, len(obs), loc.ctypes.data, n_loci))
    return obs.tobytes()


def test_refusals_leave_the_session_usable(oracle, tmp_path):
    """every refusal the header lists: VLR_ERR_INVALID_ARGUMENT with a message that names the locus or the competitor, and the session
    goes on as if the call had not been made (the refusals return before anything is uploaded: csrc/vlr_fragpileup.hip)"""
    import ctypes as C
    from varlociraptor_amd import basecalls
    L = engine.lib()
    ref = ac.contig()
    sites, comp = sorted_sites(ref, ac.two_deletions(ref))
    recs = ac.by_start(ac.del_reads(ref, "G", 4) + ac.del_reads(ref, "A", 2, prefix="t"))
    bam, fa = bc.write_case(tmp_path, "ref", {"a1": ref}, recs)
    with_comp = F.device_indel_observations(bam, sites, ac.PROPS, True, F.RealignSpec(), fa, 0, competitors=comp)[0].tobytes()
    without = F.device_indel_observations(bam, sites, ac.PROPS, True, F.RealignSpec(), fa, 0)[0].tobytes()
    assert with_comp != without
    w = comp[0][0]
    bases = np.frombuffer(w * 16, np.uint8).copy()
    limit = abi.FRAGPILEUP_MAX_INDEL_LEN + 2 * int(64 * 1.5)
    # an indel session: every malformed table is refused, the good one is taken once, and the results are those of a clean session
    h = _open_indel(L, sites, fa)
    try:
        said = _refused(L, h, [0, 16, 16], [len(w) * k for k in range(17)], bases)                 # sixteen competitors at locus 0
        assert "locus 0" in said and "16" in said
        assert "locus 1" in _refused(L, h, [0, 2, 1], [0, len(w), 2 * len(w)], bases)              # descending competitor offsets
        assert "competitor 1" in _refused(L, h, [0, 1, 2], [0, len(w), len(w) - 1], bases)         # descending window offsets
        said = _refused(L, h, [0, 1, 1], [0, limit + 1], np.full(limit + 1, ord("A"), np.uint8))   # a window above the session's limit
        assert "competitor 0" in said and str(limit) in said
        assert "competitor 0" in _refused(L, h, [0, 1, 1], [0, 0], bases)                          # an empty window
        _refused(L, h, [0, 1, 1])                                                                  # competitors without their windows
        with pytest.raises(engine.EngineError):                                                    # a file that cannot be opened is not the first BAM
            engine._check(L.vlr_fragpileup_add_bam(h, str(tmp_path / "missing.bam").encode()))
        good = F.competitor_arrays(comp)
        engine._check(L.vlr_fragpileup_set_alt_variants(h, *(a.ctypes.data for a in good)))
        assert "already" in _refused(L, h, [0, 0, 0])                                              # a second call
        assert _finish(L, h, 2, bam) == with_comp
    finally:
        L.vlr_fragpileup_close(h)
    # after a BAM was added
    h = _open_indel(L, sites, fa)
    try:
        engine._check(L.vlr_fragpileup_add_bam(h, bam.encode()))
        assert "add_bam" in _refused(L, h, [0, 0, 0])
        assert _finish(L, h, 2) == without
    finally:
        L.vlr_fragpileup_close(h)
    # sessions that do not realign: a plain one and a methylation one
    loci = bc.loci_of([ac.mnv_site(ref)[1]], {"a1": ref})
    arrays = basecalls.locus_arrays(loci)
    h = C.c_void_p()
    engine._check(L.vlr_fragpileup_open(0, 1, *(a.ctypes.data for a in arrays), 1, ac.PROPS.window, ac.PROPS.max_mapq, ac.PROPS.max_read_len, 1 << 12, 1 << 16, 1 << 12, 0,
                                        C.byref(h)))
    try:
        assert "vlr_fragpileup_open_realign" in _refused(L, h, [0, 0])
        assert _finish(L, h, 1, bam) == F.device_observations(bam, loci, ac.PROPS, 0, True)[0].tobytes()
    finally:
        L.vlr_fragpileup_close(h)
    h = C.c_void_p()
    ref_id, start = np.zeros(1, np.int32), np.array([ac.MNV_AT], np.int64)
    engine._check(L.vlr_fragpileup_open_methylation(0, 1, ref_id.ctypes.data, start.ctypes.data, abi.METH_CONVERTED, ac.PROPS.window, ac.PROPS.max_mapq, ac.PROPS.max_read_len,
                                                    1 << 12, 1 << 16, 1 << 12, 0, C.byref(h)))
    try:
        assert "vlr_fragpileup_open_realign" in _refused(L, h, [0, 0])
        _finish(L, h, 1, bam)
    finally:
        L.vlr_fragpileup_close(h)


# ------------------------------------------------------------------------------------------------ an MNV in a realigning session
def test_an_mnv_with_a_competitor_in_a_realigning_session(oracle, tmp_path):
    ref = ac.contig()
    mnv, snv, mnv2 = ac.mnv_site(ref)
    cands = [mnv, snv, mnv2]
    # reads without an I / D operation that enclose the site, one of them carrying the second MNV, and one read with a deletion nearby
    recs = ac.plain_reads(ref, ac.MNV_AT, 5, "p")
    start = ac.MNV_AT - 20
    carrier = bc.make_read(ref, start, [("M", ac.READ)], edits={20: chr(mnv2[3][0]), 21: chr(mnv2[3][1])}, name="carrier")
    gapped = bc.make_read(ref, start, [("M", 10), ("D", 1), ("M", ac.READ - 10)], name="gapped")
    recs = ac.by_start(recs + [carrier, gapped])
    bam, fa = bc.write_case(tmp_path, "mnv", {"a1": ref}, recs)
    loci = bc.loci_of(cands, {"a1": ref})
    spec = F.RealignSpec()
    key = lambda l: (l.start, bytes(l.ref), bytes(l.alt))
    by_key = {(c[1], bytes(c[2]), bytes(c[3])): k for k, c in enumerate(cands)}
    groups = F.alt_variant_groups(cands)
    comp = [[F.competitor_window(ref, *cands[j][1:], spec.window) for j in groups[by_key[key(l)]]] for l in loci]
    obs, loc, res, ev, rres, ah, cnt = F.device_observations(bam, loci, ac.PROPS, 0, realign=spec, fasta=fa, evidences=True, competitors=comp)
    assert res.status == 0
    records = read_bam(bam)[1]
    want = F.restate(records, loci, ac.PROPS, basecalls_tables(), realign=spec, ref_seqs={0: ref.upper()}, device=0, competitors=comp)
    assert hit_keys(ev) == [e.key() for e in want.evidences]
    assert [(float(h["ln_ref"]), float(h["ln_alt"]), int(h["dist_ref"]), int(h["dist_alt"])) for h in ev] == [(e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt) for e in want.evidences]
    assert [(int(a["winner"]), int(a["n_tied"]), int(a["n_ref_side_hits"])) for a in ah] == [(e.winner, e.n_tied, e.n_ref_side_hits) for e in want.evidences]
    # the two MNVs realign all seven enclosing reads, the SNV only the read with the deletion
    is_mnv = [len(l.ref) > 1 for l in loci]
    per = [sum(1 for h in ev if int(h["locus"]) == j) for j in range(3)]
    assert per == [7 if m else 1 for m in is_mnv]
    # the read that carries the second MNV counts against the first one through the competitor, at distance 0
    names = [r.qname for r in records]
    first = by_key_index(loci, mnv)
    c = [k for k, h in enumerate(ev) if int(h["locus"]) == first and names[int(h["record"])] == "carrier"]
    assert len(c) == 1 and int(ah[c[0]]["winner"]) > 0 and int(ev[c[0]]["dist_ref"]) == 0 and float(ev[c[0]]["ln_ref"]) > float(ev[c[0]]["ln_alt"])
    at = 0
    for j, w in enumerate(want.per_locus):
        n = int(loc[j]["n_obs"])
        got = F.obs_from_array(obs[at:at + n])
        assert [g.key() for g in got] == [o.key() for o in w], j
        at += n
    assert at == len(obs)


def basecalls_tables():
    from varlociraptor_amd import basecalls
    return basecalls.library_tables()


def by_key_index(loci, cand):
    return [k for k, l in enumerate(loci) if (l.start, bytes(l.ref), bytes(l.alt)) == (cand[1], bytes(cand[2]), bytes(cand[3]))][0]


# ------------------------------------------------------------------------------------------------ the command
def test_the_command_with_and_without_the_flag(oracle, tmp_path):
    import json
    from varlociraptor_amd import alignprops, cli, ingest
    import struct
    ref = ac.contig()
    cands = ac.two_deletions(ref)
    recs = ac.by_start(ac.del_reads(ref, "G", 8) + ac.del_reads(ref, "ref", 4, prefix="r"))
    bam, fa = bc.write_case(tmp_path, "cmd", {"a1": ref}, recs)
    vcf, props = os.path.join(str(tmp_path), "c.vcf"), os.path.join(str(tmp_path), "p.json")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=a1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for c, pos, r, a in cands:
            f.write("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (c, pos + 1, r.decode(), a.decode()))
    json.dump(PJ, open(props, "w"))
    out = {k: os.path.join(str(tmp_path), k + ".bcf") for k in ("flag", "noflag", "direct")}
    args = ["preprocess", "variants", fa, "--candidates", vcf, "--bam", bam, "--alignment-properties", props, "--atomic-candidate-variants", "--indel-candidates"]
    cli.main(args + ["--alt-variants", "--output", out["flag"]])
    cli.main(args + ["--output", out["noflag"]])
    # without the flag: the bytes the function writes without the argument, as it always has
    assert F.preprocess_variants(fa, vcf, bam, out["direct"], props, 0, atomic_candidate_variants=True, indel_candidates=F.RealignSpec()) == 2

    def records_of(path):
        d = alignprops.inflate_bgzf(path)
        l_text, = struct.unpack_from("<I", d, 5)
        return bytes(d[9 + l_text:])
    assert records_of(out["noflag"]) == records_of(out["direct"]) != records_of(out["flag"])
    with_flag, _ = ingest.read_observations([out["flag"]])
    without, _ = ingest.read_observations([out["noflag"]])
    off = with_flag.obs_offset
    assert with_flag.n_loci == 2 and int(off[1]) == 12 and list(off) == list(without.obs_offset)
    sl = slice(0, int(off[1]))                                      # TGA>T: all twelve reads are reference support with the flag ...
    pr, pa = with_flag.columns["prob_ref"][sl].astype(float), with_flag.columns["prob_alt"][sl].astype(float)
    assert (pr > pa + 10.0).sum() == 12
    pr0, pa0 = without.columns["prob_ref"][sl].astype(float), without.columns["prob_alt"][sl].astype(float)
    assert (pr0 > pa0 + 10.0).sum() == 4                            # ... and only the four reference reads without it
    # the tables of the command are those of the function on the device, which are the CPU restatement's within the bound
    dev = F.observations(bam, fa, cands, PJ, device=0, indel_candidates=F.RealignSpec(64, "exact", *F.gap_hop_of(PJ)), alt_variants=True)
    cpu = F.observations(bam, fa, cands, PJ, device="cpu", indel_candidates=F.RealignSpec(64, "exact", *F.gap_hop_of(PJ)), alt_variants=True)
    for d, c in zip(dev, cpu):
        assert d.records == c.records and np.abs(d.prob_ref - c.prob_ref).max() <= TOL and np.abs(d.prob_alt - c.prob_alt).max() <= TOL


# ------------------------------------------------------------------------------------------------ a multi-allelic reference testcase
def test_the_three_mnvs_of_test_giab_30_on_the_device(oracle, golden_dir, tmp_path):
    """the three MNV alleles at 1:301 of test_giab_30 (tests/golden/bam/ALTVARIANTS.md) through the realigning session with competitors:
    the tables are those of the CPU restatement within the bound, and every allele meets the testcase's block"""
    import json
    import sys
    import fragment_cases as fc
    from varlociraptor_amd import alignprops
    from varlociraptor_amd.readwindows import read_fasta
    sys.path.insert(0, os.path.join(os.path.dirname(golden_dir), "..", "tools"))
    import make_altvariant_fixtures as tool
    d = os.path.join(golden_dir, "bam", "test_giab_30")
    cand = tool.candidates_of(d)
    bam = fc.fixture_case(golden_dir, "test_giab_30")[0]
    fasta = str(tmp_path / "ref.fa")                       # (the fixtures hold their reference without an index)
    alignprops.write_fasta(fasta, read_fasta(os.path.join(d, "ref.fa")))
    pj = json.load(open(os.path.join(d, "properties.json")))
    spec = F.RealignSpec(64, "exact", *F.gap_hop_of(pj))
    dev = F.observations(bam, fasta, cand, pj, device=0, realign=spec, alt_variants=True)
    cpu = F.observations(bam, fasta, cand, pj, device="cpu", realign=spec, alt_variants=True)
    alone = F.observations(bam, fasta, cand, pj, device=0, realign=spec)
    for t, c in zip(dev, cpu):
        assert t.records == c.records and len(t) == 19 and np.abs(t.prob_ref - c.prob_ref).max() <= TOL and np.abs(t.prob_alt - c.prob_alt).max() <= TOL
    assert [int((t.prob_alt > t.prob_ref).sum()) for t in dev] == [g[1] for g in tool.call_site(d, True)]
    assert any((a.prob_ref != t.prob_ref).any() for a, t in zip(alone, dev))
    for n, n_alt, vaf, phred in tool.call_site(d, True, device=0, fasta=fasta):
        assert fc.FIXTURES["test_giab_30"][0](vaf, phred)
