"""Deletion and insertion candidates of `preprocess variants` on the CPU (no GPU): the restatement of varlociraptor_amd/fragments.py with
expectations stated from the records, and csrc/vlr_fragpileup_host.cpp — the indel arms of csrc/vlr_fragpileup.h compiled with
-fsanitize=address,undefined into a stand-alone program (nothing is preloaded into any process; every record, contig, alt window,
member array and gathered window lies in a heap block of exactly its size) — against that restatement, f64 compared with ==."""
import math
import os
import subprocess

import numpy as np
import pytest

import basecall_cases as bc
import fragindel_cases as ic
import host_program
from varlociraptor_amd import abi, fragments
from varlociraptor_amd.basecalls import Hit
from varlociraptor_amd.readwindows import BamRecord, IndelLocus, read_bam

F = fragments


def rec(pos, cigar, name="q", flag=0, mapq=60):
    n = sum(l for op, l in cigar if op in "MIS=X")
    return BamRecord(name, flag, 0, pos, mapq, list(cigar), b"A" * n, bytes([30] * n), 0, 0, 0)


def deletion(start, length):
    return F.IndelSite(0, IndelLocus("deletion", start, start + length, -length, b""))


def insertion(start, length):
    return F.IndelSite(0, IndelLocus("insertion", start, start + 1, length, b""))


def test_centerpoint_rounds_half_away_from_zero():
    # len / 2 = 0.5, 1, 1.5, 2.5, 3 -> 1, 1, 2, 3, 3 (Python's round() would give 0, 1, 2, 2, 3)
    assert [F.centerpoint(100, n) - 100 for n in (1, 2, 3, 5, 6)] == [1, 1, 2, 3, 3]


def test_fetch_merge_boundary():
    # W = 10: the centerpoint locus [s + c, s + c + 1) merges into [s, s + 1) when s + c - 10 <= s + 1 + 10, i.e. c <= 21 = 2 W + 1
    W, s = 10, 1000
    assert F.fetches_merge(s, s + 42, W)            # c = 21; the end locus: s + 41 - 10 <= s + 22 + 10
    assert not F.fetches_merge(s, s + 44, W)        # c = 22
    assert F.fetches_merge(s, s + 41, W) and F.fetches_merge(s, s + 40, W)   # c = 21 (20.5 rounds up), c = 20
    assert F.fetches_merge(5, 47, W)                # the window saturates at 0


def hits_for(*ordinals, strand=abi.STRAND_FORWARD):
    return {(o, 0): Hit(0, o, -1.0, -2.0, strand, None, 0, 60, 0, 0, (o,)) for o in ordinals}


def test_validity_every_arm():
    d = deletion(100, 10)        # [100, 110), centerpoint 105
    obs = lambda l, r, isz, site=d: F.indel_fragment_observation((0, l), (1, r) if r is not None else None, site, 0, 60, isz, hits_for(0, 1))
    # encloses the centerpoint, neither read overlaps [100, 110): none
    assert obs(rec(50, [("M", 40)]), rec(120, [("M", 40)]), True) is None
    # left overlaps, but the pair does not enclose the centerpoint (right ends at 104): none with an insert size, one without
    l, r = rec(70, [("M", 32)]), rec(80, [("M", 24)])
    assert obs(l, r, True) is None
    o = obs(l, r, False)
    assert o is not None and o.insert_size == 0 and (o.len_left, o.len_right) == (32, 24)
    # strict inequalities: left.pos == centerpoint, right.end_pos == centerpoint
    assert obs(rec(105, [("M", 30)]), rec(150, [("M", 30)]), True) is None
    assert obs(rec(104, [("M", 30)]), rec(150, [("M", 30)]), True) is not None
    assert obs(rec(90, [("M", 12)]), rec(95, [("M", 10)]), True) is None          # right ends at 105
    assert obs(rec(90, [("M", 12)]), rec(95, [("M", 11)]), True) is not None      # right ends at 106
    # a single read: valid when it overlaps
    assert obs(rec(109, [("M", 30)]), None, True) is not None and obs(rec(110, [("M", 30)]), None, True) is None
    # an insertion [200, 201): either mate
    i = insertion(200, 4)
    assert obs(rec(150, [("M", 30)]), rec(190, [("M", 30)]), True, i) is not None
    assert obs(rec(190, [("M", 30)]), rec(250, [("M", 30)]), True, i) is not None
    assert obs(rec(150, [("M", 30)]), rec(201, [("M", 30)]), True, i) is None
    # overlap through a soft clip only: the alignment ends at 100, its trailing clip reaches the locus
    assert obs(rec(70, [("M", 30), ("S", 5)]), None, False) is not None and obs(rec(70, [("M", 30)]), None, False) is None
    # MAPQ 0 of either read drops the pair; a merged strand of none gives no observation
    assert obs(rec(90, [("M", 30)], mapq=0), rec(150, [("M", 30)]), True) is None
    assert F.indel_fragment_observation((0, rec(90, [("M", 30)])), None, d, 0, 60, True, hits_for(0, strand=abi.STRAND_NONE)) is None


def test_insert_size_on_hand_cigars():
    # left: pos 100 - (3 S + 2 H) = 95 .. 130; right: 200 .. 240 + 4 H = 244: inner 200 - 130 = 70, spans 35 + 44
    l = rec(100, [("H", 2), ("S", 3), ("M", 30)])
    r = rec(200, [("M", 40), ("H", 4)])
    assert F.clips(l) == (3, 2, 0, 0) and F.clips(r) == (0, 0, 0, 4)
    assert F.estimate_insert_size(l, r) == 149 == 244 - 95
    # pos smaller than the leading clips: the start saturates at 0
    assert F.estimate_insert_size(rec(2, [("S", 5), ("M", 20)]), rec(50, [("M", 20)])) == 70
    # the value is right_end - left_start whatever the order of the starts: a `left` at 104 with a `right` over [90, 106) gives 2 ...
    d = deletion(100, 10)
    both = {(3, 0): hits_for(3)[(3, 0)], (9, 0): hits_for(9)[(9, 0)]}
    o = F.indel_fragment_observation((3, rec(104, [("M", 10)])), (9, rec(90, [("M", 16)])), d, 0, 60, True, both)
    assert o.insert_size == 106 - 104 and not o.flags
    # ... and one over [90, 104) would give 0, but it does not reach over the centerpoint 105: no such pair is valid for a deletion, and
    # the flag is the front end's to raise, with both ordinals
    assert F.estimate_insert_size(rec(104, [("M", 10)]), rec(90, [("M", 14)])) == 0
    bad = F.IndelObs(o.obs, 0, 10, 16, abi.FRAGPILEUP_INDEL_NONPOSITIVE_ISIZE)
    with pytest.raises(F.NonPositiveInsertSize, match="records 3 and 9"):
        F.indel_table_of([bad], d, ic.PROPS, ic.IPROPS, fragments.basecalls.TABLES)


def test_isize_support():
    ip = F.IndelProps((300.0, 10.0), None, None, None)
    pr, pa = F.isize_support(300, 50, ip)
    assert pr > pa and math.isfinite(pr)
    pr, pa = F.isize_support(350, 50, ip)
    assert pa > pr
    assert F.isize_support(350, 50, ip)[1] == F.isize_support(300, 50, ip)[0]     # the same pmf, shifted
    # the ref pmf underflows (100 sd away) and the value is not within one sd of the alt mean: unreliable, ln 1 twice
    assert F.isize_support(1300, 500, ip) == (0.0, 0.0)
    # ... but within one sd of the alt mean the ln 0 stays
    pr, pa = F.isize_support(1300, 1000, ip)
    assert pr == -math.inf and math.isfinite(pa)
    # the other side: the alt pmf underflows; away from the ref mean by more than one sd -> unreliable; within one sd -> kept
    assert F.isize_support(420, 2000, ip) == (0.0, 0.0)
    pr, pa = F.isize_support(305, 2000, ip)
    assert pa == -math.inf and math.isfinite(pr)
    with pytest.raises(F.UnrealisticIsizeSd):
        F.isize_support(300, 5, F.IndelProps((300.0, 0.0), None, None, None))


def test_prob_sample_alt_by_hand():
    d = deletion(100, 10)
    # enclosable within max_del_cigar_len: every base feasible -> ln 1
    assert F.prob_sample_alt_read(d, 100, F.IndelProps(None, 10, None, 0.1)) == 0.0
    # longer than the longest D: the soft-clip arm, int(100 * 0.06) = 6 of min(10, 100) placements
    assert F.prob_sample_alt_read(d, 100, F.IndelProps(None, 9, None, 0.06)) == math.log(6) - math.log(10)
    # no maximum and no soft clip: ln 1
    assert F.prob_sample_alt_read(d, 100, F.IndelProps(None, None, None, None)) == 0.0
    # an insertion reads max_ins_cigar_len
    assert F.prob_sample_alt_read(insertion(5, 10), 100, F.IndelProps(None, 50, 9, 0.06)) == math.log(6) - math.log(10)
    # a pair without an insert size: 1 - (1 - a)(1 - b)
    ip = F.IndelProps(None, 9, None, 0.06)
    a, b = 0.6, 0.3            # int(50 * 0.06) = 3 of 10
    assert F.prob_sample_alt(d, 100, 50, ip) == pytest.approx(math.log(1 - (1 - a) * (1 - b)), abs=1e-12)
    assert F.prob_sample_alt(d, 100, None, ip) == math.log(6) - math.log(10)


def test_expected_prob_sample_alt_against_a_brute_force_sum():
    ip = F.IndelProps((300.0, 10.0), 5, None, 0.1)
    prev = 0.0
    for length in (1, 5, 6, 40, 120):
        d = deletion(1000, length)
        got = F.prob_sample_alt(d, 100, 100, ip)
        lf = 100 if length <= 5 else 10
        total = 0.0
        for x in range(240, 360):
            inner = max(x - 200, 0)
            bad_alt = 2 * (100 - lf) + inner + 1
            bad_ref = max(inner + 1 - length, 0)
            if x > bad_alt and x > bad_ref:
                total += math.exp(F.isize_pmf(x, 300.0, 10.0)) * (x - bad_alt) / (x - bad_ref)
        assert got == pytest.approx(math.log(total), abs=1e-9) and got <= 0.0 and got <= prev + 1e-12
        prev = got


def test_running_maxima_cross_the_feasible_bases_boundary():
    # the second candidate is 8 bases long; the properties start with max_del_cigar_len = 4; a member of the first candidate carries 8D
    ip = F.IndelProps(None, 4, None, 0.1)
    d = deletion(500, 8)
    assert F.feasible_bases(d, 100, ip) == 10
    ip2 = F.raised(ip, 8, 0, (0, 0))
    assert ip2.max_del_cigar_len == 8 and F.feasible_bases(d, 100, ip2) == 100
    # only what is already Some rises; the soft-clip fraction rises as a fraction
    assert F.raised(F.IndelProps(None, None, None, None), 8, 3, (5, 50)).key() == (None, None, None, None)
    assert F.raised(ip, 0, 0, (30, 100)).frac_max_softclip == 0.3
    assert F.clip_frac_greater((1, 2), (2, 5)) and not F.clip_frac_greater((1, 2), (2, 4)) and F.clip_frac_greater((2, 4), (1, 2))


# ---------------------------------------------------------------------------------------------- the header's text under the sanitizers
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return host_program.build(tmp_path_factory, "vlr_fragpileup_host")


def run_program(program, tmp, contigs, sites, records, props, has_isize, spec, evidences):
    paths = [os.path.join(str(tmp), n) for n in ("iin.bin", "iout.bin")]
    with open(paths[0], "wb") as f:
        f.write(ic.pack_host_input(contigs, sites, records, props, has_isize, spec, evidences))
    r = subprocess.run([program] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    return ic.unpack_host_output(open(paths[1], "rb").read(), len(sites))


def evidence_keys(evs):
    return [e.key() for e in evs]


def hit_keys(arr):
    return [(int(h["locus"]), int(h["record"]), int(h["status"]), (int(h["read_begin"]), int(h["read_begin"]) + int(h["read_len"])),
             (int(h["ref_begin"]), int(h["ref_begin"]) + int(h["ref_len"])), int(h["flag"]), int(h["mapq"])) for h in arr]


def same_as_restatement(oracle, program, tmp, contigs, sites, records, props, has_isize, spec=fragments.RealignSpec()):
    bam, _ = bc.write_case(tmp, "icase", contigs, records)
    rs = F.restate_indel(read_bam(bam)[1], sites, props, has_isize, spec, {0: list(contigs.values())[0].upper()})
    obs, obx, loc, lox, hits, windows = run_program(program, tmp, contigs, sites, records, props, has_isize, spec, rs.evidences)
    assert hit_keys(hits) == evidence_keys(rs.evidences) and not hits["pad"].any()
    assert windows == b"".join(e.ev.ref_allele + e.alt_allele + e.ev.read_window + e.ev.quals for e in rs.evidences)
    ic.assert_same(obs, obx, loc, lox, rs)
    return obs, obx, hits, rs


def test_host_program_equals_restatement(oracle, program, tmp_path):
    ref = ic.contig()
    _, sites = ic.sites_of(ref)
    for has_isize in (True, False):
        obs, obx, hits, rs = same_as_restatement(oracle, program, tmp_path, {"i1": ref}, sites, ic.pairs(ref, 90), ic.PROPS, has_isize)
        assert len(obs) > 40 and len(hits) == sum(rs.n_members)
        assert bool((obx["insert_size"] > 0).any()) == has_isize and (rs.maxima[0][0], rs.maxima[1][1]) == (ic.DEL_LEN, len(ic.INS_SEQ))
    # window edges: a deletion behind the first base and one that ends at the last base of the contig, an insertion at the last base
    n = len(ref)
    cands = [("i1", 0, ref[0:4], ref[0:1]), ("i1", n - 5, ref[n - 5:n], ref[n - 5:n - 4]), ("i1", n - 1, ref[n - 1:n], ref[n - 1:n] + b"AC")]
    _, edge = ic.sites_of(ref, cands=cands)
    recs = [bc.make_read(ref, 0, [("M", 30)], name="first"), bc.make_read(ref, 0, [("M", 1), ("D", 3), ("M", 29)], name="first_alt"),
            bc.make_read(ref, n - 30, [("M", 30)], name="last", flag=0x10), bc.make_read(ref, n - 1, [("M", 1)], name="one_base")]
    obs, obx, hits, rs = same_as_restatement(oracle, program, tmp_path, {"i1": ref}, edge, recs, fragments.Props(50, 60, 30), True)
    assert len(hits) == sum(rs.n_members) >= 5


def test_command_refuses_without_the_flag_and_writes_with_it(oracle, tmp_path):
    ref = ic.contig()
    cands, _ = ic.sites_of(ref)
    bam, fa = bc.write_case(tmp_path, "cmd", {"i1": ref}, ic.pairs(ref, 60))
    vcf = os.path.join(str(tmp_path), "c.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for c, pos, r, a in cands:
            f.write("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (c, pos + 1, r.decode(), a.decode()))
    props = os.path.join(str(tmp_path), "p.json")
    import json
    json.dump({"insert_size": {"mean": 130.0, "sd": 12.0}, "max_del_cigar_len": 4, "max_ins_cigar_len": 4, "frac_max_softclip": 0.1, "max_read_len": ic.READ,
               "max_mapq": 60}, open(props, "w"))
    out = os.path.join(str(tmp_path), "o.bcf")
    with pytest.raises(F.PreprocessError, match="is not an SNV or MNV: indel, structural and breakend candidates are not built"):
        F.preprocess_variants(fa, vcf, bam, out, props, "cpu", True)
    assert not os.path.exists(out)
    tabs = F.observations(bam, fa, cands, json.load(open(props)), device="cpu", indel_candidates=F.RealignSpec())
    assert [len(t) > 10 for t in tabs] == [True, True] and all((t.prob_sample_alt <= 0).all() for t in tabs)
    # the deletion pairs carry the insert-size term: prob_sample_alt of a pair is the expectation over the insert sizes, below ln 1
    assert (tabs[0].prob_sample_alt < 0).any()


def command_case(tmp_path, extra=()):
    """(fasta, vcf, bam, properties path, candidates) of the synthetic pairs with the deletion, the insertion and `extra` VCF rows"""
    import json
    ref = ic.contig()
    cands, _ = ic.sites_of(ref)
    bam, fa = bc.write_case(tmp_path, "cmd2", {"i1": ref}, ic.pairs(ref, 60))
    vcf, props = os.path.join(str(tmp_path), "c2.vcf"), os.path.join(str(tmp_path), "p2.json")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=i1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for c, pos, r, a in list(cands) + list(extra):
            f.write("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (c, pos + 1, r.decode(), a.decode()))
    json.dump({"insert_size": {"mean": 130.0, "sd": 12.0}, "max_del_cigar_len": 4, "max_ins_cigar_len": 4, "frac_max_softclip": 0.1, "max_read_len": ic.READ,
               "max_mapq": 60}, open(props, "w"))
    return ref, fa, vcf, bam, props, cands


def test_command_writes_a_file_that_round_trips(oracle, tmp_path):
    """preprocess_variants with indel candidates on the CPU path: the written BCF read back through ingest carries, per candidate, the
    observations of the restatement, the indel variant class, no ref / alt base, and prob_sample_alt"""
    import json
    from varlociraptor_amd import ingest
    ref, fa, vcf, bam, props, cands = command_case(tmp_path, extra=[("i1", 60, ref_base(60), other_base(60))])
    out = os.path.join(str(tmp_path), "o2.bcf")
    assert F.preprocess_variants(fa, vcf, bam, out, props, "cpu", True, score_indel_reads_from_alignment=True, indel_candidates=F.RealignSpec()) == 3
    batch, _ = ingest.read_observations([out])
    snv = ("i1", 60, ref_base(60), other_base(60))
    pj = json.load(open(props))
    want = F.observations(bam, fa, list(cands) + [snv], pj, device="cpu", indel_candidates=F.RealignSpec())
    off = batch.obs_offset
    assert batch.n_loci == 3 and [int(off[k + 1] - off[k]) for k in range(3)] == [len(t) for t in want] and len(want[0]) > 10 and len(want[2]) > 3
    assert list(batch.locus["variant_type"]) == [abi.VT_INDEL, abi.VT_INDEL, abi.VT_SNV]
    assert list(batch.locus["ref_base"][:2]) == [0, 0] and list(batch.locus["alt_base"][:2]) == [0, 0]
    for k, t in enumerate(want):
        sl = slice(int(off[k]), int(off[k + 1]))
        for col, arr in (("prob_sample_alt", t.prob_sample_alt if t.prob_sample_alt is not None else 0.0 * t.prob_alt), ("prob_alt", t.prob_alt), ("prob_ref", t.prob_ref)):
            a, b = batch.columns[col][sl].astype(float), arr.astype("float32").astype(float)
            fin = (a > -1e30) & (b > -1e30)          # (ln 0 has its own encoding in the file)
            # the observation format keeps a probability as a half-precision float where that loses little (11 significant bits)
            assert (fin == (b > -1e30)).all() and (abs(a[fin] - b[fin]) <= 2.0 ** -10 * np.maximum(1.0, abs(b[fin]))).all(), (k, col)
    # the SNV record of the mixed file is what today's path writes for it alone
    alone = F.observations(bam, fa, [snv], pj, device="cpu")[0]
    assert (alone.prob_alt == want[2].prob_alt).all() and (alone.prob_ref == want[2].prob_ref).all() and alone.records == want[2].records
    pb, _ = F.pileup(want, list(cands) + [snv])
    strand_altlocus = abi.BIAS_STRAND | abi.BIAS_ALTLOCUS
    assert list(pb.locus["locus_flags"][:2]) == [strand_altlocus, strand_altlocus] and pb.locus["locus_flags"][2] & abi.LOCUS_HAS_SNV


def ref_base(pos):
    return ic.contig()[pos:pos + 1]


def other_base(pos):
    return b"A" if ref_base(pos) != b"A" else b"C"


def test_command_refusals_name_the_candidate(oracle, tmp_path):
    ref = ic.contig()
    spec = F.RealignSpec()

    def run(extra, window=None):
        _, fa, vcf, bam, props, _ = command_case(tmp_path, extra=extra)
        if window is not None:
            import json
            pj = json.load(open(props))
            pj["insert_size"] = {"mean": float(window), "sd": 0.5}
            json.dump(pj, open(props, "w"))
        out = os.path.join(str(tmp_path), "r.bcf")
        try:
            return F.preprocess_variants(fa, vcf, bam, out, props, "cpu", True, score_indel_reads_from_alignment=True, indel_candidates=spec)
        finally:
            assert not os.path.exists(out)
    with pytest.raises(F.PreprocessError, match=r"i1:301 %s>GG is a replacement" % ref[300:303].decode()):
        run([("i1", 300, ref[300:303], b"GG")])
    with pytest.raises(F.PreprocessError, match=r"i1:301 .><DEL> is a symbolic or breakend allele"):
        run([("i1", 300, ref[300:301], b"<DEL>")])
    with pytest.raises(F.PreprocessError, match=r"i1:301 .>.\[i1:350\[ is a symbolic or breakend allele"):
        run([("i1", 300, ref[300:301], ref[300:301] + b"[i1:350[")])
    # a deletion of 120 bases with a window of 20 + 6 * 0.5 = 23: centerpoint 60 > 2 * 23 + 1, the fetches do not merge
    with pytest.raises(F.PreprocessError, match=r"i1:201 .* do not merge into one fetch with a window of 23"):
        run([("i1", 200, ref[200:321], ref[200:201])], window=20)
    # the length limit of a session
    big = ic.contig(6000, 2)
    n = abi.FRAGPILEUP_MAX_INDEL_LEN
    assert F.indel_site(big, 0, 100, big[100:101 + n], big[100:101], 64, "x").length == n
    with pytest.raises(F.PreprocessError, match="candidate big:101 .* of 4097 bases is longer than the 4096"):
        F.indel_site(big, 0, 100, big[100:102 + n], big[100:101], 64, "big:101 del")
    with pytest.raises(F.PreprocessError, match="of 4097 bases is longer"):
        F.indel_site(big, 0, 100, big[100:101], big[100:101] + b"A" * (n + 1), 64, "big:101 ins")


ISSUE_154 = lambda vafs, ph: vafs["normal"] == 0.0 and 0.15 < vafs["tumor"] < 0.25 and ph["PROB_ARTIFACT"] == math.inf and ph["PROB_SOMATIC_TUMOR"] < 0.08


@pytest.mark.parametrize("name", sorted(ic.indels_rows()))
def test_reference_testcases_meet_their_recorded_rows(oracle, name):
    """tests/golden/bam/INDELS.md (tools/make_indel_fragment_fixtures.py): the restatement -> pileup -> oracle gives the recorded number of
    fragment observations and MAP VAFs; a row marked met meets the testcase's `expected:` block (bam_pairs.BAM_CASES restates the blocks
    of the three cases that were already fixtures, ISSUE_154 that of the two-sample case — a deletion without an insert size in the
    properties, each sample preprocessed on its own; test_giab_08 has an empty block); a refused row is refused, with its reason."""
    import sys
    import bam_pairs as bp
    sys.path.insert(0, os.path.join(host_program.ROOT, "tools"))
    import make_indel_fragment_fixtures as tool
    row = ic.indels_rows()[name]
    if row is None:
        with pytest.raises(F.RealignStrandInfo, match="record 0 carries an SI:Z tag"):
            tool.call_case(name)
        return
    _, got = tool.call_case(name)
    n, vafs, phred = got["fragment"]
    assert n == row[0] and tool.vaf_text(vafs) == row[1] and row[2]
    assert got["read"][0] >= n
    if name in bp.BAM_CASES:
        assert got["read"][0] > n                 # paired reads: a pair is one observation, not two
        assert bp.BAM_CASES[name]["expected"](list(vafs.values())[0], phred)
    if name == "issue_154":
        assert ISSUE_154(vafs, phred)
