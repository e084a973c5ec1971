"""Deletion and insertion candidates in the fragment session on the device (vlr_fragpileup_open_indel, csrc/vlr_fragpileup.hip) against
the restatement of varlociraptor_amd/fragments.py: integer columns, strands, flags, insert sizes and per-locus maxima with ==, the raw
scores and distances of every evidence with == against the same windows sent through realign.best_hits / prob_related* (the
restatement scored on the device), finished supports within 1e-9 of the restatement scored on the CPU.  Every test
here needs the entry point and the flag, which the parent commit does not have."""
import os

import numpy as np
import pytest

import basecall_cases as bc
import fragindel_cases as ic
from varlociraptor_amd import abi, engine, fragments
from varlociraptor_amd.readwindows import read_bam

pytestmark = pytest.mark.gpu
F = fragments
TOL = 1e-9


def device(bams, sites, props=ic.PROPS, has_isize=True, spec=F.RealignSpec(), fa=None, **kw):
    return F.device_indel_observations(bams, sites, props, has_isize, spec, fa, 0, **kw)


def restated(bams, contigs, sites, props, has_isize, spec, dev):
    recs = [r for b in ([bams] if isinstance(bams, str) else bams) for r in read_bam(b)[1]]
    return F.restate_indel(recs, sites, props, has_isize, spec, {0: list(contigs.values())[0].upper()}, dev)


def hit_keys(arr):
    return [(int(h["locus"]), int(h["record"]), int(h["status"]), (int(h["read_begin"]), int(h["read_begin"]) + int(h["read_len"])),
             (int(h["ref_begin"]), int(h["ref_begin"]) + int(h["ref_len"])), int(h["flag"]), int(h["mapq"])) for h in arr]


def same(tmp, name, contigs, sites, records, props=ic.PROPS, has_isize=True, spec=F.RealignSpec(), **kw):
    bam, fa = bc.write_case(tmp, name, contigs, records)
    obs, obx, loc, lox, res, ev, rres = device(bam, sites, props, has_isize, spec, fa, **kw)
    assert res.status == 0, res.status
    on_dev = restated(bam, contigs, sites, props, has_isize, spec, 0)
    assert hit_keys(ev) == [e.key() for e in on_dev.evidences] and not ev["pad"].any()
    # raw scores and distances: the same windows through the same kernels
    assert [(float(h["ln_ref"]), float(h["ln_alt"]), int(h["dist_ref"]), int(h["dist_alt"])) for h in ev] == \
        [(e.ln_ref, e.ln_alt, e.dist_ref, e.dist_alt) for e in on_dev.evidences]
    ic.assert_same(obs, obx, loc, lox, on_dev)                                       # the same normalisation on both sides: ==
    return obs, obx, loc, lox, ev, bam, fa


@pytest.fixture(scope="module")
def case():
    ref = ic.contig()
    return ref, ic.sites_of(ref)[1], ic.pairs(ref, 120)


@pytest.mark.parametrize("mode", ["exact", "fast", "homopolymer"])
def test_device_equals_restatement(oracle, tmp_path, case, mode):
    ref, sites, recs = case
    spec = F.RealignSpec(64, mode)
    obs, obx, loc, lox, ev, bam, fa = same(tmp_path, "m_" + mode, {"i1": ref}, sites, recs, spec=spec)
    assert len(obs) > 60 and (obx["insert_size"] > 0).any() and len(ev) == int(loc["n_members"].sum())
    # the CPU pair HMMs of the mode: finished supports within the project's bound for this comparison
    on_cpu = restated(bam, {"i1": ref}, sites, ic.PROPS, True, spec, "cpu")
    ic.assert_same(obs, obx, loc, lox, on_cpu, TOL)
    if mode == "exact":
        # without an insert size in the properties no pair carries one and more pairs are valid
        o2, x2, l2, _, _, _, _ = same(tmp_path, "noisz", {"i1": ref}, sites, recs, has_isize=False)
        assert not x2["insert_size"].any() and int(l2["n_obs"][0]) >= int(loc["n_obs"][0])


def test_host_side_terms_agree(oracle, tmp_path, case):
    ref, sites, recs = case
    bam, fa = bc.write_case(tmp_path, "terms", {"i1": ref}, recs)
    cands, _ = ic.sites_of(ref)
    pj = {"insert_size": {"mean": 130.0, "sd": 12.0}, "max_del_cigar_len": 4, "max_ins_cigar_len": 4, "frac_max_softclip": 0.1, "max_read_len": ic.READ, "max_mapq": 60}
    dev = F.observations(bam, fa, cands, pj, device=0, indel_candidates=F.RealignSpec())
    cpu = F.observations(bam, fa, cands, pj, device="cpu", indel_candidates=F.RealignSpec())
    for d, c in zip(dev, cpu):
        assert len(d) == len(c) > 10 and d.records == c.records
        assert (d.prob_sample_alt == c.prob_sample_alt).all() and (d.prob_hit_base == c.prob_hit_base).all() and (d.strand == c.strand).all()
        assert np.abs(d.prob_ref - c.prob_ref).max() <= TOL and np.abs(d.prob_alt - c.prob_alt).max() <= TOL


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257])
def test_member_counts_at_wave_and_workgroup_edges(oracle, tmp_path, n):
    ref = ic.contig()
    _, sites = ic.sites_of(ref)
    rng = np.random.RandomState(n)
    recs = []
    for k in range(n):      # single reads and pairs that start in front of the deletion's end, sorted by start
        p = int(rng.randint(100, 150))
        recs.append((p, k, ic.read_at(ref, p, "w%04d" % (k // 2 if k % 5 else 5000 + k), bool(k & 1), flag=0x10 if k % 3 == 0 else 0)))
    recs.sort(key=lambda x: (x[0], x[1]))
    obs, obx, loc, lox, ev, _, _ = same(tmp_path, "n%d" % n, {"i1": ref}, sites[:1], [r for _, _, r in recs])
    assert int(loc["n_members"][0]) == n == len(ev)


def test_a_name_with_three_records_replaces_right_twice(oracle, tmp_path):
    """mod.rs:325-338: the first record of a name is `left`, every later one replaces `right`: of three records the pair is (first, third).
    With an insert size the pair (100, 112) would not reach over the centerpoint 153; (100, 140) does."""
    ref = ic.contig()
    _, sites = ic.sites_of(ref)
    recs = [ic.read_at(ref, 100, "tri", False, flag=0x41, mtid=0, mpos=140), ic.read_at(ref, 112, "tri", False, flag=0x811, mtid=0, mpos=100),
            ic.read_at(ref, 140, "tri", False, flag=0x91, mtid=0, mpos=100), ic.read_at(ref, 130, "other", True)]
    obs, obx, loc, lox, ev, _, _ = same(tmp_path, "tri", {"i1": ref}, sites[:1], recs)
    assert int(loc["n_members"][0]) == 4 and len(ev) == 4
    # file order: ordinals 0, 1, 2 carry the name `tri`; the pair is (0, 2) = [100, 140) + [140, 180): it reaches over the centerpoint,
    # the right read overlaps [150, 156) and, being the reference over the deletion, carries a strand; insert size 180 - 100
    pairs = [(int(o["left"]), int(o["right"])) for o in obs if int(o["right"]) != abi.FRAGPILEUP_NO_RECORD]
    assert pairs == [(0, 2)]
    k = [int(o["left"]) for o in obs].index(0)
    assert int(obx["insert_size"][k]) == 80 and (int(obx["len_left"][k]), int(obx["len_right"][k])) == (ic.READ, ic.READ) and int(obs["strand"][k]) == abi.STRAND_REVERSE


@pytest.mark.parametrize("n", [4096, 4097])
def test_deepest_locus_and_the_fallback(oracle, tmp_path, n):
    """VLR_FRAGPILEUP_MAX_MEMBERS members are formed on the device; one more flags the locus, and the front end finishes it with the
    restatement (scored on the device): the tables equal those of the CPU path within the bound either way"""
    ref = ic.contig()
    cands, sites = ic.sites_of(ref)
    recs = sorted(((100 + k % 50, k, ic.read_at(ref, 100 + k % 50, "d%05d" % k, bool(k & 1), flag=0x10 if k % 3 == 0 else 0)) for k in range(n)), key=lambda x: x[:2])
    bam, fa = bc.write_case(tmp_path, "deep%d" % n, {"i1": ref}, [r for _, _, r in recs])
    _, _, loc, _, res, _, _ = device(bam, sites[:1], fa=fa)
    deep = n > abi.FRAGPILEUP_MAX_MEMBERS
    assert int(loc["n_members"][0]) == n and bool(loc["status"][0] & abi.FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS) == deep and (int(loc["n_obs"][0]) == 0) == deep
    pj = {"insert_size": {"mean": 130.0, "sd": 12.0}, "max_del_cigar_len": 4, "max_ins_cigar_len": 4, "frac_max_softclip": 0.1, "max_read_len": ic.READ, "max_mapq": 60}
    dev, = F.observations(bam, fa, cands[:1], pj, device=0, indel_candidates=F.RealignSpec(64, "fast"))
    cpu, = F.observations(bam, fa, cands[:1], pj, device="cpu", indel_candidates=F.RealignSpec(64, "fast"))
    assert len(dev) == len(cpu) > 1000 and dev.records == cpu.records and (dev.prob_sample_alt == cpu.prob_sample_alt).all()
    assert np.abs(dev.prob_ref - cpu.prob_ref).max() <= TOL and np.abs(dev.prob_alt - cpu.prob_alt).max() <= TOL


def test_contig_edges_one_base_window_and_two_loci(oracle, tmp_path):
    ref = ic.contig()
    n = len(ref)
    cands = [("i1", 0, ref[0:4], ref[0:1]), ("i1", 1, ref[1:2], ref[1:2] + b"GG"), ("i1", n - 5, ref[n - 5:n], ref[n - 5:n - 4]),
             ("i1", n - 1, ref[n - 1:n], ref[n - 1:n] + b"AC")]
    _, sites = ic.sites_of(ref, cands=cands)
    recs = [bc.make_read(ref, 0, [("M", 30)], name="first"), bc.make_read(ref, 0, [("M", 1), ("D", 3), ("M", 29)], name="first_alt"),
            bc.make_read(ref, n - 30, [("M", 30)], name="last", flag=0x10), bc.make_read(ref, n - 1, [("M", 1)], name="one_base")]
    obs, obx, loc, lox, ev, _, _ = same(tmp_path, "edges", {"i1": ref}, sites, recs, props=F.Props(50, 60, 30))
    # `first` and `first_alt` are members of the deletion at 0 and of the insertion at 1; the deletion [n - 5, n - 1) has `last` alone
    # (`one_base` starts at n - 1, its end), the insertion at n - 1 both; `one_base` has a read window of one base
    assert [int(x) for x in loc["n_members"]] == [2, 2, 1, 2] and 1 in [int(x) for x in ev["read_len"]]
    # a read of 128 bases over --indel-window 64: the MAX_PATTERN_LEN trim
    big = ic.contig(600, 9)
    c2 = [("i1", 300, big[300:304], big[300:301])]
    _, s2 = ic.sites_of(big, cands=c2)
    rec = bc.make_read(big, 230, [("M", 140)], name="long")
    _, _, _, _, ev2, _, _ = same(tmp_path, "long", {"i1": big}, s2, [rec], props=F.Props(300, 60, 140))
    assert int(ev2["read_len"][0]) == 128


def test_determinism_and_capacities(oracle, tmp_path, case):
    ref, sites, recs = case
    bam, fa = bc.write_case(tmp_path, "det", {"i1": ref}, recs)
    base = device(bam, sites, fa=fa)
    half = len(recs) // 2
    b1, _ = bc.write_case(tmp_path, "det_a", {"i1": ref}, recs[:half])
    b2, _ = bc.write_case(tmp_path, "det_b", {"i1": ref}, recs[half:])
    for other in (device(bam, sites, fa=fa, window_bytes=4096), device(bam, sites, fa=fa, window_bytes=1 << 20), device([b1, b2], sites, fa=fa),
                  device(bam, sites, fa=fa, pair_byte_limit=2000)):
        for k in (0, 1, 2, 3, 5):
            assert base[k].tobytes() == other[k].tobytes(), k
    assert device(bam, sites, fa=fa, pair_byte_limit=2000)[6].n_ranges > 1
    need = int(base[6].needed_evidences)
    _, _, _, _, res, _, rres = device(bam, sites, fa=fa, evidence_capacity=need - 1, retry=False)
    assert res.status == abi.FRAGPILEUP_EVIDENCE_OVERFLOW and int(rres.needed_evidences) == need and res.n_obs == 0
    again = device(bam, sites, fa=fa, evidence_capacity=need, retry=False)
    assert again[4].status == 0 and again[0].tobytes() == base[0].tobytes()


def test_member_name_and_key_capacities_at_the_edge(oracle, tmp_path, case):
    """The Side records of an indel session are sized by the member capacity, the names and the alt-locus keys by theirs: each of the
    three one short of what the input needs is reported as that overflow alone (no guard word behind a buffer changed) with the needed
    sizes counted on; all three exactly at need, and all three at 1 with the retry, give what a roomy session gives.  (The records of
    `case` carry no XA tag, so two that do stand in front of them: a key capacity of need - 1 = -1 would be a refused argument.  The
    counts are compared field by field without their `seconds`, which are timers.)"""
    from varlociraptor_amd import alignprops
    ref, sites, recs = case
    xa = [ic.read_at(ref, 40, "xa%d" % k, False, aux=alignprops.aux_field("XA", "Z", "i2,+%d,40M,0;i3,-77,40M,1;" % (100 + k))) for k in range(2)]
    bam, fa = bc.write_case(tmp_path, "caps", {"i1": ref}, xa + recs)        # (the reads of `case` start at 40 or behind it: still sorted)
    roomy = device(bam, sites, fa=fa)
    need = {"member_capacity": int(roomy[4].needed_members), "name_capacity": int(roomy[4].needed_name_bytes), "key_capacity": int(roomy[4].needed_keys)}
    n_ev = int(roomy[6].needed_evidences)
    assert roomy[4].status == 0 and min(need.values()) > 0 and len(roomy[0]) > 60

    def fields(c):
        return [(f, getattr(c, f)) for f, _ in c._fields_ if f != "seconds"]

    def assert_equals_roomy(got):
        for k in (0, 1, 2, 3, 5):
            assert got[k].dtype == roomy[k].dtype and got[k].tobytes() == roomy[k].tobytes(), k
        assert fields(got[4]) == fields(roomy[4]) and fields(got[6]) == fields(roomy[6])
    for cap, bit in (("member_capacity", abi.FRAGPILEUP_MEMBER_OVERFLOW), ("name_capacity", abi.FRAGPILEUP_NAME_OVERFLOW), ("key_capacity", abi.FRAGPILEUP_KEY_OVERFLOW)):
        res = device(bam, sites, fa=fa, evidence_capacity=n_ev, retry=False, **dict(need, **{cap: need[cap] - 1}))[4]
        print(cap, need[cap] - 1, "status", res.status)
        assert res.status == bit and not res.status & abi.FRAGPILEUP_GUARD_DAMAGED, (cap, res.status)
        assert (int(res.needed_members), int(res.needed_name_bytes), int(res.needed_keys)) == tuple(need.values()), cap
    assert_equals_roomy(device(bam, sites, fa=fa, evidence_capacity=n_ev, retry=False, **need))
    assert_equals_roomy(device(bam, sites, fa=fa, member_capacity=1, name_capacity=1, key_capacity=1))


def test_refusals(oracle, tmp_path):
    ref = ic.contig(6000, 2)
    ok = [("i1", 100, ref[100:100 + abi.FRAGPILEUP_MAX_INDEL_LEN + 1], ref[100:101])]
    _, sites = ic.sites_of(ref, cands=ok)
    rec = bc.make_read(ref, 90, [("M", 40)], name="r")
    same(tmp_path, "longest", {"i1": ref}, sites, [rec], props=F.Props(5000, 60, 40))          # the longest locus a session accepts
    _, over = ic.sites_of(ref, cands=[("i1", 100, ref[100:100 + abi.FRAGPILEUP_MAX_INDEL_LEN + 2], ref[100:101])])
    bam, fa = bc.write_case(tmp_path, "beyond", {"i1": ref}, [rec])
    with pytest.raises(engine.EngineError, match="longer than the 4096 bases"):
        device(bam, over, F.Props(5000, 60, 40), fa=fa)
    # a leading-N CIGAR and an SI:Z record are named by ordinal
    from varlociraptor_amd import alignprops
    small = ic.contig()
    cands, sites = ic.sites_of(small)
    recs = [bc.make_read(small, 120, [("M", 40)], name="plain"), bc.make_read(small, 126, [("N", 2), ("M", 38)], name="leading_N"),
            bc.make_read(small, 130, [("M", 40)], name="with_SI", aux=alignprops.aux_field("SI", "Z", "+" * 40))]
    bam, fa = bc.write_case(tmp_path, "refused", {"i1": small}, recs)
    pj = {"insert_size": None, "max_del_cigar_len": 4, "max_ins_cigar_len": 4, "frac_max_softclip": 0.1, "max_read_len": ic.READ, "max_mapq": 60}
    with pytest.raises(F.LeadingRefSkip, match="record 1"):
        F.observations(bam, fa, cands[:1], pj, device=0, indel_candidates=F.RealignSpec())
    bam, fa = bc.write_case(tmp_path, "refused2", {"i1": small}, [recs[0], recs[2]])
    with pytest.raises(F.RealignStrandInfo, match="record 1"):
        F.observations(bam, fa, cands[:1], pj, device=0, indel_candidates=F.RealignSpec())


def test_command_on_the_device(oracle, tmp_path, case):
    import json
    from varlociraptor_amd import cli, ingest
    ref, sites, recs = case
    cands, _ = ic.sites_of(ref)
    bam, fa = bc.write_case(tmp_path, "cmd", {"i1": ref}, recs)
    vcf, props, out = (os.path.join(str(tmp_path), n) for n in ("c.vcf", "p.json", "o.bcf"))
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n##contig=<ID=i1>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        f.write("i1\t61\t.\t%s\t%s\t.\t.\t.\n" % (chr(ref[60]), "A" if ref[60] != 65 else "C"))
        for c, pos, r, a in cands:
            f.write("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (c, pos + 1, r.decode(), a.decode()))
    json.dump({"insert_size": {"mean": 130.0, "sd": 12.0}, "max_del_cigar_len": 4, "max_ins_cigar_len": 4, "frac_max_softclip": 0.1, "max_read_len": ic.READ,
               "max_mapq": 60}, open(props, "w"))
    args = ["preprocess", "variants", fa, "--candidates", vcf, "--bam", bam, "--alignment-properties", props, "--atomic-candidate-variants", "--output", out]
    with pytest.raises(SystemExit):
        cli.main(args)                                   # without the flag: today's refusal, no file
    assert not os.path.exists(out)
    cli.main(args + ["--indel-candidates", "--realign-indel-reads", "--pairhmm-mode", "fast"])
    batch, _ = ingest.read_observations([out])
    pj = json.load(open(props))
    snv = ("i1", 60, ref[60:61], b"A" if ref[60:61] != b"A" else b"C")
    spec = F.RealignSpec(64, "fast", *F.gap_hop_of(pj))
    want = F.observations(bam, fa, [snv] + list(cands), pj, device=0, realign_indel_reads=True, realign=spec, indel_candidates=spec)
    cpu = F.observations(bam, fa, [snv] + list(cands), pj, device="cpu", realign_indel_reads=True, realign=spec, indel_candidates=spec)
    today, = F.observations(bam, fa, [snv], pj, device=0, realign_indel_reads=True, realign=spec)       # the SNV alone, through today's session
    assert (today.prob_alt == want[0].prob_alt).all() and (today.prob_ref == want[0].prob_ref).all() and today.records == want[0].records and len(today) > 3
    off = batch.obs_offset
    assert batch.n_loci == 3 and [int(off[k + 1] - off[k]) for k in range(3)] == [len(t) for t in want]
    assert list(batch.locus["variant_type"]) == [abi.VT_SNV, abi.VT_INDEL, abi.VT_INDEL] and list(batch.locus["ref_base"][1:]) == [0, 0]
    for k, (t, c) in enumerate(zip(want, cpu)):
        assert t.records == c.records and np.abs(t.prob_alt - c.prob_alt).max() <= TOL and np.abs(t.prob_ref - c.prob_ref).max() <= TOL
        sl = slice(int(off[k]), int(off[k + 1]))
        psa = t.prob_sample_alt if t.prob_sample_alt is not None else np.zeros(len(t))
        for col, arr in (("prob_sample_alt", psa), ("prob_alt", t.prob_alt), ("prob_ref", t.prob_ref), ("prob_mapping", t.prob_mapping)):
            a, b = batch.columns[col][sl].astype(float), arr.astype("float32").astype(float)
            fin = b > -1e30
            # the observation format keeps a probability as a half-precision float where that loses little (11 significant bits)
            assert ((a > -1e30) == fin).all() and (abs(a[fin] - b[fin]) <= 2.0 ** -10 * np.maximum(1.0, abs(b[fin]))).all(), (k, col)
    assert (want[1].prob_sample_alt < 0).any()


@pytest.mark.parametrize("name", sorted(ic.indels_rows()))
def test_command_on_the_device_for_the_recorded_testcases(oracle, golden_dir, tmp_path, name):
    """every row of tests/golden/bam/INDELS.md through `preprocess variants --indel-candidates` on the device, every sample of a case on
    its own with its own properties: the written observations are those of the device tables, which equal the CPU restatement's within
    the bound; the call from them gives the recorded MAP VAFs and meets the `expected:` block of a row marked met; the refused row is
    refused by the command, no file written"""
    import sys
    import bam_pairs as bp
    from test_fragment_indel_host import ISSUE_154
    from varlociraptor_amd import alignprops, cli, ingest, readwindows
    sys.path.insert(0, os.path.join(os.path.dirname(golden_dir), "..", "tools"))
    import make_indel_fragment_fixtures as tool
    row = ic.indels_rows()[name]
    d = os.path.join(golden_dir, "bam", name)
    rec, cand = tool.candidate_of(d)
    fa = os.path.join(str(tmp_path), "ref.fa")                       # (the fixtures hold their reference without an index)
    alignprops.write_fasta(fa, readwindows.read_fasta(os.path.join(d, "ref.fa")))
    vcf = os.path.join(str(tmp_path), "c.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n%s\t%s\t.\t%s\t%s\t.\t.\t.\n" % (rec[0], rec[1], rec[3], rec[4]))
    total = 0
    for sample, bam, pj in tool.samples_of(d):
        props = os.path.join(d, "properties.json" if sample is None else "properties.%s.json" % sample)
        out = os.path.join(str(tmp_path), "o.%s.bcf" % sample)
        args = ["preprocess", "variants", fa, "--candidates", vcf, "--bam", bam, "--alignment-properties", props, "--atomic-candidate-variants", "--output", out,
                "--indel-candidates"]
        if row is None:
            with pytest.raises(SystemExit):
                cli.main(args)
            assert not os.path.exists(out)
            return
        cli.main(args)
        batch, _ = ingest.read_observations([out])
        spec = tool.spec_of(pj)
        dev, = F.observations(bam, fa, cand, pj, device=0, indel_candidates=spec)
        cpu, = F.observations(bam, fa, cand, pj, device="cpu", indel_candidates=spec)
        assert batch.n_obs == len(dev) == len(cpu) > 0 and dev.records == cpu.records and (dev.prob_sample_alt == cpu.prob_sample_alt).all()
        assert np.abs(dev.prob_ref - cpu.prob_ref).max() <= TOL and np.abs(dev.prob_alt - cpu.prob_alt).max() <= TOL
        total += len(dev)
    _, got = tool.call_case(name, device=0, fasta=fa)
    n, vafs, phred = got["fragment"]
    assert n == total == row[0] and tool.vaf_text(vafs) == row[1] and row[2]
    if name in bp.BAM_CASES:
        assert bp.BAM_CASES[name]["expected"](list(vafs.values())[0], phred)
    if name == "issue_154":
        assert ISSUE_154(vafs, phred)
