"""Rates of the indel session of the fragment pass (vlr_fragpileup_open_indel, csrc/vlr_fragpileup.hip): records/s and evidences/s with
the seconds of each stage, on a synthetic coordinate-sorted paired BAM of a stated depth with a stated share of deletion / insertion
fragments, and on the deletion / insertion fixtures under tests/golden/bam/ (INDELS.md); against today's path for the same loci in
the same process — `readwindows.device_supports` (the per-read indel session) plus the pairing of its hits by QNAME in Python, which
is what a caller had to do for one observation per fragment — alternated run by run.  profiles/fragindel.md holds the figures.

    python tools/fragindel_rate.py --make DIR [--depth 30] [--loci 200] [--alt-share 0.3]     # writes DIR/indels.bam, DIR/indels.fa (no GPU)
    python tools/fragindel_rate.py --run DIR [--rounds 5] [--fixtures]                          # one JSON line per input

The BAM: pairs of 100-base reads (MAPQ 60, qualities 30) with inner distances of 50-250 bases at sorted positions of one contig; a
deletion of 1-12 bases or an insertion of 1-8 bases (of A) every 300 bases, alternating; `--alt-share` of the fragments come from
the alt haplotype: a read of theirs that spans a candidate with ten bases on either side carries the D / I operation.  `--depth` is
the mean number of reads over a base.  Every run after the first of a process is timed; the JSON gives the median and the range.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

READ = 100
SPACING = 300
PROPS = {"insert_size": {"mean": 350.0, "sd": 60.0}, "max_del_cigar_len": 12, "max_ins_cigar_len": 8, "frac_max_softclip": 0.1, "max_read_len": READ, "max_mapq": 60}


def candidates_of(ref, n_loci, rng):
    out = []
    for k in range(n_loci):
        pos = 500 + k * SPACING
        if k % 2 == 0:
            n = int(rng.integers(1, 13))
            out.append(("s1", pos, bytes(ref[pos:pos + n + 1]), bytes(ref[pos:pos + 1])))
        else:
            n = int(rng.integers(1, 9))
            out.append(("s1", pos, bytes(ref[pos:pos + 1]), bytes(ref[pos:pos + 1]) + b"A" * n))
    return out


def make(d, depth, n_loci, alt_share, seed=7):
    import basecall_cases as bc
    from varlociraptor_amd import alignprops
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    contig_len = 1000 + n_loci * SPACING
    ref = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), contig_len))
    cands = candidates_of(ref, n_loci, rng)
    n_pairs = depth * contig_len // (2 * READ)
    starts = np.sort(rng.integers(0, contig_len - 2 * READ - 260, n_pairs))
    recs = []
    for k, p in enumerate(starts):
        p = int(p)
        q = p + READ + int(rng.integers(50, 251))
        alt = rng.random() < alt_share
        name = "p%07d" % k
        for pos, flag, mpos in ((p, 0x63, q), (q, 0x93, p)):
            cigar = [("M", READ)]
            if alt:
                j = (pos - 500 + SPACING - 1) // SPACING          # the first candidate at or behind pos
                if 0 <= j < n_loci:
                    c = cands[j]
                    a = c[1] - pos + 1
                    dl, il = len(c[2]) - 1, len(c[3]) - 1
                    if 10 <= a and a + il + 10 <= READ:
                        cigar = [("M", a), ("D", dl), ("M", READ - a)] if dl else [("M", a), ("I", il), ("M", READ - a - il)]
            recs.append((pos, len(recs), bc.make_read(ref, pos, cigar, name=name, flag=flag, mtid=0, mpos=mpos)))
    recs.sort(key=lambda x: (x[0], x[1]))
    alignprops.write_bam(os.path.join(d, "indels.bam"), [("s1", contig_len)], [r for _, _, r in recs])
    alignprops.write_fasta(os.path.join(d, "indels.fa"), {"s1": ref})
    json.dump({"depth": depth, "loci": n_loci, "alt_share": alt_share, "records": len(recs), "candidates": [(c, p, r.decode(), a.decode()) for c, p, r, a in cands]},
              open(os.path.join(d, "indels.json"), "w"))
    print("wrote %d records over %d candidates, depth %d" % (len(recs), n_loci, depth))


def new_path(bam, fa, sites, props, has_isize, spec):
    from varlociraptor_amd import fragments
    t0 = time.perf_counter()
    obs, obx, loc, lox, res, ev, rres = fragments.device_indel_observations(bam, sites, props, has_isize, spec, fa, 0, member_capacity=1 << 22, name_capacity=1 << 26,
                                                                            evidence_capacity=1 << 22)
    wall = time.perf_counter() - t0
    assert res.status == 0, res.status
    s, r = list(res.seconds), list(rres.seconds)
    stages = {"file read": s[0], "upload + inflate": s[1], "record split": s[2], "member pass": s[3], "fragment pass": s[4], "window gather": r[0], "edit distance + band": r[1],
              "pair HMM": r[2], "collect + normalise + apply": r[3], "observations to the host": s[7]}
    dig = hashlib.sha1(obs.tobytes() + obx.tobytes() + loc.tobytes() + lox.tobytes() + ev.tobytes()).hexdigest()[:12]
    return wall, stages, int(res.n_records), len(ev), len(obs), dig


def old_path(bam, fa, cands, spec):
    """today: the per-read indel session, then one (left, right) per QNAME and locus in Python"""
    from varlociraptor_amd import readwindows as rw
    t0 = time.perf_counter()
    sup = rw.device_supports(bam, fa, cands, spec.mode, spec.gap, spec.hop, spec.window)
    t1 = time.perf_counter()
    names = [r.raw_name for r in rw.read_bam(bam)[1]]
    n_frag = 0
    for s in sup:
        pairs = {}
        for i, h in enumerate(s.hits):
            c = pairs.setdefault(names[int(h["record"])], [i, None])
            if c[0] != i:
                c[1] = i
        n_frag += len(pairs)
    t2 = time.perf_counter()
    return t2 - t0, {"device_supports": t1 - t0, "pairing in Python (with read_bam)": t2 - t1}, sum(len(s.hits) for s in sup), n_frag


def measure(label, bam, fa, cands, pj, rounds):
    from varlociraptor_amd import alignprops, fragments, readwindows as rw
    props, ip = fragments.props_of(pj), fragments.indel_props_of(pj)
    spec = fragments.RealignSpec(64, "exact", *fragments.gap_hop_of(pj))
    seqs = rw.read_fasta(fa)
    tid = {n: k for k, (n, _) in enumerate(alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)[0])}
    sites = sorted((fragments.indel_site(seqs[c], tid[c], p, r, a, 64, "%s:%d" % (c, p + 1)) for c, p, r, a in cands), key=lambda s: (s.ref_id, s.start))
    new, old = [], []
    for k in range(rounds + 1):            # alternated; the first round warms up both
        n = new_path(bam, fa, sites, props, ip.insert_size is not None, spec)
        o = old_path(bam, fa, cands, spec)
        if k:
            new.append(n)
            old.append(o)
    med = lambda v: statistics.median(v)
    spread = lambda v: [round(min(v), 4), round(max(v), 4)]
    wn, wo = [x[0] for x in new], [x[0] for x in old]
    out = {"input": label, "records": new[0][2], "candidates": len(cands), "rounds": rounds,
           "indel session": {"evidences": new[0][3], "observations": new[0][4], "digest": new[0][5], "equal digests": len({x[5] for x in new}) == 1,
                             "seconds": round(med(wn), 4), "range": spread(wn), "records/s": round(new[0][2] / med(wn)), "evidences/s": round(new[0][3] / med(wn)),
                             "stages": {k: round(med([x[1][k] for x in new]), 5) for k in new[0][1]}},
           "today": {"evidences": old[0][2], "fragments paired": old[0][3], "seconds": round(med(wo), 4), "range": spread(wo), "records/s": round(new[0][2] / med(wo)),
                     "evidences/s": round(old[0][2] / med(wo)), "stages": {k: round(med([x[1][k] for x in old]), 5) for k in old[0][1]}}}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make")
    ap.add_argument("--run")
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--loci", type=int, default=200)
    ap.add_argument("--alt-share", type=float, default=0.3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fixtures", action="store_true")
    a = ap.parse_args()
    if a.make:
        make(a.make, a.depth, a.loci, a.alt_share)
    if a.run:
        meta = json.load(open(os.path.join(a.run, "indels.json")))
        cands = [(c, p, r.encode(), al.encode()) for c, p, r, al in meta["candidates"]]
        measure("synthetic: depth %d, %d candidates, alt share %g" % (meta["depth"], meta["loci"], meta["alt_share"]), os.path.join(a.run, "indels.bam"),
                os.path.join(a.run, "indels.fa"), cands, PROPS, a.rounds)
        if a.fixtures:
            import fragindel_cases as ic
            import make_indel_fragment_fixtures as tool
            from varlociraptor_amd import alignprops, readwindows as rw
            for name, row in sorted(ic.indels_rows().items()):
                if row is None:
                    continue
                d = os.path.join(ROOT, "tests", "golden", "bam", name)
                fa = os.path.join(a.run, name + ".fa")
                alignprops.write_fasta(fa, rw.read_fasta(os.path.join(d, "ref.fa")))
                for sample, bam, pj in tool.samples_of(d):
                    measure(name + ("" if sample is None else ":" + sample), bam, fa, tool.candidate_of(d)[1], pj, a.rounds)


if __name__ == "__main__":
    main()
