"""Rates of the fragment session (vlr_fragpileup_*, csrc/vlr_fragpileup.hip): observations/s and records/s with the seconds of each
stage on a synthetic coordinate-sorted paired BAM and on the fixtures under tests/golden/bam/, the cost of the two host steps of the
front end (prob_hit_base and the MAPQ adjustment), and — on the first loci of the same input — the whole front end against the path it
extends (basecalls.allele_supports with merge_mates, which computes less: no mates outside the locus, no features).
profiles/fragpileup.md holds the figures measured with it.

    python tools/fragpileup_rate.py --make DIR [--records 1000000]     # writes DIR/pairs.bam, DIR/pairs.fa (no GPU)
    python tools/fragpileup_rate.py --run DIR [--repeat 3]             # one JSON line

The BAM: pairs of 100-base reads (CIGAR 100M, random bases, qualities 20-40, MAPQ 60, every 16th pair MAPQ 20) with inserts of
200-400 bases at sorted positions of one contig of records x 10 bases (10x coverage); the loci: an SNV every 100 bases; the window
follows from insert_size mean 300, sd 50: 600 bases, so a locus has about 60 members.  Every record carries an XA:Z tag with one entry
(as bwa writes them for repeats; here on all records, so that the key pool and the alt-locus mode see the most they can at this depth).
--run also times one session over a single locus with VLR_FRAGPILEUP_MAX_MEMBERS members (tests/fragment_cases.py: deep_loci): the
per-locus sort at the size the limit allows.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

READ_LEN = 100
NAME_LEN = 8


def make(d, n_records, seed=5):
    from varlociraptor_amd import alignprops
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    n_pairs = n_records // 2
    contig_len = n_records * 10
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), contig_len)
    p1 = rng.integers(0, contig_len - 500, n_pairs)
    p2 = p1 + rng.integers(100, 301, n_pairs)
    pos = np.concatenate([p1, p2])
    mpos = np.concatenate([p2, p1])
    flag = np.concatenate([np.full(n_pairs, 0x63), np.full(n_pairs, 0x93)])
    pair = np.concatenate([np.arange(n_pairs), np.arange(n_pairs)])
    order = np.argsort(pos, kind="stable")
    pos, mpos, flag, pair = pos[order], mpos[order], flag[order], pair[order]
    n = len(pos)
    size = 4 + 32 + NAME_LEN + 1 + 4 + READ_LEN // 2 + READ_LEN + 3 + 21
    rec = np.zeros((n, size), np.uint8)

    def put(off, arr, dt):
        rec[:, off:off + np.dtype(dt).itemsize] = np.ascontiguousarray(arr.astype(dt)).view(np.uint8).reshape(n, -1)
    put(0, np.full(n, size - 4), "<u4")
    put(4, np.zeros(n), "<i4")
    put(8, pos, "<i4")
    rec[:, 12] = NAME_LEN + 1
    rec[:, 13] = np.where(pair % 16 == 0, 20, 60)
    put(16, np.ones(n), "<u2")
    put(18, flag, "<u2")
    put(20, np.full(n, READ_LEN), "<i4")
    put(24, np.zeros(n), "<i4")
    put(28, mpos, "<i4")
    names = np.char.zfill(pair.astype(str), NAME_LEN - 1)
    rec[:, 36] = ord("p")
    rec[:, 37:36 + NAME_LEN] = np.frombuffer("".join(names).encode(), np.uint8).reshape(n, NAME_LEN - 1)
    c0 = 36 + NAME_LEN + 1
    put(c0, np.full(n, (READ_LEN << 4) | 0), "<u4")
    # the reference's bases with 1 % substitutions
    bases = ref[pos[:, None] + np.arange(READ_LEN)[None, :]]
    sub = rng.random((n, READ_LEN)) < 0.01
    bases = np.where(sub, rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, READ_LEN)), bases)
    code = np.zeros(256, np.uint8)
    code[list(b"ACGT")] = [1, 2, 4, 8]
    cc = code[bases]
    rec[:, c0 + 4:c0 + 4 + READ_LEN // 2] = (cc[:, 0::2] << 4) | cc[:, 1::2]
    q0 = c0 + 4 + READ_LEN // 2
    rec[:, q0:q0 + READ_LEN] = rng.integers(20, 41, (n, READ_LEN), dtype=np.uint8)
    # XA:Z "c,+NNNNNNNNN,100M,0;": an alternative hit somewhere on the contig; a tenth of the reads of a region share one
    alt = np.where(rng.random(n) < 0.1, (pos // 5000) * 5000 + 17, rng.integers(0, contig_len, n))
    xa = np.char.add(np.char.add("XAZc,+", np.char.zfill(alt.astype(str), 9)), ",100M,0;")
    rec[:, q0 + READ_LEN:size - 1] = np.frombuffer("".join(xa).encode(), np.uint8).reshape(n, 3 + 20)
    head = alignprops.encode_bam([("c", contig_len)], [])
    with open(os.path.join(d, "pairs.bam"), "wb") as f:
        f.write(alignprops.bgzf_compress(head + rec.tobytes()))
    alignprops.write_fasta(os.path.join(d, "pairs.fa"), {"c": ref.tobytes()})
    print("wrote", d, n, "records on", contig_len, "bases")


def loci_of(d):
    from varlociraptor_amd import abi, basecalls
    from varlociraptor_amd.readwindows import read_fasta
    ref = read_fasta(os.path.join(d, "pairs.fa"))["c"]
    other = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
    return ref, [basecalls.Locus(abi.BASEPILEUP_SNV, 0, p, ref[p:p + 1], other[ref[p]]) for p in range(50, len(ref) - 50, 100)]


def host_steps(obs, lrec, props, t):
    """seconds of the two host steps of the front end over the device's integer columns, with the restatement's own functions"""
    from varlociraptor_amd import fragments
    t0 = time.perf_counter()
    _ = [-math.log(x) for x in obs["len_sum"].tolist()]
    t_hit = time.perf_counter() - t0
    t0 = time.perf_counter()
    mq = obs["min_mapq"].tolist()
    for r in lrec:
        o0, n = int(r["obs_offset"]), int(r["n_obs"])
        fragments.adjusted_prob_mapping([t.call[q] for q in mq[o0:o0 + n]], props.max_mapq, t)
    return t_hit, time.perf_counter() - t0


def run(d, repeat, front_loci):
    import fragment_cases as fc
    from varlociraptor_amd import basecalls, fragments
    ref, loci = loci_of(d)
    props = fragments.Props(fragments.window_of((300.0, 50.0), READ_LEN, None), 60, READ_LEN)
    bam = os.path.join(d, "pairs.bam")
    t = basecalls.library_tables()
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        obs, lrec, res = fragments.device_observations(bam, loci, props, 0, member_capacity=12_000_000, name_capacity=16_000_000, key_capacity=2_000_000)
        wall = time.perf_counter() - t0
        s = list(res.seconds)
        span = s[5] + s[4] + s[7]
        if best is None or span < best["seconds_span"]:
            best = dict(records=int(res.n_records), members=int(res.n_members), observations=int(res.n_obs), loci=len(loci), status=int(res.status),
                        keys=int(res.needed_keys), seconds_read=s[0], seconds_upload_inflate=s[1], seconds_split=s[2], seconds_member_pass=s[3], seconds_fragment_pass=s[4],
                        seconds_stream_total=s[5], seconds_inflate_kernels=s[6], seconds_to_host=s[7], seconds_span=span, seconds_wall=wall)
    best.update(records_per_s=best["records"] / best["seconds_span"], observations_per_s=best["observations"] / best["seconds_span"],
                members_per_locus_max=int(lrec["n_members"].max()), loci_too_deep=int(res.n_loci_too_deep))
    t_hit, t_adj = host_steps(obs, lrec, props, t)
    best.update(host_prob_hit_base_seconds=t_hit, host_mapq_adjustment_seconds=t_adj)
    # the whole front end and the path it extends, on the first loci
    cands = [("c", l.start, l.ref, l.alt) for l in loci[:front_loci]]
    t0 = time.perf_counter()
    tabs = fragments.observations(bam, os.path.join(d, "pairs.fa"), cands, props, device=0)
    best.update(front_loci=front_loci, front_fragments_seconds=time.perf_counter() - t0, front_fragments_observations=sum(len(x) for x in tabs))
    t0 = time.perf_counter()
    sup = basecalls.allele_supports(bam, os.path.join(d, "pairs.fa"), cands, device=0)
    best.update(front_basecalls_seconds=time.perf_counter() - t0, front_basecalls_observations=sum(len(x) for x in sup))
    # one locus at the member limit: the cost of the per-locus sort where it is largest
    import basecall_cases as bc
    import tempfile
    contigs, dc, drecs, dprops = fc.deep_loci([4096])
    with tempfile.TemporaryDirectory() as tmp:
        dbam, _ = bc.write_case(tmp, "deep", contigs, drecs)
        dl = bc.loci_of(dc, contigs)
        fragments.device_observations(dbam, dl, dprops, 0)
        _, _, r = fragments.device_observations(dbam, dl, dprops, 0)
    best.update(deep_locus_members=4096, deep_locus_fragment_pass_seconds=list(r.seconds)[4], deep_locus_observations=int(r.n_obs))
    # the fixtures: one small file each
    fx = dict(observations=0, records=0, seconds=0.0)
    golden = os.path.join(ROOT, "tests", "golden")
    from varlociraptor_amd import alignprops
    from varlociraptor_amd.readwindows import read_fasta
    for name in sorted(fc.FIXTURES):
        fbam, fasta, _, cand, fprops = fc.fixture_case(golden, name)
        contigs, _ = alignprops.bam_header(alignprops.inflate_bgzf(fbam), fbam)
        seqs = read_fasta(fasta)
        fl = [basecalls.locus(seqs[c], [n for n, _ in contigs].index(c), p, r, a) for c, p, r, a in cand]
        t0 = time.perf_counter()
        o, _, r = fragments.device_observations(fbam, fl, fprops, 0)
        fx["seconds"] += time.perf_counter() - t0
        fx["observations"] += len(o)
        fx["records"] += int(r.n_records)
    best.update(fixtures=fx)
    print(json.dumps(best))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--make")
    ap.add_argument("--run")
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--front-loci", type=int, default=2000)
    a = ap.parse_args()
    if a.make:
        make(a.make, a.records)
    if a.run:
        run(a.run, a.repeat, a.front_loci)
