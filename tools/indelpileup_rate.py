"""Rates of the indel allele-support pass (vlr_indelpileup_*, csrc/vlr_indelpileup.hip): evidences/s and records/s of the device path per
stage, and today's Python path (readwindows.read_bam + evidence_windows + allele_supports: a per-read CIGAR walk on the host, the same
kernels) on the same input, or on a slice of it.  profiles/indelpileup.md holds the figures measured with it.

    python tools/indelpileup_rate.py --make DIR [--records 400000] [--loci 20000]       # writes DIR/rate.bam, slice.bam, ref.fa, loci.npz (no GPU)
    python tools/indelpileup_rate.py --run DIR [--repeat 3] [--mode exact] [--capacity 8000000]   # one JSON line
    python tools/indelpileup_rate.py --fixtures [--repeat 3]                             # one JSON line per testcase of tests/golden/bam

The BAM: reads of 100 bases (CIGAR 100M, the reference's bases with 1 % mismatches, qualities 20-40) at sorted random positions of one
contig of 2 * 10^6 bases; the loci: deletions, insertions and replacements of 1-6 bases at random positions — about one evidence per
read with 20 000 loci, five with 100 000.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONTIG_LEN = 2_000_000
READ_LEN = 100
SLICE = 4000
STAGES = ("read", "upload_inflate", "split", "count_scan", "fill_gather", "edit_band", "realign", "collect", "hits_to_host_and_order", "total", "inflate_kernels")


def make(d, n_records, n_loci, seed=5):
    from varlociraptor_amd import alignprops
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    contig = rng.choice(np.frombuffer(b"ACGT", np.uint8), CONTIG_LEN)
    alignprops.write_fasta(os.path.join(d, "ref.fa"), {"c": contig.tobytes()})
    size = 4 + 32 + 2 + 4 + READ_LEN // 2 + READ_LEN
    rec = np.zeros((n_records, size), np.uint8)
    pos = np.sort(rng.integers(0, CONTIG_LEN - READ_LEN, n_records)).astype("<i4")

    def put(off, arr, dt):
        rec[:, off:off + np.dtype(dt).itemsize] = np.ascontiguousarray(arr.astype(dt)).view(np.uint8).reshape(n_records, -1)
    put(0, np.full(n_records, size - 4), "<u4")
    put(4, np.zeros(n_records), "<i4")
    put(8, pos, "<i4")
    rec[:, 12] = 2
    rec[:, 13] = 60
    put(16, np.ones(n_records), "<u2")
    put(18, rng.choice([0, 16], n_records), "<u2")
    put(20, np.full(n_records, READ_LEN), "<i4")
    put(24, np.full(n_records, -1), "<i4")
    put(28, np.full(n_records, -1), "<i4")
    rec[:, 36] = ord("r")
    put(38, np.full(n_records, (READ_LEN << 4) | 0), "<u4")
    bases = contig[pos[:, None].astype(np.int64) + np.arange(READ_LEN)]
    miss = rng.random((n_records, READ_LEN)) < 0.01
    bases = np.where(miss, rng.choice(np.frombuffer(b"ACGT", np.uint8), (n_records, READ_LEN)), bases)
    code = np.zeros(256, np.uint8)
    code[list(b"ACGT")] = [1, 2, 4, 8]
    code = code[bases]
    rec[:, 42:42 + READ_LEN // 2] = (code[:, 0::2] << 4) | code[:, 1::2]
    rec[:, 42 + READ_LEN // 2:] = rng.integers(20, 41, (n_records, READ_LEN), dtype=np.uint8)
    head = alignprops.encode_bam([("c", CONTIG_LEN)], [])
    with open(os.path.join(d, "rate.bam"), "wb") as f:
        f.write(alignprops.bgzf_compress(head + rec.tobytes()))
    with open(os.path.join(d, "slice.bam"), "wb") as f:
        f.write(alignprops.bgzf_compress(head + rec[:SLICE].tobytes()))
    start = np.sort(rng.choice(CONTIG_LEN - 400, n_loci, replace=False) + 200)
    np.savez(os.path.join(d, "loci.npz"), start=start, kind=rng.integers(0, 3, n_loci), a=rng.integers(1, 7, n_loci), b=rng.integers(1, 7, n_loci),
             ins=rng.choice(np.frombuffer(b"ACGT", np.uint8), (n_loci, 8)))
    print("wrote", d, n_records, "records,", n_loci, "loci")


def load_candidates(d, contig):
    z = np.load(os.path.join(d, "loci.npz"))
    out = []
    for s, k, a, b, ins in zip(z["start"], z["kind"], z["a"], z["b"], z["ins"]):
        s, a, b = int(s), int(a), int(b)
        if k == 0:
            out.append(("c", s, contig[s:s + 1 + a], contig[s:s + 1]))
        elif k == 1:
            out.append(("c", s, contig[s:s + 1], contig[s:s + 1] + bytes(ins[:a])))
        else:
            b = b if b != a + 1 else b + 1
            out.append(("c", s, contig[s:s + 1 + a], bytes(ins[:b])))
    return out


def device(bam, fasta, rid, loci, mode, gap, hop, repeat, capacity):
    from varlociraptor_amd import readwindows as rw
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        arr, res, _ = rw.device_hits(bam, fasta, rid, loci, mode, gap, hop, hit_capacity=capacity)
        wall = time.perf_counter() - t0
        s = list(res.seconds)
        span = s[9] + s[8]
        if best is None or span < best["seconds_span"]:
            best = dict(evidences=int(res.n_hits), records=int(res.n_records), x_bytes=int(res.x_bytes), y_bytes=int(res.y_bytes), seconds_span=span, seconds_wall=wall,
                        **{"seconds_" + n: s[k] for k, n in enumerate(STAGES)})
    best.update(records_per_s=best["records"] / best["seconds_span"], evidences_per_s=best["evidences"] / best["seconds_span"])
    return best


def python_path(bam, ref_seq, loci, gap, hop):
    """today's path: read_bam + evidence_windows + allele_supports per locus; (records, evidences, seconds)"""
    from varlociraptor_amd import readwindows as rw
    t0 = time.perf_counter()
    _, recs = rw.read_bam(bam)
    n = 0
    for loc in loci:
        reads = rw.evidence_windows(recs, ref_seq, loc)
        if reads:
            rw.allele_supports(reads, loc.alt_allele, gap, hop)
        n += len(reads)
    return len(recs), n, time.perf_counter() - t0


def run(d, repeat, mode, capacity):
    from varlociraptor_amd import engine
    from varlociraptor_amd import readwindows as rw
    contig = rw.read_fasta(os.path.join(d, "ref.fa"))["c"]
    loci = [rw.indel_locus(contig, pos, ref, alt) for _, pos, ref, alt in load_candidates(d, contig)]
    out = device(os.path.join(d, "rate.bam"), os.path.join(d, "ref.fa"), [0] * len(loci), loci, mode, None, None, repeat, capacity)
    out.update(mode=mode, build_id=engine.build_id(), loci=len(loci))
    # the Python path on the slice, against the loci its reads can reach (it walks every record per locus)
    _, recs = rw.read_bam(os.path.join(d, "slice.bam"))
    hi = max(r.end_pos() for r in recs) + 200
    near = [l for l in loci if l.start < hi]
    n_rec, n_ev, dt = python_path(os.path.join(d, "slice.bam"), contig, near, None, None)
    out.update(python_records=n_rec, python_loci=len(near), python_evidences=n_ev, python_seconds=dt, python_evidences_per_s=n_ev / dt if dt else 0.0)
    print(json.dumps(out))


def fixtures(repeat):
    import tempfile
    import bam_pairs as bp
    import indel_cases as ic
    from varlociraptor_amd import engine, realign
    golden = os.path.join(ROOT, "tests", "golden")
    tmp = tempfile.mkdtemp()   # (the testcases hold their reference without a .fai)
    for name in sorted(bp.BAM_CASES):
        spec = bp.BAM_CASES[name]
        bam, fasta, contigs, names, cand = ic.fixture_case(golden, name, tmp)
        gap = realign.GapParams(*spec["gap"]) if spec["gap"] else None
        hop = realign.HopParams(*spec["hop"]) if spec.get("hop") else None
        loci, rid, _ = ic.loci_of(cand, contigs, names=names)
        out = device(bam, fasta, rid, loci, "homopolymer" if hop else "exact", gap, hop, repeat, 1 << 16)
        n_rec, n_ev, dt = python_path(bam, contigs[cand[0][0]].upper(), loci, gap, hop)
        out.update(testcase=name, build_id=engine.build_id(), python_evidences=n_ev, python_seconds=dt, python_evidences_per_s=n_ev / dt)
        print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--make")
    ap.add_argument("--run")
    ap.add_argument("--fixtures", action="store_true")
    ap.add_argument("--records", type=int, default=400_000)
    ap.add_argument("--loci", type=int, default=20_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--mode", default="exact")
    ap.add_argument("--capacity", type=int, default=8_000_000)
    a = ap.parse_args()
    if a.make:
        make(a.make, a.records, a.loci)
    if a.run:
        run(a.run, a.repeat, a.mode, a.capacity)
    if a.fixtures:
        fixtures(a.repeat)
