"""Rates of the SNV / MNV allele-support pass (vlr_basepileup_*, csrc/vlr_basepileup.hip) on a synthetic BAM: hits/s and records/s of the
device path per stage, and the restatement's rate (varlociraptor_amd/basecalls.py) on a slice of the same input.  profiles/basepileup.md
holds the figures measured with it.

    python tools/basepileup_rate.py --make DIR [--records 1000000] [--loci 100000]     # writes DIR/rate.bam, DIR/slice.bam, DIR/loci.npz (no GPU)
    python tools/basepileup_rate.py --run DIR [--repeat 3]                             # one JSON line

The BAM: reads of 100 bases (CIGAR 100M, random bases, qualities 20-40) at sorted random positions of one contig of 10^7 bases; the
loci: random positions of that contig, half of them MNVs of 2-9 bases — about one enclosed locus per read.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTIG_LEN = 10_000_000
READ_LEN = 100


def make(d, n_records, n_loci, seed=5):
    from varlociraptor_amd import alignprops
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
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
    code = rng.choice(np.array([1, 2, 4, 8], np.uint8), (n_records, READ_LEN))
    rec[:, 42:42 + READ_LEN // 2] = (code[:, 0::2] << 4) | code[:, 1::2]
    rec[:, 42 + READ_LEN // 2:] = rng.integers(20, 41, (n_records, READ_LEN), dtype=np.uint8)
    head = alignprops.encode_bam([("c", CONTIG_LEN)], [])
    with open(os.path.join(d, "rate.bam"), "wb") as f:
        f.write(alignprops.bgzf_compress(head + rec.tobytes()))
    with open(os.path.join(d, "slice.bam"), "wb") as f:
        f.write(alignprops.bgzf_compress(head + rec[:20000].tobytes()))
    start = np.sort(rng.integers(0, CONTIG_LEN - 16, n_loci))
    length = np.where(np.arange(n_loci) % 2 == 1, rng.integers(2, 10, n_loci), 1)
    bases = rng.choice(np.frombuffer(b"ACGT", np.uint8), (n_loci, 9))
    np.savez(os.path.join(d, "loci.npz"), start=start, length=length, ref=bases, alt=np.roll(bases, 1, axis=1))
    print("wrote", d, n_records, "records,", n_loci, "loci")


def load_loci(d):
    from varlociraptor_amd import abi, basecalls
    z = np.load(os.path.join(d, "loci.npz"))
    return [basecalls.Locus(abi.BASEPILEUP_SNV if l == 1 else abi.BASEPILEUP_MNV, 0, int(s), bytes(r[:l]), bytes(a[:l]))
            for s, l, r, a in zip(z["start"], z["length"], z["ref"], z["alt"])]


def run(d, repeat):
    from varlociraptor_amd import basecalls
    from varlociraptor_amd.readwindows import read_bam
    loci = load_loci(d)
    bam = os.path.join(d, "rate.bam")
    best = None
    for _ in range(repeat):
        t0 = time.perf_counter()
        arr, res = basecalls.device_hits(bam, loci, 0, hit_capacity=4_000_000)
        wall = time.perf_counter() - t0
        s = list(res.seconds)
        if best is None or s[5] < best["seconds_total"]:
            best = dict(hits=int(res.n_hits), records=int(res.n_records), seconds_read=s[0], seconds_upload_inflate=s[1], seconds_split=s[2], seconds_kernels=s[3],
                        seconds_hits_to_host_and_order=s[4], seconds_total=s[5], seconds_inflate_kernels=s[6], seconds_wall=wall)
    span = best["seconds_total"] + best["seconds_hits_to_host_and_order"]
    best.update(records_per_s=best["records"] / span, hits_per_s=best["hits"] / span, kernel_share=best["seconds_kernels"] / span,
                record_stream_bytes=best["records"] * 192, record_stream_GBps_in_kernels=2 * best["records"] * 192 / best["seconds_kernels"] / 1e9)
    _, recs = read_bam(os.path.join(d, "slice.bam"))
    t0 = time.perf_counter()
    sc = basecalls.score_records(recs, loci)
    dt = time.perf_counter() - t0
    best.update(restatement_records=len(recs), restatement_hits=len(sc.hits), restatement_records_per_s=len(recs) / dt, restatement_hits_per_s=len(sc.hits) / dt)
    print(json.dumps(best))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--make")
    ap.add_argument("--run")
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--loci", type=int, default=100_000)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    if a.make:
        make(a.make, a.records, a.loci)
    if a.run:
        run(a.run, a.repeat)
