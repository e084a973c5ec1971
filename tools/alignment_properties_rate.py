"""Records/s of `estimate alignment-properties`: the HIP path (vlr_bamstats_*) and the pure-Python restatement, on the fixtures of
tests/golden/alignment_properties/ and on a synthetic BAM of N records (default 10 M, written once to --dir), with the time of each
stage of the device path (file read, upload + inflate, record split, take + select kernels, reference upload, statistics kernel,
insert sizes back, host finish).  The restatement is timed on the fixtures and on the first --cpu-records records of the synthetic
BAM only.  One JSON line per input.

    python tools/alignment_properties_rate.py [--records 10000000] [--dir /tmp/ap_rate] [--device 0]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from varlociraptor_amd import alignprops as A  # noqa: E402

STAGES = ("read", "upload_inflate", "split", "take_select", "ref_upload", "stats_kernel", "insert_sizes_d2h", "total", "inflate_kernel", "serial_walk_splits")


def synthetic(path_dir, n):
    """n paired 150-base records (rounded up to 20 000) on a 10 Mb contig, 1 % with a deletion: one block of 20 000 records repeated."""
    fasta, bam = os.path.join(path_dir, "ref.fa"), os.path.join(path_dir, f"synth_{n}.bam")
    if os.path.exists(bam):
        return fasta, bam
    rng = np.random.default_rng(5)
    L = 10_000_000
    ref = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L).tobytes()
    A.write_fasta(fasta, {"s": ref})
    contigs = [("s", L)]
    block = []
    for k in range(20000):
        pos = int(rng.integers(0, L - 400))
        if k % 100 == 0:
            cig, seq = [("M", 70), ("D", 2), ("M", 80)], ref[pos:pos + 70] + ref[pos + 72:pos + 152]
        else:
            cig, seq = [("M", 150)], ref[pos:pos + 150]
        block.append(A.encode_record(0, pos, 60, 0x1 | (0x40 if k % 2 == 0 else 0x80), cig, seq.decode(), 0, pos + 200, 350))
    comp = A.bgzf_compress(b"".join(block))[:-28]     # one block of 20 000 records, compressed once and repeated
    with open(bam, "wb") as f:
        f.write(A.bgzf_compress(A.encode_bam(contigs, []))[:-28])
        for _ in range((n + 19999) // 20000):
            f.write(comp)
        f.write(A.bgzf_compress(b""))
    return fasta, bam


def run(name, fasta, bams, device, cpu_records):
    out = {"input": name}
    t = time.perf_counter()
    c = A.count_bams_device(fasta, bams, 10 ** 12, device)
    td = time.perf_counter() - t
    t = time.perf_counter()
    A.to_json(A.finish(c))
    th = time.perf_counter() - t
    out.update(records=c.n_taken + c.n_skipped, device_s=round(td, 4), device_records_per_s=round((c.n_taken + c.n_skipped) / td),
               stages_s={k: round(v, 4) for k, v in zip(STAGES, c.seconds)}, host_finish_s=round(th, 4))
    t = time.perf_counter()
    cc = A.count_bams(fasta, bams, cpu_records)
    tc = time.perf_counter() - t
    out.update(cpu_records=cc.n_taken + cc.n_skipped, cpu_s=round(tc, 4), cpu_records_per_s=round((cc.n_taken + cc.n_skipped) / tc))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10_000_000)
    ap.add_argument("--dir", default="/tmp/ap_rate")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--cpu-records", type=int, default=20000)
    a = ap.parse_args()
    fx = os.path.join(ROOT, "tests", "golden", "alignment_properties")
    fa = os.path.join(fx, "chr10.fa")
    for b in ("tumor-first30000.reads_with_soft_clips.bam", "tumor-first30000.bunch_of_reads_made_single_ended.bam"):
        run(b, fa, [os.path.join(fx, b)], a.device, 10 ** 9)
    os.makedirs(a.dir, exist_ok=True)
    t = time.perf_counter()
    fasta, bam = synthetic(a.dir, a.records)
    print(json.dumps({"synthetic_written_s": round(time.perf_counter() - t, 1), "bytes": os.path.getsize(bam)}), flush=True)
    run(f"synthetic_{a.records}", fasta, [bam], a.device, a.cpu_records)
