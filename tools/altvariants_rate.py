#!/usr/bin/env python
"""Per-stage seconds of an indel fragment session (vlr_fragpileup_open_indel) on a synthetic BAM with 0, 1 and 3 competitors per
locus (vlr_fragpileup_set_alt_variants), and of the same input without the call — the path every session took before.  On a commit
without the entry point only the last is measured, so the same command gives the parent's figures.

    python tools/altvariants_rate.py [--loci 256] [--reads 48] [--warmup 2] [--repeats 7] [--only-no-call] [--out FILE]

One JSON line per configuration: the median over the repeats of the session's own stage timers (vlr_fragpileup_result seconds:
member pass kernels, fragment pass; vlr_fragpileup_realign_result seconds: window gather, edit distance (with expand and select in a
session with competitors), pair HMM (with the compaction), collect + apply), the wall seconds of the whole call, the evidences and the
pairs through the edit-distance kernel and the pair HMM.  profiles/altvariants.md records a run and how it was made."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from varlociraptor_amd import alignprops, fragments  # noqa: E402
from varlociraptor_amd import readwindows as rw  # noqa: E402

READ, STEP = 60, 200


def synthetic(n_loci, reads, seed=3):
    """(contig, per locus the 2-base deletion candidate and three more deletions at its position, encoded records): at each site half
    of the reads carry the 2-base deletion, a quarter the 1-base one (the first competitor), a quarter the reference"""
    rng = random.Random(seed)
    ref = bytes(rng.choice(b"ACGT") for _ in range(STEP * n_loci + STEP))
    cands, recs = [], []
    for k in range(n_loci):
        at = STEP * k + 100
        cands.append([("s1", at, ref[at:at + 1 + d], ref[at:at + 1]) for d in (2, 1, 3, 4)])
        for j in range(reads):
            p = at - READ + 10 + j % (READ - 20)
            a = at - p + 1
            d = (2, 2, 1, 0)[j % 4]
            cigar = [("M", READ)] if d == 0 else [("M", a), ("D", d), ("M", READ - a)]
            seq, r = b"", p
            for op, l in cigar:
                if op == "M":
                    seq += ref[r:r + l]
                r += l
            recs.append((p, len(recs), alignprops.encode_record(0, p, 60, 0x10 if j % 2 else 0, cigar, seq.decode(), qual=bytes([30] * READ), name="r%d_%d" % (k, j))))
    recs.sort(key=lambda x: x[:2])
    return ref, cands, [r for _, _, r in recs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loci", type=int, default=256)
    ap.add_argument("--reads", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--only-no-call", action="store_true", help="only the session without vlr_fragpileup_set_alt_variants (for a kernel trace)")
    ap.add_argument("--out")
    a = ap.parse_args()
    ref, cands, recs = synthetic(a.loci, a.reads)
    tmp = tempfile.mkdtemp()
    bam, fa = os.path.join(tmp, "s.bam"), os.path.join(tmp, "s.fa")
    alignprops.write_bam(bam, [("s1", len(ref))], recs, 0xff00)
    alignprops.write_fasta(fa, {"s1": ref})
    spec = fragments.RealignSpec()
    props = fragments.Props(READ + 10, 60, READ)
    sites = [fragments.IndelSite(0, rw.indel_locus(ref, c[0][1], c[0][2], c[0][3], spec.window)) for c in cands]
    has_feature = hasattr(fragments, "competitor_window")
    configs = [("no call", None)]
    if has_feature and not a.only_no_call:
        for k in (0, 1, 3):
            configs.append(("%d competitors" % k, [[fragments.competitor_window(ref, x[1], x[2], x[3], spec.window) for x in c[1:1 + k]] for c in cands]))
    lines = []
    for label, comp in configs:
        kw = {} if comp is None else {"competitors": comp}
        runs = []
        for it in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            got = fragments.device_indel_observations(bam, sites, props, True, spec, fa, 0, **kw)
            wall = time.perf_counter() - t0
            if it >= a.warmup:
                runs.append((wall, list(got[4].seconds), list(got[6].seconds)))
        med = lambda xs: statistics.median(xs)
        line = {"config": label, "loci": a.loci, "records": len(recs), "evidences": int(got[6].n_evidences), "observations": int(got[4].n_obs), "ranges": int(got[6].n_ranges),
                "wall_s": med([r[0] for r in runs]), "member_pass_s": med([r[1][3] for r in runs]), "fragment_pass_s": med([r[1][4] for r in runs]),
                "gather_s": med([r[2][0] for r in runs]), "edit_s": med([r[2][1] for r in runs]), "hmm_s": med([r[2][2] for r in runs]),
                "collect_apply_s": med([r[2][3] for r in runs]), "warmup": a.warmup, "repeats": a.repeats}
        if comp is not None:
            line["edit_pairs"], line["hmm_pairs"] = int(got[8].n_edit_pairs), int(got[8].n_hmm_pairs)
        else:
            line["edit_pairs"] = line["hmm_pairs"] = 2 * int(got[6].n_evidences)
        lines.append(json.dumps(line))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
