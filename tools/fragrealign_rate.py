"""Rates of the realigning fragment session (vlr_fragpileup_open_realign, csrc/vlr_fragpileup.hip with csrc/vlr_pairscore.h): records/s and
realigned evidences/s with the seconds of each stage on a synthetic coordinate-sorted paired BAM in which a stated share of the reads
carries an insertion over a candidate, and on the test_giab_* fixtures under tests/golden/bam/; the same input scored from the
alignment (--score-indel-reads-from-alignment: the plain session, which a checkout of the parent commit runs as well — that is the
price of the realignment); and the Python path for the same evidences (read_bam + windows + realign.best_hits / prob_related).
profiles/fragrealign.md holds the figures measured with it.

    python tools/fragrealign_rate.py --make DIR [--records 1000000] [--indel-share 0.05]     # writes DIR/pairs.bam, DIR/pairs.fa (no GPU)
    python tools/fragrealign_rate.py --run DIR [--what realign|plain|python|fixtures]         # one JSON line per run
    VLR_PACKAGE_ROOT=<checkout of the parent commit, built> python tools/fragrealign_rate.py --run DIR --what plain

The BAM: pairs of 100-base reads (random bases along the contig, 1 % substitutions, qualities 20-40, MAPQ 60) with inserts of 200-400
bases at sorted positions of one contig of records x 10 bases (10x coverage); every read has three CIGAR operations, 40M 30M 30M, or —
the stated share — 40M 1I 59M; the loci: an SNV every 100 bases, so every read encloses one and an indel-bearing read is one evidence
(sometimes two).  --what python takes the first --python-evidences evidences.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.environ.get("VLR_PACKAGE_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tests"))

READ_LEN = 100
NAME_LEN = 8


def make(d, n_records, share, seed=5):
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
    indel = rng.random(n) < share
    size = 4 + 32 + NAME_LEN + 1 + 12 + READ_LEN // 2 + READ_LEN
    rec = np.zeros((n, size), np.uint8)

    def put(off, arr, dt):
        rec[:, off:off + np.dtype(dt).itemsize] = np.ascontiguousarray(np.asarray(arr).astype(dt)).view(np.uint8).reshape(n, -1)
    put(0, np.full(n, size - 4), "<u4")
    put(4, np.zeros(n), "<i4")
    put(8, pos, "<i4")
    rec[:, 12] = NAME_LEN + 1
    rec[:, 13] = 60
    put(16, np.full(n, 3), "<u2")
    put(18, flag, "<u2")
    put(20, np.full(n, READ_LEN), "<i4")
    put(24, np.zeros(n), "<i4")
    put(28, mpos, "<i4")
    names = np.char.zfill(pair.astype(str), NAME_LEN - 1)
    rec[:, 36] = ord("p")
    rec[:, 37:36 + NAME_LEN] = np.frombuffer("".join(names).encode(), np.uint8).reshape(n, NAME_LEN - 1)
    c0 = 36 + NAME_LEN + 1
    put(c0, np.full(n, (40 << 4) | 0), "<u4")
    put(c0 + 4, np.where(indel, (1 << 4) | 1, (30 << 4) | 0), "<u4")
    put(c0 + 8, np.where(indel, (59 << 4) | 0, (30 << 4) | 0), "<u4")
    # the reference's bases with 1 % substitutions; an indel-bearing read has one base of its own behind its first 40
    col = np.arange(READ_LEN)[None, :]
    src = pos[:, None] + np.where(indel[:, None] & (col > 40), col - 1, col)
    bases = ref[src]
    sub = rng.random((n, READ_LEN)) < 0.01
    bases = np.where(sub, rng.choice(np.frombuffer(b"ACGT", np.uint8), (n, READ_LEN)), bases)
    code = np.zeros(256, np.uint8)
    code[list(b"ACGT")] = [1, 2, 4, 8]
    cc = code[bases]
    rec[:, c0 + 12:c0 + 12 + READ_LEN // 2] = (cc[:, 0::2] << 4) | cc[:, 1::2]
    q0 = c0 + 12 + READ_LEN // 2
    rec[:, q0:q0 + READ_LEN] = rng.integers(20, 41, (n, READ_LEN), dtype=np.uint8)
    head = alignprops.encode_bam([("c", contig_len)], [])
    with open(os.path.join(d, "pairs.bam"), "wb") as f:
        f.write(alignprops.bgzf_compress(head + rec.tobytes()))
    alignprops.write_fasta(os.path.join(d, "pairs.fa"), {"c": ref.tobytes()})
    print("wrote", d, n, "records,", int(indel.sum()), "with an insertion, on", contig_len, "bases")


def loci_of(d):
    from varlociraptor_amd import abi, basecalls
    from varlociraptor_amd.readwindows import read_fasta
    ref = read_fasta(os.path.join(d, "pairs.fa"))["c"]
    other = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
    return ref, [basecalls.Locus(abi.BASEPILEUP_SNV, 0, p, ref[p:p + 1], other[ref[p]]) for p in range(50, len(ref) - 50, 100)]


CAPS = dict(member_capacity=12_000_000, name_capacity=16_000_000, key_capacity=1 << 16)


def run(d, what, python_evidences):
    from varlociraptor_amd import engine, fragments
    ref, loci = loci_of(d)
    props = fragments.Props(fragments.window_of((300.0, 50.0), READ_LEN, None), 60, READ_LEN)
    bam, fa = os.path.join(d, "pairs.bam"), os.path.join(d, "pairs.fa")
    out = dict(what=what, build=engine.build_id(), package=ROOT)
    t0 = time.perf_counter()
    if what == "plain":
        obs, lrec, res = fragments.device_observations(bam, loci, props, 0, False, **CAPS)
    elif what == "realign":
        obs, lrec, res, ev, rres = fragments.device_observations(bam, loci, props, 0, realign=fragments.RealignSpec(), fasta=fa, evidences=True, evidence_capacity=1 << 17, **CAPS)
        rs = list(rres.seconds)
        out.update(evidences=int(rres.n_evidences), x_bytes=int(rres.x_bytes), y_bytes=int(rres.y_bytes), ranges=int(rres.n_ranges), seconds_gather=rs[0],
                   seconds_edit_band=rs[1], seconds_pair_hmm=rs[2], seconds_collect_normalise_apply=rs[3])
    elif what == "python":
        from varlociraptor_amd import readwindows as rw
        _, recs = rw.read_bam(bam)
        t_read = time.perf_counter() - t0
        t1 = time.perf_counter()
        good = [(k, r) for k, r in enumerate(recs)]
        evs = []
        for o, rec in good:
            if len(evs) >= python_evidences:
                break
            if not fragments.basecalls.contains_indel_op(rec):
                continue
            first = max(0, (rec.pos - 50 + 99) // 100)
            for li in range(first, min(first + 2, len(loci))):
                if fragments.basecalls.enclosing(rec, loci[li]):
                    evs.append(fragments.realign_evidence(rec, loci[li], li, o, ref, 64))
        t_windows = time.perf_counter() - t1
        t1 = time.perf_counter()
        fragments.score_pairs(fragments.evidence_pair_batch(evs), fragments.RealignSpec(), device=0)
        out.update(evidences=len(evs), records=len(recs), seconds_read_bam=t_read, seconds_windows=t_windows, seconds_kernels=time.perf_counter() - t1)
        print(json.dumps(out))
        return
    wall = time.perf_counter() - t0
    s = list(res.seconds)
    span = s[5] + s[4] + s[7] + sum(out.get(k, 0.0) for k in ("seconds_edit_band", "seconds_pair_hmm", "seconds_collect_normalise_apply"))
    out.update(records=int(res.n_records), members=int(res.n_members), observations=int(res.n_obs), status=int(res.status), seconds_member_pass=s[3],
               seconds_fragment_pass=s[4], seconds_stream_total=s[5], seconds_to_host=s[7], seconds_span=span, seconds_wall=wall, records_per_s=int(res.n_records) / span)
    if what == "realign":
        out.update(evidences_per_s=out["evidences"] / span)
    print(json.dumps(out))


def fixtures():
    """the test_giab_* fixtures with a BAM: one small file each, realigned and from the alignment"""
    import json as js
    import fragment_cases as fc
    from varlociraptor_amd import alignprops, basecalls, fragments
    from varlociraptor_amd.readwindows import read_fasta
    golden = os.path.join(HERE, "tests", "golden")
    import tempfile
    tmp = tempfile.mkdtemp()
    out = dict(what="fixtures", records=0, evidences=0, observations_realigned=0, observations_plain=0, seconds_realign=0.0, seconds_plain=0.0)
    for name in sorted(n for n in fc.FIXTURES if n.startswith("test_giab_")):
        bam, held, _, cand, props = fc.fixture_case(golden, name)
        contigs, _ = alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)
        seqs = read_fasta(held)
        fasta = os.path.join(tmp, name + ".fa")     # the testcases hold their reference without an index: a copy with its .fai
        alignprops.write_fasta(fasta, seqs)
        loci = [basecalls.locus(seqs[c], [n for n, _ in contigs].index(c), p, r, a) for c, p, r, a in cand]
        spec = fragments.RealignSpec(64, "exact", *fragments.gap_hop_of(js.load(open(os.path.join(golden, "bam", name, "properties.json")))))
        t0 = time.perf_counter()
        o, _, r, ev, _ = fragments.device_observations(bam, loci, props, 0, realign=spec, fasta=fasta, evidences=True)
        out["seconds_realign"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        p, _, _ = fragments.device_observations(bam, loci, props, 0, False)
        out["seconds_plain"] += time.perf_counter() - t0
        out["records"] += int(r.n_records)
        out["evidences"] += len(ev)
        out["observations_realigned"] += len(o)
        out["observations_plain"] += len(p)
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--make")
    ap.add_argument("--run")
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--indel-share", type=float, default=0.05)
    ap.add_argument("--what", choices=["realign", "plain", "python", "fixtures"], default="realign")
    ap.add_argument("--python-evidences", type=int, default=5000)
    a = ap.parse_args()
    if a.make:
        make(a.make, a.records, a.indel_share)
    if a.run and a.what == "fixtures":
        fixtures()
    elif a.run:
        run(a.run, a.what, a.python_evidences)
