"""Rates of the methylation session of the fragment pass (vlr_fragpileup_open_methylation, csrc/vlr_fragpileup.hip over
csrc/vlr_methylation.h) and the untouched sessions beside it; profiles/methylation.md holds the figures.

    python tools/methylation_rate.py --make DIR [--records 1000000] [--long-records 20000]    # writes the two synthetic BAMs (numpy; no GPU)
    python tools/methylation_rate.py --run DIR [--rounds 5] [--fixtures]                        # one JSON line per input
    python tools/methylation_rate.py --sessions [--strip-new] [--dir DIR]                       # the SNV / MNV, realigning and indel sessions: digests, pass times

--make: `converted.bam` — pairs (flags 99 / 147) of 150-base reads, MAPQ 60, qualities 30, inner distance 0-200, coordinate sorted, on one
contig with a CpG every 50 bases; a forward-orientation read shows T for C at a CpG with probability 0.3 (both mates of a pair are of
forward orientation).  `annotated.bam` — unpaired forward reads of 15 000 bases (flag 0) on a contig of A / T with a CpG every 50 bases,
each with MM:Z:C+m and ML:B:C calls at every second of its CpGs.  Candidates: every CpG.
--run: every run after the first of a process is timed; the JSON gives the median and the range of the wall-clock seconds of the whole
call (file read included), the session's own stage counters, and the rate of the Python restatement on the first records of the same
input (it pairs every record with every locus: a slice is all it can take).
--sessions: 40 000 synthetic pairs over 120 SNV / MNV loci (tests/fragment_cases.synthetic) through the plain and the realigning
session, and the synthetic pairs of tests/fragindel_cases through the indel session: digest of the output bytes, milliseconds of the
member pass and of the fragment pass.  --strip-new takes the entry points of the methylation session out of the signature table, so
that the same script loads a library built from the parent commit (VLR_LIB).
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

SPACING = 50
SEQ_CODE = {ord("A"): 1, ord("C"): 2, ord("G"): 4, ord("T"): 8}


def pack_bases(bases):
    """(n, l) ASCII bases -> (n, (l + 1) // 2) packed nibbles"""
    lut = np.zeros(256, np.uint8)
    for k, v in SEQ_CODE.items():
        lut[k] = v
    codes = lut[bases]
    if codes.shape[1] & 1:
        codes = np.concatenate([codes, np.zeros((codes.shape[0], 1), np.uint8)], axis=1)
    return (codes[:, 0::2] << 4) | codes[:, 1::2]


def records_block(pos, flag, mpos, names, bases, aux=None):
    """n records of one length, all M, MAPQ 60, qualities 30, as an (n, bytes) array (aux: a list of bytes per record, or None)"""
    from varlociraptor_amd.alignprops import reg2bin
    n, l = bases.shape
    name_len = names.shape[1] + 1
    head = np.zeros(n, np.dtype([("bs", "<u4"), ("tid", "<i4"), ("pos", "<i4"), ("lrn", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("ncig", "<u2"), ("flag", "<u2"), ("lseq", "<i4"),
                                 ("mtid", "<i4"), ("mpos", "<i4"), ("tlen", "<i4")]))
    head["tid"], head["pos"], head["lrn"], head["mapq"], head["ncig"], head["flag"], head["lseq"] = 0, pos, name_len, 60, 1, flag, l
    head["mtid"], head["mpos"] = np.where(mpos >= 0, 0, -1), mpos
    head["bin"] = [reg2bin(int(p), int(p) + l) for p in pos] if n <= 50000 else 4680      # (the sessions do not read the bin)
    fixed = np.concatenate([head.view(np.uint8).reshape(n, 36), names, np.zeros((n, 1), np.uint8),
                            np.tile(np.frombuffer(np.array([(l << 4) | 0], "<u4").tobytes(), np.uint8), (n, 1)), pack_bases(bases), np.full((n, l), 30, np.uint8)], axis=1)
    if aux is None:
        fixed[:, 0:4] = np.frombuffer(np.array([fixed.shape[1] - 4], "<u4").tobytes(), np.uint8)
        return [fixed.tobytes()]
    out = []
    for k in range(n):
        body = fixed[k, 4:].tobytes() + aux[k]
        out.append(len(body).to_bytes(4, "little") + body)
    return out


def digits(v, width):
    v = np.asarray(v, np.int64)
    return np.stack([(v // 10 ** (width - 1 - j)) % 10 + 48 for j in range(width)], axis=1).astype(np.uint8)


def make(d, n_records, n_long, seed=11):
    from varlociraptor_amd import alignprops
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    # ---- converted: depth 30
    read, n_pairs = 150, n_records // 2
    contig_len = max(n_records * read // 30, 4000)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), contig_len)
    cpg = np.arange(100, contig_len - 100, SPACING)
    ref[cpg], ref[cpg + 1] = ord("C"), ord("G")
    p1 = np.sort(rng.integers(0, contig_len - 2 * read - 210, n_pairs))
    p2 = p1 + read + rng.integers(0, 201, n_pairs)
    pos = np.concatenate([p1, p2])
    flag = np.concatenate([np.full(n_pairs, 99), np.full(n_pairs, 147)])
    mpos = np.concatenate([p2, p1])
    names = np.concatenate([np.full((2 * n_pairs, 1), ord("p"), np.uint8), digits(np.concatenate([np.arange(n_pairs)] * 2), 8)], axis=1)
    order = np.lexsort((flag, pos))
    pos, flag, mpos, names = pos[order], flag[order], mpos[order], names[order]
    chunks = []
    for a in range(0, 2 * n_pairs, 100000):
        b = min(a + 100000, 2 * n_pairs)
        bases = ref[pos[a:b, None] + np.arange(read)[None, :]]
        at_c = (pos[a:b, None] + np.arange(read)[None, :] - 100) % SPACING == 0
        bases = np.where(at_c & (bases == ord("C")) & (rng.random(bases.shape) < 0.3), ord("T"), bases).astype(np.uint8)
        chunks += records_block(pos[a:b], flag[a:b], mpos[a:b], names[a:b], bases)
    with open(os.path.join(d, "converted.bam"), "wb") as f:
        f.write(alignprops.bgzf_compress(alignprops.encode_bam([("s1", contig_len)], chunks)))
    meta = {"converted": {"records": 2 * n_pairs, "contig_len": int(contig_len), "loci": len(cpg), "read": read}}
    # ---- annotated: depth 30
    read = 15000
    contig_len = max(n_long * read // 30, 2 * read)
    ref = rng.choice(np.frombuffer(b"AT", np.uint8), contig_len)
    cpg = np.arange(100, contig_len - 100, SPACING)
    ref[cpg], ref[cpg + 1] = ord("C"), ord("G")
    pos = np.sort(rng.integers(0, contig_len - read, n_long))
    recs = []
    for a in range(0, n_long, 2000):
        b = min(a + 2000, n_long)
        bases = ref[pos[a:b, None] + np.arange(read)[None, :]]
        aux = []
        for k in range(a, b):
            n_c = len(range((100 - int(pos[k])) % SPACING, read, SPACING))       # the read's C's: one per CpG it covers
            calls = (n_c + 1) // 2                                               # every second of them
            mm = "C+m,0" + ",1" * (calls - 1) + ";"
            aux.append(alignprops.aux_field("MM", "Z", mm) + b"MLBC" + calls.to_bytes(4, "little") + rng.integers(0, 256, calls, dtype=np.uint8).tobytes())
        recs += records_block(pos[a:b], np.zeros(b - a, np.int64), np.full(b - a, -1), np.concatenate([np.full((b - a, 1), ord("l"), np.uint8), digits(np.arange(a, b), 7)], axis=1),
                              bases.astype(np.uint8), aux)
    with open(os.path.join(d, "annotated.bam"), "wb") as f:
        f.write(alignprops.bgzf_compress(alignprops.encode_bam([("s1", contig_len)], recs)))
    meta["annotated"] = {"records": n_long, "contig_len": int(contig_len), "loci": len(cpg), "read": read}
    json.dump(meta, open(os.path.join(d, "methylation.json"), "w"))
    print("wrote", meta)


def session(bam, loci, props, readtype):
    from varlociraptor_amd import methylation
    t0 = time.perf_counter()
    n = len(loci)
    obs, lrec, res = methylation.device_observations(bam, loci, props, readtype, 0, member_capacity=max(1 << 16, 80 * n), name_capacity=1 << 26, key_capacity=1 << 16)
    wall = time.perf_counter() - t0
    assert res.status == 0, res.status
    s = list(res.seconds)
    stages = {"file read": s[0], "upload + inflate": s[1], "record split": s[2], "member pass": s[3], "fragment pass": s[4], "observations to the host": s[7]}
    return wall, stages, int(res.n_records), int(res.n_members), len(obs), hashlib.sha1(obs.tobytes() + lrec.tobytes()).hexdigest()[:12]


def restatement_rate(bam, loci, props, readtype, n_first):
    """records/s and observations/s of the Python restatement over the first n_first records and the loci they reach"""
    from varlociraptor_amd import alignprops, methylation
    from varlociraptor_amd.readwindows import read_bam
    import gzip
    import tempfile
    data = alignprops.inflate_bgzf(bam)
    # cut the decompressed BAM behind n_first records
    import struct
    l_text, = struct.unpack_from("<i", data, 4)
    o = 8 + l_text
    n_ref, = struct.unpack_from("<i", data, o)
    o += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<i", data, o)
        o += 8 + l_name
    k, last = 0, 0
    while o < len(data) and k < n_first:
        bs, = struct.unpack_from("<i", data, o)
        last, = struct.unpack_from("<i", data, o + 8)
        o += 4 + bs
        k += 1
    with tempfile.NamedTemporaryFile(suffix=".bam") as f:
        f.write(gzip.compress(bytes(data[:o]), 1))
        f.flush()
        t0 = time.perf_counter()
        recs = read_bam(f.name)[1]
        t1 = time.perf_counter()
    sub = [l for l in loci if l.start <= last] if o < len(data) else list(loci)      # (the whole file: every locus)
    rs = methylation.restate(recs, sub, props, readtype)
    t2 = time.perf_counter()
    n_obs = sum(len(x) for x in rs.per_locus)
    return {"records": k, "loci": len(sub), "observations": n_obs, "read_bam s": round(t1 - t0, 3), "restate s": round(t2 - t1, 3), "records/s": round(k / (t2 - t0)),
            "observations/s": round(n_obs / (t2 - t0))}


def measure(label, bam, loci, props, readtype, rounds, n_first):
    runs = [session(bam, loci, props, readtype) for _ in range(rounds + 1)][1:]
    wall = [r[0] for r in runs]
    med = statistics.median(wall)
    out = {"input": label, "read type": readtype, "records": runs[0][2], "loci": len(loci), "members": runs[0][3], "observations": runs[0][4], "digest": runs[0][5],
           "equal digests": len({r[5] for r in runs}) == 1, "rounds": rounds, "seconds": round(med, 4), "range": [round(min(wall), 4), round(max(wall), 4)],
           "records/s": round(runs[0][2] / med), "observations/s": round(runs[0][4] / med),
           "stages": {k: round(statistics.median([r[1][k] for r in runs]), 5) for k in runs[0][1]}}
    if n_first:
        out["restatement"] = restatement_rate(bam, loci, props, readtype, n_first)
    print(json.dumps(out), flush=True)


def run(d, rounds, fixtures):
    from varlociraptor_amd import alignprops, fragments, methylation
    meta = json.load(open(os.path.join(d, "methylation.json")))
    for kind, readtype, n_first in (("converted", "converted", 4000), ("annotated", "annotated", 60)):
        m = meta[kind]
        loci = [methylation.MethLocus(0, int(p)) for p in range(100, m["contig_len"] - 100, SPACING)]
        props = fragments.Props(m["read"] + 10, 60, m["read"])
        measure("synthetic %s: %d records of %d bases, a CpG every %d bases" % (kind, m["records"], m["read"], SPACING), os.path.join(d, kind + ".bam"), loci, props, readtype,
                rounds, n_first)
    if fixtures:
        import make_methylation_fixtures as tool
        for name in tool.CASES:
            _, bam, pj, rec, case, _ = tool.load_case(name)
            names = [c for c, _ in alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)[0]]
            measure(name, bam, [methylation.MethLocus(names.index(rec[0]), int(rec[1]) - 1)], fragments.props_of(pj), case["methylation_readtype"], rounds, 10 ** 9)


def sessions(strip_new, d=None, rounds=6):
    """the sessions every earlier commit had, on synthetic inputs (written into directory d once, reused by later processes): digest,
    member-pass and fragment-pass milliseconds"""
    import pickle
    import tempfile
    from varlociraptor_amd import abi
    if strip_new:
        for name in ("vlr_fragpileup_open_methylation", "vlr_methylation_tables"):
            abi.SIGNATURES.pop(name)
    import basecall_cases as bc
    import fragindel_cases as ic
    import fragment_cases as fc
    from varlociraptor_amd import fragments
    tmp = d or tempfile.mkdtemp()
    os.makedirs(tmp, exist_ok=True)
    ref = ic.contig()
    _, sites = ic.sites_of(ref)
    if os.path.exists(os.path.join(tmp, "inputs.pkl")):
        contigs, cands, props = pickle.load(open(os.path.join(tmp, "inputs.pkl"), "rb"))
    else:
        contigs, cands, recs, props = fc.synthetic(40000, 120)
        bc.write_case(tmp, "snv", contigs, recs)
        bc.write_case(tmp, "indel", {"i1": ref}, ic.pairs(ref, 2000))
        pickle.dump((contigs, cands, props), open(os.path.join(tmp, "inputs.pkl"), "wb"))
    bam, fa, ibam, ifa = (os.path.join(tmp, n) for n in ("snv.bam", "snv.fa", "indel.bam", "indel.fa"))
    loci = bc.loci_of(cands, contigs)
    ms = lambda v: "%.3f (%.3f .. %.3f)" % (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3)
    out = {}
    for label, call in (("plain", lambda: fragments.device_observations(bam, loci, props, member_capacity=1 << 21, name_capacity=1 << 24)),
                        ("realign", lambda: fragments.device_observations(bam, loci, props, realign=fragments.RealignSpec(), fasta=fa, member_capacity=1 << 21, name_capacity=1 << 24,
                                                                          evidence_capacity=1 << 18)),
                        ("indel", lambda: fragments.device_indel_observations(ibam, sites, ic.PROPS, True, fragments.RealignSpec(), ifa, 0))):
        member, frag, dig = [], [], set()
        for k in range(rounds + 1):
            got = call()
            res = got[2] if label != "indel" else got[4]
            assert res.status == 0
            if k:
                member.append(res.seconds[3])
                frag.append(res.seconds[4])
            dig.add(hashlib.sha1(b"".join(x.tobytes() for x in got if isinstance(x, np.ndarray))).hexdigest()[:12])
        out[label] = {"digest": sorted(dig), "member pass ms": ms(member), "fragment pass ms": ms(frag), "member median": statistics.median(member) * 1e3,
                      "fragment median": statistics.median(frag) * 1e3}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--make")
    ap.add_argument("--run")
    ap.add_argument("--records", type=int, default=1000000)
    ap.add_argument("--long-records", type=int, default=20000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--fixtures", action="store_true")
    ap.add_argument("--sessions", action="store_true")
    ap.add_argument("--strip-new", action="store_true")
    ap.add_argument("--dir", help="where --sessions keeps its inputs")
    a = ap.parse_args()
    if a.make:
        make(a.make, a.records, a.long_records)
    if a.run:
        run(a.run, a.rounds, a.fixtures)
    if a.sessions:
        sessions(a.strip_new, a.dir)


if __name__ == "__main__":
    main()
