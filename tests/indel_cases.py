"""Inputs shared by tests/test_indel_cases_host.py, tests/test_indelpileup_host.py and tests/test_gpu_indelpileup.py: hand-made records
and loci for every rule of varlociraptor_amd/readwindows.py `evidence` (the restatement of csrc/vlr_indelpileup.h), a seeded synthetic
set, and the expectation both the host program and the kernels are compared with.  Records are encoded with alignprops' BAM writer,
as tests/basecall_cases.py does."""
from __future__ import annotations

import os
import random

import numpy as np

from basecall_cases import make_read, write_case   # noqa: F401
from varlociraptor_amd import readwindows as rw

WINDOW = 64


def _contig(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


# one contig of a few hundred bases, lower case around the first deletion, and a second short one
_C1 = _contig(600, 5)
C1 = _C1[:100] + _C1[100:140].lower() + _C1[140:]
C2 = _contig(80, 6)
HAND_CONTIGS = {"c1": C1, "c2": C2}
U1, U2 = C1.upper(), C2.upper()


def _other(seq, n, seed):
    """n bases that differ from seq[k] at every k"""
    rng = random.Random(seed)
    return bytes(rng.choice([b for b in b"ACGT" if b != (seq[k] if k < len(seq) else 0)]) for k in range(n))


# label -> (contig, 0-based position, REF, ALT)
HAND_CANDIDATES = {
    "del_clamps_at_0": ("c1", 20, U1[20:23], U1[20:21]),                       # locus [20, 22): the ref window starts at 0
    "del": ("c1", 120, U1[120:124], U1[120:121]),                              # locus [120, 123), inside the lower-case bases
    "ins": ("c1", 200, U1[200:201], U1[200:201] + b"GAT"),                     # locus [200, 201)
    "repl": ("c1", 260, U1[260:263], _other(U1[260:263], 5, 1)),               # locus [260, 263)
    "long_del": ("c1", 300, U1[300:451], U1[300:301]),                         # locus [300, 450): 150 bases, longer than a read
    "ins_clamps_at_end": ("c1", 585, U1[585:586], U1[585:586] + b"CC"),        # the ref window ends at the contig's end
    "del_near_end": ("c1", 590, U1[590:596], U1[590:591]),                     # the alt window would read behind the contig
    "ins_c2": ("c2", 30, U2[30:31], U2[30:31] + b"TT"),
}


def hand_records():
    """{label: record}, in file order"""
    out = {}

    def add(label, pos, cigar, edits=None, contig=C1, **kw):
        out[label] = make_read(contig, pos, cigar, edits, name=label, **kw)
    add("plain_over_del", 90, [("M", 60)])
    add("carries_del", 100, [("M", 21), ("D", 3), ("M", 40)])                  # read_pos(123) lands inside the deletion
    add("lead_softclip", 112, [("S", 5), ("M", 40)])
    add("lead_clip_longer_than_pos", 3, [("S", 10), ("M", 40)])                # rpos = max(0, 3 - 10)
    add("trail_softclip", 165, [("M", 30), ("S", 8)])                          # reaches ins [200, 201) by its clip alone
    add("hard_clips", 100, [("H", 5), ("M", 50), ("H", 3)])
    add("hard_then_soft_clip", 110, [("H", 4), ("S", 3), ("M", 40)])
    add("carries_ins", 180, [("M", 21), ("I", 3), ("M", 30)])                  # an I at the locus
    add("D_covers_locus_start", 100, [("M", 15), ("D", 10), ("M", 30)])        # read_pos(120) lands inside the deletion
    add("leading_D", 100, [("D", 3), ("M", 40)])
    add("begins_with_N", 100, [("N", 5), ("M", 40)])                           # LEADING_REFSKIP
    add("inside_long_del", 340, [("M", 50)])                                   # branch 4, enclosed
    add("inside_long_del_130", 310, [("M", 130)])                              # branch 4, a read window of 127
    add("N_spans_long_del", 290, [("M", 5), ("N", 170), ("M", 20)])            # branch 4, not enclosed: NO_OVERLAP
    add("clip_reaches_long_del", 258, [("M", 40), ("S", 10)])                  # only the clip reaches [300, 450): branch 2 through the clip
    add("covers_repl_start_only", 222, [("M", 40)])                            # branch 2
    add("covers_repl_end_only", 262, [("M", 40)])                              # branch 3
    add("window_1", 300, [("M", 1)])
    add("window_63", 300, [("M", 63)])
    add("window_64", 300, [("M", 100)])
    add("window_65", 299, [("M", 100)])
    add("window_128_odd_trim", 100, [("M", 200)])                              # 129 bases around ins: exceed 1, nothing off the front
    add("window_trim_odd_25", 280, [("M", 60), ("I", 3), ("M", 140)])          # encloses long_del: 153 bases, max_window 0, 12 / 13 off
    add("flag_secondary", 90, [("M", 60)], flag=0x100)
    add("flag_qcfail", 90, [("M", 60)], flag=0x200)
    add("flag_duplicate", 90, [("M", 60)], flag=0x400)
    add("flag_supplementary", 90, [("M", 60)], flag=0x800)
    add("flag_unmapped", 90, [("M", 60)], flag=0x4)
    add("mapq_0", 170, [("M", 60)], mapq=0, flag=0x10)
    add("paired_first", 170, [("M", 60)], flag=0x41)
    add("on_c2", 10, [("M", 40)], contig=C2, tid=1)
    add("on_c2_behind", 40, [("M", 30)], contig=C2, tid=1)
    add("near_end", 540, [("M", 60)])
    add("quals", 95, [("M", 50)], {25: "N"}, qual=bytes((7 * k) % 94 for k in range(50)))
    add("empty_seq", 121, [("M", 0)], qual=b"")                                 # inside del, no bases: a read window shorter than 1
    return out


def loci_of(candidates, contigs, window=WINDOW, names=None):
    """(IndelLocus list, ref ids, order) sorted by (ref_id, start); order[j] = index of sorted locus j in `candidates`; `names`: the
    contigs of the BAM header when they are not the keys of `contigs`"""
    names = list(names or contigs)
    cands = list(candidates)
    loci = [rw.indel_locus(contigs[c].upper(), pos, ref, alt, window) for c, pos, ref, alt in cands]
    rid = [names.index(c) for c, _, _, _ in cands]
    order = sorted(range(len(loci)), key=lambda k: (rid[k], loci[k].start))
    return [loci[k] for k in order], [rid[k] for k in order], order


def expected(bam, contigs, loci, rid, window=WINDOW, first_ordinal=0, names=None):
    """[(sorted locus index, Evidence)] locus-major, record order within a locus: what vlr_indelpileup_read hands out"""
    _, recs = rw.read_bam(bam)
    names = list(names or contigs)
    out = []
    for j, (loc, r) in enumerate(zip(loci, rid)):
        out += [(j, e) for e in rw.evidence(recs, contigs[names[r]], loc, window, first_ordinal, ref_id=r)]
    return out


def hit_keys(arr):
    """the descriptor fields of a hit array (abi.INDELPILEUP_HIT_DTYPE) as tuples, comparable with evidence_keys"""
    return [(int(h["locus"]), int(h["record"]), int(h["status"]), (int(h["read_begin"]), int(h["read_begin"]) + int(h["read_len"])),
             (int(h["ref_begin"]), int(h["ref_begin"]) + int(h["ref_len"])), int(h["flag"]), int(h["mapq"])) for h in arr]


def evidence_keys(exp):
    return [(j, e.record, e.status, e.read_interval, e.ref_interval, e.flag, e.mapq) for j, e in exp]


def pair_batch(exp, loci):
    """the PairBatch of an expectation: pairs 2e = (ref allele, read), 2e + 1 = (alt allele, read)"""
    from varlociraptor_amd.realign import PairBatch
    pb = PairBatch()
    for j, e in exp:
        pb.add(e.ref_allele, e.read_window, e.quals, -1)
        pb.add(loci[j].alt_allele if e.status == 0 else b"", e.read_window, e.quals, -1)
    return pb


# ---------------------------------------------------------------------------------------------- seeded synthetic set
def synthetic(n_records=260, n_loci=40, seed=23):
    """(contigs, candidates, records): reads of 20-70 bases (a few of 130-260) on contig s1 with M, I, D, N, S, H, =, X operations, now
    and then a leading D or N, mismatches, Ns and mixed qualities, an unsorted tail and every flag; indel candidates of all three kinds
    on s1 (lower case in places) and a few on s2, a contig with two reads."""
    rng = random.Random(seed)
    s1 = bytearray(rng.choice(b"ACGT") for _ in range(2000))
    for a in (300, 900, 1500):
        s1[a:a + 80] = bytes(s1[a:a + 80]).lower()
    contigs = {"s1": bytes(s1), "s2": bytes(rng.choice(b"ACGT") for _ in range(300))}
    cands = []
    for k in range(n_loci):
        c = "s1" if k % 8 else "s2"
        u = contigs[c].upper()
        kind = rng.choice("DIR")
        pos = rng.randrange(0, len(u) - 40)
        if k == 1:
            kind, pos = "D", 1                      # ref window clamps at 0
        if k == 2:
            kind, pos = "I", len(u) - 3             # ref window clamps at the end
        if k == 3:
            kind, pos = "D", 1000                   # [1000, 1090): longer than the short reads
        if kind == "D":
            dl = rng.randint(1, 12) if k != 3 else 90
            cands.append((c, pos, u[pos:pos + dl + 1], u[pos:pos + 1]))
        elif kind == "I":
            cands.append((c, pos, u[pos:pos + 1], u[pos:pos + 1] + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 10)))))
        else:
            rl, al = rng.randint(2, 8), rng.randint(1, 9)
            if rl == al:
                al += 1
            cands.append((c, pos, u[pos:pos + rl], _other(u[pos:pos + rl], al, k)))
    recs, starts = [], sorted(rng.randrange(0, 1900) for _ in range(n_records))
    tail = n_records // 10
    starts = starts[:-tail] + [rng.randrange(0, 1900) for _ in range(tail)]
    for k, pos in enumerate(starts):
        target = rng.randint(130, 260) if k % 9 == 0 else rng.randint(20, 70)
        cigar, used = [], 0
        if rng.random() < 0.15:
            cigar.append(("H", rng.randint(1, 9)))
        if rng.random() < 0.25:
            l = rng.randint(1, 12)
            cigar.append(("S", l))
            used += l
        elif rng.random() < 0.06:
            cigar.append((rng.choice("DN"), rng.randint(1, 4)))
        while used < target:
            l = min(rng.randint(3, 40), target - used)
            cigar.append((rng.choice("MMM=X"), l))
            used += l
            if used < target and rng.random() < 0.5:
                op = rng.choice("IDDN")
                l = rng.randint(1, 6)
                cigar.append((op, l))
                if op == "I":
                    used += l
        if k == 7:
            pos, cigar = 1020, [("M", 40)]          # inside the 90-base deletion
        if k == 11:
            pos, cigar = 995, [("N", 3), ("M", 30)]  # begins with a reference skip, at that deletion
        if cigar[-1][0] in "IDN":
            cigar.append(("M", 2))
        if rng.random() < 0.25 and k not in (7, 11):
            cigar.append(("S", rng.randint(1, 10)))
        if rng.random() < 0.1:
            cigar.append(("H", 3))
        n = sum(l for op, l in cigar if op in "MIS=X")
        edits = {i: rng.choice("ACGTN") for i in range(n) if rng.random() < 0.04}
        qual = bytes(rng.choice([0, 2, 11, 20, 30, 37, 41, 93]) if rng.random() < 0.3 else 30 for _ in range(n))
        flag = rng.choice([0, 0x10, 0x41, 0x91, 0x800, 0x810]) if rng.random() < 0.9 else rng.choice([0x100, 0x200, 0x400, 0x4])
        ctg, tid = ("s2", 1) if k in (5, 6) else ("s1", 0)
        p = pos if tid == 0 else rng.randrange(0, 200)
        ref = contigs[ctg]
        if p + sum(l for op, l in cigar if op in "MDN=X") > len(ref):
            p = max(0, len(ref) - 400)
        recs.append(make_read(ref, p, cigar, edits, qual=qual, flag=flag, mapq=rng.choice([0, 20, 60]), name="q%d" % (k // 2), tid=tid))
    return contigs, cands, recs


def split_records(bam):
    """the encoded records of a BAM file, and its contigs"""
    import struct
    from varlociraptor_amd import alignprops
    d = alignprops.inflate_bgzf(bam)
    contigs, o = alignprops.bam_header(d, bam)
    records = []
    while o < len(d):
        bs, = struct.unpack_from("<I", d, o)
        records.append(bytes(d[o:o + 4 + bs]))
        o += 4 + bs
    return contigs, records


def fixture_case(golden_dir, name, tmp=None):
    """(bam, fasta, contigs {name: bytes}, header names, [candidate]) of a testcase of bam_pairs.BAM_CASES.  The testcases hold their
    reference without an index: with `tmp`, `fasta` is a copy of it there with its .fai (what vlr_indelpileup_open reads through)."""
    import glob
    from varlociraptor_amd import alignprops
    d = os.path.join(golden_dir, "bam", name)
    bam, = glob.glob(os.path.join(d, "*.bam"))
    var = open(os.path.join(d, "variant.tsv")).read().split("\n")[1].split("\t")
    fasta = os.path.join(d, "ref.fa")
    seqs = rw.read_fasta(fasta)
    if tmp is not None:
        fasta = os.path.join(str(tmp), name + ".ref.fa")
        alignprops.write_fasta(fasta, seqs)
    names, _ = split_records_header(bam)
    contigs = {n: seqs[n] for n in names if n in seqs}   # (a contig the FASTA lacks has no locus)
    return bam, fasta, contigs, names, [(var[0], int(var[1]) - 1, var[3].encode(), var[4].encode())]


def split_records_header(bam):
    from varlociraptor_amd import alignprops
    contigs, o = alignprops.bam_header(alignprops.inflate_bgzf(bam), bam)
    return [c for c, _ in contigs], o


def as_arrays(loci, rid):
    """the locus arrays of vlr_indelpileup_open / the host program"""
    alt_off = np.zeros(len(loci) + 1, np.uint64)
    alt_off[1:] = np.cumsum([len(l.alt_allele) for l in loci])
    return (np.array(rid, np.int32), np.array([l.start for l in loci], np.int64), np.array([l.end for l in loci], np.int64), alt_off,
            b"".join(bytes(l.alt_allele) for l in loci))
