"""Inputs shared by tests/test_altvariant_cases_host.py, tests/test_altvariants_host_program.py and tests/test_gpu_altvariants.py: a
contig of a few hundred bases with hand-placed multi-allelic sites, and reads that carry a chosen allele.

    DEL_AT   ... T G A C ...      two deletions at one POS: TGA>T (deletes GA) and TG>T (deletes G)
                                  a read with the G deleted   is T A C: 0 edits from TG>T, 1 from the reference (T G A C), 1 from TGA>T (T C)
                                  a read with the A deleted   is T G C: 1 edit from the reference, from TGA>T and from TG>T alike (the tie)
    MNV_AT   ... two bases        an MNV, an SNV and a second MNV at one POS
    INS_AT   ... one base         sixteen insertions at one POS: every one has fifteen competitors
    LONE_AT  ...                  a deletion alone at its POS: no competitor
"""
from __future__ import annotations

import random

import basecall_cases as bc
from varlociraptor_amd import fragments
from varlociraptor_amd import readwindows as rw

READ = 40
DEL_AT, MNV_AT, INS_AT, LONE_AT = 150, 90, 230, 40
PROPS = fragments.Props(45, 60, READ)      # (a window of 45: a read is a member of the site it was made for alone)
IPROPS = fragments.IndelProps((130.0, 12.0), 4, 4, 0.1)
INSERTS = [b"A", b"C", b"G", b"AC", b"CA", b"GT", b"TG", b"ACG", b"CGT", b"GTA", b"TAC", b"AACC", b"CCGG", b"GGTT", b"TTAA", b"ACGTA"]


def contig(n=400, seed=23):
    """random bases with T G A C at DEL_AT; the neighbours of the site are fixed too, so that no shifted alignment is as cheap as the
    intended one"""
    rng = random.Random(seed)
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    s[DEL_AT - 2:DEL_AT + 6] = b"CATGACTC"
    return bytes(s)


def two_deletions(ref):
    """(TGA>T, TG>T) as (contig, 0-based position, REF, ALT), in file order"""
    assert ref[DEL_AT:DEL_AT + 4] == b"TGAC"
    return [("a1", DEL_AT, b"TGA", b"T"), ("a1", DEL_AT, b"TG", b"T")]


def mnv_site(ref):
    """(an MNV, an SNV, a second MNV) at MNV_AT"""
    r2 = ref[MNV_AT:MNV_AT + 2]
    other = lambda b: bytes([next(c for c in b"ACGT" if c != b)])
    last = lambda b: bytes([next(c for c in b"TGCA" if c != b)])
    return [("a1", MNV_AT, r2, other(r2[0]) + other(r2[1])), ("a1", MNV_AT, r2[:1], last(r2[0])), ("a1", MNV_AT, r2, last(r2[0]) + last(r2[1]))]


def insertions(ref, n=16):
    return [("a1", INS_AT, ref[INS_AT:INS_AT + 1], ref[INS_AT:INS_AT + 1] + INSERTS[k]) for k in range(n)]


def lone_deletion(ref):
    return [("a1", LONE_AT, ref[LONE_AT:LONE_AT + 4], ref[LONE_AT:LONE_AT + 1])]


def sites_and_windows(ref, cands, window=64):
    """(IndelSite per candidate in the order given, competitor windows per candidate) of deletion / insertion candidates: the grouping
    and the windows as the front end builds them"""
    sites = [fragments.IndelSite(0, rw.indel_locus(ref, pos, r, a, window)) for _, pos, r, a in cands]
    comp = [[fragments.competitor_window(ref, cands[j][1], cands[j][2], cands[j][3], window) for j in g] for g in fragments.alt_variant_groups(cands)]
    return sites, comp


def del_read(ref, start, which, name, length=READ, **kw):
    """a read of `length` bases from `start` over DEL_AT: which = "ref", "G" (the G deleted: the TG>T allele), "A" (the A deleted) or
    "GA" (both: the TGA>T allele), aligned with a D operation"""
    a = DEL_AT - start + 1          # bases up to and including the anchor T
    if which == "ref":
        cigar = [("M", length)]
    elif which == "G":
        cigar = [("M", a), ("D", 1), ("M", length - a)]
    elif which == "A":
        cigar = [("M", a + 1), ("D", 1), ("M", length - a - 1)]
    else:
        cigar = [("M", a), ("D", 2), ("M", length - a)]
    return bc.make_read(ref, start, cigar, name=name, **kw)


def del_reads(ref, which, n, first=118, flag=0, prefix="d"):
    """n single reads over DEL_AT, coordinate sorted (they start at first, first + 1, ... and wrap so that each keeps 8 bases on either
    side of the site)"""
    starts = sorted(first + k % 24 for k in range(n))
    return [del_read(ref, p, which, "%s%s%04d" % (prefix, which, k), flag=flag if k % 2 else flag | 0x10) for k, p in enumerate(starts)]


def plain_reads(ref, at, n, prefix, width=24, length=READ):
    """n reads of the reference that enclose the position `at`, coordinate sorted, no I / D operation"""
    starts = sorted(at - length + 8 + k % width for k in range(n))
    return [bc.make_read(ref, p, [("M", length)], name="%s%04d" % (prefix, k), flag=0x10 if k % 3 == 0 else 0) for k, p in enumerate(starts)]


def ins_reads(ref, n, k_ins=3, prefix="i"):
    """n reads over INS_AT that carry insertion INSERTS[k_ins] (aligned with an I operation, the inserted bases set), coordinate sorted"""
    ins = INSERTS[k_ins]
    out = []
    for k, p in enumerate(sorted(INS_AT - READ + 12 + k % 16 for k in range(n))):
        a = INS_AT - p + 1
        edits = {a + j: chr(ins[j]) for j in range(len(ins))}
        out.append(bc.make_read(ref, p, [("M", a), ("I", len(ins)), ("M", READ - a - len(ins))], edits=edits, name="%s%04d" % (prefix, k), flag=0x10 if k % 2 else 0))
    return out


def by_start(records):
    """encoded records sorted by their position (bytes 8 .. 12 of an encoded record, behind block_size and refID), stable"""
    import struct
    return sorted(records, key=lambda r: struct.unpack_from("<i", r, 8)[0])
