"""Inputs shared by tests/test_methylation_host.py and tests/test_gpu_methylation.py: hand-made records for every rule of
varlociraptor_amd/methylation.py (csrc/vlr_methylation.h) at one CpG of a random contig, with the observation each fragment must
give stated from its sequence — never from the code under test —, a long synthetic annotated record, the packing of a methylation
session's input for the host program, and the reference's methylation testcases held under tests/golden/bam/
(tools/make_methylation_fixtures.py).

An expectation is (prob_ref, prob_alt, strand, read position) of the fragment, None for no observation, or ("status", bit) where the
reference fails.  A probability is a sum of terms: ("call", q) = ln(1 - 10^(-q/10)), ("miscall", q) = -q ln(10) / 10 + ln 0.3333,
("any",) = ln 0.25, ("meth", ml) = ln((ml + 0.5) / 256), ("unmeth", ml) = ln(1 - (ml + 0.5) / 256) as the tables hold it, ("ln0",),
("ln1",); `resolve` turns them into numbers on the tables it is given."""
from __future__ import annotations

import math
import os
import random
import struct

import numpy as np

import basecall_cases as bc
from varlociraptor_amd import abi, alignprops, fragments, methylation

A = alignprops.aux_field
CPG = 100                       # REF[100:102] = CG: the candidate's POS - 1
READ = 30
PROPS = fragments.Props(200, 60, 40)
FIXTURES = ("test_prinz_call_meth_1", "test_prinz_call_meth_2", "test_prinz_af_scan", "test_mapq_meth", "test_prinz_pacbio_zero")
RECORDED_COUNTS = {"test_prinz_call_meth_1": 2, "test_prinz_call_meth_2": 13, "test_prinz_af_scan": 20, "test_mapq_meth": 14, "test_prinz_pacbio_zero": 24}
PACBIO_WITH_FLAG_RULE = 22      # the annotated case under read_invalid, which its recordings predate


def contig(n=220, seed=3):
    rng = random.Random(seed)
    s = bytearray(rng.choice(b"ACGT") for _ in range(n))
    s[CPG:CPG + 2] = b"CG"
    return bytes(s)


REF = contig()
FWD, REV = abi.STRAND_FORWARD, abi.STRAND_REVERSE


def resolve(terms, t, mt):
    if terms is None:
        return None
    total = 0.0
    for term in terms:
        k = term[0]
        total += {"call": lambda: t.call[term[1]], "miscall": lambda: t.miscall[term[1]] + t.confusion, "any": lambda: t.any, "meth": lambda: mt.ln_meth[term[1]],
                  "unmeth": lambda: mt.ln_unmeth[term[1]], "ln0": lambda: -math.inf, "ln1": lambda: 0.0}[k]()
    return total


class Cases:
    """fragments of one read type at the CpG, in file order, each with its expectation"""
    def __init__(self, readtype):
        self.readtype = readtype
        self.records = []
        self.expect = {}            # name -> expectation
        self.first = {}             # name -> ordinal of the fragment's first record

    def add(self, name, expect, *recs):
        assert name not in self.expect
        self.expect[name] = expect
        self.first[name] = len(self.records)
        self.records += list(recs)

    def read(self, name, pos, cigar=None, edits=None, **kw):
        return bc.make_read(REF, pos, cigar or [("M", READ)], edits, name=name, **kw)


def at(pos, rev=False):
    """read index of the CpG's C (the G for reverse orientation) in an all-M read that starts at pos"""
    return CPG + (1 if rev else 0) - pos


def converted_cases():
    c = Cases("converted")
    C30, M30 = [("call", 30)], [("miscall", 30)]
    # the accepted flags, each alone: 0 / 99 / 147 are of forward orientation (read at the C), 16 / 83 / 163 of reverse orientation (read at the G);
    # the strand is the record's reverse flag
    for flag, rev, strand in ((0, False, FWD), (99, False, FWD), (147, False, REV), (16, True, REV), (83, True, REV), (163, True, FWD)):
        c.add("flag_%d" % flag, (M30, C30, strand, at(85, rev)), c.read("flag_%d" % flag, 85, flag=flag))
    for flag in (65, 97, 2048, 2064):
        c.add("flag_%d" % flag, None, c.read("flag_%d" % flag, 85, flag=flag))
    # converted (unmethylated) bases: T forward, A reverse
    c.add("fwd_T", (C30, M30, FWD, at(80)), c.read("fwd_T", 80, edits={at(80): "T"}))
    c.add("rev_A", (C30, M30, REV, at(80, True)), c.read("rev_A", 80, edits={at(80, True): "A"}, flag=16))
    # pairs that both cover the CpG: supports add, strands of both records -> both, two alt supports at different read positions -> none
    c.add("pair_99_147", ([("miscall", 30)] * 2, [("call", 30)] * 2, abi.STRAND_BOTH, None), c.read("pair_99_147", 80, flag=99, mtid=0, mpos=90),
          c.read("pair_99_147", 90, flag=147, mtid=0, mpos=80))
    c.add("pair_83_163", ([("miscall", 30)] * 2, [("call", 30)] * 2, abi.STRAND_BOTH, None), c.read("pair_83_163", 78, flag=163, mtid=0, mpos=88),
          c.read("pair_83_163", 88, flag=83, mtid=0, mpos=78))
    # a reverse-orientation record that ends at start + 1 encloses the locus and has no base at the G; a forward one that ends there reads the C
    c.add("rev_ends_at_G", None, c.read("rev_ends_at_G", CPG + 1 - READ, flag=16))
    c.add("fwd_ends_at_G", (M30, C30, FWD, READ - 1), c.read("fwd_ends_at_G", CPG + 1 - READ))
    c.add("fwd_starts_at_C", (M30, C30, FWD, 0), c.read("fwd_starts_at_C", CPG))
    c.add("rev_starts_at_C", (M30, C30, REV, 1), c.read("rev_starts_at_C", CPG, flag=16))
    # the position inside a deletion and inside a reference skip
    c.add("in_D", None, c.read("in_D", 90, [("M", 8), ("D", 6), ("M", 20)]))
    c.add("in_N", None, c.read("in_N", 90, [("M", 8), ("N", 6), ("M", 20)]))
    c.add("behind_D", (M30, C30, FWD, 8), c.read("behind_D", 88, [("M", 8), ("D", 4), ("M", 20)]))
    # mutations: A / G forward, C / T reverse
    for b in "AG":
        c.add("fwd_mut_" + b, None, c.read("fwd_mut_" + b, 80, edits={at(80): b}))
    for b in "CT":
        c.add("rev_mut_" + b, None, c.read("rev_mut_" + b, 80, edits={at(80, True): b}, flag=16))
    # N alone: ln 0.25 twice, no strand, no observation; beside an informative mate the supports add and the mate's position stands
    c.add("N_alone", None, c.read("N_alone", 80, edits={at(80): "N"}))
    c.add("N_with_mate", ([("any",), ("miscall", 30)], [("any",), ("call", 30)], REV, at(92)), c.read("N_with_mate", 82, edits={at(82): "N"}, flag=99, mtid=0, mpos=92),
          c.read("N_with_mate", 92, flag=147, mtid=0, mpos=82))
    # qualities 0 and 93 at the position
    q = lambda pos, v: bytes([30] * at(pos) + [v] + [30] * (READ - at(pos) - 1))
    c.add("q0", ([("miscall", 0)], [("call", 0)], FWD, at(81)), c.read("q0", 81, qual=q(81, 0)))
    c.add("q93_T", ([("call", 93)], [("miscall", 93)], FWD, at(81)), c.read("q93_T", 81, edits={at(81): "T"}, qual=q(81, 93)))
    # SI:Z at the read position: '-' on a forward record, '+' on a reverse one
    si = lambda pos, ch, rev=False: "".join(ch if i == at(pos, rev) else ("+" if ch != "+" else "-") for i in range(READ))
    c.add("si_minus", (M30, C30, REV, at(83)), c.read("si_minus", 83, aux=A("SI", "Z", si(83, "-"))))
    c.add("si_plus_rev", (M30, C30, FWD, at(83, True)), c.read("si_plus_rev", 83, flag=16, aux=A("SI", "Z", si(83, "+", True))))
    # a MAPQ of 0 in a pair drops the fragment
    c.add("pair_mapq0", None, c.read("pair_mapq0", 80, flag=99, mtid=0, mpos=90, mapq=0), c.read("pair_mapq0", 90, flag=147, mtid=0, mpos=80))
    return c


def mm_aux(mm, ml, mm_tag="MM", ml_tag="ML", mm_type="Z", ml_sub="C"):
    out = b""
    if mm is not None:
        out += A(mm_tag, mm_type, mm)
    if ml is not None:
        out += A(ml_tag, "B", (ml_sub, list(ml)))
    return out


def annotated_cases():
    c = Cases("annotated")
    pos = 85
    seq = REF[pos:pos + READ].decode()
    q, qr = at(pos), at(pos, True)
    k = seq[:q].count("C")                    # the CpG's C is the k-th C of the read
    total_c = seq.count("C")
    kr = seq[qr + 1:].count("G")              # the G is the kr-th G counted from the read's end
    total_g = seq.count("G")
    assert 1 <= k < total_c - 1 and 0 <= kr < total_g
    hit = lambda ml, strand=FWD, p=q: ([("unmeth", ml)], [("meth", ml)], strand, p)
    outside = ([("ln1",)], [("ln0",)], FWD, q)

    def one(name, expect, aux, flag=0, edits=None):
        c.add(name, expect, c.read(name, pos, edits=edits, flag=flag, aux=aux))
    one("plain", hit(200), mm_aux("C+m,%d;" % k, [200]))
    one("h_before_m", hit(200), mm_aux("C+h,0,1;C+m,%d;" % k, [10, 20, 200]))
    one("m_question", hit(3), mm_aux("C+m?,%d;" % k, [3]))
    one("m_dot", hit(255), mm_aux("C+m.,%d;" % k, [255]))
    one("minus_strand_header", hit(128), mm_aux("C-m,%d;" % k, [128]))
    c.add("Mm_beside_MM", hit(200), c.read("Mm_beside_MM", pos, aux=mm_aux("C+m,%d;" % (k + 1), [7]) + mm_aux("C+m,%d;" % k, [200], "Mm", "Ml")))
    one("ML_missing", None, mm_aux("C+m,%d;" % k, None))
    one("ML_too_short", hit(0), mm_aux("C+m,0,%d;" % (k - 1), [77]))
    one("ML_subtype_S", None, mm_aux("C+m,%d;" % k, [200], ml_sub="S"))
    one("MM_type_A", None, A("MM", "A", "C") + mm_aux(None, [200]))
    one("MM_empty", outside, mm_aux("", [200]))
    one("block_without_comma", hit(200), mm_aux("C+m;C+m,%d;" % k, [200]))
    one("unparsable_token", hit(200), mm_aux("C+m,x,%d,-1;" % k, [200]))
    one("two_blocks_one_position", hit(200), mm_aux("C+m,%d;C+m,%d;" % (k, k), [100, 200]))
    one("past_last_C_before", None, mm_aux("C+m,%d;" % total_c, [200]))
    one("past_last_C_behind", None, mm_aux("C+m,%d,%d;" % (k, total_c), [200, 9]))
    one("past_last_C_later_block", None, mm_aux("C+m,%d;C+m,%d;" % (k, total_c), [200, 9]))
    one("last_C_exactly", outside, mm_aux("C+m,%d;" % (total_c - 1), [200]))
    one("not_in_map", outside, mm_aux("C+m,%d;" % (k + 1), [200]))
    one("no_MM_tag", None, b"")
    one("reverse_orientation", hit(200, REV, qr), mm_aux("C+m,%d;" % kr, [200]), flag=16)
    one("reverse_not_in_map", ([("ln1",)], [("ln0",)], REV, qr), mm_aux("C+m,%d;" % (kr + 1), [200]), flag=16)
    # mutations: G / A / T forward, C / A / T reverse (the map of the mutated read is still usable: deltas stay below its C's / G's)
    for b in "GAT":
        one("fwd_mut_" + b, None, mm_aux("C+m,0;", [200]), edits={q: b})
    for b in "CAT":
        one("rev_mut_" + b, None, mm_aux("C+m,0;", [200]), flag=16, edits={qr: b})
    one("fwd_N", outside, mm_aux("C+m,0;", [200]), edits={q: "N"})
    for flag in (65, 2048):
        one("flag_%d" % flag, None, mm_aux("C+m,%d;" % k, [200]), flag=flag)
    # a mapless record whose mate has a map: the mate's support alone; both mates with a map: the supports add
    c.add("mapless_with_mate", hit(200, REV), c.read("mapless_with_mate", pos, flag=99, mtid=0, mpos=pos), c.read("mapless_with_mate", pos, flag=147, mtid=0, mpos=pos,
                                                                                                              aux=mm_aux("C+m,%d;" % k, [200])))
    c.add("both_mates", ([("unmeth", 200), ("unmeth", 100)], [("meth", 200), ("meth", 100)], abi.STRAND_BOTH, q),
          c.read("both_mates", pos, flag=99, mtid=0, mpos=pos, aux=mm_aux("C+m,%d;" % k, [200])), c.read("both_mates", pos, flag=147, mtid=0, mpos=pos, aux=mm_aux("C+m,%d;" % k, [100])))
    return c


def error_cases():
    """{name: (read type, records, status bit)}: what the reference fails on"""
    c = Cases("converted")
    return {"leading_N": ("converted", [c.read("leading_N", 80, [("N", 3), ("M", 27)])], abi.BASEPILEUP_HIT_LEADING_REFSKIP),
            "si_invalid": ("converted", [c.read("si_invalid", 83, aux=A("SI", "Z", "x" * READ))], abi.BASEPILEUP_HIT_INVALID_STRAND_INFO),
            "si_too_short": ("converted", [c.read("si_too_short", 83, aux=A("SI", "Z", "+++"))], abi.BASEPILEUP_HIT_READ_POS_OUT_OF_BOUNDS),
            "leading_N_annotated": ("annotated", [c.read("leading_N_annotated", 80, [("N", 3), ("M", 27)], aux=mm_aux("C+m,0;", [1]))], abi.BASEPILEUP_HIT_LEADING_REFSKIP)}


def all_cases():
    return [converted_cases(), annotated_cases()]


LOCI = [methylation.MethLocus(0, CPG)]


def write_bam(tmp, name, records, contigs=None, member_bytes=0xff00):
    return bc.write_case(tmp, name, contigs or {"m1": REF}, records, member_bytes)


def check_expectations(cases, obs, t, mt):
    """the observations (fragments.FragObs, name order) of the cases' records against the stated expectations"""
    by_left = {o.left: o for o in obs}
    assert len(by_left) == len(obs)
    firsts = set(cases.first.values())
    assert set(by_left) <= firsts, "an observation whose first record starts no fragment"
    for name, exp in cases.expect.items():
        o = by_left.get(cases.first[name])
        if exp is None:
            assert o is None, (cases.readtype, name, o)
            continue
        assert o is not None, (cases.readtype, name)
        pr, pa, strand, pos = exp
        assert (o.prob_ref, o.prob_alt, o.strand, o.read_position, o.third_allele, o.status) == (resolve(pr, t, mt), resolve(pa, t, mt), strand, pos, 0, 0), (cases.readtype, name, o)


# ---------------------------------------------------------------------------------------------- a long annotated record
def long_record(rev, n=20000, n_loci=300, seed=17):
    """(contig, record, loci, {locus start: ML value or None}) — one annotated record of n bases, all M, over a contig with n_loci CpGs it
    covers; every third CpG is in its 5mC map, in one block."""
    rng = random.Random(seed)
    s = bytearray(rng.choice(b"AT") for _ in range(n + 200))
    starts = sorted(rng.sample(range(120, n + 60, 2), n_loci))
    starts = [p for i, p in enumerate(starts) if i == 0 or p - starts[i - 1] >= 2]
    for p in starts:
        s[p:p + 2] = b"CG"
    ref = bytes(s)
    pos = 100
    seq = ref[pos:pos + n].decode()
    target = "G" if rev else "C"
    where = [i for i, ch in enumerate(seq) if ch == target]
    if rev:
        where.reverse()
    index = {qp: i for i, qp in enumerate(where)}
    called, deltas, mls, last = {}, [], [], -1
    order = starts if not rev else list(reversed(starts))
    for j, p in enumerate(order):
        if j % 3:
            continue
        i = index[p + (1 if rev else 0) - pos]
        deltas.append(i - last - 1)
        last = i
        mls.append((7 * j + 3) % 256)
        called[p] = mls[-1]
    aux = A("MM", "Z", "C+m," + ",".join(map(str, deltas)) + ";") + A("ML", "B", ("C", mls))
    rec = alignprops.encode_record(0, pos, 60, 16 if rev else 0, [("M", n)], seq, aux=aux, name="long", qual=bytes([30] * n))
    return ref, rec, [methylation.MethLocus(0, p) for p in starts], {p: called.get(p) for p in starts}


# ---------------------------------------------------------------------------------------------- the host program
def pack_host_input(readtype, loci, records, props=PROPS):
    blob = b"VFMH" + struct.pack("<iqiiq", methylation.READTYPES[readtype], props.window, props.max_mapq, props.max_read_len, len(loci))
    blob += np.array([l.ref_id for l in loci], np.int32).tobytes() + np.array([l.start for l in loci], np.int64).tobytes()
    starts = np.concatenate(([0], np.cumsum([len(r) for r in records]))).astype(np.uint64)
    return blob + struct.pack("<q", len(records)) + starts.tobytes() + b"".join(records)


def parse_host_output(data, n_loci, n_records):
    """(call, miscall, ln_meth, ln_unmeth, observations, locus records, record classes)"""
    tabs = np.frombuffer(data, "<f8", 1024)
    n_obs, = struct.unpack_from("<q", data, 8192)
    o = 8200
    obs = np.frombuffer(data, abi.FRAGPILEUP_OBS_DTYPE, n_obs, o)
    o += n_obs * abi.FRAGPILEUP_OBS_DTYPE.itemsize
    loc = np.frombuffer(data, abi.FRAGPILEUP_LOCUS_DTYPE, n_loci, o)
    o += n_loci * abi.FRAGPILEUP_LOCUS_DTYPE.itemsize
    cls = np.frombuffer(data, np.uint8, n_records, o)
    assert o + n_records == len(data)
    return tabs[:256], tabs[256:512], tabs[512:768], tabs[768:], obs, loc, cls


# ---------------------------------------------------------------------------------------------- the held testcases
def golden_bam_dir():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam")


def max_f32_deviation():
    """the bound tools/make_methylation_fixtures.py measured against the recordings (METHYLATION.md)"""
    for line in open(os.path.join(golden_bam_dir(), "METHYLATION.md")):
        if line.startswith("MAX_F32_DEVIATION = "):
            return float(line.split("=")[1])
    raise AssertionError("METHYLATION.md holds no MAX_F32_DEVIATION")
