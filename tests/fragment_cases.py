"""Inputs shared by tests/test_fragment_cases_host.py, tests/test_fragpileup_host.py and tests/test_gpu_fragpileup.py: hand-made BAM records
for every rule of varlociraptor_amd/fragments.py with the expected observations stated by hand (only the fields a case is about), a
seeded synthetic paired BAM, and loci with chosen member counts for the sort of the fragment kernel."""
from __future__ import annotations

import random
from dataclasses import dataclass
from typing import Dict, List

import basecall_cases as bc
from varlociraptor_amd import abi, alignprops, fragments

REF = bc.HAND_REF
A = alignprops.aux_field
FWD, REV, BOTH = abi.STRAND_FORWARD, abi.STRAND_REVERSE, abi.STRAND_BOTH
NONE = abi.FRAG_ORIENT_NONE


def snv(pos, alt=None):
    ref = REF[pos:pos + 1]
    if alt is None:
        alt = "A" if ref != b"A" else "C"
    return ("c1", pos, ref, alt.encode())


def rd(name, pos, cigar=(("M", 12),), alt_at=None, flag=0, **kw):
    """a read along REF; alt_at: the reference position that carries T (the alt base of snv(20, "T"))"""
    edits = kw.pop("edits", None) or {}
    if alt_at is not None:
        q, r = 0, pos
        for op, l in cigar:
            if op in "M=X":
                if r <= alt_at < r + l:
                    edits[q + alt_at - r] = kw.pop("base", "T")
                r += l
                q += l
            elif op in "IS":
                q += l
            elif op in "DN":
                r += l
    return bc.make_read(REF, pos, list(cigar), edits, flag=flag, name=name, **kw)


@dataclass
class Case:
    name: str
    records: List[bytes]
    candidates: list
    props: fragments.Props
    expect: List[List[Dict]]      # per candidate, per observation in name order: the fields the case is about


P30 = fragments.Props(30, 60, 12)
P10 = fragments.Props(10, 60, 12)
C20 = [snv(20, "T")]


def hand_cases() -> List[Case]:
    out = []

    def case(name, records, expect, candidates=C20, props=P30):
        out.append(Case(name, records, candidates, props, expect))
    # ---- pairing
    case("pair_both_enclose", [rd("p", 12, alt_at=20, flag=0x63, mtid=0, mpos=17), rd("p", 17, alt_at=20, flag=0x93, mtid=0, mpos=12)],
         [[dict(left=0, right=1, len_sum=24, min_mapq=60, strand=BOTH, read_position=None, orientation=abi.FRAG_F1R2, paired=True, is_max_mapq=True, alt=True)]])
    case("pair_left_only_encloses", [rd("p", 12, alt_at=20, flag=0x41), rd("p", 15, (("M", 4),), flag=0x81)],
         [[dict(left=0, right=1, len_sum=16, strand=FWD, read_position=8, alt=True)]])
    case("pair_right_only_encloses", [rd("p", 2, (("S", 2), ("M", 10)), flag=0x41, mapq=40), rd("p", 15, alt_at=20, flag=0x91)],
         [[dict(left=0, right=1, len_sum=24, min_mapq=40, softclipped=True, is_max_mapq=False, strand=REV, read_position=5, alt=True)]])
    case("three_records_last_wins", [rd("t", 2, (("M", 10),), flag=0x41), rd("t", 5, (("M", 10),), flag=0x81), rd("t", 15, alt_at=20, flag=0x881)],
         [[dict(left=0, right=2, len_sum=22, alt=True)]])
    case("first_and_last_in_template_skipped", [rd("t", 12, flag=0xC1), rd("t", 15, alt_at=20, flag=0xC1)],
         [[dict(left=0, right=None, len_sum=12, alt=False, read_position=8)]])
    # ---- MAPQ
    case("pair_with_mapq0_dropped", [rd("p", 12, alt_at=20, flag=0x41, mapq=0), rd("p", 15, alt_at=20, flag=0x91)], [[]])
    case("single_with_mapq0_kept", [rd("s", 12, alt_at=20, mapq=0)], [[dict(left=0, right=None, min_mapq=0, is_max_mapq=False)]])
    # ---- window edges (W = 10, locus [20, 21): members start in [10, 21))
    case("window_edges", [rd("out", 9, (("M", 5),), flag=0x41), rd("in", 10, (("M", 5),), flag=0x41), rd("in", 12, flag=0x81), rd("out", 12, flag=0x81),
                          rd("last", 20), rd("behind", 21)],
         [[dict(left=1, right=2, len_sum=17), dict(left=4, right=None, read_position=0), dict(left=3, right=None, len_sum=12)]], props=P10)
    case("locus_below_window", [rd("a", 0, alt_at=3, base="A"), rd("b", 3, alt_at=3, base="A")], [[dict(left=0, read_position=3, alt=True), dict(left=1, read_position=0)]],
         candidates=[snv(3, "A")])
    case("two_loci_share_members_one_locus_empty", [rd("p", 10, (("M", 12),), flag=0x41), rd("p", 18, flag=0x91)],
         [[dict(left=0, right=1, strand=BOTH)], [dict(left=0, right=1, strand=REV, read_position=6)], []], candidates=[snv(20, "T"), snv(24, "A"), snv(90)])
    # ---- names: byte order, a shorter name first
    case("name_order", [rd("r1a", 12), rd("r10", 12), rd("r1", 12), rd("abcdefgh1", 12), rd("abcdefgh0", 12), rd("abcdefghijklmnop2", 12), rd("abcdefghijklmnop1", 12),
                        rd("z" * 254, 12, flag=0x41), rd("z" * 254, 15, flag=0x91), rd("z" * 253 + "y", 12)],
         [[dict(left=4), dict(left=3), dict(left=6), dict(left=5), dict(left=2), dict(left=1), dict(left=0), dict(left=9, right=None), dict(left=7, right=8)]])
    # names are bytes, not text: 0xfe and 0xff are no UTF-8, differ, and order as bytes
    def renamed(rec, byte):
        b = bytearray(rec)
        b[37] = byte
        return bytes(b)
    case("name_bytes_not_utf8", [renamed(rd("q?", 12), 0xff), renamed(rd("q?", 12, flag=0x41), 0xfe), renamed(rd("q?", 15, flag=0x81), 0xfe)],
         [[dict(left=1, right=2), dict(left=0, right=None)]])
    # ---- orientation from the flags: (flag, mpos) of a read at 12
    ff = [(0x41 | 0x20, 30, abi.FRAG_F1R2), (0x41, 30, abi.FRAG_F1F2), (0x51, 30, abi.FRAG_R1F2), (0x51 | 0x20, 30, abi.FRAG_R1R2),
          (0x41 | 0x20, 5, abi.FRAG_R2F1), (0x41, 5, abi.FRAG_F2F1), (0x51, 5, abi.FRAG_F2R1), (0x51 | 0x20, 5, abi.FRAG_R2R1),
          (0x81 | 0x20, 30, abi.FRAG_F2R1), (0x41, 12, NONE), (0x40, 30, NONE), (0x49, 30, NONE)]
    case("orientation_flags", [rd("o%02d" % k, 12, flag=f, mtid=0, mpos=mp) for k, (f, mp, _) in enumerate(ff)] + [rd("other_contig", 12, flag=0x41, mtid=1, mpos=30)],
         [[dict(left=k, orientation=o) for k, (_, _, o) in enumerate(ff)] + [dict(left=len(ff), orientation=NONE)]])
    case("orientation_ro", [rd("a_single", 12, flag=0x61, mtid=0, mpos=30, aux=A("RO", "Z", "R1R2")), rd("b_double", 12, flag=0x61, mtid=0, mpos=30, aux=A("RO", "Z", "F1R2,F2R1")),
                            rd("c_not_a_string", 12, flag=0x61, mtid=0, mpos=30, aux=A("RO", "i", 3)), rd("d_none", 12, flag=0x61, mtid=0, mpos=30, aux=A("NM", "C", 0) + A("RO", "Z", "None")),
                            rd("e_disagree", 12, flag=0x61, mtid=0, mpos=15), rd("e_disagree", 15, flag=0x91, mtid=0, mpos=30)],
         [[dict(left=0, orientation=abi.FRAG_R1R2), dict(left=1, orientation=NONE), dict(left=2, orientation=abi.FRAG_F1R2), dict(left=3, orientation=NONE),
           dict(left=4, right=5, orientation=NONE, status=0)]])
    case("orientation_ro_invalid", [rd("x", 12, aux=A("RO", "Z", "F1R3")), rd("y", 12, flag=0x41, aux=A("RO", "Z", "")), rd("y", 15, flag=0x81)],
         [[dict(left=0, status=abi.FRAGPILEUP_OBS_INVALID_RO), dict(left=1, right=2, status=abi.FRAGPILEUP_OBS_INVALID_RO)]])
    # ---- soft clips
    case("softclip_behind_hardclip", [rd("a", 12, (("H", 3), ("S", 2), ("M", 12)), alt_at=20), rd("b", 12, (("M", 12), ("S", 1), ("H", 2))), rd("c", 12, (("H", 3), ("M", 12))),
                                      rd("d", 12, (("M", 6), ("I", 1), ("M", 6)))],
         [[dict(left=0, softclipped=True, read_position=13, len_sum=14), dict(left=1, softclipped=True), dict(left=2, softclipped=False, read_position=11), dict(left=3, softclipped=False)]])
    # ---- XA (max_read_len 12: buckets of 120 bases)
    case("xa_entries", [rd("a_none", 12), rd("b_trailing", 12, aux=A("XA", "Z", "chr2,+130,12M,0;")), rd("c_three_items", 12, aux=A("XA", "Z", "chr2,+130,12M;chr3,-500,12M,1;")),
                        rd("d_pair", 12, flag=0x41, aux=A("XA", "Z", "chr2,-239,12M,0;;chr9,x,12M,0;")), rd("d_pair", 15, flag=0x81, aux=A("XA", "Z", "chr3,+480,12M,0")),
                        rd("e_not_a_string", 12, aux=A("XA", "i", 1)), rd("f_more", 12, aux=A("XA", "Z", "chr2,+125,12M,0"))],
         [[dict(left=0, alt_loci=[], alt_locus=abi.ALTLOCUS_NONE), dict(left=1, alt_loci=[(b"chr2", 130)], alt_locus=abi.ALTLOCUS_MAJOR),
           dict(left=2, alt_loci=[(b"chr3", 500)], alt_locus=abi.ALTLOCUS_SOME), dict(left=3, right=4, alt_loci=[(b"chr2", 239), (b"chr3", 480)], alt_locus=abi.ALTLOCUS_MAJOR),
           dict(left=5, alt_loci=[], alt_locus=abi.ALTLOCUS_NONE), dict(left=6, alt_locus=abi.ALTLOCUS_MAJOR)]])
    case("xa_tie", [rd("a", 12, aux=A("XA", "Z", "chr2,+130,12M,0;chr3,+10,12M,0;")), rd("b", 12, aux=A("XA", "Z", "chr2,+131,12M,0;chr3,+11,12M,0;")), rd("c", 12)],
         [[dict(left=0, alt_locus=abi.ALTLOCUS_NONE), dict(left=1, alt_locus=abi.ALTLOCUS_NONE), dict(left=2, alt_locus=abi.ALTLOCUS_NONE)]])
    # ---- read position
    case("readpos_all_distinct", [rd("a", 12, alt_at=20), rd("b", 13, alt_at=20), rd("c", 14, alt_at=20)], [[dict(major=False)] * 3])
    case("readpos_tie", [rd("a", 12, alt_at=20), rd("b", 12, alt_at=20), rd("c", 14, alt_at=20), rd("d", 14, alt_at=20)], [[dict(major=False)] * 4])
    case("readpos_winner", [rd("a", 12, alt_at=20), rd("b", 12, alt_at=20), rd("c", 14, alt_at=20), rd("d", 12), rd("e", 14), rd("f", 14)],
         [[dict(major=True), dict(major=True), dict(major=False), dict(major=True, alt=False), dict(major=False), dict(major=False)]])
    # ---- strand
    case("merged_strand_none_dropped", [rd("n", 12, alt_at=20, base="N"), rd("p", 12, alt_at=20, base="N", flag=0x41), rd("p", 15, alt_at=20, base="N", flag=0x91), rd("q", 12)],
         [[dict(left=3)]])
    return out


def check_case(case: Case, tables_per_candidate, obs_per_candidate):
    """the stated fields of `case` against fragments.ObsTable / FragObs lists of its candidates (in candidate order)"""
    for want, tab, obs in zip(case.expect, tables_per_candidate, obs_per_candidate):
        assert len(obs) == len(want) == len(tab), (case.name, len(obs), len(want))
        for k, (w, o) in enumerate(zip(want, obs)):
            for f, v in w.items():
                if f == "alt":
                    got = o.prob_alt > o.prob_ref
                elif f == "major":
                    got = bool(tab.read_position_major[k])
                elif f == "alt_locus":
                    got = int(tab.alt_locus[k])
                else:
                    got = getattr(o, f)
                assert got == v, (case.name, k, f, got, v)


def write_case(tmp, case: Case, member_bytes=0xff00):
    return bc.write_case(tmp, case.name, {"c1": REF, "c2": REF[:50]}, case.records, member_bytes)


def loci_of(case: Case):
    """(loci sorted, order): order[j] = index of the j-th sorted locus among the case's candidates"""
    names = ["c1", "c2"]
    from varlociraptor_amd import basecalls
    loci = [basecalls.locus(REF, names.index(c), pos, ref, alt) for c, pos, ref, alt in case.candidates]
    order = sorted(range(len(loci)), key=lambda k: (loci[k].ref_id, loci[k].start))
    return [loci[k] for k in order], order


# ---------------------------------------------------------------------------------------------- seeded synthetic paired BAM
def synthetic(n_pairs=1500, n_loci=120, seed=5):
    """(contigs, candidates, records, props): pairs of 30-base reads with inserts of 40-120 bases on a contig of 4000 bases, coordinate
    sorted, a tenth of them with a soft clip, an insertion, a MAPQ of 0 or 20, an XA or RO tag, a duplicate flag, a third record of the
    name; SNVs and short MNVs every ~33 bases, reads carry the alt bases half of the time."""
    rng = random.Random(seed)
    ref = bytes(rng.choice(b"ACGT") for _ in range(4000))
    cands, alt_at = [], {}
    for k in range(n_loci):
        ln = rng.randint(2, 4) if k % 5 == 0 else 1
        pos = 20 + k * 33 + rng.randint(0, 5)
        r = ref[pos:pos + ln]
        alt = bytes(rng.choice([b for b in b"ACGT" if b != x]) for x in r)
        cands.append(("s1", pos, r, alt))
        for j in range(ln):
            alt_at[pos + j] = chr(alt[j])
    recs = []
    for k in range(n_pairs):
        p1 = rng.randrange(0, 3800)
        p2 = min(p1 + rng.randint(10, 90), 3960)
        name = "f%d" % rng.randrange(10 ** rng.randint(1, 6)) + ("x%d" % k)
        mq1, mq2 = (rng.choice([0, 20, 60]), rng.choice([0, 20, 60])) if rng.random() < 0.15 else (60, 60)
        for which, (pos, mpos, mq) in enumerate(((p1, p2, mq1), (p2, p1, mq2))):
            cigar = [("M", 30)]
            x = rng.random()
            if x < 0.05:
                cigar = [("S", 3), ("M", 27)]
            elif x < 0.1:
                cigar = [("M", 10), ("I", 2), ("M", 18)]
            elif x < 0.13:
                cigar = [("H", 4), ("M", 30), ("S", 2)]
            edits, r, q = {}, pos, 0
            for op, l in cigar:
                if op == "M":
                    for j in range(l):
                        if r + j in alt_at and rng.random() < 0.5:
                            edits[q + j] = alt_at[r + j]
                        elif rng.random() < 0.02:
                            edits[q + j] = rng.choice("ACGTN")
                    r += l
                    q += l
                elif op in "IS":
                    q += l
            flag = 0x1 | (0x40 if which == 0 else 0x80) | (0x20 if which == 0 else 0x10)
            if rng.random() < 0.03:
                flag ^= 0x30
            if rng.random() < 0.02:
                flag |= 0x400
            aux = b""
            if rng.random() < 0.05:
                aux += A("XA", "Z", "s%d,%s%d,30M,0;" % (rng.randint(1, 2), rng.choice("+-"), rng.randrange(0, 2000)))
            if rng.random() < 0.03:
                aux += A("RO", "Z", rng.choice(["F1R2", "F2R1", "F1R2,F2R1", "None"]))
            recs.append((pos, bc.make_read(ref, pos, cigar, edits, flag=flag, name=name, mapq=mq, mtid=0, mpos=mpos, aux=aux)))
            if which == 1 and rng.random() < 0.03:
                recs.append((pos + 1, bc.make_read(ref, pos + 1, [("M", 30)], {}, flag=0x881, name=name, mapq=60, mtid=0, mpos=mpos)))
    recs.sort(key=lambda x: x[0])
    return {"s1": ref, "s2": ref[:100]}, cands, [r for _, r in recs], fragments.Props(130, 60, 30)


def xa_heavy(n_reads, entries):
    """a hand Case: n_reads single reads over the SNV at 20, each with `entries` XA entries, all but the first read's in one bucket"""
    recs = [rd("h%04d" % k, 12, alt_at=20 if k % 2 else None, aux=A("XA", "Z", ("chr%d,+%d,12M,0;" % (2 if k else 3, 130 + k % 100)) * entries)) for k in range(n_reads)]
    return Case("xa_heavy_%d_%d" % (n_reads, entries), recs, C20, P30, [[]])


def deep_loci(counts, gap=40):
    """(contigs, candidates, records, props): one SNV per entry of `counts` with exactly that many members: single reads of 12 bases that
    start at the locus, half of them with the alt base, names in a scrambled order, every fourth a pair."""
    rng = random.Random(17)
    ref = bytes(rng.choice(b"ACGT") for _ in range(gap * (len(counts) + 1)))
    cands, recs = [], []
    for k, n in enumerate(counts):
        pos = gap * k + 20
        r = ref[pos:pos + 1]
        alt = bytes([rng.choice([b for b in b"ACGT" if b != r[0]])])
        cands.append(("d1", pos, r, alt))
        names = ["n%dL%d" % (rng.randrange(1 << 30), k) for _ in range(n)]
        j = 0
        while j < n:
            pair = j + 1 < n and j % 4 == 0
            for which in range(2 if pair else 1):
                start = pos - rng.randint(0, 8)
                edits = {pos - start: chr(alt[0])} if rng.random() < 0.5 else {}
                flag = (0x1 | (0x40 if which == 0 else 0x80) | (0x10 if which else 0x20)) if pair else 0
                recs.append((k, start, bc.make_read(ref, start, [("M", 12)], edits, flag=flag, name=names[j], mapq=60, mtid=0 if pair else -1, mpos=start + 1 if pair else -1)))
            j += 2 if pair else 1
    recs.sort(key=lambda x: (x[0], x[1]))
    return {"d1": ref}, cands, [r for _, _, r in recs], fragments.Props(8, 60, 12)


# ---------------------------------------------------------------------------------------------- reference testcases (tests/golden/bam/FRAGMENTS.md)
# testcase -> (predicate over (MAP allele frequency, PHRED posterior by event): the `expected:` block of its testcase.yaml, listed as met)
FIXTURES = {
    "test_giab_02": (lambda vaf, ph: vaf == 0.5, False),                                # 1:1192 TTTATG>TTGATG `NA12878 == 0.5` (needs realignment)
    "test_giab_03": (lambda vaf, ph: vaf == 0.5, False),                                # 1:1194 T>G           `NA12878 == 0.5` (needs realignment)
    "test_giab_07": (lambda vaf, ph: vaf == 0.0, True),                                 # 1:217 C>A            `index == 0.0`
    "test_giab_10": (lambda vaf, ph: vaf == 0.5, True),                                 # 1:302 T>C            `index == 0.5`
    "test_giab_28": (lambda vaf, ph: vaf == 1.0, True),                                 # 1:298 C>T            `NA12878 == 1.0`
    "test_giab_29": (lambda vaf, ph: vaf == 0.5 and ph["PROB_PRESENT"] <= 0.05, True),  # 1:299 G>A            `NA12878 == 0.5`, `PROB_PRESENT <= 0.05`
    "test_giab_30": (lambda vaf, ph: vaf == 0.0, True),                                 # 1:301 TGGGAGGGC>GGGGAGGGG `NA12878 == 0.0`
    "test_giab_33": (lambda vaf, ph: vaf == 0.5, True),                                 # 1:301 A>G            `NA12878 == 0.5`
    "test_uzuner_only_N": (lambda vaf, ph: vaf == 0.0, True),                           # 6:273 A>C            `sample == 0.0`
    "test_uzuner_clonal_1": (lambda vaf, ph: vaf == 1.0, True),                         # chr6:401 CGC>AGC     `sample == 1.0`
    "test_uzuner_clonal_2": (lambda vaf, ph: vaf == 1.0, True),                         # chr6:401 TTC>GTG     `sample == 1.0`
    "test_uzuner_clonal_3": (lambda vaf, ph: vaf == 1.0, True),                         # chr6:402 GG>TG       `sample == 1.0`
    "test_uzuner_fp_mnv1": (lambda vaf, ph: vaf == 0.0, True),                          # chr6:400 CAG>TGC     `sample == 0.0`
}
MUST_MEET = ("test_giab_30", "test_uzuner_clonal_1")
MIN_MET = 8


def fixture_case(golden_dir, name):
    """(bam path, fasta path, scenario path, [candidate], Props) of a held testcase"""
    import json
    import os
    bam, fasta, scenario, cand = bc.fixture_case(golden_dir, name)
    props = fragments.props_of(json.load(open(os.path.join(golden_dir, "bam", name, "properties.json"))))
    return bam, fasta, scenario, cand, props


def assert_same(obs, lrec, rs, tables=None):
    """the observations and locus records of the kernels (or of the host program) against a fragments.Restated of the same loci, field
    for field, f64 with ==; a locus flagged as too deep must have more than MAX_MEMBERS members and no observations"""
    assert [int(x) for x in lrec["n_members"]] == list(rs.n_members)
    at = 0
    for j, want in enumerate(rs.per_locus):
        n = int(lrec[j]["n_obs"])
        assert int(lrec[j]["obs_offset"]) == at, j
        if int(lrec[j]["status"]) & abi.FRAGPILEUP_LOCUS_TOO_MANY_MEMBERS:
            assert rs.n_members[j] > abi.FRAGPILEUP_MAX_MEMBERS and n == 0
            continue
        if int(lrec[j]["status"]) & abi.FRAGPILEUP_LOCUS_TOO_MANY_ALT_LOCI:
            assert sum(len(w.alt_loci) for w in want) > abi.FRAGPILEUP_MAX_MEMBERS and n == 0
            continue
        assert sum(len(w.alt_loci) for w in want) <= abi.FRAGPILEUP_MAX_MEMBERS
        assert rs.n_members[j] <= abi.FRAGPILEUP_MAX_MEMBERS and int(lrec[j]["status"]) == 0
        got = fragments.obs_from_array(obs[at:at + n])
        assert [g.key() for g in got] == [w.key() for w in want], j
        major = fragments.major_read_position(want)
        mj = int(lrec[j]["major_read_position"])
        assert (None if mj == abi.BASEPILEUP_NO_READ_POSITION else mj) == major, j
        bits = [bool(int(b) & abi.FRAGPILEUP_READPOS_MAJOR) for b in obs[at:at + n]["bits"]]
        assert bits == [major is not None and w.status == 0 and w.read_position == major for w in want], j
        # the device's alt-locus class (mode over hashed keys) against the restatement's (mode over the string keys)
        assert [int(c) for c in obs[at:at + n]["alt_locus"]] == fragments.alt_locus_classes(want, rs.max_read_len)[1], j
        at += n
    assert at == len(obs)
