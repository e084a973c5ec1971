"""Inputs shared by tests/test_basecalls_host.py, tests/test_basepileup_host.py and tests/test_gpu_basepileup.py: the records of the
reference's own SNV unit test (variants/types/snv.rs:316-416), hand-made records for every rule of varlociraptor_amd/basecalls.py, a
seeded synthetic BAM, and the reference testcases held under tests/golden/bam/ (tools/make_basecall_fixtures.py) with their
`expected:` blocks as predicates."""
from __future__ import annotations

import glob
import os
import random

from varlociraptor_amd import abi, alignprops, basecalls
from varlociraptor_amd.readwindows import read_bam

# testcase -> predicate over (MAP allele frequency, PHRED posterior by event): the `expected:` block of its testcase.yaml
FIXTURES = {
    "test_giab_07": lambda vaf, ph: vaf == 0.0,                                   # 1:217 C>A        `index == 0.0`
    "test_giab_10": lambda vaf, ph: vaf == 0.5,                                   # 1:302 T>C        `index == 0.5`
    "test_giab_28": lambda vaf, ph: vaf == 1.0,                                   # 1:298 C>T        `NA12878 == 1.0`
    "test_giab_29": lambda vaf, ph: vaf == 0.5 and ph["PROB_PRESENT"] <= 0.05,    # 1:299 G>A        `NA12878 == 0.5`, `PROB_PRESENT <= 0.05`
    "test_giab_33": lambda vaf, ph: vaf == 0.5,                                   # 1:301 A>G        `NA12878 == 0.5`
    "test_uzuner_only_N": lambda vaf, ph: vaf == 0.0,                             # 6:273 A>C        `sample == 0.0`
    "test_uzuner_clonal_2": lambda vaf, ph: vaf == 1.0,                           # chr6:401 TTC>GTG `sample == 1.0`
    "test_uzuner_clonal_3": lambda vaf, ph: vaf == 1.0,                           # chr6:402 GG>TG   `sample == 1.0`
    "test_uzuner_fp_mnv1": lambda vaf, ph: vaf == 0.0,                            # chr6:400 CAG>TGC `sample == 0.0`
}


def fixture_case(golden_dir, name):
    """(bam path, fasta path, scenario path, [candidate]) of a held testcase"""
    d = os.path.join(golden_dir, "bam", name)
    bam, = glob.glob(os.path.join(d, "*.bam"))
    var = open(os.path.join(d, "variant.tsv")).read().split("\n")[1].split("\t")
    return bam, os.path.join(d, "ref.fa"), os.path.join(d, "scenario.yaml"), [(var[0], int(var[1]) - 1, var[3].encode(), var[4].encode())]


# ---------------------------------------------------------------------------------------------- snv.rs:316-416
SNV_RS_REF = b"CCTATACGCGT"
SNV_RS_CANDIDATE = ("ref", 5, b"A", b"G")


def snv_rs_records():
    E = alignprops.encode_record
    return [
        E(0, 2, 60, 0, [("H", 5), ("S", 2), ("M", 6)], "AATATACG", qual=bytes([20, 20, 30, 30, 30, 40, 30, 30]), name="HC_SC_M"),
        E(0, 2, 60, 0, [("H", 2), ("I", 2), ("M", 6)], "TTTATGCG", qual=bytes([20, 20, 20, 20, 20, 30, 20, 20]), name="HC_Ins_M"),
        E(0, 0, 60, 0, [("=", 2), ("X", 1), ("D", 2), ("=", 5)], "CCAACGCG", qual=bytes([30, 30, 30, 50, 30, 30, 30, 30]), name="Eq_Diff_Del_Eq"),
        E(0, 1, 60, 0, [("M", 4), ("D", 1), ("M", 4)], "CTATCGCG", qual=bytes([10, 30, 30, 30, 30, 30, 30, 30]), name="M_Del_M"),
        E(0, 0, 60, 0, [("=", 1), ("X", 1), ("=", 2), ("N", 3), ("M", 4)], "CTTAGCGT", qual=bytes([10, 30, 30, 30, 30, 30, 30, 30]), name="M_RefSkip_M"),
    ]


# ---------------------------------------------------------------------------------------------- hand cases
HAND_REF = b"ACGTTGCAAGCTTAGGCTAACGGATCCATGCAAGTCCGATTGACCTAGGATCGATTACAGGCTTAAGCGTACCGGTTAACCGGATATCGCGATTAGCCATG"
SNV_AT = 20          # HAND_REF[20] = C
MNV_AT = 40          # HAND_REF[40:43] = TGA
HAND_CANDIDATES = [("c1", SNV_AT, b"C", b"T"), ("c1", MNV_AT, b"TGA", b"CCA")]


def make_read(ref, pos, cigar, edits=None, qual=None, q=30, **kw):
    """A record whose bases follow `ref` along `cigar` (inserted bases A, soft-clipped bases T), then `edits` {read index: base}."""
    seq, r = [], pos
    for op, l in cigar:
        if op in "M=X":
            seq += [chr(c) for c in ref[r:r + l]]
            r += l
        elif op == "I":
            seq += ["A"] * l
        elif op == "S":
            seq += ["T"] * l
        elif op in "DN":
            r += l
    for i, b in (edits or {}).items():
        seq[i] = b
    if qual is None:
        qual = bytes([q] * len(seq))
    return alignprops.encode_record(kw.pop("tid", 0), pos, kw.pop("mapq", 60), kw.pop("flag", 0), cigar, "".join(seq), qual=qual, **kw)


def hand_records():
    """{label: record}, in file order"""
    R, out = HAND_REF, {}
    A = alignprops.aux_field

    def add(label, *a, **kw):
        out[label] = make_read(R, *a, name=kw.pop("name", label), **kw)
    # Enclosing at the exact boundaries, and one base short on either side (SNV [20, 21), MNV [40, 43))
    add("snv_starts_at_locus", 20, [("M", 10)])
    add("snv_ends_at_locus", 11, [("M", 10)])
    add("snv_starts_behind", 21, [("M", 10)])
    add("snv_ends_before", 10, [("M", 10)])
    add("mnv_starts_at_locus", 40, [("M", 10)])
    add("mnv_ends_at_locus", 33, [("M", 10)])
    add("mnv_starts_behind", 41, [("M", 10)])
    add("mnv_ends_before", 32, [("M", 10)])
    # bases at the SNV: alt, N, a third base; qualities 0, 93, 255
    add("snv_alt", 15, [("M", 12)], {5: "T"})
    add("snv_N", 15, [("M", 12)], {5: "N"})
    add("snv_third", 15, [("M", 12)], {5: "G"}, flag=0x10)
    add("snv_q0", 15, [("M", 12)], {5: "T"}, qual=bytes([30] * 5 + [0] + [30] * 6))
    add("snv_q93", 15, [("M", 12)], qual=bytes([30] * 5 + [93] + [30] * 6))
    add("snv_q255", 15, [("M", 12)], {5: "T"}, qual=bytes([30] * 5 + [255] + [30] * 6))
    add("snv_hardclip_softclip", 18, [("H", 4), ("S", 3), ("M", 8)], {5: "T"})
    # MNV: ref, alt, across a deletion and a reference skip, N inside
    add("mnv_ref", 35, [("M", 15)])
    add("mnv_alt", 35, [("M", 15)], {5: "C", 6: "C"}, flag=0x10)
    add("mnv_across_D", 35, [("M", 6), ("D", 1), ("M", 8)])
    add("mnv_across_N", 35, [("M", 4), ("N", 2), ("M", 9)])
    add("mnv_N_inside", 35, [("M", 15)], {5: "C", 6: "N"})
    # third-allele override: alt at two bases, a third base at the last one.  All q30: 3 * 0.001 expected substitutions against 1 (fires);
    # q30 at the locus and q1 elsewhere in a 20-base read: 3 * 0.675 = 2.03 against 1 (explainable)
    add("mnv_override_fires", 35, [("M", 20)], {5: "C", 6: "C", 7: "G"})
    add("mnv_override_explainable", 35, [("M", 20)], {5: "C", 6: "C", 7: "G"}, qual=bytes([1] * 5 + [30] * 3 + [1] * 12))
    # SI tag: strand per position; OR over the informative bases of an MNV
    add("snv_si_minus", 15, [("M", 12)], {5: "T"}, aux=A("NM", "C", 1) + A("SI", "Z", "+++++-++++++"))
    add("snv_si_dot", 15, [("M", 12)], {5: "T"}, aux=A("SI", "Z", "+++++.++++++") + A("XB", "B", ("s", [1, -2, 3])))
    add("mnv_si_both", 35, [("M", 15)], {5: "C", 6: "C"}, aux=A("SI", "Z", "+++++-+++++++++"))
    add("mnv_si_same", 35, [("M", 15)], {5: "C", 6: "C"}, aux=A("SI", "Z", "-----+++-------"))
    add("snv_si_not_a_string", 15, [("M", 12)], {5: "T"}, aux=A("SI", "i", 7), flag=0x10)
    # the flag rule (sample.rs:281-286)
    add("flag_secondary", 15, [("M", 12)], flag=0x100)
    add("flag_qcfail", 15, [("M", 12)], flag=0x200)
    add("flag_duplicate", 15, [("M", 12)], flag=0x400)
    add("flag_unmapped", 15, [("M", 12)], flag=0x4)
    add("flag_supplementary", 15, [("M", 12)], {5: "T"}, flag=0x800)
    # mates (one QNAME): alt + alt at different read positions, alt + ref, ref + alt, ref + ref
    add("pair_aa_1", 12, [("M", 12)], {8: "T"}, flag=0x41, name="pair_aa")
    add("pair_aa_2", 17, [("M", 12)], {3: "T"}, flag=0x91, name="pair_aa")
    add("pair_ar_1", 12, [("M", 12)], {8: "T"}, flag=0x41, name="pair_ar")
    add("pair_ar_2", 17, [("M", 12)], flag=0x91, name="pair_ar")
    add("pair_ra_1", 12, [("M", 12)], flag=0x41, name="pair_ra")
    add("pair_ra_2", 17, [("M", 12)], {3: "T"}, flag=0x91, name="pair_ra")
    add("pair_rr_1", 12, [("M", 12)], flag=0x41, name="pair_rr")
    add("pair_rr_2", 12, [("M", 12)], flag=0x91, name="pair_rr")
    # a read with an insertion in front of the SNV (NEEDS_REALIGN with realign_indel_reads)
    add("snv_behind_insertion", 12, [("M", 4), ("I", 2), ("M", 8)], {10: "T"})
    return out


def hand_error_records():
    """records the reference fails on: an SI tag shorter than the read position, an SI character outside + - * ."""
    A = alignprops.aux_field
    return {"si_too_short": make_read(HAND_REF, 15, [("M", 12)], {5: "T"}, aux=A("SI", "Z", "+++"), name="si_too_short"),
            "si_invalid": make_read(HAND_REF, 15, [("M", 12)], {5: "T"}, aux=A("SI", "Z", "+++++x++++++"), name="si_invalid")}


def write_case(tmp, name, contigs, records, member_bytes=0xff00):
    """<tmp>/<name>.bam and <tmp>/<name>.fa from {contig: sequence} and encoded records"""
    bam, fa = os.path.join(str(tmp), name + ".bam"), os.path.join(str(tmp), name + ".fa")
    alignprops.write_bam(bam, [(c, len(s)) for c, s in contigs.items()], list(records), member_bytes)
    alignprops.write_fasta(fa, contigs)
    return bam, fa


def loci_of(candidates, contigs):
    """basecalls.Locus per candidate, sorted by (ref_id, start)"""
    names = list(contigs)
    loci = [basecalls.locus(contigs[c], names.index(c), pos, ref, alt) for c, pos, ref, alt in candidates]
    return sorted(loci, key=lambda l: (l.ref_id, l.start))


# ---------------------------------------------------------------------------------------------- seeded synthetic BAM
def synthetic(n_records=300, n_loci=2000, seed=11):
    """(contigs, candidates, records): reads of 20-60 bases on contig s1 with M, I, D, N, S, H, =, X operations, mismatches and Ns,
    a few SI tags, an unsorted tail; loci on s1 (inside and outside every read), on s2 (a contig without reads); half of them MNVs of
    2-9 bases."""
    rng = random.Random(seed)
    contigs = {"s1": bytes(rng.choice(b"ACGT") for _ in range(3000)), "s2": bytes(rng.choice(b"ACGT") for _ in range(500))}
    cands = []
    for k in range(n_loci):
        c = "s1" if k % 10 else "s2"
        ln = rng.randint(2, 9) if k % 2 else 1
        pos = rng.randrange(0, len(contigs[c]) - ln)
        ref = contigs[c][pos:pos + ln]
        alt = bytes(rng.choice([b for b in b"ACGT" if b != r]) if (j == 0 or rng.random() < 0.6) else r for j, r in enumerate(ref))
        cands.append((c, pos, ref, alt))
    alt_at = {}
    for c, pos, ref, alt in cands:
        if c == "s1":
            for j in range(len(ref)):
                alt_at.setdefault(pos + j, chr(alt[j]))
    recs, starts = [], sorted(rng.randrange(0, 2600) for _ in range(n_records))
    tail = n_records // 10
    starts = starts[:-tail] + [rng.randrange(0, 2600) for _ in range(tail)]   # an unsorted tail
    for k, pos in enumerate(starts):
        target = rng.randint(20, 60)
        cigar, used = [], 0
        if rng.random() < 0.15:
            cigar.append(("H", rng.randint(1, 9)))
        if rng.random() < 0.2:
            l = rng.randint(1, 5)
            cigar.append(("S", l))
            used += l
        while used < target:
            l = min(rng.randint(3, 25), target - used)
            cigar.append((rng.choice("MMM=X"), l))
            used += l
            if used < target and rng.random() < 0.5:
                op = rng.choice("IDN")
                l = rng.randint(1, 4)
                cigar.append((op, l))
                if op == "I":
                    used += l
        if cigar[-1][0] in "IDN":
            cigar.append(("M", 2))
        if rng.random() < 0.2:
            cigar.append(("S", rng.randint(1, 4)))
        if rng.random() < 0.1:
            cigar.append(("H", 3))
        n = sum(l for op, l in cigar if op in "MIS=X")
        edits, r, i = {}, pos, 0
        for op, l in cigar:   # carry the alt base of a locus half of the time, now and then another base or an N
            if op in "M=X":
                for j in range(l):
                    x = rng.random()
                    if r + j in alt_at and x < 0.5:
                        edits[i + j] = alt_at[r + j]
                    elif x < 0.53:
                        edits[i + j] = rng.choice("ACGTN")
                r += l
                i += l
            elif op in "IS":
                i += l
            elif op in "DN":
                r += l
        qual = bytes(rng.choice([0, 2, 11, 20, 30, 37, 41, 93]) if rng.random() < 0.3 else 30 for _ in range(n))
        aux = b""
        if rng.random() < 0.15:
            aux = alignprops.aux_field("NM", "C", 2) + alignprops.aux_field("SI", "Z", "".join(rng.choice("+-*.") for _ in range(n)))
        flag = rng.choice([0, 0x10, 0x41, 0x91, 0x800, 0x810]) if rng.random() < 0.93 else rng.choice([0x100, 0x200, 0x400, 0x4])
        recs.append(make_read(contigs["s1"], pos, cigar, edits, qual=qual, flag=flag, aux=aux, mapq=rng.choice([0, 20, 60]), name="q%d" % (k // 2)))
    return contigs, cands, recs


def restatement(bam, loci, tables=basecalls.TABLES, realign_indel_reads=False):
    _, recs = read_bam(bam)
    return basecalls.score_records(recs, loci, tables, realign_indel_reads)


def hit_keys(hits):
    return [h.key() for h in hits]
