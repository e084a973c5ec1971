"""Inputs shared by tests/test_fragment_realign_host.py and tests/test_gpu_fragrealign.py: hand-made records for every rule of the
realignment of indel-bearing reads over SNV / MNV candidates (varlociraptor_amd/fragments.py, csrc/vlr_fragpileup.h), whose expectations
follow from the sequences alone, synthetic 30-base reads with a chosen number of realigned evidences, and the comparisons of the
kernels' evidences and observations with the restatement."""
from __future__ import annotations

import random
from typing import List

import numpy as np

import basecall_cases as bc
import fragment_cases as fc
from varlociraptor_amd import abi, alignprops, basecalls, fragments, realign
from varlociraptor_amd import readwindows as rw

A = alignprops.aux_field
REF = bc.HAND_REF                    # 101 bases; REF[20] = C, REF[40:43] = TGA
SNV20 = ("c1", 20, b"C", b"T")
MNV40 = ("c1", 40, b"TGA", b"CCA")
P30 = fragments.Props(30, 60, 40)
KERNEL_VS_RESTATEMENT = 1e-9


def read_with(seq: str, pos: int, cigar, name: str, **kw) -> bytes:
    """a record with exactly these bases"""
    q = kw.pop("q", 30)
    return alignprops.encode_record(kw.pop("tid", 0), pos, kw.pop("mapq", 60), kw.pop("flag", 0), list(cigar), seq, qual=bytes([q] * len(seq)), name=name, **kw)


def allele(pos0: int, pos1: int, alt: bool, cand=SNV20) -> str:
    """REF[pos0:pos1] with the candidate's alt bases in place when `alt`"""
    s = bytearray(REF[pos0:pos1])
    if alt:
        for k, b in enumerate(cand[3]):
            if pos0 <= cand[1] + k < pos1:
                s[cand[1] + k - pos0] = b
    return s.decode()


I5 = [("M", 5), ("I", 1), ("M", 19)]      # at 8: read 0-4 on 8..12, read 5 inserted, read 6-24 on 13..31: the SNV at 20 sees read base 13
D3 = [("M", 5), ("D", 3), ("M", 20)]      # at 8: read 0-4 on 8..12, 13..15 deleted, read 5-24 on 16..35: the SNV at 20 sees read base 9


def hand_records():
    """{label: record} over SNV20 and MNV40.  REF[8:33] = AGCTTAGGCTAA C GGATCCATGCAA.
    alt_misplaced: the 25 bases ARE the alt allele over [8, 33) (T at 20), but the aligner put an insertion in front: the SNV sees read
        base 13 = REF[21] = G, a third base, so base-by-base scoring does not support alt.  Realigned, the read equals the alt window.
    ref_misplaced: the 25 bases ARE the reference over [8, 33), aligned with a 3-base deletion: the SNV sees read base 9 = REF[17] = T,
        the alt base.  Realigned, the read equals the ref window.
    uninformative: N where the alleles differ."""
    out = {}
    out["alt_misplaced"] = read_with(allele(8, 33, True), 8, I5, "alt_misplaced")
    out["ref_misplaced"] = read_with(allele(8, 33, False), 8, D3, "ref_misplaced", flag=0x10)
    n_at_snv = allele(8, 20, False) + "N" + allele(21, 33, False)
    out["uninformative"] = read_with(n_at_snv, 8, I5, "uninformative")
    # both mates realigned, both the alt allele: forward + reverse
    out["both_1"] = read_with(allele(8, 33, True), 8, I5, "pair_both", flag=0x63, mtid=0, mpos=12)
    out["both_2"] = read_with(allele(12, 37, True), 12, [("M", 4), ("I", 1), ("M", 20)], "pair_both", flag=0x93, mtid=0, mpos=8)
    # one mate realigned (the reference), one scored base by base (alt at read position 5, reverse)
    out["mixed_1"] = read_with(allele(8, 33, False), 8, D3, "pair_mixed", flag=0x63, mtid=0, mpos=15)
    out["mixed_2"] = read_with(allele(15, 35, True), 15, [("M", 20)], "pair_mixed", flag=0x93, mtid=0, mpos=8)
    # an uninformative realigned mate and a mate that carries a strand
    out["unin_pair_1"] = read_with(n_at_snv, 8, I5, "pair_unin", flag=0x63, mtid=0, mpos=15)
    out["unin_pair_2"] = read_with(allele(15, 35, True), 15, [("M", 20)], "pair_unin", flag=0x93, mtid=0, mpos=8)
    out["mapq0"] = read_with(allele(8, 33, True), 8, I5, "mapq0", mapq=0)
    # an MNV [40, 43) TGA > CCA: the reference with base 41 deleted (one edit from ref, three from alt); the alt allele with an insertion
    out["mnv_across_D"] = read_with(allele(30, 41, False) + allele(42, 55, False), 30, [("M", 11), ("D", 1), ("M", 13)], "mnv_across_D")
    out["mnv_alt_with_I"] = read_with(allele(30, 55, True, MNV40), 30, I5, "mnv_alt_with_I", flag=0x10)
    return out


def refused_records():
    """{label: record}: a CIGAR that begins with N (N over 6..7, then 12M 1I 11M from 8), and an SI:Z tag on a record that needs realignment"""
    return {"plain": read_with(allele(15, 35, True), 15, [("M", 20)], "plain"),
            "leading_N": read_with(allele(8, 20, False) + "A" + allele(20, 31, False), 6, [("N", 2), ("M", 12), ("I", 1), ("M", 11)], "leading_N"),
            "with_SI": read_with(allele(8, 33, True), 8, I5, "with_SI", aux=A("SI", "Z", "+" * 25))}


def edge_records():
    """{label: (record, candidate)}: window edges"""
    out = {}
    # the read ends exactly at the locus end (1..5, insertion, 6..20): read_pos(locus end) is None, the arm (Some, None)
    out["ends_at_locus_end"] = (bc.make_read(REF, 1, [("M", 5), ("I", 1), ("M", 15)], name="ends_at_locus_end"), SNV20)
    # loci in the first and the last rw bases of the contig: both clamps, the alt window clamped on its own
    first = ("c1", 2, REF[2:3], b"A")
    out["first_bases"] = (bc.make_read(REF, 0, [("M", 10), ("I", 1), ("M", 13)], {2: "A"}, name="first_bases"), first)
    last = ("c1", 98, REF[98:99], b"C")
    out["last_bases"] = (bc.make_read(REF, 76, [("M", 8), ("I", 1), ("M", 17)], {23: "C"}, name="last_bases"), last)
    return out


def long_read_case():
    """(contigs, candidate, record): a read of 151 bases that encloses an SNV in its middle on a contig of 400 bases, with an insertion:
    the read window of 2 * 64 + 1 bases is trimmed to MAX_PATTERN_LEN, an exceed of 1 (odd: the floor half in front, the ceiling half
    behind; for an enclosing read (qe - qs) + 2 * (window - (qe - qs) / 2) never exceeds by more)"""
    rng = random.Random(3)
    ref = bytes(rng.choice(b"ACGT") for _ in range(400))
    cand = ("L1", 200, ref[200:201], b"A" if ref[200:201] != b"A" else b"C")
    n = 151
    seq = ref[130:130 + 20] + b"A" + ref[150:130 + n - 1]
    return {"L1": ref}, cand, read_with(seq.decode(), 130, [("M", 20), ("I", 1), ("M", n - 21)], "long")


def counted(n_evidences: int, n_plain: int = 3, seed: int = 1):
    """(contigs, candidates, records, props): 30-base reads over one SNV at 100 of a 220-base contig; exactly n_evidences of them carry an
    insertion (each is one realigned evidence), n_plain do not; half carry the alt base; coordinate sorted"""
    rng = random.Random(seed)
    ref = bytes(rng.choice(b"ACGT") for _ in range(220))
    alt = bytes([rng.choice([b for b in b"ACGT" if b != ref[100]])])
    recs = []
    for k in range(n_evidences + n_plain):
        indel = k < n_evidences
        pos = rng.randint(75, 95)
        cigar = [("M", 4), ("I", 1), ("M", 25)] if indel else [("M", 30)]
        edits = {100 - pos + (1 if indel else 0): chr(alt[0])} if rng.random() < 0.5 else {}
        recs.append((pos, k, bc.make_read(ref, pos, cigar, edits, name="e%05d" % k, flag=0x10 if k % 3 == 0 else 0)))
    recs.sort(key=lambda x: (x[0], x[1]))
    return {"k1": ref}, [("k1", 100, ref[100:101], alt)], [r for _, _, r in recs], fragments.Props(40, 60, 30)


def ref_seqs_of(contigs):
    return {k: s.upper() for k, s in enumerate(contigs.values())}


def restated(bams, contigs, loci, props, spec, tables=basecalls.TABLES, device="cpu"):
    recs = [r for b in ([bams] if isinstance(bams, str) else bams) for r in rw.read_bam(b)[1]]
    return fragments.restate(recs, loci, props, tables, realign=spec, ref_seqs=ref_seqs_of(contigs), device=device)


def evidence_keys(evs: List[fragments.RealignEvidence]):
    """(locus, record, status, read interval, ref interval, flag, mapq)"""
    return [e.key() for e in evs]


def hit_keys(arr):
    return [(int(h["locus"]), int(h["record"]), int(h["status"]), (int(h["read_begin"]), int(h["read_begin"]) + int(h["read_len"])),
             (int(h["ref_begin"]), int(h["ref_begin"]) + int(h["ref_len"])), int(h["flag"]), int(h["mapq"])) for h in arr]


def windows_of(hits, contigs, loci, records, window):
    """the pair batch rebuilt from the coordinates of the device's evidences alone"""
    names = list(contigs)
    pb = realign.PairBatch()
    for h in hits:
        if h["status"]:
            pb.add(b"", b"", b"")
            pb.add(b"", b"", b"")
            continue
        loc = loci[int(h["locus"])]
        seq = contigs[names[loc.ref_id]].upper()
        rec = records[int(h["record"])]
        b, n = int(h["read_begin"]), int(h["read_len"])
        read, q = rec.seq[b:b + n].upper(), rec.qual[b:b + n]
        pb.add(seq[int(h["ref_begin"]):int(h["ref_begin"]) + int(h["ref_len"])], read, q)
        pb.add(rw.substitution_locus(seq, loc.start, loc.ref, loc.alt, window).alt_allele, read, q)
    return pb


def assert_observations_close(obs, lrec, rs, tol=KERNEL_VS_RESTATEMENT):
    """the kernels' observations against a Restated: every integer field ==, the supports within `tol`"""
    assert [int(x) for x in lrec["n_members"]] == list(rs.n_members)
    at = 0
    for j, want in enumerate(rs.per_locus):
        n = int(lrec[j]["n_obs"])
        assert int(lrec[j]["obs_offset"]) == at and int(lrec[j]["status"]) == 0, j
        got = fragments.obs_from_array(obs[at:at + n])
        assert [g.key()[2:] for g in got] == [w.key()[2:] for w in want], j
        for g, w in zip(got, want):
            assert abs(g.prob_ref - w.prob_ref) <= tol and abs(g.prob_alt - w.prob_alt) <= tol, (j, g, w)
        mj = int(lrec[j]["major_read_position"])
        assert (None if mj == abi.BASEPILEUP_NO_READ_POSITION else mj) == fragments.major_read_position(want), j
        at += n
    assert at == len(obs)
