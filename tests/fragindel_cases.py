"""Inputs shared by tests/test_fragment_indel_host.py and tests/test_gpu_fragindel.py: a deletion and an insertion candidate on a random
contig with synthetic read pairs (reference and alt haplotype, the alt reads aligned with a D / I operation or soft-clipped at the
breakpoint), the packing of an indel session's input for the host program, and the comparison of observations with the restatement."""
from __future__ import annotations

import random

import numpy as np

import basecall_cases as bc
from varlociraptor_amd import abi, fragments
from varlociraptor_amd import readwindows as rw

READ = 40
DEL_AT, DEL_LEN = 150, 6        # the anchor base and the deleted bases behind it
INS_AT, INS_SEQ = 230, b"GATTC"
PROPS = fragments.Props(200, 60, READ)
IPROPS = fragments.IndelProps((130.0, 12.0), 4, 4, 0.1)


def contig(n=400, seed=5):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def sites_of(ref, window=64, cands=None):
    """(candidates, IndelSite sorted by start)"""
    cands = cands or [("i1", DEL_AT, ref[DEL_AT:DEL_AT + DEL_LEN + 1], ref[DEL_AT:DEL_AT + 1]), ("i1", INS_AT, ref[INS_AT:INS_AT + 1], ref[INS_AT:INS_AT + 1] + INS_SEQ)]
    sites = [fragments.IndelSite(0, rw.indel_locus(ref, pos, r, a, window)) for _, pos, r, a in cands]
    return cands, sorted(sites, key=lambda s: s.start)


def read_at(ref, pos, name, alt, **kw):
    """a READ-base record at pos: the reference, or (alt) the haplotype with the deletion and the insertion, aligned with D / I where the
    read spans the breakpoint with 5 bases on either side, soft-clipped behind it otherwise"""
    cigar = [("M", READ)]
    if alt and pos <= DEL_AT < pos + READ - 1:
        a = DEL_AT - pos + 1
        cigar = [("M", a), ("D", DEL_LEN), ("M", READ - a)] if 5 <= a <= READ - 5 else [("M", a), ("S", READ - a)]
    elif alt and pos <= INS_AT < pos + READ - 1:
        a = INS_AT - pos + 1
        if 5 <= a <= READ - 5 - len(INS_SEQ):
            cigar = [("M", a), ("I", len(INS_SEQ)), ("M", READ - a - len(INS_SEQ))]
    rec = bc.make_read(ref, pos, cigar, name=name, **kw)
    return rec


def pairs(ref, n, seed=1, single_every=7):
    """n fragments over the two candidates, coordinate sorted: pairs (0x63 / 0x93) with an inner distance of 5 .. 70 and every
    `single_every`-th a single read.  Membership is on a record's start, so a pair is a pair at the deletion only when the right mate
    starts in front of its end (156): the left reads start from 40."""
    rng = random.Random(seed)
    recs = []
    for k in range(n):
        alt = rng.random() < 0.5
        p = rng.randint(40, 215)
        name = "f%05d" % k
        if k % single_every == 0:
            recs.append((p, 2 * k, read_at(ref, p, name, alt, flag=0x10 if k % 2 else 0)))
            continue
        q = p + READ + rng.randint(5, 70)
        recs.append((p, 2 * k, read_at(ref, p, name, alt, flag=0x63, mtid=0, mpos=q)))
        recs.append((q, 2 * k + 1, read_at(ref, q, name, alt, flag=0x93, mtid=0, mpos=p)))
    recs.sort(key=lambda x: (x[0], x[1]))
    return [r for _, _, r in recs]


def pack_host_input(contigs, sites, records, props, has_isize, spec, evidences):
    import struct
    blob = b"VFIH" + struct.pack("<qiiiiq", props.window, props.max_mapq, props.max_read_len, int(has_isize), spec.window, len(contigs))
    for seq in contigs.values():
        blob += struct.pack("<q", len(seq)) + seq.upper()
    alt_off = np.concatenate(([0], np.cumsum([len(s.locus.alt_allele) for s in sites]))).astype(np.uint64)
    kinds = {"deletion": abi.INDELPILEUP_DELETION, "insertion": abi.INDELPILEUP_INSERTION}
    blob += struct.pack("<q", len(sites)) + np.array([s.ref_id for s in sites], np.int32).tobytes() + np.array([s.start for s in sites], np.int64).tobytes()
    blob += np.array([s.end for s in sites], np.int64).tobytes() + np.array([kinds[s.kind] for s in sites], np.uint8).tobytes() + alt_off.tobytes()
    blob += b"".join(bytes(s.locus.alt_allele) for s in sites)
    starts = np.concatenate(([0], np.cumsum([len(r) for r in records]))).astype(np.uint64)
    blob += struct.pack("<q", len(records)) + starts.tobytes()
    blob += struct.pack("<q", len(evidences)) + np.array([[e.ln_ref, e.ln_alt] for e in evidences], np.float64).tobytes()
    return blob + b"".join(records)


def unpack_host_output(d, n_loci):
    import struct
    n, = struct.unpack_from("<q", d, 0)
    o = 8
    obs = np.frombuffer(d, abi.FRAGPILEUP_OBS_DTYPE, n, o); o += 56 * n
    obx = np.frombuffer(d, abi.FRAGPILEUP_INDEL_OBS_DTYPE, n, o); o += 24 * n
    loc = np.frombuffer(d, abi.FRAGPILEUP_LOCUS_DTYPE, n_loci, o); o += 24 * n_loci
    lox = np.frombuffer(d, abi.FRAGPILEUP_INDEL_LOCUS_DTYPE, n_loci, o); o += 16 * n_loci
    ne, = struct.unpack_from("<q", d, o)
    o += 8
    return obs, obx, loc, lox, np.frombuffer(d, abi.INDELPILEUP_HIT_DTYPE, ne, o), d[o + 64 * ne:]


def assert_same(obs, obx, loc, lox, rs, tol=0.0):
    """the observations, side records, locus records and maxima against an IndelRestated: integers, strands, flags, insert sizes and
    maxima with ==, the supports within `tol` (0: ==)"""
    assert [int(x) for x in loc["n_members"]] == list(rs.n_members)
    assert [(int(x["max_del"]), int(x["max_ins"]), (int(x["max_clip"]), int(x["max_clip_l_seq"]))) for x in lox] == list(rs.maxima)
    at = 0
    for j, want in enumerate(rs.per_locus):
        n = int(loc[j]["n_obs"])
        assert int(loc[j]["obs_offset"]) == at and int(loc[j]["status"]) == 0, j
        got = fragments.indel_obs_from_arrays(obs[at:at + n], obx[at:at + n])
        assert [g.key()[2:] for g in got] == [w.key()[2:] for w in want], j
        for g, w in zip(got, want):
            assert abs(g.obs.prob_ref - w.obs.prob_ref) <= tol and abs(g.obs.prob_alt - w.obs.prob_alt) <= tol, (j, g, w)
        assert int(loc[j]["major_read_position"]) == abi.BASEPILEUP_NO_READ_POSITION
        at += n
    assert at == len(obs) == len(obx) and not obx["pad"].any()


def indels_rows():
    """{testcase: (observations per fragment, MAP VAF per fragment as written, met)} of the rows of tests/golden/bam/INDELS.md that were
    built; {testcase: None} for a refused one"""
    import os
    rows = {}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam", "INDELS.md")
    for line in open(path):
        c = [x.strip() for x in line.split("|")]
        if len(c) < 7 or not c[1].startswith(("test_", "test5", "issue_")):
            continue
        if c[5].startswith("refused"):
            rows[c[1]] = None
            continue
        n, rest = c[5].split(",", 1)
        rows[c[1]] = (int(n), rest.split()[0].rstrip(","), rest.strip().endswith("yes"))
    return rows
