"""`estimate alignment-properties` on the GPU (vlr_bamstats_*, csrc/vlr_bamstats.hip): the device counts must equal the pure-Python
restatement's (varlociraptor_amd/alignprops.py) exactly — transition matrix, every homopolymer-run counter, maxima, flag counters
and the insert sizes — on the reference's fixtures and on synthetic BAMs that reach every branch: paired reads of known insert size,
a lower-case soft-masked reference, N bases, homopolymers longer than the dense LDS bound, hard clips, every skip flag, EF tags of
every integer type behind aux fields of every type, a 70 000-base record and records that straddle BGZF members.  Also: the cap
(--num-records) at the exact record, byte-identical JSON under forced window sizes and across runs, the CLI end to end, and clean
errors for a truncated BAM and a CIGAR past its contig."""
import os
import subprocess
import sys

import numpy as np
import pytest

from varlociraptor_amd import alignprops as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "alignment_properties")
FASTA = os.path.join(FX, "chr10.fa")
SOFT = os.path.join(FX, "tumor-first30000.reads_with_soft_clips.bam")
SINGLE = os.path.join(FX, "tumor-first30000.bunch_of_reads_made_single_ended.bam")


def assert_same(dev: A.Counts, cpu: A.Counts):
    assert np.array_equal(dev.transitions, cpu.transitions), np.argwhere(dev.transitions != cpu.transitions)
    assert dev.hops == cpu.hops
    assert dev.insert_sizes == cpu.insert_sizes
    for k in ("max_del", "max_ins", "frac_max_softclip", "max_read_len", "max_mapq", "n_taken", "n_skipped", "n_not_usable", "n_softclips",
              "n_not_paired", "n_not_first", "n_mate_unmapped", "n_tid_mismatch"):
        assert getattr(dev, k) == getattr(cpu, k), k


def _both(fasta, bams, n, **kw):
    return A.count_bams_device(fasta, bams, n, 0, **kw), A.count_bams(fasta, bams, n)


# ------------------------------------------------------------------------------------------------ synthetic inputs
AUX_LEAD = [A.aux_field("XA", "A", "q"), A.aux_field("Xc", "c", -3), A.aux_field("XC", "C", 200), A.aux_field("Xs", "s", -300),
            A.aux_field("XS", "S", 60000), A.aux_field("Xi", "i", -70000), A.aux_field("XI", "I", 4000000000), A.aux_field("Xf", "f", 0.5),
            A.aux_field("XZ", "Z", "some text"), A.aux_field("XH", "H", "BEEF"), A.aux_field("XB", "B", ("I", [1, 2, 3])),
            A.aux_field("Xb", "B", ("f", [0.25])), A.aux_field("Xe", "B", ("c", []))]


def bases(rng, n, alphabet=b"ACGT"):
    return rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n).tobytes()


def make_reference(rng, n=60000):
    seq = bytearray(bases(rng, n))
    seq[1000:1100] = b"A" * 100                       # homopolymers longer than the dense bound (32)
    seq[2000:2045] = b"c" * 45
    seq[3000:3050] = b"T" * 25 + b"t" * 25
    seq[5000:9000] = bytes(seq[5000:9000]).lower()   # soft-masked
    seq[9000:9030] = b"N" * 30
    for k in range(12000, 20000, 97):                 # many short homopolymers
        seq[k:k + rng.integers(2, 12)] = bytes([seq[k]]) * 1
        L = int(rng.integers(2, 12))
        seq[k:k + L] = bytes([seq[k]]) * L
    return bytes(seq[:n])


def make_record(rng, ref, tid, read_len=None, flag=None):
    """A record whose CIGAR fits its contig and read; its sequence follows the reference with errors, homopolymer-aware indels."""
    L = len(ref)
    rl = int(read_len or rng.integers(20, 250))
    for _ in range(100):
        pos = int(rng.integers(0, L - 4 * rl - 400))
        if rng.random() < 0.3:
            pos = int(rng.choice([990, 1050, 1095, 1990, 2030, 2990, 3020, 4995, 8990, 9010, 12000 + 97 * int(rng.integers(0, 80))]))
        if pos + 4 * rl + 400 < L:
            break
    cig, seq = [], bytearray()
    rpos, q = pos, 0
    if rng.random() < 0.15:
        cig.append(("H", int(rng.integers(1, 20))))
    if rng.random() < 0.25:
        s = int(rng.integers(1, 15))
        cig.append(("S", s)); seq += bases(rng, s); q += s
    while q < rl:
        r = rng.random()
        if r < 0.08 and cig and cig[-1][0] in "M=X":
            l = int(rng.integers(1, 6)) if rng.random() < 0.8 else int(rng.integers(6, 40))
            cig.append(("D", l)); rpos += l
        elif r < 0.16 and cig and cig[-1][0] in "M=X":
            l = int(rng.integers(1, 5))
            b = ref[rpos] if rng.random() < 0.6 else int(rng.choice(list(b"ACGTN")))
            cig.append(("I", l)); seq += bytes([b]).upper() * l; q += l
        elif r < 0.18 and cig and cig[-1][0] in "M=X":
            l = int(rng.integers(1, 30)); cig.append(("N", l)); rpos += l
        else:
            l = int(min(rl - q, rng.integers(1, 80)))
            op = "M" if rng.random() < 0.7 else ("=" if rng.random() < 0.5 else "X")
            part = bytearray(bytes(ref[rpos:rpos + l]).upper())
            for k in range(l):
                if rng.random() < 0.02:
                    part[k] = int(rng.choice(list(b"ACGTN")))
            cig.append((op, l)); seq += part; q += l; rpos += l
    if rng.random() < 0.2:
        s = int(rng.integers(1, 10)); cig.append(("S", s)); seq += bases(rng, s)
    if flag is None:
        flag = int(rng.choice([0x1 | 0x40, 0x1 | 0x80, 0x1 | 0x40 | 0x8, 0, 0x1 | 0x40 | 0x100, 0x800, 0x1 | 0x40 | 0x10]))
        r = rng.random()
        if r < 0.04: flag |= 0x400
        elif r < 0.08: flag |= 0x200
        elif r < 0.12: flag |= 0x4
    mapq = 0 if rng.random() < 0.04 else int(rng.integers(1, 61))
    tlen = int(rng.integers(200, 500)) * (1 if rng.random() < 0.5 else -1)
    mtid = tid if rng.random() < 0.9 else -1
    aux = b""
    if rng.random() < 0.5:
        lead = [AUX_LEAD[int(i)] for i in rng.choice(len(AUX_LEAD), size=int(rng.integers(0, 5)), replace=False)]
        t = str(rng.choice(list("cCsSiIfA")))
        ef = A.aux_field("EF", t, 1 if t in "cCsSiI" else (1.0 if t == "f" else "1")) if rng.random() < 0.7 else A.aux_field("EF", "C", 0)
        aux = b"".join(lead) + ef + (A.aux_field("EF", "C", 0) if rng.random() < 0.3 else b"")
    if rng.random() < 0.02:
        seq = bytearray(); cig = []                     # empty SEQ: skipped
    return A.encode_record(tid, pos, mapq, flag, cig, seq.decode(), mtid, pos + 10, tlen, aux)


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    rng = np.random.default_rng(11)
    d = tmp_path_factory.mktemp("ap")
    refs = {"s1": make_reference(rng), "s2": make_reference(rng, 30000), "unused": b"ACGT" * 10}
    fasta = str(d / "ref.fa")
    A.write_fasta(fasta, refs)
    contigs = [("s1", len(refs["s1"])), ("s2", len(refs["s2"])), ("unused", 40)]
    recs = [make_record(rng, refs["s1" if k % 3 else "s2"], 0 if k % 3 else 1) for k in range(3000)]
    # a 70 000-base record (it spans many members), records of known insert size (paired, first, regular)
    big_ref = {"long": bases(rng, 80000)}
    for k in range(0, 80000, 500):
        big_ref["long"] = big_ref["long"][:k] + b"G" * 40 + big_ref["long"][k + 40:]
    refs.update(big_ref)
    A.write_fasta(fasta, refs)
    contigs.append(("long", 80000))
    lr = A.encode_record(3, 100, 60, 0, [("M", 70000)], big_ref["long"][100:70100].decode(), -1, -1, 0, A.aux_field("EF", "S", 1))
    known = [A.encode_record(0, 20000 + 7 * k, 50, 0x1 | 0x40, [("M", 100)], refs["s1"][20000 + 7 * k:20100 + 7 * k].decode().upper(), 0,
                             20200, 300 + k) for k in range(40)]
    recs = recs[:1500] + [lr] + known + recs[1500:]
    bam = str(d / "a.bam")
    A.write_bam(bam, contigs, recs, member_bytes=3000)   # small members: records straddle them
    bam2 = str(d / "b.bam")
    A.write_bam(bam2, contigs, recs[::-1][:800])
    return fasta, bam, bam2, len(recs)


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("bam", [SOFT, SINGLE])
def test_fixtures_match_the_restatement(bam):
    dev, cpu = _both(FASTA, [bam], 1_000_000)
    assert_same(dev, cpu)
    assert dev.n_taken > 0


def test_reference_pins_hold_through_the_device_path():
    p = A.finish(A.count_bams_device(FASTA, [SOFT], 1_000_000, 0))
    assert (p.insert_size, p.max_del_cigar_len, p.max_ins_cigar_len, p.frac_max_softclip) == (None, 2, 4, 0.63)
    q = A.finish(A.count_bams_device(FASTA, [SINGLE], 1_000_000, 0))
    assert (q.insert_size, q.max_del_cigar_len, q.max_ins_cigar_len, q.frac_max_softclip) == (None, None, None, 0.03)


def test_synthetic_bams_match_the_restatement(synth):
    fasta, bam, bam2, n = synth
    dev, cpu = _both(fasta, [bam, bam2], 10 ** 9)
    assert_same(dev, cpu)
    # every branch was reached
    assert cpu.max_read_len >= 70000 and cpu.n_skipped > 50 and len(cpu.insert_sizes) >= 40
    assert any(k0 >= 32 for (_b, k0, _k1) in cpu.hops)                 # spill keys
    assert any(b in b"acgt" for (b, _k0, _k1) in cpu.hops)             # soft-masked keys
    assert cpu.transitions[:, 14].sum() > 0 and cpu.transitions[0:4, 4].sum() > 0 and cpu.transitions[0:4, 5].sum() > 0
    assert 70000 in cpu.insert_sizes                                   # the unpaired EF = 1 long read: end - pos


def test_num_records_cuts_at_the_exact_record(synth):
    fasta, bam, _bam2, n = synth
    _, full = _both(fasta, [bam], 10 ** 9)
    for cap in (1, 2, 17, 1499, full.n_taken - 1, full.n_taken, full.n_taken + 1, full.n_taken + 333):
        dev, cpu = _both(fasta, [bam, bam], cap)
        assert_same(dev, cpu)
        assert cpu.n_taken == min(cap, 2 * full.n_taken)


def test_json_is_identical_under_window_sizes_and_runs(synth):
    fasta, bam, bam2, _ = synth
    outs = set()
    for w in (0, 0, 1 << 16, 1 << 20, 5000):
        c = A.count_bams_device(fasta, [bam, bam2], 10 ** 9, 0, window_bytes=w)
        outs.add(A.to_json(A.finish(c)))
    assert len(outs) == 1
    assert outs == {A.to_json(A.finish(A.count_bams(fasta, [bam, bam2], 10 ** 9)))}


def test_cli_end_to_end_matches_the_restatement(tmp_path):
    def run(dev):
        r = subprocess.run([sys.executable, "-m", "varlociraptor_amd", "estimate", "alignment-properties", FASTA, "--bams", SOFT, SOFT,
                            "--device", dev], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout
    gpu, cpu = run("0"), run("cpu")
    assert gpu == cpu
    assert '"max_del_cigar_len": 2,' in gpu and '"frac_max_softclip": 0.63,' in gpu


def test_truncated_bam_is_a_clean_error(synth, tmp_path):
    fasta, bam, _, _ = synth
    raw = open(bam, "rb").read()
    cut = tmp_path / "cut.bam"
    cut.write_bytes(raw[:len(raw) // 2])               # inside a member
    with pytest.raises(A.AlignPropsError, match="truncated"):
        A.count_bams_device(fasta, [str(cut)], 10 ** 9, 0)
    d = A.inflate_bgzf(bam)
    cut2 = tmp_path / "cut2.bam"
    cut2.write_bytes(A.bgzf_compress(d[:len(d) - 37]))   # whole members, the last record cut
    with pytest.raises(A.AlignPropsError, match="truncated"):
        A.count_bams_device(fasta, [str(cut2)], 10 ** 9, 0)
    with pytest.raises(A.AlignPropsError):
        A.count_bams(fasta, [str(cut2)], 10 ** 9)


def test_cigar_past_the_contig_end_is_a_clean_error(tmp_path):
    fasta = str(tmp_path / "r.fa")
    A.write_fasta(fasta, {"c": b"ACGTACGTAC" * 10})
    good = A.encode_record(0, 10, 60, 0, [("M", 20)], ("ACGTACGTAC" * 2), -1, -1, 0)
    bad = A.encode_record(0, 90, 60, 0, [("M", 20)], "A" * 20, -1, -1, 0)
    bam = str(tmp_path / "x.bam")
    A.write_bam(bam, [("c", 100)], [good, good, bad, good])
    with pytest.raises(A.AlignPropsError, match="record 2"):
        A.count_bams_device(fasta, [bam], 10 ** 9, 0)
    with pytest.raises(A.AlignPropsError, match="record 2"):
        A.count_bams(fasta, [bam], 10 ** 9)
    dev, cpu = _both(fasta, [bam], 2)                  # the cap stops in front of it
    assert_same(dev, cpu)
