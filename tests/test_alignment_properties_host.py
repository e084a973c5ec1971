"""`estimate alignment-properties` on the host: the pure-Python restatement of alignment_properties.rs (varlociraptor_amd/alignprops.py)
against the reference's own pinned numbers, hand-built records for each restated quirk, the finishing math, the JSON writer and
loader, the default record count from BAI / CSI indices, and the CLI's errors.  The HIP path is compared against this restatement in
tests/test_gpu_alignment_properties.py."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from varlociraptor_amd import alignprops as A
from varlociraptor_amd import realign

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = os.path.join(ROOT, "tests", "golden", "alignment_properties")
FASTA = os.path.join(FX, "chr10.fa")
SOFT = os.path.join(FX, "tumor-first30000.reads_with_soft_clips.bam")
SINGLE = os.path.join(FX, "tumor-first30000.bunch_of_reads_made_single_ended.bam")


def _rec(pos, cigar, seq, flag=0x1 | 0x40, mapq=60, tid=0, mtid=0, tlen=0, aux=b""):
    ops = {"M": 0, "I": 1, "D": 2, "N": 3, "S": 4, "H": 5, "P": 6, "=": 7, "X": 8}
    return A.Record(tid, pos, mapq, flag, [(ops[o], l) for o, l in cigar], seq.encode(), mtid, tlen, aux, 0)


def _stats(rec, ref):
    c = A.Counts()
    irregular, end = A.cigar_stats(rec, ref, c, "test")
    return c, irregular, end


# ------------------------------------------------------------------------------------------------ the reference's pinned numbers
def test_soft_clip_fixture_reproduces_the_reference_test():
    """alignment_properties.rs:1083-1100 test_estimate_all_reads_have_short_clips."""
    p, c = A.estimate(FASTA, [SOFT], 1_000_000)
    assert p.insert_size is None
    assert (p.max_del_cigar_len, p.max_ins_cigar_len, p.frac_max_softclip) == (2, 4, 0.63)
    assert c.n_taken > 0


def test_single_end_fixture_reproduces_the_reference_test():
    """alignment_properties.rs:1102-1120 test_estimate_all_reads_single_end."""
    p, _ = A.estimate(FASTA, [SINGLE], 1_000_000)
    assert (p.insert_size, p.max_del_cigar_len, p.max_ins_cigar_len, p.frac_max_softclip) == (None, None, None, 0.03)


# ------------------------------------------------------------------------------------------------ quirks, record by record
def test_deletion_backward_extension_skips_the_base_in_front():
    ref = b"AAGAACC"
    # D2 at rpos 3 over "AA": forward stops at C; backward reads ref[..2] reversed = A, A (ref[2] = G is skipped): len 2 + 2
    c, irregular, end = _stats(_rec(0, [("M", 3), ("D", 2), ("M", 2)], "AAGCC"), ref)
    assert irregular and end == 7
    assert c.hops[(ord("A"), 4, 2)] == 1
    T = c.transitions
    assert T[0, 0] >= 2 and T[0, 6] == 1          # match_A -> match_A by l, match_A -> HopAX once
    assert T[6, 6] == 4                           # num_hops = len - (l - 2) = 4
    assert T[6, A.state_match(ord("C"))] == 0     # exit at ref[rpos + len + 1] = ref[8]: past the end, not counted
    assert T[0:4, A.GAP_X].sum() == 0             # a homopolymer deletion of length 2 is not a gap


def test_single_base_deletion_counts_as_gap_and_hop():
    ref = b"CCATTGG"
    # D1 at rpos 2 ("A"): homopolymer of one; extension: forward T stops, backward ref[..1] = C: len 1 < 2, no hop; gap (l == 1)
    c, _, _ = _stats(_rec(0, [("M", 2), ("D", 1), ("M", 4)], "CCTTGG"), ref)
    assert not c.hops.get((ord("A"), 1, 0))
    T = c.transitions
    assert T[0, A.GAP_X] == 1 and T[A.GAP_X, A.GAP_X] == 0
    assert T[A.GAP_X, A.state_match(ref[2 + 1 + 1])] == 1   # exit at ref[rpos + l + 1]


def test_insertion_key_base_and_hop_key():
    ref = b"GGcAAT"
    # I2 "CC" at rpos 3: ref[3] = 'A' is not the inserted base: key base = qseq[qpos] = 'C'; backward ref[..3] = c, G: len 2 + 1
    c, _, _ = _stats(_rec(0, [("M", 3), ("I", 2), ("M", 3)], "GGCCCAAT"), ref)
    assert c.hops[(ord("C"), 1, 2)] == 1 and c.hops[(ord("G"), 2, 2)] == 1 and c.hops[(ord("A"), 2, 2)] == 1   # + the match runs
    assert len(c.hops) == 3
    T = c.transitions
    assert T[1, 9] == 1 and T[9, 9] == 3          # match_C -> HopCY, num_hops = 3 - 0
    assert T[9, A.state_match(ref[4])] == 1       # exit at ref[rpos + 1]
    # the same insertion where ref[rpos] (lower case) equals the inserted base: the raw reference byte is the key base
    ref2 = b"GGAcAT"
    c2, _, _ = _stats(_rec(0, [("M", 3), ("I", 1), ("M", 3)], "GGACcAT".upper()), ref2)
    assert (ord("c"), 1, 1) in c2.hops


def test_match_runs_use_raw_bytes_within_one_operation():
    ref = b"aaaAAAN"
    c, _, _ = _stats(_rec(0, [("M", 3), ("=", 4)], "AAAAAAN"), ref)
    # 'a' x3 (lower case, its own counter) and 'A' x3 in the second operation; N matches N but 'N' runs of 1 count nothing
    assert c.hops == {(ord("a"), 3, 3): 1, (ord("A"), 3, 3): 1}
    T = c.transitions
    assert T[0, 0] == 2 + 2                       # windows inside each operation only (no a -> A window across the boundary)
    assert T[0, A.OTHER] == 1                     # A -> N: the Other state receives counts


def test_mismatched_run_and_short_runs_do_not_count():
    c, _, _ = _stats(_rec(0, [("M", 4)], "CCAT"), b"AAAT")
    assert c.hops == {}


def test_hard_clip_and_soft_clip_make_a_record_irregular():
    _, irr, _ = _stats(_rec(0, [("H", 5), ("M", 3)], "ACG"), b"ACGT")
    assert irr
    c, irr2, _ = _stats(_rec(0, [("S", 1), ("M", 3)], "TACG"), b"ACGT")
    assert irr2 and c.frac_max_softclip == 0.25 and c.n_softclips == 1


def test_cigar_past_the_contig_is_an_error():
    with pytest.raises(A.AlignPropsError):
        _stats(_rec(2, [("M", 5)], "ACGTA"), b"ACGTAC")
    with pytest.raises(A.AlignPropsError):
        _stats(_rec(0, [("M", 2), ("D", 8)], "AC"), b"ACGT")


def test_ef_tag_of_every_integer_type_behind_other_aux_fields():
    lead = (A.aux_field("XA", "A", "q") + A.aux_field("XZ", "Z", "hello") + A.aux_field("XH", "H", "1AE3") + A.aux_field("Xf", "f", 1.5)
            + A.aux_field("XB", "B", ("s", [1, -2, 3])) + A.aux_field("Xi", "i", -7))
    for t in "cCsSiI":
        assert A.aux_ef_is_one(lead + A.aux_field("EF", t, 1))
        assert not A.aux_ef_is_one(lead + A.aux_field("EF", t, 0))
    assert not A.aux_ef_is_one(lead + A.aux_field("EF", "f", 1.0))
    assert not A.aux_ef_is_one(lead + A.aux_field("EF", "A", "1"))
    assert not A.aux_ef_is_one(A.aux_field("EF", "C", 2) + A.aux_field("EF", "C", 1))   # the first EF decides


# ------------------------------------------------------------------------------------------------ finishing math
def test_percentile_is_r8():
    rng = np.random.default_rng(3)
    for n in (1, 2, 3, 7, 20, 101, 1000):
        v = list(rng.integers(100, 600, size=n).astype(float))
        for p in (5, 95):
            want = float(np.quantile(np.array(v), p / 100, method="median_unbiased"))
            assert A.percentile_r8(v, p) == pytest.approx(want, rel=0, abs=1e-9)
    assert A.percentile_r8([5.0, 1.0], 5) == 1.0 and A.percentile_r8([5.0, 1.0], 95) == 5.0


def test_insert_size_mean_and_sample_sd():
    v = list(range(100, 200)) + [5000, 1]
    mean, sd = A.insert_size(v)
    lo, hi = A.percentile_r8([float(x) for x in v], 5), A.percentile_r8([float(x) for x in v], 95)
    kept = [x for x in v if lo <= x <= hi]
    assert mean == pytest.approx(np.mean(kept), rel=1e-15)
    assert sd == pytest.approx(np.std(kept, ddof=1), rel=1e-12)
    m1, s1 = A.insert_size([312])
    assert m1 == 312.0 and math.isnan(s1)           # one kept value: sd NaN (written as null)
    assert A.insert_size([]) is None


def test_gap_and_hop_parameters_and_their_fallbacks():
    T = np.zeros((16, 16), dtype=np.int64)
    assert A.gap_params(T) is None and A.hop_params(T) is None
    T[0, 0] = 100000
    T[0, A.GAP_X], T[A.GAP_X, A.GAP_X], T[A.GAP_X, 0] = 200, 150, 200
    T[0, A.GAP_Y], T[A.GAP_Y, A.GAP_Y], T[A.GAP_Y, 0] = 120, 99, 120
    assert A.gap_params(T) is None                   # GapY extension below 100
    T[A.GAP_Y, A.GAP_Y] = 300
    g = A.gap_params(T)
    from_match = int(T[0:4, 0:14].sum())
    assert g.prob_insertion_artifact == math.log(200 / from_match)       # deletions (GapX) feed prob_insertion_*
    assert g.prob_insertion_extend_artifact == math.log(150 / 350)
    assert g.prob_deletion_artifact == math.log(120 / from_match)
    assert g.prob_deletion_extend_artifact == math.log(300 / 420)
    for m in range(4):
        T[m, m] = max(T[m, m], 1000)
        T[m, 6 + 2 * m], T[6 + 2 * m, 6 + 2 * m] = 10, 95
        T[m, 7 + 2 * m], T[7 + 2 * m, 7 + 2 * m] = 5, 90
    assert A.hop_params(T) is None                   # start + extend = 95 for HopY
    T[3, 13] = 20
    assert A.hop_params(T) is None
    for m in range(4):
        T[m, 7 + 2 * m] = 20
    h = A.hop_params(T)
    assert h.prob_seq_homopolymer[1] == math.log(105 / int(T[1, 0:14].sum()))
    assert h.prob_ref_homopolymer[2] == math.log(110 / int(T[2, 0:14].sum()))
    assert tuple(h.prob_seq_extend_homopolymer) == tuple(h.prob_seq_homopolymer)


def test_wildtype_model():
    hops = {(65, 5, 5): 30, (97, 5, 5): 5, (67, 7, 2): 12, (67, 1, 2): 3}   # deletion (len 7, l 5) -> 5; insertion (l 2) -> -1
    m = A.wildtype_model(hops)
    n = 30 + 12
    assert m == {-1: 3 / n, 0: 35 / n, 5: 12 / n}
    z = A.wildtype_model({(65, 2, 2): 3})
    assert z == {0: math.inf}                        # denominator 0: non-finite, written as null
    assert A.wildtype_model({}) == {}


# ------------------------------------------------------------------------------------------------ JSON and loading
def test_ryu_number_formatting():
    cases = {3.0: "3.0", 0.63: "0.63", 1e-5: "0.00001", 1e-6: "1e-6", 1.5e-7: "1.5e-7", 312.25: "312.25", 1e16: "1e16",
             1.2345e16: "1.2345e16", 1234567890123456.0: "1234567890123456.0", -12.785891140783116: "-12.785891140783116",
             math.inf: "null", -math.inf: "null", math.nan: "null", 0.0: "0.0", 123e-9: "1.23e-7"}
    for x, s in cases.items():
        assert A.ryu(x) == s, (x, A.ryu(x))


def test_json_layout_and_load_round_trip():
    p, _ = A.estimate(FASTA, [SOFT], 1_000_000)
    p.insert_size = (312.5, math.nan)
    p.wildtype_homopolymer_error_model = {3: 0.25, -2: 0.5, 0: math.inf}
    text = A.to_json(p)
    lines = text.split("\n")
    keys = [l.strip().split('"')[1] for l in lines if l.startswith('  "')]
    assert keys == ["insert_size", "max_del_cigar_len", "max_ins_cigar_len", "frac_max_softclip", "max_read_len", "max_mapq",
                    "gap_params", "hop_params", "wildtype_homopolymer_error_model", "initial"]
    assert '    "sd": null' in lines and '  "initial": false' == lines[-2] and lines[-1] == "}"
    assert '  "max_del_cigar_len": 2,' in lines and '  "frac_max_softclip": 0.63,' in lines
    model = text[text.index('"wildtype_homopolymer_error_model"'):]
    assert model.index('"-2"') < model.index('"0": null') < model.index('"3": 0.25')
    q = A.load(text)
    assert q.gap_params == p.gap_params and tuple(q.hop_params.prob_seq_homopolymer) == (-math.inf,) * 4
    assert isinstance(q.gap_params, realign.GapParams) and isinstance(q.hop_params, realign.HopParams)
    assert q.max_del_cigar_len == 2 and q.frac_max_softclip == 0.63 and q.insert_size[0] == 312.5 and math.isnan(q.insert_size[1])
    assert A.to_json(q) == text


def test_load_ignores_extra_fields_and_applies_defaults(tmp_path):
    f = tmp_path / "props.json"
    f.write_text('{"insert_size": null, "max_del_cigar_len": null, "max_ins_cigar_len": 3, "frac_max_softclip": null, '
                 '"max_read_len": 151, "cigar_counts": {"whatever": 1}, "gap_params": {"prob_insertion_artifact": -10.0, '
                 '"prob_deletion_artifact": null, "prob_insertion_extend_artifact": -1.0, "prob_deletion_extend_artifact": null}}')
    q = A.load(str(f))
    assert q.max_mapq == 60 and q.max_ins_cigar_len == 3
    assert q.gap_params.prob_deletion_artifact == -math.inf and q.gap_params.prob_insertion_artifact == -10.0
    assert q.hop_params == realign.HopParams() and q.wildtype_homopolymer_error_model == A.DEFAULT_WILDTYPE_MODEL


# ------------------------------------------------------------------------------------------------ default record count
def test_index_mapped_counts_match_the_records_and_the_default_count():
    d = A.inflate_bgzf(SOFT)
    _contigs, o = A.bam_header(d)
    mapped = sum(1 for r in A.iter_records(d, o) if not r.flag & A.FLAG_UNMAPPED and r.tid >= 0)
    assert A.index_mapped(SOFT + ".bai") == mapped == A.index_mapped(SOFT + ".csi")
    assert A.num_alignments([SOFT, SOFT], required=True) == 2 * mapped
    b = A.chi2_1_inverse_cdf(1.0 - 0.1 / 82)
    assert math.erfc(math.sqrt(b / 2)) == pytest.approx(0.1 / 82, rel=1e-12)
    # with the finite-population correction the count needed is about every alignment in the file
    assert A.default_num_records(mapped) == mapped
    assert A.default_num_records(None) > 10 ** 13


def test_num_records_caps_across_repeated_files():
    _, c1 = A.estimate(FASTA, [SOFT], None)
    _, c2 = A.estimate(FASTA, [SOFT, SOFT], 5 + c1.n_taken)
    assert c2.n_taken == c1.n_taken + 5
    _, c3 = A.estimate(FASTA, [SOFT], 7)
    assert c3.n_taken == 7


# ------------------------------------------------------------------------------------------------ CLI
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "varlociraptor_amd", "estimate", "alignment-properties", *args], cwd=ROOT,
                          capture_output=True, text=True)


def test_cli_needs_an_index_without_num_records(tmp_path):
    bam = tmp_path / "x.bam"
    shutil.copyfile(SINGLE, bam)
    r = _cli(FASTA, "--bams", str(bam), "--device", "cpu")
    assert r.returncode != 0 and "index" in r.stderr
    r2 = _cli(FASTA, "--bams", str(bam), "--num-records", "100", "--device", "cpu")
    assert r2.returncode == 0, r2.stderr
    assert '"frac_max_softclip": 0.03' in r2.stdout


def test_cli_contig_missing_from_the_reference(tmp_path):
    fa = tmp_path / "other.fa"
    A.write_fasta(str(fa), {"chr1": b"ACGT" * 50})
    r = _cli(str(fa), "--bams", SINGLE, "--device", "cpu")
    assert r.returncode != 0 and "chr10" in r.stderr and "missing" in r.stderr
