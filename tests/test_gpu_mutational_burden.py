"""`estimate mutational-burden` on the device: vlr_range_group_lse against the numpy restatement, its determinism, and
vlr_calls_mutational_burden (record pass + reduction in the engine) against the restatement of the command."""
import io
import math

import numpy as np
import pytest

from calls_consumers_util import CODING, TMB_EVENTS, TMB_VCF, TUMOR_AF, edited_tmb_vcf
from varlociraptor_amd import bcfio, burden
from varlociraptor_amd.bcfio import BcfReader, BcfWriter

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def _bound(m_cell, want):
    """A sum of m non-negative terms in another order moves by at most (m - 1) * 2^-53 relative; exp / ln1p add a few ulp."""
    return (2.0 * m_cell + 64.0) * U * np.maximum(1.0, np.abs(want))


def _ranges(R):
    if R == 1:
        return burden.ranges("multibar", 0.2)
    if R == 19:
        return burden.ranges("hist")
    return burden.ranges("curve")


def _entries(n, G, lo, hi, seed):
    rng = np.random.default_rng(seed)
    vaf = rng.random(n, dtype=np.float32)
    bounds = np.concatenate([lo, hi[np.isfinite(hi)], [1.0]]).astype(np.float32)   # many VAFs exactly on range bounds after widening
    on = rng.random(n) < 0.3
    vaf[on] = rng.choice(bounds, int(on.sum()))
    vaf = vaf.astype(np.float64)
    lp = -rng.random(n) * rng.choice([1.0, 50.0, 1500.0], n)                     # 0 .. -1500: terms below the f64 range beside the maximum
    lp[rng.random(n) < 0.01] = -np.inf
    live = [g for g in range(G) if G == 1 or g % 5 != 3]                          # some groups stay empty
    grp = rng.choice(np.array(live, np.int32), n).astype(np.int32) if n else np.zeros(0, np.int32)
    return vaf, lp, grp


def _counts(vaf, grp, lo, hi, G):
    c = np.zeros((len(lo), G))
    for r in range(len(lo)):
        c[r] = np.bincount(grp[(lo[r] <= vaf) & (vaf < hi[r])], minlength=G)
    return c


@pytest.mark.parametrize("G", [1, 14, 28])
@pytest.mark.parametrize("R", [1, 19, 100])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 10 ** 6])
def test_kernel_matches_restatement(n, R, G):
    lo, hi = _ranges(R)
    vaf, lp, grp = _entries(n, G, lo, hi, seed=n * 1000 + R * 31 + G)
    got = burden.range_group_lse(vaf, lp, grp, lo, hi, G, device=0)
    want = burden.range_group_lse(vaf, lp, grp, lo, hi, G)
    assert got.shape == want.shape == (R, G)
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    m = _counts(vaf, grp, lo, hi, G)
    err = np.abs(got[fin] - want[fin])
    assert np.all(err <= _bound(m[fin], want[fin])), (n, R, G, float(err.max()) if err.size else 0.0)
    again = burden.range_group_lse(vaf, lp, grp, lo, hi, G, device=0)
    assert got.tobytes() == again.tobytes()


def test_kernel_limits_and_nan():
    lo, hi = np.linspace(0.0, 0.9, 128), np.full(128, np.inf)
    G = 14 * 16
    vaf, lp, grp = _entries(200000, G, lo, hi, seed=3)
    got = burden.range_group_lse(vaf, lp, grp, lo, hi, G, device=0)       # the group-tiled path
    want = burden.range_group_lse(vaf, lp, grp, lo, hi, G)
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.array_equal(fin, np.isfinite(got))
    assert np.all(np.abs(got[fin] - want[fin]) <= _bound(_counts(vaf, grp, lo, hi, G)[fin], want[fin]))
    lp2 = lp.copy()
    lp2[7] = np.nan
    got2 = burden.range_group_lse(vaf, lp2, grp, lo, hi, G, device=0)
    hit = (lo <= vaf[7]) & (vaf[7] < hi)
    assert np.all(np.isnan(got2[hit, grp[7]])) and hit.any()
    rest = np.ones_like(got2, bool)
    rest[hit, grp[7]] = False
    assert got2[rest].tobytes() == got[rest].tobytes()
    with pytest.raises(Exception, match="outside"):
        _raw_bad_group()


def _raw_bad_group():
    from varlociraptor_amd import engine
    L = engine.lib()
    v = np.array([0.5]); p = np.array([-1.0]); g = np.array([5], np.int32); lo = np.array([0.0]); hi = np.array([1.0]); out = np.zeros(2)
    rc = L.vlr_range_group_lse(0, 1, v.ctypes.data, p.ctypes.data, g.ctypes.data, 1, lo.ctypes.data, hi.ctypes.data, 2, out.ctypes.data)
    assert rc != 0
    raise engine.EngineError(rc, L.vlr_last_error().decode())


def _fixture_bcf(tmp_path, edited=True):
    v, b = str(tmp_path / "x.vcf"), str(tmp_path / "x.bcf")
    if edited:
        edited_tmb_vcf(v, tumor_af=TUMOR_AF)
    bcfio.vcf_to_bcf(v if edited else TMB_VCF, b)
    return b


@pytest.mark.parametrize("mode", ["table", "curve", "hist", "multibar"])
def test_command_rows_match_restatement_on_the_edited_fixture(mode, tmp_path):
    b = _fixture_bcf(tmp_path)
    samples = ["tumor", "normal"]
    dev, host = io.StringIO(), io.StringIO()
    got = burden.estimate(b, TMB_EVENTS, samples, 3e7, mode, cutoff=0.2, device=0, out=dev)
    want = burden.estimate(b, TMB_EVENTS, samples, 3e7, mode, cutoff=0.2, device="cpu", out=host)
    key = lambda r: tuple((k, v) for k, v in r.items() if k != "mb")
    assert [key(r) for r in got] == [key(r) for r in want] and len(got) > 0
    # entries per cell, from the restatement's record pass
    by_sample = mode == "multibar"
    lo, hi = burden.ranges(mode, 0.2)
    rd = BcfReader(b)
    vaf, _, grp = burden.collect_entries(rd, rd.samples, TMB_EVENTS, samples, by_sample)
    counts = _counts(vaf, grp, lo, hi, (2 if by_sample else 1) * burden.N_SIG)
    for g, w in zip(got, want):
        cell = burden.SIGNATURES.index(w["vartype"]) + (samples.index(w["sample"]) * burden.N_SIG if by_sample else 0)
        m_cell = counts[w["_range"], cell]
        assert m_cell >= 1
        # The kernel bound B = (2 m_cell + 64) 2^-53 max(1, |ln value|) carried through mb = e^c / size * 1e6.  Either side computes
        # e^c (libm: below 1 ulp = 2 * 2^-53 relative), one division and one multiplication (2^-53 each): mb_computed = mb_true (1 + e),
        # |e| <= 4 * 2^-53 to first order.  So |got - want| <= want * ((e^B - 1) + 8 * 2^-53): e^B from the two ln values, 4 * 2^-53
        # from each side's own rounding.
        c_want = math.log(w["mb"] / 1000000.0 * 3e7)
        tol = w["mb"] * (math.expm1(float(_bound(m_cell, c_want))) + 8 * U)
        assert abs(g["mb"] - w["mb"]) <= tol, (g, w, m_cell)


def test_file_path_chunking_gives_the_same_bits_and_counts(tmp_path):
    """The engine uploads the entries of a file in pieces; the same entries in one piece through vlr_range_group_lse give identical
    bits.  200 000 records, two samples, multibar; an unknown sample name is an error."""
    rng = np.random.default_rng(11)
    n = 200000
    hdr = "##fileformat=VCFv4.2\n##contig=<ID=1>\n"
    for e in ("SOMATIC_TUMOR_LOW", "SOMATIC_TUMOR_HIGH", "ABSENT"):
        hdr += '##INFO=<ID=PROB_%s,Number=A,Type=Float,Description="Posterior probability for event %s (PHRED)">\n' % (e, e.lower())
    hdr += '##INFO=<ID=ANN,Number=.,Type=String,Description="Functional annotations">\n##FORMAT=<ID=AF,Number=A,Type=Float,Description="allele frequency">\n'
    hdr += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tnormal\ttumor\n"
    ann = "%s|missense_variant|MODERATE|G|ENSG|transcript|ENST|%s|1/2|c.1A>C|p.K1N|1/10|1/9|%s||"
    alleles = [("A", "C"), ("C", "T"), ("G", "A"), ("T", "G"), ("AC", "A"), ("A", "AGG"), ("AC", "GT"), ("ACG", "TT"), ("C", "G"), ("T", "A")]
    ph = np.round(rng.exponential(20.0, (n, 2)), 2)
    af = np.round(rng.random((n, 2)), 3)
    src = str(tmp_path / "big.bcf")
    with BcfWriter(src, hdr) as w:
        for i in range(n):
            ref, alt = alleles[i % len(alleles)]
            coding = i % 3 != 0
            info = "PROB_SOMATIC_TUMOR_LOW=%s;PROB_ABSENT=3" % ph[i, 0] + ("" if i % 11 == 0 else ";PROB_SOMATIC_TUMOR_HIGH=%s" % ph[i, 1])
            if i % 13:
                info += ";ANN=" + ann % (alt, "protein_coding" if coding else "lincRNA", "3/99" if i % 7 else "")
            w.write_line("1\t%d\t.\t%s\t%s\t.\t.\t%s\tAF\t%s\t%s" % (i + 1, ref, alt, info, "." if i % 17 == 0 else af[i, 0], af[i, 1]))
    events, samples = ["SOMATIC_TUMOR_LOW", "SOMATIC_TUMOR_HIGH"], ["tumor", "normal"]
    lo, hi = burden.ranges("multibar", 0.2)
    got, n_ent = burden.cells_native(src, events, samples, True, lo, hi, device=0)
    r = BcfReader(src)
    vaf, lp, grp = burden.collect_entries(r, r.samples, events, samples, True)
    assert n_ent == len(vaf) > 100000
    one_piece = burden.range_group_lse(vaf, lp, grp, lo, hi, 28, device=0)
    assert got.tobytes() == one_piece.tobytes()
    want = burden.range_group_lse(vaf, lp, grp, lo, hi, 28)
    fin = np.isfinite(want)
    assert np.array_equal(np.isneginf(got), np.isneginf(want)) and fin.sum() >= 16
    assert np.all(np.abs(got[fin] - want[fin]) <= _bound(_counts(vaf, grp, lo, hi, 28)[fin], want[fin]))
    lo, hi = burden.ranges("curve")
    got, _ = burden.cells_native(src, events, samples, False, lo, hi, device=0)
    vaf, lp, grp = burden.collect_entries(BcfReader(src), r.samples, events, samples, False)
    assert got.tobytes() == burden.range_group_lse(vaf, lp, grp, lo, hi, 14, device=0).tobytes()
    with pytest.raises(Exception, match="Sample nosuch not found"):
        burden.cells_native(src, events, ["tumor", "nosuch"], True, lo, hi, device=0)


def test_unedited_fixture_gives_the_no_records_error(tmp_path):
    b = _fixture_bcf(tmp_path, edited=False)
    with pytest.raises(Exception, match="no valid records were found"):
        burden.cells_native(b, TMB_EVENTS, ["tumor"], False, *burden.ranges("table"), device=0)


def test_non_acgt_snv_names_the_record(tmp_path):
    v, b = str(tmp_path / "n.vcf"), str(tmp_path / "n.bcf")
    edited_tmb_vcf(v, tumor_af=TUMOR_AF)
    lines = open(v).read().split("\n")
    k = [i for i, l in enumerate(lines) if l and not l.startswith("#")][0]
    f = lines[k].split("\t")
    f[4] = "N"
    lines[k] = "\t".join(f)
    open(v, "w").write("\n".join(lines))
    bcfio.vcf_to_bcf(v, b)
    with pytest.raises(Exception, match="1:10007"):
        burden.cells_native(b, TMB_EVENTS, ["tumor"], False, *burden.ranges("table"), device=0)
    with pytest.raises(ValueError, match="1:10007"):
        burden.cells_host(b, TMB_EVENTS, ["tumor"], False, *burden.ranges("table"))
