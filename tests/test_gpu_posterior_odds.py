"""`filter-calls posterior-odds` on the device: vlr_posterior_odds_keep against the numpy restatement (exact equality of the keep
bits) and vlr_calls_filter_odds against the restatement of the command (same records, byte for byte)."""
import math
import os

import numpy as np
import pytest

from calls_consumers_util import ODDS_CASES, ODDS_IDS
from varlociraptor_amd import odds
from varlociraptor_amd.bcfio import BcfReader, BcfWriter

pytestmark = pytest.mark.gpu
EDGES = [math.log(b) for b in (3.0, 20.0, 150.0)]


def _near_edge(d):
    """|d - ln b| <= 1e-9 for b in (3, 20, 150), d = ln_other - ln_target: the only inputs on which the restatement (libm's exp,
    then comparisons with b) and the device (d against ln b) may decide differently."""
    with np.errstate(invalid="ignore"):
        near = np.zeros(len(d), bool)
        for e in EDGES:
            near |= np.abs(d - e) <= 1e-9
        return near


def _synthetic(n, seed):
    rng = np.random.default_rng(seed)
    draw = lambda m: -rng.exponential(4.0, m) * rng.choice([1.0, 10.0, 100.0], m)
    lt, lo = draw(n), draw(n)
    va = rng.choice(np.array([3, 3, 3, 3, 2, 1, 0], np.uint8), n)
    for k in range(0, n, 7):                       # special cases, spread over the array
        c = (k // 7) % 6
        if c == 0: lt[k], lo[k] = (lt[k], lt[k]) if k % 2 else (0.0, 1e-300)   # equal: None exactly; a positive d that e^d rounds away: None too
        elif c == 1: lt[k] = -np.inf               # -inf target: factor +inf
        elif c == 2: lo[k] = -np.inf               # -inf other: factor 0
        elif c == 3: lt[k] = lo[k] = -np.inf       # both: NaN factor
        elif c == 4: lo[k] = lt[k] + math.log(19.0)
        elif c == 5: lo[k] = lt[k] + math.log(151.0)
    while True:                                    # redraw the offenders: nothing is left out of the comparison
        with np.errstate(invalid="ignore"):
            bad = np.flatnonzero(_near_edge(lo - lt))
        if not len(bad):
            break
        lt[bad], lo[bad] = draw(len(bad)), draw(len(bad))
    return lt, lo, va


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 10 ** 6])
def test_kernel_keep_bits_equal_the_restatement(n):
    lt, lo, va = _synthetic(n, seed=n + 1)
    for lvl in range(5):
        got = odds.keep_bits(lt, lo, va, lvl, device=0)
        want = odds.keep_bits(lt, lo, va, lvl)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (n, lvl, np.flatnonzero(got != want)[:5])
    if n >= 1000:
        assert odds.keep_bits(lt, lo, va, 4).sum() > odds.keep_bits(lt, lo, va, 1).sum() > 0
        assert not odds.keep_bits(lt, lo, va, 0, device=0).any()


def _no_allele_near_an_edge(path, events):
    r = BcfReader(path)
    t, o = odds.target_tags(events), odds.other_tags(r.header_lines, events)
    d = [b - a for rec in r for a, b in odds.allele_sums(rec, t, o) if a is not None and b is not None]
    return not _near_edge(np.array(d, np.float64)).any()


def _check_file(src, events, tmp_path):
    r = BcfReader(src)
    recs = list(r)
    for lvl in (0, 2, 3):
        out = str(tmp_path / ("kept%d.bcf" % lvl))
        kept_n, total_n = odds.filter_calls_native(src, out, events, lvl, device=0)
        want = odds.filter_by_odds(recs, r.header_lines, events, lvl)
        ro = BcfReader(out)
        got = list(ro)
        assert total_n == len(recs) and kept_n == len(got) == len(want)
        assert [g["raw"] for g in got] == [w["raw"] for w in want]
        assert ro.header_text == r.header_text
    return len(want)


@pytest.mark.parametrize("path,events", ODDS_CASES, ids=ODDS_IDS)
def test_native_filter_matches_restatement_on_golden_files(path, events, tmp_path):
    """No golden file has an allele within 1e-9 of a boundary (checked here with the restatement), so none is left out."""
    assert _no_allele_near_an_edge(path, events)
    _check_file(path, events, tmp_path)


def test_native_filter_lower_case_event_is_summed_on_both_sides(tmp_path):
    path = ODDS_CASES[1][0]
    r = BcfReader(path)
    recs = list(r)
    out = str(tmp_path / "k.bcf")
    kept_n, _ = odds.filter_calls_native(path, out, ["somatic"], 3, device=0)
    want = odds.filter_by_odds(recs, r.header_lines, ["somatic"], 3)
    assert kept_n == len(want) != len(odds.filter_by_odds(recs, r.header_lines, ["SOMATIC"], 3))
    assert [g["raw"] for g in BcfReader(out)] == [w["raw"] for w in want]


def _header(desc_suffix=" (PHRED)"):
    tags = ["SOMATIC", "GERMLINE", "ABSENT", "ARTIFACT"]
    h = "##fileformat=VCFv4.2\n##contig=<ID=1>\n"
    for t in tags:
        h += '##INFO=<ID=PROB_%s,Number=A,Type=Float,Description="Posterior probability for %s variant%s">\n' % (t, t.lower(), desc_suffix)
    return h + '##FORMAT=<ID=AF,Number=A,Type=Float,Description="allele frequency">\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts\n'


def test_native_filter_on_50000_records(tmp_path):
    rng = np.random.default_rng(5)
    src = str(tmp_path / "calls.bcf")
    n = 50000
    p = rng.dirichlet([0.3, 0.3, 0.3, 0.1], n)
    ph = np.round(-10.0 * np.log10(np.maximum(p, 1e-300)), 3)
    with BcfWriter(src, _header()) as w:
        for i in range(n):
            vals = ["%.3f" % x for x in ph[i]]
            if i % 97 == 0:
                vals[0] = "."          # missing target value
            if i % 89 == 0:
                vals[2] = "nan"
            info = "PROB_SOMATIC=%s;PROB_GERMLINE=%s;PROB_ABSENT=%s" % tuple(vals[:3]) + ("" if i % 5 == 0 else ";PROB_ARTIFACT=%s" % vals[3])
            w.write_line("1\t%d\t.\t%s\t%s\t.\t.\t%s\tAF\t0.5" % (i + 1, "ACGT"[i % 4], "CGTA"[i % 4], info))
    if not _no_allele_near_an_edge(src, ["SOMATIC"]):
        pytest.fail("the seeded file has an allele within 1e-9 of a boundary: change the seed")
    kept = _check_file(src, ["SOMATIC"], tmp_path)
    assert 1000 < kept < n - 1000


def test_native_filter_refuses_a_non_phred_header(tmp_path):
    src, out = str(tmp_path / "lin.bcf"), str(tmp_path / "out.bcf")
    with BcfWriter(src, _header(" (linear)")) as w:
        w.write_line("1\t1\t.\tA\tC\t.\t.\tPROB_SOMATIC=0.5;PROB_ABSENT=0.5\tAF\t0.5")
    with pytest.raises(Exception, match="not PHRED scaled"):
        odds.filter_calls_native(src, out, ["SOMATIC"], 3, device=0)
    assert not os.path.exists(out)
