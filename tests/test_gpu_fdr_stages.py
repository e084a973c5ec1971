"""The five kernels of csrc/vlr_fdr.hip stage by stage, through vlr_selftest_fdr_stages (the run of vlr_fdr_threshold with its stages
copied back): the sort against numpy's, the PEPs against mpmath, the prefix sums against math.fsum within a bound derived from the
number of additions, the boundary search against the restatement fdr.fdr_threshold.  The inputs come from tests/fdr_cases.py;
tests/test_fdr_cases_host.py checks on the CPU that each has the property relied on here."""
import math

import numpy as np
import pytest

import fdr_cases as fc
from varlociraptor_amd import fdr

pytestmark = pytest.mark.gpu

LN_05 = math.log(0.05)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_sort(x, st, label):
    assert np.array_equal(st["sorted"], np.sort(x)[::-1]), label
    assert np.isinf(st["sorted"]).sum() == np.isinf(x).sum(), label          # no pad -inf among the first n, none of the input's lost
    assert np.array_equal(_bits(st["prob"]), _bits(st["sorted"])), label     # without `smart` the probabilities are the keys, bit for bit


def _check_scan(st, n, label):
    """cum[i] + offset[i // 1024] at 64 indices against the exactly rounded sum of the host's terms: all terms are non-negative, each is
    within PEP_ULP ulp of the host's and passes through at most A additions (fdr_cases.scan_additions counts them in the code), so the
    relative error is at most (A + 2 PEP_ULP) 2^-53.  Over all indices the sums never decrease."""
    q = fc.running_sums(st)
    idx = fc.scan_indices(n)
    ref = np.array(fc.scan_reference(st["prob"], idx))
    err = np.abs(q[idx] - ref)
    rel = np.divide(err, ref, out=err.copy(), where=ref > 0)                 # a sum of 0 admits only 0
    k = int(np.argmax(rel))
    print("%s: scan error %.2f units of 2^-53 at index %d, bound %.2f (A = %d)" % (label, rel[k] * 2.0 ** 53, idx[k], fc.scan_bound(n) * 2.0 ** 53,
                                                                               fc.scan_additions(n)))
    assert rel[k] <= fc.scan_bound(n), (label, idx[k], q[idx[k]], ref[k])
    assert np.all(np.diff(q) >= 0), (label, int(np.argmax(np.diff(q) < 0)))
    return rel[k]


def _check_search(st, desc, alpha_ln, label):
    """No expected FDR near alpha: the device's own decision stands and equals the restatement's."""
    status, index, thr = fc.restatement(desc, alpha_ln)
    assert st["near_alpha"] == 0, label
    assert (st["status"], st["boundary"] - 1) == (status, index), label
    if status == fc.VALUE:
        assert st["threshold"] == thr == desc[index], label
    assert st["fdr0"] == pytest.approx(float(fc.ln_fdr(desc[:1])[0]), abs=1e-12), label


@pytest.mark.parametrize("n", fc.SORT_SIZES)
def test_sort(n):
    """np.sort on random, presorted, constant, -inf-bearing and two-valued inputs at the sizes on the edges of the 1024-entry scan
    blocks and the 2048-key sort blocks, with a whole sort block of padding (6145) and through the global merge phases (8192, 65537)."""
    count = 0
    for name, x in fc.sort_inputs(n):
        _check_sort(x, fdr.fdr_stages_device(x, LN_05), (n, name))
        count += 1
    assert count >= 6 + 3 + 2 * 2 + 1 + 4


def test_sort_and_scan_beyond_2_to_the_20():
    """n = 2^20 + 1500: 1026 block totals, so fdr_scan_blocks runs its second chunk of 1024 with the carry, and fdr_search reads
    offsets of blocks >= 1024.  The beta-distributed list for the sort and the sums; the sort patterns at this size as well (the
    steps at the power-of-two multiples of 1024 and around 2^20: fdr_cases.step_positions_large)."""
    n = fc.LARGE_N
    p, alpha_ln = fc.beta_case(n)
    st = fdr.fdr_stages_device(p, alpha_ln)
    _check_sort(p, st, (n, "beta"))
    assert len(st["block_offset"]) == 1026
    _check_scan(st, n, "beta %d" % n)
    _check_search(st, np.sort(p)[::-1], alpha_ln, (n, "beta"))
    # the offsets of the second chunk continue the first chunk's: each is its predecessor plus that block's total
    tot = st["cum"][1023::1024]
    assert np.allclose(np.diff(st["block_offset"]), tot[:1025], rtol=1e-9, atol=0.0)
    for name, x in fc.sort_inputs(n, steps=fc.step_positions_large(n)):
        st = fdr.fdr_stages_device(x, LN_05)
        _check_sort(x, st, (n, name))


def test_pep_stage():
    """prob = ln(1 - e^p) (`smart`) and pep_ln = ln(1 - e^prob) against mpmath, each for the f64 input the kernel had, in ulp of the
    exact value; exact values of -inf and 0 by class.  Bound: fdr_cases.PEP_ULP = 1.39 + 4 (measured on the device: 1.58)."""
    p = fc.pep_inputs()
    st = fdr.fdr_stages_device(p, LN_05, smart=True)
    _srt = np.sort(p)[::-1]
    assert np.array_equal(st["sorted"], _srt)
    assert np.signbit(st["sorted"][st["sorted"] == 0.0]).sum() == 1          # both zeros came through
    e_prob = fc.ulp_errors(st["prob"], st["sorted"])
    e_pep = fc.ulp_errors(st["pep_ln"], st["prob"])
    plain = fdr.fdr_stages_device(p, LN_05, smart=False)
    assert np.array_equal(_bits(plain["prob"]), _bits(plain["sorted"]))
    e_plain = fc.ulp_errors(plain["pep_ln"], plain["sorted"])
    for name, e, src in (("prob (smart)", e_prob, st["sorted"]), ("pep_ln (smart)", e_pep, st["prob"]), ("pep_ln", e_plain, plain["sorted"])):
        k = int(np.argmax(e))
        print("%s: %.3f ulp at input %r, bound %.2f" % (name, e[k], src[k], fc.PEP_ULP))
    for name, e, src in (("prob (smart)", e_prob, st["sorted"]), ("pep_ln (smart)", e_pep, st["prob"]), ("pep_ln", e_plain, plain["sorted"])):
        k = int(np.argmax(e))
        assert e[k] <= fc.PEP_ULP, (name, src[k], e[k])
    # the linear PEPs of block 0 alone are its prefix sums' first entry
    assert st["cum"][0] == pytest.approx(-np.expm1(st["prob"][0]), rel=4 * 2.0 ** -52)


@pytest.mark.parametrize("n", fc.BETA_SIZES)
def test_scan_and_search_on_beta_lists(n):
    p, alpha_ln = fc.beta_case(n)
    st = fdr.fdr_stages_device(p, alpha_ln)
    desc = np.sort(p)[::-1]
    _check_sort(p, st, n)
    _check_scan(st, n, "beta %d" % n)
    _check_search(st, desc, alpha_ln, n)
    assert fdr.fdr_threshold_device(p, alpha_ln) == st["threshold"]


def test_scan_with_a_block_total_2_to_the_53_above_the_sum_before_it():
    """1024 x PEP 1e-22, 1000 x 1e-18, 100 x 0.5: block 1's total (about 12) swallows the 1.024e-19 before it in `off + v`, so an
    exclusive offset formed by subtracting it again is 0 and every running sum of block 1 is up to 9 % (8e14 units of 2^-53) low.
    The same bound as everywhere else, no special case."""
    desc = fc.dynamic_range_list()
    st = fdr.fdr_stages_device(np.random.default_rng(1).permutation(desc), LN_05)
    assert np.array_equal(st["sorted"], desc)
    print("block offsets:", st["block_offset"])
    _check_scan(st, len(desc), "dynamic range")
    assert st["block_offset"][0] == 0.0 and st["block_offset"][1] == pytest.approx(1.024e-19, rel=1e-12)


@pytest.mark.parametrize("tie", (False, True))
@pytest.mark.parametrize("E", fc.EDGES)
def test_search_with_the_boundary_on_a_block_edge(E, tie):
    """The boundary entry is the first of scan block E / 1024 (for E = 2^20 its offset comes from the second chunk of
    fdr_scan_blocks); a tie with the entry before bars it and leaves E - 1.  The margins to ln alpha (0.041, 0.021, 4.2e-5) are far
    above the nomination window and the summation error."""
    desc, alpha_ln = fc.planted_edge(E, tie)
    x = np.random.default_rng(E).permutation(desc)
    st = fdr.fdr_stages_device(x, alpha_ln)
    assert np.array_equal(st["sorted"], desc)
    assert st["boundary"] - 1 == (E - 1 if tie else E) and st["near_alpha"] == 0 and st["status"] == fc.VALUE
    assert st["threshold"] == desc[E]
    if not tie:
        assert desc[E] != desc[E - 1]
    _check_search(st, desc, alpha_ln, (E, tie))
    assert fdr.fdr_threshold_device(x, alpha_ln) == desc[E]


def test_search_does_not_admit_an_entry_behind_a_lost_block_offset():
    """1024 x PEP 0.5e-20, one of 600e-20, 1100 x 0.5, alpha 1e-20: entry 1024 has ln FDR -45.970 > ln alpha = -46.052; with a block
    offset of 0 for block 1 it comes out at -46.587 and is admitted, outside the nomination window, so no host fallback helps."""
    desc, alpha_ln = fc.flip_case()
    st = fdr.fdr_stages_device(np.random.default_rng(2).permutation(desc), alpha_ln)
    assert np.array_equal(st["sorted"], desc)
    q = fc.running_sums(st)
    print("ln FDR of entry 1024: %.3f (ln alpha %.3f), block offsets %r" % (math.log(q[1024]) - math.log(1025), alpha_ln, st["block_offset"]))
    _check_search(st, desc, alpha_ln, "flip")
    assert (st["boundary"] - 1, st["status"], st["threshold"]) == (0, fc.VALUE, -5e-21)
    _check_scan(st, len(desc), "flip")


def test_near_alpha_entries_are_nominated_and_decided_in_the_reference_order():
    from test_fdr import _threshold_reference_order
    rng = np.random.default_rng(6)
    for desc, alpha_ln in fc.near_alpha_lists():
        st = fdr.fdr_stages_device(rng.permutation(desc), alpha_ln)
        want = _threshold_reference_order(list(desc), alpha_ln)
        assert st["near_alpha"] == 1, (desc, alpha_ln)
        assert st["status"] == fc.VALUE and st["threshold"] == want, (desc, alpha_ln)
        assert 0 <= st["boundary"] <= len(desc)


def test_raw_status_codes():
    """All four raw codes through the diagnostic entry (the Python wrapper of vlr_fdr_threshold maps EMPTY and NONE both to None).  No
    list is barred into VLR_FDR_NONE by a tie (tests/test_fdr_cases_host.py::test_status_none_cannot_be_reached); alpha = NaN, which
    fails every comparison of the kernel and of the host decision, is the one way to see the code."""
    st = fdr.fdr_stages_device([], LN_05)
    assert (st["status"], st["boundary"], st["near_alpha"], st["threshold"]) == (fc.EMPTY, 0, 0, 0.0)
    assert all(len(st[k]) == 0 for k in ("sorted", "prob", "pep_ln", "cum", "block_offset"))
    desc = np.array([math.log(0.5), math.log(0.4)])
    st = fdr.fdr_stages_device(desc[::-1].copy(), LN_05)
    assert (st["status"], st["threshold"], st["boundary"], st["near_alpha"]) == (fc.LN_ONE, 0.0, 0, 0)
    assert st["fdr0"] == pytest.approx(math.log(0.5), abs=1e-15) and fc.restatement(desc, LN_05)[0] == fc.LN_ONE
    desc = np.array([0.0, math.log(0.999), math.log(0.5)])                   # a certain call: PEP 0, ln FDR -inf
    st = fdr.fdr_stages_device(desc[::-1].copy(), LN_05)
    assert (st["status"], st["boundary"], st["threshold"], st["fdr0"]) == (fc.VALUE, 2, math.log(0.999), -math.inf)
    assert fc.restatement(desc, LN_05)[:2] == (fc.VALUE, 1)
    st = fdr.fdr_stages_device([1e-9, 0.0, math.log(0.99)], LN_05)          # a rounding error above ln 1 is capped before the sort
    assert st["sorted"].tolist() == [0.0, 0.0, math.log(0.99)] and st["status"] == fc.VALUE
    st = fdr.fdr_stages_device([math.log(0.99), math.log(0.5)], math.nan)
    assert (st["status"], st["boundary"], st["near_alpha"], st["threshold"]) == (fc.NONE, 0, 0, 0.0)
    assert fdr.fdr_threshold_device([math.log(0.99), math.log(0.5)], math.nan) is None
