"""The cases of tests/test_gpu_fdr_stages.py are what they claim to be — checked on the CPU against fdr.fdr_threshold and numpy alone, so
that a GPU failure there is a statement about a kernel of csrc/vlr_fdr.hip and not about its input or its reference."""
import math

import numpy as np
import pytest

import fdr_cases as fc
from varlociraptor_amd import fdr


def test_sort_inputs_are_valid_keys_and_hit_the_padding_rules():
    assert fc.SORT_SIZES == (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6145, 8192, 65537)
    for n in fc.SORT_SIZES[:-1] + (6145,):
        cases = dict(fc.sort_inputs(n))
        for name, x in cases.items():
            assert x.shape == (n,) and x.dtype == np.float64 and not np.isnan(x).any() and x.max() <= 0.0, (n, name)
        two = {k: v for k, v in cases.items() if k.split("_")[0] in ("density", "step", "alternating", "sawtooth")}
        assert all(set(np.unique(v)) <= {0.0, -1.0} for v in two.values())
        assert np.isinf(cases["with_neg_inf"]).sum() >= 1
        steps = [int(k.rsplit("_", 1)[1]) for k in cases if k.startswith("step_up_")]
        assert steps == fc.step_positions(n) and all(m in steps for m in range(0, n + 1, 1024))
        assert all((cases["step_up_%d" % m] == 0.0).sum() == n - m for m in steps)
    # 6145 keys pad to 8192: the last sort block holds padding only
    npad = 2048
    while npad < 6145:
        npad <<= 1
    assert npad == 8192 and npad - 6145 >= fc.SORT_BLOCK - 1 and 6145 <= npad - fc.SORT_BLOCK + 1
    big = fc.step_positions_large(fc.LARGE_N)
    assert {1 << 20, (1 << 20) - 1, (1 << 20) + 1, fc.LARGE_N, 1023, 1024, 1025} <= set(big) and {1024 << k for k in range(11)} <= set(big) and len(big) <= 20


def test_pep_reference_and_host_formula():
    """The mpmath reference agrees with the plain expression at 1200 bits; the host's libm evaluation of the kernel's formula lies
    within 1.48 ulp of it on pep_inputs() (at p = -0.69304, next to the branch point; 1.39 was the figure on another draw of the
    same families), the linear 1 - e^p within 0.5 ulp.  PEP_ULP is not looser than that measurement plus 4."""
    import mpmath
    for p in (-270.0, -0.7, -0.693, -1e-10, -1e-300, -5.0, -740.0, -1.0):
        with mpmath.workprec(1200):
            plain = mpmath.log(1 - mpmath.exp(mpmath.mpf(p)))
            assert abs(fc.ln_one_minus_exp_mp(p) - plain) <= abs(plain) * mpmath.mpf(2) ** -100, p
    with mpmath.workprec(400):                                   # the trap the reference avoids
        bad = mpmath.log(1 - mpmath.exp(mpmath.mpf(-280.0)))
    assert bad == 0 and fc.ln_one_minus_exp_mp(-280.0) < 0
    p = fc.pep_inputs()
    assert 10000 <= len(p) <= 20000 and ((p >= -0.70) & (p <= -0.68)).sum() >= 3000
    for v in (fc.BRANCH, np.nextafter(fc.BRANCH, -np.inf), -745.2, -800.0, 0.0, -np.inf):
        assert (p == v).any()
    assert np.signbit(p[p == 0.0]).tolist() == [True, False]
    err = fc.ulp_errors(fc.ln_one_minus_exp_host(p), p)
    print("host formula: %.3f ulp at p = %r" % (err.max(), p[err.argmax()]))
    assert 1.0 < err.max() <= 1.5 and fc.PEP_ULP <= err.max() + 4.0
    q = p[np.isfinite(p) & (p != 0.0)][::5]
    with mpmath.workprec(fc.MP_BITS):
        lin = [float(abs(mpmath.mpf(float(-np.expm1(x))) + mpmath.expm1(mpmath.mpf(float(x)))) / mpmath.mpf(float(np.spacing(-np.expm1(x))))) for x in q]
    print("host 1 - e^p: %.3f ulp" % max(lin))
    assert max(lin) <= 0.5 + 1e-9
    # class comparisons: an exact -inf or 0 admits only that
    assert fc.ulp_errors(np.array([-np.inf, 0.0, -0.0, -1e-300, 5e-324]), np.array([0.0, -np.inf, -np.inf, 0.0, -np.inf])).tolist() == [0.0, 0.0, 0.0, np.inf, np.inf]


def test_scan_indices_and_addition_count():
    for n in fc.BETA_SIZES + (fc.LARGE_N, 2124):
        idx = fc.scan_indices(n)
        assert len(idx) == 64 and idx == sorted(set(idx)) and {i for i in (0, 1023, 1024, 1025, n - 1) if i < n} <= set(idx)
        if n <= 8192:
            assert set(range(0, n, 1024)) <= set(idx)
    assert {(1 << 20) - 1, 1 << 20, (1 << 20) + 1} <= set(fc.scan_indices(fc.LARGE_N))
    assert fc.scan_additions(1025) == fc.scan_additions(1 << 20) == 45 and fc.scan_additions((1 << 20) + 1) == fc.scan_additions(fc.LARGE_N) == 61
    assert fc.scan_bound(fc.LARGE_N) == (61 + 2 * 5.39) * 2.0 ** -53


@pytest.mark.parametrize("n", fc.BETA_SIZES)
def test_beta_cases_have_a_clear_boundary_and_scan_within_the_bound_in_the_kernels_order(n):
    p, alpha_ln = fc.beta_case(n)
    desc = np.sort(p)[::-1]
    status, index, thr = fc.restatement(desc, alpha_ln)
    assert status == fc.VALUE and 0 < index <= n // 2 and thr == desc[index]
    assert fc.alpha_margin(desc, alpha_ln) > 1e-6
    if n == 4097:   # ties: the boundary entry is the first of a run
        assert desc[index] == desc[index + 1] and desc[index - 1] != desc[index] and index < n // 2
    # the order of the kernels with exact terms: within the bound, far from it (ordinary inputs: a few units of 2^-53)
    term = -np.expm1(desc)
    for mode in ("subtract", "shift"):
        cum, offs = fc.emulate_device_scan(term, mode)
        q = cum + offs[np.arange(n) // 1024]
        idx = fc.scan_indices(n)
        ref = np.array(fc.scan_reference(desc, idx))
        assert np.all(np.abs(q[idx] - ref) <= 8 * 2.0 ** -53 * ref), mode
        assert np.all(np.diff(q) >= 0)


def test_large_beta_case():
    p, alpha_ln = fc.beta_case(fc.LARGE_N)
    assert len(p) == (1 << 20) + 1500 and -(-len(p) // 1024) == 1026     # two block totals in the second chunk of fdr_scan_blocks
    desc = np.sort(p)[::-1]
    assert fc.alpha_margin(desc, alpha_ln) > 1e-6
    status, index, _ = fc.restatement(desc, alpha_ln)
    assert status == fc.VALUE and index == len(p) // 2      # the boundary entry lies in scan block 512; its sum crosses 512 offsets


def test_dynamic_range_list_loses_the_offset_under_the_subtraction_only():
    desc = fc.dynamic_range_list()
    assert len(desc) == 2124 and np.all(np.diff(desc) <= 0)
    term = -np.expm1(desc)
    assert term[0] == 1e-22 and term[1024] == 1e-18 and term[-1] == 0.5
    idx = fc.scan_indices(len(desc))
    ref = np.array(fc.scan_reference(desc, idx))
    cum, offs = fc.emulate_device_scan(term, "subtract")
    assert offs[0] == 0.0 and offs[1] == 0.0 and offs[2] == pytest.approx(12.0)   # block 1 should start from 1.024e-19
    q = cum + offs[np.arange(len(desc)) // 1024]
    k = idx.index(1024)
    assert (ref[k] - q[1024]) / ref[k] == pytest.approx(0.0929, abs=1e-3)        # 9 % low: 8e14 units of 2^-53
    assert np.max(np.abs(q[idx] - ref) / ref) > 1e14 * 2.0 ** -53
    cum, offs = fc.emulate_device_scan(term, "shift")
    assert offs[0] == 0.0 and offs[1] == pytest.approx(1.024e-19, rel=1e-12)
    q = cum + offs[np.arange(len(desc)) // 1024]
    assert np.max(np.abs(q[idx] - ref) / ref) <= 8 * 2.0 ** -53 < fc.scan_bound(len(desc))
    assert np.all(np.diff(q) >= 0)


@pytest.mark.parametrize("E", fc.EDGES)
def test_planted_edges(E):
    margins = {1024: 0.0407, 2048: 0.0210, 1 << 20: 4.24e-5}
    desc, alpha_ln = fc.planted_edge(E, tie=False)
    assert len(desc) == E + 65 and np.all(np.diff(desc) < 0)
    assert fc.restatement(desc, alpha_ln) == (fc.VALUE, E, desc[E]) and desc[E] != desc[E - 1]
    pep_ln = fc.ln_one_minus_exp_host(desc)
    assert pep_ln[E] != pep_ln[E - 1]
    m = fc.alpha_margin(desc, alpha_ln)
    assert m == pytest.approx(margins[E], rel=0.01) and m > 1e-6
    tied, alpha_ln = fc.planted_edge(E, tie=True)
    assert tied[E] == tied[E - 1] and fc.ln_one_minus_exp_host(tied[E:E + 1]) == fc.ln_one_minus_exp_host(tied[E - 1:E])   # still a tie as a PEP
    assert fc.restatement(tied, alpha_ln)[:2] == (fc.VALUE, E - 1)
    assert fc.alpha_margin(tied, alpha_ln) == pytest.approx(margins[E], rel=0.01)
    # the expected FDR of entry E is below alpha in both: only the tie bars it
    assert fc.ln_fdr(tied)[E] < alpha_ln < fc.ln_fdr(tied)[E + 1]


def test_flip_case_flips_under_the_subtraction_only():
    desc, alpha_ln = fc.flip_case()
    assert len(desc) == 2125 and alpha_ln == math.log(1e-20)
    assert fc.restatement(desc, alpha_ln) == (fc.VALUE, 0, -5e-21)
    f = fc.ln_fdr(desc)
    assert f[1024] == pytest.approx(-45.970, abs=1e-3) and f[1024] > alpha_ln == pytest.approx(-46.052, abs=1e-3)
    window = 1e-9 * max(1.0, abs(alpha_ln))                       # the near-alpha nomination of fdr_search
    assert fc.alpha_margin(desc, alpha_ln) > 1e-6 > window
    term = -np.expm1(desc)
    got = {}
    for mode in ("subtract", "shift"):
        cum, offs = fc.emulate_device_scan(term, mode)
        q = cum + offs[np.arange(len(desc)) // 1024]
        with np.errstate(divide="ignore"):
            lf = np.log(q) - np.log(np.arange(1, len(desc) + 1))
        assert np.min(np.abs(lf - alpha_ln)) > window              # no fallback in either order
        pep_ln = fc.ln_one_minus_exp_host(desc)
        ok = (lf <= alpha_ln) & np.concatenate([[True], pep_ln[1:] != pep_ln[:-1]])
        got[mode] = (int(np.flatnonzero(ok)[-1]), lf[1024])
    assert got["subtract"][0] == 1024 and got["subtract"][1] == pytest.approx(-46.587, abs=1e-3)
    assert got["shift"][0] == 0 and got["shift"][1] == pytest.approx(-45.970, abs=1e-3)


def test_near_alpha_lists_sit_inside_the_nomination_window():
    from test_fdr import _threshold_reference_order
    lists = list(fc.near_alpha_lists())
    assert len(lists) == 30
    for desc, alpha_ln in lists:
        assert np.all(np.diff(desc) <= 0)
        assert fc.alpha_margin(desc, alpha_ln) <= 1e-12 < 1e-9 * max(1.0, abs(alpha_ln))
        assert _threshold_reference_order(list(desc), alpha_ln) in list(desc)


def test_status_none_cannot_be_reached():
    """VLR_FDR_NONE needs a list with no admissible entry whose first entry does not exceed alpha.  Entry 0 has no predecessor, so no tie
    bars it: it is admissible whenever its expected FDR is <= alpha, and otherwise the status is VLR_FDR_LN_ONE.  For every alpha that is
    not NaN one of the two holds, so no list is "barred by a tie" into NONE; this looks for a counterexample among tie-heavy lists.
    Only alpha = NaN fails both comparisons, and the GPU test observes the raw code with it."""
    rng = np.random.default_rng(3)
    seen = set()
    for _ in range(300):
        n = int(rng.integers(1, 8))
        desc = np.sort(rng.choice([0.0, -1e-3, -0.1, -0.693, -2.0, -np.inf], n))[::-1]
        for alpha_ln in (-np.inf, -50.0, -3.0, -0.1, 0.0):
            status, index, _ = fc.restatement(desc, alpha_ln)
            seen.add(status)
            assert status in (fc.VALUE, fc.LN_ONE)
            f0 = min(float(fc.ln_one_minus_exp_host(desc[:1])[0]), 0.0)
            assert (status == fc.LN_ONE) == (f0 > alpha_ln)
    assert seen == {fc.VALUE, fc.LN_ONE}
    assert fc.restatement(np.array([]), -3.0)[0] == fc.EMPTY
    assert fdr.fdr_threshold([], -3.0) is None
