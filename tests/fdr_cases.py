"""Inputs of tests/test_gpu_fdr_stages.py: what the five kernels of csrc/vlr_fdr.hip are fed, stage by stage, and the references they
are held against.  tests/test_fdr_cases_host.py checks on the CPU that every case has the property its GPU test relies on."""
import functools
import math

import numpy as np

from varlociraptor_amd import fdr

EMPTY, VALUE, LN_ONE, NONE = 0, 1, 2, 3          # VLR_FDR_* (include/vlr.h)

SCAN_BLOCK = 1024                                  # entries per workgroup of fdr_pep_scan / fdr_search
SORT_BLOCK = 2048                                  # keys per workgroup of fdr_bitonic_local
LARGE_N = (1 << 20) + 1500                         # more than 1024 scan blocks: the second chunk of fdr_scan_blocks

# ------------------------------------------------------------------------------------------------ sort
# 6145 pads to 8192 with one whole sort block of padding; the sizes around 1024 / 2048 / 4096 sit on scan- and sort-block edges
SORT_SIZES = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6145, 8192, 65537)


def step_positions(n):
    """Every multiple of 1024 up to n, +-1."""
    return sorted({m + d for m in range(0, n + 1, 1024) for d in (-1, 0, 1) if 0 <= m + d <= n})


def step_positions_large(n):
    """At LARGE_N a step at every multiple of 1024, +-1, in both directions would be 6 150 runs over 2^21 padded keys, each with an
    np.sort of 10^6 keys: minutes.  The steps sit at the power-of-two multiples of 1024 (every merge size of the network) and at n,
    and +-1 around 1024, 2^20 and the last multiple of 1024: 19 positions."""
    last = n // 1024 * 1024
    return sorted({1024 << k for k in range(0, 11)} | {n} | {m + d for m in (1024, 1 << 20, last) for d in (-1, 0, 1)})


def two_valued(n, rng, steps):
    """(name, keys from {0.0, -1.0}).  The comparators of a bitonic network do not look at the data, so a network that sorts every
    two-valued input sorts every input (0-1 principle); these patterns aim at the padding, the block edges and the direction bit
    (gi & k)."""
    i = np.arange(n)
    for d in (0.01, 0.5, 0.99):
        yield "density_%g" % d, -(rng.random(n) < d).astype(np.float64)
    for m in steps:
        yield "step_up_%d" % m, -(i < m).astype(np.float64)      # -1 ... -1 0 ... 0: every key has to move
        yield "step_down_%d" % m, -(i >= m).astype(np.float64)   # already in place
    yield "alternating", -(i & 1).astype(np.float64)
    for period in (2048, 4096):
        yield "sawtooth_%d" % period, -((i % period) < period // 2).astype(np.float64)
        yield "sawtooth_%d_inverted" % period, -((i % period) >= period // 2).astype(np.float64)


def sort_inputs(n, seed=0, steps=None):
    """(name, keys) one after the other; all keys <= 0 and none NaN: what vlr_fdr_threshold accepts."""
    rng = np.random.default_rng([n, seed])
    x = -rng.exponential(3.0, n)
    yield "random", x
    yield "descending", np.sort(x)[::-1].copy()
    yield "ascending", np.sort(x)
    yield "all_equal", np.full(n, -0.25)
    y = x.copy()
    y[rng.random(n) < 0.3] = -np.inf
    y[rng.integers(0, n)] = -np.inf
    yield "with_neg_inf", y
    yield "all_neg_inf", np.full(n, -np.inf)
    yield from two_valued(n, rng, step_positions(n) if steps is None else steps)


# ------------------------------------------------------------------------------------------------ PEPs
# The allowance of the device in ulp of the exact value: the distance of the host's libm evaluation of the same two-branch formula
# from the exact value, plus two library calls per value at 2 ulp each (what tests/test_detmath.py gives an exponential against
# libm).  The host figure was 1.39 when the bound was set and is 1.48 on pep_inputs() (test_fdr_cases_host.py measures it, at
# p = -0.69304 next to the branch point); the bound keeps the smaller figure, so it is a chosen bound, tighter than the rule allows.
PEP_ULP = 1.39 + 4.0

BRANCH = -0.693
MP_BITS = 256


def pep_inputs(seed=11):
    """At most 20 000 ln probabilities for the `smart` conversion: the whole f64 range of magnitudes, both sides of the branch point
    of ln_one_minus_exp, ordinary values, and the edge values (exp underflows below -745.13)."""
    rng = np.random.default_rng(seed)
    parts = [-10.0 ** rng.uniform(-300.0, 2.87, 4000), np.linspace(-0.70, -0.68, 3000), -rng.uniform(0.0, 5.0, 4000),
             np.array([BRANCH, np.nextafter(BRANCH, -np.inf), -745.2, -800.0, -0.0, 0.0, -np.inf])]
    p = np.concatenate(parts)
    assert len(p) <= 20000
    return p


def ln_one_minus_exp_host(p):
    """The formula of the kernel (bio LogProb::ln_one_minus_exp) with the host's libm, vectorised."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return np.where(p < BRANCH, np.log1p(-np.exp(p)), np.log(-np.expm1(p)))


def ln_one_minus_exp_mp(p):
    """ln(1 - e^p) of the f64 p as an mpmath number.  Evaluated branch-wise, log1p(-e^p) below -1 and log(-expm1(p)) above, so that no
    1 - e^p is formed: for p ~ -270 that difference needs more than 400 bits, or the reference itself is wrong by 10^12 ulp.
    test_fdr_cases_host.py holds this against the plain expression at 1200 bits."""
    import mpmath
    with mpmath.workprec(MP_BITS):
        x = mpmath.mpf(float(p))
        if x == 0:
            return mpmath.mpf("-inf")
        if x == mpmath.mpf("-inf"):
            return mpmath.mpf(0)
        return +(mpmath.log1p(-mpmath.exp(x)) if x < -1 else mpmath.log(-mpmath.expm1(x)))


def ulp_errors(got, inputs):
    """|got - ln(1 - e^input)| in ulp of the exact value, per element; an exact value of -inf or 0 is compared by class (and sign of
    the infinity) and reported as 0 ulp or inf."""
    import mpmath
    out = np.zeros(len(inputs))
    with mpmath.workprec(MP_BITS):
        for k, (g, p) in enumerate(zip(got, inputs)):
            ref = _mp_cached(float(p))
            if ref == mpmath.mpf("-inf"):
                out[k] = 0.0 if g == -np.inf else np.inf
            elif ref == 0:
                out[k] = 0.0 if g == 0.0 else np.inf
            elif not np.isfinite(g):
                out[k] = np.inf
            else:
                out[k] = float(abs(mpmath.mpf(float(g)) - ref) / mpmath.mpf(float(np.spacing(abs(float(ref))))))
    return out


@functools.lru_cache(maxsize=None)
def _mp_cached(p):
    return ln_one_minus_exp_mp(p)


# ------------------------------------------------------------------------------------------------ scan
def scan_additions(n):
    """A: the largest number of f64 additions a term passes through on its way into cum[i] + offset[i // 1024], counted in
    csrc/vlr_fdr.hip.  fdr_pep_scan: 6 shuffle steps of the wave scan, at most 15 `off += wsum[w]` over the earlier waves' totals,
    1 `v += off` = 22 into the block total.  fdr_scan_blocks over the totals: the same 6 + 15 + 1 = 22 (its `off` starts from the
    carry); a total that went into the carry passes through 15 + 1 more in every later chunk of 1024 totals.  fdr_search: 1."""
    chunks = -(-(-(-n // SCAN_BLOCK)) // 1024)
    return 22 + 22 + 16 * (chunks - 1) + 1


def scan_bound(n):
    """Relative error of a sum of non-negative terms each of which is off by at most PEP_ULP ulp (2 * 2^-53 relative each) and passes
    through at most A roundings."""
    return (scan_additions(n) + 2.0 * PEP_ULP) * 2.0 ** -53


def scan_indices(n, seed=5):
    """64 indices: the block edges the kernels have, the end, and random ones."""
    fixed = [0, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, n - 1]
    if n <= 8192:
        fixed += list(range(0, n, 1024))
    idx = sorted({i for i in fixed if 0 <= i < n})
    rng = np.random.default_rng([n, seed])
    while len(idx) < min(64, n):
        idx = sorted(set(idx) | {int(rng.integers(0, n))})
    return idx


def scan_reference(prob, indices):
    """math.fsum of the linear PEPs 1 - e^prob up to each index (exactly rounded sums of the host's terms)."""
    term = -np.expm1(np.asarray(prob, dtype=np.float64))
    return [math.fsum(term[:i + 1]) for i in indices]


def running_sums(st):
    """The quantity fdr_search forms: cum[i] + offset[i // 1024], one IEEE addition."""
    return st["cum"] + st["block_offset"][np.arange(len(st["cum"])) // SCAN_BLOCK]


def beta_list(n, seed=4):
    """The lists of tests/test_fdr.py: ln of beta(6, 1) draws, 5 % certain calls; rounded to two decimals (ties) at n = 4097."""
    rng = np.random.default_rng([n, seed])
    p = np.log(rng.beta(6.0, 1.0, n))
    p[rng.random(n) < 0.05] = 0.0
    if n == 4097:
        p = np.round(p, 2)
    return rng.permutation(p)


BETA_SIZES = (1025, 4097, 65537)


def ln_fdr(desc):
    """ln expected FDR per entry of a descending list, as the restatement forms it (numpy, f64)."""
    desc = np.asarray(desc, dtype=np.float64)
    pep = -np.expm1(desc)
    with np.errstate(divide="ignore"):
        return np.minimum(np.log(np.cumsum(pep)) - np.log(np.arange(1, len(desc) + 1)), 0.0)


def beta_case(n):
    """(keys in random order, alpha_ln): alpha half way (in ln) between the expected FDRs of the entries n // 2 and n // 2 + 1."""
    p = beta_list(n)
    f = ln_fdr(np.sort(p)[::-1])
    k = n // 2
    return p, float(0.5 * (f[k] + f[k + 1]))


def dynamic_range_list():
    """1024 x PEP 1e-22, 1000 x 1e-18, 100 x 0.5 as p = log1p(-PEP), already descending: the total of scan block 1 (about 12) is more
    than 2^53 times the sum of block 0 (1.024e-19), so an exclusive offset formed as `off + v - x` loses `off` altogether."""
    pep = np.concatenate([np.full(1024, 1e-22), np.full(1000, 1e-18), np.full(100, 0.5)])
    return np.log1p(-pep)


# the order of the kernels, restated in numpy for the host test (what the subtraction loses, and that a shifted scan does not)
def _wave_scan(v):
    """Inclusive Hillis-Steele scan over rows of 64 (the shuffle loop of both scan kernels)."""
    v = v.copy()
    o = 1
    while o < 64:
        u = v.copy()
        v[:, o:] = u[:, o:] + u[:, :-o]
        o <<= 1
    return v


def _block_scan(x, carry=0.0):
    """One workgroup of 1024: (inclusive values, per-thread `off`)."""
    v = _wave_scan(x.reshape(16, 64))
    off = np.empty(16)
    acc = carry
    for w in range(16):
        off[w] = acc
        acc = acc + v[w, 63]
    return v, off


def emulate_device_scan(term, exclusive):
    """(cum, block offsets) in the kernels' order.  exclusive = "subtract": `off + v - x`; "shift": `off + (inclusive value of the
    lane before, 0 in lane 0)`."""
    n = len(term)
    nb = -(-n // SCAN_BLOCK)
    t = np.zeros(nb * SCAN_BLOCK)
    t[:n] = term
    cum = np.empty_like(t)
    totals = np.zeros(-(-nb // 1024) * 1024)
    for b in range(nb):
        v, off = _block_scan(t[b * 1024:(b + 1) * 1024])
        c = v + off[:, None]
        cum[b * 1024:(b + 1) * 1024] = c.ravel()
        totals[b] = c[15, 63]
    offs = np.empty_like(totals)
    carry = 0.0
    for c0 in range(0, len(totals), 1024):
        x = totals[c0:c0 + 1024]
        v, off = _block_scan(x, carry)
        if exclusive == "subtract":
            e = (off[:, None] + v) - x.reshape(16, 64)
        else:
            prev = np.zeros_like(v)
            prev[:, 1:] = v[:, :-1]
            e = off[:, None] + prev
        offs[c0:c0 + 1024] = e.ravel()
        carry = off[15] + v[15, 63]
    return cum[:n], offs[:nb]


# ------------------------------------------------------------------------------------------------ search
def restatement(desc, alpha_ln):
    """(status, index of the boundary entry or -1, threshold) of fdr.fdr_threshold on a descending list.  The entry it names is the
    first of its run of equal PEPs, hence the first with that probability."""
    desc = np.asarray(desc, dtype=np.float64)
    if len(desc) == 0:
        return EMPTY, -1, 0.0
    thr = fdr.fdr_threshold(desc.copy(order="C"), alpha_ln)
    if thr is None:
        return NONE, -1, 0.0
    if thr == 0.0 and float(ln_one_minus_exp_host(desc[:1])[0]) > alpha_ln:
        return LN_ONE, -1, 0.0
    return VALUE, int(np.flatnonzero(desc == thr)[0]), thr


def alpha_margin(desc, alpha_ln):
    """min over all entries of |ln FDR_i - ln alpha|."""
    return float(np.min(np.abs(ln_fdr(desc) - alpha_ln)))


EDGES = (1024, 2048, 1 << 20)


def planted_edge(E, tie):
    """(descending list, alpha_ln): PEPs 0.005 + 0.01 i / E for i <= E, then 64 from 0.9 upward; alpha is the mean of the expected
    FDRs of the entries E and E + 1, so the boundary is entry E — whose block offset, for E = 2^20, the second chunk of
    fdr_scan_blocks made.  tie: PEP[E] = PEP[E - 1] bars entry E and leaves E - 1."""
    pep = np.concatenate([0.005 + 0.01 * np.arange(E + 1) / E, 0.9 + 0.001 * np.arange(64)])
    if tie:
        pep[E] = pep[E - 1]
    desc = np.log1p(-pep)
    c = np.cumsum(pep)
    alpha = 0.5 * (c[E] / (E + 1) + c[E + 1] / (E + 2))
    return desc, math.log(alpha)


def flip_case():
    """(descending list, alpha_ln): 1024 x PEP 0.5e-20, one of 600e-20, 1100 x 0.5; alpha 1e-20.  Entry 1024 has an expected FDR of
    1.085e-20 > alpha; a block offset of 0 for block 1 makes it 0.585e-20 and admits it."""
    pep = np.concatenate([np.full(1024, 0.5e-20), [600e-20], np.full(1100, 0.5)])
    return np.log1p(-pep), math.log(1e-20)


def near_alpha_lists(seed=9):
    """The construction of test_device_threshold_with_expected_fdr_exactly_at_alpha: the running mean of the first k + 1 PEPs is alpha
    to rounding.  Yields (descending list, alpha_ln)."""
    rng = np.random.default_rng(seed)
    for alpha in (0.05, 0.1, 0.25):
        for _ in range(10):
            while True:   # the planted entry stays below the 0.4 the unrelated entries start from, so it is entry k after the sort
                k = int(rng.integers(1, 6))
                peps = rng.uniform(0.2 * alpha, alpha, k)
                peps = np.append(peps, alpha * (k + 1) - peps.sum())
                if peps[-1] < 0.35:
                    break
            peps = np.sort(np.append(peps, rng.uniform(0.4, 0.9, int(rng.integers(0, 4)))))
            yield np.array([math.log1p(-q) for q in peps]), math.log(alpha)
