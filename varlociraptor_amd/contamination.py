"""`estimate contamination` (reference src/estimation/contamination.rs, src/cli.rs:460-497, 1283-1307).

How much a "sample" is contaminated by a "contaminant", from the allele-frequency distributions (FORMAT/AFD lists) of the
de-novo SNVs of the sample: `call_variants` runs the command's embedded scenario with the two plug points
(`calldriver.ContaminationCandidateFilter`, and `ContaminationEstimator` below as the call processor), the estimator keeps the calls
with P(denovo) >= 0.95 and evaluates the posterior of 4 x 101 events (maximum somatic VAF x contamination).  The grid — one
interpolated density per kept observation and event — runs as HIP (`vlr_contamination_posterior`, csrc/vlr_contam.hip;
`device=k`); `device="cpu"` is the float64 numpy restatement of contamination.rs:84-224 that the CPU suite uses and the GPU
suite compares against.  One device: multi-rank runs are out of scope.
"""
from __future__ import annotations

import csv
import json
import math
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import calldriver

N_C = 101                              # contaminations: linspace(0.0, 1.0, 101)
MAX_SOMATIC_VAFS = (0.25, 0.5, 0.75, 1.0)
BLOCK = 128                            # VLR_CONTAM_BLOCK: observations per partial sum (the fixed summation order, include/vlr.h)
_STEP = (1.0 - 0.0) / (N_C - 1)
CONTAMINATIONS = [0.0 + _STEP * i for i in range(N_C)]   # itertools_num::linspace: a + step * i
DENOVO_MIN_PROB = 0.95                 # VariantObservation::new (contamination.rs:59)
AFD_CAPACITY = 256                     # entries per AFD list the calls are evaluated with; a longer list is an error, never truncated

SCENARIO_EVENTS = {"denovo": "sample:]0.0,1.0] & contaminant:0.0", "other": "sample:[0.0,1.0] & contaminant:]0.0,1.0]"}


def scenario():
    """The command's embedded scenario (contamination.rs:440-455): both samples at resolution 0.01 over [0.0,1.0]."""
    from .scenario import Sample, Scenario
    return Scenario({"sample": Sample(resolution=0.01, universe="[0.0,1.0]"), "contaminant": Sample(resolution=0.01, universe="[0.0,1.0]")},
                    dict(SCENARIO_EVENTS))


# ---------------------------------------------------------------------------------------------------- number formatting
def rust_float(x: float) -> str:
    """Rust's `{}` for f64: the shortest decimal that round-trips, never an exponent (`1`, `0`, `0.5700000000000001`, `-0`),
    `NaN`, `inf`, `-inf`."""
    x = float(x)
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    return np.format_float_positional(x, unique=True, trim="-")


def rust_round(x: float) -> float:
    """f64::round: half away from zero (Python's round() is half to even)."""
    a = abs(x)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1.0
    return math.copysign(r, x)


# ---------------------------------------------------------------------------------------------------- prior
def _gsl_lnfact(n: int) -> float:
    # gsl_sf_lnfact: ln of the tabulated n! up to GSL_SF_FACT_NMAX = 170, lngamma(n + 1) above
    return math.log(float(math.factorial(n))) if n <= 170 else math.lgamma(n + 1.0)


def _gsl_lnchoose(n: int, k: int) -> float:
    if k == n or k == 0:
        return 0.0
    if 2 * k > n:
        k = n - k
    return _gsl_lnfact(n) - _gsl_lnfact(k) - _gsl_lnfact(n - k)


def gsl_binomial_pdf(k: int, p: float, n: int) -> float:
    """gsl_ran_binomial_pdf(k, p, n) (randist/binomial.c): exact cases p = 0 and p = 1, exp(lnchoose + k ln p + (n - k) log1p(-p))
    otherwise, 0 for k > n."""
    if k > n:
        return 0.0
    if p == 0.0:
        return 1.0 if k == 0 else 0.0
    if p == 1.0:
        return 1.0 if k == n else 0.0
    return math.exp(_gsl_lnchoose(n, k) + k * math.log(p) + (n - k) * math.log1p(-p))


def ln_prior(prior_estimate: Optional[Tuple[float, int]] = None) -> np.ndarray:
    """Prior::prob (contamination.rs:136-155) at the 101 contaminations: ln of the binomial pdf of k = round(p n) among n cells
    (an underflow becomes -inf), ln 1 without an estimate."""
    out = np.zeros(N_C, np.float64)
    if prior_estimate is None:
        return out
    p, n = float(prior_estimate[0]), int(prior_estimate[1])
    kf = rust_round(p * n)
    k = 0 if not (kf > 0) else int(min(kf, 4294967295.0))   # `as u32` saturates (NaN -> 0)
    for i, c in enumerate(CONTAMINATIONS):
        P = gsl_binomial_pdf(k, c, n)
        out[i] = math.log(P) if P > 0.0 else -math.inf
    return out


# ---------------------------------------------------------------------------------------------------- restatement
def _ln_one_minus_exp(p):
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return np.where(p < -0.693, np.log1p(-np.exp(p)), np.log(-np.expm1(p)))


def _ln_add_exp(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        sw = b > a
        hi, lo = np.where(sw, b, a), np.where(sw, a, b)
        return np.where(hi == -np.inf, hi, hi + np.log1p(np.exp(lo - hi)))


def pdf(vaf: np.ndarray, lnprob: np.ndarray, x) -> np.ndarray:
    """VariantObservation::pdf (contamination.rs:84-117) of ONE list (sorted by VAF, keys unique) at the points x, with the
    falling-segment decision of include/vlr.h (linear interpolation in probability space on every segment)."""
    off = np.array([0, len(vaf)], np.int64)
    x = np.asarray(x, np.float64)
    return _terms(off, np.asarray(vaf, np.float64), np.asarray(lnprob, np.float64), x.reshape(1, -1)).reshape(x.shape)


def _terms(off, lv, lp, x):
    """pdf of list o at x[o, :] for every row o (vectorised lower-bound search over the CSR lists)."""
    R, E = x.shape
    base = off[:-1][:, None]
    n = (off[1:] - off[:-1])[:, None]
    lo = np.zeros((R, E), np.int64)
    ln_ = np.broadcast_to(n, (R, E)).copy()
    top = max(len(lv) - 1, 0)
    while True:
        act = ln_ > 0
        if not act.any():
            break
        half = ln_ >> 1
        key = lv[np.minimum(base + lo + half, top)] if len(lv) else np.zeros((R, E))
        go = act & (key < x)
        lo = np.where(go, lo + half + 1, lo)
        ln_ = np.where(go, ln_ - half - 1, np.where(act, half, ln_))
    ninf = np.full((R, E), -np.inf)
    if not len(lv):
        return ninf
    j = np.minimum(base + lo, top)
    jm = np.maximum(j - 1, 0)
    inside = lo < n
    exact = inside & (lv[j] == x)
    between = inside & (lo > 0) & ~exact
    xa, xb, a, b = lv[jm], lv[j], lp[jm], lp[j]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ea, eb = np.exp(a), np.exp(b)
        ldx = np.log(x - xa)
        rising = _ln_add_exp(a, np.log((eb - ea) / (xb - xa)) + ldx)
        s = np.log((ea - eb) / (xb - xa)) + ldx
        falling = np.where(s >= a, b, a + _ln_one_minus_exp(s - a))
        val = np.where(eb >= ea, rising, falling)
    return np.where(exact, lp[j], np.where(between, val, ninf))


def _event_axes():
    mv = np.repeat(np.array(MAX_SOMATIC_VAFS, np.float64), N_C)
    c = np.tile(np.array(CONTAMINATIONS, np.float64), len(MAX_SOMATIC_VAFS))
    purity = 1.0 - c
    return mv, c, purity, mv * purity


def ln_joint_host(list_offset, list_vaf, list_lnprob, map_vaf, ln_prob_denovo, max_vaf: float, ln_prior_: Sequence[float],
                  chunk_blocks: int = 16) -> np.ndarray:
    """Likelihood + prior of the 404 events (contamination.rs:160-180) in float64 numpy, summed in the kernel's fixed order
    (blocks of BLOCK observations, each sequentially in record order, then the block sums in block order)."""
    off = np.asarray(list_offset, np.int64)
    lv, lp = np.asarray(list_vaf, np.float64), np.asarray(list_lnprob, np.float64)
    mvec, dvec = np.asarray(map_vaf, np.float64), np.asarray(ln_prob_denovo, np.float64)
    n = len(off) - 1
    _, _, purity, mvp = _event_axes()
    zero_purity = purity == 0.0
    total = np.zeros(len(mvp), np.float64)
    step = BLOCK * chunk_blocks
    for o0 in range(0, n, step):
        o1 = min(o0 + step, n)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = mvec[o0:o1] / max_vaf
        x = mvp[None, :] * q[:, None]
        t = _terms(off[o0:o1 + 1], lv, lp, x)
        t[:, zero_purity] = _ln_one_minus_exp(dvec[o0:o1])[:, None]
        nb = (o1 - o0 + BLOCK - 1) // BLOCK
        pad = np.zeros((nb * BLOCK, len(mvp)))
        pad[:o1 - o0] = t    # + 0.0 leaves a partial sum as it is: the padding rows change nothing
        pad = pad.reshape(nb, BLOCK, len(mvp))
        acc = np.zeros((nb, len(mvp)))
        with np.errstate(invalid="ignore"):
            for r in range(BLOCK):
                acc = acc + pad[:, r, :]
            for b in range(nb):
                total = total + acc[b]
    return np.tile(np.asarray(ln_prior_, np.float64), len(MAX_SOMATIC_VAFS)) + total


def ln_sum_exp(v: Sequence[float]) -> float:
    """bio LogProb::ln_sum_exp; NaN in, NaN out."""
    v = [float(x) for x in v]
    if any(x != x for x in v):
        return math.nan
    if not v:
        return -math.inf
    im = max(range(len(v)), key=lambda k: (v[k], -k))
    m = v[im]
    if m == -math.inf:
        return -math.inf
    s = 0.0
    for k, x in enumerate(v):
        if k != im and x != -math.inf:
            s += math.exp(x - m)
    return m + math.log1p(s)


def ln_marginal_host(ln_joint: Sequence[float]) -> float:
    """Marginal::compute (contamination.rs:196-224): ln_simpsons_integrate_exp over the 101 contaminations per maximum somatic VAF
    (terms in the order of the call path's Simpson: interior points, then both ends), ln_sum_exp of the four integrals."""
    lj = np.asarray(ln_joint, np.float64).reshape(len(MAX_SOMATIC_VAFS), N_C)
    integrals = []
    for f in lj:
        terms = [float(f[i]) + math.log(float(2 + (i % 2) * 2)) for i in range(1, N_C - 1)] + [float(f[0]), float(f[N_C - 1])]
        integrals.append(ln_sum_exp(terms) + math.log(1.0 - 0.0) - math.log(float(N_C - 1)) - math.log(3.0))
    return ln_sum_exp(integrals)


def simpson_weights() -> np.ndarray:
    """Simpson weight times h / 3 of each of the 404 events: sum(weight * e^posterior) over all events is 4 x ... = 1 when normalised."""
    w = np.array([1.0] + [2.0 + (i % 2) * 2.0 for i in range(1, N_C - 1)] + [1.0]) * (_STEP / 3.0)
    return np.tile(w, len(MAX_SOMATIC_VAFS))


def posterior_grid(list_offset, list_vaf, list_lnprob, map_vaf, ln_prob_denovo, max_vaf: float, ln_prior_: Sequence[float],
                   device="cpu") -> Tuple[np.ndarray, float]:
    """(ln_joint[404], ln_marginal): `device` "cpu" = the numpy restatement; an int k or "cuda[:k]" = vlr_contamination_posterior
    on device k."""
    if isinstance(device, str) and device == "cpu":
        lj = ln_joint_host(list_offset, list_vaf, list_lnprob, map_vaf, ln_prob_denovo, max_vaf, ln_prior_)
        return lj, ln_marginal_host(lj)
    dev = device if isinstance(device, int) else (int(str(device).split(":")[1]) if ":" in str(device) else 0)
    return posterior_grid_device(list_offset, list_vaf, list_lnprob, map_vaf, ln_prob_denovo, max_vaf, ln_prior_, dev)


def posterior_grid_device(list_offset, list_vaf, list_lnprob, map_vaf, ln_prob_denovo, max_vaf: float, ln_prior_: Sequence[float],
                          device: int = 0) -> Tuple[np.ndarray, float]:
    """vlr_contamination_posterior (include/vlr.h; kernels in csrc/vlr_contam.hip)."""
    import ctypes as C
    from . import engine
    L = engine.lib()
    off = np.ascontiguousarray(list_offset, np.int64)
    lv, lp = np.ascontiguousarray(list_vaf, np.float64), np.ascontiguousarray(list_lnprob, np.float64)
    mv, pd = np.ascontiguousarray(map_vaf, np.float64), np.ascontiguousarray(ln_prob_denovo, np.float64)
    pr = np.ascontiguousarray(ln_prior_, np.float64)
    n = len(off) - 1
    if n < 0 or len(mv) != n or len(pd) != n or len(pr) != N_C or len(lv) != len(lp) or (n >= 0 and int(off[-1]) > len(lv)):
        raise ValueError("inconsistent contamination inputs")
    out = np.zeros(len(MAX_SOMATIC_VAFS) * N_C, np.float64)
    marg = C.c_double()
    engine.check(L.vlr_contamination_posterior(int(device), n, off.ctypes.data, lv.ctypes.data, lp.ctypes.data, mv.ctypes.data, pd.ctypes.data,
                                               float(max_vaf), pr.ctypes.data, out.ctypes.data, C.byref(marg)))
    return out, float(marg.value)


# ---------------------------------------------------------------------------------------------------- the call processor
class ContaminationEstimator(calldriver.CallProcessor):
    """ContaminationEstimator (contamination.rs:260-399): keeps, per call, the sample's AFD list (sorted by VAF, CSR), its MAP VAF,
    ln P(denovo), chrom and 0-based position when the MAP is not an artifact and P(denovo) >= 0.95; `finalize` evaluates the grid
    and writes the outputs."""

    def __init__(self, output: Optional[str] = None, output_plot: Optional[str] = None, output_max_vaf_variants: Optional[str] = None,
                 prior_estimate: Optional[Tuple[float, int]] = None, device=0, out=None):
        self.output, self.output_plot, self.output_max_vaf_variants = output, output_plot, output_max_vaf_variants
        self.prior_estimate, self.device, self.out = prior_estimate, device, out
        self._vaf: List[np.ndarray] = []
        self._lp: List[np.ndarray] = []
        self._len: List[np.ndarray] = []
        self._map: List[np.ndarray] = []
        self._den: List[np.ndarray] = []
        self.chrom: List[str] = []
        self.pos: List[int] = []
        self.k_denovo = self.s_sample = None

    def setup(self, out_names, sample_names):
        self.k_denovo = list(out_names).index("denovo")
        self.s_sample = list(sample_names).index("sample")

    def process_calls(self, chunk: "calldriver.CallChunk"):
        res, s = chunk.results, self.s_sample
        pd = np.asarray(res.ln_posterior[:, self.k_denovo], np.float64)
        mv = np.asarray(res.map_vaf[:, s], np.float64)
        with np.errstate(invalid="ignore"):
            # vaf_dist present = the MAP is not an artifact (calling.rs:889-925): no bias in the MAP, a MAP VAF
            keep = (np.asarray(res.map_bias) == 0).all(axis=1) & ~np.isnan(mv) & (np.exp(pd) >= DENOVO_MIN_PROB)
        idx = np.nonzero(keep)[0]
        if not len(idx):
            return
        cnt = np.asarray(res.afd_count[idx, s], np.int64)
        if (cnt > res.afd_capacity).any():
            l = int(idx[np.argmax(cnt > res.afd_capacity)])
            raise RuntimeError("AFD list of record %d holds %d entries, more than the capacity of %d: refusing a truncated list"
                               % (chunk.offset + int(chunk.loci[l]), int(res.afd_count[l, s]), res.afd_capacity))
        for j, l in enumerate(idx):
            v = np.array(res.afd_vaf[l, s, :cnt[j]], np.float64)
            p = np.array(res.afd_lnprob[l, s, :cnt[j]], np.float64)
            order = np.argsort(v, kind="stable")
            v, p = v[order], p[order]
            last = np.ones(len(v), bool)       # a repeated key keeps its last value (BTreeMap::collect)
            last[:-1] = v[1:] != v[:-1]
            self._vaf.append(v[last])
            self._lp.append(p[last])
            self._len.append(np.array([int(last.sum())], np.int64))
            rec = int(chunk.loci[l])
            self.chrom.append(chunk.sites.chrom(rec))
            self.pos.append(int(chunk.sites.pos[rec]) - 1)   # Call.pos = first_record.pos(): 0-based
        self._map.append(mv[idx])
        self._den.append(pd[idx])

    # the kept observations as arrays
    def observations(self):
        lens = np.concatenate(self._len) if self._len else np.zeros(0, np.int64)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        lv = np.concatenate(self._vaf) if self._vaf else np.zeros(0)
        lp = np.concatenate(self._lp) if self._lp else np.zeros(0)
        mv = np.concatenate(self._map) if self._map else np.zeros(0)
        pd = np.concatenate(self._den) if self._den else np.zeros(0)
        return off, lv, lp, mv, pd

    def finalize(self):
        off, lv, lp, mv, pd = self.observations()
        self.max_vaf = float(max(mv.max(), 0.0)) if len(mv) else 0.0          # VAFDist::new: starts at AlleleFreq(0.0)
        self.ln_prior = ln_prior(self.prior_estimate)
        self.ln_joint, self.ln_marginal = posterior_grid(off, lv, lp, mv, pd, self.max_vaf, self.ln_prior, device=self.device)
        rows = posterior_rows(self.ln_joint, self.ln_marginal)
        self.rows = rows
        if self.output_plot:
            with open(self.output_plot, "w") as fh:
                json.dump(plot_spec(mv, self.ln_prior, rows), fh, indent=2)
                fh.write("\n")
        if self.output_max_vaf_variants:
            with open(self.output_max_vaf_variants, "w", newline="") as fh:
                w = csv.writer(fh, lineterminator="\n")
                w.writerow(["chrom", "pos"])
                for k in range(len(mv)):
                    if mv[k] == self.max_vaf:
                        w.writerow([self.chrom[k], str(self.pos[k])])
        fh = open(self.output, "w", newline="") if self.output else (self.out or sys.stdout)
        try:
            fh.write(format_table(rows))
        finally:
            if self.output:
                fh.close()


def posterior_rows(ln_joint, ln_marginal: float):
    """ModelInstance::event_posteriors: (mv, c, ln posterior) of the 404 events, posterior descending; ties (left unordered by the
    reference) by (mv, c) ascending, NaN last."""
    mvs, cs, _, _ = _event_axes()
    post = np.asarray(ln_joint, np.float64) - ln_marginal
    rows = [(float(mvs[e]), float(cs[e]), float(post[e])) for e in range(len(post))]
    rows.sort(key=lambda r: (r[2] != r[2], -r[2] if r[2] == r[2] else 0.0, r[0], r[1]))
    return rows


def format_table(rows) -> str:
    lines = ["maximum somatic VAF\tcontamination\tposterior density"]
    lines += ["%s\t%s\t%s" % (rust_float(mv), rust_float(c), rust_float(math.exp(p))) for mv, c, p in rows]
    return "\n".join(lines) + "\n"


def _json_num(x: float):
    return float(x) if math.isfinite(x) else None   # serde_json writes a non-finite f64 as null


def plot_spec(map_vaf, ln_prior_, rows) -> dict:
    """A vega-lite spec of our own with the reference's two datasets: `empirical_vaf_dist` ({vaf, count} per floor(100 vaf) / 100
    bin, VAFDist::hist_as_json) and `densities` (Prior::as_json's 101 rows, then one row per event in the order of the table)."""
    bins = {}
    for v in np.asarray(map_vaf, np.float64):
        b = math.floor(float(v) * 100.0) / 100.0
        bins[b] = bins.get(b, 0) + 1
    hist = [{"vaf": b, "count": bins[b]} for b in sorted(bins)]
    dens = [{"purity": 1.0 - c, "density": _json_num(math.exp(p)), "category": "prior"} for c, p in zip(CONTAMINATIONS, ln_prior_)]
    dens += [{"purity": 1.0 - c, "density": _json_num(math.exp(p)), "category": "posterior, max VAF=%s" % rust_float(mv)} for mv, c, p in rows]
    return {
        "$schema": "https://vega.github.io/schema/vega-lite/v5.json",
        "description": "contamination estimate: empirical VAF distribution of the de-novo SNVs, prior and posterior densities of purity",
        "datasets": {"empirical_vaf_dist": hist, "densities": dens},
        "vconcat": [
            {"data": {"name": "empirical_vaf_dist"}, "mark": "bar", "title": "MAP VAF of the kept observations",
             "encoding": {"x": {"field": "vaf", "type": "quantitative", "title": "VAF"}, "y": {"field": "count", "type": "quantitative"}}},
            {"data": {"name": "densities"}, "mark": {"type": "line", "point": False}, "title": "purity",
             "encoding": {"x": {"field": "purity", "type": "quantitative"}, "y": {"field": "density", "type": "quantitative"},
                          "color": {"field": "category", "type": "nominal"}}},
        ],
    }


def estimate_contamination(sample: str, contaminant: str, output: Optional[str] = None, output_plot: Optional[str] = None,
                           output_max_vaf_variants: Optional[str] = None, prior_estimate: Optional[Tuple[float, int]] = None,
                           device=0, out=None) -> ContaminationEstimator:
    """estimate_contamination (contamination.rs:430-473): no bias omitted, no full prior, samples ordered by name."""
    est = ContaminationEstimator(output, output_plot, output_max_vaf_variants, prior_estimate, device=device, out=out)
    calldriver.call_variants(scenario(), {"sample": sample, "contaminant": contaminant}, afd_capacity=AFD_CAPACITY, device=device if isinstance(device, int) else 0,
                             processor=est, candidate_filter=calldriver.ContaminationCandidateFilter())
    return est
