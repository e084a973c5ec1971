"""`estimate contamination` on the GPU: the posterior grid of vlr_contamination_posterior (csrc/vlr_contam.hip) against the numpy
restatement (contamination.py), its determinism, the command end to end, and the model on lists built around a known contamination."""
import csv
import io
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from varlociraptor_amd import cli, contamination as ct

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = 120


def _inputs(n, seed, max_len=CAPACITY, exact_hits=True, nan_list=False, ragged=True):
    """Random CSR lists of 0..max_len entries (sorted, unique keys) over [0, 1]; some lists hold the expected VAFs of a few events
    as keys, some observations have P(denovo) = 1.  ragged=False: every list spans [0, 1] (finite likelihoods); otherwise
    short and empty lists too (which put most events at -inf)."""
    rng = np.random.default_rng(seed)
    map_vaf = rng.uniform(0.02, 0.95, n)
    max_vaf = float(map_vaf.max()) if n else 0.0
    pd = np.log(rng.uniform(0.95, 1.0, n))
    if n:
        pd[rng.integers(0, n, max(1, n // 50))] = 0.0
    _, _, _, mvp = ct._event_axes()
    vaf, lp = [], []
    for o in range(n):
        k = int(rng.integers(0 if ragged else 2, max_len + 1))
        keys = set(np.round(rng.uniform(0.0, 1.0, k), 3).tolist())
        if exact_hits and o % 3 == 0 and k:
            for e in rng.integers(0, 404, 4):
                keys.add(float(mvp[e] * (map_vaf[o] / max_vaf)))     # the kernel's expected VAF, bit for bit
        v = np.array(sorted(keys - {0.0, 1.0}))[:max(k - 2, 0)]
        if not ragged or k > 4:
            v = np.concatenate([[0.0], v, [1.0]])
        vaf.append(v)
        lp.append(rng.normal(-2.0, 1.5, len(v)))
    if nan_list and n > 3:
        lp[3][len(lp[3]) // 2] = math.nan
    off = np.concatenate([[0], np.cumsum([len(v) for v in vaf])]).astype(np.int64)
    cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0)
    return off, cat(vaf), cat(lp), map_vaf, pd, max_vaf


def _abs_term_sums(off, lv, lp, mv, pd, max_vaf):
    _, _, purity, mvp = ct._event_axes()
    tot = np.zeros(404)
    for o0 in range(0, len(mv), 4096):
        o1 = min(o0 + 4096, len(mv))
        with np.errstate(invalid="ignore", divide="ignore"):
            t = ct._terms(off[o0:o1 + 1], lv, lp, mvp[None, :] * (mv[o0:o1] / max_vaf)[:, None])
        t[:, purity == 0.0] = ct._ln_one_minus_exp(pd[o0:o1])[:, None]
        with np.errstate(invalid="ignore"):
            tot += np.where(np.isfinite(t), np.abs(t), 0.0).sum(axis=0)
    return tot


def _same_grid(got, want, bound):
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isneginf(got), np.isneginf(want))
    assert np.array_equal(np.isposinf(got), np.isposinf(want))
    fin = np.isfinite(want)
    d = np.abs(got[fin] - want[fin])
    assert np.all(d <= 1e-12 * np.maximum(1.0, bound[fin])), d.max()


@pytest.mark.parametrize("n,ragged", [(0, True), (1, True), (63, True), (64, True), (65, True), (1000, True),
                                      (1, False), (63, False), (64, False), (65, False), (1000, False), (100003, False)])
def test_kernel_matches_the_restatement(n, ragged):
    off, lv, lp, mv, pd, max_vaf = _inputs(n, seed=n + 1, max_len=CAPACITY if n < 100000 else 24, nan_list=(n == 1000), ragged=ragged)
    for prior in (None, (0.2, 40)):
        pr = ct.ln_prior(prior)
        got, gm = ct.posterior_grid(off, lv, lp, mv, pd, max_vaf, pr, device=0)
        want, wm = ct.posterior_grid(off, lv, lp, mv, pd, max_vaf, pr, device="cpu")
        bound = _abs_term_sums(off, lv, lp, mv, pd, max_vaf)
        _same_grid(got, want, bound)
        if n == 0:
            assert np.array_equal(got, np.tile(pr, 4))
        if prior is None and not ragged and n != 1000:
            assert np.isfinite(got.reshape(4, 101)[:, :100]).all()   # lists spanning [0, 1]: finite likelihoods below c = 1
        if math.isnan(wm) or math.isinf(wm):
            assert (math.isnan(gm) and math.isnan(wm)) or gm == wm
        else:
            assert abs(gm - wm) <= 1e-12 * max(1.0, bound.max())
    if n == 1000:
        assert np.isnan(got).any()          # a NaN in a list reaches the events that interpolate on it
    if n >= 63:
        assert np.all(got.reshape(4, 101)[:, 100] == -math.inf)   # P(denovo) = 1 somewhere: no contamination of 1


def test_kernel_is_deterministic():
    off, lv, lp, mv, pd, max_vaf = _inputs(20011, seed=9, max_len=60)
    pr = ct.ln_prior((0.1, 200))
    a, am = ct.posterior_grid(off, lv, lp, mv, pd, max_vaf, pr, device=0)
    b, bm = ct.posterior_grid(off, lv, lp, mv, pd, max_vaf, pr, device=0)
    assert a.tobytes() == b.tobytes() and np.float64(am).tobytes() == np.float64(bm).tobytes()


def test_kernel_refuses_unsorted_lists():
    from varlociraptor_amd import engine
    off = np.array([0, 3], np.int64)
    with pytest.raises(engine.EngineError):
        ct.posterior_grid(off, np.array([0.1, 0.3, 0.2]), np.zeros(3), np.array([0.5]), np.array([0.0]), 0.5, np.zeros(101), device=0)


def test_model_finds_a_known_contamination():
    """Lists whose density peaks at 1 * (1 - c_true) * q_o: among the rows of maximum somatic VAF 1 the posterior mode is c_true
    (across maximum somatic VAFs the model is not identifiable: mv = 0.75 at c = 0.067 explains the same VAFs)."""
    rng = np.random.default_rng(11)
    n, c_true = 200, 0.3
    q = rng.uniform(0.1, 0.9, n)
    mx = float(q.max())
    keys = np.arange(101) / 100.0
    lv = np.tile(keys, n)
    lp = np.concatenate([-((keys - 1.0 * (1.0 - c_true) * q_ / mx) ** 2) / (2 * 0.03 ** 2) for q_ in q])
    off = (np.arange(n + 1) * 101).astype(np.int64)
    pd = np.full(n, math.log(0.99))
    for dev in (0, "cpu"):
        lj, m = ct.posterior_grid(off, lv, lp, q, pd, mx, ct.ln_prior(None), device=dev)
        mode = ct.CONTAMINATIONS[int(np.argmax((lj - m)[3 * 101:]))]
        assert abs(mode - c_true) <= 0.01 + 1e-12, (dev, mode)


# ---------------------------------------------------------------------------------------------------- the command
def _observations(tmp_path):
    """Synthetic tumor-normal pileups as in the plug-point test: the normal written as `contaminant`, the tumor as `sample`."""
    from varlociraptor_amd import ingest, synth
    sc = ct.scenario()
    cfg = synth.config3()
    cfg.depth = 40.0
    batch = synth.generate(cfg, 600, seed=41)
    paths = {}
    for s_, name in enumerate(sc.sample_names):     # contaminant = 0 (the normal), sample = 1 (the tumor)
        paths[name] = str(tmp_path / ("%s.bcf" % name))
        ingest.write_observations(paths[name], batch, s_)
    return paths


def _run(paths, out_dir, chunk=None, extra=()):
    env = dict(os.environ)
    env.pop("VLR_CLI_CHUNK", None)
    if chunk:
        env["VLR_CLI_CHUNK"] = str(chunk)
    os.makedirs(out_dir, exist_ok=True)
    files = {k: os.path.join(out_dir, k) for k in ("t.tsv", "p.json", "v.csv")}
    cmd = [sys.executable, "-m", "varlociraptor_amd", "estimate", "contamination", "--sample", paths["sample"], "--contaminant", paths["contaminant"],
           "--output", files["t.tsv"], "--output-plot", files["p.json"], "--output-max-vaf-variants", files["v.csv"]] + list(extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return {k: open(v).read() for k, v in files.items()}


def test_cli_end_to_end(tmp_path):
    paths = _observations(tmp_path)
    got = _run(paths, str(tmp_path / "a"))
    # what the plug point hands a collecting processor, evaluated by the restatement
    ref = ct.ContaminationEstimator(device="cpu", out=io.StringIO())
    cli.call_variants(ct.scenario(), paths, afd_capacity=ct.AFD_CAPACITY, processor=ref, candidate_filter=cli.ContaminationCandidateFilter())
    off, lv, lp, mv, pd = ref.observations()
    assert len(mv) >= 20, len(mv)
    assert np.all(np.exp(pd) >= 0.95)
    assert all(np.all(np.diff(lv[off[o]:off[o + 1]]) > 0) for o in range(len(mv)))

    lines = got["t.tsv"].split("\n")
    assert lines[0] == "maximum somatic VAF\tcontamination\tposterior density" and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    assert len(rows) == 404
    dens = np.array([float(r[2]) for r in rows])
    key = [(float(r[0]), float(r[1])) for r in rows]
    assert len(set(key)) == 404
    assert np.all(np.diff(dens) <= 0)      # (the tie order, by (mv, c), is tested on the host: equal densities may hide unequal ln)
    want = {(mv_, c_): math.exp(p_) for mv_, c_, p_ in ref.rows}
    for (k_, d_) in zip(key, dens):
        # relative agreement where the density is a normal number; below that both sides are at the underflow
        assert d_ == pytest.approx(want[k_], rel=1e-8, abs=1e-290), k_
    for r in rows:
        assert r[0] in ("0.25", "0.5", "0.75", "1") and r[1] == ct.rust_float(float(r[1]))

    # the observations at the maximum MAP VAF, 0-based positions, in record order
    max_vaf = float(mv.max())
    want_v = [[ref.chrom[k], str(ref.pos[k])] for k in range(len(mv)) if mv[k] == max_vaf]
    got_v = list(csv.reader(io.StringIO(got["v.csv"])))
    assert got_v[0] == ["chrom", "pos"] and got_v[1:] == want_v and len(want_v) >= 1

    # the plot's two datasets
    spec = json.loads(got["p.json"])
    hist = spec["datasets"]["empirical_vaf_dist"]
    bins = {}
    for v in mv:
        b = math.floor(v * 100.0) / 100.0
        bins[b] = bins.get(b, 0) + 1
    assert [(h["vaf"], h["count"]) for h in hist] == sorted(bins.items())
    d = spec["datasets"]["densities"]
    assert len(d) == 101 + 404
    assert [x["category"] for x in d[:101]] == ["prior"] * 101 and [x["purity"] for x in d[:101]] == [1.0 - c for c in ct.CONTAMINATIONS]
    assert all(x["density"] == 1.0 for x in d[:101])
    post = d[101:]
    assert [x["category"] for x in post] == ["posterior, max VAF=%s" % r[0] for r in rows]
    for x, (mv_, c_), dd in zip(post, key, dens):
        assert x["purity"] == 1.0 - c_ and x["density"] == pytest.approx(dd, rel=1e-15, abs=0.0)


def test_cli_output_does_not_depend_on_the_chunking(tmp_path):
    paths = _observations(tmp_path)
    a = _run(paths, str(tmp_path / "a"), extra=("--prior-estimate", "0.25", "--prior-considered-cells", "30"))
    b = _run(paths, str(tmp_path / "b"), chunk=97, extra=("--prior-estimate", "0.25", "--prior-considered-cells", "30"))
    assert a["t.tsv"] == b["t.tsv"] and a["v.csv"] == b["v.csv"] and a["p.json"] == b["p.json"]
    spec = json.loads(a["p.json"])
    prior = [x["density"] for x in spec["datasets"]["densities"][:101]]
    assert prior == [math.exp(p) for p in ct.ln_prior((0.25, 30))]
