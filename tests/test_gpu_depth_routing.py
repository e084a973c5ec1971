"""Which kernel evaluates a locus at batch scale.  A locus is evaluated by the LDS-resident call kernel, or flagged
VLR_LOCUS_TOO_DEEP by it and re-evaluated by the deep launch from the plan's HBM pool, or it comes back flagged.  The choice is made
by the LDS budget of the batch (fit_budget in vlr_host.cpp: the deepest locus, or the 16-workgroup budget `m16` when at most 0.5 % of
a batch of >= 100 000 loci exceed it), by the size of the deep pool (VLR_DEEP_POOL_MB) and by the pool's bump allocator in the kernel.

Batch A: 100 000 tumor-normal loci at 20x with 300 loci at 400x per sample shuffled in (0.3 % of the batch): every entry point with
the 16-workgroup budget, with and without AFD lists, and without a deep pool.  Batch B: nearly every locus above the budget and a pool
that holds a few hundred of them, so that each deep pass runs short."""
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

from varlociraptor_amd import abi, engine, synth
from varlociraptor_amd.batch import CallResults, PileupBatch

from parity import compare, describe

pytestmark = pytest.mark.gpu

AFD_CAP = 64
RESULT_FIELDS = ("ln_posterior", "ln_marginal", "map_vaf", "map_bias", "best_event", "status")
N_STATUS_BITS = 7   # VLR_LOCUS_* bits of include/vlr.h: anything above is internal to the kernels and must never come back


def oracle_mt(oracle, scenario, batch, afd_capacity=0, threads=8):
    """The oracle on every locus of `batch`, in slices over threads (with the AFD lists when afd_capacity > 0)."""
    n = batch.n_loci
    bounds = np.linspace(0, n, min(threads, max(1, n)) + 1).astype(int)
    oracle.lib()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        parts = list(ex.map(lambda i: oracle.call(scenario, batch, afd_capacity=afd_capacity, begin=int(bounds[i]), end=int(bounds[i + 1]),
                                                  want_events=True), range(len(bounds) - 1)))
    ref = CallResults(n, scenario.n_out, batch.n_samples, afd_capacity)
    ref.event_ln_posterior = np.full((n, 1 + 2 * len(scenario.event_names)), np.nan)
    fields = RESULT_FIELDS + (("afd_count", "afd_vaf", "afd_lnprob") if afd_capacity else ())
    for i, p in enumerate(parts):
        lo, hi = int(bounds[i]), int(bounds[i + 1])
        for f in fields:
            getattr(ref, f)[lo:hi] = getattr(p, f)[lo:hi]
        ref.event_ln_posterior[lo:hi] = p.event_ln_posterior
    return ref


def take(res, idx):
    """The loci `idx` of a result (the fields compare() and the AFD checks read)."""
    out = SimpleNamespace(afd_capacity=getattr(res, "afd_capacity", 0))
    for f in RESULT_FIELDS + ("afd_count", "afd_vaf", "afd_lnprob"):
        a = getattr(res, f, None)
        setattr(out, f, None if a is None else np.asarray(a)[idx])
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def identical(got, ref, idx=None):
    """Bit-identical results (NaN equals NaN whatever its payload); the names of the fields that differ."""
    bad = []
    for f in RESULT_FIELDS:
        g, r = np.asarray(getattr(got, f)), np.asarray(getattr(ref, f))
        if idx is not None:
            g, r = g[idx], r[idx]
        same = bits(g) == bits(r)
        if g.dtype == np.float64:
            same |= np.isnan(g) & np.isnan(r)
        if not same.all():
            bad.append("%s (%d loci)" % (f, int((~same.reshape(len(g), -1).all(axis=1)).sum())))
    return bad


def internal_bits(res):
    return (np.asarray(res.status).astype(np.uint32) >> N_STATUS_BITS) != 0


def too_deep(res):
    return (np.asarray(res.status) & abi.LOCUS_TOO_DEEP) != 0


def check_oracle(got, ref, label):
    m = compare(got, ref, label=label)
    print(describe(m))
    assert m["frac_within"] == 1.0 and m["bias_equal"] and m["status_equal"], describe(m)


def check_afd(got, ref, label):
    """AFD counts, and the sorted lists where they fit the capacity, equal the oracle's (loci whose MAP event is an exact tie of
    posteriors, which compare() allows, are skipped: their lists follow the chosen event)."""
    n_entries = 0
    for l in range(len(ref.status)):
        if got.best_event[l] != ref.best_event[l]:
            continue
        for s in range(ref.afd_count.shape[1]):
            k = int(ref.afd_count[l, s])
            assert got.afd_count[l, s] == k, (label, l, s, int(got.afd_count[l, s]), k)
            if k <= AFD_CAP:
                assert np.array_equal(np.sort(got.afd_vaf[l, s, :k]), np.sort(ref.afd_vaf[l, s, :k])), (label, l, s)
                n_entries += k
    return n_entries


# ---------------------------------------------------------------------------------------------------------------- batch A

@pytest.fixture(scope="module")
def batch_a():
    cfg = synth.config3()
    cfg.depth = 20.0
    shallow = synth.generate(cfg, 100_000, seed=301)
    cfg_deep = synth.config3()
    cfg_deep.depth, cfg_deep.max_depth = 400.0, 1000
    deep = synth.generate(cfg_deep, 300, seed=302)
    both = PileupBatch.concat([shallow, deep])
    # shuffled: the deep loci land in every host chunk and every AFD sub-range, not in one of them
    perm = np.random.default_rng(303).permutation(both.n_loci)
    b = both.select(perm)
    depth = b.depth().sum(axis=1)
    deep_idx = np.nonzero(perm >= shallow.n_loci)[0]
    shallow_idx = np.nonzero(perm < shallow.n_loci)[0]
    assert depth[shallow_idx].max() < depth[deep_idx].min()
    assert depth.max() <= engine.MAX_OBS_LDS   # every locus fits the LDS at the budget of the deepest one
    # the loci compared with the oracle: all deep ones and a seeded sample of the shallow ones
    sample = np.sort(np.concatenate([deep_idx, np.random.default_rng(304).choice(shallow_idx, 4000, replace=False)]))
    return SimpleNamespace(cfg=cfg, b=b, depth=depth, deepest=int(depth.max()), deep=deep_idx, shallow=shallow_idx, sample=sample)


@pytest.fixture(scope="module")
def oracle_a(oracle, batch_a):
    """The oracle (with AFD lists) on the sampled loci of batch A."""
    return oracle_mt(oracle, batch_a.cfg.scenario, batch_a.b.select(batch_a.sample), afd_capacity=AFD_CAP)


@pytest.fixture(scope="module")
def lds_resident_a(batch_a):
    """Batch A with every locus LDS-resident: a plan budget of MAX_OBS_LDS and, in each host chunk, the budget of its deepest locus
    (VLR_NO_FIT_BUDGET)."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VLR_NO_FIT_BUDGET", "1")
        res = run_host(batch_a.cfg.scenario, batch_a.b)
    assert not too_deep(res).any()
    return res


def run_host(scenario, b, plan_budget=engine.MAX_OBS_LDS, fit=False):
    """vlr_batch_run_host under the plan budget `plan_budget` (None: the plan's default, 200 per sample), or with `fit` under the
    budget vlr_plan_fit_max_obs sets for the whole batch (as the cli does)."""
    plan = engine.Plan(scenario)
    if fit:
        plan.fit_max_obs(b.obs_offset)
    elif plan_budget is not None:
        plan.set_max_obs(plan_budget)
    res = plan.call_host(b)
    plan.close()
    return res


def run_device(scenario, b, afd_capacity=0):
    """As bench.py: vlr_plan_fit_max_obs, vlr_plan_reserve, then vlr_batch_run on device columns.  Returns (budget,
    results with the AFD lists on the host)."""
    import torch
    plan = engine.Plan(scenario)
    budget = plan.fit_max_obs(b.obs_offset)
    plan.reserve(b.n_loci, with_afd=afd_capacity)
    db = engine.DeviceBatch(b, "cuda:0")
    out = engine.DeviceResults(b.n_loci, plan.n_out, plan.n_samples, "cuda:0", afd_capacity=afd_capacity)
    plan.call_device(db, out)
    torch.cuda.synchronize()
    res = out.to_host()
    plan.close()
    res.afd_capacity = afd_capacity
    if afd_capacity:
        res.afd_count = out.afd_count.cpu().numpy()
        res.afd_vaf = out.afd_vaf.cpu().numpy()
        res.afd_lnprob = out.afd_lnprob.cpu().numpy()
    del db, out
    return budget, res


def fitted_budget(scenario, b):
    plan = engine.Plan(scenario)
    budget = plan.fit_max_obs(b.obs_offset)
    plan.close()
    return budget


def test_16_workgroup_budget_through_every_entry_point(batch_a, oracle_a, lds_resident_a, monkeypatch):
    """The 16-workgroup budget with the default pool: the deep loci go to the deep launch behind the 4-wave instance.  Device entry
    point (bench.py), the cli's host entry point under the budget fitted to the whole batch, host entry point in one chunk of
    >= 100 000 loci (the same branch) and in default chunks (below 100 000 loci: the budget of the deepest locus).  Nothing flagged,
    oracle parity, bit-identical to the all-LDS-resident run."""
    A = batch_a
    sc = A.cfg.scenario
    budget, dev = run_device(sc, A.b)
    # precondition: this batch takes the 16-workgroup budget (if it ever sits below the shallow tail on gfx950, raise the
    # shallow depth of batch A to 30x: the branch must be reached)
    assert budget < A.deepest, (budget, A.deepest)
    print("batch A: budget %d, %d loci above it" % (budget, int((A.depth > budget).sum())))
    runs = [("device", dev), ("cli: fitted budget, host chunks", run_host(sc, A.b, fit=True))]
    monkeypatch.setenv("VLR_HOST_CHUNK_MB", "100000")   # one chunk: host_chunk_start sees all 100 300 loci
    runs.append(("host, one chunk", run_host(sc, A.b)))
    monkeypatch.delenv("VLR_HOST_CHUNK_MB")
    runs.append(("host, chunks", run_host(sc, A.b)))
    # (and under the plan's default budget of 2 x 200 observations: the deep loci go to the deep launch behind it)
    runs.append(("host, chunks, default plan budget", run_host(sc, A.b, plan_budget=None)))
    for label, res in runs:
        assert not too_deep(res).any(), (label, np.nonzero(too_deep(res))[0][:10])
        assert not internal_bits(res).any(), label
        check_oracle(take(res, A.sample), oracle_a, "batch A, " + label)
        # the deep launch computes what the LDS-resident kernel computes, to the bit
        bad = identical(res, lds_resident_a)
        assert not bad, (label, bad)


def test_16_workgroup_budget_with_afd_lists(batch_a, oracle_a, monkeypatch):
    """Batch A with AFD lists on the device entry point.  A 256 MiB log budget holds at most ~26 000 loci' logs (>= 1 261 words
    a locus), so vlr_batch_run walks the batch in sub-ranges on two lanes; the deep call launch and the deep replay launch run behind
    them from the same pool."""
    A = batch_a
    monkeypatch.setenv("VLR_AFD_LOG_BUDGET_MB", "256")
    budget, got = run_device(A.cfg.scenario, A.b, afd_capacity=AFD_CAP)
    assert budget < A.deepest, (budget, A.deepest)   # precondition: the 16-workgroup budget, deep loci behind it
    assert not too_deep(got).any(), np.nonzero(too_deep(got))[0][:10]
    assert not internal_bits(got).any()
    sub = take(got, A.sample)
    check_oracle(sub, oracle_a, "batch A with AFD")
    n_entries = check_afd(sub, oracle_a, "batch A with AFD")
    assert n_entries > len(A.sample)   # the lists are not trivially empty
    deep_in_sample = np.searchsorted(A.sample, A.deep)
    assert (sub.afd_count[deep_in_sample] > 0).any()   # and the deep replay made some


def test_no_deep_pool_keeps_every_locus_that_fits_the_lds(batch_a, lds_resident_a, oracle, monkeypatch):
    """Without a deep pool (VLR_DEEP_POOL_MB=0), or with one too small for the loci above the 16-workgroup budget, a batch that would
    take that budget keeps the budget of its deepest locus: no locus that fits the LDS comes back flagged, and the results are those
    of the LDS-resident run.  Loci that do not fit the LDS at all still come back flagged when there is no pool."""
    A = batch_a
    sc = A.cfg.scenario
    assert fitted_budget(sc, A.b) < A.deepest   # precondition: with the default pool the batch takes the 16-workgroup budget
    for mb in ("0", "1"):   # no pool; 1 MiB, about a fifth of what the 300 deep loci need
        monkeypatch.setenv("VLR_DEEP_POOL_MB", mb)
        assert fitted_budget(sc, A.b) >= A.deepest, mb
        _, dev = run_device(sc, A.b)
        runs = [("device", dev), ("cli: fitted budget, host chunks", run_host(sc, A.b, fit=True))]
        monkeypatch.setenv("VLR_HOST_CHUNK_MB", "100000")
        runs.append(("host, one chunk", run_host(sc, A.b)))
        monkeypatch.delenv("VLR_HOST_CHUNK_MB")
        for label, res in runs:
            label = "pool %s MiB, %s" % (mb, label)
            assert not too_deep(res).any(), (label, int(too_deep(res).sum()))
            bad = identical(res, lds_resident_a)
            assert not bad, (label, bad)
    # the contract that stays: above what the LDS can hold at all, no pool means flagged, never silently wrong
    monkeypatch.setenv("VLR_DEEP_POOL_MB", "0")
    cfg_far = synth.config3()
    cfg_far.depth, cfg_far.max_depth = 4500.0, 10000
    far = synth.generate(cfg_far, 4, seed=305)
    cfg_near = synth.config3()
    cfg_near.depth = 20.0
    b = PileupBatch.concat([synth.generate(cfg_near, 12, seed=306), far, synth.generate(cfg_near, 12, seed=307)])
    depth = b.depth().sum(axis=1)
    far_idx = np.arange(12, 16)
    assert depth[far_idx].min() > 1.1 * engine.MAX_OBS_LDS   # (kept ones too: 2 % of the reads are dropped at most)
    got = run_host(sc, b)
    assert np.array_equal(np.nonzero(too_deep(got))[0], far_idx), np.nonzero(too_deep(got))[0]
    near = np.setdiff1d(np.arange(b.n_loci), far_idx)
    check_oracle(take(got, near), oracle_mt(oracle, sc, b.select(near)), "next to loci above the LDS, no pool")


# ---------------------------------------------------------------------------------------------------------------- batch B

@pytest.mark.parametrize("afd", [0, AFD_CAP], ids=["calls", "afd"])
@pytest.mark.parametrize("seed", [401, 402, 403])
def test_short_deep_pool_each_locus_is_complete_or_flagged(oracle, monkeypatch, seed, afd):
    """A budget of 64 observations sends nearly every locus to the deep launch, and a 1 MiB pool (~43 000 observations) holds about
    200 of ~3 000.  The deep call pass and, with AFD lists, the deep replay allocate from the same pool one after the other; which
    loci win depends on the order of the atomics.  Every locus is either flagged VLR_LOCUS_TOO_DEEP or complete: posteriors, MAP,
    biases, status and AFD lists of the oracle."""
    cfg = synth.config3()
    b = synth.generate(cfg, 3000, seed=seed)
    monkeypatch.setenv("VLR_DEEP_POOL_MB", "1")
    plan = engine.Plan(cfg.scenario)
    plan.set_max_obs(64)
    got = plan.call_host(b, afd_capacity=afd)
    plan.close()
    assert not internal_bits(got).any()
    flagged = too_deep(got)
    done = np.nonzero(~flagged)[0]
    assert (b.depth().sum(axis=1)[done] > 64).any()   # precondition: the deep launch evaluated loci ...
    assert flagged.any()                              # ... and ran out of pool
    print("seed %d afd %d: %d of %d loci evaluated" % (seed, afd, len(done), b.n_loci))
    ref = oracle_mt(oracle, cfg.scenario, b.select(done), afd_capacity=afd)
    sub = take(got, done)
    # above all: no unflagged locus without posteriors (a NaN MAP where the oracle has one)
    lost = np.isnan(sub.map_vaf).any(axis=1) & ~np.isnan(ref.map_vaf).any(axis=1)
    assert not lost.any(), ("unflagged, not evaluated", done[lost][:10])
    check_oracle(sub, ref, "pool pressure, seed %d" % seed)
    if afd:
        check_afd(sub, ref, "pool pressure, seed %d" % seed)
