"""The fused coefficient pass of the lean call kernel against one row pass per hypothesis.

Where artifact hypotheses survive the gates of a locus, the lean unit takes the surviving hypotheses in groups: ONE pass over the
observation rows builds the coefficients of the group's first hypothesis and of the next parked sets' worth of them, parks the latter
in device memory and reloads them at their turn; the next group reuses the sets.  The
hypothesis-independent part of every term (all transcendentals) is computed once, the per-hypothesis selects and products are the
same expressions in the same order, so every result must equal, bit for bit, what VLR_NO_FUSED_COEF=1 (read per launch: one row
pass per hypothesis) gives.  Plan.fused_counters() says whether a comparison compared anything."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from varlociraptor_amd import abi, engine, synth
from varlociraptor_amd.batch import PileupBatch

from parity import compare, describe
from test_gpu_edge_cases import oracle_mt, with_depth
from test_gpu_lean_instance import _assert_same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SWITCHES = ("VLR_NO_FUSED_COEF", "VLR_FUSED_SETS")


def _run(plan, batch, fused=True, sets=None, afd=0):
    """One call with the fused pass allowed (at `sets` parked sets per locus, default: the unit's capacity) or switched off;
    returns (results, (fused row passes, sets parked, sets reloaded, hypotheses redone) of this call)."""
    saved = {k: os.environ.pop(k, None) for k in _SWITCHES}
    try:
        if not fused:
            os.environ["VLR_NO_FUSED_COEF"] = "1"
        if sets is not None:
            os.environ["VLR_FUSED_SETS"] = str(sets)
        plan.fused_counters(reset=True)
        got = plan.call_host(batch, afd_capacity=afd)
        return got, plan.fused_counters()
    finally:
        for k in _SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _on_off(sc, batch, label):
    plan = engine.Plan(sc)
    on, cnt = _run(plan, batch, True)
    off, cnt_off = _run(plan, batch, False)
    lean = plan.last_instance()[1]
    plan.close()
    assert cnt_off == (0, 0, 0, 0), "%s: VLR_NO_FUSED_COEF=1 must keep one row pass per hypothesis, counters %r" % (label, cnt_off)
    _assert_same(on, off, label)
    return on, cnt, lean


def test_every_build_matrix_workload_is_bit_identical_with_the_fused_pass_on_and_off():
    spec = importlib.util.spec_from_file_location("matrix_run", os.path.join(ROOT, "tools", "matrix_run.py"))
    matrix_run = importlib.util.module_from_spec(spec)
    saved_path = list(sys.path)
    try:
        spec.loader.exec_module(matrix_run)   # (puts tools/ on sys.path for its own imports)
        todo = matrix_run.workloads("quick")
    finally:
        sys.path[:] = saved_path
    counters, rejected = {}, []
    for name, sc, batch, _afd in todo:
        try:
            engine.Plan(sc).close()
        except engine.EngineError:
            rejected.append(name)  # rejected by the plan compiler: nothing runs it
            continue
        _, cnt, _ = _on_off(sc, batch, name)
        counters[name] = cnt
    print("fused counters (passes, parked, reloaded, redone):", {n: c for n, c in counters.items() if any(c)})
    print("rejected by the plan compiler:", rejected)
    assert len(todo) >= 9 and len(counters) + len(rejected) == len(todo)
    assert all(n.startswith("fuzz_") for n in rejected), rejected
    for must in ("tn_tiny", "config3", "config4"):
        passes, parked, reloaded, _ = counters[must]
        assert parked > 0 and reloaded == parked and passes > 0, "%s: counters %r" % (must, counters[must])


@pytest.fixture(scope="module")
def artifacts():
    """config 3 with an injected artifact at every locus: (config, batch, results of the fused launch, its counters)."""
    cfg = synth.config3()
    cfg.artifact_fraction = 1.0
    batch = synth.generate(cfg, 160, seed=47)
    plan = engine.Plan(cfg.scenario)
    on, cnt = _run(plan, batch, True)
    assert plan.last_instance()[1], "a plain tumor-normal launch must take the lean unit"
    plan.close()
    return cfg, batch, on, cnt


def test_every_locus_has_a_second_hypothesis(oracle, artifacts):
    cfg, batch, on, cnt = artifacts
    plan = engine.Plan(cfg.scenario)
    off, cnt_off = _run(plan, batch, False)
    plan.close()
    assert cnt_off == (0, 0, 0, 0)
    _assert_same(on, off, "artifact at every locus")
    ref = oracle_mt(oracle, cfg.scenario, batch)
    m = compare(on, ref, label="artifact at every locus")
    assert m["frac_within"] == 1.0 and m["bias_equal"] and m["status_equal"], describe(m)
    passes, parked, reloaded, redone = cnt
    print("fused counters:", cnt)
    assert reloaded == parked
    # hypotheses evaluated per locus (h = none and the artifact hypotheses, parked or redone): more than one on average
    assert passes > 0 and (batch.n_loci + parked + redone) / batch.n_loci > 1.0, cnt


@pytest.mark.parametrize("sets", [1, 0])
def test_hypotheses_beyond_the_parked_sets_keep_their_own_row_pass(artifacts, sets):
    cfg, batch, on, cnt_full = artifacts
    plan = engine.Plan(cfg.scenario)
    got, cnt = _run(plan, batch, True, sets=sets)
    plan.close()
    _assert_same(on, got, "%d parked sets" % sets)
    passes, parked, reloaded, redone = cnt
    print("fused counters at %d sets:" % sets, cnt, "full:", cnt_full)
    assert reloaded == parked
    if sets == 0:   # every artifact hypothesis takes the row pass of its own, and is counted
        assert passes == 0 and parked == 0 and redone > cnt_full[3]
    else:           # groups of two: one set parked per fused pass, more passes than with two sets
        assert 0 < parked <= passes and passes >= cnt_full[0]


def test_a_launch_with_afd_lists_gives_the_same_arrays(artifacts):
    cfg, batch, on, _ = artifacts
    plan = engine.Plan(cfg.scenario)
    with_afd, cnt = _run(plan, batch, True, afd=64)
    lean = plan.last_instance()[1]
    plan.close()
    assert not lean and cnt == (0, 0, 0, 0), "a launch with AFD buffers takes the general unit, which has no fused pass"
    _assert_same(on, with_afd, "with AFD lists")


def _with_depths(batch, depths):
    """The first len(depths) loci of `batch` with every pileup cut to the given (sample 0, sample 1) depths."""
    S = batch.n_samples
    off = batch.obs_offset.astype(np.int64)
    idx, new_off = [], [0]
    for l, dd in enumerate(depths):
        for s, d in enumerate(dd):
            o0, o1 = off[l * S + s], off[l * S + s + 1]
            assert o1 - o0 >= d, "pileup (%d, %d) has %d rows, %d wanted" % (l, s, o1 - o0, d)
            idx.append(np.arange(o0, o0 + d))
            new_off.append(new_off[-1] + d)
    idx = np.concatenate(idx)
    cols = {k: v[idx] for k, v in batch.columns.items()}
    loc = {k: v[:len(depths)] for k, v in batch.locus.items()}
    return PileupBatch(S, np.asarray(new_off, np.uint32), cols, loc)


# (normal, tumor) rows per locus: around the 64-observation blocks of the row pass (1, 63, 64, 65, 128, 129), an empty pileup in either
# sample, around the 16 x 13 = 208 observations of the register-resident chain runner, and the plan's pileup budget of 2 x 200
ROW_DEPTHS = [(1, 1), (63, 1), (64, 64), (65, 63), (128, 64), (129, 65), (0, 40), (40, 0), (207, 129), (208, 192), (64, 128), (127, 129),
              (1, 64), (209, 65), (192, 8), (200, 200)]


@pytest.mark.parametrize("orient_other", [0.0, 0.05], ids=["every-row-kept", "rows-dropped"])
def test_row_block_boundaries(orient_other):
    """`every-row-kept`: no observation has the orientation that SNV loci drop, so the kept counts ARE the depths above;
    `rows-dropped`: one row in twenty is dropped, the compaction offsets inside a block differ from the lane numbers."""
    cfg = with_depth(synth.config3(), 280.0, artifact_fraction=1.0, other_orientation=orient_other, max_depth=400)
    deep = synth.generate(cfg, 16, seed=5)
    assert int(deep.depth().min()) >= 209
    batch = _with_depths(deep, ROW_DEPTHS)
    assert [tuple(int(v) for v in r) for r in batch.depth()] == ROW_DEPTHS
    _, cnt, lean = _on_off(cfg.scenario, batch, "row boundaries")
    print("fused counters:", cnt)
    assert lean and cnt[1] > 0 and cnt[2] == cnt[1], cnt


def test_loci_above_the_pileup_budget_go_through_the_deep_launch():
    cfg = synth.config3()
    batch = synth.generate(cfg, 300, seed=8)
    plan = engine.Plan(cfg.scenario)
    plan.set_max_obs(200)  # about half of the 2 x 100x pileups lie above it: flagged by the call launch, evaluated by the deep launch
    on, cnt = _run(plan, batch, True)
    off, _ = _run(plan, batch, False)
    plan.close()
    depth = batch.depth().sum(axis=1)
    assert (depth > 200).any() and (depth <= 200).any(), "the batch must have loci on both sides of the budget"
    assert not (np.asarray(on.status) & abi.LOCUS_TOO_DEEP).any()
    _assert_same(on, off, "deep launch")
    assert cnt[2] == cnt[1]


def test_rescue_and_all_ones_terms_keep_their_own_row_pass(oracle):
    """Whole terms below the f64 range (prob_alt, prob_ref, prob_missed_allele around -800, as
    test_whole_terms_below_the_f64_range_take_the_scaled_coefficient_pass builds them) need the scaled second pass: the fused
    pass must hand such a hypothesis back to the row pass of its own.  Half of the loci are indels, whose prob_sample_alt
    terms give non-zero third coefficients (the e rows of the parked sets)."""
    cfg = with_depth(synth.config3(type_mix={abi.VT_SNV: 0.5, abi.VT_INDEL: 0.5}), 40.0, artifact_fraction=1.0)
    clean = synth.generate(cfg, 96, seed=61)
    assert (clean.columns["prob_sample_alt"] != 0).any()
    _, cnt_clean, lean = _on_off(cfg.scenario, clean, "indel loci")
    assert lean and cnt_clean[1] > 0 and cnt_clean[2] == cnt_clean[1], cnt_clean
    b = synth.generate(cfg, 96, seed=61)
    rng = np.random.default_rng(61)
    hit = rng.random(b.n_obs) < 0.15
    for col, v in (("prob_alt", -800.0), ("prob_ref", -805.0), ("prob_missed_allele", -802.0)):
        a = b.columns[col]
        a[hit] = np.float32(v) + rng.integers(-20, 20, int(hit.sum())).astype(np.float32)
    got, cnt, _ = _on_off(cfg.scenario, b, "rescue batch")
    print("fused counters, rescue batch:", cnt)
    assert cnt[3] > 0 and cnt[2] == cnt[1], cnt
    assert not (got.status & 0xF).any()
    ref = oracle_mt(oracle, cfg.scenario, b)
    m = compare(got, ref, label="rescue batch")
    assert m["frac_within"] == 1.0 and m["bias_equal"] and m["status_equal"], describe(m)
