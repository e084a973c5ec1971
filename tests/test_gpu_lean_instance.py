"""The lean build of the call kernel (vlr_kernels_lean.hip) against the general build.

The lean unit is the same kernel source with everything compiled out that the host has proved unreachable for the plan and the
launch (AFD log and replay, l2fc operands, the general tree walk, plans above two samples).  No arithmetic differs, so for every
plan that takes it the results must equal the general unit's bit for bit (VLR_NO_LEAN=1, read per launch, forces the general
unit), and a plan or launch that needs any of the parts left out must take the general unit.

Single-sample plans qualify by shape but keep the general unit: the 6-wave instance they run was measured 3.5-5 % slower in the
lean build (config 2: 2.81 -> 2.93 ms per 100 000 loci, profiles/lean_unit.md), so the selection tests below expect the general
unit for them."""
import os
import sys

import numpy as np
import pytest

from varlociraptor_amd import abi, engine, synth
from varlociraptor_amd.scenario import Sample, Scenario

from parity import compare, describe
from test_gpu_edge_cases import oracle_mt, with_depth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("ln_posterior", "ln_marginal", "map_vaf", "map_bias", "best_event", "status")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind == "f" else a


def _run(plan, batch, lean, afd=0):
    """One call of `plan` with the lean unit allowed (lean=True) or forced off; returns (results, (waves, lean flag))."""
    old = os.environ.pop("VLR_NO_LEAN", None)
    try:
        if not lean:
            os.environ["VLR_NO_LEAN"] = "1"
        got = plan.call_host(batch, afd_capacity=afd)
        return got, plan.last_instance()
    finally:
        os.environ.pop("VLR_NO_LEAN", None)
        if old is not None:
            os.environ["VLR_NO_LEAN"] = old


def _assert_same(a, b, label):
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y)), "%s: %s differs between the lean and the general unit" % (label, f)


def test_every_build_matrix_workload_is_bit_identical_with_the_lean_unit_on_and_off():
    """All workloads of tests/test_gpu_build_matrix.py (tools/matrix_run.py: tiny and empty pileups, configs 2-5, 24 fuzzer
    scenarios), launched without AFD lists so that the plans that qualify take the lean unit."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("matrix_run", os.path.join(ROOT, "tools", "matrix_run.py"))
    matrix_run = importlib.util.module_from_spec(spec)
    saved_path = list(sys.path)
    try:
        spec.loader.exec_module(matrix_run)   # (puts tools/ on sys.path for its own imports)
        todo = matrix_run.workloads("quick")
    finally:
        sys.path[:] = saved_path
    n_lean = 0
    names, rejected = [], []
    for name, sc, batch, _afd in todo:
        try:
            plan = engine.Plan(sc)
        except engine.EngineError:
            rejected.append(name)  # rejected by the plan compiler: no unit runs it (matrix_run.main() records the same)
            continue
        on, (w_on, lean_on) = _run(plan, batch, True)
        off, (w_off, lean_off) = _run(plan, batch, False)
        plan.close()
        assert not lean_off, name
        assert w_on == w_off, "%s: the lean launcher chose another instance (%d waves per SIMD, general %d)" % (name, w_on, w_off)
        _assert_same(on, off, name)
        n_lean += bool(lean_on)
        names.append((name, lean_on))
    print("lean unit taken by:", [n for n, l in names if l])
    print("rejected by the plan compiler:", rejected)
    # no case left out: 4 single-sample depths + 5 configs + 24 fuzzer scenarios, each either compared or rejected by name, and only
    # fuzzer scenarios may be rejected
    assert len(todo) >= 9 and len(names) + len(rejected) == len(todo)
    assert all(n.startswith("fuzz_") for n in rejected), rejected
    assert len(names) >= 9 + (len(todo) - 9) // 2, "too few workloads compared: %d of %d" % (len(names), len(todo))
    took = dict(names)
    # the tumor-normal workloads must have exercised the lean unit, or the comparison above compared nothing
    for must in ("tn_tiny", "config3", "config4"):
        assert took.get(must), "%s did not take the lean unit" % must
    for must_not in ("config2", "single_3", "config5"):
        assert must_not in took and not took[must_not], "%s must take the general unit" % must_not


@pytest.mark.parametrize("cfg_fn", [synth.config3, synth.config4], ids=["tumor-normal", "tumor-normal-mixed"])
def test_plain_launches_take_the_lean_unit_and_afd_launches_the_general_one(oracle, cfg_fn):
    cfg = cfg_fn()
    batch = synth.generate(cfg, 160, seed=31)
    plan = engine.Plan(cfg.scenario)
    plain, (_, lean) = _run(plan, batch, True)
    assert lean, "a plain launch of this plan must take the lean unit"
    with_afd, (_, lean_afd) = _run(plan, batch, True, afd=64)
    assert not lean_afd, "a launch with AFD buffers must take the general unit"
    forced, (_, lean_forced) = _run(plan, batch, False)
    assert not lean_forced
    plan.close()
    _assert_same(plain, forced, cfg.name)
    _assert_same(plain, with_afd, cfg.name + " with AFD")
    ref = oracle_mt(oracle, cfg.scenario, batch)
    m = compare(plain, ref, label=cfg.name)
    assert m["frac_within"] == 1.0 and m["bias_equal"] and m["status_equal"], describe(m)
    ref_afd = oracle.call(cfg.scenario, batch, afd_capacity=64)
    assert np.array_equal(with_afd.afd_count, ref_afd.afd_count)


def _general_only_plans():
    # an l2fc term (tests/test_gpu_edge_cases.py test_log2_fold_change_events)
    samples = {"a": Sample(resolution=0.05, universe="[0.0,1.0]"), "b": Sample(resolution=0.05, universe="[0.0,1.0]")}
    sc = Scenario(samples, {"a_greater": "l2fc(a,b) > 1.0 & a:]0.0,1.0] & b:]0.0,1.0]",
                            "similar": "l2fc(a,b) <= 1.0 & l2fc(a,b) >= -1.0 & a:]0.0,1.0] & b:]0.0,1.0]",
                            "b_greater": "l2fc(a,b) < -1.0 & a:]0.0,1.0] & b:]0.0,1.0]"})
    cfg = synth.SynthConfig(name="lfc", config_id=9, scenario=sc, depth=25.0, type_mix={abi.VT_SNV: 1.0},
                            classes=[("absent", 0.3, ((0.0, 0.0), (0.0, 0.0))), ("a", 0.35, ((0.3, 0.9), (0.02, 0.2))),
                                     ("both", 0.35, ((0.2, 0.6), (0.2, 0.6)))])
    yield "l2fc term", sc, synth.generate(cfg, 60, seed=15)
    # tables above 64 entries (resolution 1e-4: nested ranges through the general walk)
    sc = Scenario({"a": Sample(resolution=0.0001, universe="[0.0,1.0]"), "b": Sample(resolution=0.0001, universe="[0.0,1.0]")},
                  {"both": "a:]0.0,0.5[ & b:]0.0,1.0]", "only_b": "a:0.0 & b:]0.0,1.0]"})
    cfg = with_depth(synth.config3(), 12.0)
    cfg.scenario = sc
    cfg.purity = None
    yield "table capacity above 64", sc, synth.generate(cfg, 6, seed=22)
    # a wide plan: five nested ranges on a path
    names = ["r%d" % i for i in range(5)]
    smp = {n: Sample(resolution=0.999, universe="[0.0,1.0]") for n in names}
    sc = Scenario(smp, {"all": " & ".join("%s:]0.0,1.0[" % n for n in names), "none_but_first": "r0:]0.0,1.0] & " + " & ".join("%s:0.0" % n for n in names[1:])})
    classes = [("absent", 0.4, tuple((0.0, 0.0) for _ in names)), ("all", 0.6, tuple((0.2, 0.8) for _ in names))]
    cfg = synth.SynthConfig(name="nest5", config_id=62, scenario=sc, depth=8.0, type_mix={abi.VT_SNV: 1.0}, classes=classes, purity=None)
    yield "wide plan", sc, synth.generate(cfg, 8, seed=72)
    # a pedigree: more than two samples, Set spectra
    cfg = synth.config5()
    yield "pedigree", cfg.scenario, synth.generate(cfg, 100, seed=5)
    # a single-sample plan: qualifies by shape, but its 6-wave instance is slower in the lean build
    cfg = synth.config2()
    yield "single sample", cfg.scenario, synth.generate(cfg, 160, seed=31)


def test_plans_that_need_a_part_left_out_take_the_general_unit(oracle):
    seen = 0
    for label, sc, batch in _general_only_plans():
        plan = engine.Plan(sc)
        got, (_, lean) = _run(plan, batch, True)
        plan.close()
        assert not lean, "%s: must take the general unit" % label
        ref = oracle_mt(oracle, sc, batch)
        m = compare(got, ref, label=label)
        assert m["frac_within"] == 1.0 and m["bias_equal"] and m["status_equal"], describe(m)
        seen += 1
    assert seen == 5


def test_loci_above_the_pileup_budget_go_through_the_deep_launch_with_the_lean_unit_on_and_off():
    cfg = synth.config3()
    batch = synth.generate(cfg, 300, seed=8)
    plan = engine.Plan(cfg.scenario)
    full, (_, lean_full) = _run(plan, batch, True)
    plan.set_max_obs(200)  # about half of the 2 x 100x pileups lie above it: flagged by the call launch, evaluated by the deep launch
    on, (_, lean_on) = _run(plan, batch, True)
    off_, (_, lean_off) = _run(plan, batch, False)
    plan.close()
    assert lean_on and not lean_off
    S = batch.n_samples
    off = np.asarray(batch.obs_offset).reshape(-1).astype(np.int64)
    depth = off[S::S][: batch.n_loci] - off[0:-1:S][: batch.n_loci]
    assert (depth > 200).any() and (depth <= 200).any(), "the batch must have loci on both sides of the budget"
    assert not (np.asarray(on.status) & abi.LOCUS_TOO_DEEP).any()
    _assert_same(on, off_, "deep launch")
    assert lean_full
