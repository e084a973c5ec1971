"""The outer rounds of the lean unit's nested root (outer_root in vlr_kernels.hip) against the general unit's walk_root.

In the lean unit the one nested root shape it admits — a proper Range node over one leaf Range node — is not walked by the general
state machine: the outer chain's state lives in wave-uniform registers across the chain batches, its pending points are recomputed
from that state, and one block per round delivers, advances and sets up the next tasks.  No arithmetic differs, so every case below
runs a few dozen loci with the lean unit allowed and again with VLR_NO_LEAN=1 (the general unit: walk_root with its Frame / RangeSt
records), asserts that the first launch took the lean unit, compares all six result fields bit for bit, and compares the lean
results against the oracle under the suite's criterion.

The shapes are the smallest at which the driver takes another path: Simpson grids in either frame, a dead inner range (rounds
without a batch), a narrow outer range, contamination in either direction, held / stashed / riding chains of other events in every
combination, two nested roots in one scenario, artifact hypotheses after parked coefficient sets, odd batch sizes.

Nesting order: the operands of a conjunction are sorted by sample name (Formula::sort), so the outer Range is always on the FIRST
sample and the leaf on the second — "outer on the second sample" cannot be built.  What can differ is which of the two is the
contaminated one, and that is what the role cases vary: the leaf sample contaminated by the outer one (tumor-normal), the outer
sample contaminated by the leaf one (the chain then moves two pileups), and neither."""
import numpy as np
import pytest

from varlociraptor_amd import abi, engine, synth
from varlociraptor_amd.scenario import Contamination, Sample, Scenario

from parity import compare, describe
from test_gpu_edge_cases import oracle_mt, with_depth
from test_gpu_lean_instance import _assert_same, _run

pytestmark = pytest.mark.gpu

NORMAL_UNIVERSE = "[0.0,0.5[ | 0.5 | 1.0"
NESTED = "tumor:]0.0,1.0] & normal:]0.0,0.5["
CHAINS = (("somatic_tumor", "tumor:]0.0,1.0] & normal:0.0"), ("germline_het", "tumor:]0.0,1.0] & normal:0.5"),
          ("germline_hom", "tumor:]0.0,1.0] & normal:1.0"))


def _tn_scenario(events, contamination=0.25, tumor_res=0.01, normal_res=0.1):
    cont = Contamination("normal", contamination) if contamination else None
    return Scenario({"tumor": Sample(resolution=tumor_res, universe="[0.0,1.0]", contamination=cont),
                     "normal": Sample(resolution=normal_res, universe=NORMAL_UNIVERSE)}, dict(events))


def _tn_config(sc, depth, contaminated=True, **kw):
    """The tumor-normal generator (sample order: normal 0, tumor 1) on scenario `sc`."""
    cfg = with_depth(synth.config3(), float(depth), **kw)
    cfg.scenario = sc
    if not contaminated:
        cfg.purity = None
    return cfg


def _ab_config(sc, depth):
    """Two samples a (index 0, the outer one) and b (index 1, the leaf)."""
    return synth.SynthConfig(name="ab", config_id=71, scenario=sc, depth=float(depth), type_mix={abi.VT_SNV: 0.8, abi.VT_INDEL: 0.2},
                             classes=[("absent", 0.3, ((0.0, 0.0), (0.0, 0.0))), ("only_b", 0.3, ((0.0, 0.0), (0.05, 0.45))),
                                      ("both", 0.4, ((0.05, 0.6), (0.05, 0.45)))], purity=None)


def _check(oracle, sc, batch, label):
    """Lean unit against the general unit (bit for bit) and against the oracle; returns the lean results and the plan's fused counters."""
    plan = engine.Plan(sc)
    plan.fused_counters(reset=True)
    on, (w_on, lean_on) = _run(plan, batch, True)
    fused = plan.fused_counters()
    off, (w_off, lean_off) = _run(plan, batch, False)
    plan.close()
    assert lean_on, "%s: the plan must take the lean unit, or nothing of the new driver is compared" % label
    assert not lean_off and w_on == w_off, label
    _assert_same(on, off, label)
    ref = oracle_mt(oracle, sc, batch)
    m = compare(on, ref, label=label)
    assert m["frac_within"] == 1.0 and m["bias_equal"] and m["status_equal"], describe(m)
    return on, fused


def _column(sc, event):
    """Column of a named event in ln_posterior: absent first, the named events in name order, the artifact event last."""
    return 1 + sorted(sc.events).index(event)


@pytest.mark.parametrize("depth", [2, 4, 9, 12, 30, 100])
def test_depth_ladder(oracle, depth):
    """n_obs < 5: 11-point Simpson grids in the outer and the inner frame; n_obs < 10: the excluded range start is visited;
    above: adaptive rounds over observable bounds."""
    cfg = with_depth(synth.config3(), float(depth))
    batch = synth.generate(cfg, 40, seed=100 + depth)
    _check(oracle, cfg.scenario, batch, "depth %d" % depth)


def test_dead_inner_range(oracle):
    """The inner range starts above 0 and the inner sample's pileup is clear-ref at many loci: the set-up step returns without
    chains, every outer point is recorded as ln 0 and the frame advances without a batch."""
    sc = Scenario({"tumor": Sample(resolution=0.01, universe="[0.0,1.0]"), "normal": Sample(resolution=0.1, universe=NORMAL_UNIVERSE)},
                  {"nested": "tumor:]0.1,1.0] & normal:]0.0,0.5[", "somatic_tumor": "tumor:]0.1,1.0] & normal:0.0"})
    cfg = _tn_config(sc, 30, contaminated=False)
    cfg.classes = [("normal_only", 0.6, ((0.05, 0.45), (0.0, 0.0))), ("both", 0.4, ((0.05, 0.45), (0.2, 0.6)))]
    batch = synth.generate(cfg, 48, seed=211)
    on, _ = _check(oracle, sc, batch, "dead inner range")
    dead = np.isneginf(np.asarray(on.ln_posterior)[:, _column(sc, "nested")])
    print("loci with a dead inner range: %d of %d" % (int(dead.sum()), batch.n_loci))
    assert dead.sum() >= 8 and (~dead).sum() >= 8, "the batch must hold loci with and without a dead inner range"


def test_narrow_outer_range(oracle):
    """An outer observable range narrower than its resolution: a 3-point Simpson grid in the outer frame over adaptive inner chains."""
    sc = Scenario({"a": Sample(resolution=0.5, universe="[0.0,1.0]"), "b": Sample(resolution=0.05, universe="[0.0,1.0]")},
                  {"both": "a:]0.0,0.4[ & b:]0.0,1.0]", "only_b": "a:0.0 & b:]0.0,1.0]"})
    batch = synth.generate(_ab_config(sc, 25), 40, seed=223)
    _check(oracle, sc, batch, "narrow outer range")


def _role_cases():
    tn = dict(CHAINS + (("somatic_normal", NESTED),))
    yield "leaf contaminated by outer", _tn_scenario(tn), True
    yield "tumor-normal, no contamination", _tn_scenario(tn, contamination=0.0), False
    ab = {"both": "a:]0.0,1.0] & b:]0.0,0.5[", "only_b": "a:0.0 & b:]0.0,0.5["}
    for label, cont in (("outer contaminated by leaf", Contamination("b", 0.25)), ("a over b, no contamination", None)):
        yield label, Scenario({"a": Sample(resolution=0.05, universe="[0.0,1.0]", contamination=cont),
                               "b": Sample(resolution=0.1, universe=NORMAL_UNIVERSE)}, ab), None


ROLE_CASES = list(_role_cases())


@pytest.mark.parametrize("case", ROLE_CASES, ids=[c[0] for c in ROLE_CASES])
def test_contamination_roles(oracle, case):
    """Without contamination the outer sample enters each inner chain only as a fixed likelihood at its outer point (`vary` holds the
    outer sample alone); contaminating the leaf sample, it also sets each chain's contaminant VAF; contaminated BY the leaf sample,
    its pileup moves with the chain and nothing varies with the outer point alone."""
    label, sc, tn_contaminated = case
    cfg = _ab_config(sc, 30) if tn_contaminated is None else _tn_config(sc, 30, contaminated=tn_contaminated)
    batch = synth.generate(cfg, 40, seed=307)
    _check(oracle, sc, batch, label)


EVENT_SETS = [("nested alone", (("somatic_normal", NESTED),)),
              ("one chain event", CHAINS[:1] + (("somatic_normal", NESTED),)),
              ("two chain events", CHAINS[:2] + (("somatic_normal", NESTED),)),
              ("three chain events", CHAINS + (("somatic_normal", NESTED),)),
              ("two nested roots", CHAINS[:1] + (("normal_low", "tumor:]0.0,1.0] & normal:]0.0,0.25["),
                                                 ("normal_high", "tumor:]0.0,1.0] & normal:[0.25,0.5[")))]


@pytest.mark.parametrize("case", EVENT_SETS, ids=[c[0] for c in EVENT_SETS])
def test_event_sets_beside_the_nested_root(oracle, case):
    """Zero to three single-chain events beside the nested root: none, one held, two held, two held and one in the stash, riding
    along in the free rows of the nested root's batches; two nested roots: the register state is set up again for the second."""
    label, events = case
    sc = _tn_scenario(events)
    batch = synth.generate(_tn_config(sc, 30), 40, seed=401)
    _check(oracle, sc, batch, label)


def test_rounds_under_artifact_hypotheses(oracle):
    """Strand-bias evidence at every locus: the rounds also run under artifact hypotheses, after parked coefficient sets were reloaded."""
    cfg = with_depth(synth.config3(), 40.0)
    cfg.artifact_fraction = 1.0
    batch = synth.generate(cfg, 48, seed=503)
    on, (passes, parked, reloaded, _redone) = _check(oracle, cfg.scenario, batch, "artifact at every locus")
    print("fused counters (passes, parked, reloaded):", passes, parked, reloaded)
    assert parked > 0 and reloaded > 0, "no parked coefficient set was reloaded: the artifact rounds were not exercised"
    assert (np.asarray(on.map_bias).sum(axis=1) > 0).any()


@pytest.mark.parametrize("n_loci", [1, 13])
def test_batch_sizes(oracle, n_loci):
    cfg = with_depth(synth.config3(), 30.0)
    batch = synth.generate(cfg, n_loci, seed=601)
    _check(oracle, cfg.scenario, batch, "%d loci" % n_loci)
