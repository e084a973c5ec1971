"""The host logic of the `call variants` driver (varlociraptor_amd/calldriver.py): grouping, carry, concatenation, the plan and
model caches and the environment switches.  Pure numpy: no device, no engine call."""
import numpy as np
import pytest

from varlociraptor_amd import calldriver as cd, cli
from varlociraptor_amd.batch import CallResults

FIXED = cd.FIELDS[:6]
AFD = cd.FIELDS[6:]


def filled(n_loci, seed, afd_capacity=0, n_out=2, n_samples=1):
    """a CallResults (default numpy allocation) with a different value in every cell"""
    rng = np.random.default_rng(seed)
    r = CallResults(n_loci, n_out, n_samples, afd_capacity)
    for f in cd.FIELDS:
        a = getattr(r, f)
        if a is not None:
            a[...] = rng.integers(1, 200, a.shape) if a.dtype.kind in "iu" else rng.normal(size=a.shape)
    return r


def rows_equal(a, la, b, lb, fields):
    return all(np.array_equal(getattr(a, f)[la], getattr(b, f)[lb]) for f in fields)


def test_regroup_representatives():
    assert cd.regroup_representatives(np.array([0, 7, 0, 7, 9, 7, 9], np.uint64)).tolist() == [0, 1, 2, 1, 4, 1, 4]
    assert cd.regroup_representatives(np.zeros(5, np.uint64)).tolist() == [0, 1, 2, 3, 4]
    assert cd.regroup_representatives(np.zeros(0, np.uint64)).tolist() == []


@pytest.mark.parametrize("afd_capacity", [0, 3])
def test_breakend_rows_are_carried_into_the_next_chunk(afd_capacity):
    fields = FIXED + (AFD if afd_capacity else ())
    one, two = filled(4, 1, afd_capacity), filled(4, 2, afd_capacity)
    one_before, two_before = filled(4, 1, afd_capacity), filled(4, 2, afd_capacity)
    carried = {}
    cd.carry_breakends(one, np.array([0, 0, 5, 0], np.uint64), carried)
    assert sorted(carried) == [5]
    assert all(rows_equal(one, l, one_before, l, fields) for l in range(4))   # a first record keeps its own result
    cd.carry_breakends(two, np.array([5, 6, 0, 5], np.uint64), carried)
    for l in (0, 3):
        assert rows_equal(two, l, one, 2, fields)
        assert not rows_equal(two, l, two_before, l, FIXED)
    for l in (1, 2):
        assert rows_equal(two, l, two_before, l, fields)
    assert sorted(carried) == [5, 6] and sorted(carried[6]) == sorted(fields)
    assert all(np.array_equal(carried[6][f], getattr(two, f)[1]) for f in fields)
    if not afd_capacity:
        assert two.afd_count is None and two.afd_vaf is None and two.afd_lnprob is None


def test_fan_out_copies_the_representative_to_its_group():
    res, before = filled(5, 3, afd_capacity=3), filled(5, 3, afd_capacity=3)
    cd.fan_out(res, np.array([0, 1, 1, 3, 1], np.int64))
    for l, src in enumerate([0, 1, 1, 3, 1]):
        assert rows_equal(res, l, before, src, cd.FIELDS)
    assert not rows_equal(before, 2, before, 1, FIXED)


def test_scatter_reassembles_the_chunk_from_sub_results():
    want = filled(5, 4, afd_capacity=3)
    res = CallResults(5, 2, 1, 3)
    for loci in (np.array([0, 2, 3]), np.array([1, 4])):
        sub = CallResults(len(loci), 2, 1, 3)
        for f in cd.FIELDS:
            getattr(sub, f)[...] = getattr(want, f)[loci]
        cd.scatter(res, sub, loci)
    for f in cd.FIELDS:
        assert np.array_equal(getattr(res, f), getattr(want, f)), f


def test_concat_fixed():
    assert cd.concat_fixed([]) is None
    assert cd.concat_fixed([None]) is None
    r3, r2 = filled(3, 5, afd_capacity=3), filled(2, 6, afd_capacity=3)
    assert cd.concat_fixed([r3]) is r3
    assert cd.concat_fixed([None, r2]) is r2
    tot = cd.concat_fixed([None, r3, r2])
    assert tot.n_loci == 5 and tot.afd_count is None and tot.afd_vaf is None and tot.afd_lnprob is None
    for f in FIXED:
        assert np.array_equal(getattr(tot, f), np.concatenate([getattr(r3, f), getattr(r2, f)])), f


class FakePlan:
    built = []

    def __init__(self, scenario, device=0):
        self.scenario, self.device, self.closed, self.reserved = scenario, device, 0, []
        FakePlan.built.append(self)

    def reserve(self, n_loci, afd_capacity):
        self.reserved.append((n_loci, afd_capacity))

    def close(self):
        self.closed += 1


@pytest.mark.parametrize("chunk_records", [0, 32768])
def test_plan_cache_keeps_four_plans_and_closes_the_oldest(chunk_records):
    FakePlan.built = []
    cache = cd.PlanCache(device=3, afd_capacity=128, plan_class=FakePlan)
    cache.reserve_loci = chunk_records
    plans = [cache.get(("sig", k), "scenario %d" % k) for k in range(5)]
    assert FakePlan.built == plans and len(set(map(id, plans))) == 5
    assert [p.closed for p in plans] == [1, 0, 0, 0, 0]
    assert list(cache.plans) == [("sig", k) for k in range(1, 5)]
    assert all(p.device == 3 and p.scenario == "scenario %d" % k for k, p in enumerate(plans))
    assert cache.get(("sig", 3), "scenario 3") is plans[3] and len(FakePlan.built) == 5   # cached: nothing is built
    for p in plans:   # reserve: on creation, and only when a device reader fixed the chunk size
        assert p.reserved == ([(32768, 128)] if chunk_records else [])
    cache.close_all()
    assert [p.closed for p in plans] == [1, 1, 1, 1, 1] and not cache.plans


def test_plan_cache_builds_engine_plans_by_default():
    from varlociraptor_amd import engine
    assert cd.PlanCache().plan_class is engine.Plan


TWO_CONTIGS = 'samples:\n  normal:\n    resolution: 0.1\n    universe: {all: "[0.0,1.0]", X: "{0.0,1.0}"}\nevents:\n  present: "normal:]0.0,1.0]"\n'


@pytest.fixture
def per_contig(tmp_path):
    y = tmp_path / "s.yaml"
    y.write_text(TWO_CONTIGS)
    return lambda contig: cli.scenario_from_yaml(str(y), contig)


def test_model_cache_resolves_per_contig_and_installs_first_record_priors(per_contig):
    models = cd.ModelCache(per_contig, {"normal": "normal.bcf"})
    assert models.sample_order == ["normal"]
    het = -0.25
    # the first record of contig "1" (index 0) in mode 0 carries a heterozygosity; a later record of the same model does not count
    models.record_first(np.array([0, 0, 256], np.int64), ["1", "X"], np.array([het, -9.0, np.nan]), np.array([np.nan, -7.0, np.nan]))
    assert models.first_of_contig == {("1", 0): (het, None), ("X", 0): (None, None)}
    one, x = models.resolve("1", 0), models.resolve("X", 0)
    assert cd._scenario_signature(one) != cd._scenario_signature(x)
    assert one.samples["normal"].universe != x.samples["normal"].universe
    assert one.variant_heterozygosity_ln == het and one.variant_somatic_effective_mutation_rate_ln is None
    assert x.variant_heterozygosity_ln is None and x.variant_somatic_effective_mutation_rate_ln is None
    assert models.resolve("1", 2).variant_heterozygosity_ln is None   # another model mode: its own first record
    assert models.resolve("1", 0) is one


def test_model_cache_checks_the_sample_names(per_contig):
    with pytest.raises(SystemExit, match="invalid observation sample name 'tumor'"):
        cd.ModelCache(per_contig, {"normal": "n.bcf", "tumor": "t.bcf"}).resolve("1")
    with pytest.raises(SystemExit, match="no observations given for sample 'normal'"):
        cd.ModelCache(per_contig, {}).resolve("1")
    with pytest.raises(SystemExit, match="invalid observation sample name 'tumor'"):   # a plain Scenario: checked at once
        cd.ModelCache(per_contig("1"), {"normal": "n.bcf", "tumor": "t.bcf"})


SWITCH_VARS = ("VLR_INGEST", "VLR_INGEST_HOST", "VLR_INGEST_SHARDED", "VLR_INGEST_SUMMARIES", "VLR_AFD_TEXT", "VLR_CLI_CHUNK", "VLR_CLI_QUEUE",
               "VLR_INGEST_SHARD_REPORT")
DEFAULTS = dict(native=True, host_reader=False, sharded=True, summaries=True, afd_text=True, chunk=0, queue=2, shard_report=None)


@pytest.fixture
def clean_env(monkeypatch):
    for name in SWITCH_VARS:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


def as_dict(sw):
    return {k: getattr(sw, k) for k in DEFAULTS}


def test_switches_defaults(clean_env):
    sw = cd.Switches.from_env()
    assert as_dict(sw) == DEFAULTS
    with pytest.raises(Exception):   # frozen
        sw.chunk = 4


@pytest.mark.parametrize("name,value,field,want", [
    ("VLR_INGEST", "python", "native", False), ("VLR_INGEST", "native", "native", True), ("VLR_INGEST_HOST", "1", "host_reader", True),
    ("VLR_INGEST_HOST", "0", "host_reader", False), ("VLR_INGEST_SHARDED", "0", "sharded", False), ("VLR_INGEST_SUMMARIES", "0", "summaries", False),
    ("VLR_AFD_TEXT", "0", "afd_text", False), ("VLR_AFD_TEXT", "1", "afd_text", True), ("VLR_CLI_CHUNK", "250", "chunk", 250),
    ("VLR_CLI_QUEUE", "5", "queue", 5), ("VLR_INGEST_SHARD_REPORT", "/tmp/report", "shard_report", "/tmp/report")])
def test_switches_read_each_variable(clean_env, name, value, field, want):
    clean_env.setenv(name, value)
    assert as_dict(cd.Switches.from_env()) == dict(DEFAULTS, **{field: want})


def test_switches_ingest_argument_wins_over_the_environment(clean_env):
    clean_env.setenv("VLR_INGEST", "native")
    assert cd.Switches.from_env("python").native is False
    clean_env.setenv("VLR_INGEST", "python")
    assert cd.Switches.from_env("native").native is True
    assert cd.Switches.from_env(None).native is False
