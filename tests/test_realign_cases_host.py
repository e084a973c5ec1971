"""The batches of tests/test_gpu_realign_guard.py are what they claim to be — checked on the CPU oracle alone, so that a GPU failure
there is a statement about the kernel and not about its input.  An unrelated pair must lie below ln P = -709, under which linear f64
holds nothing without scaling; a planted pair must lie near ln 1."""
import numpy as np

import realign_cases as rc
from varlociraptor_amd.realign import GapParams


def _pairhmm(oracle, pb, gap=None):
    return oracle.pairhmm_batch(pb, gap or GapParams(), threads=8)


def test_q93_guard_batches(oracle):
    unrelated, planted = rc.guard_q93()
    assert len(unrelated) == 400 and len(planted) == 400
    assert all(len(y) == 128 and len(x) == 200 for x, y in zip(unrelated.x, unrelated.y))
    assert all(len(y) == 128 and len(x) == 458 and x[300:428] == y for x, y in zip(planted.x, planted.y))
    assert all(q == bytes([93]) * 128 for q in unrelated.q + planted.q)
    u, p = _pairhmm(oracle, unrelated), _pairhmm(oracle, planted)
    assert u.max() < -709.0 and abs(u.max() - -1258.5) < 0.1, u.max()      # measured maximum -1258.5
    assert p.min() > -0.01 and abs(p.min() - -0.001006) < 1e-5, p.min()    # measured minimum -0.001006
    # the band of 100 edits admits the planted alignment and leaves the unrelated pairs out of linear range
    ub, pb_ = _pairhmm(oracle, rc.banded(unrelated, rc.GUARD_BAND)), _pairhmm(oracle, rc.banded(planted, rc.GUARD_BAND))
    assert np.all(ub[np.isfinite(ub)] < -709.0) and np.isfinite(ub).sum() >= 390 and pb_.min() > -0.01


def test_smaller_guard_batches(oracle):
    assert sorted(rc.GUARD_SMALL) == ["gap_extension", "mixed_quals", "q41", "q60", "q80", "q93_len64", "q93_len96"]
    for name, (_, len_y, quals, _) in rc.GUARD_SMALL.items():
        pb, gap, first_planted = rc.guard_small(name)
        assert len(pb) == 200 and first_planted == 100
        assert all(len(y) == len_y for y in pb.y) and all(set(q) <= set(quals) for q in pb.q)
        p = _pairhmm(oracle, pb, gap)
        # a planted read costs its own match emissions (ln(1 - 10^-q/10) per base: -1 at Q2) and 128 match transitions (4e-2 with
        # gap extension's larger gap opens), nothing else
        floor = np.array([sum(np.log1p(-10.0 ** (-q / 10.0)) for q in pb.q[k]) for k in range(100, 200)])
        assert (p[100:] - floor).min() > -0.05 and (p[100:] - floor).max() <= 1e-9, (name, (p[100:] - floor).min())
        # an unrelated read lies at least 2^-700 down (three rescalings and more), most batches below the range of linear f64
        assert p[:100].max() < -500.0, (name, p[:100].max())
        if min(quals) >= 41 and len_y >= 96:
            assert p[:100].max() < -709.0, (name, p[:100].max())


def test_homopolymer_guard_batch(oracle):
    pb, hop, first_planted = rc.guard_homopolymer()
    assert len(pb) == 400 and first_planted == 200
    p = oracle.homopoly_batch(pb, GapParams(), hop, threads=8)
    # a planted read: every match state is left with 1 - (gaps + hop_x + hop_y) >= 0.9, 128 times
    assert p[:200].max() < -709.0 and p[200:].min() > 128 * np.log(0.9), (p[:200].max(), p[200:].min())


def test_shape_batches_have_the_stated_sizes():
    pb = rc.small_shapes()
    assert len(pb) == 62 * 30 == 1860
    assert {len(x) for x in pb.x} == {1, 2, 3, 4, 5} and {len(y) for y in pb.y} == {1, 2, 3, 4}
    assert pb.q[-1] == bytes(rc.SMALL_QUALS)
    geo = rc.wave_geometry(4)
    assert len(geo) == 280 and set(geo.band) == {4}
    assert {len(y) for y in geo.y} == set(rc.GEOMETRY_LEN_Y) and {len(x) for x in geo.x} == set(rc.GEOMETRY_LEN_X)
    assert sum(len(v[0]) for v in rc.kernel_pair_batches().values()) == 2 * 402 + 200 + 15


def test_wave_geometry_covers_the_neighbour_kinds():
    pb = rc.wave_geometry()
    assert len(pb) == 2 * len(rc.GEOMETRY_LEN_X) * len(rc.GEOMETRY_LEN_Y)
    kinds = set()
    for w in range(len(pb) // 2):
        a, b = len(pb.y[2 * w]), len(pb.y[2 * w + 1])
        kinds.add(("short" if a <= 64 else "long", "short" if b <= 64 else "long", len(pb.x[2 * w]) != len(pb.x[2 * w + 1])))
    assert {("short", "short", True), ("short", "short", False), ("short", "long", False), ("long", "long", True), ("long", "long", False)} <= kinds
