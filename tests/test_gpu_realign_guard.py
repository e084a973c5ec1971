"""The pair-HMM kernels (varlociraptor_amd/csrc/vlr_realign.hip) where a kernel goes wrong and random windows do not look:

  1. the per-lane power-of-two scaling of the three summing kernels, on Q93 x 128-base reads that are unrelated to the allele
     (ln P below -1250: hundreds of rescalings) or an exact copy planted behind 300 unrelated bases (ln P = -0.001: a lane that
     has scaled tiny lead-in cells up is handed the bulk), unbanded and with a band of 100 edits; lower qualities, shorter reads,
     per-base quality mixtures, gap extension; the homopolymer kernel's copy of the guard;
  2. the one-pair-per-wave kernel (VLR_REALIGN_SINGLE, read once per process: a child process) against the two-pair kernel,
     bit for bit;
  3. every allele of 1..5 and read of 1..4 bases over {A, C}: start row, start column, insertion chain, one-cell matrices,
     reads longer than the allele, in all four kernels;
  4. read lengths on lane / half-wave edges against allele lengths on the edges of the 64-column (two pairs per wave: 32) chunk
     in which the allele bases are loaded;
  5. quality 0, 1, 2, N bases, lower case; the device-pointer entries of the homopolymer and fast modes; gap opens that sum
     to more than one.

Every pair is compared with the CPU restatement (oracle/vlr_realign_oracle.cpp): |d ln P| <= 1e-9 * max(1, 1e-3 |ref|) for the
summing kernels (the bound of tests/test_gpu_realign.py::check), 1e-9 * max(1, |ref|) for fast mode, equality for the edit
distance.  Two -inf are equal; a NaN is a failure.  tests/test_realign_cases_host.py checks the batches themselves."""
import functools
import math
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import realign_cases as rc
from varlociraptor_amd import engine, realign
from varlociraptor_amd.realign import GapParams, HopParams, PairBatch

pytestmark = pytest.mark.gpu
TOL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def agree(got, ref, rel=1e-3, what=""):
    """Every pair within TOL * max(1, rel * |ref|); -inf equals -inf; no NaN on either side."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    assert not np.isnan(ref).any(), (what, "NaN in the reference", np.nonzero(np.isnan(ref))[0][:20].tolist())
    both_inf = np.isneginf(got) & np.isneginf(ref)
    with np.errstate(invalid="ignore"):
        d = np.where(both_inf, 0.0, np.abs(got - ref))
        bad = np.nonzero(~(d <= TOL * np.maximum(1.0, np.abs(ref) * rel)))[0]   # (a NaN or an infinite difference is not <=)
    print("%s: %d pairs, %d wrong, max |d ln P| %.3g" % (what, len(got), len(bad), float(np.max(np.where(np.isfinite(d), d, 0.0), initial=0.0))))
    assert len(bad) == 0, (what, len(bad), bad[:40].tolist(), got[bad[:8]].tolist(), ref[bad[:8]].tolist())


def _threaded(f, n):
    with ThreadPoolExecutor(max_workers=8) as ex:
        return np.array(list(ex.map(f, range(n))))


def ref_pairhmm(oracle, pb, gap):
    return oracle.pairhmm_batch(pb, gap, threads=8)


def ref_homopoly(oracle, pb, gap, hop):
    return oracle.homopoly_batch(pb, gap, hop, threads=8)


def ref_fast(oracle, pb, gap):
    g = rc.gap_list(gap)
    return _threaded(lambda k: oracle.pathhmm_best(pb.x[k], pb.y[k], pb.q[k], g), len(pb))


def with_band(pb, band):
    return pb if band < 0 else rc.banded(pb, band)


# ---- 1. scaling guard ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _q93():
    return rc.guard_q93()


@pytest.mark.parametrize("band", [-1, rc.GUARD_BAND])
@pytest.mark.parametrize("kind", ["unrelated", "planted"])
def test_scaling_guard_q93_x_128(oracle, kind, band):
    pb = with_band(_q93()[0 if kind == "unrelated" else 1], band)
    assert len(pb) == 400
    agree(realign.prob_related(pb), ref_pairhmm(oracle, pb, GapParams()), what="q93 %s band %d" % (kind, band))


@pytest.mark.parametrize("band", [-1, rc.GUARD_BAND])
@pytest.mark.parametrize("name", sorted(rc.GUARD_SMALL))
def test_scaling_guard_other_qualities_lengths_and_gaps(oracle, name, band):
    pb, gap, _ = rc.guard_small(name)
    pb = with_band(pb, band)
    assert len(pb) == 200
    agree(realign.prob_related(pb, gap), ref_pairhmm(oracle, pb, gap), what="%s band %d" % (name, band))


@pytest.mark.parametrize("band", [-1, rc.GUARD_BAND])
def test_scaling_guard_of_the_homopolymer_kernel(oracle, band):
    pb, hop, _ = rc.guard_homopolymer()
    pb = with_band(pb, band)
    assert len(pb) == 400
    agree(realign.prob_related_homopolymer(pb, GapParams(), hop), ref_homopoly(oracle, pb, GapParams(), hop), what="homopolymer q93 band %d" % band)


# ---- 2. one pair per wave == two pairs per wave ----------------------------------------------------------------------------

def test_one_pair_per_wave_kernel_is_bit_identical_to_the_two_pair_kernel(oracle, tmp_path):
    assert "VLR_REALIGN_SINGLE" not in os.environ   # this process runs vlr_realign_kernel2
    batches = rc.kernel_pair_batches()
    names = sorted(batches)
    two = np.concatenate([realign.prob_related(*batches[n]) for n in names])
    assert realign.last_pairs_per_wave() == 2
    out = str(tmp_path / "single.npy")
    env = dict(os.environ, VLR_REALIGN_SINGLE="1", PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "realign_cases.py"), out], env=env, cwd=ROOT, check=True, timeout=120)
    one = np.load(out)
    assert one[-1] == 1.0, "the child process did not launch vlr_realign_kernel"
    one = one[:-1]
    assert one.shape == two.shape and len(two) == 2 * 402 + 200 + 15
    assert not np.isnan(two).any()
    assert one.tobytes() == two.tobytes(), np.nonzero(~((one == two) | (np.isneginf(one) & np.isneginf(two))))[0][:20].tolist()
    # and both are right
    ref = np.concatenate([ref_pairhmm(oracle, *batches[n]) for n in names])
    agree(two, ref, what="two pairs per wave")


# ---- 3. exhaustive small shapes --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gap", [GapParams(), rc.EXT_GAP], ids=["default_gap", "gap_extension"])
@pytest.mark.parametrize("band", [-1, 0, 1])
def test_small_shapes_pair_hmm(oracle, band, gap):
    pb = rc.small_shapes(band)
    assert len(pb) == 1860
    agree(realign.prob_related(pb, gap), ref_pairhmm(oracle, pb, gap), what="small shapes band %d" % band)


@pytest.mark.parametrize("band", [-1, 1])
def test_small_shapes_homopolymer(oracle, band):
    pb = rc.small_shapes(band)
    agree(realign.prob_related_homopolymer(pb, rc.EXT_GAP, rc.SMALL_HOP), ref_homopoly(oracle, pb, rc.EXT_GAP, rc.SMALL_HOP), what="small shapes homopolymer band %d" % band)


@pytest.mark.parametrize("gap", [GapParams(), rc.EXT_GAP], ids=["default_gap", "gap_extension"])
def test_small_shapes_fast_mode(oracle, gap):
    pb = rc.small_shapes()
    agree(realign.prob_best_path(pb, gap), ref_fast(oracle, pb, gap), rel=1.0, what="small shapes fast")


def _check_edit(oracle, pb):
    dist, end, hits = realign.best_hits(pb)
    for k in range(len(pb)):
        assert (int(dist[k]), int(end[k]), int(hits[k])) == oracle.edit_distance(pb.x[k], pb.y[k]), (k, pb.x[k], pb.y[k])


def test_small_shapes_edit_distance(oracle):
    _check_edit(oracle, rc.small_shapes())


# ---- 4. wave geometry ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("band", [-1, 4, 9])
def test_wave_geometry_summing_kernels(oracle, band):
    pb = rc.wave_geometry(band)
    agree(realign.prob_related(pb), ref_pairhmm(oracle, pb, GapParams()), what="geometry band %d" % band)
    agree(realign.prob_related(pb, rc.EXT_GAP), ref_pairhmm(oracle, pb, rc.EXT_GAP), what="geometry, gap extension, band %d" % band)
    agree(realign.prob_related_homopolymer(pb, GapParams(), rc.SMALL_HOP), ref_homopoly(oracle, pb, GapParams(), rc.SMALL_HOP), what="geometry homopolymer band %d" % band)


def test_wave_geometry_fast_mode_and_edit_distance(oracle):
    pb = rc.wave_geometry()
    agree(realign.prob_best_path(pb, rc.EXT_GAP), ref_fast(oracle, pb, rc.EXT_GAP), rel=1.0, what="geometry fast")
    _check_edit(oracle, pb)


# ---- 5. inputs and entries -------------------------------------------------------------------------------------------------

def test_quality_edges_n_bases_and_lower_case_in_all_three_modes(oracle):
    pb = rc.input_edges()
    for gap in (GapParams(), rc.EXT_GAP):
        agree(realign.prob_related(pb, gap), ref_pairhmm(oracle, pb, gap), what="input edges")
        agree(realign.prob_related_homopolymer(pb, gap, rc.SMALL_HOP), ref_homopoly(oracle, pb, gap, rc.SMALL_HOP), what="input edges homopolymer")
        agree(realign.prob_best_path(pb, gap), ref_fast(oracle, pb, gap), rel=1.0, what="input edges fast")


def test_device_resident_entries_equal_the_host_entries():
    import torch
    pb = rc.wave_geometry(9)
    dp = realign.DevicePairs(pb)
    hop = rc.SMALL_HOP
    for gap in (GapParams(), rc.EXT_GAP):
        got = dp.run_homopolymer(gap, hop).cpu().numpy()
        torch.cuda.synchronize()
        assert got.tobytes() == realign.prob_related_homopolymer(pb, gap, hop).tobytes()
        got = dp.run_fast(gap).cpu().numpy()
        torch.cuda.synchronize()
        assert got.tobytes() == realign.prob_best_path(pb, gap).tobytes()
        got = dp.run(gap).cpu().numpy()
        torch.cuda.synchronize()
        assert got.tobytes() == realign.prob_related(pb, gap).tobytes()


def test_gap_opens_that_sum_to_more_than_one_are_rejected_by_all_six_entries(oracle):
    from varlociraptor_amd import abi
    pb = PairBatch()
    pb.add(b"ACGTACGT", b"CGTA", [30] * 4)
    dp = realign.DevicePairs(pb)
    bad = GapParams(math.log(0.6), math.log(0.6), -math.inf, -math.inf)
    entries = [lambda g: realign.prob_related(pb, g), lambda g: realign.prob_best_path(pb, g), lambda g: realign.prob_related_homopolymer(pb, g, HopParams()),
               lambda g: dp.run(g), lambda g: dp.run_fast(g), lambda g: dp.run_homopolymer(g, HopParams())]
    for f in entries:
        with pytest.raises(engine.EngineError) as e:
            f(bad)
        assert e.value.code == abi.ERR_INVALID_ARGUMENT
    # a sum of exactly one stays legal: no match transition is left, the results equal the oracle's
    one = GapParams(math.log(0.5), math.log(0.5), math.log(0.2), math.log(0.3))
    wide = rc.input_edges()
    dw = realign.DevicePairs(wide)
    refs = [ref_pairhmm(oracle, wide, one), ref_fast(oracle, wide, one), ref_homopoly(oracle, wide, one, rc.SMALL_HOP)]
    host = [realign.prob_related(wide, one), realign.prob_best_path(wide, one), realign.prob_related_homopolymer(wide, one, rc.SMALL_HOP)]
    dev = [dw.run(one).cpu().numpy(), dw.run_fast(one).cpu().numpy(), dw.run_homopolymer(one, rc.SMALL_HOP).cpu().numpy()]
    for k, rel in enumerate((1e-3, 1.0, 1e-3)):
        agree(host[k], refs[k], rel=rel, what="gap opens summing to one, entry %d" % k)
        assert dev[k].tobytes() == host[k].tobytes()
