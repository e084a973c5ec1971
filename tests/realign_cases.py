"""Pair batches of the pair-HMM guard tests, built from fixed numpy seeds: tests/test_gpu_realign_guard.py runs them on the GPU,
tests/test_realign_cases_host.py checks on the CPU oracle that they are what they claim to be (unrelated pairs far below the range
of linear f64, planted pairs near ln 1).  Run as a program, this module evaluates one named batch with prob_related and writes the
result to an .npy file: the guard test starts it in a child process to reach the one-pair-per-wave kernel."""
from __future__ import annotations

import itertools
import math

import numpy as np

from varlociraptor_amd import realign_synth
from varlociraptor_amd.realign import GapParams, HopParams, PairBatch

B = np.frombuffer(b"ACGT", np.uint8)
EXT_GAP = GapParams(math.log(1e-4), math.log(2e-4), math.log(0.2), math.log(0.3))   # the extension set of tests/test_gpu_realign.py
GUARD_BAND = 100


def gap_list(gap: GapParams):
    return [gap.prob_insertion_artifact, gap.prob_deletion_artifact, gap.prob_insertion_extend_artifact, gap.prob_deletion_extend_artifact]


def hop_params(rng) -> HopParams:
    """Random hop parameters, as _hop() of tests/test_gpu_realign.py."""
    return HopParams([math.log(v) for v in rng.uniform(0.001, 0.05, 4)], [math.log(v) for v in rng.uniform(0.001, 0.05, 4)],
                     [math.log(v) for v in rng.uniform(0.05, 0.5, 4)], [math.log(v) for v in rng.uniform(0.05, 0.5, 4)])


def _bases(rng, n) -> bytes:
    return B[rng.integers(0, 4, n)].tobytes()


def _quals(rng, quals, n):
    return [int(quals[0])] * n if len(quals) == 1 else [int(q) for q in rng.choice(quals, n)]


def unrelated(rng, n, len_y=128, len_x=200, quals=(93,), pb=None) -> PairBatch:
    """Random reads against random alleles: the read is drawn first."""
    pb = pb if pb is not None else PairBatch()
    for _ in range(n):
        y = _bases(rng, len_y)
        x = _bases(rng, len_x)
        pb.add(x, y, _quals(rng, quals, len_y))
    return pb


def planted(rng, n, len_y=128, lead=300, tail=30, quals=(93,), pb=None) -> PairBatch:
    """An exact copy of the read behind `lead` unrelated bases: the lanes carry hundreds of columns of tiny lead-in cells before
    the bulk arrives."""
    pb = pb if pb is not None else PairBatch()
    for _ in range(n):
        y = _bases(rng, len_y)
        x = _bases(rng, lead) + y + _bases(rng, tail)
        pb.add(x, y, _quals(rng, quals, len_y))
    return pb


def banded(pb: PairBatch, max_edit_dist: int) -> PairBatch:
    out = PairBatch()
    for k in range(len(pb)):
        out.add(pb.x[k], pb.y[k], pb.q[k], max_edit_dist)
    return out


def guard_q93():
    """(400 unrelated, 400 planted) pairs of 128-base reads at Q93 from one generator seeded with 93."""
    rng = np.random.default_rng(93)
    return unrelated(rng, 400), planted(rng, 400)


# name -> (seed, read length, qualities, gap parameters); 100 unrelated pairs followed by 100 planted ones each
GUARD_SMALL = {
    "q41": (141, 128, (41,), GapParams()),
    "q60": (160, 128, (60,), GapParams()),
    "q80": (180, 128, (80,), GapParams()),
    "q93_len64": (164, 64, (93,), GapParams()),      # two pairs per wave
    "q93_len96": (196, 96, (93,), GapParams()),
    "mixed_quals": (102, 128, (2, 20, 41, 93), GapParams()),
    "gap_extension": (103, 128, (93,), EXT_GAP),
}


def guard_small(name):
    """(batch of 200, gap parameters, index of the first planted pair)."""
    seed, len_y, quals, gap = GUARD_SMALL[name]
    rng = np.random.default_rng(seed)
    pb = unrelated(rng, 100, len_y=len_y, quals=quals)
    planted(rng, 100, len_y=len_y, quals=quals, pb=pb)
    return pb, gap, 100


def guard_homopolymer():
    """(200 unrelated + 200 planted pairs at Q93 x 128 bases, hop parameters, index of the first planted pair)."""
    rng = np.random.default_rng(94)
    pb = unrelated(rng, 200)
    planted(rng, 200, pb=pb)
    return pb, hop_params(rng), 200


SMALL_QUALS = (2, 20, 40, 93)
SMALL_HOP = HopParams([math.log(v) for v in (0.03, 0.01, 0.02, 0.04)], [math.log(v) for v in (0.02, 0.05, 0.01, 0.03)],
                      [math.log(v) for v in (0.3, 0.1, 0.2, 0.4)], [math.log(v) for v in (0.15, 0.45, 0.25, 0.35)])


def small_shapes(max_edit_dist=-1) -> PairBatch:
    """Every allele over {A, C} of 1..5 bases against every read over {A, C} of 1..4 bases: 62 x 30 = 1860 pairs."""
    words = lambda n: [bytes(w) for k in range(1, n + 1) for w in itertools.product(b"AC", repeat=k)]
    pb = PairBatch()
    for x in words(5):
        for y in words(4):
            pb.add(x, y, [SMALL_QUALS[j % 4] for j in range(len(y))], max_edit_dist)
    return pb


GEOMETRY_LEN_Y = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128)
GEOMETRY_LEN_X = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193)


def wave_geometry(max_edit_dist=-1) -> PairBatch:
    """Every read length on a lane / half-wave edge against every allele length on an allele chunk edge (32 columns with two pairs
    per wave, 64 with one).  The shorter sequence is cut from the longer one and the read gets two substitutions.  Read-length-major
    order first — neighbours (2w, 2w+1) share the read length and differ in the allele length: short+short, long+long — then
    allele-length-major order, where neighbours differ in the read length: short+short, short+long (64 | 65), long+long."""
    rng = np.random.default_rng(44)
    order = [(lx, ly) for ly in GEOMETRY_LEN_Y for lx in GEOMETRY_LEN_X] + [(lx, ly) for lx in GEOMETRY_LEN_X for ly in GEOMETRY_LEN_Y]
    pb = PairBatch()
    for lx, ly in order:
        if ly <= lx:
            x = _bases(rng, lx)
            o = int(rng.integers(0, lx - ly + 1))
            y = bytearray(x[o:o + ly])
        else:
            y = bytearray(_bases(rng, ly))
            o = int(rng.integers(0, ly - lx + 1))
            x = bytes(y[o:o + lx])
        for _ in range(2):
            p = int(rng.integers(0, ly))
            y[p] = B[(int(np.searchsorted(B, y[p])) + 1 + int(rng.integers(0, 3))) % 4]
        pb.add(x, bytes(y), [int(q) for q in rng.choice([20, 30, 40], ly)], max_edit_dist)
    return pb


def input_edges() -> PairBatch:
    """Quality edges (at Q0 the match emission is 0 and the insertion emission 1), N bases and a lower-case read."""
    rng = np.random.default_rng(45)
    x = _bases(rng, 60)
    y = x[10:40]
    pb = PairBatch()
    for q in (0, 1, 2):
        pb.add(x, y, [q] * 30)
    pb.add(x, y, [0, 40] * 15)
    pb.add(x, y, [40, 0, 40] * 10)
    pb.add(x, y, [int(v) for v in rng.choice([0, 1, 2, 40, 93], 30)])
    pb.add(x, y[:7] + b"N" + y[8:], [30] * 30)                               # N in the read
    pb.add(x[:17] + b"N" + x[18:], y, [30] * 30)                             # N in the allele
    pb.add(x[:17] + b"N" + x[18:], y[:7] + b"N" + y[8:], [30] * 30)          # in both, at the same column
    pb.add(x[:17] + b"n" + x[18:], y[:7] + b"N" + y[8:], [30] * 30)
    pb.add(x, y.lower(), [30] * 30)                                          # a lower-case read
    pb.add(x.lower(), y[:12].lower() + y[12:], [0, 2, 30] * 10, 6)
    return pb


def short_long_neighbours() -> PairBatch:
    """The mixed short/long neighbour list of test_two_pairs_per_wave_on_short_read_windows (tests/test_gpu_realign.py)."""
    rng = np.random.default_rng(8)
    x = _bases(rng, 260)
    pb = PairBatch()
    for ly in (1, 2, 31, 32, 33, 63, 64, 65, 100, 128, 64, 5, 64, 64, 3):
        o = int(rng.integers(0, 100))
        pb.add(x, x[o:o + ly], [int(q) for q in rng.choice([20, 30, 40], ly)], int(rng.choice([-1, 4, 9])))
    return pb


def kernel_pair_batches():
    """name -> (batch, gap parameters): what the one-pair and the two-pair kernel must agree on bit for bit."""
    out = {}
    for band in (True, False):
        out["synth_banded" if band else "synth_unbanded"] = (realign_synth.generate(201, seed=17, window=24, banded=band)[0], GapParams())
    pb, gap, _ = guard_small("q93_len64")
    out["q93_len64"] = (pb, gap)
    out["short_long"] = (short_long_neighbours(), EXT_GAP)
    return out


if __name__ == "__main__":
    import sys

    from varlociraptor_amd import realign
    batches = kernel_pair_batches()
    names = sorted(batches)
    got = [realign.prob_related(*batches[n]) for n in names]
    np.save(sys.argv[1], np.concatenate(got + [np.array([float(realign.last_pairs_per_wave())])]))   # last element: which kernel ran
