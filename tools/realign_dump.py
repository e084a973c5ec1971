#!/usr/bin/env python
"""Results of the five kernels of csrc/vlr_realign.hip on every pair batch of tests/realign_cases.py, as one .npz: a change that must
not move a bit is checked by writing one file per engine build (VLR_LIB selects the library) and comparing them byte for byte.

  python tools/realign_dump.py OUT.npz            every batch x {exact, homopolymer, fast, edit distance / end / hit count}
  python tools/realign_dump.py --compare A B      A, B: .npz files or directories of .npy files (bench.py --dump-outputs);
                                                  prints one line per array, exit status 1 unless all are equal as bytes

Which pair-HMM kernel `exact` launches follows VLR_REALIGN_SINGLE, as everywhere."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def batches():
    """(name, batch, gap parameters, hop parameters)"""
    import realign_cases as rc
    from varlociraptor_amd.realign import GapParams
    gaps = (("default_gap", GapParams()), ("gap_extension", rc.EXT_GAP))
    for kind, pb in zip(("unrelated", "planted"), rc.guard_q93()):
        yield "guard_q93/%s/band-1" % kind, pb, GapParams(), rc.SMALL_HOP
        yield "guard_q93/%s/band%d" % (kind, rc.GUARD_BAND), rc.banded(pb, rc.GUARD_BAND), GapParams(), rc.SMALL_HOP
    for name in rc.GUARD_SMALL:
        pb, gap, _ = rc.guard_small(name)
        yield "guard_small/" + name, pb, gap, rc.SMALL_HOP
    pb, hop, _ = rc.guard_homopolymer()
    yield "guard_homopolymer/band-1", pb, GapParams(), hop
    yield "guard_homopolymer/band%d" % rc.GUARD_BAND, rc.banded(pb, rc.GUARD_BAND), GapParams(), hop
    for band in (-1, 0, 1):
        for gname, gap in gaps:
            yield "small_shapes/band%d/%s" % (band, gname), rc.small_shapes(band), gap, rc.SMALL_HOP
    for band in (-1, 4, 9):
        for gname, gap in gaps:
            yield "wave_geometry/band%d/%s" % (band, gname), rc.wave_geometry(band), gap, rc.SMALL_HOP
    for gname, gap in gaps:
        yield "input_edges/" + gname, rc.input_edges(), gap, rc.SMALL_HOP
    for name, (pb, gap) in sorted(rc.kernel_pair_batches().items()):
        yield "kernel_pair_batches/" + name, pb, gap, rc.SMALL_HOP


def dump(path):
    from varlociraptor_amd import realign
    out = {}
    for name, pb, gap, hop in batches():
        out[name + "/exact"] = realign.prob_related(pb, gap)
        out[name + "/homopolymer"] = realign.prob_related_homopolymer(pb, gap, hop)
        out[name + "/fast"] = realign.prob_best_path(pb, gap)
        out[name + "/edit_dist"], out[name + "/edit_end"], out[name + "/edit_hits"] = realign.best_hits(pb)
    out["pairs_per_wave"] = np.array([realign.last_pairs_per_wave()])
    np.savez(path, **out)
    print("%s: %d arrays, %d values, exact kernel: %d pair(s) per wave" % (path, len(out), sum(a.size for a in out.values()), out["pairs_per_wave"][0]))


def load(path):
    if os.path.isdir(path):
        return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path)) if f.endswith(".npy")}
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def compare(pa, pb, ignore=("pairs_per_wave",)):
    a, b = load(pa), load(pb)
    bad = sorted(set(a) ^ set(b))
    for k in bad:
        print("%-60s only in one" % k)
    for k in sorted(set(a) & set(b)):
        if k in ignore:
            continue
        same = a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
        print("%-60s %7d values  %s" % (k, a[k].size, "equal" if same else "DIFFERENT"))
        if not same:
            bad.append(k)
    print("%s vs %s: %s" % (pa, pb, "all arrays equal as bytes" if not bad else "%d arrays differ" % len(bad)))
    return 1 if bad or not a else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    dump(sys.argv[1])
