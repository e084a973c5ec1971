"""Time the posterior grid of `estimate contamination`: vlr_contamination_posterior (HIP) against the numpy restatement.

    python tools/contamination_rate.py [--sizes 1000,10000,100000,1000000] [--cpu-max 100000] [--reps 5] [--out rate.json]

N observations with AFD lists of 20-120 entries spanning [0, 1] (sorted keys).  The device figure is the whole C ABI call: upload of
the lists, both kernels, the copy back and the host epilogue (median of --reps calls after one warm-up); the numpy figure is one
call of the restatement (skipped above --cpu-max).  One JSON line per N, with the build id of the library.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from varlociraptor_amd import contamination as ct, engine  # noqa: E402


def inputs(n, seed=1):
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 121, n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos = np.arange(off[-1]) - np.repeat(off[:-1], lens)           # index within the list
    lv = pos / np.repeat(lens - 1, lens).astype(np.float64)         # evenly spaced keys over [0, 1]
    lp = rng.normal(-2.0, 1.5, off[-1])
    mv = rng.uniform(0.02, 0.95, n)
    pd = np.log(rng.uniform(0.95, 1.0, n))
    return off, lv, lp, mv, pd, float(mv.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000,1000000")
    ap.add_argument("--cpu-max", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    engine.build()
    lines = []
    pr = ct.ln_prior((0.2, 100))
    for n in (int(x) for x in a.sizes.split(",")):
        off, lv, lp, mv, pd, mx = inputs(n)
        ct.posterior_grid(off, lv, lp, mv, pd, mx, pr, device=a.device)      # warm-up (module load, first allocation)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            g, gm = ct.posterior_grid(off, lv, lp, mv, pd, mx, pr, device=a.device)
            ts.append(time.perf_counter() - t0)
        rec = {"n_obs": n, "list_entries": int(off[-1]), "device_call_ms": 1e3 * float(np.median(ts)), "device_call_ms_min": 1e3 * min(ts),
               "interpolations": 404 * n, "build_id": engine.build_id()}
        if n <= a.cpu_max:
            t0 = time.perf_counter()
            w, wm = ct.posterior_grid(off, lv, lp, mv, pd, mx, pr, device="cpu")
            rec["numpy_ms"] = 1e3 * (time.perf_counter() - t0)
            fin = np.isfinite(w)
            rec["max_abs_diff_ln_joint"] = float(np.abs(g[fin] - w[fin]).max()) if fin.any() else 0.0
            rec["same_nonfinite"] = bool(np.array_equal(fin, np.isfinite(g)))
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        with open(a.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
