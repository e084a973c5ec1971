"""Time the two kernels behind the consumers of a calls file against their numpy restatements: vlr_posterior_odds_keep
(`filter-calls posterior-odds`) and vlr_range_group_lse (`estimate mutational-burden`).

    python tools/calls_consumers_rate.py [--sizes 10000,100000,1000000,10000000] [--cpu-max 1000000] [--reps 5] [--out rate.json]

N entries, R = 100 ranges [t_j, inf) (the curve / table mode), G = 14 groups.  Two device figures per size: `kernel_ms`, the
kernels alone (device time between a hipEvent pair around the launches, vlr_callstats_last_kernel_ms; median over --reps calls),
and `device_call_ms`, the whole C ABI call with allocation, upload and copy back (median of --reps calls after one warm-up).  A
numpy figure is one call of the restatement (skipped above --cpu-max).  Rates: entries per second, and GB/s against the stream a
pass has to read once (20 bytes per entry for the burden reduction, which reads it in two passes; 17 bytes per allele for the odds
decision).  One JSON line per N and kernel, with the build id of the library.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from varlociraptor_amd import burden, engine, odds  # noqa: E402


def timed(f, reps, which):
    """(result, median call s, min call s, median kernel s) of `reps` calls after one warm-up (module load, first allocation)."""
    f()
    ts, ks = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
        ks.append(burden.last_kernel_ms()[which] * 1e-3)
    return out, float(np.median(ts)), min(ts), float(np.median(ks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000,10000000")
    ap.add_argument("--cpu-max", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out")
    a = ap.parse_args()
    engine.build()
    lo, hi = burden.ranges("curve")
    lines = []
    for n in (int(x) for x in a.sizes.split(",")):
        rng = np.random.default_rng(n)
        vaf = rng.random(n, dtype=np.float32).astype(np.float64)
        lp = -rng.exponential(8.0, n)
        grp = rng.integers(0, 14, n).astype(np.int32)
        got, med, best, ker = timed(lambda: burden.range_group_lse(vaf, lp, grp, lo, hi, 14, device=a.device), a.reps, 0)
        rec = {"kernel": "vlr_range_group_lse", "n": n, "ranges": 100, "groups": 14, "kernel_ms": 1e3 * ker, "kernel_entries_per_s": n / ker if ker else None,
               "kernel_GBps_of_20B_stream": 20.0 * n / ker / 1e9 if ker else None, "device_call_ms": 1e3 * med, "device_call_ms_min": 1e3 * best,
               "device_entries_per_s": n / med, "device_GBps_of_20B_stream": 20.0 * n / med / 1e9, "build_id": engine.build_id()}
        if n <= a.cpu_max:
            t0 = time.perf_counter()
            want = burden.range_group_lse(vaf, lp, grp, lo, hi, 14)
            dt = time.perf_counter() - t0
            fin = np.isfinite(want)
            rec.update({"numpy_ms": 1e3 * dt, "numpy_entries_per_s": n / dt, "numpy_GBps_of_20B_stream": 20.0 * n / dt / 1e9,
                        "max_abs_diff": float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0, "same_nonfinite": bool(np.array_equal(fin, np.isfinite(got)))})
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        lt, lo_ = -rng.exponential(3.0, n), -rng.exponential(3.0, n)
        va = rng.integers(0, 4, n).astype(np.uint8)
        got, med, best, ker = timed(lambda: odds.keep_bits(lt, lo_, va, 3, device=a.device), a.reps, 1)
        rec = {"kernel": "vlr_posterior_odds_keep", "n": n, "kernel_ms": 1e3 * ker, "kernel_entries_per_s": n / ker if ker else None,
               "kernel_GBps_of_17B_stream": 17.0 * n / ker / 1e9 if ker else None, "device_call_ms": 1e3 * med, "device_call_ms_min": 1e3 * best, "device_entries_per_s": n / med,
               "device_GBps_of_17B_stream": 17.0 * n / med / 1e9, "build_id": engine.build_id()}
        if n <= a.cpu_max:
            t0 = time.perf_counter()
            want = odds.keep_bits(lt, lo_, va, 3)
            dt = time.perf_counter() - t0
            rec.update({"numpy_ms": 1e3 * dt, "numpy_entries_per_s": n / dt, "numpy_GBps_of_17B_stream": 17.0 * n / dt / 1e9, "decisions_differing": int((got != want).sum())})
        lines.append(rec)
        print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for rec in lines:
                fh.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
