"""bench.py's two kinds of run: a plain run prints the headline figure of its timed steps and nothing that needs runs or checks of
its own; `--full` adds those legs.  Both time the same steps and leave the same results."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline")
LEGS = ("with_afd", "pcie_inclusive", "end_to_end", "cpu_baseline", "parity", "posterior_normalisation_max_err", "status_counts")
N_LOCI = 20000


def bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--loci", str(N_LOCI), "--steps", "2", "--warmup", "1"] + list(args),
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_legs(tmp_path):
    plain = bench("--dump-outputs", str(tmp_path / "plain"))
    full = bench("--full", "--cpu-loci", "200", "--dump-outputs", str(tmp_path / "full"))
    for k in HEADLINE:
        assert k in plain and k in full, k
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["roofline"]["kernel_ms"] > 0
    assert not [k for k in LEGS if k in plain]

    assert full["with_afd"]["value"] > 0
    assert full["pcie_inclusive"]["value"] > 0
    assert full["end_to_end"]["value"], full["end_to_end"]
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["tuned"]["value"] > 0
    assert full["parity"]["n_checked"] == 200 and full["parity"]["frac_within_1e-6"] == 1.0, full["parity"]
    assert full["posterior_normalisation_max_err"] < 1e-9
    assert sum(full["status_counts"].values()) == N_LOCI

    # the legs of --full run after the timed steps: both runs leave the same results
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and "ln_posterior.npy" in names
    for n in names:
        a, b = np.load(tmp_path / "plain" / n), np.load(tmp_path / "full" / n)
        assert len(a) == N_LOCI and np.array_equal(a, b), n
