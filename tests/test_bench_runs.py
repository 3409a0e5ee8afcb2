"""bench.py as a command: a plain run prints the headline line and nothing it does not need; --full adds the rest."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what only --full measures (config c3 with one GPU adds c5_layer and small_fits as well)
FULL_ONLY = ("time_to_converge", "cpu_baseline", "parity_full_size", "cpu_baseline_sparse")


def _bench(*extra):
    """One bench.py run on config tiny in a fresh process; its single JSON line."""
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", "12", "--warmup", "2", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _headline(j):
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline", "kernels", "elbo"):
        assert k in j, k
    assert j["steps"] == 12 and j["warmup"] == 2 and j["unit"] == "iter/s" and j["dtype"] == "f64" and j["higher_is_better"]
    assert j["value"] > 0 and abs(j["value"] * j["ms_per_step"] - 1e3) < 1e-6


@pytest.mark.gpu
def test_plain_run_is_the_headline_line_alone():
    j = _bench()
    _headline(j)
    assert not set(FULL_ONLY) & set(j), sorted(set(FULL_ONLY) & set(j))


@pytest.mark.gpu
def test_full_run_adds_the_baselines_and_the_parity():
    j = _bench("--full", "--cpu-seconds", "1")
    _headline(j)
    assert set(FULL_ONLY) <= set(j), sorted(set(FULL_ONLY) - set(j))
    assert j["time_to_converge"]["iterations"] >= 1
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_baseline_sparse"]["value"] > 0
    p = j["parity_full_size"]
    assert p["elbo_rel_err"] < 1e-10 and p["rho_max_abs"] < 1e-10, p
