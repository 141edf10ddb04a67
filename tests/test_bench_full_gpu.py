"""GPU: bench.py at two decoder layers.  A plain run prints the headline line and measures nothing beside it; --full adds the keys of the
measurements that take runs of their own, on the same timed region, inputs and dumped outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config", "roofline", "host")
EXTRA_KEYS = ("roofline_linear_eps_smallm", "config5_seq4096", "mode_explicit", "batch4", "batch1", "config4_gemma3_4b_text",
              "config4_gemma3_4b_image_text", "dropin_monkey_patch", "cpu_baseline")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--layers", "2"]
                       + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_alone_and_full_adds_the_rest(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    for key in HEADLINE:
        assert key in plain, key
    assert [k for k in EXTRA_KEYS if k in plain] == []
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["steps"] == 2 and plain["warmup"] == 1
    assert abs(plain["value"] - 4 * 1e3 / plain["ms_per_step"]) <= 1e-6 * plain["value"]
    assert plain["roofline"]["launches"] > 0 and 0.0 < plain["roofline"]["frac"] < 1.0
    # --full at this depth: the small-M tables (the probes of the 32-layer models need the full depth; the CPU baseline is dropped by its
    # own option, which goes on working under --full)
    full = _bench("--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert "roofline_linear_eps_smallm" in full and "cpu_baseline" not in full
    assert set(plain) == set(full) - {"roofline_linear_eps_smallm"}
    for key in ("metric", "unit", "higher_is_better", "dtype", "n_gpus", "steps", "warmup", "config"):
        assert plain[key] == full[key], key
    for name in ("R_tok", "idx", "logit", "logits"):
        assert np.array_equal(np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")), name
