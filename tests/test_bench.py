"""bench.py's two kinds of run on one GPU: a plain run prints the headline and what it is computed from, nothing
that takes a run of its own; --full adds the end-to-end PAF figures and the CPU baseline with its parity check."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("paf_end_to_end", "paf_end_to_end_mash", "paf_lines_per_s", "cpu_baseline", "cpu_baseline_t1", "parity")


def bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0",
                                   "--pairs", "512"] + list(args), env=env, timeout=300)
    return json.loads([ln for ln in out.decode().splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_only(hip_lib):
    line = bench()
    for k in HEADLINE:
        assert k in line, k
    assert line["unit"] == "bp/s" and line["higher_is_better"] is True and line["value"] > 0
    assert line["pairs_per_step"] == 512 and line["steps"] == 1 and line["warmup"] == 0
    assert "roofline" in line
    for k in FULL_ONLY:
        assert k not in line, k


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline_and_parity(hip_lib, oracle):
    line = bench("--full", "--no-paf", "--cpu-seconds", "0.5")
    for k in HEADLINE:
        assert k in line, k
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline_t1"]["value"] > 0
    assert line["parity"]["pairs"] > 0 and line["parity"]["mismatches"] == 0
    assert "paf_end_to_end" not in line
