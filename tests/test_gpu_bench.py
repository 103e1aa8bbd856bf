"""bench.py as a program on the GPU: a plain run measures only its timed steps, and --dump-outputs
writes what the last of them returned (one short run of the default config, shared by the tests)."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain_run(device, tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_dump")
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--warmup-seconds", "0.1", "--dump-outputs", str(d)], capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), d


def test_plain_run_reports_the_headline_fields_only(plain_run):
    import bench

    line, _ = plain_run
    assert line["metric"] == bench.METRIC and line["unit"] == "TFLOPS" and line["dtype"] == "fp16"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["full"] is False
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps
    assert line["value"] == pytest.approx(bench.flops(bench.CONFIGS["c2"]) / (line["ms_per_step"] * 1e-3) / 1e12,
                                          rel=1e-3)
    # what takes runs of its own is left to --full
    assert line["cpu_baseline"] is None and "kernel_ms_median" not in line["roofline"]


def test_dump_outputs_holds_the_sampled_rows_of_the_last_step(plain_run):
    import numpy as np

    import bench

    line, d = plain_run
    files = sorted(d.iterdir())
    assert [p.name for p in files] == ["out.npy"]
    assert sum(p.stat().st_size for p in files) <= 64_000_000
    a = np.load(files[0])
    c = bench.CONFIGS["c2"]
    keep = bench.DUMP_BYTES // 4 // c["D"]
    assert a.dtype == np.float32 and a.shape == (keep, c["D"]) and np.isfinite(a).all()
    assert line["outputs"]["out"] == {"shape": [c["B"], c["Hq"], c["Sq"], c["D"]], "rows_sampled": keep,
                                      "of": c["B"] * c["Hq"] * c["Sq"]}
    # non-causal attention over 4096 N(0,1) values: every output row is an average, well inside the inputs' range
    assert 0.0 < np.abs(a).max() < 1.0
