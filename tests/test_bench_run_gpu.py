"""bench.py end to end on a small batch: a plain run prints the headline line and nothing else, `--dump-outputs` writes the
last timed step's outputs, and a `--full` run of the same arguments computes the same outputs and passes its parity checks."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout=600):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--files", "4", "--steps", "3", "--warmup", "1"] + args,
                         capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _outputs(d):
    return {n[:-4]: np.load(os.path.join(d, n)) for n in sorted(os.listdir(d))}


@pytest.mark.gpu
@pytest.mark.numeric_tolerance
def test_plain_run_and_its_outputs(gpu, tmp_path):
    plain = _run(["--dump-outputs", str(tmp_path / "plain")])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in plain, key
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0 and plain["higher_is_better"] is True
    assert plain["cpu_baseline"] is None and plain["parity"] == {} and "other_workloads" not in plain and "full_record" not in plain
    got = _outputs(tmp_path / "plain")
    assert set(got) == {"mp3", "vorbis", "flac"}
    assert got["mp3"].dtype == np.float32 and got["vorbis"].dtype == np.float32 and got["flac"].dtype == np.float64
    assert sum(a.nbytes for a in got.values()) <= 64 << 20 and all(a.size > 0 and np.isfinite(a).all() for a in got.values())
    assert np.array_equal(got["flac"], np.rint(got["flac"]))
    # every plane of this batch (4 MP3 / 4 Vorbis / 16 FLAC files: 21 / 20 / 42 M samples) is larger than its share of the
    # budget, so each dump is the seeded sample gathered on the device (index_select), as at full size
    plane = {k["codec"]: k["samples_per_launch"] for k in plain["roofline"]["kernels"]}
    for name, a in got.items():
        quota = (48 << 20) // 3 // a.itemsize
        assert plane[name] > quota and a.size == quota, (name, plane[name], a.size)

    full = _run(["--full", "--no-cpu-baseline", "--no-others", "--no-full-fetch", "--full-line", "--dump-outputs", str(tmp_path / "full")])
    assert set(full["parity"]) == {"mp3", "vorbis", "flac"} and all(p["mismatches"] == 0 for p in full["parity"].values())
    again = _outputs(tmp_path / "full")
    assert set(again) == set(got)
    for name in got:
        assert np.array_equal(got[name].view(np.uint8), again[name].view(np.uint8)), name
