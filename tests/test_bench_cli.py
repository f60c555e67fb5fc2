"""bench.py's command line: --steps is the number of timed steps, a plain run prints the headline line only, and
--dump-outputs writes the logits of the last timed step (seeded inputs: two runs of one build write the same bytes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_float32_and_samples_rows_beyond_the_cap(tmp_path, monkeypatch):
    small = np.arange(12, dtype=np.float64).reshape(4, 3)
    bench.dump_outputs(str(tmp_path / "d"), "logits", small, np)
    got = np.load(tmp_path / "d" / "logits.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 10 * 3 * 4)      # room for 10 rows of 3 floats
    big = np.arange(100 * 3, dtype=np.float32).reshape(100, 3)
    bench.dump_outputs(str(tmp_path / "a"), "x", big, np)
    bench.dump_outputs(str(tmp_path / "b"), "x", big, np)
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.shape == (10, 3) and np.array_equal(a, b)             # a fixed sample, the same every time
    assert (np.diff(a[:, 0]) > 0).all() and np.isin(a, big).all()  # whole rows, in order


@pytest.mark.parametrize("bad", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_are_checked_before_any_work(bad):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_steps_logits(tmp_path):
    import vh_synth as S
    vithip = pytest.importorskip("vithip")
    cfg, B = S.CONFIGS["vit_tiny"], 4
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "vit_tiny", "--batch", str(B),
           "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "images/s" and line["higher_is_better"]
    assert line["dtype"] == "bf16" and line["value"] > 0
    assert line["ms_per_step"] == pytest.approx(B * 1e3 / line["value"], rel=1e-2)
    for extra in ("parity", "cpu_baseline", "fp16", "step_ms", "events_cost"):
        assert extra not in line
    got = np.load(tmp_path / "logits.npy")
    assert got.dtype == np.float32 and got.shape == (B, cfg["classes"])
    # the same seeds through the library directly: the dump is what the timed path computed
    ctx = vithip.VitContext(cfg, dtype=vithip.DTYPE_BF16, max_batch=B)
    ctx.init_weights_seeded(0)
    din = vithip.DeviceBuffer(B * cfg["image_size"] ** 2 * cfg["channels"] * 4)
    dout = vithip.DeviceBuffer(B * cfg["classes"] * 4)
    ctx.fill_input_seeded(1, B, din.ptr)
    ctx.forward_device(din.ptr, B, dout.ptr)
    want = dout.to_numpy(np.float32, (B, cfg["classes"]))
    din.free(); dout.free()
    ctx.close()
    assert np.array_equal(got, want)
