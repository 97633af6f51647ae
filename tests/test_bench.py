"""bench.py's own options: --dump-outputs (the last timed step's frames as .npy files) and --full (every side
measurement; a plain run times the steps and prints the line, nothing else)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import load_scene
from tests.util import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _frames(rng, f, h, w):
    return dict(depth=rng.random((f, h, w), dtype=np.float32), color=rng.random((f, h, w, 3), dtype=np.float32),
                normal=rng.random((f, h, w, 3), dtype=np.float32))


def test_dump_outputs_writes_whole_frames_below_the_limit(tmp_path):
    import bench
    fr = _frames(np.random.default_rng(1), 1, 36, 64)
    bench.dump_outputs(str(tmp_path / "out"), fr, 12345.0)
    for k, v in fr.items():
        got = np.load(tmp_path / "out" / f"{k}.npy")
        assert got.dtype == np.float32 and same_bits(got, v), k
    rays = np.load(tmp_path / "out" / "ray_count.npy")
    assert rays.dtype == np.float64 and rays.tolist() == [12345.0]
    assert not (tmp_path / "out" / "pixel_index.npy").exists()


def test_dump_outputs_samples_the_same_pixels_above_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 10**6)
    fr = _frames(np.random.default_rng(2), 2, 200, 300)      # 2 x 60 000 pixels x 28 bytes = 3.4 MB
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), fr, 7.0)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 2 * 10**6
    idx = np.load(tmp_path / "a" / "pixel_index.npy")
    assert idx.dtype == np.float64 and np.array_equal(idx, np.load(tmp_path / "b" / "pixel_index.npy"))
    assert np.all(np.diff(idx) > 0) and idx[-1] < 2 * 200 * 300
    flat = idx.astype(np.int64)
    for k, v in fr.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        assert got.dtype == np.float32 and same_bits(got, v.reshape(2 * 200 * 300, -1)[flat].reshape(got.shape)), k


def _bench(args, tmp_path, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=tmp_path, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(ca, tmp_path):
    """A plain run: the line's headline fields, none of the --full side measurements, and --dump-outputs bitwise the
    single-process render of the same scene (image order: the tile order of the timed steps must not matter)."""
    line = _bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--width", "256", "--height", "144",
                   "--dump-outputs", str(tmp_path / "out")], tmp_path)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["metric"] == "Mrays/sec (primary+secondary)" and line["unit"] == "Mrays/s" and line["higher_is_better"]
    assert line["dtype"] == "f32" and line["value"] > 0
    assert "cpu_baseline" not in line and line["config"]["kernel_ms_image_order"] is None
    for k in ("c4_strong", "two_steps_in_flight", "dense_64k_roofline", "c4_roofline", "first_launch_kernel_ms", "extras"):
        assert k not in line["config"], k
    s = load_scene(ca, "bunny", 256, 144)
    ds = ca.DeviceScene(s)
    ds.set_variant(ca.VAR_NO_REORDER)
    want = ds.render(bounces=5)
    ds.close()
    for k in ("depth", "color", "normal"):
        got = np.load(tmp_path / "out" / f"{k}.npy")
        assert got.dtype == np.float32 and got.shape == (1,) + want[k].shape, k
        assert same_bits(got[0], want[k]), k
    rays = np.load(tmp_path / "out" / "ray_count.npy")
    assert rays.tolist() == [float(want["ray_count"])] == [line["config"]["rays_per_step"]]


@pytest.mark.gpu
def test_full_run_keeps_the_side_measurements(ca, tmp_path):
    """--full brings back the image-order probe and the extras; the CPU baseline is left out here (it takes tens of
    seconds and is exercised by every --full run of the benchmark itself)."""
    line = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--width", "256", "--height", "144", "--full",
                   "--no-cpu-baseline"], tmp_path)
    assert line["steps"] == 2 and line["config"]["kernel_ms_image_order"] > 0
    assert "two_steps_in_flight" in line["config"] and "first_launch_kernel_ms" in line["config"]
    assert "extras" not in line["config"]
