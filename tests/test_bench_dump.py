"""CPU tests (no GPU) of bench.py's --dump-outputs writer: float32 / float64 arrays, at most 64 MB in all, and for a
frame too large to store whole a fixed pixel sample that is the same from run to run."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _total_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_whole_frame(tmp_path):
    bench = _bench()
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, size=(1080, 1920, 4), dtype=np.uint8)
    counters = np.array([448 * 1920 * 1080, 12345, 678, 9], dtype=np.int64)
    bench.dump_outputs(str(tmp_path), frame, counters)
    assert sorted(os.listdir(tmp_path)) == ["counters.npy", "frame.npy"]
    f, c = np.load(tmp_path / "frame.npy"), np.load(tmp_path / "counters.npy")
    assert f.dtype == np.float32 and (f == frame).all()
    assert c.dtype == np.float64 and (c == counters).all()
    assert _total_bytes(tmp_path) <= 64 << 20


def test_dump_sampled_frame(tmp_path):
    bench = _bench()
    H, W = 2160, 3840
    frame = (np.arange(H * W * 4, dtype=np.uint32) % 251).astype(np.uint8).reshape(H, W, 4)
    counters = np.zeros(4, dtype=np.int64)
    for tag in ("a", "b"):
        bench.dump_outputs(str(tmp_path / tag), frame, counters)
    a, b = tmp_path / "a", tmp_path / "b"
    assert sorted(os.listdir(a)) == ["counters.npy", "frame_sample.npy", "frame_sample_pixels.npy"]
    assert _total_bytes(a) <= 64 << 20
    pix, vals = np.load(a / "frame_sample_pixels.npy"), np.load(a / "frame_sample.npy")
    assert pix.dtype == np.float64 and vals.dtype == np.float32 and vals.shape == (pix.size, 4)
    ip = pix.astype(np.int64)
    assert (np.diff(ip) > 0).all() and ip[0] >= 0 and ip[-1] < H * W
    assert (vals == frame.reshape(-1, 4)[ip]).all()
    assert (np.load(b / "frame_sample_pixels.npy") == pix).all() and (np.load(b / "frame_sample.npy") == vals).all()
