"""bench.py's command line and output dump, without a GPU: what is refused before anything starts, and the size
and sampling of --dump-outputs.  (The dump of a real run is checked in tests/test_gpu_dist.py.)"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_steps_must_be_positive():
    """ms_per_step = time / steps: a run without timed steps is refused"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 2 and b"--steps" in r.stderr


def _dump(n, d):
    code = ("import sys, numpy as np, bench\n"
            "n = int(sys.argv[1])\n"
            "a = np.arange(3 * n, dtype=np.float32).reshape(n, 3)\n"
            "bench.dump_outputs(sys.argv[2], a, a + 1, a + 2)\n"
            "print(bench.DUMP_MAX_BODIES)\n")
    r = subprocess.run([sys.executable, "-c", code, str(n), str(d)], cwd=ROOT, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return int(r.stdout.decode().split()[-1])


def test_dump_is_whole_below_the_cap(tmp_path):
    n = 1000
    _dump(n, tmp_path)
    assert sorted(os.listdir(tmp_path)) == ["acc.npy", "pos.npy", "vel.npy"]
    a = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    for k, off in (("pos", 0), ("vel", 1), ("acc", 2)):
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, a + off)


def test_dump_above_the_cap_is_a_fixed_sample_within_64_mb(tmp_path):
    """more bodies than the cap: the same seeded sample of rows every time, rows kept whole, at most 64 MB in all"""
    n = (1 << 20) + 4097
    cap = _dump(n, tmp_path / "a")
    assert _dump(n, tmp_path / "b") == cap and cap < n
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1000 * 1000
    for k, off in (("pos", 0), ("vel", 1), ("acc", 2)):
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert a.shape == (cap, 3) and a.dtype == np.float32 and np.array_equal(a, b)
        rows = (a[:, 0] - off).astype(np.int64) // 3          # row i of the input starts with 3 i (+ off)
        assert (np.diff(rows) > 0).all() and rows[-1] < n       # distinct bodies, ascending
        assert np.array_equal(a - off, np.stack([3 * rows, 3 * rows + 1, 3 * rows + 2], 1).astype(np.float32))
