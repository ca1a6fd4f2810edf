"""bench.py without a GPU: the arguments it refuses and the files --dump-outputs writes (the GPU side of both is
tests/test_gpu_parity.py::test_plain_bench_run_is_lean_and_dumps_what_it_timed)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench


@pytest.mark.parametrize("args", [["--steps", "0"], ["--steps", "-1"], ["--warmup", "-1"]])
def test_steps_mean_timed_steps(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and not r.stdout.strip(), (r.returncode, r.stderr[-500:])


def test_dump_of_a_frame_within_the_limit_is_the_frame(tmp_path):
    frame = np.random.default_rng(1).standard_normal((27, 45, 4)).astype(np.float32)
    bench.dump_outputs(np, str(tmp_path / "out"), frame)
    assert sorted(os.listdir(tmp_path / "out")) == ["framebuffer.npy"]
    got = np.load(str(tmp_path / "out" / "framebuffer.npy"))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), frame.view(np.uint32))


def test_dump_of_a_big_frame_is_a_fixed_sample_within_the_limit(tmp_path):
    H, W = 2160, 3840                                        # 132 MB of float32 RGBA
    frame = np.arange(H * W * 4, dtype=np.float32).reshape(H, W, 4)
    for d in ("a", "b"):
        bench.dump_outputs(np, str(tmp_path / d), frame)
    names = ["framebuffer_sample.npy", "framebuffer_sample_index.npy"]
    assert sorted(os.listdir(tmp_path / "a")) == names
    total = sum(os.path.getsize(tmp_path / "a" / n) for n in names)
    assert total <= bench.DUMP_LIMIT_BYTES
    sample, index = (np.load(str(tmp_path / "a" / n)) for n in names)
    assert sample.dtype == np.float32 and index.dtype == np.float64 and sample.shape == (index.size, 4) and index.size > 100000
    assert (np.diff(index) > 0).all() and index[0] >= 0 and index[-1] < H * W
    assert np.array_equal(sample, frame.reshape(-1, 4)[index.astype(np.int64)])
    for n in names:                                          # same arguments, same sample
        assert np.array_equal(np.load(str(tmp_path / "a" / n)), np.load(str(tmp_path / "b" / n)))
