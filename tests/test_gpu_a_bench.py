"""
bench.py as it is run: a plain run measures the headline alone and prints its line (and the dump of its outputs); --full
adds every other measurement and check.  Both at small sizes, each in a fresh child process.

The file sorts among the first GPU tests on purpose: the children start before this pytest process has made a HIP call
of its own (see test_gpu_a_ranks.py).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config",
            "whole_path")
FULL_ONLY = ("roofline", "kernels", "coded_line_fraction", "sensitivity", "f64_layout", "host_to_host", "configs",
             "configs4_share", "cpu_baseline", "speedup_vs_cpu_port")


def _bench(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


def test_options_without_a_gpu():
    """argument checks happen before anything is imported that needs a GPU"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--full" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--skip-extras"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(tmp_path):
    frames = 4096
    d = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--frames", str(frames), "--dump-outputs", str(tmp_path)],
               timeout=300)
    for k in HEADLINE:
        assert k in d, k
    assert not [k for k in FULL_ONLY if k in d]
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["frames_per_gpu_per_step"] == frames
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - frames * 1024 / (d["ms_per_step"] * 1e-3) / 1e6) <= 1e-2 * d["value"]
    idx = np.load(os.path.join(str(tmp_path), "frame_index.npy"))
    assert np.array_equal(idx, np.arange(frames, dtype=np.float64))           # (fewer frames than the sample: all of them)
    for k in ("overall_scale", "scale_factor", "bit_alloc", "mantissa", "reservoir_out"):
        assert np.load(os.path.join(str(tmp_path), k + ".npy")).shape[0] == frames


@pytest.mark.gpu
def test_full_run_keeps_every_measurement():
    d = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--frames", "8192", "--extra-frames", "4096",
                "--h2h-frames", "8192", "--c4-frames", "8192", "--single-hops", "1024", "--cpu-frames", "8"], timeout=600)
    for k in HEADLINE + FULL_ONLY:
        assert k in d, k
    assert set(d["configs"]) == {"stereo_ms", "block_switching", "stream_mode", "single_stream"}
    assert [r["name"] for r in d["kernels"]] == ["mdct_long_kernel", "smr_kernel", "bitalloc_kernel", "quantize_kernel"]
    assert d["host_to_host"]["equals_resident_result"] is True
    assert d["configs"]["single_stream"]["host_to_host"]["bytes_equal_resident"] is True
    assert d["configs"]["single_stream"]["before_per_block_loop"]["bytes_equal_chained_call"] is True
