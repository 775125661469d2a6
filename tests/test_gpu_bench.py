"""bench.py's plain run on the GPU: the headline line and nothing else, and --dump-outputs writing what the last timed decode handed its
caller -- which must be the synthetic input, regenerated here on the host by the oracle's generator."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("hsrle_bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path, oracle):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "HSRLE_FORCE_DIST")}
    dump = tmp_path / "out"
    r = subprocess.run([sys.executable, BENCH, "--size-gib", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    size = 1 << 30
    assert j["steps"] == 3 and j["warmup"] == 1 and j["n_gpus"] == 1
    assert j["unit"] == "GiB/s" and j["higher_is_better"] is True and j["dtype"] == "u8" and j["ms_per_step"] > 0
    assert abs(j["value"] - size / 2**30 / (j["ms_per_step"] * 1e-3)) <= 0.01 * j["value"]
    for k in ("bit_exact", "encode", "roofline", "cpu_baseline", "extras", "gather_ms"):
        assert k not in j, f"{k} belongs to --full"

    files = sorted(os.listdir(dump))
    assert files == ["decoded_mib_sums.npy", "decoded_sample.npy", "status.npy"]
    assert sum(os.path.getsize(dump / f) for f in files) <= 64 << 20
    arrays = {f[:-4]: np.load(dump / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert arrays["status"][0] == 0

    bench = _bench_module()
    src = oracle.synth(0, 1, 2, size)   # run-distributed(8), seed 2: the headline input of one GPU
    idx = np.sort(np.random.default_rng(0).integers(0, size, size=bench.DUMP_SAMPLE, dtype=np.int64))
    assert np.array_equal(arrays["decoded_sample"], src[idx].astype(np.float32))
    sums = src.reshape(-1, bench.DUMP_CHUNK).sum(axis=1, dtype=np.int64).astype(np.float64)
    assert np.array_equal(arrays["decoded_mib_sums"], sums)
