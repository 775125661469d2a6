"""bench.py --gpus N without a launcher: the parent spawns N ranks before anything touches the GPU and relays rank 0's line
(VERDICT r1 item 1 / ADVICE: `--gpus` used to be parsed and ignored).  Plumbing only: HSRLE_BENCH_DRYRUN=1 makes the ranks report and
leave before the first GPU call, so this runs on a CPU-only machine."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(HSRLE_BENCH_DRYRUN="1", **env)
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, env=e, capture_output=True, text=True, timeout=120)


def test_gpus_n_spawns_n_ranks_and_relays_rank0():
    r = _run(["--gpus", "2"])
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line == {"dryrun": True, "n_gpus": 2, "master": "127.0.0.1"}


def test_gpus_must_match_world_size():
    r = _run(["--gpus", "4"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29511")
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr and r.stdout.strip() == ""


def test_steps_must_be_positive():
    r = _run(["--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr and r.stdout.strip() == ""


def test_full_and_dump_outputs_are_options():
    r = _run(["--full", "--dump-outputs", "unused"])
    assert r.returncode == 0 and json.loads(r.stdout)["dryrun"] is True


def test_launcher_env_is_honoured():
    r = _run(["--gpus", "2"], WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT="29512")
    assert r.returncode == 0 and json.loads(r.stdout)["n_gpus"] == 2
