"""Detrended scaling on channel shards as separate processes: two gloo ranks
sharing the box's one GPU run their shard sessions through dist.TorchComm
(tools/shard_check.py --detrend ... --detrend-shards), so the slots of detrended
row statistics cross a real process group, and the merged result must be
bit-identical to one unsharded detrended session.  The w24 pieces of the 600
channels straddle the shard edge at 256."""
import json
import os
import socket
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(world, extra, out_dir, timeout=240, pg_timeout=120):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), IC_PG_TIMEOUT=str(pg_timeout), PYTHONUNBUFFERED="1")
        cmd = [sys.executable, os.path.join(REPO, "tools", "shard_check.py"), "--backend", "gloo",
               "--out", str(out_dir), *extra]
        procs.append(subprocess.Popen(cmd, env=env, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                      text=True))
    t0 = time.time()
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=max(1.0, timeout - (time.time() - t0)))[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    recs = {}
    for r in range(world):
        path = os.path.join(str(out_dir), "rank%d.json" % r)
        if os.path.exists(path):
            with open(path) as f:
                recs[r] = json.loads(f.read())
    return [p.returncode for p in procs], recs, logs


def test_process_shards_match_one_detrended_session(tmp_path):
    rcs, recs, logs = _run_ranks(2, ["--shape", "8", "600", "128", "--detrend", "1,2", "--detrend-pieces", ";w24",
                                     "--detrend-shards"], tmp_path)
    assert rcs == [0, 0], "\n".join(logs)
    assert sorted(recs) == [0, 1]
    r0 = recs[0]
    assert r0["bit_identical"] and not r0["failed"], r0
    assert r0["detrend"][:2] == [1, 2] and r0["pieces"] == [1, 25], r0
    assert recs[1]["loops"] == r0["loops"] and recs[1]["zapped"] == r0["zapped"]
