"""bench.py end to end on the small C1 workload: a plain run prints the headline
and nothing that takes runs of its own, ``--dump-outputs`` writes what a caller
of the timed path receives, the same from run to run, and ``--full`` still
carries the roofline, the other fit mode and the CPU baseline."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HEADLINE = {"metric": "profiles cleaned/sec (whole node)", "unit": "profiles/s", "higher_is_better": True,
            "dtype": "f64"}
FULL_ONLY = ("roofline", "fast_mode", "cpu_baseline")


def _bench(capsys, *args):
    import bench
    capsys.readouterr()
    bench.main(["--gpus", "1", "--workload", "C1", *args])
    lines = [line for line in capsys.readouterr().out.splitlines() if line.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _check_headline(rec, steps):
    import bench
    for k, v in HEADLINE.items():
        assert rec[k] == v, k
    assert rec["steps"] == steps and rec["n_gpus"] == 1
    nsub, nchan = bench.WORKLOADS["C1"][:2]
    assert rec["ms_per_step"] > 0
    # value and ms_per_step are one measurement; ms_per_step is rounded to 1 us (half of that off at most)
    ms = rec["ms_per_step"]
    assert rec["value"] == pytest.approx(nsub * nchan / (ms * 1e-3), rel=6e-4 / ms + 1e-6)


def test_plain_run_is_lean_and_dumps_what_a_caller_receives(capsys, tmp_path):
    import torch

    import bench
    from iterative_cleaner_amd import _native
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    rec = _bench(capsys, "--steps", "3", "--warmup", "1", "--dump-outputs", d1)
    _check_headline(rec, 3)
    for k in FULL_ONLY:
        assert k not in rec
    assert "per_rank" not in rec["config"] and "mask_flips_vs_exact" not in rec["config"]
    _bench(capsys, "--steps", "2", "--warmup", "0", "--dump-outputs", d2)

    names = sorted(os.listdir(d1))
    assert names == sorted(n + ".npy" for n in ("test", "test_nonfinite", "weights", "amp", "amp_nonfinite", "info",
                                                "template", "template_nonfinite", "loops", "changed", "nzero",
                                                "bad_fits"))
    assert sorted(os.listdir(d2)) == names
    total = 0
    dump = {}
    for n in names:
        arr = np.load(os.path.join(d1, n))
        assert arr.dtype in (np.float32, np.float64) and np.isfinite(arr).all(), n
        assert arr.tobytes() == np.load(os.path.join(d2, n)).tobytes(), n   # same inputs, same outputs
        total += os.path.getsize(os.path.join(d1, n))
        dump[n[:-4]] = arr
    assert total <= 64 * 10 ** 6

    # the same archive through a session of the caller's own
    nsub, nchan, nbin, seed, rfi = bench.WORKLOADS["C1"]
    cube, w0, shift = bench.make_cube_device(nsub, nchan, nbin, seed, rfi, torch.device("cuda", 0))
    with _native.GpuSession(nsub, nchan, nbin, max_iter=5, device=0) as s:
        torch.cuda.synchronize()
        s.upload_device(cube.data_ptr(), w0.data_ptr(), shift.data_ptr())
        out = s.run()
        amp, info = s.fit()
        template = s.template()
    def same(name, want):   # the finite values bit for bit, every other entry by its kind
        vals, code = bench.finite_pair(want.ravel())
        return dump[name].tobytes() == vals.tobytes() and np.array_equal(dump[name + "_nonfinite"], code)

    assert dump["weights"].tobytes() == out["weights"].ravel().tobytes()
    assert same("test", out["test"]) and same("amp", amp) and same("template", template)
    assert np.array_equal(dump["info"], info.ravel())
    assert dump["loops"].tolist() == [out["loops"], out["n_iter"], out["converged"]]
    for k in ("changed", "nzero", "bad_fits"):
        assert np.array_equal(dump[k], out[k]), k
    assert rec["config"]["loops"] == out["loops"] and rec["config"]["iterations"] == out["n_iter"]


def test_full_run_keeps_every_figure(capsys):
    rec = _bench(capsys, "--full", "--steps", "2", "--warmup", "1", "--cpu-budget", "0.2")
    _check_headline(rec, 2)
    for k in FULL_ONLY:
        assert k in rec, k
    roof = rec["roofline"]
    assert roof["kernel"] in roof["per_kernel"]
    assert rec["fast_mode"]["fit_mode"] == "closed" and rec["fast_mode"]["mask_flips_vs_exact"] >= 0
    assert rec["cpu_baseline"]["value"] > 0
