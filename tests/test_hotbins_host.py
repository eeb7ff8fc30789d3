"""The written definition of the hot-bin repair (hotbins.py) on hand-made
profiles, its argument and environment parsing, the refusals, the C-ABI surface
and the full-polarisation host patch.  No GPU."""
import os
import re

import numpy as np
import pytest

from helpers import bits_equal
from iterative_cleaner_amd import hotbins as hb

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _rp(x, w=1.0, o=0, start=0, length=0, thr=6.0, rounds=4):
    out, n, bins = hb.repair_profile(np.asarray(x, F), w, o, start, length, thr, rounds)
    return out.tolist(), n, bins.tolist()


# the profile of the rounds test, worked by hand: round 1 has m = 5.5, mad = 4,
# lim = 6 * 1.4826 * 4 = 35.6: only 1000; round 2 (11 live) m = 5, mad = 3, lim =
# 26.7: 35 (30 away); round 3 (10 live) m = 3.5, mad = 2.5: nothing
X12 = [35, 1000, 0, 7, 2, 7, 6, 1, 5, 6, 1, 1]


# ---------------------------------------------------------------- the definition

def test_rounds_one_against_four():
    out, n, bins = _rp(X12, rounds=1)
    assert (n, bins) == (1, [1])
    assert out[1] == 5.0 and out[0] == 35.0          # the survivors' median after the removal (odd count)
    out, n, bins = _rp(X12, rounds=4)
    assert (n, bins) == (2, [0, 1])
    assert out[:2] == [3.5, 3.5] and out[2:] == X12[2:]   # 10 survivors: the two middle ones, (2 + 5) * 0.5
    assert _rp(X12, rounds=2)[1:] == (2, [0, 1]) and _rp(X12, rounds=8)[1:] == (2, [0, 1])


def test_even_and_odd_counts_and_tied_medians():
    # odd |O| = 9: the middle one; the spike is replaced by the median of the other 8, (3 + 4) * 0.5
    out, n, bins = _rp([0, 1, 2, 3, 100, 4, 5, 6, 7], thr=5.0)
    assert (n, bins, out[4]) == (1, [4], 3.5)
    # even |O| = 8, the two middle values tied: m = 2, devs 2 2 1 0 0 1 98 1 -> mad = 1
    out, n, bins = _rp([0, 4, 1, 2, 2, 3, 100, 3], thr=5.0)
    assert (n, bins, out[6]) == (1, [6], 2.0)
    # f32 values whose mean is no f32: the fill is f32((a + b) * 0.5 in f64), round half even
    a, b = F(1.0), np.nextafter(F(1.0), F(2.0))
    x = [a, a, a, a, b, b, b, b, F(50.0), F(-50.0), a, b]
    out, n, bins = hb.repair_profile(np.array(x, F), 1.0, 0, 0, 0, 1e10, 4)
    assert n == 0                                     # mad = half an ulp, lim huge: nothing hot
    out, n, bins = hb.repair_profile(np.array(x, F), 1.0, 0, 0, 0, 1e3, 4)
    assert (n, bins.tolist()) == (2, [8, 9])
    mid = (np.float64(a) + np.float64(b)) * 0.5
    assert out[8] == F(mid) and out[8] == a           # the tie rounds to the even mantissa


def test_mad_zero_constant_profile():
    out, n, bins = _rp([2.5] * 16)
    assert (n, bins) == (0, []) and out == [2.5] * 16
    x = [2.5] * 16
    x[3] = 1e6                                        # mad is still 0: the rounds stop, nothing is touched
    out, n, bins = _rp(x)
    assert (n, out) == (0, [float(F(v)) for v in x])
    # signed zeros: -0.0 sorts before +0.0, the deviations are all +0.0
    out, n, _ = hb.repair_profile(np.array([0.0, -0.0] * 6, F), 1.0, 0, 0, 0, 3.0, 4)
    assert n == 0 and bits_equal(out, np.array([0.0, -0.0] * 6, F))


def test_nonfinite_samples():
    base = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 500, 13, 14, 15]
    # window = bins 4..7
    for bad in (np.nan, np.inf, -np.inf):
        x = list(base)
        x[9] = bad                                    # in O: the profile is skipped
        out, n, bins = hb.repair_profile(np.array(x, F), 1.0, 0, 4, 4, 5.0, 4)
        assert n == 0 and bins.size == 0 and bits_equal(out, np.array(x, F))
        x = list(base)
        x[5] = bad                                    # on-pulse: ignored
        out, n, bins = hb.repair_profile(np.array(x, F), 1.0, 0, 4, 4, 5.0, 4)
        assert (n, bins.tolist()) == (1, [12])
        assert bits_equal(out[5:6], np.array([bad], F)) and out[12] == 9.0   # median of 0-3, 8-11, 13-15


def test_cap_at_and_one_over():
    # |O| = 16, cap 4: the base spreads over -1..1, nothing natural is hot
    base = np.sin(0.7 * np.arange(16)).astype(F)
    x = base.copy()
    x[[1, 6, 9, 14]] = 100.0
    out, n, bins = hb.repair_profile(x, 1.0, 0, 0, 0, 4.0, 4)
    assert (n, bins.tolist()) == (4, [1, 6, 9, 14])
    live = np.delete(base, [1, 6, 9, 14]).astype(np.float64)
    assert np.all(out[[1, 6, 9, 14]] == F(np.median(live)))
    x[11] = -100.0                                    # five: one over
    out, n, bins = hb.repair_profile(x, 1.0, 0, 0, 0, 4.0, 4)
    assert n == -1 and bins.size == 0 and bits_equal(out, x)
    # |O| = 19 (window of 1): cap is 19 // 4 = 4 still
    x = np.sin(0.7 * np.arange(20)).astype(F)
    x[[1, 6, 9, 14]] = 100.0
    assert hb.repair_profile(x, 1.0, 0, 19, 1, 4.0, 4)[1] == 4
    x[11] = 100.0
    assert hb.repair_profile(x, 1.0, 0, 19, 1, 4.0, 4)[1] == -1


def test_windows_offsets_and_widening():
    assert hb.window(64, 10, 20) == (10, 10) and hb.window(64, 10, 20, True) == (9, 12)
    assert hb.window(64, 60, 4) == (60, 8) and hb.window(64, 0, 64) == (0, 0)      # wrapped; L = nbin mod nbin
    assert hb.window(64, 5, 5, True) == (5, 0)                                     # nothing stays nothing
    assert hb.window(64, 0, 63, True) == (63, 64)                                  # never beyond nbin
    on = hb.on_pulse(16, 0, 14, 4)
    assert np.nonzero(on)[0].tolist() == [0, 1, 14, 15]
    on = hb.on_pulse(16, 3, 14, 4)                    # stored bin j holds dedispersed bin j - 3
    assert np.nonzero(on)[0].tolist() == [1, 2, 3, 4]
    # a spike at stored bin 2 is on-pulse with offset 3 and off-pulse with offset 0
    x = np.sin(0.7 * np.arange(32)).astype(F)
    x[2] = 80.0
    assert hb.repair_profile(x, 1.0, 3, 30, 4, 4.0, 4)[1] == 0
    out, n, bins = hb.repair_profile(x, 1.0, 0, 30, 4, 4.0, 4)
    assert (n, bins.tolist()) == (1, [2])
    # widened: a spike one bin outside the window is protected
    x = np.sin(0.7 * np.arange(32)).astype(F)
    x[9] = 80.0
    assert hb.repair_profile(x, 1.0, 0, *hb.window(32, 10, 14), 4.0, 4)[1] == 1
    out, n, _ = hb.repair_profile(x, 1.0, 0, *hb.window(32, 10, 14, True), 4.0, 4)
    assert n == 0 and bits_equal(out, x)
    # the offsets of a cube
    o, widen = hb.profile_offsets(2, 3, 16, shift=[1, 17, -1])
    assert o.tolist() == [[1, 1, 15]] * 2 and widen is False
    o, widen = hb.profile_offsets(2, 3, 16, delay=[0.5, 1.5, -0.51])
    assert o.tolist() == [[0, 2, 15]] * 2 and widen is True                        # round half even
    o, widen = hb.profile_offsets(2, 2, 16, delay=[[2.4, 18.6], [2.6, -30.2]])
    assert o.tolist() == [[2, 3], [3, 2]] and widen is True
    o, widen = hb.profile_offsets(2, 2, 16, delay=[9.0, 9.0], input_dedispersed=True)
    assert o.tolist() == [[0, 0], [0, 0]] and widen is False


def test_zero_weight_and_on_pulse_spike():
    x = np.sin(0.7 * np.arange(32)).astype(F)
    x[20] = 90.0
    out, n, _ = hb.repair_profile(x, 0.0, 0, 0, 0, 4.0, 4)
    assert n == 0 and bits_equal(out, x)
    assert hb.repair_profile(x, 0.3, 0, 0, 0, 4.0, 4)[1] == 1
    out, n, _ = hb.repair_profile(x, 1.0, 0, 18, 5, 4.0, 4)          # the spike is on-pulse
    assert n == 0 and bits_equal(out, x)


def test_repair_cube_and_the_list():
    rng = np.random.default_rng(0)
    cube = rng.standard_normal((3, 4, 64)).astype(F)
    w0 = np.ones((3, 4), F)
    w0[2, 0] = 0
    shift = np.array([0, 1, 2, 70])
    cube[0, 1, 5] += 30
    cube[0, 1, 50] -= 30
    cube[1, 3, 7] += 30
    cube[2, 0, 9] += 30
    cube[2, 2, 10 + 2 + 3] += 30                      # on-pulse (window 10..20, shift 2)
    fixed, res = hb.repair_cube(cube, w0, (6.0, 10, 20), shift=shift)
    assert res["count"].tolist() == [[0, 2, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]]
    assert res["total"] == 3 and res["bins"].tolist() == [5, 50, 7]
    assert res["offsets"].tolist() == [0, 0, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3]
    changed = np.argwhere(fixed != cube).tolist()
    assert changed == [[0, 1, 5], [0, 1, 50], [1, 3, 7]]
    assert abs(fixed[0, 1, 5]) < 0.5 and fixed[0, 1, 5] == fixed[0, 1, 50]
    # shards of the channels merge back into the same result
    parts = [hb.repair_cube(cube[:, c0:c1], w0[:, c0:c1], (6.0, 10, 20), shift=shift[c0:c1])[1]
             for c0, c1 in ((0, 1), (1, 4))]
    merged = hb.merge_shards(parts)
    for key in ("count", "offsets", "bins"):
        assert bits_equal(merged[key], res[key]), key


# ---------------------------------------------------------------- arguments, environment, refusals

def test_normalise_and_env(monkeypatch):
    assert hb.normalise((3, 10, 20)) == (3.0, 10, 20, 4)
    assert hb.normalise([3.5, 10, 20, 2]) == (3.5, 10, 20, 2)
    assert hb.normalise(np.array([3.0, 1, 2, 8])) == (3.0, 1, 2, 8)
    for off in (False, 0, (), (0, 1, 2), (-1.0, 1, 2, 99)):
        assert hb.normalise(off) is None
    for bad in ((3, 1), (3, 1, 2, 3, 4), (3, 1.5, 2), (np.nan, 1, 2), (np.inf, 1, 2), (3, 1, 2, 0), (3, 1, 2, 9),
                (3, True, 2)):
        with pytest.raises(ValueError):
            hb.normalise(bad)
    monkeypatch.delenv("IC_HOTBINS", raising=False)
    assert hb.normalise(None) is None
    for text, want in (("", None), ("0", None), (" 4.5,10,20 ", (4.5, 10, 20, 4)), ("4,10,20,2", (4.0, 10, 20, 2)),
                       ("0,10,20", None), ("1e1, 3 ,7", (10.0, 3, 7, 4))):
        monkeypatch.setenv("IC_HOTBINS", text)
        assert hb.normalise(None) == want, text
    for text in ("4", "4,10", "4,10,20,2,1", "x,1,2", "4,1.5,2", "4,10,20,9", "nan,1,2"):
        monkeypatch.setenv("IC_HOTBINS", text)
        with pytest.raises(ValueError):
            hb.normalise(None)
    monkeypatch.setenv("IC_HOTBINS", "4,10,20")
    assert hb.normalise((2, 1, 2)) == (2.0, 1, 2, 4)              # an argument wins over the switch


def test_refusals():
    assert hb.check_window(64, 0, 56) == (0, 56)                   # 8 off-pulse bins: the fewest
    for nbin, a, b, widen in ((64, 0, 57, False), (64, 0, 55, True), (64, 64, 4, False), (64, -1, 4, False),
                              (64, 0, 65, False), (64, 0, -1, False), (8200, 0, 10, False), (7, 0, 0, False)):
        with pytest.raises(ValueError):
            hb.check_window(nbin, a, b, widen)
    with pytest.raises(ValueError, match="off-pulse"):
        hb.repair_profiles(np.zeros((1, 16), F), [1], None, 0, 3.0, 0, 9)
    with pytest.raises(ValueError, match="off-pulse"):
        hb.repair_cube(np.zeros((1, 2, 16), F), np.ones((1, 2), F), (3.0, 2, 9), delay=[0.0, 0.0])


def test_c_abi_surface():
    """The four calls are declared, exported by name in the binding, and the
    ABI version did not move."""
    from iterative_cleaner_amd import _native
    text = open(os.path.join(REPO, "include", "iterative_cleaner.h")).read()
    for name in ("ic_set_hotbins", "ic_get_hotbins", "ic_get_hotbin_list", "ic_hotbins_profiles"):
        assert re.search(r"\bint %s\(" % name, text) and name in _native.EXPORTS
    assert re.search(r"#define IC_ABI_VERSION 9\b", text) and _native.ABI_VERSION == 9
    for fn in ("run_loop", "clean"):
        import inspect

        from iterative_cleaner_amd import batch, cleaner, sharded
        assert "hotbins" in inspect.signature(getattr(cleaner, fn)).parameters
    for fn in (batch.pipeline, batch.run_lanes, batch.clean_batch, _native.GpuSession.__init__):
        assert "hotbins" in inspect.signature(fn).parameters
    assert "hotbins" in sharded._LOOP_KEYS
    assert sharded._loop_kwargs(dict(hotbins=(3, 1, 2)), (2, 4), 64)["hotbins"] == (3.0, 1, 2, 4)
    assert "hotbins" not in sharded._loop_kwargs(dict(hotbins=(0, 1, 2)), (2, 4), 64)


# ---------------------------------------------------------------- the torchrun merge

def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _merge_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from iterative_cleaner_amd import sharded
        from iterative_cleaner_amd.dist import TorchComm
        cube, w0, shift, chans = _shard_case()
        c0, c1 = chans[rank]
        _, res = hb.repair_cube(cube[:, c0:c1], w0[:, c0:c1], (6.0, 10, 20), shift=shift[c0:c1])
        nsub, nchan, nbin = cube.shape
        out = dict(loops=2, n_iter=2, converged=True, changed=np.array([3, 0]), nzero=np.array([3, 3]),
                   bad_fits=np.array([0, 0]), test=np.full((nsub, c1 - c0), 0.5), weights=w0[:, c0:c1].copy(),
                   hotbins=res)
        merged = sharded._merge_dist(out, None, chans, (nsub, nchan, nbin), TorchComm("cpu"), None, False)
        q.put((rank, {k: merged["hotbins"][k] for k in ("count", "total", "offsets", "bins")},
               merged["weights"]))
    finally:
        dist.destroy_process_group()


def _shard_case():
    rng = np.random.default_rng(8)
    cube = rng.standard_normal((3, 5, 64)).astype(F)
    w0 = np.ones((3, 5), F)
    shift = np.array([0, 1, 2, 3, 4])
    for s, c, b in ((0, 0, 3), (0, 4, 40), (1, 2, 50), (1, 2, 51), (2, 1, 0), (2, 3, 63)):
        cube[s, c, b] += 40
    return cube, w0, shift, [(0, 2), (2, 5)]           # unequal slices: the gather pads


def test_two_rank_merge_of_the_lists():
    """sharded._merge_dist over gloo, world 2: every rank ends with the whole
    archive's counts and list, equal to one unsharded repair."""
    import multiprocessing as mp
    cube, w0, shift, chans = _shard_case()
    _, want = hb.repair_cube(cube, w0, (6.0, 10, 20), shift=shift)
    assert want["total"] == 6
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_merge_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == [0, 1]
    for _, got, weights in res:
        for key in ("count", "offsets", "bins"):
            assert bits_equal(got[key], want[key]), key
        assert got["total"] == want["total"] and bits_equal(weights, w0)


# ---------------------------------------------------------------- the full-polarisation host patch

HOT = (5.0, 16, 28)


def _two_pol_archive(stored_dedispersed=False):
    """(archive, spiked profiles): 4 x 2 pol x 6 x 64, a pulse at phase 0.3 (bins
    17..21), spikes in three profiles that differ between the polarisations."""
    from iterative_cleaner_amd import synth
    from iterative_cleaner_amd.archive import Archive
    data, w0, shift = synth.make_cube(4, 6, 64, 7, 0.0, npol=2, dead_frac=0.0)
    hits = {(0, 1): [3, 40], (2, 5): [50], (3, 0): [0, 60, 63]}
    for (s, c), bins in hits.items():
        for j, b in enumerate(bins):
            data[s, 0, c, b] += 30.0 + j
            data[s, 1, c, b] -= 12.0
    ar = Archive(data, w0, shift, dedispersed=False, filename="two_pol.fits")
    if stored_dedispersed:
        ar.dedisperse()
    return ar, hits


def _loop_cube(ar):
    from iterative_cleaner_amd import cleaner
    d = ar.get_data()
    cube = (d[:, 0] + d[:, 1]).astype(F) if d.shape[1] > 1 else d[:, 0]
    if ar.get_dedispersed():
        cube = cleaner._to_dispersed(cube, ar.get_dm_shift())
    return np.ascontiguousarray(cube)


@pytest.mark.parametrize("stored_dedispersed", (False, True))
def test_full_polarisation_patch_through_psrfits(tmp_path, stored_dedispersed):
    """The stand-in archive saved as PSRFITS and loaded, patched at the hit list
    of its total-intensity cube: every polarisation's listed bins hold that
    polarisation's own median, nothing else moves, the archive is marked changed
    and the unloaded file holds the patched profiles re-quantised."""
    from iterative_cleaner_amd import archive_io, cleaner, psrfits
    ar0, hits = _two_pol_archive(stored_dedispersed)
    path = str(tmp_path / "two_pol.fits")
    ar0.unload(path)
    ar = archive_io.load(path)
    assert ar.get_quantised() is not None and ar.get_dedispersed() == stored_dedispersed
    shift = ar.get_dm_shift()
    before = ar.get_data()
    fixed, res = hb.repair_cube(_loop_cube(ar), ar.get_weights(), HOT, shift=shift)
    assert sorted(map(tuple, np.argwhere(res["count"] > 0).tolist())) == sorted(hits)
    assert res["total"] == 6
    cleaner._patch_hotbins(ar, res, HOT, shift, None, stored_dedispersed)
    assert ar.get_quantised() is None                         # changed: unload re-quantises
    after = ar.get_data()
    start, length = hb.window(64, HOT[1], HOT[2])
    touched = np.zeros(after.shape, bool)
    for (s, c), bins in hits.items():
        o = 0 if stored_dedispersed else int(shift[c])
        stored = [(b - int(shift[c])) % 64 for b in bins] if stored_dedispersed else bins
        live = ~hb.on_pulse(64, o, start, length)
        live[stored] = False
        for p in range(2):
            want = F(hb._median(before[s, p, c][live].astype(np.float64)))
            assert np.all(after[s, p, c][stored] == want), (s, p, c)
            touched[s, p, c, stored] = True
    assert bits_equal(after[~touched], before[~touched])
    assert np.abs(after[touched]).max() < 2.0 and np.abs(before[touched]).min() > 8.0
    # -p: the pscrunched archive, patched, is the cube the GPU repaired
    ar_p = archive_io.load(path)
    ar_p.pscrunch()
    cleaner._patch_hotbins(ar_p, res, HOT, shift, None, stored_dedispersed)
    assert bits_equal(_loop_cube(ar_p), fixed)
    # the round trip: the patched profiles come back re-quantised, within their own step
    out_path = str(tmp_path / "patched.fits")
    ar.unload(out_path)
    back = archive_io.load(out_path)
    q, scl, offs = psrfits.quantise(after)
    assert bits_equal(back.get_data(), psrfits.decode(q, scl, offs))
    step = scl[..., None]
    assert np.all(np.abs(back.get_data() - after) <= 0.5001 * step + 1e-6)
    assert np.abs(back.get_data()[touched]).max() < 2.0


def test_patch_pols_equals_the_archive_patch():
    from iterative_cleaner_amd import cleaner
    ar, hits = _two_pol_archive()
    shift = ar.get_dm_shift()
    data = ar.get_data()
    _, res = hb.repair_cube(_loop_cube(ar), ar.get_weights(), HOT, shift=shift)
    assert hb.patch_pols(data, res, HOT, shift=shift) == len(hits)
    cleaner._patch_hotbins(ar, res, HOT, shift, None, False)
    assert bits_equal(ar.get_data(), data)
