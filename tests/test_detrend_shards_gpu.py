"""Detrended scaling on channel shards (ic_shard_enable_detrend; shard_rowtrends,
k_unpack_rowtrends, k_combine_dt_sh, k_combine_pw_sh), in-process shards on
device 0.

The yardstick is one unsharded GpuSession with the same detrend /
detrend_pieces; tests/test_detrend_gpu.py and tests/test_detrend_pieces_gpu.py
pin that session to iterative_cleaner_amd/detrend.py bit for bit.  A sharded
run must give its loop results, weights, test values, diagnostics, template and
trend coefficients BIT FOR BIT (a NaN matches a NaN where NaN samples are
planted); no tolerance.  Two cases also push the sharded run's gathered
diagnostics through the written definition (tests/detrend_ref.combine,
tests/detrend_pieces_ref.combine), so the shard path is not checked against the
GPU alone.

The cubes carry a 3x bandpass slope across the band and a 1.5x gain drift over
the subints, so both directions have a trend; every case asserts that its
detrended test values differ from the undetrended sharded ones and that a
subint coefficient is non-zero, so it cannot pass by ignoring the trend.  (The
C oracle's first-iteration diagnostics of the 7 x 520 x 64 (seed 41), 3 x 1024 x
32 (42) and 4 x 1024 x 32 (44) cubes, put through detrend.py on the CPU before
the seeds were fixed: every subint line of every diagnostic has a non-zero
trend, and thousands of test values differ from the undetrended ones.)

On a library without ic_shard_enable_detrend every test here fails: the
keyword shard_detrend is unknown and clean_cube_local would drop detrend.
"""
import threading

import numpy as np
import pytest

import detrend_pieces_ref
import detrend_ref
from helpers import bits_equal, bits_equal_nan

pytestmark = pytest.mark.gpu

IC_EINVAL = -1
KEYS = ("weights", "test", "std", "mean", "ptp", "fft", "T", "trend_chan", "trend_subint")

_CUBES, _ONE, _PLAIN = {}, {}, {}


def _cube(shape, seed):
    """synth.make_cube under a bandpass slope (gain 3 at channel 0 falling to 1)
    and a gain drift (1 at subint 0 rising to 1.5); read-only."""
    from iterative_cleaner_amd import synth
    if (shape, seed) not in _CUBES:
        nsub, nchan, nbin = shape
        data, w0, shift = synth.make_cube(nsub, nchan, nbin, seed, 0.1)
        gain = np.linspace(3.0, 1.0, nchan)[None, :, None] * np.linspace(1.0, 1.5, nsub)[:, None, None]
        raw = np.ascontiguousarray((data[:, 0].astype(np.float64) * gain).astype(np.float32))
        for a in (raw, w0, shift):
            a.setflags(write=False)
        _CUBES[(shape, seed)] = (raw, w0, shift)
    return _CUBES[(shape, seed)]


def _single(raw, w0, shift, detrend, pieces=None, **kw):
    """The yardstick: one unsharded session, with its details and trends."""
    from iterative_cleaner_amd import _native
    with _native.GpuSession(*raw.shape, device=0, detrend=detrend, detrend_pieces=pieces, **kw) as s:
        s.upload(raw, w0, shift)
        out = s.run()
        out["std"], out["mean"], out["ptp"], out["fft"] = s.diagnostics()
        out["T"] = s.template()
        out["trend_chan"], out["trend_subint"] = s.trends()
    return out


def _one(shape, seed, detrend, pieces=None):
    key = (shape, seed, detrend, pieces)
    if key not in _ONE:
        _ONE[key] = _single(*_cube(shape, seed), detrend, pieces)
    return _ONE[key]


def _plain(shape, seed, world):
    """The undetrended sharded test values of a cube."""
    from iterative_cleaner_amd import sharded
    key = (shape, seed, world)
    if key not in _PLAIN:
        _PLAIN[key] = sharded.clean_cube_local(*_cube(shape, seed), world)["test"]
    return _PLAIN[key]


def _sharded(raw, w0, shift, world, detrend, pieces=None, **kw):
    from iterative_cleaner_amd import sharded
    return sharded.clean_cube_local(raw, w0, shift, world, want_details=True, detrend=detrend,
                                    detrend_pieces=pieces, shard_detrend=True, **kw)


def _same(out, one, what, eq=bits_equal):
    assert out["loops"] == one["loops"] and out["n_iter"] == one["n_iter"], what
    assert np.array_equal(out["changed"], one["changed"]) and np.array_equal(out["nzero"], one["nzero"]), what
    for key in KEYS:
        assert eq(out[key], one[key]), "%s: %s differs" % (what, key)


def _not_ignored(out, plain_test, what):
    assert not bits_equal_nan(out["test"], plain_test), "%s: the detrended test values are the undetrended ones" % what
    assert out["trend_subint"].any(), "%s: every subint coefficient is zero" % what


CASES = [
    # shape, seed, worlds, orders, pieces
    ((7, 520, 64), 41, (1, 2), (1, 2), None),              # shards of 1 and 2 super-blocks, rows 4 + 3; 1-rank group
    ((3, 1024, 32), 42, (4,), (2, 1), None),               # a rank that owns no rows; rows_pad padding
    ((9, 1100, 128), 43, (2, 4), (1, 2), (None, "w24")),   # 46 pieces; [240, 264) split between ranks
    ((9, 1100, 128), 43, (2, 4), (1, 2), ("2", "w24")),    # channel pieces over the subints as well
    ((4, 1024, 32), 44, (2,), (1, 1), (None, "w2")),       # the 512-piece cap: the largest slot per row
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%dx%d-%s" % (c[0] + (c[4],)))
def test_shards_match_the_unsharded_detrended_session(case):
    shape, seed, worlds, orders, pieces = case
    raw, w0, shift = _cube(shape, seed)
    one = _one(shape, seed, orders, pieces)
    if pieces is not None and pieces[1] == "w24":
        from iterative_cleaner_amd import _native
        edges = [c0 for w in worlds for c0, _ in _native.shard_layout(shape[0], shape[1], w)[0][1:]]
        assert edges and any(e % 24 for e in edges)    # a shard edge inside a piece: that piece is split between ranks
    for world in worlds:
        out = _sharded(raw, w0, shift, world, orders, pieces)
        _same(out, one, "world %d" % world)
        _not_ignored(out, _plain(shape, seed, world), "world %d" % world)
        assert out["trend_chan"].shape[1] == shape[1] and out["trend_subint"].shape[1] == shape[0]


def test_non_finite_samples_and_dead_lines_cross_the_exchange():
    """A NaN and an Inf sample (they poison the template, so every line holds a
    non-finite value: rule 1, a zero trend, NaN medians), a zero-weight channel
    and a constant channel, at world 2: NaN for NaN, and the zero coefficients
    arrive as they left."""
    shape, seed = (7, 520, 64), 45
    raw, w0, shift = (a.copy() for a in _cube(shape, seed))
    raw[1, 300, 10] = np.nan
    raw[4, 100, 50] = np.inf
    raw[:, 400, :] = 1.25
    w0[:, 17] = 0.0
    one = _single(raw, w0, shift, (1, 2), (None, "w24"))
    out = _sharded(raw, w0, shift, 2, (1, 2), (None, "w24"))
    _same(out, one, "world 2", eq=bits_equal_nan)
    assert np.isnan(one["test"]).any()
    # a diagnostic whose every row holds a non-finite valid value: zero trends throughout
    assert any(not one["trend_subint"][q].any() for q in range(4))


@pytest.mark.parametrize("opts,fit_tail", [({"rowstat_waves": 4}, None), ({"rowstat_minlen": 16384}, None),
                                           ({"tail_split": 1, "diag_fork": 2}, 1024), ({"diag_fork": 0}, 1024),
                                           ({"fork_delay": 0, "template_incr": 0}, 1024),
                                           ({"grid_cap": 1}, None), ({"grid_cap": 3}, 0)])
def test_row_forms_and_schedule_options(opts, fit_tail):
    """1100 channels >= rowstat_minlen 1024: eight waves per row by default; four,
    and one (rowstat_minlen above the row: 16384, the option's largest value),
    and the schedule options, give the default unsharded session's bits; under
    grid_cap 1 and 3 k_unpack_rowtrends (1656 entries) and k_combine_pw_sh take
    their grid-stride loops through several trips."""
    shape, seed, orders, pieces = (9, 1100, 128), 43, (1, 2), (None, "w24")
    out = _sharded(*_cube(shape, seed), 2, orders, pieces, options=opts, fit_tail=fit_tail)
    _same(out, _one(shape, seed, orders, pieces), str(opts))


@pytest.mark.parametrize("mode", ["delay", "closed", "f64"])
def test_other_modes(mode):
    """Fractional delays, the closed-form fit, and f64 data (ptp in f64), at
    6 x 1100 x 256, world 2."""
    from iterative_cleaner_amd import synth
    shape, seed, orders = (6, 1100, 256), 46, (1, 2)
    raw, w0, shift = _cube(shape, seed)
    kw = {}
    if mode == "delay":
        kw["delay"] = synth.fractional_delays(shift, shape[2])
        shift = np.zeros_like(shift)
    elif mode == "closed":
        kw["fit_mode"] = 1
    else:
        kw["data_f64"] = True
    one = _single(raw, w0, shift, orders, **kw)
    out = _sharded(raw, w0, shift, 2, orders, **kw)
    assert out["ptp"].dtype == (np.float64 if mode == "f64" else np.float32)
    _same(out, one, mode)
    assert out["trend_subint"].any()


@pytest.mark.parametrize("pieced", [False, True], ids=["whole", "pieces"])
def test_sharded_run_follows_the_written_definition(pieced):
    """The sharded run's gathered diagnostics through detrend.py and restated's
    scalers on the CPU reproduce its test values, weights and coefficients."""
    shape, seed, orders = (7, 520, 64), 41, (1, 2)
    raw, w0, shift = _cube(shape, seed)
    out = _sharded(raw, w0, shift, 2, orders, (None, "w24") if pieced else None)
    diags = (out["std"], out["mean"], out["ptp"], out["fft"])
    valid = np.asarray(w0) != 0
    if pieced:
        test, cc, sc = detrend_pieces_ref.combine(diags, valid, 5.0, 5.0, orders, None, list(range(0, 520, 24)))
    else:
        test, cc, sc, _ = detrend_ref.combine(diags, valid, 5.0, 5.0, orders)
    assert bits_equal_nan(out["test"], test)
    with np.errstate(invalid="ignore"):
        want_w = np.where(test >= 1.0, np.float32(0.0), np.asarray(w0, np.float32)).astype(np.float32)
    assert bits_equal(out["weights"], want_w)
    assert bits_equal_nan(out["trend_chan"], cc.reshape(out["trend_chan"].shape))
    assert bits_equal_nan(out["trend_subint"], sc) and sc.any()


def _group(raw, w0, shift, world, kw, between=None):
    """`world` in-process shard sessions with timing on: one run, or two with
    `between(session)` called on every session in between.  Returns per run
    (merged test, merged weights, loops, per-rank launch counts, per-rank
    trends or None)."""
    from iterative_cleaner_amd import _native
    nsub, nchan, nbin = raw.shape
    chans, _ = _native.shard_layout(nsub, nchan, world)
    runs = []
    with _native.ShardGroup(world) as group:
        sess = []
        try:
            for r in range(world):
                sess.append(_native.ShardSession(nsub, nchan, nbin, r, world, group=group, device=0, **kw))
            for n in range(2 if between else 1):
                res, errors = [None] * world, []

                def work(r):
                    try:
                        s = sess[r]
                        s.set_timing(True)
                        s.upload(raw[:, chans[r][0]:chans[r][1]], w0[:, chans[r][0]:chans[r][1]],
                                 np.asarray(shift)[chans[r][0]:chans[r][1]])
                        out = s.run()
                        out["launches"] = {k: v["launches"] for k, v in s.kernel_times().items()}
                        try:
                            out["trends"] = s.trends()
                        except _native.NativeError:
                            out["trends"] = None
                        res[r] = out
                    except Exception as e:  # noqa: BLE001 - re-raised below
                        errors.append(e)
                threads = [threading.Thread(target=work, args=(r,)) for r in range(world)]
                for t in threads:
                    t.start()
                for t in threads:
                    t.join()
                if errors:
                    raise errors[0]
                runs.append(dict(test=np.concatenate([o["test"] for o in res], axis=1),
                                 weights=np.concatenate([o["weights"] for o in res], axis=1),
                                 loops=res[0]["loops"], launches=[o["launches"] for o in res],
                                 trends=[o["trends"] for o in res]))
                if between and n == 0:
                    for s in sess:
                        between(s)
        finally:
            for s in sess:
                s.close()
    return runs


def test_off_is_off():
    """Shards that opted in with orders (0, 0) and shards that never did: the
    same bits and the same launch counts per kernel id, `exchange` and
    `k_shard_pack` included."""
    raw, w0, shift = _cube((7, 520, 64), 41)
    never, = _group(raw, w0, shift, 2, {})
    off, = _group(raw, w0, shift, 2, dict(shard_detrend=True, detrend=(0, 0)))
    assert bits_equal(never["test"], off["test"]) and bits_equal(never["weights"], off["weights"])
    assert never["loops"] == off["loops"]
    assert never["launches"] == off["launches"]
    assert all(l["exchange"] > 0 and l["k_shard_pack"] > 0 for l in never["launches"])
    assert off["trends"] == [None, None]
    on, = _group(raw, w0, shift, 2, dict(shard_detrend=True, detrend=(1, 2)))
    assert on["launches"] != never["launches"] and not bits_equal_nan(on["test"], never["test"])


def test_pieces_taken_back():
    """set_detrend_pieces(None, None) on every shard returns to the whole-line
    pair's bits (and the slots are sized anew)."""
    shape, seed, orders = (9, 1100, 128), 43, (1, 2)
    raw, w0, shift = _cube(shape, seed)
    first, second = _group(raw, w0, shift, 2, dict(shard_detrend=True, detrend=orders, detrend_pieces=(None, "w24")),
                           between=lambda s: s.set_detrend_pieces(None, None))
    pw, whole = _one(shape, seed, orders, (None, "w24")), _one(shape, seed, orders)
    for run, one in ((first, pw), (second, whole)):
        assert run["loops"] == one["loops"]
        assert bits_equal(run["test"], one["test"]) and bits_equal(run["weights"], one["weights"])
        assert bits_equal(np.concatenate([t[0] for t in run["trends"]], axis=1), one["trend_chan"])
        assert all(bits_equal(t[1], one["trend_subint"]) for t in run["trends"])
    assert not bits_equal(first["test"], second["test"])


def test_the_default_still_refuses():
    from iterative_cleaner_amd import _native, sharded
    with _native.ShardGroup(2) as g:
        sess = [_native.ShardSession(3, 512, 64, r, 2, group=g, device=0) for r in range(2)]
        try:
            for s in sess:
                with pytest.raises(_native.NativeError, match="rc=%d" % IC_EINVAL) as e:
                    s.set_detrend(1, 1)
                assert "ic_shard_enable_detrend" in str(e.value) and "not supported" in str(e.value)
                with pytest.raises(_native.NativeError, match="ic_shard_enable_detrend"):
                    s.set_detrend_pieces(None, [0, 16])
        finally:
            for s in sess:
                s.close()
    raw, w0, shift = _cube((7, 520, 64), 41)
    with pytest.raises(ValueError, match="shard_detrend"):
        sharded.clean_cube_local(raw, w0, shift, 2, detrend=(1, 2))
    with pytest.raises(TypeError, match="detrnd"):
        sharded.clean_cube_local(raw, w0, shift, 2, detrnd=(1, 2))


def test_subint_pieces_are_the_archives():
    """On a shard the subint starts are checked against the archive's nchan
    (1100), not the shard's (512 / 588); the channel starts against nsub."""
    from iterative_cleaner_amd import _native
    with _native.ShardGroup(2) as g:
        sess = [_native.ShardSession(9, 1100, 64, r, 2, group=g, device=0, shard_detrend=True) for r in range(2)]
        try:
            for s in sess:
                s.set_detrend_pieces(None, [0, 600, 1099])
                assert s.pieces == (1, 3)
                with pytest.raises(_native.NativeError, match="rc=%d" % IC_EINVAL):
                    s.set_detrend_pieces(None, [0, 1100])
                with pytest.raises(_native.NativeError, match="rc=%d" % IC_EINVAL):
                    s.set_detrend_pieces([0, 9], None)
        finally:
            for s in sess:
                s.close()
    with _native.GpuSession(9, 1100, 64, device=0) as s:      # unsharded: IC_OK and nothing else
        assert s.lib.ic_shard_enable_detrend(s.h) == 0


def _one_rank(make):
    """A one-rank shard session made by make(kw) with orders (1, 2) and w24
    pieces at 8 x 600 x 256 against the unsharded session."""
    shape, seed, orders, pieces = (8, 600, 256), 47, (1, 2), (None, "w24")
    raw, w0, shift = _cube(shape, seed)
    one = _one(shape, seed, orders, pieces)
    with make(dict(device=0, shard_detrend=True, detrend=orders, detrend_pieces=pieces)) as s:
        s.upload(raw, w0, shift)
        out = s.run()
        cc, sc = s.trends()
    assert out["loops"] == one["loops"] and np.array_equal(out["changed"], one["changed"])
    assert bits_equal(out["weights"], one["weights"]) and bits_equal(out["test"], one["test"])
    assert bits_equal(cc, one["trend_chan"]) and bits_equal(sc, one["trend_subint"]) and sc.any()


@pytest.mark.parametrize("backend", ["nccl", "gloo"])
def test_torch_comm_one_rank_shard_session(backend):
    """The slots come from the host's alloc during the first detrended run, not
    at create; every buffer is released on close."""
    import torch
    import torch.distributed as dist

    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd.dist import TorchComm
    dev = torch.device("cuda", 0)
    kw = dict(store=dist.HashStore(), rank=0, world_size=1)
    if backend == "nccl":
        kw["device_id"] = dev
    dist.init_process_group(backend, **kw)
    try:
        comm = TorchComm(dev)
        _one_rank(lambda skw: _native.ShardSession(8, 600, 256, 0, 1, comm=comm, **skw))
        assert comm.error is None
        assert len(comm.bufs) == 0
    finally:
        dist.destroy_process_group()


def test_native_rccl_one_rank_shard_session():
    import torch
    import torch.distributed as dist

    from iterative_cleaner_amd import _native
    from iterative_cleaner_amd.dist import share_rccl_id
    dist.init_process_group("nccl", store=dist.HashStore(), rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        rid = share_rccl_id()
        _one_rank(lambda skw: _native.ShardSession(8, 600, 256, 0, 1, rccl_id=rid, **skw))
    finally:
        dist.destroy_process_group()
