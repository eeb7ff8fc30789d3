"""The host side of detrending on channel shards: the IC_DETREND_SHARDS switch,
run_loop's opt-in, sharded._loop_kwargs, and the declared interface.  No GPU and
no library: the session layer is monkeypatched."""
import argparse
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("value,on", [(None, False), ("", False), ("0", False), ("1", True), ("yes", True)])
def test_switch_is_parsed(monkeypatch, value, on):
    from iterative_cleaner_amd import detrend
    if value is None:
        monkeypatch.delenv("IC_DETREND_SHARDS", raising=False)
    else:
        monkeypatch.setenv("IC_DETREND_SHARDS", value)
    assert detrend.shards_enabled() is on


def _patched(monkeypatch, world=2, rank=1):
    """run_loop under a pretended channel sharding; clean_cube_dist records its call."""
    from iterative_cleaner_amd import _native, cleaner, dist, sharded
    monkeypatch.setattr(dist, "channel_sharding", lambda: True)
    monkeypatch.setattr(dist, "rank_world", lambda: (rank, world, rank))

    def no_session(*a, **k):
        raise AssertionError("a session was made")
    monkeypatch.setattr(_native, "GpuSession", no_session)
    monkeypatch.setattr(_native, "ShardSession", no_session)
    monkeypatch.setattr(_native, "shard_layout", lambda nsub, nchan, w: ([(0, 256), (256, nchan)], [(0, 1), (1, nsub)]))
    calls = []

    def fake_dist(cube, w0, shift, global_shape, device, **kw):
        calls.append(dict(cube=cube, global_shape=global_shape, **kw))
        return {"n_iter": 0}
    monkeypatch.setattr(sharded, "clean_cube_dist", fake_dist)
    return cleaner, calls


ARGS = argparse.Namespace(max_iter=1, chanthresh=5.0, subintthresh=5.0, pulse_region=[0, 0, 1])


def _inputs(nchan=600):
    return np.zeros((3, nchan, 32), np.float32), np.ones((3, nchan), np.float32), np.zeros(nchan, np.int64)


def test_run_loop_still_refuses_without_the_switch(monkeypatch):
    cleaner, calls = _patched(monkeypatch)
    monkeypatch.delenv("IC_DETREND_SHARDS", raising=False)
    with pytest.raises(ValueError, match="channel sharding") as e:
        cleaner.run_loop(*_inputs(), ARGS, detrend=(1, 2))
    assert "is not available under channel sharding" in str(e.value)      # today's wording ...
    assert "IC_DETREND_SHARDS=1" in str(e.value) and "detrend_shards=True" in str(e.value)   # ... and the hint
    monkeypatch.setenv("IC_DETREND_SHARDS", "1")
    with pytest.raises(ValueError, match="channel sharding"):             # the keyword overrides the switch
        cleaner.run_loop(*_inputs(), ARGS, detrend=(1, 2), detrend_shards=False)
    assert calls == []


@pytest.mark.parametrize("how", ["env", "keyword"])
def test_run_loop_hands_the_opt_in_on(monkeypatch, how):
    """detrend, the pieces resolved on the whole archive's lines (600 channels,
    not this rank's 344) and shard_detrend=True reach clean_cube_dist."""
    cleaner, calls = _patched(monkeypatch)
    kw = {}
    if how == "env":
        monkeypatch.setenv("IC_DETREND_SHARDS", "1")
    else:
        monkeypatch.delenv("IC_DETREND_SHARDS", raising=False)
        kw["detrend_shards"] = True
    cleaner.run_loop(*_inputs(), ARGS, detrend=(1, 2), detrend_pieces=(None, "w24"), **kw)
    call, = calls
    assert call["cube"].shape == (3, 344, 32) and call["global_shape"] == (3, 600, 32)
    assert call["shard_detrend"] is True and tuple(call["detrend"][:2]) == (1, 2)
    cb, sb = call["detrend_pieces"]
    assert cb is None and list(sb) == list(range(0, 600, 24))
    # a rank that was handed its slice only: the pieces are still the archive's
    calls.clear()
    cube, w0, shift = _inputs(344)
    cleaner.run_loop(cube, w0, shift, ARGS, detrend=(1, 2), detrend_pieces=(None, "w24"), nchan_total=600, **kw)
    assert list(calls[0]["detrend_pieces"][1]) == list(range(0, 600, 24))
    # undetrended: nothing new is passed
    calls.clear()
    cleaner.run_loop(*_inputs(), ARGS, **kw)
    assert not {"detrend", "detrend_pieces", "shard_detrend"} & set(calls[0])


def test_loop_kwargs_keeps_the_keywords():
    from iterative_cleaner_amd import sharded
    kw = sharded._loop_kwargs(dict(detrend=(1, 2), detrend_pieces=(None, "w24"), shard_detrend=True, max_iter=3),
                              (9, 1100))
    assert kw["detrend"] == (1, 2, 4, 5.0) and kw["shard_detrend"] is True and kw["max_iter"] == 3
    assert kw["detrend_pieces"] == (None, tuple(range(0, 1100, 24)))
    # resolved starts pass through unchanged (run_loop resolves before it calls)
    again = sharded._loop_kwargs(dict(detrend=(1, 2), detrend_pieces=kw["detrend_pieces"], shard_detrend=True),
                                 (9, 1100))
    assert again["detrend_pieces"] == kw["detrend_pieces"]
    plain = sharded._loop_kwargs(dict(max_iter=3))
    assert not {"detrend", "detrend_pieces", "shard_detrend"} & set(plain)
    with pytest.raises(ValueError, match="shard_detrend"):
        sharded._loop_kwargs(dict(detrend=(1, 2)), (9, 1100))
    with pytest.raises(ValueError, match="needs detrend"):
        sharded._loop_kwargs(dict(detrend_pieces=(None, "w24"), shard_detrend=True), (9, 1100))
    with pytest.raises(TypeError, match="no_such_keyword"):
        sharded._loop_kwargs(dict(no_such_keyword=1))
    assert sharded._loop_kwargs(dict(delay=np.zeros(4))) == plain | dict(max_iter=5)


def test_interface_is_declared():
    from iterative_cleaner_amd import _native
    header = open(os.path.join(REPO, "include", "iterative_cleaner.h")).read()
    assert re.search(r"\bint ic_shard_enable_detrend\(void \*session\);", header)
    assert "ic_shard_enable_detrend" in _native.EXPORTS
    assert re.search(r"#define\s+IC_ABI_VERSION\s+9\b", header) and _native.ABI_VERSION == 9
    doc = header.split("int ic_shard_enable_detrend(")[0].split("Detrended scaling on channel shards")[1]
    assert "EVERY rank" in doc and "exchange different sizes" in doc and "67 MB" in doc
    src = open(os.path.join(REPO, "iterative_cleaner_amd", "csrc", "ic_session.hip")).read()
    assert re.search(r"\bint ic_shard_enable_detrend\(void \*session\)\s*\{", src)
    import inspect
    assert "shard_detrend" in inspect.signature(_native.ShardSession.__init__).parameters
