"""Host side of the batch scheduler's residuals, no device needed: the two
entry points are declared and bound, the ABI version stays, and pipeline /
run_lanes check their residual slots and keep results in input order, on
stand-in sessions that record the protocol (queue after run, wait before the
hand-over, one download in flight per session)."""
import os
import random
import re
import threading
import time

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 3, 8)


def test_declarations():
    from iterative_cleaner_amd import _native
    with open(os.path.join(REPO, "include", "iterative_cleaner.h")) as fh:
        text = fh.read()
    for name in ("ic_get_residual_quantised_async", "ic_residual_wait"):
        assert re.search(r"\bint %s\(" % name, text) and name in _native.EXPORTS
    assert re.search(r"#define IC_ABI_VERSION 9\b", text) and _native.ABI_VERSION == 9
    assert hasattr(_native.GpuSession, "residual_quantised_async") and hasattr(_native.GpuSession, "residual_wait")


class FakeSession:
    """The upload / run / residual protocol of one session; the 'download'
    writes the archive's tag into the slot when it is waited for."""

    shape = SHAPE

    def __init__(self, no_iter=()):
        self.queue, self.ran, self.flying = [], [], []
        self.no_iter = set(no_iter)
        self.lock = threading.Lock()

    def upload_async(self, tag, *_):
        with self.lock:
            assert len(self.queue) < 2, "more than two uploads in flight"
            self.queue.append(tag)

    def run(self, fetch=True):
        with self.lock:
            tag = self.queue.pop(0)
        time.sleep(random.random() * 0.002)
        self.ran.append(tag)
        return {"tag": tag, "n_iter": 0 if tag in self.no_iter else 1}

    def residual_quantised_async(self, q, scl, offs):
        assert self.ran, "a residual before any run"
        assert len(self.flying) < 1, "two downloads in flight on one session"
        self.flying.append((self.ran[-1], q, scl, offs))

    def residual_wait(self):
        for tag, q, scl, offs in self.flying:
            q[...] = tag
            scl[...] = tag
            offs[...] = -tag
        self.flying = []


def _slots(n, dtype=">i2", shape=SHAPE):
    return [(np.zeros(shape, dtype), np.zeros(shape[:2], np.float32), np.zeros(shape[:2], np.float32))
            for _ in range(n)]


def _check(out):
    q, scl, offs = out["residual_q"]
    tag = out["tag"]
    assert np.all(q == tag) and np.all(scl == tag) and np.all(offs == -tag), tag


def test_pipeline_residuals_in_order_and_valid_when_yielded():
    from iterative_cleaner_amd import batch
    s = FakeSession(no_iter=(3, 4, 9))
    items = [(k, None, None) for k in range(12)]
    got = []
    for out in batch.pipeline(s, items, residuals=_slots(2)):
        got.append(out["tag"])
        if out["tag"] in s.no_iter:
            assert "residual_q" not in out        # no iteration: no residual (run_loop's rule)
        else:
            _check(out)                           # its download has landed, nothing has overwritten it
    assert got == list(range(12)) and not s.flying and not s.queue
    assert list(batch.pipeline(s, [], residuals=_slots(2))) == []


@pytest.mark.parametrize("lanes", [2, 3])
def test_run_lanes_residuals_in_order_and_valid_when_yielded(lanes):
    from iterative_cleaner_amd import batch
    random.seed(lanes)
    sessions = [FakeSession(no_iter=(5,)) for _ in range(lanes)]
    items = [(k, None, None) for k in range(31)]
    got = []
    for out in batch.run_lanes(sessions, items, residuals=[_slots(2) for _ in sessions]):
        got.append(out["tag"])
        if out["tag"] != 5:
            _check(out)
            time.sleep(0.001)                     # a slow consumer: the lanes must not run over its slot
            _check(out)
    assert got == list(range(31))
    assert sorted(t for s in sessions for t in s.ran) == list(range(31))


def test_argument_checks():
    from iterative_cleaner_amd import batch
    items = [(k, None, None) for k in range(3)]
    with pytest.raises(ValueError, match="at least 2"):
        list(batch.pipeline(FakeSession(), items, residuals=_slots(1)))
    with pytest.raises(ValueError, match="at least 2"):
        list(batch.run_lanes([FakeSession(), FakeSession()], items, residuals=[_slots(2), _slots(1)]))
    with pytest.raises(ValueError, match="per session"):
        list(batch.run_lanes([FakeSession(), FakeSession()], items, residuals=[_slots(2)]))
    with pytest.raises(ValueError, match="int16"):
        list(batch.pipeline(FakeSession(), items, residuals=_slots(2, np.float32)))
    with pytest.raises(ValueError, match="int16"):
        list(batch.pipeline(FakeSession(), items, residuals=_slots(2, shape=(2, 3, 9))))
    bad = _slots(2)
    bad[1] = (bad[1][0], bad[1][1].astype(np.float64), bad[1][2])
    with pytest.raises(ValueError, match="float32"):
        list(batch.pipeline(FakeSession(), items, residuals=bad))
    bad = _slots(2)
    bad[0] = (bad[0][0][:, :, ::2], bad[0][1], bad[0][2])            # not contiguous (and the wrong shape)
    with pytest.raises(ValueError):
        list(batch.pipeline(FakeSession(), items, residuals=bad))
    with pytest.raises(ValueError, match="triple"):
        list(batch.pipeline(FakeSession(), items, residuals=[bad[1][:2], bad[1][:2]]))
