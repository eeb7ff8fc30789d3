"""The committed chirp-z fixtures are what the reference produces today.

Regenerates the smallest one (``any_clean_s4x12x448_fft_ded``: fractional
delays at 448 bins, stored dedispersed) with ``tests/golden/make_golden_any.py``
and compares every array and the meta record with the committed file, as
tests/test_golden_regen.py does for the power-of-two fixtures.  Needs the
reference sources; skipped where they are absent (the GPU box).
"""
import json
import os
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/iterative_cleaner.py"

pytestmark = pytest.mark.skipif(not os.path.exists(REF), reason="reference sources absent (GPU box)")


def test_regenerated_smallest_any_case_matches_committed_fixture():
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden  # noqa: E402
    import make_golden_any  # noqa: E402

    ic = make_golden.import_reference()
    name = make_golden_any.SMALLEST
    committed = np.load(make_golden_any.fixture_path(name))
    with tempfile.TemporaryDirectory() as wd, tempfile.TemporaryDirectory() as out:
        make_golden_any.run_case(ic, name, wd, out)
        fresh = np.load(make_golden_any.fixture_path(name, out))
        assert set(fresh.files) == set(committed.files)
        for k in committed.files:
            a, b = committed[k], fresh[k]
            if k == "meta":
                assert json.loads(str(a)) == json.loads(str(b))
                continue
            assert a.dtype == b.dtype and a.shape == b.shape, k
            assert a.tobytes() == b.tobytes(), k


def test_every_committed_any_fixture_has_a_generator_case():
    import glob
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden_any  # noqa: E402
    have = sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, "golden", "any_clean_*.npz")))
    assert have == sorted("any_clean_%s.npz" % n for n in make_golden_any.CASES)
