import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


class _Golden(dict):
    @property
    def files(self):
        return list(self)


def load_golden(name):
    """tests/golden/<name>.npz and its parts <name>.<key>.npz (large arrays stored apart so that no fixture file exceeds
    1 MiB) as one mapping with np.load's ``files``."""
    out = _Golden()
    for path in [os.path.join(GOLDEN, name + ".npz")] + sorted(glob.glob(os.path.join(GOLDEN, glob.escape(name) + ".*.npz"))):
        with np.load(path) as f:
            out.update({k: f[k] for k in f.files})
    return out
