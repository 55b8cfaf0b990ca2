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
    config.addinivalue_line("markers", "slow: full-size property test")


class _GoldenParts(dict):
    """A fixture kept as <stem>.part<i>.npz pieces (each under the 1 MiB limit of a committed file), read as one."""

    @property
    def files(self):
        return list(self)


def load_golden(name):
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        return np.load(path)
    parts = sorted(glob.glob(os.path.join(GOLDEN, name[:-len(".npz")] + ".part*.npz")))
    if not parts:
        raise FileNotFoundError(path)
    g = _GoldenParts()
    for p in parts:
        with np.load(p) as z:
            g.update((k, z[k]) for k in z.files)
    return g


@pytest.fixture(scope="session")
def golden():
    return load_golden
