import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# before any test touches the HIP runtime: the package turns hipGraph packet capture off for the process
# (ouzelum_amd/__init__.py), which only takes effect if the runtime has not started yet
import ouzelum_amd  # noqa: E402,F401


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs through the HIP C-ABI)")


@pytest.fixture(scope="session")
def golden():
    from tests import golden_io
    d = os.path.join(ROOT, "tests", "golden")

    def load(name):   # a fixture too large for one committed file is stored in parts (tests/golden_io.py)
        return golden_io.load(os.path.join(d, name))
    return load
