import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a ROCm GPU (MI355X) and the built libpbn_env.so")


@pytest.fixture(scope="session")
def reference_files():
    """The reference's own data files the suite reads, stored verbatim under tests/golden/:
    kaban/<name>.ispl (the four network definitions) and pbn7_bdq_final.pt (models/pbn7/bdq_final.pt)."""
    return GOLDEN
