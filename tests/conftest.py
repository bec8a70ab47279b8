import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
# The suite checks the pipeline as the package configures it: importing lsm_speech_classifier_amd sets
# GPU_MAX_HW_QUEUES (12 queues for the overlapped pipeline's streams) unless the environment already holds a value,
# which then wins.  A value inherited from the calling shell is dropped here, before any test imports the package or
# starts HIP; tests that need another count start a process of their own with it.
os.environ.pop("GPU_MAX_HW_QUEUES", None)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


@pytest.fixture(scope="session")
def oracle_c():
    """Plain-C oracle, built on demand (test infrastructure)."""
    from oracle import cport
    cport.build()
    return cport
