import os
import sys
from pathlib import Path

import pytest

# The oracle tests replay the reference's torch CPU arithmetic bit for bit against tests/golden/.  torch hands float32
# sqrt / cos / exp and its BLAS calls to MKL, whose automatic code path depends on the CPU model (an Intel AVX-512 host and
# an AMD EPYC host differ in the last bit); the fixtures are recorded on MKL's COMPATIBLE path (golden/make_goldens.py),
# which every x86 host runs.  MKL reads this when torch first calls into it, so it is set before any test imports torch.
os.environ["MKL_CBWR"] = "COMPATIBLE"

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

GOLDEN = Path(__file__).resolve().parent / "golden"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
