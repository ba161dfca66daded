import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture
def golden_threads():
    """8 intra-op CPU threads for the duration of a test.  The fp32 golden values were recorded with the work split over >= 8
    threads; fewer threads reorder the CPU convolutions' weight / bias gradient reductions, which moves ill-conditioned entries
    past the fixtures' tolerances (1 - 4 threads) on the same host."""
    import torch

    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="session")
def golden():
    import torch

    cache = {}

    def load(name):
        if name not in cache:
            cache[name] = torch.load(os.path.join(GOLDEN, name), weights_only=True)
        return cache[name]

    return load
