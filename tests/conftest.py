import os
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    # the GPU tests patch HuggingFace and torch.nn classes process-wide (lxt_amd.efficient.monkey_patch never un-patches, like the
    # reference's); the CPU tests expect those classes as shipped, so they run first
    items.sort(key=lambda item: item.get_closest_marker("gpu") is not None)


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
