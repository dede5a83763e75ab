import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run on the GPU box via gpurun)")


def pytest_collection_modifyitems(session, config, items):
    # tests/test_gpu_0_rccl.py starts its ranks while this process has not opened the GPU; its name sorts it first among
    # the GPU modules only, and a CPU module before it (test_abi.py asks the library for a device count) opens the GPU on a
    # GPU machine -- so in a run of the whole suite it goes first (a stable sort: the rest keep their order)
    items.sort(key=lambda item: os.path.basename(str(item.fspath)) != "test_gpu_0_rccl.py")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN
