import os
import sys

import pytest

# repo root importable without installation
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an AMD GPU (MI355X); excluded on CPU-only CI")


@pytest.hookimpl(tryfirst=True)
def pytest_runtest_setup(item):
    """A test without the gpu marker checks the CPU reference path (fp32, tiny
    models whose head sizes the HIP kernels do not serve) and must give the
    same verdict on a machine that has a GPU: hide the device from the test,
    from its fixtures of any scope, and from the processes it starts."""
    if "gpu" in item.keywords:
        return
    import torch

    mp = pytest.MonkeyPatch()
    mp.setattr(torch.cuda, "is_available", lambda: False)
    mp.setattr(torch.cuda, "device_count", lambda: 0)
    # an out-of-range ordinal leaves a child process with no visible device
    mp.setenv("HIP_VISIBLE_DEVICES", "-1")
    mp.setenv("CUDA_VISIBLE_DEVICES", "-1")
    item._cpu_only_patch = mp


@pytest.hookimpl(trylast=True)
def pytest_runtest_teardown(item):
    mp = getattr(item, "_cpu_only_patch", None)
    if mp is not None:
        mp.undo()
        del item._cpu_only_patch


def pytest_collection_modifyitems(config, items):
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU available")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)
