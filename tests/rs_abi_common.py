"""Shared by the GPU tests of module/rs.h (test_gpu_rs_host.py, test_gpu_rs_ptrs.py,
test_gpu_rs_ptrs_wide.py, test_gpu_handle_edits.py): the knobs fixture, and shard arrays whose rows are
separate device allocations.  torch is imported inside the helpers that need it."""
import ctypes as C

import numpy as np
import pytest

import quicknet_amd as qa


@pytest.fixture
def knobs():
    """Set knobs for one test and put back what was there before (qfec_tune_get)."""
    saved = {}

    def set_(key, value):
        if key not in saved:
            saved[key] = qa.tune_get(key)
        qa.tune(key, value)

    yield set_
    for key, value in saved.items():
        qa.tune(key, value)


def device_rows(host_rows):
    """One torch tensor per row: separate allocations, so the array is not one contiguous batch."""
    import torch

    rows = [torch.from_numpy(np.ascontiguousarray(r)).to("cuda:0") for r in host_rows]
    B = len(host_rows[0])
    assert any(rows[i].data_ptr() != rows[0].data_ptr() + i * B for i in range(1, len(rows)))
    return rows


def ptr_array(rows):
    return (C.c_void_p * len(rows))(*[r.ctypes.data if isinstance(r, np.ndarray) else r.data_ptr() for r in rows])


def fetch(rows):
    import torch

    torch.cuda.synchronize()
    return np.stack([r.cpu().numpy() if not isinstance(r, np.ndarray) else r for r in rows])
