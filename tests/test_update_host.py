"""CPU tests of the host half of qfec_encode_update and qfec_update: every argument the calls refuse
is refused with QFEC_EINVAL and a cause in qfec_last_error, with null device pointers or pointers
that are never dereferenced, so the decision is made before a device is touched; and a call with no
groups, or a code with no parity rows, is done without one.  No kernel is launched here."""
import pytest

import quicknet_amd as qa

QFEC_EINVAL = -1
D, P, R, S = 64, 4096, 8192, 12288  # stand-ins for device pointers (never dereferenced)


def last_error():
    return qa.lib().qfec_last_error().decode()


# (first, count, part, parity, groups, block_size, pitch, accumulate) -> the cause named
ENCODE_UPDATE_REFUSED = [
    ((-1, 1, D, P, 1, 16, 16, 1), "first < 0"),
    ((0, 0, D, P, 1, 16, 16, 1), "count < 1"),
    ((0, -3, D, P, 1, 16, 16, 1), "count < 1"),
    ((0, 5, D, P, 1, 16, 16, 1), "first \\+ count > k"),
    ((3, 2, D, P, 1, 16, 16, 1), "first \\+ count > k"),
    ((4, 1, D, P, 1, 16, 16, 1), "first \\+ count > k"),
    ((2**31 - 1, 2**31 - 1, D, P, 1, 16, 16, 1), "first \\+ count > k"),
    ((0, 1, D, P, -1, 16, 16, 1), "groups < 0"),
    ((0, 1, D, P, 1, 0, 16, 1), "block_size < 1"),
    ((0, 1, D, P, 1, 32, 16, 1), "pitch < block_size"),
    ((0, 1, D, P, 1, 16, 16, 2), "accumulate"),
    ((0, 1, D, P, 1, 16, 16, -1), "accumulate"),
    ((0, 1, None, P, 1, 16, 16, 1), "null buffer"),
    ((0, 1, D, None, 1, 16, 16, 0), "null buffer"),
    ((0, 1, None, None, 1, 16, 16, 0), "null buffer"),
]


@pytest.mark.parametrize("args,why", ENCODE_UPDATE_REFUSED)
def test_encode_update_refuses_on_the_host(args, why):
    import re

    L = qa.lib()
    code = qa.Code.cauchy(4, 2)
    first, count, *rest = args
    assert L.qfec_encode_update(code._h, first, count, *rest, None) == QFEC_EINVAL
    assert "qfec_encode_update:" in last_error() and re.search(why, last_error()), last_error()


def test_encode_update_null_code():
    L = qa.lib()
    assert L.qfec_encode_update(None, 0, 1, D, P, 1, 16, 16, 1, None) == QFEC_EINVAL
    assert "qfec_encode_update:" in last_error() and "null code" in last_error()
    assert L.qfec_encode_update(None, 0, 1, None, None, 0, 16, 16, 1, None) == QFEC_EINVAL


# (shard, data, rows, parity, groups, block_size, pitch, invalid) -> the cause named
UPDATE_REFUSED = [
    ((S, D, R, P, -1, 16, 16, None), "groups < 0"),
    ((S, D, R, P, 1, 0, 16, None), "block_size < 1"),
    ((S, D, R, P, 1, -5, 16, None), "block_size < 1"),
    ((S, D, R, P, 1, 32, 16, None), "pitch < block_size"),
    ((None, D, R, P, 1, 16, 16, None), "null buffer"),
    ((S, D, None, P, 1, 16, 16, None), "null buffer"),
    ((S, D, R, None, 1, 16, 16, None), "null buffer"),
    ((None, None, None, None, 1, 16, 16, None), "null buffer"),
    ((S, None, None, P, 1, 16, 16, None), "null buffer"),  # d_data may be null, d_rows may not
]


@pytest.mark.parametrize("args,why", UPDATE_REFUSED)
def test_update_refuses_on_the_host(args, why):
    import re

    L = qa.lib()
    code = qa.Code.cauchy(4, 2)
    assert L.qfec_update(code._h, *args, None) == QFEC_EINVAL
    assert "qfec_update:" in last_error() and re.search(why, last_error()), last_error()


def test_update_null_code():
    L = qa.lib()
    assert L.qfec_update(None, S, D, R, P, 1, 16, 16, None, None) == QFEC_EINVAL
    assert "qfec_update:" in last_error() and "null code" in last_error()
    assert L.qfec_update(None, None, None, None, None, 0, 16, 16, None, None) == QFEC_EINVAL


@pytest.mark.parametrize("k,m", [(4, 2), (40, 8), (200, 55)])
def test_nothing_to_do_is_ok_without_a_device(k, m):
    """groups = 0: QFEC_OK with null buffers, for any shape the code constructor takes (there is no
    k + m limit on these calls)."""
    L = qa.lib()
    code = qa.Code.cauchy(k, m)
    assert L.qfec_encode_update(code._h, 0, k, None, None, 0, 16, 16, 0, None) == 0
    assert L.qfec_encode_update(code._h, k - 1, 1, None, None, 0, 16, 16, 1, None) == 0
    assert L.qfec_update(code._h, None, None, None, None, 0, 16, 16, None, None) == 0
    # a bad argument still loses to nothing-to-do
    assert L.qfec_encode_update(code._h, 0, k + 1, None, None, 0, 16, 16, 0, None) == QFEC_EINVAL
    assert L.qfec_update(code._h, None, None, None, None, 0, 32, 16, None, None) == QFEC_EINVAL


def test_no_parity_rows_is_ok_without_a_device():
    """m = 0 (a Vandermonde code may have none): QFEC_OK, nothing launched, no device looked for."""
    L = qa.lib()
    code = qa.Code.vandermonde(4, 0)
    assert L.qfec_encode_update(code._h, 0, 4, D, P, 3, 16, 16, 0, None) == 0
    assert L.qfec_update(code._h, S, D, R, P, 3, 16, 16, None, None) == 0


def test_python_face_checks_shapes_before_the_call():
    """Code.encode_update / Code.update refuse a host tensor and a wrong shape themselves."""
    import torch

    code = qa.Code.cauchy(4, 2)
    part = torch.zeros((2, 1, 16), dtype=torch.uint8)
    par = torch.zeros((2, 3, 16), dtype=torch.uint8)
    with pytest.raises(qa.QfecError, match="shape mismatch"):
        code.encode_update(part, par, 0)
    with pytest.raises(qa.QfecError, match="shape mismatch"):
        code.update(torch.zeros(3, dtype=torch.int32), torch.zeros((2, 16), dtype=torch.uint8),
                    torch.zeros((2, 2, 16), dtype=torch.uint8))
    with pytest.raises(qa.QfecError, match="expected a device tensor"):
        code.encode_update(part, torch.zeros((2, 2, 16), dtype=torch.uint8), 0)
    assert qa.QFEC_UPD_NONE == -1
