"""CPU tests of the host half of incremental parity on pointer tables: qfec_encode_update_ptrs,
qfec_update_ptrs, qfec_encode_update_ptrs_var and qfec_update_ptrs_var.  Every argument the calls refuse
is refused with QFEC_EINVAL and a cause after the call's name in qfec_last_error, with null device
pointers or pointers that are never dereferenced, so the decision is made before a device is touched;
a call with no groups, or a code with no parity rows, is done without one; and a bad argument wins
over nothing-to-do.  No kernel is launched here, and the calls add no host geometry of their own: the
launch is cut by ptrs_geom at 16-B lanes (tests/test_ptrs_host.py)."""
import re

import pytest

import quicknet_amd as qa

QFEC_EINVAL = -1
T, S, N, L, GL, NL = 64, 4096, 8192, 12288, 16384, 20480  # stand-ins for device pointers (never dereferenced)


def last_error():
    return qa.lib().qfec_last_error().decode()


def refused(name, rc, why):
    assert rc == QFEC_EINVAL
    err = last_error()
    assert err.startswith(name + ":") and re.search(why, err), err


RANGE_CAUSES = [((-1, 1), "first < 0"), ((0, 0), "count < 1"), ((0, -3), "count < 1"), ((0, 5), r"first \+ count > k"),
                ((3, 2), r"first \+ count > k"), ((4, 1), r"first \+ count > k"),
                ((2**31 - 1, 2**31 - 1), r"first \+ count > k")]

# (first, count, shards, groups, block_size, accumulate)
ENCODE_UPDATE_PTRS_REFUSED = [(fc + (T, 1, 16, 1), why) for fc, why in RANGE_CAUSES] + [
    ((0, 1, T, -1, 16, 1), "groups < 0"),
    ((0, 1, T, 1, 0, 1), "block_size < 1"),
    ((0, 1, T, 1, -7, 1), "block_size < 1"),
    ((0, 1, T, 1, 16, 2), "accumulate"),
    ((0, 1, T, 1, 16, -1), "accumulate"),
    ((0, 1, None, 1, 16, 0), "null d_shards"),
]


@pytest.mark.parametrize("args,why", ENCODE_UPDATE_PTRS_REFUSED)
def test_encode_update_ptrs_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(4, 2)
    first, count, *rest = args
    refused("qfec_encode_update_ptrs", qa.lib().qfec_encode_update_ptrs(code._h, first, count, *rest, None), why)


# (first, count, shards, lens, group_len, groups, max_len, accumulate, invalid)
ENCODE_UPDATE_PTRS_VAR_REFUSED = [(fc + (T, L, GL, 1, 16, 1, None), why) for fc, why in RANGE_CAUSES] + [
    ((0, 1, T, L, GL, -1, 16, 1, None), "groups < 0"),
    ((0, 1, T, L, GL, 1, 0, 1, None), "max_len < 1"),
    ((0, 1, T, L, GL, 1, 16, 3, None), "accumulate"),
    ((0, 1, None, L, GL, 1, 16, 0, None), "null d_shards"),
    ((0, 1, T, None, GL, 1, 16, 0, None), "null d_lens"),
    ((0, 1, T, L, None, 1, 16, 0, None), "null d_group_len"),
]


@pytest.mark.parametrize("args,why", ENCODE_UPDATE_PTRS_VAR_REFUSED)
def test_encode_update_ptrs_var_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(4, 2)
    first, count, *rest = args
    refused("qfec_encode_update_ptrs_var",
            qa.lib().qfec_encode_update_ptrs_var(code._h, first, count, *rest, None), why)


# (shards, shard, new, delta_only, groups, block_size, invalid)
UPDATE_PTRS_REFUSED = [
    ((T, S, N, 0, -1, 16, None), "groups < 0"),
    ((T, S, N, 0, 1, 0, None), "block_size < 1"),
    ((T, S, N, 0, 1, -5, None), "block_size < 1"),
    ((T, S, N, 2, 1, 16, None), "delta_only"),
    ((T, S, N, -1, 1, 16, None), "delta_only"),
    ((None, S, N, 0, 1, 16, None), "null d_shards"),
    ((T, None, N, 0, 1, 16, None), "null d_shard"),
    ((T, S, None, 1, 1, 16, None), "null d_new"),
]


@pytest.mark.parametrize("args,why", UPDATE_PTRS_REFUSED)
def test_update_ptrs_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(4, 2)
    refused("qfec_update_ptrs", qa.lib().qfec_update_ptrs(code._h, *args, None), why)


# (shards, lens, group_len, shard, new, new_len, delta_only, groups, max_len, invalid)
UPDATE_PTRS_VAR_REFUSED = [
    ((T, L, GL, S, N, NL, 0, -1, 16, None), "groups < 0"),
    ((T, L, GL, S, N, NL, 0, 1, 0, None), "max_len < 1"),
    ((T, L, GL, S, N, NL, 7, 1, 16, None), "delta_only"),
    ((None, L, GL, S, N, NL, 0, 1, 16, None), "null d_shards"),
    ((T, None, GL, S, N, NL, 0, 1, 16, None), "null d_lens"),
    ((T, L, None, S, N, NL, 0, 1, 16, None), "null d_group_len"),
    ((T, None, None, S, N, NL, 1, 1, 16, None), "null d_group_len"),  # d_lens may be null in delta mode
    ((T, L, GL, None, N, NL, 0, 1, 16, None), "null d_shard"),
    ((T, L, GL, S, None, NL, 0, 1, 16, None), "null d_new"),
    ((T, L, GL, S, N, None, 1, 1, 16, None), "null d_new_len"),
]


@pytest.mark.parametrize("args,why", UPDATE_PTRS_VAR_REFUSED)
def test_update_ptrs_var_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(4, 2)
    refused("qfec_update_ptrs_var", qa.lib().qfec_update_ptrs_var(code._h, *args, None), why)


def test_null_code():
    lib = qa.lib()
    refused("qfec_encode_update_ptrs", lib.qfec_encode_update_ptrs(None, 0, 1, T, 1, 16, 1, None), "null code")
    refused("qfec_update_ptrs", lib.qfec_update_ptrs(None, T, S, N, 0, 1, 16, None, None), "null code")
    refused("qfec_encode_update_ptrs_var",
            lib.qfec_encode_update_ptrs_var(None, 0, 1, T, L, GL, 1, 16, 1, None, None), "null code")
    refused("qfec_update_ptrs_var", lib.qfec_update_ptrs_var(None, T, L, GL, S, N, NL, 0, 1, 16, None, None), "null code")
    # and with nothing to do
    refused("qfec_encode_update_ptrs", lib.qfec_encode_update_ptrs(None, 0, 1, None, 0, 16, 1, None), "null code")
    refused("qfec_update_ptrs_var",
            lib.qfec_update_ptrs_var(None, None, None, None, None, None, None, 0, 0, 16, None, None), "null code")


@pytest.mark.parametrize("k,m", [(4, 2), (40, 8), (60, 8), (200, 55)])
def test_nothing_to_do_is_ok_without_a_device(k, m):
    """groups = 0: QFEC_OK with null pointers, for any shape the code constructor takes (no k + m limit);
    a bad argument still wins over nothing-to-do."""
    lib = qa.lib()
    code = qa.Code.cauchy(k, m)
    assert lib.qfec_encode_update_ptrs(code._h, 0, k, None, 0, 16, 0, None) == 0
    assert lib.qfec_encode_update_ptrs(code._h, k - 1, 1, None, 0, 16, 1, None) == 0
    assert lib.qfec_update_ptrs(code._h, None, None, None, 1, 0, 16, None, None) == 0
    assert lib.qfec_encode_update_ptrs_var(code._h, 0, k, None, None, None, 0, 16, 0, None, None) == 0
    assert lib.qfec_update_ptrs_var(code._h, None, None, None, None, None, None, 0, 0, 16, None, None) == 0
    refused("qfec_encode_update_ptrs", lib.qfec_encode_update_ptrs(code._h, 0, k + 1, None, 0, 16, 0, None), "first")
    refused("qfec_encode_update_ptrs", lib.qfec_encode_update_ptrs(code._h, 0, k, None, 0, 16, 5, None), "accumulate")
    refused("qfec_update_ptrs", lib.qfec_update_ptrs(code._h, None, None, None, 0, 0, 0, None, None), "block_size < 1")
    refused("qfec_update_ptrs", lib.qfec_update_ptrs(code._h, None, None, None, 2, 0, 16, None, None), "delta_only")
    refused("qfec_encode_update_ptrs_var",
            lib.qfec_encode_update_ptrs_var(code._h, -1, k, None, None, None, 0, 16, 0, None, None), "first < 0")
    refused("qfec_update_ptrs_var",
            lib.qfec_update_ptrs_var(code._h, None, None, None, None, None, None, 0, 0, 0, None, None), "max_len < 1")


def test_no_parity_rows_is_ok_without_a_device():
    """m = 0 (a Vandermonde code may have none): QFEC_OK, nothing launched, no device looked for; a bad
    argument still wins."""
    lib = qa.lib()
    code = qa.Code.vandermonde(4, 0)
    assert lib.qfec_encode_update_ptrs(code._h, 0, 4, T, 3, 16, 0, None) == 0
    assert lib.qfec_update_ptrs(code._h, T, S, N, 0, 3, 16, None, None) == 0
    assert lib.qfec_encode_update_ptrs_var(code._h, 0, 4, T, L, GL, 3, 16, 0, None, None) == 0
    assert lib.qfec_update_ptrs_var(code._h, T, L, GL, S, N, NL, 0, 3, 16, None, None) == 0
    refused("qfec_encode_update_ptrs", lib.qfec_encode_update_ptrs(code._h, 2, 3, T, 3, 16, 0, None), "first")
    refused("qfec_update_ptrs_var", lib.qfec_update_ptrs_var(code._h, T, L, GL, S, None, NL, 0, 3, 16, None, None),
            "null d_new")


def test_python_face_checks_before_the_call():
    """The wrappers refuse a host tensor, a wrong count, a wrong dtype and a bad range themselves."""
    import torch

    code = qa.Code.cauchy(4, 2)
    ptrs = torch.zeros(12, dtype=torch.int64)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)  # noqa: E731
    with pytest.raises(qa.QfecError, match=r"groups \* \(k \+ m\)"):
        code.encode_update_ptrs(torch.zeros(13, dtype=torch.int64), 0, 1, 16)
    with pytest.raises(qa.QfecError, match="not inside"):
        code.encode_update_ptrs(ptrs, 3, 2, 16)
    with pytest.raises(qa.QfecError, match="not inside"):
        code.encode_update_ptrs_var(ptrs, 0, 0, i32(8), i32(2), 16)
    with pytest.raises(qa.QfecError, match="expected a device tensor"):
        code.encode_update_ptrs(ptrs, 0, 1, 16)
    with pytest.raises(qa.QfecError, match="shard has 3 elements"):
        code.update_ptrs(ptrs, i32(3), torch.zeros(2, dtype=torch.int64), 16)
    with pytest.raises(qa.QfecError, match="int64 addresses expected"):
        code.update_ptrs(ptrs, i32(2), i32(2), 16)
    with pytest.raises(qa.QfecError, match="lens has 7 elements"):
        code.encode_update_ptrs_var(ptrs, 0, 1, i32(7), i32(2), 16)
    with pytest.raises(qa.QfecError, match="group_len has 3 elements"):
        code.update_ptrs_var(ptrs, i32(8), i32(3), i32(2), torch.zeros(2, dtype=torch.int64), i32(2), 16)
    with pytest.raises(qa.QfecError, match="delta_only alone"):
        code.update_ptrs_var(ptrs, None, i32(2), i32(2), torch.zeros(2, dtype=torch.int64), i32(2), 16)
    with pytest.raises(qa.QfecError, match="new_len has dtype"):
        code.update_ptrs_var(ptrs, i32(8), i32(2), i32(2), torch.zeros(2, dtype=torch.int64),
                             torch.zeros(2, dtype=torch.int64), 16)
