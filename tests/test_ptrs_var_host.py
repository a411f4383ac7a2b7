"""CPU tests of the host half of qfec_encode_ptrs_var and qfec_reconstruct_ptrs_var: every argument the
calls refuse is refused with QFEC_EINVAL and a cause in qfec_last_error, with stand-in pointers that are
never dereferenced, so the decision is made before a device is touched; empty work is done without
one; k + m > 24 is QFEC_EUNSUP for the reconstruct and accepted by the encode; a well-formed call on a
machine without a GPU is QFEC_ENODEV.  Also the Python face's count and dtype checks, and the rule by
which a group's own length is cut inside the kernels (ptrs_var_geom in quicknet_amd/csrc/qfec_geom.hpp,
through tests/ptrs_var_geom_host/shim.cpp, compiled here with g++).  No kernel is launched here."""
import ctypes as C
import os
import subprocess

import pytest

import quicknet_amd as qa

QFEC_OK, QFEC_EINVAL, QFEC_ENODEV, QFEC_EUNSUP = 0, -1, -2, -5
T, N, GL, M = 4096, 8192, 12288, 16384  # stand-ins for the table, the lengths, the group lengths, the marks


def last_error():
    return qa.lib().qfec_last_error().decode()


# (shards, lens, groups, max_len) -> the cause named
ENCODE_REFUSED = [
    ((T, N, -1, 16), "groups < 0"),
    ((T, N, 1, 0), "max_len < 1"),
    ((T, N, 1, -7), "max_len < 1"),
    ((None, N, 1, 16), "null d_shards"),
    ((T, None, 1, 16), "null d_lens"),
    ((None, None, 1, 16), "null d_shards"),
    ((None, None, -1, 0), "groups < 0"),
]


@pytest.mark.parametrize("args,why", ENCODE_REFUSED)
def test_encode_ptrs_var_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(4, 2)
    assert qa.lib().qfec_encode_ptrs_var(code._h, *args, None, None, None) == QFEC_EINVAL
    assert "qfec_encode_ptrs_var:" in last_error() and why in last_error(), last_error()


# (shards, lens, group_len, marks, groups, max_len) -> the cause named
RECONSTRUCT_REFUSED = [
    ((T, N, GL, M, -1, 16), "groups < 0"),
    ((T, N, GL, M, 1, 0), "max_len < 1"),
    ((None, N, GL, M, 1, 16), "null d_shards"),
    ((T, None, GL, M, 1, 16), "null d_lens"),
    ((T, N, GL, None, 1, 16), "null d_marks"),
    ((T, N, None, M, 1, 16), "null d_group_len"),
    ((None, None, None, None, 1, 16), "null d_shards"),
]


@pytest.mark.parametrize("args,why", RECONSTRUCT_REFUSED)
def test_reconstruct_ptrs_var_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(4, 2)
    assert qa.lib().qfec_reconstruct_ptrs_var(code._h, *args, None, None, None) == QFEC_EINVAL
    assert "qfec_reconstruct_ptrs_var:" in last_error() and why in last_error(), last_error()


def test_null_code():
    L = qa.lib()
    assert L.qfec_encode_ptrs_var(None, T, N, 1, 16, None, None, None) == QFEC_EINVAL
    assert "qfec_encode_ptrs_var:" in last_error() and "null code" in last_error()
    assert L.qfec_reconstruct_ptrs_var(None, T, N, GL, M, 1, 16, None, None, None) == QFEC_EINVAL
    assert "qfec_reconstruct_ptrs_var:" in last_error() and "null code" in last_error()
    assert L.qfec_encode_ptrs_var(None, None, None, 0, 16, None, None, None) == QFEC_EINVAL


@pytest.mark.parametrize("k,m", [(4, 2), (20, 5), (200, 55)])
def test_no_groups_is_ok_without_a_device(k, m):
    L = qa.lib()
    code = qa.Code.cauchy(k, m)
    assert L.qfec_encode_ptrs_var(code._h, None, None, 0, 16, None, None, None) == QFEC_OK
    assert L.qfec_reconstruct_ptrs_var(code._h, None, None, None, None, 0, 16, None, None, None) == QFEC_OK
    # a bad argument still loses to nothing-to-do
    assert L.qfec_encode_ptrs_var(code._h, None, None, 0, 0, None, None, None) == QFEC_EINVAL
    assert L.qfec_reconstruct_ptrs_var(code._h, None, None, None, None, 0, 0, None, None, None) == QFEC_EINVAL


def test_encode_without_parity_rows_is_ok_without_a_device():
    code = qa.Code.vandermonde(4, 0)
    assert qa.lib().qfec_encode_ptrs_var(code._h, T, N, 3, 16, None, None, None) == QFEC_OK


def test_wide_code_is_unsupported_for_the_reconstruct_only():
    """k + m = 25: no pattern LUT on pointer tables, said before a device is looked for; the encode
    takes the code (and then wants a device)."""
    code = qa.Code.cauchy(20, 5)
    assert qa.lib().qfec_reconstruct_ptrs_var(code._h, T, N, GL, M, 1, 16, None, None, None) == QFEC_EUNSUP
    assert "qfec_reconstruct_ptrs_var:" in last_error() and "25" in last_error()
    ok = qa.Code.cauchy(20, 4)  # k + m = 24 gets past that check
    assert qa.lib().qfec_reconstruct_ptrs_var(ok._h, None, N, GL, M, 1, 16, None, None, None) == QFEC_EINVAL
    if qa.device_count() == 0:
        assert qa.lib().qfec_encode_ptrs_var(code._h, T, N, 1, 16, None, None, None) == QFEC_ENODEV


def test_well_formed_calls_need_a_device():
    if qa.device_count() > 0:
        pytest.skip("a GPU is present: the calls would run")
    L = qa.lib()
    code = qa.Code.cauchy(4, 2)
    assert L.qfec_encode_ptrs_var(code._h, T, N, 1, 16, None, None, None) == QFEC_ENODEV
    assert L.qfec_reconstruct_ptrs_var(code._h, T, N, GL, M, 1, 16, None, None, None) == QFEC_ENODEV


def test_python_face_checks_counts_and_dtypes():
    import torch

    code = qa.Code.cauchy(4, 2)  # 12 pointers = 2 groups: 8 lengths, 2 group lengths, 12 marks
    ptrs = torch.zeros(12, dtype=torch.int64)
    lens, glen, marks = torch.zeros(8, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(12, dtype=torch.uint8)
    for n in (5, 7, 13):
        with pytest.raises(qa.QfecError, match="groups \\* \\(k \\+ m\\)"):
            code.encode_ptrs_var(torch.zeros(n, dtype=torch.int64), lens, 16)
        with pytest.raises(qa.QfecError, match="groups \\* \\(k \\+ m\\)"):
            code.reconstruct_ptrs_var(torch.zeros(n, dtype=torch.int64), lens, glen, marks, 16)
    with pytest.raises(qa.QfecError, match="lens has 7 elements, 8 expected"):
        code.encode_ptrs_var(ptrs, torch.zeros(7, dtype=torch.int32), 16)
    with pytest.raises(qa.QfecError, match="lens has dtype torch.int64"):
        code.encode_ptrs_var(ptrs, torch.zeros(8, dtype=torch.int64), 16)
    with pytest.raises(qa.QfecError, match="group_len has 3 elements, 2 expected"):
        code.encode_ptrs_var(ptrs, lens, 16, group_len=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(qa.QfecError, match="group_len has dtype torch.uint8"):
        code.encode_ptrs_var(ptrs, lens, 16, group_len=torch.zeros(2, dtype=torch.uint8))
    with pytest.raises(qa.QfecError, match="marks"):
        code.reconstruct_ptrs_var(ptrs, lens, glen, torch.zeros(11, dtype=torch.uint8), 16)
    with pytest.raises(qa.QfecError, match="lens has 9 elements, 8 expected"):
        code.reconstruct_ptrs_var(ptrs, torch.zeros(9, dtype=torch.int32), glen, marks, 16)
    with pytest.raises(qa.QfecError, match="lens has dtype torch.int16"):
        code.reconstruct_ptrs_var(ptrs, torch.zeros(8, dtype=torch.int16), glen, marks, 16)
    with pytest.raises(qa.QfecError, match="group_len has 1 elements, 2 expected"):
        code.reconstruct_ptrs_var(ptrs, lens, torch.zeros(1, dtype=torch.int32), marks, 16)
    with pytest.raises(qa.QfecError, match="group_len has dtype torch.int64"):
        code.reconstruct_ptrs_var(ptrs, lens, torch.zeros(2, dtype=torch.int64), marks, 16)
    with pytest.raises(qa.QfecError, match="expected a device tensor"):
        code.encode_ptrs_var(ptrs, lens, 16)
    with pytest.raises(qa.QfecError, match="expected a device tensor"):
        code.reconstruct_ptrs_var(ptrs, lens, glen, marks, 16)


# ------------------------------------------------------------------ the in-kernel geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ptrs_var_geom_host", "shim.cpp")
HDR = os.path.join(ROOT, "quicknet_amd", "csrc", "qfec_geom.hpp")
OUT = os.path.join(ROOT, "tests", "ptrs_var_geom_host", "_build", "libptrs_var_geom_shim.so")
MAX_LEN = 1400


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", OUT, SRC], check=True)
    L = C.CDLL(OUT)
    L.ptrs_var_geom_shape.restype = None
    L.ptrs_var_geom_shape.argtypes = [C.c_uint, C.c_uint, C.POINTER(C.c_uint)]
    L.ptrs_var_launch_wpg.restype = C.c_uint
    L.ptrs_var_launch_wpg.argtypes = [C.c_int, C.c_int]
    return L


# L -> (live waves, whole columns, tail start, tail count) on 16-B lanes and on 8-B lanes
GEOM = {
    0: ((0, 0, 0, 0), (0, 0, 0, 0)),
    1: ((1, 0, 0, 1), (1, 0, 0, 1)),
    15: ((1, 0, 0, 15), (1, 1, 8, 7)),
    16: ((1, 1, 16, 0), (1, 2, 16, 0)),
    17: ((1, 1, 16, 1), (1, 2, 16, 1)),
    1008: ((1, 63, 1008, 0), (2, 126, 1008, 0)),
    1024: ((1, 64, 1024, 0), (2, 128, 1024, 0)),
    1025: ((2, 64, 1024, 1), (3, 128, 1024, 1)),
    1400: ((2, 87, 1392, 8), (3, 175, 1400, 0)),
}


@pytest.mark.parametrize("L", sorted(GEOM))
def test_ptrs_var_geom_shapes(shim, L):
    for lane_bytes, want in zip((16, 8), GEOM[L]):
        out = (C.c_uint * 4)()
        shim.ptrs_var_geom_shape(L, lane_bytes, out)
        live, vcols, tail0, tailn = tuple(out)
        assert (live, vcols, tail0, tailn) == want
        assert tail0 == vcols * lane_bytes and tail0 + tailn == L and tailn < lane_bytes
        span = 64 * lane_bytes  # bytes of a slab
        assert live == (L + span - 1) // span             # a wave is live exactly when its slab starts below L
        assert live <= shim.ptrs_var_launch_wpg(MAX_LEN, lane_bytes)  # the launch has that wave
        if L:
            assert (live - 1) * 64 < vcols + (1 if tailn else 0) <= live * 64  # the last live wave has work
            if tailn:
                assert (live - 1) * span <= tail0 < live * span               # and the tail lies in its slab
