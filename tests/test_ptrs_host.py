"""CPU tests of the host half of qfec_encode_ptrs and qfec_reconstruct_ptrs: every argument the calls
refuse is refused with QFEC_EINVAL and a cause in qfec_last_error, with stand-in pointers that are
never dereferenced, so the decision is made before a device is touched; empty work is done without
one; k + m > 24 is QFEC_EUNSUP for the reconstruct; a well-formed call on a machine without a GPU is
QFEC_ENODEV.  Also the knob rs_dev_ptrs, the Python face's own checks, and the launch geometry
(ptrs_geom in quicknet_amd/csrc/qfec_geom.hpp, through tests/ptrs_geom_host/shim.cpp, compiled here
with g++).  No kernel is launched here."""
import ctypes as C
import os
import re
import subprocess

import pytest

import quicknet_amd as qa

QFEC_OK, QFEC_EINVAL, QFEC_ENODEV, QFEC_EUNSUP = 0, -1, -2, -5
T, M = 4096, 8192  # stand-ins for the device table and the marks (never dereferenced)


def last_error():
    return qa.lib().qfec_last_error().decode()


def test_error_codes_are_the_headers():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qfec.h")).read()
    for name, value in (("QFEC_EINVAL", QFEC_EINVAL), ("QFEC_ENODEV", QFEC_ENODEV), ("QFEC_EUNSUP", QFEC_EUNSUP)):
        assert re.search(rf"{name}\s*=?\s*\(?{value}\b", text), name


# (shards, groups, block_size) -> the cause named
ENCODE_REFUSED = [
    ((T, -1, 16), "groups < 0"),
    ((T, 1, 0), "block_size < 1"),
    ((T, 1, -7), "block_size < 1"),
    ((None, 1, 16), "null d_shards"),
    ((None, -1, 16), "groups < 0"),
]


@pytest.mark.parametrize("args,why", ENCODE_REFUSED)
def test_encode_ptrs_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(4, 2)
    assert qa.lib().qfec_encode_ptrs(code._h, *args, None) == QFEC_EINVAL
    assert "qfec_encode_ptrs:" in last_error() and why in last_error(), last_error()


# (shards, marks, groups, block_size) -> the cause named
RECONSTRUCT_REFUSED = [
    ((T, M, -1, 16), "groups < 0"),
    ((T, M, 1, 0), "block_size < 1"),
    ((None, M, 1, 16), "null d_shards"),
    ((T, None, 1, 16), "null d_marks"),
    ((None, None, 1, 16), "null d_shards"),
]


@pytest.mark.parametrize("args,why", RECONSTRUCT_REFUSED)
def test_reconstruct_ptrs_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(4, 2)
    assert qa.lib().qfec_reconstruct_ptrs(code._h, *args, None, None) == QFEC_EINVAL
    assert "qfec_reconstruct_ptrs:" in last_error() and why in last_error(), last_error()


def test_null_code():
    L = qa.lib()
    assert L.qfec_encode_ptrs(None, T, 1, 16, None) == QFEC_EINVAL
    assert "qfec_encode_ptrs:" in last_error() and "null code" in last_error()
    assert L.qfec_reconstruct_ptrs(None, T, M, 1, 16, None, None) == QFEC_EINVAL
    assert "qfec_reconstruct_ptrs:" in last_error() and "null code" in last_error()
    assert L.qfec_encode_ptrs(None, None, 0, 16, None) == QFEC_EINVAL


@pytest.mark.parametrize("k,m", [(4, 2), (20, 5), (200, 55)])
def test_no_groups_is_ok_without_a_device(k, m):
    L = qa.lib()
    code = qa.Code.cauchy(k, m)
    assert L.qfec_encode_ptrs(code._h, None, 0, 16, None) == QFEC_OK
    assert L.qfec_reconstruct_ptrs(code._h, None, None, 0, 16, None, None) == QFEC_OK
    # a bad argument still loses to nothing-to-do
    assert L.qfec_encode_ptrs(code._h, None, 0, 0, None) == QFEC_EINVAL
    assert L.qfec_reconstruct_ptrs(code._h, None, None, 0, 0, None, None) == QFEC_EINVAL


def test_encode_without_parity_rows_is_ok_without_a_device():
    code = qa.Code.vandermonde(4, 0)
    assert qa.lib().qfec_encode_ptrs(code._h, T, 3, 16, None) == QFEC_OK


def test_reconstruct_of_a_wide_code_is_unsupported():
    """k + m = 25: no pattern LUT and no host-record path on pointer tables; said before a device is
    looked for (the same answer with and without a GPU)."""
    code = qa.Code.cauchy(20, 5)
    assert qa.lib().qfec_reconstruct_ptrs(code._h, T, M, 1, 16, None, None) == QFEC_EUNSUP
    assert "qfec_reconstruct_ptrs:" in last_error() and "25" in last_error()
    ok = qa.Code.cauchy(20, 4)  # k + m = 24 gets past that check
    assert qa.lib().qfec_reconstruct_ptrs(ok._h, None, M, 1, 16, None, None) == QFEC_EINVAL


def test_well_formed_calls_need_a_device():
    if qa.device_count() > 0:
        pytest.skip("a GPU is present: the calls would run")
    L = qa.lib()
    code = qa.Code.cauchy(4, 2)
    assert L.qfec_encode_ptrs(code._h, T, 1, 16, None) == QFEC_ENODEV
    assert L.qfec_reconstruct_ptrs(code._h, T, M, 1, 16, None, None) == QFEC_ENODEV


def test_knob_rs_dev_ptrs():
    L = qa.lib()
    assert qa.tune_get("rs_dev_ptrs") == 0
    try:
        assert L.qfec_tune(b"rs_dev_ptrs", 1) == 0 and qa.tune_get("rs_dev_ptrs") == 1
        for bad in (-1, 2, 7):
            assert L.qfec_tune(b"rs_dev_ptrs", bad) == QFEC_EINVAL
            assert qa.tune_get("rs_dev_ptrs") == 1
    finally:
        assert L.qfec_tune(b"rs_dev_ptrs", 0) == 0
    assert qa.tune_get("rs_dev_ptrs") == 0


def test_python_face_checks_the_pointer_count():
    import torch

    code = qa.Code.cauchy(4, 2)
    for n in (5, 7, 13):
        with pytest.raises(qa.QfecError, match="groups \\* \\(k \\+ m\\)"):
            code.encode_ptrs(torch.zeros(n, dtype=torch.int64), 16)
        with pytest.raises(qa.QfecError, match="groups \\* \\(k \\+ m\\)"):
            code.reconstruct_ptrs(torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.uint8), 16)
    with pytest.raises(qa.QfecError, match="groups \\* \\(k \\+ m\\)"):
        code.encode_ptrs(torch.zeros((2, 6), dtype=torch.int64), 16)
    with pytest.raises(qa.QfecError, match="marks"):
        code.reconstruct_ptrs(torch.zeros(12, dtype=torch.int64), torch.zeros(11, dtype=torch.uint8), 16)
    with pytest.raises(qa.QfecError, match="expected a device tensor"):
        code.encode_ptrs(torch.zeros(12, dtype=torch.int64), 16)


# ------------------------------------------------------------------ geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ptrs_geom_host", "shim.cpp")
HDR = os.path.join(ROOT, "quicknet_amd", "csrc", "qfec_geom.hpp")
OUT = os.path.join(ROOT, "tests", "ptrs_geom_host", "_build", "libptrs_geom_shim.so")
LANES = 0x7FFFFFFF


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", OUT, SRC], check=True)
    L = C.CDLL(OUT)
    L.ptrs_geom_shape.restype = C.c_longlong
    L.ptrs_geom_shape.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_uint)]
    L.ptrs_lanes.restype = C.c_int
    L.ptrs_lanes.argtypes = [C.c_int, C.c_int]
    return L


def geom(L, block, lane_bytes):
    out = (C.c_uint * 4)()
    per = L.ptrs_geom_shape(block, lane_bytes, out)
    return tuple(out), per


# block -> (vcols, wpg, tail0, tailn) on 16-B lanes and on 8-B lanes
GEOM = {
    1: ((0, 1, 0, 1), (0, 1, 0, 1)),
    15: ((0, 1, 0, 15), (1, 1, 8, 7)),
    16: ((1, 1, 16, 0), (2, 1, 16, 0)),
    17: ((1, 1, 16, 1), (2, 1, 16, 1)),
    1000: ((62, 1, 992, 8), (125, 2, 1000, 0)),
    1024: ((64, 1, 1024, 0), (128, 2, 1024, 0)),
    1400: ((87, 2, 1392, 8), (175, 3, 1400, 0)),
}


@pytest.mark.parametrize("block", sorted(GEOM))
def test_ptrs_geom_shapes(shim, block):
    for lane_bytes, want in zip((16, 8), GEOM[block]):
        (vcols, wpg, tail0, tailn), per = geom(shim, block, lane_bytes)
        assert (vcols, wpg, tail0, tailn) == want
        assert tail0 == vcols * lane_bytes and tail0 + tailn == block and tailn < lane_bytes
        assert (wpg - 1) * 64 < vcols + (1 if tailn else 0) <= wpg * 64  # the last wave exists and has work
        assert wpg * 64 * lane_bytes >= block                            # the byte spans reach the end
        assert per * 64 * wpg <= LANES < (per + 1) * 64 * wpg


def test_ptrs_geom_wave_boundaries(shim):
    """One column past a wave, with and without a tail: the tail's lanes sit in the last wave."""
    assert geom(shim, 1025, 16)[0] == (64, 2, 1024, 1)   # the second wave holds only the tail
    assert geom(shim, 1040, 16)[0] == (65, 2, 1040, 0)
    assert geom(shim, 1023, 16)[0] == (63, 1, 1008, 15)
    assert geom(shim, 513, 8)[0] == (64, 2, 512, 1)


def test_lane_width_rule(shim):
    for k in (1, 3, 4, 8, 9):
        assert shim.ptrs_lanes(1, k) == 16 and shim.ptrs_lanes(0, k) == 16
    for k in (10, 16, 20):
        assert shim.ptrs_lanes(1, k) == 8 and shim.ptrs_lanes(0, k) == 16
