"""The launch geometry (quicknet_amd/csrc/qfec_geom.hpp) on CPU: lanes per row of the flat and the
8-byte-lane mappings for the shapes the GPU suite runs, what turns 16-byte columns off, and the cut
of a batch into launches at sizes no GPU test can reach.  tests/geom_host/shim.cpp is compiled here
with g++."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "geom_host", "shim.cpp")
HDR = os.path.join(ROOT, "quicknet_amd", "csrc", "qfec_geom.hpp")
OUT = os.path.join(ROOT, "tests", "geom_host", "_build", "libgeom_shim.so")

LANES = 0x7FFFFFFF  # the most lanes (flat) or waves (8-byte lanes) a launch function accepts
BASE = 0x7F0000000000  # a 16-B aligned address


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", OUT, SRC], check=True)
    L = C.CDLL(OUT)
    L.geom_shape.restype = None
    L.geom_shape.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_int, C.c_longlong, C.c_ulonglong, C.c_ulonglong,
                             C.POINTER(C.c_uint), C.POINTER(C.c_longlong)]
    L.geom_chunks.restype = C.c_longlong
    L.geom_chunks.argtypes = [C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_longlong]
    L.geom_chunks_stop.restype = C.c_longlong
    L.geom_chunks_stop.argtypes = [C.c_longlong, C.c_longlong, C.c_longlong, C.POINTER(C.c_int)]
    return L


def shape(L, k, m, block, pitch, data=BASE, parity=BASE + (1 << 30), dgs=None, pgs=None):
    out = (C.c_uint * 4)()
    per = (C.c_longlong * 2)()
    L.geom_shape(data, parity, k, block, pitch, k * pitch if dgs is None else dgs, m * pitch if pgs is None else pgs,
                 out, per)
    return tuple(out), tuple(per)


def chunks(L, groups, per):
    cap = groups // per + 2
    g0 = (C.c_longlong * cap)()
    gn = (C.c_longlong * cap)()
    n = L.geom_chunks(groups, per, g0, gn, cap)
    assert n <= cap
    return list(zip(g0[:n], gn[:n]))


# (k, m, block, pitch) of the GPU suite -> vec16, cols, cols8, wpg8 by the formulas each launch site
# carried before they moved into the header:
#   vec16 = bases, pitch 16-B aligned and round_up(block, 16) <= pitch
#   cols  = vec16 ? ceil(block / 16) : block
#   cols8 = vec16 && k < 14 ? 2 * cols : ceil(block / 8);  wpg8 = ceil(cols8 / 64)
@pytest.mark.parametrize("k,m,block,pitch,want", [
    (10, 3, 1024, 1040, (1, 64, 128, 2)),
    (16, 4, 1400, 1424, (1, 88, 175, 3)),   # k >= 14: just the row's 8-B columns
    (9, 5, 100, 128, (1, 7, 14, 1)),
    (4, 2, 37, 37, (0, 37, 5, 1)),          # pitch not a multiple of 16: byte lanes
])
def test_geom_gpu_suite_shapes(shim, k, m, block, pitch, want):
    got, per = shape(shim, k, m, block, pitch)
    assert got == want
    assert per[0] == LANES // want[1]
    assert per[1] * 64 * want[3] <= LANES < (per[1] + 1) * 64 * want[3]


def test_geom_vec16_off(shim):
    on = (1, 64, 128, 2)
    assert shape(shim, 10, 3, 1024, 1040)[0] == on
    off = (0, 1024, 128, 2)  # bytes; the 8-B columns are then the row's own, ceil(1024 / 8)
    assert shape(shim, 10, 3, 1024, 1040, data=BASE + 8)[0] == off
    assert shape(shim, 10, 3, 1024, 1040, parity=BASE + 4)[0] == off
    assert shape(shim, 10, 3, 1024, 1040, dgs=10 * 1040 + 8)[0] == off
    assert shape(shim, 10, 3, 1024, 1040, pgs=3 * 1040 + 1)[0] == off
    assert shape(shim, 10, 3, 1024, 1032)[0] == off       # pitch % 16 != 0
    assert shape(shim, 10, 3, 1025, 1024 + 16)[0] == (1, 65, 130, 3)
    assert shape(shim, 16, 4, 1400, 1424, data=BASE + 1)[0] == (0, 1400, 175, 3)


def check_cover(ch, groups):
    at = 0
    for g0, gn in ch:
        assert g0 == at and gn >= 1
        at += gn
    assert at == groups


def test_geom_chunks_flat(shim):
    """3e9 groups of one lane each: more lanes than one launch takes."""
    groups = 3 * 10**9
    (vec16, cols, _, _), (per, _) = shape(shim, 4, 2, 1, 1)
    assert (vec16, cols) == (0, 1)
    ch = chunks(shim, groups, per)
    assert len(ch) == 2
    check_cover(ch, groups)
    assert all(gn * cols <= LANES for _, gn in ch)


def test_geom_chunks_lane8(shim):
    """2^31 groups of three waves each."""
    groups = 1 << 31
    (_, _, _, wpg8), (_, per) = shape(shim, 16, 4, 1400, 1424)
    assert wpg8 == 3
    ch = chunks(shim, groups, per)
    check_cover(ch, groups)
    assert all(gn * wpg8 <= LANES for _, gn in ch)          # what launch_repair / launch_locate_erased accept
    assert all(gn * wpg8 * 64 <= LANES for _, gn in ch)     # the header's rule: lanes, as in the flat mapping


def test_geom_chunks_small_and_stop(shim):
    assert chunks(shim, 0, 5) == []
    assert chunks(shim, 5, 5) == [(0, 5)]
    assert chunks(shim, 11, 5) == [(0, 5), (5, 5), (10, 1)]
    rc = C.c_int(0)
    assert shim.geom_chunks_stop(11, 5, 1, C.byref(rc)) == 2 and rc.value == -7
    assert shim.geom_chunks_stop(11, 5, 9, C.byref(rc)) == 3 and rc.value == 0
