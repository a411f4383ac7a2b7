"""qfec_update's launch geometry (wave_geom in quicknet_amd/csrc/qfec_geom.hpp) on CPU: columns per
row and waves per group for the shapes the GPU suite and the A/B tool run, and the cut of a batch
into launches at sizes no GPU test can reach.  tests/update_geom_host/shim.cpp is compiled here with
g++."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "update_geom_host", "shim.cpp")
HDR = os.path.join(ROOT, "quicknet_amd", "csrc", "qfec_geom.hpp")
OUT = os.path.join(ROOT, "tests", "update_geom_host", "_build", "libupdate_geom_shim.so")

LANES = 0x7FFFFFFF  # the most lanes launch_update accepts
BASE = 0x7F0000000000  # a 16-B aligned address


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(OUT) or os.path.getmtime(OUT) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", OUT, SRC], check=True)
    L = C.CDLL(OUT)
    L.update_geom.restype = None
    L.update_geom.argtypes = [C.c_ulonglong, C.c_ulonglong, C.c_int, C.c_longlong, C.c_ulonglong, C.c_ulonglong,
                              C.POINTER(C.c_uint), C.POINTER(C.c_longlong)]
    L.update_chunks.restype = C.c_longlong
    L.update_chunks.argtypes = [C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong)]
    return L


def geom(L, m, block, pitch, rows=BASE):
    out = (C.c_uint * 3)()
    per = C.c_longlong(0)
    L.update_geom(rows, BASE + (1 << 30), block, pitch, pitch, m * pitch, out, C.byref(per))
    return tuple(out), per.value


# (m, block, pitch) -> cols = ceil(block / 16), wpg = ceil(cols / 64)
@pytest.mark.parametrize("m,block,pitch,want", [
    (3, 1024, 1040, (64, 1)),
    (3, 1024, 1024, (64, 1)),
    (4, 1400, 1424, (88, 2)),
    (5, 100, 128, (7, 1)),
    (8, 64, 64, (4, 1)),
    (3, 1025, 1040, (65, 2)),   # one column past a wave
])
def test_wave_geom_shapes(shim, m, block, pitch, want):
    (vec16, cols, wpg), per = geom(shim, m, block, pitch)
    assert (vec16, cols, wpg) == (1,) + want
    assert cols * 16 <= pitch      # the last lane's access ends inside the row
    assert per * 64 * wpg <= LANES < (per + 1) * 64 * wpg


def test_wave_geom_unaligned_layouts_are_flat(shim):
    """Pitch 37 and an odd rows base: byte lanes, and qfec_update then takes FlatGeom's split."""
    assert geom(shim, 2, 37, 37)[0][0] == 0
    assert geom(shim, 3, 1024, 1040, rows=BASE + 4)[0][0] == 0


def test_update_chunks_beyond_one_launch(shim):
    """2^31 groups of two waves each: every launch within the limit, the batch covered in order."""
    (_, _, wpg), per = geom(shim, 4, 1400, 1424)
    assert wpg == 2
    most = C.c_longlong(0)
    n = shim.update_chunks(1 << 31, per, C.byref(most))
    assert n == -(-(1 << 31) // per) and n >= 64 * wpg
    assert most.value * wpg * 64 <= LANES
    assert shim.update_chunks(0, per, C.byref(most)) == 0
    assert shim.update_chunks(per, per, C.byref(most)) == 1 and most.value == per
    assert shim.update_chunks(per + 1, per, C.byref(most)) == 2
