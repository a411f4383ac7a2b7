"""module/rs.h (reed_solomon_encode / reed_solomon_reconstruct) on arrays whose shards are all in
device memory but not back to back, with the knob rs_dev_ptrs = 1: the pointer array goes to the
device and the pointer-table kernels work on the caller's rows in place.  Results and return codes
equal the oracle's and those of the staged branch (knob 0); arrays the knob does not cover still take
their old branch.

Run on an MI355X:  python -m pytest tests/test_gpu_rs_ptrs.py -m gpu -q
"""
import ctypes as C
import re

import numpy as np
import pytest

import quicknet_amd as qa
from quicknet_amd.synth import marks_to_rs_layout, synth_bytes
from rs_abi_common import device_rows, fetch, knobs, ptr_array  # noqa: F401  (knobs is a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

DEV = torch.device("cuda:0")
SHAPES = [(10, 3, 1000, 12), (16, 4, 1400, 9)]
shape_ids = [f"{k}-{m}-B{B}-G{G}" for k, m, B, G in SHAPES]


def marks_for(G, k, m, seed):
    """Per group 0 .. m + 1 erasures; group 0 untouched, group 1 unrecoverable (m + 1 data rows)."""
    rng = np.random.default_rng(seed)
    gm = np.zeros((G, k + m), np.uint8)
    for g in range(G):
        gm[g, rng.choice(k + m, int(rng.integers(0, m + 2)), replace=False)] = 1
    gm[0, :] = 0
    gm[1, :] = 0
    gm[1, :m + 1] = 1
    gm[2, :] = 0
    gm[2, [0, k - 1]] = 1  # recoverable whatever was drawn
    return gm


def encoded(oracle, rows_pk, k, m, B, G, seed, stale=0x33):
    """(data [G,k,B], the oracle's parity [G,m,B] over parity shards that held `stale`)."""
    data = synth_bytes(seed, G * k * B).reshape(G, k, B)
    want = np.full((G, m, B), stale, np.uint8)
    oracle.rs_encode(rows_pk, data, want, B)
    return data, want


@pytest.mark.parametrize("chunk", [0, 5])
@pytest.mark.parametrize("k,m,B,G", SHAPES, ids=shape_ids)
def test_rs_device_rows_encode_and_reconstruct(oracle, knobs, k, m, B, G, chunk):
    """All-device scattered rows at knob 1: the encode equals the oracle's; the reconstruct, over marks
    with an untouched and an unrecoverable group, returns the oracle's code (-1) and leaves the
    oracle's rows; parity rows are never written by it.  host_chunk = 5 forces several chunks."""
    knobs("rs_dev_ptrs", 1)
    knobs("host_chunk", chunk)
    n = k + m
    rs = qa.ReedSolomon(k, m)
    L = qa.lib()
    data, want = encoded(oracle, oracle.cauchy(k, m), k, m, B, G, 0xD0 + k)
    rows = device_rows(list(data.reshape(G * k, B)) + [np.full(B, 0x33, np.uint8)] * (G * m))
    assert L.reed_solomon_encode(rs._h, ptr_array(rows), G * n, B) == 0
    assert np.array_equal(fetch(rows[G * k:]).reshape(G, m, B), want)
    assert np.array_equal(fetch(rows[:G * k]).reshape(G, k, B), data)

    gm = marks_for(G, k, m, 31 + k)
    marks = marks_to_rs_layout(gm, k)
    d = data.copy()
    d.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
    par = synth_bytes(0xBEE + k, G * m * B).reshape(G, m, B)  # inconsistent parity pins the survivor rule
    rows = device_rows(list(d.reshape(G * k, B)) + list(par.reshape(G * m, B)))
    exp = d.copy()
    rc_o = oracle.rs_reconstruct(oracle.cauchy(k, m), exp, par.copy(), marks, B)
    rc = L.reed_solomon_reconstruct(rs._h, ptr_array(rows), C.c_void_p(marks.ctypes.data), G * n, B)
    assert rc == rc_o == -1
    assert np.array_equal(fetch(rows[:G * k]).reshape(G, k, B), exp)
    assert np.array_equal(fetch(rows[G * k:]).reshape(G, m, B), par)
    assert np.array_equal(exp[0], d[0]) and np.array_equal(exp[1], d[1])  # untouched, unrecoverable
    # every group recoverable: 0
    gm[1, :] = 0
    gm = np.where(gm.sum(1, keepdims=True) > m, 0, gm).astype(np.uint8)
    marks = marks_to_rs_layout(gm, k)
    d = data.copy()
    d.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
    rows = device_rows(list(d.reshape(G * k, B)) + list(want.reshape(G * m, B)))
    rc = L.reed_solomon_reconstruct(rs._h, ptr_array(rows), C.c_void_p(marks.ctypes.data), G * n, B)
    assert rc == 0
    assert np.array_equal(fetch(rows[:G * k]).reshape(G, k, B), data)
    rs.close()


def test_rs_device_rows_device_marks(oracle, knobs):
    """The marks in device memory too."""
    knobs("rs_dev_ptrs", 1)
    k, m, B, G = 10, 3, 1000, 12
    n = k + m
    rs = qa.ReedSolomon(k, m)
    data, want = encoded(oracle, oracle.cauchy(k, m), k, m, B, G, 0xD1)
    gm = marks_for(G, k, m, 5)
    marks = marks_to_rs_layout(gm, k)
    d = data.copy()
    d.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
    rows = device_rows(list(d.reshape(G * k, B)) + list(want.reshape(G * m, B)))
    exp = d.copy()
    rc_o = oracle.rs_reconstruct(oracle.cauchy(k, m), exp, want.copy(), marks, B)
    dmarks = torch.from_numpy(marks).to(DEV)
    rc = qa.lib().reed_solomon_reconstruct(rs._h, ptr_array(rows), C.c_void_p(dmarks.data_ptr()), G * n, B)
    assert rc == rc_o == -1
    assert np.array_equal(fetch(rows[:G * k]).reshape(G, k, B), exp)
    rs.close()


def test_rs_device_rows_quirk_edit(oracle, knobs):
    """The public rs->parity edited to a zero column-0 coefficient: that parity row keeps its shard's
    old bytes where rs.c keeps them (rs.c:116-117), on the caller's rows in place."""
    knobs("rs_dev_ptrs", 1)
    knobs("host_chunk", 5)
    k, m, B, G = 10, 3, 1000, 12
    n = k + m
    rs = qa.ReedSolomon(k, m)
    pk = rs.parity.copy()
    pk[1, 0] = 0
    rs.parity[:] = pk
    data = synth_bytes(0xED18, G * k * B).reshape(G, k, B)
    stale = synth_bytes(0x0DE, G * m * B).reshape(G, m, B)
    want = stale.copy()
    oracle.rs_encode(pk, data, want, B)
    assert not np.array_equal(want[:, 1], np.zeros_like(want[:, 1]))
    rows = device_rows(list(data.reshape(G * k, B)) + list(stale.reshape(G * m, B)))
    assert qa.lib().reed_solomon_encode(rs._h, ptr_array(rows), G * n, B) == 0
    assert np.array_equal(fetch(rows[G * k:]).reshape(G, m, B), want)
    rs.close()


def test_rs_trace_names_the_branch(oracle, knobs, capfd, monkeypatch):
    """QFEC_RS_TRACE=1: `(ptrs)` at knob 1 and `(staged)` at knob 0 for the same array, and the two
    runs leave identical bytes, for the encode and for the reconstruct."""
    k, m, B, G = 10, 3, 1000, 12
    n = k + m
    L = qa.lib()
    data, want = encoded(oracle, oracle.cauchy(k, m), k, m, B, G, 0xD2)
    gm = marks_for(G, k, m, 9)
    marks = marks_to_rs_layout(gm, k)
    d = data.copy()
    d.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
    got = {}
    monkeypatch.setenv("QFEC_RS_TRACE", "1")
    for knob, tag in ((1, "ptrs"), (0, "staged")):
        knobs("rs_dev_ptrs", knob)
        rs = qa.ReedSolomon(k, m)
        rows = device_rows(list(data.reshape(G * k, B)) + [np.full(B, 0x33, np.uint8)] * (G * m))
        capfd.readouterr()
        assert L.reed_solomon_encode(rs._h, ptr_array(rows), G * n, B) == 0
        err = capfd.readouterr().err
        assert re.search(rf"reed_solomon_encode \({tag}\)", err), err[-1000:]
        enc = fetch(rows[G * k:])
        rows = device_rows(list(d.reshape(G * k, B)) + list(want.reshape(G * m, B)))
        rc = L.reed_solomon_reconstruct(rs._h, ptr_array(rows), C.c_void_p(marks.ctypes.data), G * n, B)
        err = capfd.readouterr().err
        assert re.search(rf"reed_solomon_reconstruct \({tag}\)", err), err[-1000:]
        got[knob] = (enc, rc, fetch(rows[:G * k]))
        rs.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[1][0].reshape(G, m, B), want)
    assert got[0][1] == got[1][1] == -1
    assert np.array_equal(got[0][2], got[1][2])


def test_rs_arrays_the_knob_does_not_cover(oracle, knobs, capfd, monkeypatch):
    """A mixed host/device array and an RS(20,10) device array (k + m > 24) at knob 1 still take the
    staged branch and still match the oracle."""
    knobs("rs_dev_ptrs", 1)
    monkeypatch.setenv("QFEC_RS_TRACE", "1")
    L = qa.lib()
    # mixed: every third row in host memory
    k, m, B, G = 10, 3, 1000, 12
    n = k + m
    data, want = encoded(oracle, oracle.cauchy(k, m), k, m, B, G, 0xD3)
    host = list(data.reshape(G * k, B).copy()) + [np.full(B, 0x33, np.uint8) for _ in range(G * m)]
    dev = device_rows(host)
    rows = [host[i] if i % 3 == 0 else dev[i] for i in range(G * n)]
    rs = qa.ReedSolomon(k, m)
    capfd.readouterr()
    assert L.reed_solomon_encode(rs._h, ptr_array(rows), G * n, B) == 0
    assert "reed_solomon_encode (staged)" in capfd.readouterr().err
    assert np.array_equal(fetch(rows[G * k:]).reshape(G, m, B), want)
    gm = marks_for(G, k, m, 13)
    marks = marks_to_rs_layout(gm, k)
    d = data.copy()
    d.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
    host = list(d.reshape(G * k, B).copy()) + list(want.reshape(G * m, B).copy())
    dev = device_rows(host)
    rows = [host[i] if i % 3 == 0 else dev[i] for i in range(G * n)]
    exp = d.copy()
    rc_o = oracle.rs_reconstruct(oracle.cauchy(k, m), exp, want.copy(), marks, B)
    assert L.reed_solomon_reconstruct(rs._h, ptr_array(rows), C.c_void_p(marks.ctypes.data), G * n, B) == rc_o == -1
    assert "reed_solomon_reconstruct (staged)" in capfd.readouterr().err
    assert np.array_equal(fetch(rows[:G * k]).reshape(G, k, B), exp)
    rs.close()
    # RS(20,10): the encode has no k + m limit and runs on the pointers; the reconstruct is staged
    k, m, B, G = 20, 10, 1000, 5
    n = k + m
    data, want = encoded(oracle, oracle.cauchy(k, m), k, m, B, G, 0xD4)
    rs = qa.ReedSolomon(k, m)
    rows = device_rows(list(data.reshape(G * k, B)) + [np.full(B, 0x33, np.uint8)] * (G * m))
    assert L.reed_solomon_encode(rs._h, ptr_array(rows), G * n, B) == 0
    assert np.array_equal(fetch(rows[G * k:]).reshape(G, m, B), want)
    gm = marks_for(G, k, m, 17)
    marks = marks_to_rs_layout(gm, k)
    d = data.copy()
    d.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
    rows = device_rows(list(d.reshape(G * k, B)) + list(want.reshape(G * m, B)))
    exp = d.copy()
    rc_o = oracle.rs_reconstruct(oracle.cauchy(k, m), exp, want.copy(), marks, B)
    capfd.readouterr()
    assert L.reed_solomon_reconstruct(rs._h, ptr_array(rows), C.c_void_p(marks.ctypes.data), G * n, B) == rc_o
    assert "reed_solomon_reconstruct (staged)" in capfd.readouterr().err
    assert np.array_equal(fetch(rows[:G * k]).reshape(G, k, B), exp)
    rs.close()
