"""module/rs.h (reed_solomon_reconstruct) on arrays whose shards are all in device memory but not back
to back, with k + m > 24 and the knobs rs_dev_ptrs = rs_dev_ptrs_wide = 1: the pointer array and the
marks go to the device, RECONSTRUCT plans are built there and applied on the caller's rows in place.
Bytes and return codes equal the oracle's and those of the staged branch (rs_dev_ptrs_wide = 0);
arrays the knob does not cover still take their old branch.

Run on an MI355X:  python -m pytest tests/test_gpu_rs_ptrs_wide.py -m gpu -q
"""
import ctypes as C

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
SHAPES = [(20, 10, 1000, 7), (40, 8, 1400, 6)]
shape_ids = [f"{k}-{m}-B{B}-G{G}" for k, m, B, G in SHAPES]


def marks_for(G, k, m, seed):
    """Per group 0 .. m erasures; group 0 untouched, group 1 unrecoverable (m + 1 data rows), group 2
    with data and parity lost."""
    rng = np.random.default_rng(seed)
    gm = np.zeros((G, k + m), np.uint8)
    for g in range(G):
        gm[g, rng.choice(k + m, int(rng.integers(1, m + 1)), replace=False)] = 1
    gm[0, :] = 0
    gm[1, :] = 0
    gm[1, :m + 1] = 1
    gm[2, :] = 0
    gm[2, [0, k - 1, k, k + 2]] = 1
    return gm


def batch(k, m, B, G, seed, recoverable=False):
    """(damaged data, inconsistent parity, marks): the parity pins the survivor rule."""
    gm = marks_for(G, k, m, seed)
    if recoverable:
        gm[1, :] = 0
    marks = marks_to_rs_layout(gm, k)
    d = synth_bytes(seed, G * k * B).reshape(G, k, B)
    d.reshape(G * k, B)[marks[:G * k] == 1] = 0x5A
    par = synth_bytes(seed + 1, G * m * B).reshape(G, m, B)
    return d, par, marks


def reconstruct(rs, d, par, marks, B):
    G, k, m = d.shape[0], d.shape[1], par.shape[1]
    rows = device_rows(list(d.reshape(G * k, B)) + list(par.reshape(G * m, B)))
    rc = qa.lib().reed_solomon_reconstruct(rs._h, ptr_array(rows), C.c_void_p(marks.ctypes.data), G * (k + m), B)
    return rc, fetch(rows[:G * k]).reshape(G, k, B), fetch(rows[G * k:]).reshape(G, m, B)


@pytest.mark.parametrize("chunk", [0, 3])
@pytest.mark.parametrize("k,m,B,G", SHAPES, ids=shape_ids)
def test_rs_wide_device_rows(oracle, knobs, capfd, monkeypatch, k, m, B, G, chunk):
    """Both knobs at 1 against the live rs.c and against rs_dev_ptrs_wide = 0: the same bytes, the
    same return code (-1 with an under-determined group, which stays untouched; 0 without), and the
    trace names the branch taken.  host_chunk = 3 forces several chunks."""
    knobs("rs_dev_ptrs", 1)
    knobs("host_chunk", chunk)
    monkeypatch.setenv("QFEC_RS_TRACE", "1")
    rows_pk = oracle.cauchy(k, m)
    for recoverable, want_rc in ((False, -1), (True, 0)):
        d, par, marks = batch(k, m, B, G, 0xE0 + k, recoverable)
        exp = d.copy()
        assert oracle.rs_reconstruct(rows_pk, exp, par.copy(), marks, B) == want_rc
        assert not np.array_equal(exp, d)
        got = {}
        for wide, tag in ((1, "ptrs wide"), (0, "staged")):
            knobs("rs_dev_ptrs_wide", wide)
            rs = qa.ReedSolomon(k, m)
            capfd.readouterr()
            got[wide] = reconstruct(rs, d, par, marks, B)
            err = capfd.readouterr().err
            assert f"reed_solomon_reconstruct ({tag})" in err, err[-1000:]
            rs.close()
        for wide in (1, 0):
            rc, out_d, out_p = got[wide]
            assert rc == want_rc, wide
            assert np.array_equal(out_d, exp), wide
            assert np.array_equal(out_p, par), wide  # parity rows are never written
        if not recoverable:
            assert np.array_equal(got[1][1][1], d[1]) and np.array_equal(got[1][1][0], d[0])  # unrecoverable, untouched


def test_rs_wide_edited_handle_stays_staged(oracle, knobs, capfd, monkeypatch):
    """The public rs->parity edited: device plans do not reproduce rs.c's decode of an edited handle,
    so the array takes the staged branch at either setting, with identical bytes."""
    knobs("rs_dev_ptrs", 1)
    monkeypatch.setenv("QFEC_RS_TRACE", "1")
    k, m, B, G = 20, 10, 1000, 5
    d, par, marks = batch(k, m, B, G, 0xE7, recoverable=True)
    got = {}
    for wide in (1, 0):
        knobs("rs_dev_ptrs_wide", wide)
        rs = qa.ReedSolomon(k, m)
        pk = rs.parity.copy()
        pk[1, 3] ^= 0x15
        rs.parity[:] = pk
        capfd.readouterr()
        got[wide] = reconstruct(rs, d, par, marks, B)
        assert "reed_solomon_reconstruct (staged)" in capfd.readouterr().err
        rs.close()
    assert got[0][0] == got[1][0]
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])
    assert not np.array_equal(got[1][1], d)


def test_rs_wide_leaves_narrow_codes_alone(oracle, knobs, capfd, monkeypatch):
    """RS(10,3) with both knobs at 1 still takes the LUT kernels on the table."""
    knobs("rs_dev_ptrs", 1)
    knobs("rs_dev_ptrs_wide", 1)
    monkeypatch.setenv("QFEC_RS_TRACE", "1")
    k, m, B, G = 10, 3, 1000, 6
    d, par, marks = batch(k, m, B, G, 0xE9)
    exp = d.copy()
    rc_o = oracle.rs_reconstruct(oracle.cauchy(k, m), exp, par.copy(), marks, B)
    rs = qa.ReedSolomon(k, m)
    capfd.readouterr()
    rc, out_d, out_p = reconstruct(rs, d, par, marks, B)
    assert "reed_solomon_reconstruct (ptrs)" in capfd.readouterr().err
    assert rc == rc_o == -1 and np.array_equal(out_d, exp) and np.array_equal(out_p, par)
    rs.close()


def test_rs_wide_needs_both_knobs(oracle, knobs, capfd, monkeypatch):
    """rs_dev_ptrs = 0 with rs_dev_ptrs_wide = 1: staged."""
    knobs("rs_dev_ptrs", 0)
    knobs("rs_dev_ptrs_wide", 1)
    monkeypatch.setenv("QFEC_RS_TRACE", "1")
    k, m, B, G = 20, 10, 1000, 4
    d, par, marks = batch(k, m, B, G, 0xEB, recoverable=True)
    exp = d.copy()
    assert oracle.rs_reconstruct(oracle.cauchy(k, m), exp, par.copy(), marks, B) == 0
    rs = qa.ReedSolomon(k, m)
    capfd.readouterr()
    rc, out_d, _ = reconstruct(rs, d, par, marks, B)
    assert "reed_solomon_reconstruct (staged)" in capfd.readouterr().err
    assert rc == 0 and np.array_equal(out_d, exp)
    rs.close()
