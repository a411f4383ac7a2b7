"""CPU tests of device-built check plans (qfec_check_build and friends, include/qfec.h): the check
plan arithmetic, which the host query qfec_check_build_host and the build kernel share as one text,
is held to the existing host query qfec_locate_erased_plan over the whole plan buffer; the rule for
which codes are accepted; and every argument the device calls refuse is refused on the host, with its
cause in qfec_last_error, with stand-in pointers that are never dereferenced.  No kernel is launched
here."""
import re

import numpy as np
import pytest

import quicknet_amd as qa
from locate_wide_common import FAILED, NONE, WORK, expected_check, header, layout, masks_of_every_t

QFEC_EINVAL, QFEC_EUNSUP = -1, -5
D, P, M, CK, C, MO = 64, 4096, 8192, 12288, 16384, 20480  # stand-ins for device pointers (never dereferenced)


def last_error():
    return qa.lib().qfec_last_error().decode()


def all_masks(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(np.uint8)


# (flavour, k, m, masks)
SETS = [
    ("cauchy", 4, 2, lambda: all_masks(6)),
    ("vandermonde", 4, 2, lambda: all_masks(6)),
    ("cauchy", 10, 3, lambda: masks_of_every_t(1, 13, 3, 12)),
    ("cauchy", 16, 4, lambda: masks_of_every_t(2, 20, 4, 10)),
    ("cauchy", 32, 8, lambda: masks_of_every_t(3, 40, 8, 6)),
    ("vandermonde", 32, 8, lambda: masks_of_every_t(4, 40, 8, 6)),
    ("cauchy", 60, 8, lambda: masks_of_every_t(5, 68, 8, 6)),
    ("cauchy", 70, 10, lambda: masks_of_every_t(6, 80, 10, 5)),
    ("cauchy", 200, 55, lambda: masks_of_every_t(7, 255, 55, 2)),
    ("cauchy", 128, 127, lambda: masks_of_every_t(8, 255, 127, 1)),
    ("cauchy", 1, 254, lambda: masks_of_every_t(9, 255, 254, 1)),
]


@pytest.mark.parametrize("flavour,k,m,masks", SETS, ids=[f"{s[0]}-{s[1]}-{s[2]}" for s in SETS])
def test_host_check_plan_equals_the_host_query(flavour, k, m, masks):
    """The whole buffer: S, t, status, the mark bits, K, the spares, A, the ratios and every padding
    byte, for masks of every t from 0 to m + 1."""
    code = getattr(qa.Code, flavour)(k, m)
    assert code.check_stride() == layout(k, m)[2]
    seen, ts = set(), set()
    for mk in masks():
        plan = code.check_host(mk)
        want = expected_check(code, mk)
        assert np.array_equal(plan, want), (np.nonzero(mk)[0], np.nonzero(plan != want)[0][:8])
        S, t, status = header(plan)
        assert t == int((mk != 0).sum()) and S == max(m - t, 0)
        seen.add(status)
        ts.add(t)
    assert seen == {NONE, WORK, FAILED} and ts >= set(range(min(m + 1, k + m) + 1))


@pytest.mark.parametrize("k,m", [(4, 2), (10, 3), (32, 8), (60, 8), (70, 10), (200, 55), (128, 127), (1, 254), (254, 1)])
def test_check_stride_is_the_layout_formula(k, m):
    code = qa.Code.cauchy(k, m)
    stride = qa.lib().qfec_check_stride(code._h)
    a_off, r_off, want = layout(k, m)
    assert stride == want and stride % 16 == 0 and a_off % 16 == 0 and r_off % 16 == 0
    assert stride >= 48 + k + m + m * k + k * (m - 1)
    assert qa.lib().qfec_check_stride(None) == QFEC_EINVAL and "null code" in last_error()


def every_call(code):
    """name -> a call with stand-in pointers that passes every argument check."""
    L, h = qa.lib(), code._h
    mk = np.zeros(code.k + code.m, np.uint8)
    out = np.zeros(max(int(L.qfec_check_stride(h)), 16), np.uint8)
    return {
        "qfec_check_build": lambda: L.qfec_check_build(h, M, 1, CK, None),
        "qfec_check_apply": lambda: L.qfec_check_apply(h, D, P, CK, 1, 16, 16, C, MO, None, None),
        "qfec_locate_wide": lambda: L.qfec_locate_wide(h, D, P, M, 1, 16, 16, C, MO, None, None),
        "qfec_scrub_wide": lambda: L.qfec_scrub_wide(h, D, P, M, 1, 16, 16, C, None, None, None),
        "qfec_check_build_host": lambda: L.qfec_check_build_host(h, mk.ctypes.data, out.ctypes.data),
    }


def empty_calls(code):
    """The same calls with zero groups and null buffers."""
    L, h = qa.lib(), code._h
    return {
        "qfec_check_build": lambda: L.qfec_check_build(h, None, 0, None, None),
        "qfec_check_apply": lambda: L.qfec_check_apply(h, None, None, None, 0, 16, 16, None, None, None, None),
        "qfec_locate_wide": lambda: L.qfec_locate_wide(h, None, None, None, 0, 16, 16, None, None, None, None),
        "qfec_scrub_wide": lambda: L.qfec_scrub_wide(h, None, None, None, 0, 16, 16, None, None, None, None),
    }


def assert_refused(code, why):
    for calls in (every_call(code), empty_calls(code)):
        for name, call in calls.items():
            assert call() == QFEC_EUNSUP, name
            assert name + ":" in last_error() and re.search(why, last_error()), last_error()


@pytest.mark.parametrize("k,m", [(4, 2), (10, 3), (32, 8), (200, 55)])
def test_generated_codes_are_accepted(k, m):
    """Both flavours, and qfec_code_from_rows of the generated rows, with or without the stale quirk:
    the host plan is the same bytes."""
    mk = np.zeros(k + m, np.uint8)
    mk[[0, k]] = 1
    for flavour in ("cauchy", "vandermonde"):
        code = getattr(qa.Code, flavour)(k, m)
        plan = code.check_host(mk)
        assert header(plan)[2] == (WORK if m > 2 else NONE)
        for quirk in (False, True):
            again = qa.Code.from_rows(code.rows, rs_stale_quirk=quirk)
            assert np.array_equal(again.check_host(mk), plan)
        for call in empty_calls(code).values():
            assert call() == 0


@pytest.mark.parametrize("k,m,row,col", [(4, 2, 0, 0), (32, 8, 7, 31), (32, 8, 3, 0), (200, 55, 54, 199)])
def test_one_changed_byte_is_refused(k, m, row, col):
    """Nothing but the generated rows: one byte of one row changed, and every call answers
    QFEC_EUNSUP on the host, also with zero groups and null buffers."""
    for flavour in ("cauchy", "vandermonde"):
        rows = getattr(qa.Code, flavour)(k, m).rows.copy()
        rows[row, col] ^= 0x01 if rows[row, col] != 1 else 0x02  # still non-zero
        assert_refused(qa.Code.from_rows(rows), "not those qfec_code_new generates")


def test_rows_of_another_shape_are_refused():
    """Three rows of the generated (4,4) are a fine MDS code, but not the generated (4,3)."""
    rows = qa.Code.cauchy(4, 4).rows[:3].copy()
    assert not np.array_equal(rows, qa.Code.cauchy(4, 3).rows)
    assert_refused(qa.Code.from_rows(rows), "not those qfec_code_new generates")


@pytest.mark.parametrize("k,m", [(4, 1), (254, 1)])
def test_one_parity_row_is_refused(k, m):
    assert_refused(qa.Code.cauchy(k, m), "m = 1 < 2")


def test_rs_handle_is_accepted_until_edited():
    """A reed_solomon handle is accepted; one edit of rs->m and every call answers QFEC_EUNSUP; the
    edit undone, it is accepted again."""
    rs = qa.ReedSolomon(6, 3)
    mk = np.zeros(9, np.uint8)
    mk[7] = 1
    plain = qa.Code.cauchy(6, 3)
    assert np.array_equal(rs.code().check_host(mk), plain.check_host(mk))
    rs.m_matrix[7, 2] ^= 0x21
    assert_refused(rs.code(), "decode matrix|not those qfec_code_new generates")
    rs.m_matrix[7, 2] ^= 0x21
    assert np.array_equal(rs.code().check_host(mk), plain.check_host(mk))
    rs.m_matrix[1, 2] ^= 0x21  # an identity row: the parity rows still match
    assert_refused(rs.code(), "decode matrix")
    rs.m_matrix[1, 2] ^= 0x21
    assert np.array_equal(rs.code().check_host(mk), plain.check_host(mk))


def test_fec_handle_is_accepted():
    fp = qa.FecParms(4, 7)
    mk = np.zeros(7, np.uint8)
    mk[2] = 1
    assert np.array_equal(fp.code().check_host(mk), qa.Code.vandermonde(4, 3).check_host(mk))


# (marks, groups, check) -> the cause named
BUILD_REFUSED = [
    ((M, -1, CK), "groups < 0"),
    ((M, 1, None), "null buffer"),
    ((None, 1, None), "null buffer"),
    ((M, 1, CK + 1), "d_check not 16-byte aligned"),
    ((None, 1, CK + 4), "d_check not 16-byte aligned"),
    ((M, 1, CK + 8), "d_check not 16-byte aligned"),
]


@pytest.mark.parametrize("args,why", BUILD_REFUSED)
def test_check_build_refuses_on_the_host(args, why):
    code = qa.Code.cauchy(32, 8)
    assert qa.lib().qfec_check_build(code._h, *args, None) == QFEC_EINVAL
    assert "qfec_check_build:" in last_error() and why in last_error(), last_error()


# (data, parity, third, groups, block_size, pitch) -> the cause named; third = check plan or marks
ROWS_REFUSED = [
    ((D, P, CK, -1, 16, 16), "groups < 0"),
    ((D, P, CK, 1, 0, 16), "block_size < 1"),
    ((D, P, CK, 1, -5, 16), "block_size < 1"),
    ((D, P, CK, 1, 32, 16), "pitch < block_size"),
    ((None, P, CK, 1, 16, 16), "null buffer"),
    ((D, None, CK, 1, 16, 16), "null buffer"),
]


@pytest.mark.parametrize("args,why", ROWS_REFUSED)
def test_apply_and_one_shots_refuse_on_the_host(args, why):
    L = qa.lib()
    code = qa.Code.cauchy(32, 8)
    assert L.qfec_check_apply(code._h, *args, C, MO, None, None) == QFEC_EINVAL
    assert "qfec_check_apply:" in last_error() and why in last_error(), last_error()
    assert L.qfec_locate_wide(code._h, *args, C, MO, None, None) == QFEC_EINVAL
    assert "qfec_locate_wide:" in last_error() and why in last_error(), last_error()
    assert L.qfec_scrub_wide(code._h, *args, C, None, None, None) == QFEC_EINVAL
    assert "qfec_scrub_wide:" in last_error() and why in last_error(), last_error()


def test_required_buffers_of_each_call():
    """The check plan and the culprit are required by qfec_check_apply, the culprit by
    qfec_locate_wide; a misaligned check plan is refused by qfec_check_apply at any data alignment."""
    L = qa.lib()
    h = qa.Code.cauchy(32, 8)._h
    assert L.qfec_check_apply(h, D, P, None, 1, 16, 16, C, MO, None, None) == QFEC_EINVAL and "null buffer" in last_error()
    assert L.qfec_check_apply(h, D, P, CK, 1, 16, 16, None, MO, None, None) == QFEC_EINVAL and "null buffer" in last_error()
    assert L.qfec_locate_wide(h, D, P, M, 1, 16, 16, None, MO, None, None) == QFEC_EINVAL and "null buffer" in last_error()
    for off, d in ((1, D), (4, D), (8, D + 1)):
        assert L.qfec_check_apply(h, d, P, CK + off, 1, 16, 16, C, MO, None, None) == QFEC_EINVAL
        assert "qfec_check_apply:" in last_error() and "d_check not 16-byte aligned" in last_error(), last_error()


def test_null_code_is_named():
    L = qa.lib()
    calls = {
        "qfec_check_build": lambda: L.qfec_check_build(None, M, 1, CK, None),
        "qfec_check_apply": lambda: L.qfec_check_apply(None, D, P, CK, 1, 16, 16, C, MO, None, None),
        "qfec_locate_wide": lambda: L.qfec_locate_wide(None, D, P, M, 1, 16, 16, C, MO, None, None),
        "qfec_scrub_wide": lambda: L.qfec_scrub_wide(None, D, P, M, 1, 16, 16, C, None, None, None),
        "qfec_check_build_host": lambda: L.qfec_check_build_host(None, None, None),
    }
    for name, call in calls.items():
        assert call() == QFEC_EINVAL
        assert name + ":" in last_error() and "null code" in last_error(), last_error()


def test_check_build_host_refuses_null_buffers():
    L = qa.lib()
    code = qa.Code.cauchy(4, 2)
    mk = np.zeros(6, np.uint8)
    out = np.zeros(code.check_stride(), np.uint8)
    assert L.qfec_check_build_host(code._h, None, out.ctypes.data) == QFEC_EINVAL and "null buffer" in last_error()
    assert L.qfec_check_build_host(code._h, mk.ctypes.data, None) == QFEC_EINVAL and "null buffer" in last_error()


@pytest.mark.parametrize("k,m", [(4, 2), (32, 8), (200, 55), (128, 127)])
def test_nothing_to_do_is_ok_without_a_device(k, m):
    """groups = 0: QFEC_OK with null buffers at any k + m; a bad argument still loses to it."""
    L = qa.lib()
    code = qa.Code.cauchy(k, m)
    for call in empty_calls(code).values():
        assert call() == 0
    assert L.qfec_locate_wide(code._h, None, None, None, 0, 32, 16, None, None, None, None) == QFEC_EINVAL
    assert L.qfec_scrub_wide(code._h, None, None, None, 0, 0, 16, None, None, None, None) == QFEC_EINVAL
    assert L.qfec_check_build(code._h, None, 0, CK + 2, None) == QFEC_EINVAL


def test_python_face_checks_shapes_before_the_call():
    import torch

    code = qa.Code.cauchy(32, 8)
    data = torch.zeros((2, 32, 16), dtype=torch.uint8)
    par = torch.zeros((2, 8, 16), dtype=torch.uint8)
    marks = torch.zeros(2 * 40, dtype=torch.uint8)
    with pytest.raises(qa.QfecError, match="shape mismatch"):
        code.locate_wide(data, par, marks[:-1])
    with pytest.raises(qa.QfecError, match="shape mismatch"):
        code.scrub_wide(data, par[:1], marks)
    with pytest.raises(qa.QfecError, match="check_apply: check_plan"):
        code.check_apply(data, par, torch.zeros((2, 16), dtype=torch.uint8))
    with pytest.raises(qa.QfecError, match="expected a device tensor"):
        code.locate_wide(data, par, marks)
    with pytest.raises(qa.QfecError, match="check_build"):
        code.check_build(marks[:-1])
    with pytest.raises(qa.QfecError, match="check_build: groups"):
        code.check_build()
    with pytest.raises(qa.QfecError, match="check_host"):
        code.check_host(np.zeros(39, np.uint8))
