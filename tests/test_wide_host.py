"""CPU tests of device-built decode plans (qfec_plan_build and friends, include/qfec.h): the plan
arithmetic, which the host query qfec_plan_build_host and the build kernel share as one text, is held
to the existing host queries qfec_repair_rows / qfec_decode_rows over the whole plan buffer; and
every argument the device calls refuse is refused on the host, with its cause in qfec_last_error,
with stand-in pointers that are never dereferenced.  No kernel is launched here."""
import re

import numpy as np
import pytest

import quicknet_amd as qa
from repair_common import masks_up_to
from wide_common import (FAILED, NONE, RECONSTRUCT, REPAIR, WORK, expected_plan, layout, random_masks, singular_code,
                         singular_marks, stale_code, stale_flags, stale_marks, status_of)

QFEC_EINVAL, QFEC_EUNSUP = -1, -5
D, P, M, PL, F = 64, 4096, 8192, 12288, 16384  # stand-ins for device pointers (never dereferenced)


def last_error():
    return qa.lib().qfec_last_error().decode()


def all_masks(n):
    return ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1).astype(np.uint8)


# (flavour, k, m, masks)
SETS = [
    ("cauchy", 4, 2, lambda: all_masks(6)),
    ("vandermonde", 4, 2, lambda: all_masks(6)),
    ("cauchy", 10, 3, lambda: masks_up_to(13, 4)),
    ("cauchy", 32, 8, lambda: random_masks(1, 40, 8, 200)),
    ("cauchy", 60, 8, lambda: random_masks(2, 68, 8, 200)),
    ("cauchy", 20, 12, lambda: random_masks(3, 32, 12, 200)),
    ("cauchy", 200, 55, lambda: random_masks(4, 255, 55, 200)),
    ("cauchy", 128, 127, lambda: random_masks(5, 255, 127, 200)),
    ("cauchy", 254, 1, lambda: random_masks(6, 255, 1, 200)),
    ("cauchy", 1, 254, lambda: random_masks(7, 255, 254, 200)),
    ("vandermonde", 32, 8, lambda: random_masks(8, 40, 8, 200)),
]


@pytest.mark.parametrize("flavour,k,m,masks", SETS, ids=[f"{s[0]}-{s[1]}-{s[2]}" for s in SETS])
def test_host_plan_equals_the_host_queries(flavour, k, m, masks):
    """Both modes, the whole plan buffer: t, e, status, survivors, lost ids, stale flags, rows and
    every padding byte.  The set must hold untouched, repairable and failed groups in both modes."""
    code = getattr(qa.Code, flavour)(k, m)
    quirk = flavour == "cauchy"  # qfec_code_new: rs_stale_quirk is the default for QFEC_CAUCHY
    gm = masks()
    assert code.plan_stride() == layout(k, m)[4]
    for mode in (RECONSTRUCT, REPAIR):
        seen = set()
        for mk in gm:
            plan = code.plan_host(mk, mode)
            want = expected_plan(code, mk, mode, quirk)
            assert np.array_equal(plan, want), (mode, np.nonzero(mk)[0], np.nonzero(plan != want)[0][:8])
            seen.add(int(status_of(plan)))
        assert seen == {NONE, WORK, FAILED}, (mode, seen)


def test_stale_flag_follows_the_quirk():
    """Codes from qfec_code_new are MDS and have no zero decode coefficient, so the stale flag is
    exercised on explicit rows: shard 5 alone lost, parity 0 alive, rows[0][0] = 0."""
    mk = stale_marks()
    for quirk in (1, 0):
        code, rows = stale_code(quirk)
        for mode in (RECONSTRUCT, REPAIR):
            plan = code.plan_host(mk, mode)
            assert np.array_equal(plan, expected_plan(code, mk, mode, quirk))
            assert status_of(plan) == WORK and plan[0] == 1 and plan[2] == 1
            assert list(stale_flags(plan, 30, 4)) == [quirk, 0, 0, 0]
            so, lo, _, co, _ = layout(30, 4)
            assert plan[lo] == 5 and plan[so + 29] == 30  # lost shard 5, decoded from parity row 0
            assert plan[co] == 0  # the column-0 coefficient, rows[0][0] / rows[0][5]


def test_singular_survivor_matrix_fails():
    code, _ = singular_code()
    mk = singular_marks()
    for mode in (RECONSTRUCT, REPAIR):
        plan = code.plan_host(mk, mode)
        assert status_of(plan) == FAILED and plan[0] == 2 and plan[2] == 2
        assert not plan[5:].any()
        assert np.array_equal(plan, expected_plan(code, mk, mode, 0))
    one = np.zeros(28, np.uint8)
    one[3] = 1
    assert status_of(code.plan_host(one, REPAIR)) == WORK  # one lost shard decodes: a 1 x 1 matrix


@pytest.mark.parametrize("k,m", [(4, 2), (32, 8), (60, 8), (200, 55), (128, 127), (254, 1), (1, 254)])
def test_plan_stride_is_the_layout_formula(k, m):
    code = qa.Code.cauchy(k, m)
    stride = qa.lib().qfec_plan_stride(code._h)
    assert stride == layout(k, m)[4] and stride % 16 == 0
    assert stride >= 16 + k + 2 * m + m * k
    assert qa.lib().qfec_plan_stride(None) == QFEC_EINVAL and "null code" in last_error()


# (marks, groups, mode, plan) -> the cause named
BUILD_REFUSED = [
    ((M, -1, 0, PL), "groups < 0"),
    ((M, 1, 2, PL), "mode"),
    ((M, 1, -1, PL), "mode"),
    ((None, 1, 0, PL), "null buffer"),
    ((M, 1, 1, None), "null buffer"),
    ((M, 1, 0, PL + 1), "d_plan not 16-byte aligned"),
    ((M, 1, 1, PL + 4), "d_plan not 16-byte aligned"),
    ((M, 1, 1, PL + 8), "d_plan not 16-byte aligned"),
]


@pytest.mark.parametrize("args,why", BUILD_REFUSED)
def test_plan_build_refuses_on_the_host(args, why):
    L = qa.lib()
    code = qa.Code.cauchy(32, 8)
    assert L.qfec_plan_build(code._h, *args, F, None) == QFEC_EINVAL
    assert "qfec_plan_build:" in last_error() and re.search(why, last_error()), last_error()


# (data, parity, third, groups, block_size, pitch) -> the cause named; third = plan or marks
ROWS_REFUSED = [
    ((D, P, M, -1, 16, 16), "groups < 0"),
    ((D, P, M, 1, 0, 16), "block_size < 1"),
    ((D, P, M, 1, -5, 16), "block_size < 1"),
    ((D, P, M, 1, 32, 16), "pitch < block_size"),
    ((None, P, M, 1, 16, 16), "null buffer"),
    ((D, None, M, 1, 16, 16), "null buffer"),
    ((D, P, None, 1, 16, 16), "null buffer"),
]
# qfec_plan_apply alone: its third buffer is the plan, which must be 16-byte aligned (the one-shots'
# third buffer is the marks, at any alignment)
APPLY_REFUSED = [((D, P, PL + 1, 1, 16, 16), "d_plan not 16-byte aligned"),
                 ((D, P, PL + 4, 1, 16, 16), "d_plan not 16-byte aligned"),
                 ((D + 1, P, PL + 8, 1, 16, 16), "d_plan not 16-byte aligned")]


@pytest.mark.parametrize("args,why", APPLY_REFUSED)
def test_plan_apply_refuses_a_misaligned_plan(args, why):
    L = qa.lib()
    code = qa.Code.cauchy(32, 8)
    assert L.qfec_plan_apply(code._h, *args, None) == QFEC_EINVAL
    assert "qfec_plan_apply:" in last_error() and why in last_error(), last_error()


@pytest.mark.parametrize("args,why", ROWS_REFUSED)
def test_apply_and_one_shots_refuse_on_the_host(args, why):
    L = qa.lib()
    code = qa.Code.cauchy(32, 8)
    assert L.qfec_plan_apply(code._h, *args, None) == QFEC_EINVAL
    assert "qfec_plan_apply:" in last_error() and re.search(why, last_error()), last_error()
    for name in ("qfec_reconstruct_wide", "qfec_repair_wide"):
        assert getattr(L, name)(code._h, *args, F, None) == QFEC_EINVAL
        assert name + ":" in last_error() and re.search(why, last_error()), last_error()


def test_null_code_is_named():
    L = qa.lib()
    calls = {
        "qfec_plan_build": lambda: L.qfec_plan_build(None, M, 1, 0, PL, None, None),
        "qfec_plan_apply": lambda: L.qfec_plan_apply(None, D, P, PL, 1, 16, 16, None),
        "qfec_reconstruct_wide": lambda: L.qfec_reconstruct_wide(None, D, P, M, 1, 16, 16, None, None),
        "qfec_repair_wide": lambda: L.qfec_repair_wide(None, D, P, M, 1, 16, 16, None, None),
        "qfec_plan_build_host": lambda: L.qfec_plan_build_host(None, None, 0, None),
    }
    for name, call in calls.items():
        assert call() == QFEC_EINVAL
        assert name + ":" in last_error() and "null code" in last_error(), last_error()


def test_plan_build_host_refuses():
    L = qa.lib()
    code = qa.Code.cauchy(4, 2)
    mk = np.zeros(6, np.uint8)
    out = np.zeros(code.plan_stride(), np.uint8)
    assert L.qfec_plan_build_host(code._h, mk.ctypes.data, 2, out.ctypes.data) == QFEC_EINVAL
    assert "mode" in last_error()
    assert L.qfec_plan_build_host(code._h, None, 0, out.ctypes.data) == QFEC_EINVAL
    assert "null buffer" in last_error()
    assert L.qfec_plan_build_host(code._h, mk.ctypes.data, 0, None) == QFEC_EINVAL


@pytest.mark.parametrize("k,m", [(4, 2), (32, 8), (200, 55)])
def test_nothing_to_do_is_ok_without_a_device(k, m):
    """groups = 0: QFEC_OK with null buffers at any k + m; a bad argument still loses to it."""
    L = qa.lib()
    code = qa.Code.cauchy(k, m)
    assert L.qfec_plan_build(code._h, None, 0, 1, None, None, None) == 0
    assert L.qfec_plan_apply(code._h, None, None, None, 0, 16, 16, None) == 0
    assert L.qfec_reconstruct_wide(code._h, None, None, None, 0, 16, 16, None, None) == 0
    assert L.qfec_repair_wide(code._h, None, None, None, 0, 16, 16, None, None) == 0
    assert L.qfec_plan_build(code._h, None, 0, 3, None, None, None) == QFEC_EINVAL
    assert L.qfec_repair_wide(code._h, None, None, None, 0, 32, 16, None, None) == QFEC_EINVAL


def test_edited_rs_handle_is_unsupported():
    """A reed_solomon handle whose rs->m is [I; parity] is accepted; one edit of rs->m and every plan
    call answers QFEC_EUNSUP on the host, groups = 0 included; the edit undone, it is accepted again."""
    L = qa.lib()
    rs = qa.ReedSolomon(6, 3)
    mk = np.zeros(9, np.uint8)
    mk[[1, 7]] = 1
    code = rs.code()
    plain = qa.Code.from_rows(code.rows, rs_stale_quirk=True)
    assert np.array_equal(code.plan_host(mk, REPAIR), plain.plan_host(mk, REPAIR))
    rs.m_matrix[7, 2] ^= 0x21
    code = rs.code()
    out = np.zeros(code.plan_stride(), np.uint8)
    assert L.qfec_plan_build_host(code._h, mk.ctypes.data, 1, out.ctypes.data) == QFEC_EUNSUP
    assert "qfec_plan_build_host:" in last_error() and "decode matrix" in last_error()
    assert L.qfec_plan_build(code._h, M, 1, 0, PL, None, None) == QFEC_EUNSUP
    assert L.qfec_plan_build(code._h, None, 0, 0, None, None, None) == QFEC_EUNSUP
    assert L.qfec_plan_apply(code._h, D, P, PL, 1, 16, 16, None) == QFEC_EUNSUP
    assert L.qfec_reconstruct_wide(code._h, D, P, M, 1, 16, 16, None, None) == QFEC_EUNSUP
    assert L.qfec_repair_wide(code._h, D, P, M, 1, 16, 16, None, None) == QFEC_EUNSUP
    assert "qfec_repair_wide:" in last_error()
    rs.m_matrix[7, 2] ^= 0x21
    code = rs.code()
    assert np.array_equal(code.plan_host(mk, REPAIR), plain.plan_host(mk, REPAIR))


def test_python_face_checks_shapes_before_the_call():
    import torch

    code = qa.Code.cauchy(32, 8)
    data = torch.zeros((2, 32, 16), dtype=torch.uint8)
    par = torch.zeros((2, 8, 16), dtype=torch.uint8)
    marks = torch.zeros(2 * 40, dtype=torch.uint8)
    with pytest.raises(qa.QfecError, match="shape mismatch"):
        code.reconstruct_wide(data, par, marks[:-1])
    with pytest.raises(qa.QfecError, match="shape mismatch"):
        code.plan_apply(data, par, torch.zeros((2, 16), dtype=torch.uint8))
    with pytest.raises(qa.QfecError, match="expected a device tensor"):
        code.repair_wide(data, par, marks)
    with pytest.raises(qa.QfecError, match="plan_build"):
        code.plan_build(marks[:-1], REPAIR)
    with pytest.raises(qa.QfecError, match="plan_host"):
        code.plan_host(np.zeros(39, np.uint8), 0)
    assert (qa.QFEC_PLAN_RECONSTRUCT, qa.QFEC_PLAN_REPAIR) == (0, 1)
