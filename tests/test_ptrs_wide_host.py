"""CPU tests of the plan calls on pointer tables (qfec_plan_apply_ptrs, qfec_reconstruct_ptrs_wide,
qfec_repair_ptrs_wide, include/qfec.h): every argument they refuse is refused on the host, with its
cause in qfec_last_error after the call's name, with stand-in pointers that are never dereferenced;
what needs no device needs none; the knob rs_dev_ptrs_wide.  No kernel is launched here."""
import pytest

import quicknet_amd as qa

QFEC_OK, QFEC_EINVAL, QFEC_ENODEV, QFEC_EUNSUP = 0, -1, -2, -5
T, M, PL, F = 4096, 8192, 12288, 16384  # stand-ins for device pointers (never dereferenced)
ONE_SHOTS = ("qfec_reconstruct_ptrs_wide", "qfec_repair_ptrs_wide")


def last_error():
    return qa.lib().qfec_last_error().decode()


# (table, marks or plan, groups, block_size) -> the cause named
COMMON_REFUSED = [
    ((T, M, -1, 16), "groups < 0"),
    ((T, M, 1, 0), "block_size < 1"),
    ((T, M, 1, -7), "block_size < 1"),
    ((None, M, 1, 16), "null d_shards"),
]


@pytest.mark.parametrize("args,why", COMMON_REFUSED + [((T, None, 1, 16), "null d_marks")])
def test_one_shots_refuse_on_the_host(args, why):
    L = qa.lib()
    code = qa.Code.cauchy(32, 8)
    for name in ONE_SHOTS:
        assert getattr(L, name)(code._h, *args, F, None) == QFEC_EINVAL
        assert last_error().startswith(name + ":") and why in last_error(), last_error()


@pytest.mark.parametrize("args,why", COMMON_REFUSED + [
    ((T, None, 1, 16), "null d_plan"),
    ((T, PL + 1, 1, 16), "d_plan not 16-byte aligned"),
    ((T, PL + 4, 1, 16), "d_plan not 16-byte aligned"),
    ((T + 1, PL + 8, 1, 16), "d_plan not 16-byte aligned"),
])
def test_plan_apply_ptrs_refuses_on_the_host(args, why):
    L = qa.lib()
    code = qa.Code.cauchy(32, 8)
    assert L.qfec_plan_apply_ptrs(code._h, *args, None) == QFEC_EINVAL
    assert last_error().startswith("qfec_plan_apply_ptrs:") and why in last_error(), last_error()


def test_null_code_is_named():
    L = qa.lib()
    calls = {
        "qfec_plan_apply_ptrs": lambda: L.qfec_plan_apply_ptrs(None, T, PL, 1, 16, None),
        "qfec_reconstruct_ptrs_wide": lambda: L.qfec_reconstruct_ptrs_wide(None, T, M, 1, 16, None, None),
        "qfec_repair_ptrs_wide": lambda: L.qfec_repair_ptrs_wide(None, T, M, 1, 16, None, None),
    }
    for name, call in calls.items():
        assert call() == QFEC_EINVAL
        assert last_error().startswith(name + ":") and "null code" in last_error(), last_error()


@pytest.mark.parametrize("k,m", [(4, 2), (20, 5), (200, 55)])
def test_nothing_to_do_is_ok_without_a_device(k, m):
    """groups = 0: QFEC_OK with null buffers at any k + m; a bad argument still wins."""
    L = qa.lib()
    code = qa.Code.cauchy(k, m)
    assert L.qfec_plan_apply_ptrs(code._h, None, None, 0, 16, None) == QFEC_OK
    for name in ONE_SHOTS:
        assert getattr(L, name)(code._h, None, None, 0, 16, None, None) == QFEC_OK
        assert getattr(L, name)(code._h, None, None, 0, 0, None, None) == QFEC_EINVAL
        assert "block_size < 1" in last_error()
    assert L.qfec_plan_apply_ptrs(code._h, None, None, 0, 0, None) == QFEC_EINVAL
    assert L.qfec_plan_apply_ptrs(code._h, None, PL + 4, 0, 16, None) == QFEC_EINVAL
    assert "d_plan not 16-byte aligned" in last_error()


def test_a_wide_code_is_accepted():
    """k + m = 25, where qfec_reconstruct_ptrs answers QFEC_EUNSUP: the arguments pass, the code
    passes, and the call gets as far as asking for a device."""
    if qa.device_count() > 0:
        pytest.skip("a GPU is present: the calls would run on the stand-in pointers")
    L = qa.lib()
    code = qa.Code.cauchy(20, 5)
    assert L.qfec_reconstruct_ptrs(code._h, T, M, 1, 16, None, None) == QFEC_EUNSUP
    assert L.qfec_plan_apply_ptrs(code._h, T, PL, 1, 16, None) == QFEC_ENODEV
    for name in ONE_SHOTS:
        assert getattr(L, name)(code._h, T, M, 1, 16, None, None) == QFEC_ENODEV


def test_edited_rs_handle_is_unsupported():
    """One edit of rs->m and the three calls answer QFEC_EUNSUP on the host, groups = 0 included; the
    edit undone, they are accepted again."""
    L = qa.lib()
    rs = qa.ReedSolomon(6, 3)
    rs.m_matrix[7, 2] ^= 0x21
    code = rs.code()
    for groups in (0, 1):
        assert L.qfec_plan_apply_ptrs(code._h, T, PL, groups, 16, None) == QFEC_EUNSUP
        assert last_error().startswith("qfec_plan_apply_ptrs:") and "edited handle" in last_error()
        for name in ONE_SHOTS:
            assert getattr(L, name)(code._h, T, M, groups, 16, None, None) == QFEC_EUNSUP
            assert last_error().startswith(name + ":"), last_error()
    rs.m_matrix[7, 2] ^= 0x21
    code = rs.code()
    assert L.qfec_plan_apply_ptrs(code._h, T, PL, 0, 16, None) == QFEC_OK
    for name in ONE_SHOTS:
        assert getattr(L, name)(code._h, T, M, 0, 16, None, None) == QFEC_OK
    rs.close()


def test_knob_rs_dev_ptrs_wide():
    """Default 0; 1 accepted; -1 and 2 refused and the value kept."""
    assert qa.tune_get("rs_dev_ptrs_wide") == 0
    try:
        qa.tune("rs_dev_ptrs_wide", 1)
        assert qa.tune_get("rs_dev_ptrs_wide") == 1
        for bad in (-1, 2):
            assert qa.lib().qfec_tune(b"rs_dev_ptrs_wide", bad) == QFEC_EINVAL
            assert qa.tune_get("rs_dev_ptrs_wide") == 1
    finally:
        qa.tune("rs_dev_ptrs_wide", 0)
    assert qa.tune_get("rs_dev_ptrs_wide") == 0


class _Fake:
    """What the Python face looks at before it reaches for a device pointer."""

    def __init__(self, n):
        self._n = n
        self.shape = (n,)

    def dim(self):
        return 1

    def numel(self):
        return self._n


def test_python_face_refuses_a_short_table():
    code = qa.Code.cauchy(20, 5)
    for call in (lambda p: code.plan_apply_ptrs(p, _Fake(2 * code.plan_stride()), 16),
                 lambda p: code.reconstruct_ptrs_wide(p, _Fake(50), 16),
                 lambda p: code.repair_ptrs_wide(p, _Fake(50), 16)):
        with pytest.raises(qa.QfecError, match=r"not groups \* \(k \+ m\)"):
            call(_Fake(49))
    with pytest.raises(qa.QfecError, match="marks"):
        code.repair_ptrs_wide(_Fake(50), _Fake(49), 16)
    with pytest.raises(qa.QfecError, match="plan has"):
        code.plan_apply_ptrs(_Fake(50), _Fake(17), 16)
